// sampling_body.inc — the body of sampling.hip's kernel, included into sample_rows_kernel (CONSTRAINED = false),
// sample_rows_constrained_kernel (CONSTRAINED = true), sample_rows_logprobs_kernel (CONSTRAINED and SCORED) and
// sample_rows_masked_kernel (CONSTRAINED, SCORED and MASKED), and into sample_rows_resident_kernel (none of the three, no
// history: total is the constant 0).  The Philox counter is read through SMP_OFFSET_LO / SMP_OFFSET_HI, which the including
// kernel defines: words [6] and [7] of the record, or (resident) those words as a base plus the row's position.  Expects the
// kernels' arguments (bias_ids, bias_values, cu_bias, bias_total included: null and 0 in sample_rows_kernel, where no
// statement that names them is compiled; logprobs, top_ids, top_logprobs, score_k, want likewise where SCORED is false;
// allow_words, n_masks, mask_row likewise where MASKED is false), T, CONSTRAINED, SCORED and MASKED in scope.  A sixth
// inclusion, sample_rows_resident_penalized_kernel, is the resident one with LOGGED true: step 2L builds the row's history
// from a resident token log and the row's id is appended to it (penalty_params, token_log, log_slots, log_cap: null and 0
// where LOGGED is false, and no statement that names them is compiled).
  extern __shared__ __attribute__((aligned(16))) float zs[];      // the row as fp32, n elements (rounded up to 8)
  __shared__ float part_f[2][SMP_WAVES];
  __shared__ int part_i[2][SMP_WAVES];
  __shared__ int s_first, s_last;
  __shared__ int hist[256];                                        // top-k: the counts of one radix pass
  __shared__ int s_digit, s_above;
  const int64_t row = blockIdx.x;
  const u16* p = logits + row * ld;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the row's record (hydra_hip.h): temperature, top_p, top_k, min_p (hx_sample_rows_constrained only), seed, offset
  const uint32_t* rec = sample_params + row * 8;
  const float temperature = __uint_as_float(rec[0]), top_p = __uint_as_float(rec[1]);
  const int32_t top_k = (int32_t)rec[2];
  const float u = (float)(smp_philox0(SMP_OFFSET_LO, SMP_OFFSET_HI, rec[4], rec[5]) >> 8) * 0x1p-24f;
  const bool sampled = temperature > 0.f;                          // (a NaN or a negative temperature: greedy)
  // SCORED: the row's scores are wanted (the same in every thread); a greedy row is then scored as T = 1 over all of it
  // (MASKED: scoring is optional per launch as well — with logprobs null no row is scored and want is not read)
  const bool scored = SCORED && (!MASKED || logprobs != nullptr) && (want == nullptr || want[row] >= 0);
  const float tdiv = SCORED && !sampled ? 1.f : temperature;

  // 1. the row into LDS as fp32: 16-byte loads, four in flight, like argmax_rows_kernel
  const bool gvec = (ld % 8 == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
  if (gvec) {
    const int nvec = n >> 3;
    for (int i0 = tid; i0 < nvec; i0 += 4 * SMP_THREADS) {
      u16x8 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const u16x8*>(p + (int64_t)min(i0 + SMP_THREADS * q, nvec - 1) * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + SMP_THREADS * q;
        if (i < nvec) {
          f32x4 a, b;
#pragma unroll
          for (int e = 0; e < 4; ++e) { a[e] = T::to_float(v[q][e]); b[e] = T::to_float(v[q][4 + e]); }
          *reinterpret_cast<f32x4*>(zs + i * 8) = a;
          *reinterpret_cast<f32x4*>(zs + i * 8 + 4) = b;
        }
      }
    }
    for (int i = nvec * 8 + tid; i < n; i += SMP_THREADS) zs[i] = T::to_float(p[i]);
  } else {
    for (int i = tid; i < n; i += SMP_THREADS) zs[i] = T::to_float(p[i]);
  }
  __syncthreads();

  // 1a. MASKED: every element of a masked row whose bit is clear becomes -inf, ahead of everything that looks at the
  // row.  Byte i of the row's mask (little-endian words: bits 8 i .. 8 i + 7) covers the eight elements a thread holds
  // as two f32x4 of LDS; the mask's (n + 7) / 8 bytes are read from global memory once, nothing of it for a row whose
  // index names no mask.  Bits at or above n fall on the row's padding (rounded up to 8), which nothing reads.
  if (MASKED) {
    const int32_t mr = mask_row[row];
    if (mr >= 0 && mr < n_masks) {                                 // the same in every thread of the workgroup
      const uint8_t* mb = reinterpret_cast<const uint8_t*>(allow_words + (int64_t)mr * ((n + 31) >> 5));
      const int nbytes = (n + 7) >> 3;
      for (int i = tid; i < nbytes; i += SMP_THREADS) {
        const uint32_t bits = mb[i];
        if (bits != 0xffu) {
          f32x4 a = *reinterpret_cast<f32x4*>(zs + i * 8), b = *reinterpret_cast<f32x4*>(zs + i * 8 + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[e] = (bits >> e) & 1u ? a[e] : -INFINITY;
            b[e] = (bits >> (4 + e)) & 1u ? b[e] : -INFINITY;
          }
          *reinterpret_cast<f32x4*>(zs + i * 8) = a;
          *reinterpret_cast<f32x4*>(zs + i * 8 + 4) = b;
        }
      }
      __syncthreads();
    }
  }

  // 1b. the row's slice of the bias table, held inside [0, bias_total] like the history: x + b, one fp32 addition per
  // entry, one entry per thread; the barrier because a token may be in both tables and the penalties start from x + b
  if (CONSTRAINED && bias_total > 0) {
    int32_t b0 = cu_bias[row], b1 = cu_bias[row + 1];
    b0 = min(max(b0, 0), bias_total);
    b1 = min(max(b1, b0), bias_total);
    if (b1 > b0) {                                                 // the same in every thread of the workgroup
      for (int32_t j = b0 + tid; j < b1; j += SMP_THREADS) {
        const int32_t t = bias_ids[j];
        if (t >= 0 && t < n) zs[t] = zs[t] + bias_values[j];        // (ids pairwise distinct)
      }
      __syncthreads();
    }
  }

  // 2. the row's slice of the history, held inside [0, total] whatever cu_hist says: its entries in place, one per thread
  if (total > 0) {
    int32_t h0 = cu_hist[row], h1 = cu_hist[row + 1];
    h0 = min(max(h0, 0), total);
    h1 = min(max(h1, h0), total);
    if (h1 > h0) {                                                 // the same in every thread of the workgroup
      const float f = penalties[row * 3], pp = penalties[row * 3 + 1], r = penalties[row * 3 + 2];
      for (int32_t j = h0 + tid; j < h1; j += SMP_THREADS) {
        const int32_t t = hist_ids[j];
        if (t >= 0 && t < n) zs[t] = penalized_value(zs[t], hist_counts[j], f, pp, r);   // (ids pairwise distinct)
      }
      __syncthreads();
    }
  }

  // 2L. LOGGED: the row's history is the first L' = clamp(L, 0, log_cap) words of its slot of the resident token log, L
  // the row's offset (the request's generated-token count); the row's id goes to word L once it is known (log_at).  The
  // log holds tokens WITH repeats and penalized_value wants each distinct token's count once, in one rounding: the
  // row's own word zs[t] serves as the integer counter of token t.  Every log entry keeps its (t, x = zs[t]) in
  // registers, zs[t] becomes 0, every entry adds 1 to it (integer LDS atomics: no order of arrival shows), every entry
  // reads the count back, and every entry of t writes the SAME penalized_value(x, count) — no LDS beyond the row's,
  // five barriers, L' / 1024 entries a thread.  An entry outside [0, n) takes no part.
  int32_t* log_at = nullptr;
  if (LOGGED) {
    const int32_t ls = penalty_params[row * 4 + 3];
    if (ls >= 0 && ls < log_slots) {                               // the same in every thread of the workgroup
      const int64_t L = (int64_t)(((uint64_t)(SMP_OFFSET_HI) << 32) | (uint64_t)(SMP_OFFSET_LO));
      int32_t* lrow = token_log + (int64_t)ls * log_cap;
      const int32_t len = (int32_t)(L < 0 ? 0 : L > log_cap ? log_cap : L);
      if (L >= 0 && L < log_cap) log_at = lrow + L;
      if (len > 0) {
        const float f = __int_as_float(penalty_params[row * 4]), pp = __int_as_float(penalty_params[row * 4 + 1]),
                    r = __int_as_float(penalty_params[row * 4 + 2]);
        int32_t lt[SMP_LOG_PER_THREAD];
        float lx[SMP_LOG_PER_THREAD];
#pragma unroll
        for (int q = 0; q < SMP_LOG_PER_THREAD; ++q) {
          const int j = tid + q * SMP_THREADS;
          const int32_t t = j < len ? lrow[j] : -1;
          lt[q] = t >= 0 && t < n ? t : -1;
          lx[q] = lt[q] >= 0 ? zs[lt[q]] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SMP_LOG_PER_THREAD; ++q)
          if (lt[q] >= 0) zs[lt[q]] = __int_as_float(0);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SMP_LOG_PER_THREAD; ++q)
          if (lt[q] >= 0) atomicAdd(reinterpret_cast<int*>(zs + lt[q]), 1);
        __syncthreads();
        int32_t lc[SMP_LOG_PER_THREAD];
#pragma unroll
        for (int q = 0; q < SMP_LOG_PER_THREAD; ++q) lc[q] = lt[q] >= 0 ? __float_as_int(zs[lt[q]]) : 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SMP_LOG_PER_THREAD; ++q)
          if (lt[q] >= 0) zs[lt[q]] = penalized_value(lx[q], lc[q], f, pp, r);
        __syncthreads();
      }
    }
  }

  // 3. this thread's elements into registers (NaN where it owns none: every comparison below is false for them), and
  // the greedy id
  const int chunk = ((n + SMP_THREADS - 1) / SMP_THREADS) | 1;
  const int base = tid * chunk;
  float zr[SMP_CHUNK];
  float best = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < SMP_CHUNK; ++j) {
    const bool own = j < chunk && base + j < n;
    zr[j] = own ? zs[own ? base + j : 0] : __builtin_nanf("");
    if (own && arg_better(zr[j], base + j, best, bi)) { best = zr[j]; bi = base + j; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (arg_better(ov, oi, best, bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) { part_f[0][wave] = best; part_i[0][wave] = bi; }
  if (tid == 0) { s_first = SMP_THREADS; s_last = -1; }
  __syncthreads();
  best = part_f[0][0];
  bi = part_i[0][0];
#pragma unroll
  for (int k = 1; k < SMP_WAVES; ++k)
    if (arg_better(part_f[0][k], part_i[0][k], best, bi)) { best = part_f[0][k]; bi = part_i[0][k]; }

  // z = s / T, one correctly rounded division; s -> s / T keeps the order, so the largest z is that of the greedy id
  const float m = best / tdiv;
  if (SCORED) {                                                    // no scores: the fill values, and on as without them
    const bool degenerate = best != best || !(fabsf(m) < INFINITY);
    if ((!scored || degenerate) && (!MASKED || logprobs != nullptr)) {   // (MASKED without scores: nothing to fill)
      if (tid == 0) logprobs[row] = __builtin_nanf("");
      if (tid < score_k) {
        top_ids[row * score_k + tid] = -1;
        top_logprobs[row * score_k + tid] = __builtin_nanf("");
      }
    }
  }
  if (!sampled || best != best || !(fabsf(m) < INFINITY)) {        // greedy, or degenerate: a NaN, all -inf, a +inf
    if (tid == 0) {
      ids[row] = bi;
      if (LOGGED && log_at) *log_at = bi;
      if (cut_out) cut_out[row] = __builtin_nanf("");
      if (u_out) u_out[row] = u;
    }
    // (a scored greedy row that is not degenerate goes on: its Z_S is step 6's sum)
    if (!SCORED || !scored || best != best || !(fabsf(m) < INFINITY)) return;
  }
  float er[SMP_CHUNK];
  float zmin = INFINITY;
#pragma unroll
  for (int j = 0; j < SMP_CHUNK; ++j) {
    zr[j] = zr[j] / tdiv;
    er[j] = zr[j] == zr[j] ? expf(zr[j] - m) : 0.f;
    zmin = fminf(zmin, zr[j]);                                     // (fminf passes over the NaN of an element not owned)
  }
  zmin = -wave_max(-zmin);
  if (lane == 0) part_f[1][wave] = zmin;
  __syncthreads();
  zmin = part_f[1][0];
#pragma unroll
  for (int k = 1; k < SMP_WAVES; ++k) zmin = fminf(zmin, part_f[1][k]);
  int round = 1;                                                   // alternates the reductions' LDS; [1] was the last in use

  // 4. top-k: the K-th largest key by a radix select, most significant byte first.  A pass counts, in 256 LDS bins, the
  // next byte of every key that matches the bytes chosen so far; wave 0 takes the suffix sums of the bins and picks the
  // highest byte with at least K keys at or above it (`above`: the keys above everything that matches).  The last pass
  // leaves a key of the row.  Integer atomics: the counts do not depend on the order of the additions.
  const uint32_t khi = smp_key(m);
  uint32_t kcut = smp_key(zmin);
  if (top_k > 0 && top_k < n && (!SCORED || sampled)) {            // (a greedy row ignores the truncation fields)
    uint32_t prefix = 0u;
    int above = 0;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < SMP_CHUNK; ++j) {
        if (zr[j] == zr[j]) {
          const uint32_t key = smp_key(zr[j]);
          if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
      }
      __syncthreads();
      if (wave == 0) {
        const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
        const int mine4 = c0 + c1 + c2 + c3;
        int s = mine4;                                             // suffix sum over the lanes at and above this one
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int o = __shfl_down(s, off, 64);
          if (lane + off < 64) s += o;
        }
        const int suf3 = above + s - mine4 + c3, suf2 = suf3 + c2, suf1 = suf2 + c1, suf0 = suf1 + c0;
        const unsigned long long ok = __ballot(suf0 >= top_k);
        const int top_lane = 63 - __builtin_clzll(ok);
        if (lane == top_lane) {
          const int k = suf3 >= top_k ? 3 : suf2 >= top_k ? 2 : suf1 >= top_k ? 1 : 0;
          s_digit = 4 * lane + k;
          s_above = (k == 3 ? suf3 - c3 : k == 2 ? suf2 - c2 : k == 1 ? suf1 - c1 : suf0 - c0);
        }
      }
      __syncthreads();
      prefix |= (uint32_t)s_digit << shift;
      above = s_above;
    }
    kcut = prefix;
  }

  // 4b. min_p: v_M = the smallest z with e >= min_p (the maximum has e = 1: a min_p above 1 acts as 1), one more block
  // minimum over the registers; the cut so far rises to it
  if (CONSTRAINED) {
    const float min_p = __uint_as_float(rec[3]);
    if (min_p > 0.f && (!SCORED || sampled)) {                     // (a NaN: off)
      float vm = INFINITY;
#pragma unroll
      for (int j = 0; j < SMP_CHUNK; ++j) vm = er[j] >= min_p ? fminf(vm, zr[j]) : vm;
      vm = -wave_max(-vm);
      float* pm = part_f[round ^= 1];
      if (lane == 0) pm[wave] = vm;
      __syncthreads();
      vm = pm[0];
#pragma unroll
      for (int k = 1; k < SMP_WAVES; ++k) vm = fminf(vm, pm[k]);
      kcut = min(max(kcut, smp_key(vm)), khi);
    }
  }

  // 5. top-p: the smallest key at or above v_K with A(v) = sum of e over {z > v} at most top_p * Z_K.  A only changes at
  // values of the row, so that key is one
  if (top_p < 1.f && (!SCORED || sampled)) {
    const float vk = smp_val(kcut);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < SMP_CHUNK; ++j) s += zr[j] >= vk ? er[j] : 0.f;
    const float tau = top_p * smp_block_sum(s, part_f[round ^= 1]);
    uint32_t lo = kcut, hi = khi;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      const float v = smp_val(mid);
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < SMP_CHUNK; ++j) a += zr[j] > v ? er[j] : 0.f;
      a = smp_block_sum(a, part_f[round ^= 1]);
      if (a <= tau) hi = mid; else lo = mid + 1u;
    }
    kcut = lo;
  }
  const float cut = smp_val(kcut);

  // 6. the draw: the first element of S = {z >= cut}, in index order, whose inclusive running sum of e exceeds u * Z_S
  float mine = 0.f;
  bool any = false;
#pragma unroll
  for (int j = 0; j < SMP_CHUNK; ++j) {
    const bool in = zr[j] >= cut;
    mine += in ? er[j] : 0.f;
    any |= in;
  }
  float incl = mine;                                               // inclusive scan over the wave's threads
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  float excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 0.f;
  float* wsum = part_f[round ^= 1];
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  float before = 0.f, zsum = 0.f;                                  // the waves before this one; all of them
#pragma unroll
  for (int k = 0; k < SMP_WAVES; ++k) {
    if (k == wave) before = zsum;
    zsum += wsum[k];
  }
  const float target = u * zsum;
  if (any) {
    if (before + incl > target) atomicMin(&s_first, tid);
    atomicMax(&s_last, tid);
  }
  __syncthreads();
  const int walker = s_first < SMP_THREADS ? s_first : s_last;      // rounding left no crossing: the last element of S
  if (tid == walker && (!SCORED || sampled)) {
    float run = before + excl;
    int pick = -1, last = 0;
    float zpick = 0.f, zlast = 0.f;                                // (SCORED: z of the pick, without indexing the registers)
#pragma unroll
    for (int j = 0; j < SMP_CHUNK; ++j) {
      if (zr[j] >= cut) {
        run += er[j];
        last = j;
        if (SCORED) zlast = zr[j];
        if (pick < 0 && run > target) {
          pick = j;
          if (SCORED) zpick = zr[j];
        }
      }
    }
    ids[row] = base + (pick < 0 ? last : pick);
    if (LOGGED && log_at) *log_at = base + (pick < 0 ? last : pick);
    if (cut_out) cut_out[row] = cut;
    if (u_out) u_out[row] = u;
    if (SCORED && scored) logprobs[row] = ((pick < 0 ? zlast : zpick) - m) - logf(zsum);
  }

  // 7. SCORED: lp_i = (z_i - m) - logf(Z_S) inside S, -inf outside, Z_S the sum the draw was made against (a greedy row:
  // S is the whole row, and its id has z = m).  The K alternatives are the first K elements in arg_better's order (the
  // row has no NaN here), named whether kept or not.  e is dead by now: z stays in the registers as its key (0, which no
  // value has, for an element not owned), every thread holds the best of its keys, and a round is one block argmax over
  // (key, then lower index).  The thread that owned a round's pick zeroes that key and looks through its registers
  // again — within a thread the first of equal keys has the lower index — and only ITS wave redoes the wave's argmax:
  // every other thread's and wave's candidate still stands.
  if (SCORED) {
    if (!scored) return;
    const float logz = logf(zsum);
    if (!sampled && tid == 0) logprobs[row] = -logz;
    uint32_t kr[SMP_CHUNK];
#pragma unroll
    for (int j = 0; j < SMP_CHUNK; ++j) {                          // (a number's key lies in [-inf's, +inf's], a NaN's outside)
      const uint32_t key = smp_key(zr[j]);
      kr[j] = key - 0x007fffffu <= 0xff800000u - 0x007fffffu ? key : 0u;
    }
    uint32_t ck = 0u, wk = 0u;                                     // this thread's candidate; its wave's
    int ci = 0x7fffffff, wi = 0x7fffffff, pi = -1;                 // (pi: the previous pick; 0x7fffffff: nothing is left)
    for (int r = 0; r < score_k; ++r) {
      if (r == 0 || __ballot(ci == pi) != 0ull) {                  // the same in every thread of the wave
        if (r == 0 || ci == pi) {
          ck = 0u;
          ci = 0x7fffffff;
#pragma unroll
          for (int j = 0; j < SMP_CHUNK; ++j) {
            if (base + j == pi) kr[j] = 0u;
            if (kr[j] > ck) { ck = kr[j]; ci = base + j; }
          }
        }
        wk = ck;
        wi = ci;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const uint32_t ok = __shfl_xor(wk, off, 64);
          const int oi = __shfl_xor(wi, off, 64);
          if (ok > wk || (ok == wk && oi < wi)) { wk = ok; wi = oi; }
        }
      }
      round ^= 1;
      if (lane == 0) { part_f[round][wave] = __uint_as_float(wk); part_i[round][wave] = wi; }
      __syncthreads();
      uint32_t bk = __float_as_uint(part_f[round][lane & (SMP_WAVES - 1)]);   // a tree over the sixteen, as smp_block_sum's
      int bj = part_i[round][lane & (SMP_WAVES - 1)];
#pragma unroll
      for (int off = SMP_WAVES / 2; off > 0; off >>= 1) {
        const uint32_t ok = __shfl_xor(bk, off, 64);
        const int oi = __shfl_xor(bj, off, 64);
        if (ok > bk || (ok == bk && oi < bj)) { bk = ok; bj = oi; }
      }
      if (tid == 0) {
        const float bz = smp_val(bk);
        top_ids[row * score_k + r] = bj == 0x7fffffff ? -1 : bj;
        top_logprobs[row * score_k + r] = bj != 0x7fffffff && bz >= cut ? (bz - m) - logz : -INFINITY;
      }
      pi = bj;
    }
  }
