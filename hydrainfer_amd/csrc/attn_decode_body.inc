// attn_decode_body.inc — the body of attn_decode.hip's decode kernel, included into attn_decode_kernel and
// attn_decode_alibi_kernel (see there).  Expects the kernel's arguments and T, D, NW, NT, FUSE, RANKED, ALIBI in scope.
  // Leading scalars (16 dwords) = what the head of the dependent chain  kernarg -> cu_* -> page ids -> first K / V tile
  // needs; they arrive in SGPRs WITH the wave (gemm_xreg.hip, KERNARG PRELOADING).  h_meta = group | n_splits << 8 |
  // (block_shift & 0xff) << 16.  Round 5: the prologue used to be three scalar round trips in a row (the struct, then
  // cu_k, then cu_block_lens + the rest of the struct) with two runtime integer divisions between them; now ONE batch of
  // scalar loads through the preloaded pointers, shifts instead of divisions where the page size is a power of two.
  AttnParams p = p_in;
  p.k = h_k; p.v = h_v; p.cu_k = h_cu_k; p.cu_q = h_cu_q; p.block_table = h_block_table;
  p.cu_block_lens = h_cu_block_lens; p.block_size = h_block_size;
  p.group = h_meta & 0xff; p.n_splits = (h_meta >> 8) & 0xff; p.block_shift = (int)(int8_t)((h_meta >> 16) & 0xff);
  constexpr int OE = D / 16;  // fp32 partial-output elements per lane
  constexpr int NP = NW * 4;  // partial softmax states per workgroup
  __shared__ float s_m[NP], s_l[NP];
  __shared__ float s_o[NP][D];
  __shared__ __attribute__((aligned(16))) char s_k[NW][KLds<D>::BYTES];
  __shared__ __attribute__((aligned(16))) u16 s_qkv[FUSE ? 3 : 1][FUSE ? D : 8];

  int h = blockIdx.x, b = blockIdx.y;      // (RANKED: a flat grid — both are worked out below)
  const int split = blockIdx.z;
#if HX_EXPERIMENTS
  // in-kernel time stamps (100 MHz), 16 per workgroup, wave 0 only: tools/decode_timeline.py
  auto STAMP = [&](int k) {
    if (p_in.stamps && threadIdx.x == 0)
      p_in.stamps[((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 16 + k] = __builtin_amdgcn_s_memrealtime();
  };
#else
  auto STAMP = [&](int) {};
#endif
  STAMP(0);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  constexpr int KPL = TileGeom<D>::KPL, TK = TileGeom<D>::TK, SH = TileGeom<D>::SH;
  int32_t kv_len, cbl, q_row;
  if (RANKED) {
    // Grid (heads, sequences) like the static form; workgroup number q = blockIdx.y * n_heads + blockIdx.x runs on CU
    // q mod n_cus in the dispatcher's round R = q / n_cus.  The descriptor's flag travels with the metadata of the
    // sequence the STATIC numbering would give this workgroup: an even batch (flag 0) has lost nothing; a ragged one
    // takes item k of the length-ranked list in snake order and fetches that sequence's metadata in a second round.
    int32_t ck0 = h_cu_k[b], ck1 = h_cu_k[b + 1];
    cbl = h_cu_block_lens[b];
    q_row = h_cu_q[b];
    if (h_rank_desc[0]) {
      const uint32_t n_heads = gridDim.x, q = blockIdx.y * n_heads + blockIdx.x, n_items = n_heads * gridDim.y;
      const uint32_t nc = (uint32_t)p_in.n_cus, R = q / nc, cq = q - R * nc, in_round = min(nc, n_items - R * nc);
      const uint32_t k = R * nc + ((R & 1u) ? in_round - 1u - cq : cq);
      const uint32_t rho = k / n_heads;
      h = (int)(k - rho * n_heads);
      b = h_rank_desc[1 + rho];
      ck0 = h_cu_k[b];
      ck1 = h_cu_k[b + 1];
      cbl = h_cu_block_lens[b];
      q_row = h_cu_q[b];
    }
    kv_len = ck1 - ck0;
#if HX_EXPERIMENTS
    if (p_in.stamps && threadIdx.x == 0)      // who this workgroup is: tools/ragged_timeline.py
      p_in.stamps[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16 + 8] = 1ull << 40 | (unsigned long long)b << 16 | (unsigned long long)h;
#endif
  } else {
    // the sequence's metadata: one batch of scalar loads
    const int32_t ck0 = h_cu_k[b], ck1 = h_cu_k[b + 1];
    cbl = h_cu_block_lens[b];
    q_row = h_cu_q[b];
    kv_len = ck1 - ck0;
  }
  float slope_l2 = 0.f;      // ALIBI: this (sequence, head)'s slope, one scalar load with the metadata above
  if constexpr (ALIBI) slope_l2 = alibi_slope_log2(p_in, b, h);
  const int hk = p.group == 1 ? h : h / p.group;
  const int n_tiles = (kv_len + TK - 1) >> SH;
  const int per_split = p.n_splits == 1 ? n_tiles : (n_tiles + p.n_splits - 1) / p.n_splits;
  const int t_begin = split * per_split;
  const int t_end = min(n_tiles, t_begin + per_split);
  const int tpp = p.block_size >> SH;  // tiles per page
  const int tsh = p.block_shift - SH;  // >= 0: a page is 2^tsh tiles (no runtime division on the way to the first load)
  auto page_of = [&](int t) { return tsh >= 0 ? t >> tsh : t / tpp; };
  auto row0_of = [&](int t) { return (tsh >= 0 ? t & ((1 << tsh) - 1) : t % tpp) << SH; };
  const int32_t* bt = h_block_table + cbl;

  const u16* kbase = reinterpret_cast<const u16*>(p.k) + (int64_t)hk * p.k_head_stride;
  const u16* vbase = reinterpret_cast<const u16*>(p.v) + (int64_t)hk * p.v_head_stride;

  // ORDER OF THE FIRST REQUESTS (round 5; in-kernel stamps, tools/decode_timeline.py).  A wave's loads return in the
  // order they were issued.  Rounds 1-4 requested the first K / V tile BEFORE the fused prologue's own small loads (qkv
  // slab, cos / sin): 4096 waves x 8 KiB = 33 MB of HBM traffic stood in front of a few L2 hits in every wave, the
  // prologue ended 11 us (median; up to 44 us) after the kernel's start, and until then every wave had ONE tile in
  // flight — HBM idled.  Now: page ids first, then the prologue's loads, then the first tile; the prologue's arithmetic
  // runs under the tile's latency.
  KVTile<D> bufA, bufB;
  int my_page = 0, n_my = 0;
  int chunk0 = t_begin + w;
  auto request_pages = [&]() {
    const int tj = chunk0 + NW * lane;
    my_page = (tj < t_end) ? bt[page_of(tj)] : 0;
    n_my = max(0, min(64, (t_end - chunk0 + NW - 1) / NW));  // wave-uniform
  };
  // (UNCONDITIONAL in the prologue — under a branch the compiler's wait-count model merges the two paths and makes the
  // prologue wait for the tile it has just requested — but a wave without a tile (a sequence shorter than 16 w keys, a
  // late split) touches no memory: its buffer resource has zero records, as in the main loop.  Round-5 ADVICE: it used to
  // read rows of physical block 0, i.e. relied on block 0 of whatever view the caller passed being mapped.)
  auto request_first_tile = [&]() {
    load_tile_b<T, D, NT>(bufA, p, kbase, vbase, __builtin_amdgcn_readlane(my_page, 0), row0_of(chunk0),
                          kv_len - (chunk0 << SH), lane, chunk0 < t_end);
  };
  auto begin_chunk = [&]() { request_pages(); request_first_tile(); };
  // (D = 256 with the fused prologue: the prologue's q / new-key fragments and the first tile together do not fit the
  // 256-register budget — the tile is requested behind the prologue instead of spilling)
  constexpr bool EARLY = !(FUSE && D == 256);
  STAMP(1);      // scalar metadata in
  if (EARLY) request_pages();

  // q as the MFMA B operand, identical in all 16 columns
  u16x8 qf[D / 32];
  if (!(FUSE && p.qkv_partial)) {
    const u16* qp = reinterpret_cast<const u16*>(p.q) + (int64_t)q_row * p.q_row_stride +
                    (int64_t)h * D + 8 * g;
#pragma unroll
    for (int s = 0; s < D / 32; ++s) qf[s] = *reinterpret_cast<const u16x8*>(qp + 32 * s);
  }
  if (!FUSE) {
    if (EARLY) request_first_tile();
    STAMP(2);
  }

  // FUSE: q and the new token's k arrive un-rotated and the cache does not hold the new token
  // yet.  Rotate both in registers (T arithmetic, same rounding as apply_rotary_pos_emb), use
  // k/v of the new token from registers in its tile, and append them to the cache once.
  u16x8 kn[D / 32];                              // rotated new key, fragment layout (RoPE is lane-local there)
  typename VRow<D>::type knr[VRow<D>::NV];       // the same row in the row layout of KVTile
  typename VRow<D>::type vn[VRow<D>::NV];
  const int t_new = (kv_len - 1) >> SH, r_new = (kv_len - 1) & (TK - 1);
  if (FUSE) {
    // cos / sin of the new token's position: requested FIRST (round 5), so that the position's scalar load and the two
    // vector loads behind it run under the slab reduction and its barrier instead of after them
    const u16* cs = reinterpret_cast<const u16*>(p.cos_sin) + (int64_t)p.positions[b] * D;
    u16x8 rc[D / 64], rs[D / 64];
#pragma unroll
    for (int s = 0; s < D / 64; ++s) {
      rc[s] = *reinterpret_cast<const u16x8*>(cs + 32 * s + 8 * g);
      rs[s] = *reinterpret_cast<const u16x8*>(cs + D / 2 + 32 * s + 8 * g);
    }
    if (p.qkv_partial) {
      // q, k, v of this token/head straight from the qkv GEMM's split-K slabs: thread d < D adds
      // the splits of column d in order and rounds once to T (the projection's output
      // rounding); the three rows are shared through LDS so every slab element is read once
      // per workgroup.  Every thread issues the loads (threads >= D the addresses of thread d - D: no divergent
      // branch around them, so the first tile's request below is not fenced off by a full wait).
      const float* row = p.qkv_partial + (int64_t)b * p.qkv_row;
      const int64_t col0[3] = {(int64_t)h * D, (int64_t)p.n_heads * D + (int64_t)hk * D,
                               (int64_t)p.n_heads * D + (int64_t)(p.n_heads / p.group) * D + (int64_t)hk * D};
      const int dcol = threadIdx.x & (D - 1);
      float sacc[3];
#pragma unroll
      for (int which = 0; which < 3; ++which) sacc[which] = row[col0[which] + dcol];
      if (p.qkv_splits > 1) {
#pragma unroll
        for (int which = 0; which < 3; ++which) {
          const float* src = row + col0[which] + dcol;
          for (int s = 1; s < p.qkv_splits; ++s) sacc[which] += src[s * p.qkv_slab_stride];
        }
      }
      if (EARLY) request_first_tile();      // behind the prologue's loads, in front of their use
      STAMP(2);      // page ids in, first tile requested
      if (threadIdx.x < D) {
#pragma unroll
        for (int which = 0; which < 3; ++which) s_qkv[which][threadIdx.x] = T::from_float(sacc[which]);
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < D / 32; ++s) {
        qf[s] = *reinterpret_cast<const u16x8*>(&s_qkv[0][32 * s + 8 * g]);
        kn[s] = *reinterpret_cast<const u16x8*>(&s_qkv[1][32 * s + 8 * g]);
      }
#pragma unroll
      for (int n = 0; n < VRow<D>::NV; ++n)
        vn[n] = *reinterpret_cast<const typename VRow<D>::type*>(&s_qkv[2][128 * n + VRow<D>::E * c]);
    } else {
    const u16* kp = reinterpret_cast<const u16*>(p.k_new) + (int64_t)b * p.kn_row_stride +
                    (int64_t)hk * D + 8 * g;
#pragma unroll
    for (int s = 0; s < D / 32; ++s) kn[s] = *reinterpret_cast<const u16x8*>(kp + 32 * s);
    const u16* vp = reinterpret_cast<const u16*>(p.v_new) + (int64_t)b * p.vn_row_stride +
                    (int64_t)hk * D + VRow<D>::E * c;
#pragma unroll
    for (int n = 0; n < VRow<D>::NV; ++n)
      vn[n] = *reinterpret_cast<const typename VRow<D>::type*>(vp + 128 * n);
    if (EARLY) request_first_tile();
    STAMP(2);
    }
    rope_frags<T, D>(qf, rc, rs);
    rope_frags<T, D>(kn, rc, rs);
    // fragment layout -> row layout through one row of this wave's LDS region
    if (c == 0) {
#pragma unroll
      for (int s = 0; s < D / 32; ++s) *reinterpret_cast<u16x8*>(s_k[w] + 64 * s + 16 * g) = kn[s];
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int n = 0; n < VRow<D>::NV; ++n)
      knr[n] = *reinterpret_cast<const typename VRow<D>::type*>(s_k[w] + 256 * n + 2 * VRow<D>::E * c);
    __builtin_amdgcn_wave_barrier();
    // one writer per kv head and per split set: the first q head of the group, split 0, wave 0
    if (h == hk * p.group && split == 0 && w == 0) {
      const int slot = p.new_slots[b];
      const int64_t blk = slot / p.block_size, off = slot % p.block_size;
      if (c == 0) {   // lanes (r=0, g): 4 x 16 B per step cover the 2*D-byte key row
        u16* kd = const_cast<u16*>(kbase) + blk * p.k_block_stride + off * p.k_row_stride + 8 * g;
#pragma unroll
        for (int s = 0; s < D / 32; ++s) *reinterpret_cast<u16x8*>(kd + 32 * s) = kn[s];
      }
      if (g == 0) {   // lanes (g=0, c): D/16 elements each cover the value row
        u16* vd = const_cast<u16*>(vbase) + blk * p.v_block_stride + off * p.v_row_stride + VRow<D>::E * c;
#pragma unroll
        for (int n = 0; n < VRow<D>::NV; ++n)
          *reinterpret_cast<typename VRow<D>::type*>(vd + 128 * n) = vn[n];
      }
    }
  }
  auto patch = [&](KVTile<D>& buf, int t) {
    // The new token's row AND the rows behind it: load_tile_b clamps rows past the last key to the last valid row, which
    // here is the slot this launch appends to — the cache may still hold what the allocator left there (NaN bit patterns
    // included), and a masked row's p = 0 times a NaN value is NaN.  With the new token in those rows the tile is what
    // the unfused sequence (append, then attend) loads: same bits.
    if (FUSE && t == t_new) {     // wave-uniform
#pragma unroll
      for (int i = 0; i < KPL; ++i)
        if (KPL * g + i >= r_new) {
#pragma unroll
          for (int n = 0; n < VRow<D>::NV; ++n) {
            buf.k[i][n] = knr[n];
            buf.v[i][n] = vn[n];
          }
        }
    }
  };

  STAMP(3);      // prologue done (q / new key rotated, appended)
  float m = HX_NEG_BIG, l = 0.f;
  float o[OE];
#pragma unroll
  for (int e = 0; e < OE; ++e) o[e] = 0.f;

  // my tiles: t_begin + w + NW*j.  Chunks of 64 tiles per wave share one page-id vector.  The loop body is branch-free
  // around its loads: tile j + 1 is ALWAYS requested before tile j is computed (out of range: a buffer load with zero
  // records), tile j + 2 before tile j + 1 is computed — two tiles per wave in flight, exact wait counts.
  auto issue = [&](KVTile<D>& buf, int jj) {
    const int t = chunk0 + NW * jj;
    load_tile_b<T, D, NT>(buf, p, kbase, vbase, __builtin_amdgcn_readlane(my_page, min(jj, 63)), row0_of(t),
                          kv_len - (t << SH), lane, jj < n_my);
  };
  auto run_chunk = [&](bool stamp) {
    for (int j = 0; j < n_my; j += 2) {
      issue(bufB, j + 1);
      patch(bufA, chunk0 + NW * j);
      compute_tile<T, D, ALIBI>(bufA, qf, kv_len - ((chunk0 + NW * j) << SH), p.scale_log2, lane, m, l, o, s_k[w], slope_l2);
      if (stamp && j == 0) STAMP(4);      // first tile computed
      issue(bufA, j + 2);
      if (j + 1 < n_my) {
        patch(bufB, chunk0 + NW * (j + 1));
        compute_tile<T, D, ALIBI>(bufB, qf, kv_len - ((chunk0 + NW * (j + 1)) << SH), p.scale_log2, lane, m, l, o, s_k[w], slope_l2);
      }
    }
  };
  if (!EARLY) begin_chunk();
  run_chunk(true);
  for (chunk0 += NW * 64; chunk0 < t_end; chunk0 += NW * 64) {      // contexts past 64 tiles per wave (4096 keys at NW = 4)
    begin_chunk();
    run_chunk(false);
  }
  STAMP(5);      // last tile computed
  // ---- merge the 16 partial states of this workgroup --------------------------------
  constexpr int E = VRow<D>::E, NV = VRow<D>::NV;
  const int slot = w * 4 + g;
  if (c == 0) {
    s_m[slot] = m;
    s_l[slot] = l;
  }
#pragma unroll
  for (int n = 0; n < NV; ++n)
#pragma unroll
    for (int e = 0; e < E; ++e) s_o[slot][128 * n + E * c + e] = o[n * E + e];
  __syncthreads();

  STAMP(6);      // merge barrier passed
  const int d = threadIdx.x;
  if (d < D) {
    float M = HX_NEG_BIG;
#pragma unroll
    for (int k = 0; k < NP; ++k) M = fmaxf(M, s_m[k]);
    float L = 0.f, O = 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const float wgt = fast_exp2(s_m[k] - M);
      L = fmaf(s_l[k], wgt, L);
      O = fmaf(s_o[k][d], wgt, O);
    }
    if (p.n_splits == 1) {
      const float r = (L > 0.f) ? O / L : 0.f;
      reinterpret_cast<u16*>(p.out)[(int64_t)q_row * p.o_row_stride + (int64_t)h * D + d] =
          T::from_float(r);
    } else {
      const int64_t idx = ((int64_t)b * p.n_heads + h) * p.n_splits + split;
      p.ws_o[idx * D + d] = O;
      if (d == 0) {
        p.ws_ml[idx * 2 + 0] = M;
        p.ws_ml[idx * 2 + 1] = L;
      }
    }
  }
  STAMP(7);
