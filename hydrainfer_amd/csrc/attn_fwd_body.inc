// attn_fwd_body.inc — the body of attn_fwd.hip's general kernel, included into attn_fwd_kernel and attn_fwd_alibi_kernel
// (see there).  Expects `p` and T, D, PAGED, QR, KU, ALIBI in scope.
  constexpr int NS = D / 32;       // QK k-steps
  constexpr int NDB = D / 16;      // 16-dim output blocks
  constexpr int RS = 2 * D + 32;   // LDS row stride in bytes (K and V images)
  constexpr int LPR = D / 8;       // 16-byte chunks per key row
  constexpr int KT = 32 * KU;      // keys per tile (KU = 2: half the barriers and softmax passes, and
                                   // four independent score sub-tiles per wave to hide MFMA / exp latency)
  constexpr int TILE_CHUNKS = KT * LPR;
  constexpr int NL = (TILE_CHUNKS + 255) / 256;   // chunks per thread per tile
  constexpr int TILE_BYTES = KT * RS;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // K[2][KT][RS] | V[2][KT][RS]

  // Workgroup -> (sequence, query tile, head).  The grid is COMPACT: x runs over tile slots, at most
  // total_q / tile_rows + batch of them, and each workgroup finds the sequence that owns its slot
  // by walking the cumulative lengths (a launch sized (max_q tiles) x batch would, for one 2017-token
  // chunk next to 31 decode rows, dispatch 30 752 workgroups that exit at once — measured 847 us for
  // work that takes 190 us).  Hardware deals consecutive workgroups round-robin to the 8 XCDs, each
  // with its own L2; the query tiles of one (sequence, head) stream the same K / V, so ids are
  // renumbered to put them on ONE XCD (ids congruent mod 8 form a contiguous range of slots).
  // Within a sequence the causal tiles get longer with the row index: the long ones go first.
  constexpr int WROWS = 16 * QR;             // query rows per wave
  constexpr int TQ = 4 * WROWS;              // query rows per workgroup
  int mblk, h, b;
  {
    const int gx = gridDim.x, gy = gridDim.y;
    const int total = gx * gy;
    int wg = blockIdx.x + gx * blockIdx.y;
    if (p.xcd_remap && total % 8 == 0) wg = (wg % 8) * (total / 8) + wg / 8;
    int slot = wg % gx;
    h = wg / gx;
    b = 0;
    int tiles = 0;
    for (; b < p.batch; ++b) {
      tiles = (p.cu_q[b + 1] - p.cu_q[b] + TQ - 1) / TQ;
      if (slot < tiles) break;
      slot -= tiles;
    }
    if (b == p.batch) return;                // spare slot (the grid is an upper bound)
    mblk = tiles - 1 - slot;
  }
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int hk = h / p.group;

  const int q_start = p.cu_q[b];
  const int q_len = p.cu_q[b + 1] - q_start;
  const int k_start = p.cu_k[b];
  const int kv_len = p.cu_k[b + 1] - k_start;
  const int q_row0_wg = mblk * TQ;
  if (q_row0_wg >= q_len) return;            // workgroup-uniform
  const int q_row0 = q_row0_wg + w * WROWS;  // may exceed q_len for the last workgroup's waves:
                                             // those waves still load / synchronise, never store

  char* kbuf = smem;
  char* vbuf = smem + 2 * TILE_BYTES;
  const u16* kbase = reinterpret_cast<const u16*>(p.k) + (int64_t)hk * p.k_head_stride;
  const u16* vbase = reinterpret_cast<const u16*>(p.v) + (int64_t)hk * p.v_head_stride;
  const int32_t* bt = PAGED ? p.block_table + p.cu_block_lens[b] : nullptr;

  // Q^T fragments (B operand): lane (c,g) holds Q[row 16 rb + c][32s + 8g + j]
  u16x8 qf[QR][NS];
#pragma unroll
  for (int rb = 0; rb < QR; ++rb) {
    const int qr = min(q_row0 + 16 * rb + c, q_len - 1);
    const u16* qp = reinterpret_cast<const u16*>(p.q) + (int64_t)(q_start + qr) * p.q_row_stride +
                    (int64_t)h * D + 8 * g;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[rb][s] = *reinterpret_cast<const u16x8*>(qp + 32 * s);
  }

  const int shift = kv_len - q_len;
  // visible keys of query row i: [i + shift - window_left, i + shift + window_right] (mask.h:173-193);
  // causal = (unbounded, 0); no mask = both unbounded
  const bool local = p.window_left >= 0;             // the dispatcher sets both sides for a local call
  const int wr = p.causal ? 0 : local ? p.window_right : 0x3fffffff;
  const int wl = local ? p.window_left : 0x3fffffff;
  int limit_c[QR], first_c[QR];
#pragma unroll
  for (int rb = 0; rb < QR; ++rb) {
    const int row = q_row0 + 16 * rb + c + shift;
    limit_c[rb] = (int)min((int64_t)kv_len - 1, (int64_t)row + wr);
    first_c[rb] = (int)max((int64_t)0, (int64_t)row - wl);
  }
  // a wave whose rows all lie past the sequence (q_len = 1: three of the four) only helps staging
  const int last_key_wave = q_row0 >= q_len ? -1 : (int)min((int64_t)kv_len - 1, (int64_t)q_row0 + WROWS - 1 + shift + wr);
  const int last_key_wg =
      (int)min((int64_t)kv_len - 1, (int64_t)min(q_row0_wg + 4 * WROWS - 1, q_len - 1) + shift + wr);
  const int first_key_wg = (int)max((int64_t)0, (int64_t)q_row0_wg + shift - wl);
  const int first_key_wave = (int)max((int64_t)0, (int64_t)q_row0 + shift - wl);
  const int t_first = local ? first_key_wg / KT : 0;                   // tiles left of the window are skipped
  const int n_tiles = (last_key_wg >= 0) ? last_key_wg / KT + 1 : 0;   // workgroup-uniform

  // ---- cooperative tile staging: thread owns chunks idx = tid + 256*j of the [32][D] tile
  int my_row[NL], my_chunk[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int idx = threadIdx.x + 256 * j;
    my_row[j] = idx / LPR;
    my_chunk[j] = idx % LPR;
  }
  // element offset of key row `key` given its page (paged) — the page id is looked up ONE TILE
  // AHEAD of the loads that need it, so a tile's loads are a single round trip, not two
  auto page_of = [&](int key) -> int {
    return PAGED ? bt[page_slot(min(key, kv_len - 1), p.block_size, p.block_shift)] : 0;
  };
  auto key_offset = [&](int key, int page, bool is_v) -> int64_t {
    key = min(key, kv_len - 1);
    if (PAGED) {
      const int row = page_row(key, p.block_size, p.block_shift);
      return is_v ? (int64_t)page * p.v_block_stride + (int64_t)row * p.v_row_stride
                  : (int64_t)page * p.k_block_stride + (int64_t)row * p.k_row_stride;
    }
    return (int64_t)(k_start + key) * (is_v ? p.v_row_stride : p.k_row_stride);
  };
  u16x8 kreg[NL], vreg[NL];
  int page_next[NL];      // pages of the tile that will be loaded next
  auto lookup_pages = [&](int t) {
#pragma unroll
    for (int j = 0; j < NL; ++j) page_next[j] = page_of(t * KT + my_row[j]);
  };
  auto load_tile = [&](int t) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      if (TILE_CHUNKS % 256 == 0 || threadIdx.x + 256 * j < TILE_CHUNKS) {
        const int key = t * KT + my_row[j];
        kreg[j] = *reinterpret_cast<const u16x8*>(kbase + key_offset(key, page_next[j], false) + 8 * my_chunk[j]);
        vreg[j] = *reinterpret_cast<const u16x8*>(vbase + key_offset(key, page_next[j], true) + 8 * my_chunk[j]);
      }
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      if (TILE_CHUNKS % 256 == 0 || threadIdx.x + 256 * j < TILE_CHUNKS) {
        const int off = buf * TILE_BYTES + my_row[j] * RS + my_chunk[j] * 16;
        *reinterpret_cast<u16x8*>(kbuf + off) = kreg[j];
        *reinterpret_cast<u16x8*>(vbuf + off) = vreg[j];
      }
    }
  };

  f32x4 acc[QR][NDB];
  float m[QR], l[QR];
#pragma unroll
  for (int rb = 0; rb < QR; ++rb) {
#pragma unroll
    for (int i = 0; i < NDB; ++i) acc[rb][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[rb] = HX_NEG_BIG;
    l[rb] = 0.f;
  }

  if (n_tiles > t_first) {
    lookup_pages(t_first);
    load_tile(t_first);
    lookup_pages(t_first + 1);
    store_tile(t_first & 1);
  }
  __syncthreads();

  // ALIBI: score(i, j) -= slope * |i + shift - j| (alibi.h / mask.h:112-190), added after the soft cap and before the
  // masks.  The RELATIVE form also under a causal mask, where the reference adds slope * j: a constant per row apart, the
  // same softmax, and magnitudes that stay small at long contexts.  The scores are still unscaled here (the scale is
  // folded into the exponent below), so the slope is divided by that scale — softmax_scale, or the cap when one is set,
  // as the reference does (flash_fwd_kernel.h:244).
  float slope_s = 0.f;
  int pos_c[QR];
  if constexpr (ALIBI) {
    slope_s = alibi_slope_log2(p, b, h) / p.scale_log2;
#pragma unroll
    for (int rb = 0; rb < QR; ++rb) pos_c[rb] = q_row0 + 16 * rb + c + shift;
  }

  const int q4 = c >> 2, p4 = c & 3;
  for (int t = t_first; t < n_tiles; ++t) {
    const int cur = t & 1;
    if (t + 1 < n_tiles) {
      load_tile(t + 1);                          // in flight under this tile's MFMAs
      lookup_pages(t + 2);                       // (clamped to the last key) for the next iteration
    }

    if (t * KT <= last_key_wave && t * KT + KT - 1 >= first_key_wave) {   // wave-uniform: tiles outside this wave's band
      const char* kt = kbuf + cur * TILE_BYTES;
      const char* vt = vbuf + cur * TILE_BYTES;
      // ---- S^T = K . Q^T for the 2 KU 16-key sub-tiles (A fragments from the shared K image,
      //      each used for the QR row blocks of this wave)
      f32x4 s[QR][2 * KU];
#pragma unroll
      for (int u = 0; u < 2 * KU; ++u) {
#pragma unroll
        for (int rb = 0; rb < QR; ++rb) s[rb][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < NS; ++st) {
          const u16x8 kf = *reinterpret_cast<const u16x8*>(kt + (16 * u + c) * RS + 64 * st + 16 * g);
#pragma unroll
          for (int rb = 0; rb < QR; ++rb) s[rb][u] = Mfma<T>::mma(kf, qf[rb][st], s[rb][u]);
        }
      }
      if (p.softcap_scale > 0.f) {                 // scores = softcap * tanh(q.k * scale / softcap), utils.h:383-388
#pragma unroll
        for (int rb = 0; rb < QR; ++rb)
#pragma unroll
          for (int u = 0; u < 2 * KU; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[rb][u][i] = tanhf(s[rb][u][i] * p.softcap_scale);
      }
      if constexpr (ALIBI) {
#pragma unroll
        for (int rb = 0; rb < QR; ++rb)
#pragma unroll
          for (int u = 0; u < 2 * KU; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              s[rb][u][i] -= slope_s * fabsf((float)(pos_c[rb] - (t * KT + u * 16 + 4 * g + i)));
      }
      // ---- mask + online softmax (per query column c; state replicated over g).  The scale is
      //      folded into the exponent's fma; tiles that no row of this wave masks skip the compares
      //      (wave-uniform) — the inner loop is VALU-bound (PMC: ~15 vector instructions per MFMA).
      const bool interior = !local && t * KT + KT - 1 <= min(kv_len - 1, p.causal ? q_row0 + shift : kv_len - 1);
      u16x8 pf[QR][KU];
#pragma unroll
      for (int rb = 0; rb < QR; ++rb) {
        float mx = HX_NEG_BIG;
        if (interior) {
#pragma unroll
          for (int u = 0; u < 2 * KU; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[rb][u][i]);
        } else {
#pragma unroll
          for (int u = 0; u < 2 * KU; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int key = t * KT + u * 16 + 4 * g + i;
              if (key > limit_c[rb] || key < first_c[rb]) s[rb][u][i] = -INFINITY;
              mx = fmaxf(mx, s[rb][u][i]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m[rb], mx * p.scale_log2);
        const float alpha = fast_exp2(m[rb] - m_new);
        m[rb] = m_new;
        float ps = 0.f;
#pragma unroll
        for (int hf = 0; hf < KU; ++hf)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float e = fast_exp2(fmaf(s[rb][2 * hf + (j >> 2)][j & 3], p.scale_log2, -m_new));
            ps += e;
            pf[rb][hf][j] = T::from_float(e);
          }
        l[rb] = l[rb] * alpha + ps;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {   // wave-uniform: some row's maximum moved
#pragma unroll
          for (int i = 0; i < NDB; ++i) acc[rb][i] *= alpha;
        }
      }
      // ---- O^T += V^T . P^T (V^T fragments by transposed LDS reads of the shared V image)
#pragma unroll
      for (int hf = 0; hf < KU; ++hf) {
        const char* vrd = vt + (32 * hf + 4 * g + q4) * RS + p4 * 8;
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          const u16x4 lo = lds_tr_read(vrd + db * 32);
          const u16x4 hi = lds_tr_read(vrd + 16 * RS + db * 32);
          u16x8 vf;
          vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
          vf[4] = hi[0]; vf[5] = hi[1]; vf[6] = hi[2]; vf[7] = hi[3];
#pragma unroll
          for (int rb = 0; rb < QR; ++rb) acc[rb][db] = Mfma<T>::mma(vf, pf[rb][hf], acc[rb][db]);
        }
      }
    }
    if (t + 1 < n_tiles) store_tile(cur ^ 1);
    __syncthreads();    // tile t+1 visible; everyone is done with tile t's image
  }

  // ---- epilogue: O[q 16 rb + c][dim 16db + 4g + i] = acc[rb][db][i] / L
#pragma unroll
  for (int rb = 0; rb < QR; ++rb) {
    float lr = l[rb];
    lr += __shfl_xor(lr, 16, 64);
    lr += __shfl_xor(lr, 32, 64);
    const float inv = (lr > 0.f) ? 1.0f / lr : 0.f;
    const int row = q_row0 + 16 * rb + c;
    if (row < q_len) {
      u16* op = reinterpret_cast<u16*>(p.out) + (int64_t)(q_start + row) * p.o_row_stride +
                (int64_t)h * D + 4 * g;
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        u16x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = T::from_float(acc[rb][db][i] * inv);
        *reinterpret_cast<u16x4*>(op + 16 * db) = r;
      }
    }
  }
