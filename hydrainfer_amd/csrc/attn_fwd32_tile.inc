// attn_fwd32_tile.inc — one 64-key tile step of the 32x32x16 prefill kernels: S^T = K . Q^T, mask, online softmax with
// the lazy running maximum, P rounded to T, O^T += V^T . P^T.  Included into the tile_step of attn_fwd32_kernel and of
// attn_fwd32p_kernel: whatever changes here changes both, which the tests hold bit-identical to each other.
// Expects in scope: `p`, T, ABL (timing ablations, EXPERIMENTS builds: 1 no softmax arithmetic, 2 no P V product, 4 no
// Q K product — wrong results; 0 in the persistent kernel), everything of attn_fwd32_geom.inc and attn_fwd32_lane.inc,
// `lane`, `c` (lane & 31) and `hi` (lane >> 5); the tile index `t`
// and `img_cur`, the LDS image that holds it; the Q fragments `qf`; the running state `acc`, `m`, `l`; the mask limits
// `limit_c`, `last_key_wave`, `last_key`, `q_row0`, `shift`; and `half_max(x)`, the maximum of x over lanes l and l ^ 32.
    if (t * KT <= last_key_wave) {
      const char* kt = smem + img_cur * IMG;
      const char* vt = kt + KTILE;
      f32x16 s[2];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[u][r] = 0.f;
      {
        // all K fragments of sub-tile 0 are requested before its first MFMA, those of sub-tile 1
        // under sub-tile 0's MFMAs: no MFMA waits for a read issued just before it
        const char* krd = kt + c * RSK;
        const int kz = kswz(c);
        u16x8 kfa[KS], kfb[KS];
        if (ABL & 4) {
#pragma unroll
          for (int r = 0; r < 16; ++r) { s[0][r] = 0.01f * (r + lane); s[1][r] = 0.02f * (r + t); }
        } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kfa[ks] = *reinterpret_cast<const u16x8*>(krd + 16 * ((2 * ks + hi) ^ kz));
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          kfb[ks] = *reinterpret_cast<const u16x8*>(krd + 32 * RSK + 16 * ((2 * ks + hi) ^ kz));
          s[0] = Mfma32<T>::mma(kfa[ks], qf[ks], s[0]);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s[1] = Mfma32<T>::mma(kfb[ks], qf[ks], s[1]);
        // keep that order: left alone the scheduler issues read, wait, MFMA, read, wait, MFMA (fewest registers)
        __builtin_amdgcn_sched_group_barrier(0x100, KS, 0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, KS, 0);
        }
      }
      const bool interior = t * KT + KT - 1 <= min(last_key, p.causal ? q_row0 + shift : last_key);
      float mx = HX_NEG_BIG;
      u16x8 pf[2][2];
      if (ABL & 1) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) pf[u][r >> 3][r & 7] = T::from_float(s[u][r]);
        l += 1.f;
      } else {
      if (interior) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[u][r]);
      } else {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = t * KT + 32 * u + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (key > limit_c) s[u][r] = -INFINITY;
            mx = fmaxf(mx, s[u][r]);
          }
      }
      mx = half_max(mx);
      // Lazy running maximum: a row keeps its reference m until a score exceeds it by more than 2^8 (the exponentials
      // then stay below 256: exact in fp32, eight mantissa bits as ever in T) — with the exact maximum as reference some
      // row of the 32 moved in nearly every tile and all 64 accumulator registers were rescaled every time (PMC: 33
      // v_pk_mul per wave and tile).  O = acc / l is unchanged in exact arithmetic: both carry the same factor.
      const float m_cand = fmaxf(m, mx * p.scale_log2);
      const bool grow = m_cand > m + 8.0f;
      float m_new = m;
      if (__builtin_amdgcn_ballot_w64(grow)) {
        m_new = grow ? m_cand : m;
        const float alpha = fast_exp2(m - m_new);      // 1 for the rows that keep their reference
        l *= alpha;
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][r] *= alpha;
        m = m_new;
      }
      // (single-instruction fma / add: a packed f32 instruction beside MFMAs costs more than the two it replaces —
      // MI355X_MICROARCH.md, per-instruction constants; the file is compiled without the SLP vectorizer for the same reason)
      float pa = 0.f, pb = 0.f;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          const float e0 = fast_exp2(fmaf(s[u][r], p.scale_log2, -m_new));
          const float e1 = fast_exp2(fmaf(s[u][r + 1], p.scale_log2, -m_new));
          pa += e0;
          pb += e1;
          pf[u][r >> 3][r & 7] = T::from_float(e0);
          pf[u][r >> 3][(r & 7) + 1] = T::from_float(e1);
        }
      l += pa + pb;
      }
      if (ABL & 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int k2 = 0; k2 < 2; ++k2) acc[0][u * 2 + k2] += __builtin_bit_cast(float, (uint32_t)pf[u][k2][0] << 16);
      } else
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const char* vrd = vt + (32 * u + 16 * k2) * RSV + tr_off;
#pragma unroll
          for (int db = 0; db < NDB; ++db) {
            const u16x4 lo = lds_tr_read(vrd + 64 * (db ^ tr_x));
            const u16x4 hh = lds_tr_read(vrd + 8 * RSV + 64 * (db ^ tr_x));
            u16x8 vf;
            vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
            vf[4] = hh[0]; vf[5] = hh[1]; vf[6] = hh[2]; vf[7] = hh[3];
            acc[db] = Mfma32<T>::mma(vf, pf[u][k2], acc[db]);
          }
        }
    }
