// gemm_xreg_load_x.inc — the x fragments of a wave's k-steps into xb[slot][mb], textually included ONCE into each of
// the two activations-in-registers kernels (gemm_xreg.hip) behind xb, xp, zp.  mbl = 16-row blocks of the
// fragment-major x (narrow: the constant MB; wide: ceil(M / 16), the last MFMA column block re-reads the one before);
// DBG bit 0: ablation without x loads (narrow kernel only).
auto load_x_block = [&](int q) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int t = 8 * q + j;
    if (t < KW) {
      const int r = rot(t);
      const bool ok = r < kw;
      const int ks = min(ks0 + w * KW + r, total_ks - 1);
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const int m = min(mb * 16 + c, p.M - 1);
        const u16* src = ok ? (p.x_packed ? reinterpret_cast<const u16*>(p.x) + ((int64_t)(ks * mbl + min(mb, mbl - 1)) * 64 + lane) * 8
                                          : xp + (int64_t)m * p.ldx + (int64_t)ks * 32)
                            : zp;
        if (DBG & 1) xb[t][mb] = u16x8{1, 2, 3, 4, 5, 6, (u16)t, (u16)lane};   // ablation: no x loads
        else xb[t][mb] = *reinterpret_cast<const u16x8*>(src);
      }
    }
  }
};
