// gemm_xreg_load_x_norm.inc — body text: the produced x behind the NORM = 1 hand-over into xb[slot][mb], for the k-steps
// x_ks0 + w * KW + (0 .. x_kw - 1), which the including kernel declares in front.  mbl = 16-row blocks of the
// fragment-major x (narrow: the constant MB; wide: ceil(M / 16), the last MFMA column block re-reads the one before).
// sc1 loads (kXAux; served past this CU's L1 and the XCD's L2; the bytes were written through by other CUs).
//    Round 3 measured what that costs — 256 CUs x 256 KiB = 67 MB over the XCD links: with sc0 loads (L2 hits; sound
//    only by the argument that a kernel's start invalidates the L2) or with no x loads at all the first row group
//    ends ~1 us earlier (12.7 -> 11.5 us, tools/xreg_timeline.py) and the decode step does not move: not taken.
const rsrc_t xrs = make_rsrc(p.x), zrs = make_rsrc(g_zero_line);
#pragma unroll
for (int t = 0; t < KW; ++t) {
  const int r = rot(t);
  const bool ok = r < x_kw;
  const int ks = min(x_ks0 + w * KW + r, total_ks - 1);
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    // padding slots (K rounded up to the wave's k-step count) read the zero line
    xb[t][mb] = __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(
        ok ? xrs : zrs, ok ? (uint32_t)((ks * mbl + min(mb, mbl - 1)) * 64 + lane) * 16 : (uint32_t)(lane & 7) * 16, 0, kXAux));
  }
}
