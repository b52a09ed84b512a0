// wstream_block_fp8.inc — one 128-k scale block of FP8 weights (16 rows x 128 e4m3 bytes = two load instructions: an
// image holds exactly one scale block) through the wave's transpose image: write, four MFMA steps 16x16x32 per 16 token
// rows — the A fragment a ds_read_b64 widened to T (fp8_widen.h, exact) — into a temporary that starts at zero, then
// one fma(tmp, scale, acc): a weight is never rounded after it has been scaled.  Textually included ONCE into
// gemm_skinny_fp8w_kernel and into moe_gemm_fp8w_kernel (through moe_gemm_body.inc).
// Expects in scope: everything of wstream_image.inc; T; MB; `nmb`, the 16-row blocks of x that hold rows (the dense
// kernel: the constant MB); `wbuf`, the stream's register buffer, `wscale`, its scales, and `cb`, the scale block in
// them (a scale is wave-uniform: a wave's 16 rows lie inside one 128-row block); `xp`, the lane's B-fragment address at the
// buffer's first k (row stride kRS); `accb`, the MB accumulators this stream adds to.
*reinterpret_cast<u32x4*>(tl + wr_off0) = wbuf[2 * cb];
*reinterpret_cast<u32x4*>(tl + wr_off1) = wbuf[2 * cb + 1];
__builtin_amdgcn_wave_barrier();
f32x4 tmp[MB];
#pragma unroll
for (int mb = 0; mb < MB; ++mb) tmp[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
for (int st = 0; st < 4; ++st) {
  const u16x8 af = widen<T>(a_read8(st));
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    if (mb < nmb) {
      const u16x8 xf = *reinterpret_cast<const u16x8*>(xp + mb * 16 * kRS + (4 * cb + st) * 64);
      tmp[mb] = Mfma<T>::mma(af, xf, tmp[mb]);
    }
  }
}
const float sv = wscale[cb];
#pragma unroll
for (int mb = 0; mb < MB; ++mb) {
  if (mb < nmb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) accb[mb][i] = __builtin_fmaf(tmp[mb][i], sv, accb[mb][i]);
  }
}
__builtin_amdgcn_wave_barrier();
