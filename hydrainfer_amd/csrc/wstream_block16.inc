// wstream_block16.inc — one column block of 16-bit weights (16 rows x 64 k = two load instructions) through the wave's
// transpose image: write, two MFMA steps 16x16x32 per 16 token rows straight into the accumulators.  Textually
// included ONCE into gemm_skinny_kernel and into moe_gemm_kernel (through moe_gemm_body.inc).
// Expects in scope: everything of wstream_image.inc; T; MB; `nmb`, the 16-row blocks of x that hold rows (the dense
// kernel: the constant MB); `wbuf`, the stream's register buffer, and `cb`, the column block in it; `xp`, the lane's
// B-fragment address at the buffer's first k (row stride kRS); `accb`, the MB accumulators this stream adds to.
*reinterpret_cast<u16x8*>(tl + wr_off0) = wbuf[2 * cb];
*reinterpret_cast<u16x8*>(tl + wr_off1) = wbuf[2 * cb + 1];
__builtin_amdgcn_wave_barrier();
#pragma unroll
for (int st = 0; st < 2; ++st) {
  const u16x8 af = a_read16(st);
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    if (mb < nmb) {
      const u16x8 xf = *reinterpret_cast<const u16x8*>(xp + mb * 16 * kRS + (2 * cb + st) * 64);
      accb[mb] = Mfma<T>::mma(af, xf, accb[mb]);
    }
  }
}
__builtin_amdgcn_wave_barrier();
