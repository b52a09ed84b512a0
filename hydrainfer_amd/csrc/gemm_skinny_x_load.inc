// gemm_skinny_x_load.inc — the workgroup's slice of x, [MB * 16 rows][1024 k], into registers: the first half of its way
// into LDS (second half: gemm_skinny_x_store.inc; the kernel issues its weight prefetch between the two).  Textually
// included ONCE into each split-K decode GEMM (gemm_skinny_kernel, gemm_packed_kernel, gemm_skinny_fp8w_kernel).
// The LDS image always spans 1024 k; k beyond this split's range and rows beyond M are zero there, so a short last split
// needs no predication.  The loads here always have a valid address; the zero-fill select happens at the LDS write so
// that no loaded value is consumed before the weight prefetch has been issued.
// Expects in scope: `p` (x, ldx, M), `xb` = x at the split's first k, `KR` = k of this split, kThreads, MB, and kNoXLoads
// (timing ablation of gemm_packed_kernel: constants in place of the loads — wrong results; false elsewhere).
// Gives: kCpr, XPT and the registers `xr`.
constexpr int kCpr = 1024 / 8;                           // 16-byte chunks per LDS row
constexpr int XPT = MB * 16 * kCpr / kThreads;           // chunks per thread
u16x8 xr[XPT];
#pragma unroll
for (int j = 0; j < XPT; ++j) {
  const int i = threadIdx.x + j * kThreads;
  const int row = i / kCpr, ch = i % kCpr;
  const bool ok = row < p.M && ch * 8 < KR;
  if (kNoXLoads) xr[j] = u16x8{1, 2, 3, 4, 5, 6, 7, 8};
  else xr[j] = *reinterpret_cast<const u16x8*>(xb + (int64_t)(ok ? row : 0) * p.ldx + (ok ? ch * 8 : 0));
}
