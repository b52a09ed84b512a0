// gemm_skinny_x_store.inc — the second half of gemm_skinny_x_load.inc: its registers into the LDS image of x (row
// stride kRS), rows beyond M and k beyond the split's range as zeros.  The kernel's __syncthreads() follows.
#pragma unroll
for (int j = 0; j < XPT; ++j) {
  const int i = threadIdx.x + j * kThreads;
  const int row = i / kCpr, ch = i % kCpr;
  const bool ok = row < p.M && ch * 8 < KR;
  *reinterpret_cast<u16x8*>(smem + row * kRS + ch * 16) = ok ? xr[j] : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
}
