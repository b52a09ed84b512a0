// argmax_finish.inc — the workgroup finish of argmax_rows_kernel and penalized_argmax_rows_kernel (1024 threads): the
// first of all threads' (best, bi) in hx::arg_better's order, written by thread 0.  Included text, not a function
// (profiles/token_choice_refactor.md).  In scope: best, bi (this thread's pick), s_v, s_i (16 words of LDS each), ids, row.
#pragma unroll
for (int off = 32; off > 0; off >>= 1) {
  const float ov = __shfl_xor(best, off, 64);
  const int oi = __shfl_xor(bi, off, 64);
  if (arg_better(ov, oi, best, bi)) { best = ov; bi = oi; }
}
if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = bi; }
__syncthreads();
if (threadIdx.x == 0) {
  for (int k = 1; k < 16; ++k)
    if (arg_better(s_v[k], s_i[k], best, bi)) { best = s_v[k]; bi = s_i[k]; }
  ids[row] = bi;
}
