// logprobs_stage.inc — the row of an LDS = true kernel of logprobs.hip, copied from global memory into LDS once.
// Included text, not a function: as a function it changes the kernels' code (profiles/token_choice_refactor.md).
// In scope: p (the row in global memory), n, gvec (p may be read in 16-byte pieces), staged (LDS, n rounded up to 8
// elements), src and vec (left naming the staged row, which is always read in pieces).
if (gvec) {
  const int nvec = n >> 3;
  // four independent 16-byte loads per thread in flight, like argmax_rows_kernel: one memory round trip for a
  // 32064-wide row
  for (int i0 = threadIdx.x; i0 < nvec; i0 += 4 * LP_THREADS) {
    u16x8 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const u16x8*>(p + (int64_t)min(i0 + LP_THREADS * u, nvec - 1) * 8);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + LP_THREADS * u;
      if (i < nvec) *reinterpret_cast<u16x8*>(staged + i * 8) = v[u];
    }
  }
  for (int i = nvec * 8 + threadIdx.x; i < n; i += LP_THREADS) staged[i] = p[i];
} else {
  for (int i = threadIdx.x; i < n; i += LP_THREADS) staged[i] = p[i];
}
__syncthreads();
src = staged;
vec = true;
