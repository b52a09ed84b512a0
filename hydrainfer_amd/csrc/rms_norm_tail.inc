// rms_norm_tail.inc — the second half of an RMSNorm row that its threads hold in registers: the inverse RMS from the
// row's sum of squares, then out = (T)(x * inv) * weight with two T roundings (the reference's rms_norm.cu:39).
// Included by rms_norm_vec_kernel, embed_rms_norm_row and add_rms_norm_slab_kernel.  The including kernel's names:
//   T, V, N, MAXV      element traits, the 16-byte vector of N elements, vectors per thread
//   kNT                threads per row
//   x[MAXV][N], total  the row in fp32 and its sum of squares (block_sum)
//   hidden, eps, nvec  the row's elements, epsilon, vectors
//   w_at(j, i)         the weight vector i, which is this thread's j-th: loaded here or held since the first pass
//   out_v, frag_mb     the output row; frag_mb > 0: fragment-major (hydra_hip.h), vector i of the row goes to piece
//                      (i / 4) * frag_mb * 64 + (i % 4) * 16 behind out_v; 0: row-major
  const float inv = rsqrtf(total / (float)hidden + eps);
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    const int i = threadIdx.x + j * kNT;
    if (i < nvec) {
      const V w = w_at(j, i);
      V o;
#pragma unroll
      for (int e = 0; e < N; ++e) o[e] = T::from_float(round_to<T>(x[j][e] * inv) * T::to_float(w[e]));
      out_v[frag_mb ? (i >> 2) * frag_mb * 64 + (i & 3) * 16 : i] = o;
    }
  }
