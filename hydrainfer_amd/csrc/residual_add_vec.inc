// residual_add_vec.inc — h = (T)(v + r) for one vector, the residual add in T arithmetic: the rounded sum goes to x[j]
// in fp32 and back to `residual`.  Included by rms_norm_vec_kernel<.., ADD> and layer_norm_vec_kernel<.., ADD>.
// The including kernel's names: T, V, N, v (the input vector), r (the residual vector), x, j, i, res_v.
        V h;
#pragma unroll
        for (int e = 0; e < N; ++e) {
          x[j][e] = round_to<T>(T::to_float(v[e]) + T::to_float(r[e]));
          h[e] = T::from_float(x[j][e]);
        }
        res_v[i] = h;
