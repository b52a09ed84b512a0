// rope_neox_vec_rotate.inc — one step of the vector NeoX rotation: work item i = (head h: q heads then kv heads,
// vector rv of the head's first half) of this token, rotated in place in q / k.  The body of
// `for (int i = threadIdx.x; i < total; i += 256)` in rope_neox_vec_kernel and rope_cache_neox_vec_kernel.
// The including kernel's names: T, V, N, i, vph, half, n_heads, head_dim, token, q, k, q_stride, k_stride, cs.
// Behind it h, rv, is_k and the rotated vectors xo / yo are there for the including kernel (the cache write).
    const int h = i / vph;
    const int rv = i - h * vph;
    const bool is_k = h >= n_heads;
    typename T::storage* base = !is_k ? (q + token * q_stride + (int64_t)h * head_dim)
                                      : (k + token * k_stride + (int64_t)(h - n_heads) * head_dim);
    V* xp = reinterpret_cast<V*>(base + rv * N);
    V* yp = reinterpret_cast<V*>(base + half + rv * N);
    const V cv = *reinterpret_cast<const V*>(cs + rv * N);
    const V sv = *reinterpret_cast<const V*>(cs + half + rv * N);
    V xv = *xp, yv = *yp, xo, yo;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      float a, b;
      rotate_pair<T>(T::to_float(xv[e]), T::to_float(yv[e]), T::to_float(cv[e]), T::to_float(sv[e]), a, b);
      xo[e] = T::from_float(a);
      yo[e] = T::from_float(b);
    }
    *xp = xo;
    *yp = yo;
