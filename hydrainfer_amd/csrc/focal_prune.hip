// focal_prune.hip — focal image-token pruning without a score tensor (include/hydra_hip.h: hx_focal_significance,
// hx_focal_select, hx_focal_gather).  The rule is hydrainfer/layer/token_prunning.py:5-37 applied to the PRE-softmax
// scaled logits of hydrainfer/layer/multihead_attention.py:59-62; every reduction it applies is linear, so the two
// significance vectors come from q and k directly:
//     s2[i] = scale / (H N) * sum_h q[i,h,:] . (sum_j k[j,h,:])        s1[j] = scale / (H N) * sum_h (sum_i q[i,h,:]) . k[j,h,:]
// No floating-point atomics anywhere; every sum has a fixed order, so two runs agree bit for bit.
#include "hx_common.h"

namespace hx {

#define FOCAL_SPLITS 2          // row ranges per (image, head) in the column-sum launch
#define FOCAL_TOK_PER_WG 8      // tokens per workgroup (two per wave) in the dot-product launch
#define FOCAL_MAX_WIDTH 8192    // n_heads * head_dim: two fp32 vectors of that width in LDS (64 KiB)
#define FOCAL_MAX_N 4096
#define FOCAL_SEL_THREADS 1024

template <typename T>
__device__ __forceinline__ void load8(const u16* p, float* f) {
  const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = T::to_float(v[e]);
}

// Launch A.  Workgroup (head, split, image): fp32 column sums of q and k over the split's rows.  Thread (r, c) walks the
// rows r, r + R, ... of the range with the 16-byte chunk c of the head; the R partial rows are then summed in order.
// ws: [n_images][FOCAL_SPLITS][2][W] fp32 (q sums, k sums).
template <typename T>
__global__ __launch_bounds__(256) void focal_colsum_kernel(float* __restrict__ ws, const u16* __restrict__ q,
                                                           const u16* __restrict__ k, int tokens_per_image, int skip,
                                                           int n_heads, int head_dim, int64_t q_row_stride,
                                                           int64_t k_row_stride) {
  __shared__ float red[2][2048];
  const int h = blockIdx.x, s = blockIdx.y, b = blockIdx.z;
  const int N = tokens_per_image - skip;
  const int C = head_dim >> 3;            // 16-byte chunks of a head (<= 256)
  const int R = 256 / C;
  const int per = (N + FOCAL_SPLITS - 1) / FOCAL_SPLITS;
  const int lo = s * per, hi = min(N, lo + per);
  const int r = threadIdx.x / C, c = threadIdx.x - r * C;
  float aq[8], ak[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) aq[e] = ak[e] = 0.f;
  if (r < R) {
    const int64_t row0 = (int64_t)b * tokens_per_image + skip;
    const int col = h * head_dim + c * 8;
    for (int i = lo + r; i < hi; i += R) {
      float fq[8], fk[8];
      load8<T>(q + (row0 + i) * q_row_stride + col, fq);
      load8<T>(k + (row0 + i) * k_row_stride + col, fk);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        aq[e] += fq[e];
        ak[e] += fk[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[0][r * head_dim + c * 8 + e] = aq[e];
      red[1][r * head_dim + c * 8 + e] = ak[e];
    }
  }
  __syncthreads();
  const int W = n_heads * head_dim;
  float* out = ws + ((int64_t)b * FOCAL_SPLITS + s) * 2 * W + h * head_dim;
  for (int t = threadIdx.x; t < 2 * head_dim; t += 256) {
    const int which = t >= head_dim, d = t - which * head_dim;
    float acc = 0.f;
    for (int rr = 0; rr < R; ++rr) acc += red[which][rr * head_dim + d];
    out[which * W + d] = acc;
  }
}

// Launch B.  One wave per token over the whole H*D-wide row; the two summed vectors (the splits added in order) wait in LDS.
template <typename T>
__global__ __launch_bounds__(256) void focal_dot_kernel(float* __restrict__ s1, float* __restrict__ s2,
                                                        const float* __restrict__ ws, const u16* __restrict__ q,
                                                        const u16* __restrict__ k, int tokens_per_image, int skip, int W,
                                                        int64_t q_row_stride, int64_t k_row_stride, float factor) {
  extern __shared__ float sums[];          // [0, W): column sums of q; [W, 2W): of k
  const int b = blockIdx.y;
  const int N = tokens_per_image - skip;
  const float* base = ws + (int64_t)b * FOCAL_SPLITS * 2 * W;
  for (int c = threadIdx.x; c < 2 * W; c += 256) {
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < FOCAL_SPLITS; ++s) acc += base[s * 2 * W + c];
    sums[c] = acc;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int first = blockIdx.x * FOCAL_TOK_PER_WG;
  const int64_t row0 = (int64_t)b * tokens_per_image + skip;
  for (int i = first + wave; i < min(N, first + FOCAL_TOK_PER_WG); i += 4) {
    float a1 = 0.f, a2 = 0.f;
    for (int ch = lane; ch < (W >> 3); ch += 64) {
      float fq[8], fk[8];
      load8<T>(q + (row0 + i) * q_row_stride + ch * 8, fq);
      load8<T>(k + (row0 + i) * k_row_stride + ch * 8, fk);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a2 = fmaf(fq[e], sums[W + ch * 8 + e], a2);
        a1 = fmaf(fk[e], sums[ch * 8 + e], a1);
      }
    }
    a1 = wave_sum(a1);
    a2 = wave_sum(a2);
    if (lane == 0) {
      s1[(int64_t)b * N + i] = a1 * factor;
      s2[(int64_t)b * N + i] = a2 * factor;
    }
  }
}

// ---- selection: one workgroup of 1024 threads per image
__device__ __forceinline__ float focal_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                         // (red may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float total = 0.f;
#pragma unroll
  for (int w = 0; w < FOCAL_SEL_THREADS / 64; ++w) total += red[w];
  return total;
}

// unbiased variance, two passes, fp32; element i of a thread: i = threadIdx.x + 1024 * m
__device__ __forceinline__ float focal_variance(const float* __restrict__ x, int N, float* red) {
  float a = 0.f;
  for (int i = threadIdx.x; i < N; i += FOCAL_SEL_THREADS) a += x[i];
  const float mean = focal_block_sum(a, red) / (float)N;
  a = 0.f;
  for (int i = threadIdx.x; i < N; i += FOCAL_SEL_THREADS) {
    const float d = x[i] - mean;
    a = fmaf(d, d, a);
  }
  return focal_block_sum(a, red) / (float)(N - 1);
}

// g == 0: 'rank'; g > 0: 'row' with a g x g grid (N == g * g)
__global__ __launch_bounds__(FOCAL_SEL_THREADS) void focal_select_kernel(int32_t* __restrict__ ids_out,
                                                                         const float* __restrict__ s1,
                                                                         const float* __restrict__ s2,
                                                                         const int32_t* __restrict__ n_keep, int N, int g) {
  __shared__ float sig[FOCAL_MAX_N];
  __shared__ float red[FOCAL_SEL_THREADS / 64];
  __shared__ int scan[FOCAL_SEL_THREADS];
  __shared__ float row_sum[64];
  __shared__ int row_keep[64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* x1 = s1 + (int64_t)b * N;
  const float* x2 = s2 + (int64_t)b * N;
  int32_t* ids = ids_out + (int64_t)b * N;
  const int n = min(max(n_keep[b], 0), N);
  const float v1 = focal_variance(x1, N, red);
  const float v2 = focal_variance(x2, N, red);
  const float* x = v1 > v2 ? x1 : x2;      // (token_prunning.py:22; equal variances and NaN: s2)
  for (int i = tid; i < N; i += FOCAL_SEL_THREADS) sig[i] = x[i];
  __syncthreads();
  constexpr int ROUNDS = FOCAL_MAX_N / FOCAL_SEL_THREADS;
  bool keep[ROUNDS];
  if (g > 0) {
    if (tid < g) {
      float acc = 0.f;
      for (int c = 0; c < g; ++c) acc += sig[tid * g + c];
      row_sum[tid] = acc;
    }
    __syncthreads();
    if (tid < g) {
      const float mine = row_sum[tid];
      int rank = 0;
      for (int j = 0; j < g; ++j) {
        const float o = row_sum[j];
        rank += (o > mine || (o == mine && j < tid)) ? 1 : 0;
      }
      row_keep[tid] = rank < n / g;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < ROUNDS; ++m) {
      const int i = tid + m * FOCAL_SEL_THREADS;
      keep[m] = i < N && row_keep[i / g];
    }
  } else {
    float mine[ROUNDS];
    int rank[ROUNDS];
#pragma unroll
    for (int m = 0; m < ROUNDS; ++m) {
      const int i = tid + m * FOCAL_SEL_THREADS;
      mine[m] = i < N ? sig[i] : 0.f;
      rank[m] = 0;
    }
    const int rounds = (N + FOCAL_SEL_THREADS - 1) / FOCAL_SEL_THREADS;
    for (int j = 0; j < N; ++j) {
      const float o = sig[j];
#pragma unroll
      for (int m = 0; m < ROUNDS; ++m)
        if (m < rounds) rank[m] += (o > mine[m] || (o == mine[m] && j < tid + m * FOCAL_SEL_THREADS)) ? 1 : 0;
    }
#pragma unroll
    for (int m = 0; m < ROUNDS; ++m) keep[m] = tid + m * FOCAL_SEL_THREADS < N && rank[m] < n;
  }
  // ascending id list: prefix sum over the keep flags, 1024 ids per round
  int base = 0;
#pragma unroll
  for (int m = 0; m < ROUNDS; ++m) {
    if (m * FOCAL_SEL_THREADS >= N) break;
    __syncthreads();
    scan[tid] = keep[m] ? 1 : 0;
    __syncthreads();
    for (int off = 1; off < FOCAL_SEL_THREADS; off <<= 1) {
      const int add = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += add;
      __syncthreads();
    }
    const int pos = base + scan[tid] - 1;
    if (keep[m] && pos < n) ids[pos] = tid + m * FOCAL_SEL_THREADS;
    base += scan[FOCAL_SEL_THREADS - 1];
  }
  for (int p = min(base, n) + tid; p < N; p += FOCAL_SEL_THREADS) ids[p] = -1;
}

// ---- gather: workgroup (r, image) copies row ids[b, r] of image b, 16 bytes per thread and pass
__global__ __launch_bounds__(256) void focal_gather_kernel(u32x4* __restrict__ out, const u32x4* __restrict__ tokens,
                                                           const int32_t* __restrict__ ids,
                                                           const int32_t* __restrict__ n_keep, int N, int row_vecs,
                                                           int64_t token_stride_vecs, int64_t out_stride_vecs) {
  const int r = blockIdx.x, b = blockIdx.y;
  if (r >= n_keep[b]) return;
  const int id = ids[(int64_t)b * N + r];
  if (id < 0 || id >= N) return;
  const u32x4* src = tokens + ((int64_t)b * N + id) * token_stride_vecs;
  u32x4* dst = out + ((int64_t)b * N + r) * out_stride_vecs;
  for (int v = threadIdx.x; v < row_vecs; v += 256) dst[v] = src[v];
}

template <typename T>
static int launch_significance(float* s1, float* s2, const void* q, const void* k, int n_images, int tokens_per_image,
                               int skip, int n_heads, int head_dim, int64_t q_row_stride, int64_t k_row_stride,
                               float scale, float* ws, hipStream_t s) {
  const int N = tokens_per_image - skip, W = n_heads * head_dim;
  const float factor = (float)((double)scale / ((double)n_heads * (double)N));
  launcher(focal_colsum_kernel<T>, dim3(n_heads, FOCAL_SPLITS, n_images), dim3(256), 0, s)(
      ws, (const u16*)q, (const u16*)k, tokens_per_image, skip, n_heads, head_dim, q_row_stride, k_row_stride);
  launcher(focal_dot_kernel<T>, dim3((N + FOCAL_TOK_PER_WG - 1) / FOCAL_TOK_PER_WG, n_images), dim3(256),
           (size_t)2 * W * sizeof(float), s)(s1, s2, (const float*)ws, (const u16*)q, (const u16*)k, tokens_per_image,
                                             skip, W, q_row_stride, k_row_stride, factor);
  return check_launch();
}

static int focal_shape_status(int64_t n_images, int64_t tokens_per_image, int64_t skip_leading, int64_t n_heads,
                              int64_t head_dim) {
  if (n_images < 0 || skip_leading < 0 || tokens_per_image <= skip_leading || n_heads <= 0 || head_dim <= 0)
    return HX_ERR_SHAPE;
  if (head_dim % 8 != 0 || head_dim > 2048 || n_heads * head_dim > FOCAL_MAX_WIDTH) return HX_ERR_SHAPE;
  if (tokens_per_image - skip_leading > FOCAL_MAX_N || n_images > 65535 || n_heads > 65535) return HX_ERR_SHAPE;
  return HX_OK;
}

}  // namespace hx

using namespace hx;

extern "C" int64_t hx_focal_significance_workspace_bytes(int64_t n_images, int64_t n_heads, int64_t head_dim) {
  if (n_images < 0 || n_heads <= 0 || head_dim <= 0) return HX_ERR_SHAPE;
  return n_images * FOCAL_SPLITS * 2 * n_heads * head_dim * (int64_t)sizeof(float);
}

extern "C" int hx_focal_significance(float* s1, float* s2, const void* q, const void* k, int64_t n_images,
                                     int64_t tokens_per_image, int64_t skip_leading, int64_t n_heads, int64_t head_dim,
                                     int64_t q_row_stride, int64_t k_row_stride, float scale, void* workspace,
                                     int64_t workspace_bytes, int dtype, hx_stream stream) {
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  const int st = focal_shape_status(n_images, tokens_per_image, skip_leading, n_heads, head_dim);
  if (st != HX_OK) return st;
  if (n_images == 0) return HX_OK;
  if (!s1 || !s2 || !q || !k || !workspace) return HX_ERR_NULL;
  const int64_t W = n_heads * head_dim;
  if (q_row_stride < W || k_row_stride < W || q_row_stride % 8 != 0 || k_row_stride % 8 != 0) return HX_ERR_STRIDE;
  if (!aligned16(q) || !aligned16(k) || (reinterpret_cast<uintptr_t>(workspace) & 3u)) return HX_ERR_STRIDE;
  if (workspace_bytes < hx_focal_significance_workspace_bytes(n_images, n_heads, head_dim)) return HX_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == HX_F16)
    return launch_significance<F16>(s1, s2, q, k, (int)n_images, (int)tokens_per_image, (int)skip_leading, (int)n_heads,
                                    (int)head_dim, q_row_stride, k_row_stride, scale, (float*)workspace, s);
  return launch_significance<BF16>(s1, s2, q, k, (int)n_images, (int)tokens_per_image, (int)skip_leading, (int)n_heads,
                                   (int)head_dim, q_row_stride, k_row_stride, scale, (float*)workspace, s);
}

extern "C" int hx_focal_select(int32_t* ids_out, const float* s1, const float* s2, const int32_t* n_keep,
                               int64_t n_images, int64_t N, int strategy, hx_stream stream) {
  if (n_images < 0 || N <= 0 || N > FOCAL_MAX_N) return HX_ERR_SHAPE;
  if (strategy != HX_FOCAL_RANK && strategy != HX_FOCAL_ROW) return HX_ERR_UNSUPPORTED;
  int g = 0;
  if (strategy == HX_FOCAL_ROW) {
    while ((int64_t)g * g < N) ++g;
    if ((int64_t)g * g != N) return HX_ERR_SHAPE;
  }
  if (n_images == 0) return HX_OK;
  if (!ids_out || !s1 || !s2 || !n_keep) return HX_ERR_NULL;
  launcher(focal_select_kernel, dim3((unsigned)n_images), dim3(FOCAL_SEL_THREADS), 0, (hipStream_t)stream)(
      ids_out, s1, s2, n_keep, (int)N, g);
  return check_launch();
}

extern "C" int hx_focal_gather(void* out, const void* tokens, const int32_t* ids, const int32_t* n_keep,
                               int64_t n_images, int64_t N, int64_t hidden, int64_t token_row_stride,
                               int64_t out_row_stride, int dtype, hx_stream stream) {
  const int64_t item = dtype_size(dtype);
  if (item == 0) return HX_ERR_DTYPE;
  if (n_images < 0 || N <= 0 || N > FOCAL_MAX_N || hidden <= 0 || n_images > 65535) return HX_ERR_SHAPE;
  if ((hidden * item) % 16 != 0) return HX_ERR_SHAPE;
  if (n_images == 0) return HX_OK;
  if (!out || !tokens || !ids || !n_keep) return HX_ERR_NULL;
  if (token_row_stride < hidden || out_row_stride < hidden || (token_row_stride * item) % 16 != 0 ||
      (out_row_stride * item) % 16 != 0 || !aligned16(out) || !aligned16(tokens))
    return HX_ERR_STRIDE;
  launcher(focal_gather_kernel, dim3((unsigned)N, (unsigned)n_images), dim3(256), 0, (hipStream_t)stream)(
      (u32x4*)out, (const u32x4*)tokens, ids, n_keep, (int)N, (int)(hidden * item / 16), token_row_stride * item / 16,
      out_row_stride * item / 16);
  return check_launch();
}
