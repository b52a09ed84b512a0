// penalties.hip — greedy sampling under frequency, presence and repetition penalties (include/hydra_hip.h:
// hx_penalized_argmax_rows): steps 1-2 of hydrainfer/sampling/logits_processor.py:65-72 followed by the argmax of
// hydrainfer/model/llama.py:99-104, in one launch and one pass over the logits — no fp32 copy of the row, no gather /
// scatter passes.  Steps 3-5 of the reference (temperature, top-k, top-p) cannot change the largest entry.
//
// One workgroup of 1024 threads per row.  The row's history is a CSR slice of (token id, count) pairs with pairwise
// distinct ids.  The penalised value of a history entry depends only on the RAW logit of its token, so the entries are
// handled first, one per thread: the thread marks its token in an n-bit bitmap in LDS (atomic OR), loads that one
// logit, computes the penalised value in fp32 in the reference's order and keeps the best (value, token) it has seen.
// The scan that follows is argmax_rows_kernel's (norm_rope_act.hip: 16-byte loads, four in flight) and skips every
// element whose bit is set — the bits of a 16-byte piece are one byte of the bitmap, so an untouched piece costs one LDS
// read more than the plain scan.  A workgroup reduction over the threads' candidates ends the row.
//
// Order: hx::arg_better (a NaN first, then the larger value, then the lower index) — a total order, so
// a row with an empty history gives hx_argmax_rows' answer bit for bit, whatever the reduction order.  A row with an
// empty history touches no LDS bitmap at all.
//
// Arithmetic: hx::penalized_value — x - float(c) * f ; - (c > 0 ? p : 0) ; (s < 0) ? s * r : s / r, the reference's
// values bit for bit.
#include <math.h>

#include "hx_common.h"

namespace hx {

#define PEN_THREADS 1024
#define PEN_MAX_N (1 << 18)         // the widest row: a 32 KiB bitmap, the static LDS limit of a launch without attributes

template <typename T>
__global__ __launch_bounds__(PEN_THREADS) void penalized_argmax_rows_kernel(
    int64_t* __restrict__ ids, float* __restrict__ scores_out, const u16* __restrict__ logits, int32_t n, int64_t ld,
    const int32_t* __restrict__ hist_ids, const int32_t* __restrict__ hist_counts, const int32_t* __restrict__ cu_hist,
    int32_t total, const float* __restrict__ penalties) {
  extern __shared__ uint32_t bitmap[];      // (n + 31) / 32 words; not touched by a row without history
  __shared__ float s_v[PEN_THREADS / 64];
  __shared__ int s_i[PEN_THREADS / 64];
  const int64_t row = blockIdx.x;
  const u16* p = logits + row * ld;
  float best = -INFINITY;
  int bi = 0x7fffffff;

  // the row's slice of the history, held inside [0, total] whatever cu_hist says
  int32_t h0 = cu_hist[row], h1 = cu_hist[row + 1];
  h0 = min(max(h0, 0), total);
  h1 = min(max(h1, h0), total);
  const bool masked = h1 > h0;              // the same in every thread of the workgroup
  if (masked) {
    const int words = (n + 31) >> 5;
    for (int w = threadIdx.x; w < words; w += PEN_THREADS) bitmap[w] = 0u;
    __syncthreads();
    const float f = penalties[row * 3], pp = penalties[row * 3 + 1], r = penalties[row * 3 + 2];
    for (int32_t j = h0 + (int32_t)threadIdx.x; j < h1; j += PEN_THREADS) {
      const int32_t t = hist_ids[j];
      float s = __builtin_nanf("");         // an id outside the row: nothing read, no bit set, no candidate
      if (t >= 0 && t < n) {
        atomicOr(&bitmap[t >> 5], 1u << (t & 31));
        s = penalized_value(T::to_float(p[t]), hist_counts[j], f, pp, r);
        if (arg_better(s, t, best, bi)) { best = s; bi = t; }
      }
      if (scores_out) scores_out[j] = s;
    }
    __syncthreads();
  }

  const bool vec = (ld % 8 == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
  if (vec) {
    const int nvec = n / 8;
    // four independent 16-byte loads per thread in flight, like argmax_rows_kernel
    for (int i0 = threadIdx.x; i0 < nvec; i0 += 4 * PEN_THREADS) {
      u16x8 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const u16x8*>(p + (int64_t)min(i0 + PEN_THREADS * u, nvec - 1) * 8);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + PEN_THREADS * u;
        if (i < nvec) {
          // elements 8 i .. 8 i + 7: byte i of the bitmap
          const uint32_t taken = masked ? (bitmap[i >> 2] >> ((i & 3) * 8)) & 0xffu : 0u;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = T::to_float(v[u][e]);
            if (!((taken >> e) & 1u) && arg_better(x, i * 8 + e, best, bi)) { best = x; bi = i * 8 + e; }
          }
        }
      }
    }
    for (int i = nvec * 8 + threadIdx.x; i < n; i += PEN_THREADS) {
      const float x = T::to_float(p[i]);
      const bool taken = masked && ((bitmap[i >> 5] >> (i & 31)) & 1u);
      if (!taken && arg_better(x, i, best, bi)) { best = x; bi = i; }
    }
  } else {
    for (int i = threadIdx.x; i < n; i += PEN_THREADS) {
      const float x = T::to_float(p[i]);
      const bool taken = masked && ((bitmap[i >> 5] >> (i & 31)) & 1u);
      if (!taken && arg_better(x, i, best, bi)) { best = x; bi = i; }
    }
  }
#include "argmax_finish.inc"
}

}  // namespace hx

using namespace hx;

extern "C" int hx_penalized_argmax_rows(int64_t* ids, float* scores_out, const void* logits, int64_t rows, int64_t n,
                                        int64_t ld, const int32_t* hist_ids, const int32_t* hist_counts,
                                        const int32_t* cu_hist, int64_t total, const float* penalties, int dtype,
                                        hx_stream stream) {
  if (rows < 1 || n < 1 || ld < n || n > PEN_MAX_N || rows > 0x7fffffff || total < 0 || total > 0x7fffffff) return HX_ERR_SHAPE;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  if (!ids || !logits || !cu_hist || !penalties || (total > 0 && (!hist_ids || !hist_counts))) return HX_ERR_NULL;
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = total > 0 ? (size_t)((n + 31) / 32) * sizeof(uint32_t) : 0;
  if (dtype == HX_F16)
    hx::launcher(penalized_argmax_rows_kernel<F16>, (unsigned)rows, PEN_THREADS, lds, s)(
        ids, scores_out, (const u16*)logits, (int32_t)n, ld, hist_ids, hist_counts, cu_hist, (int32_t)total, penalties);
  else
    hx::launcher(penalized_argmax_rows_kernel<BF16>, (unsigned)rows, PEN_THREADS, lds, s)(
        ids, scores_out, (const u16*)logits, (int32_t)n, ld, hist_ids, hist_counts, cu_hist, (int32_t)total, penalties);
  return check_launch();
}
