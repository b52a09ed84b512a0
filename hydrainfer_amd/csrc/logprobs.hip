// logprobs.hip — per-token log-probabilities of a decode step (include/hydra_hip.h: hx_logprob_rows): the greedy id of
// hydrainfer/model/llama.py:99-104 together with its log-softmax value and the K most likely alternatives, what
// torch.log_softmax(logits.float(), -1) + torch.topk would give in three more passes and an fp32 copy of the logits.
//
// One workgroup per row.  The row is read from HBM once into LDS (a 32064-wide 16-bit row is 63 KiB of the CU's 160);
// everything after that — the fp32 sum of exponentials and the K selection rounds — reads LDS.  Rows wider than
// LP_LDS_ELEMS stay in global memory (L2) and run the same code from there.
//
// Order.  "a before b" is hx::arg_better: a NaN first, then the larger value, then the lower index — a
// total order, so the first element is hx_argmax_rows' answer whatever the reduction order, and the top-K list (the
// first K elements) has one defined answer even in rows full of exact 16-bit ties.
// Selection.  Each thread owns a fixed subset of the row and keeps its best not-yet-taken element as its candidate.  A
// round is one workgroup reduction over the candidates; only the winner's owner needs a new one (its best element after
// the winner), which its wave finds together.  K rounds cost K reductions, not K passes over the row.
#include <math.h>

#include "hx_common.h"

namespace hx {

#define LP_THREADS 1024
#define LP_MAX_K 20
#define LP_LDS_ELEMS 65536          // 128 KiB of LDS for the row; wider rows are read from global memory
#define LP_NONE 0x7fffffff          // index of "no element": loses to every real element

// f(value, index) for every element this thread owns.  vec: the row is read in 16-byte pieces, thread t owns the pieces
// t, t + 1024, ... and the element nvec * 8 + t of the n % 8 tail; otherwise it owns the elements t, t + 1024, ...
template <typename T, typename F>
__device__ __forceinline__ void lp_for_own(const u16* src, int n, bool vec, F f) {
  if (vec) {
    const int nvec = n >> 3;
    for (int i = threadIdx.x; i < nvec; i += LP_THREADS) {
      const u16x8 v = *reinterpret_cast<const u16x8*>(src + (int64_t)i * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) f(T::to_float(v[e]), i * 8 + e);
    }
    const int i = nvec * 8 + (int)threadIdx.x;
    if (i < n) f(T::to_float(src[i]), i);
  } else {
    for (int i = threadIdx.x; i < n; i += LP_THREADS) f(T::to_float(src[i]), i);
  }
}

// this thread's first element (in the order above) that comes after (wv, wi); (NaN, -1) comes before every element
template <typename T>
__device__ __forceinline__ void lp_candidate(const u16* src, int n, bool vec, float wv, int wi, float& cv, int& ci) {
  float bv = -INFINITY;
  int bi = LP_NONE;
  lp_for_own<T>(src, n, vec, [&](float v, int i) {
    if (arg_better(wv, wi, v, i) && arg_better(v, i, bv, bi)) { bv = v; bi = i; }
  });
  cv = bv;
  ci = bi;
}

// The same for the elements of thread `owner`, by the 64 lanes of a wave together: lane l takes the owner's element
// l % 8 of its pieces l / 8, l / 8 + 8, ... (one element per lane for rows that fit in LDS), lane 0 its tail element;
// every lane returns the owner's first element after (wv, wi).
template <typename T>
__device__ __forceinline__ void lp_candidate_of(const u16* src, int n, bool vec, int owner, float wv, int wi, float& cv,
                                                int& ci) {
  const int lane = threadIdx.x & 63;
  float bv = -INFINITY;
  int bi = LP_NONE;
  auto take = [&](int i) {
    const float v = T::to_float(src[i]);
    if (arg_better(wv, wi, v, i) && arg_better(v, i, bv, bi)) { bv = v; bi = i; }
  };
  if (vec) {
    const int nvec = n >> 3;
    for (int j = owner + LP_THREADS * (lane >> 3); j < nvec; j += 8 * LP_THREADS) take(j * 8 + (lane & 7));
    if (lane == 0 && nvec * 8 + owner < n) take(nvec * 8 + owner);
  } else {
    for (int i = owner + LP_THREADS * lane; i < n; i += 64 * LP_THREADS) take(i);
  }
  wave_first(bv, bi);
  cv = bv;
  ci = bi;
}

// the first of all threads' (v, i), in every thread.  part: 16 floats + 16 ints of LDS, not in use by a reduction that
// other waves may still be reading (the callers alternate two).
__device__ __forceinline__ void lp_block_first(float& v, int& i, float* part_v, int* part_i) {
  wave_first(v, i);
  if ((threadIdx.x & 63) == 0) { part_v[threadIdx.x >> 6] = v; part_i[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = part_v[0];
  i = part_i[0];
#pragma unroll
  for (int k = 1; k < LP_THREADS / 64; ++k) {
    const float ov = part_v[k];
    const int oi = part_i[k];
    if (arg_better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

template <typename T, bool LDS>
__global__ __launch_bounds__(LP_THREADS) void logprob_rows_kernel(int64_t* __restrict__ ids, float* __restrict__ logprobs,
                                                                  int32_t* __restrict__ top_ids,
                                                                  float* __restrict__ top_logprobs,
                                                                  const u16* __restrict__ logits, int32_t n, int64_t ld,
                                                                  int32_t top_k) {
  extern __shared__ __attribute__((aligned(16))) u16 staged[];      // LDS: the row, n elements (rounded up to 8)
  __shared__ float part_v[2][LP_THREADS / 64];
  __shared__ int part_i[2][LP_THREADS / 64];
  __shared__ float part_s[LP_THREADS / 64];
  const int64_t row = blockIdx.x;
  const u16* p = logits + row * ld;
  const bool gvec = (ld % 8 == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);

  const u16* src = p;
  bool vec = gvec;
  if (LDS) {
#include "logprobs_stage.inc"
  }

  // round 0: the greedy id
  float cv;
  int ci;
  lp_candidate<T>(src, n, vec, __builtin_nanf(""), -1, cv, ci);
  float best = cv;
  int bi = ci;
  lp_block_first(best, bi, part_v[0], part_i[0]);

  // log(sum exp(x - best)): per-thread partial sums, a wave tree, sixteen partials in order — every thread holds the
  // same bits.  A NaN in the row makes best, and with it every term, NaN.
  float s = 0.f;
  lp_for_own<T>(src, n, vec, [&](float v, int) { s += expf(v - best); });
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part_s[threadIdx.x >> 6] = s;
  __syncthreads();
  s = part_s[0];
#pragma unroll
  for (int k = 1; k < LP_THREADS / 64; ++k) s += part_s[k];
  const float log_sum = logf(s);

  if (threadIdx.x == 0) {
    ids[row] = bi;
    logprobs[row] = (best - best) - log_sum;
  }
#include "logprobs_rounds.inc"
}

// ---- hx_token_logprob_rows: the score of a GIVEN id per row (prompt log-probabilities) ------------------------------
// The same order, the same selection rounds; in place of the argmax the row's target t = targets[row] is looked up (one
// load) and the rank — the number of elements before (z[t], t) — is counted in the pass that sums the exponentials.
//   top_k == 0 (perplexity, lm-eval): nothing needs the row twice.  ONE pass gives the maximum, the sum (an online
//     (max, sum) pair per thread, merged across the workgroup) and the rank; it reads global memory directly (LDS =
//     false) or the staged row (LDS = true) — profiles/token_logprob_rows.md has both, the launcher keeps the faster.
//   top_k > 0: the row is staged, round 0 finds the maximum, and the sum is logprob_rows_kernel's term for term, so the
//     top list equals its bit for bit; then the same rounds.
// A row whose target lies outside 0 .. n-1 is not scored: sentinels, and the workgroup leaves before reading the row.

// (m, s) += one element: m the largest value so far (-inf: none), s = sum exp(v - m) over the values > -inf.  One
// exponential per element; never (-inf) - (-inf): a -inf adds nothing.  A NaN element makes s NaN for good; a +inf leaves
// m = +inf, which the caller turns into s = NaN (exp(inf - inf)), as the two-pass form gives.
__device__ __forceinline__ void tlp_take(float& m, float& s, float v) {
  const float e = __expf(-fabsf(v - m));
  const bool bigger = v > m;
  s = bigger ? s * e + 1.f : s + (v == -INFINITY ? 0.f : e);
  m = bigger ? v : m;
}

// (m, s) += another pair
__device__ __forceinline__ void tlp_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  const float ref = nm == -INFINITY ? 0.f : nm;     // both empty: exp(-inf - 0) = 0 twice
  s = s * __expf(m - ref) + os * __expf(om - ref);
  m = nm;
}

template <typename T, bool LDS>
__global__ __launch_bounds__(LP_THREADS) void token_logprob_rows_kernel(float* __restrict__ logprobs, int32_t* __restrict__ ranks,
                                                                        int32_t* __restrict__ top_ids,
                                                                        float* __restrict__ top_logprobs,
                                                                        const u16* __restrict__ logits,
                                                                        const int32_t* __restrict__ targets, int32_t n,
                                                                        int64_t ld, int32_t top_k) {
  extern __shared__ __attribute__((aligned(16))) u16 staged[];      // LDS: the row, n elements (rounded up to 8)
  __shared__ float part_v[2][LP_THREADS / 64];
  __shared__ int part_i[2][LP_THREADS / 64];
  __shared__ float part_m[LP_THREADS / 64], part_s[LP_THREADS / 64];
  __shared__ int part_c[LP_THREADS / 64];
  const int64_t row = blockIdx.x;
  const int t = targets[row];
  if (t < 0 || t >= n) {                                             // a row that only samples: nothing of it is read
    if (threadIdx.x == 0) {
      logprobs[row] = __builtin_nanf("");
      ranks[row] = -1;
    }
    if ((int)threadIdx.x < top_k) {
      top_ids[row * top_k + threadIdx.x] = -1;
      top_logprobs[row * top_k + threadIdx.x] = -INFINITY;
    }
    return;
  }
  const u16* p = logits + row * ld;
  const bool gvec = (ld % 8 == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
  const float zt = T::to_float(p[t]);

  const u16* src = p;
  bool vec = gvec;
  if (LDS) {
#include "logprobs_stage.inc"
  }

  float m, s = 0.f;
  int before = 0;
  float cv = 0.f;                               // this thread's candidate and round 0's winner, for the rounds
  int ci = LP_NONE, bi = LP_NONE;
  if (top_k == 0) {
    // the one pass: maximum, sum of exponentials, rank
    m = -INFINITY;
    auto take = [&](float v, int i) {
      tlp_take(m, s, v);
      before += arg_better(v, i, zt, t) ? 1 : 0;
    };
    if (!LDS && vec) {
      // from global memory: four independent 16-byte loads per thread in flight, as in the staging loop (which
      // elements a thread takes does not matter here: no selection round follows)
      const int nvec = n >> 3;
      for (int i0 = threadIdx.x; i0 < nvec; i0 += 4 * LP_THREADS) {
        u16x8 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const u16x8*>(p + (int64_t)min(i0 + LP_THREADS * u, nvec - 1) * 8);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + LP_THREADS * u;
          if (i < nvec) {
#pragma unroll
            for (int e = 0; e < 8; ++e) take(T::to_float(v[u][e]), i * 8 + e);
          }
        }
      }
      const int i = nvec * 8 + (int)threadIdx.x;
      if (i < n) take(T::to_float(p[i]), i);
    } else {
      lp_for_own<T>(src, n, vec, take);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float om = __shfl_xor(m, off, 64);
      const float os = __shfl_xor(s, off, 64);
      tlp_merge(m, s, om, os);
      before += __shfl_xor(before, off, 64);
    }
    // sixteen partials, merged in order by every thread
    if ((threadIdx.x & 63) == 0) {
      part_m[threadIdx.x >> 6] = m;
      part_s[threadIdx.x >> 6] = s;
      part_c[threadIdx.x >> 6] = before;
    }
    __syncthreads();
    m = part_m[0];
    s = part_s[0];
    before = part_c[0];
#pragma unroll
    for (int k = 1; k < LP_THREADS / 64; ++k) {
      tlp_merge(m, s, part_m[k], part_s[k]);
      before += part_c[k];
    }
    if (m == INFINITY) s = __builtin_nanf("");
  } else {
    // round 0 (the greedy id) and logprob_rows_kernel's sum, term for term — the top list comes out bit-identical to
    // its — with the rank counted in the same pass over the staged row
    lp_candidate<T>(src, n, vec, __builtin_nanf(""), -1, cv, ci);
    m = cv;
    bi = ci;
    lp_block_first(m, bi, part_v[0], part_i[0]);
    const float best = m;
    lp_for_own<T>(src, n, vec, [&](float v, int i) {
      s += expf(v - best);
      before += arg_better(v, i, zt, t) ? 1 : 0;
    });
    s = wave_sum(s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
    if ((threadIdx.x & 63) == 0) {
      part_s[threadIdx.x >> 6] = s;
      part_c[threadIdx.x >> 6] = before;
    }
    __syncthreads();
    s = part_s[0];
    before = part_c[0];
#pragma unroll
    for (int k = 1; k < LP_THREADS / 64; ++k) {
      s += part_s[k];
      before += part_c[k];
    }
  }
  const float log_sum = logf(s);
  if (threadIdx.x == 0) {
    logprobs[row] = (zt - m) - log_sum;
    ranks[row] = before;
  }
  if (top_k == 0) return;

  const float best = m;
#include "logprobs_rounds.inc"
}

}  // namespace hx

using namespace hx;

// bytes of LDS for a staged row of n elements
static size_t lp_row_bytes(int64_t n) { return (size_t)((n + 7) / 8 * 8) * sizeof(u16); }

template <typename T>
static int launch_logprob_rows(int64_t* ids, float* logprobs, int32_t* top_ids, float* top_logprobs, const void* logits,
                               int64_t rows, int64_t n, int64_t ld, int top_k, hipStream_t s) {
  const bool staged = n <= LP_LDS_ELEMS;
  return launch_lds(staged ? logprob_rows_kernel<T, true> : logprob_rows_kernel<T, false>, (unsigned)rows, LP_THREADS,
                    staged ? lp_row_bytes(n) : 0, s, ids, logprobs, top_ids, top_logprobs, (const u16*)logits, (int32_t)n, ld,
                    top_k);
}

extern "C" int hx_logprob_rows(int64_t* ids, float* logprobs, int32_t* top_ids, float* top_logprobs, const void* logits,
                               int64_t rows, int64_t n, int64_t ld, int top_k, int dtype, hx_stream stream) {
  if (rows < 1 || n < 1 || ld < n || n > 0x7ffffff0 || rows > 0x7fffffff) return HX_ERR_SHAPE;
  if (top_k < 0 || top_k > LP_MAX_K) return HX_ERR_SHAPE;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  if (!ids || !logprobs || !logits || (top_k > 0 && (!top_ids || !top_logprobs))) return HX_ERR_NULL;
  return (dtype == HX_F16 ? launch_logprob_rows<F16> : launch_logprob_rows<BF16>)(ids, logprobs, top_ids, top_logprobs, logits,
                                                                                   rows, n, ld, top_k, (hipStream_t)stream);
}

// form: 0 — the form kept per top_k class (profiles/token_logprob_rows.md); 1 — the pass straight from global memory;
// 2 — the row staged in LDS (rows wider than LP_LDS_ELEMS: form 1 whatever is asked)
template <typename T>
static int launch_token_logprob_rows(float* logprobs, int32_t* ranks, int32_t* top_ids, float* top_logprobs, const void* logits,
                                     const int32_t* targets, int64_t rows, int64_t n, int64_t ld, int top_k, int form,
                                     hipStream_t s) {
  const bool staged = n <= LP_LDS_ELEMS && (form == 2 || (form == 0 && top_k > 0));
  return launch_lds(staged ? token_logprob_rows_kernel<T, true> : token_logprob_rows_kernel<T, false>, (unsigned)rows,
                    LP_THREADS, staged ? lp_row_bytes(n) : 0, s, logprobs, ranks, top_ids, top_logprobs, (const u16*)logits,
                    targets, (int32_t)n, ld, top_k);
}

extern "C" int hx_token_logprob_rows_ex(float* logprobs, int32_t* ranks, int32_t* top_ids, float* top_logprobs,
                                        const void* logits, const int32_t* targets, int64_t rows, int64_t n, int64_t ld,
                                        int top_k, int dtype, int form, hx_stream stream) {
  if (rows < 1 || n < 1 || ld < n || n > 0x7ffffff0 || rows > 0x7fffffff) return HX_ERR_SHAPE;
  if (top_k < 0 || top_k > LP_MAX_K || form < 0 || form > 2) return HX_ERR_SHAPE;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  if (!logprobs || !ranks || !logits || !targets || (top_k > 0 && (!top_ids || !top_logprobs))) return HX_ERR_NULL;
  return (dtype == HX_F16 ? launch_token_logprob_rows<F16> : launch_token_logprob_rows<BF16>)(
      logprobs, ranks, top_ids, top_logprobs, logits, targets, rows, n, ld, top_k, form, (hipStream_t)stream);
}

extern "C" int hx_token_logprob_rows(float* logprobs, int32_t* ranks, int32_t* top_ids, float* top_logprobs,
                                     const void* logits, const int32_t* targets, int64_t rows, int64_t n, int64_t ld,
                                     int top_k, int dtype, hx_stream stream) {
  return hx_token_logprob_rows_ex(logprobs, ranks, top_ids, top_logprobs, logits, targets, rows, n, ld, top_k, dtype, 0, stream);
}
