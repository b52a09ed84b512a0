// sampling.hip — seeded sampled decoding (include/hydra_hip.h: hx_sample_rows): steps 1-5 of
// hydrainfer/sampling/logits_processor.py:49-93 (penalties, temperature, top-k, top-p) and the draw, which the reference
// never makes (its models end in torch.argmax), in one launch behind the logits.
//
// One workgroup of 1024 threads per row.  The row is read from HBM once, as fp32 into LDS; a row's history entries are
// penalised there in place, one per thread (hx::penalized_value, so a T = 0 row gives
// hx_penalized_argmax_rows' id bit for bit).  Thread t then OWNS the contiguous elements t * chunk .. t * chunk + chunk - 1
// (chunk = ceil(n / 1024) made odd: the threads' LDS reads fall on different banks) and holds their z = s / T and
// e = expf(z - m) in registers for the rest of the kernel: up to SMP_CHUNK of each.  Contiguous ownership is what makes
// the draw an index-order scan: per-thread sums, one workgroup scan over the 1024 partial sums, and the one thread whose
// range holds the crossing walks its own elements.
//
// Selection, over a monotone 32-bit key of z.  v_K (the K-th largest z) by a RADIX SELECT: four passes of 8 bits, each an
// LDS histogram of integer counts (atomic adds from the registers) and a suffix scan by one wave.  v* (the top-p cut) by
// BISECTION: at most 32 rounds, a round summing e over {z > v} in fp32 per thread, then a wave tree, then the same tree
// over the sixteen wave sums — every thread holds the same bits, the sum does not depend on any order of arrival, and it
// is monotone in the set (the same tree with zeros for the elements left out), so the search has one answer and it is a
// value of the row.  Float sums in an atomically built histogram would depend on the order of the additions: the same
// call could then give two tokens.  Measured, 64 rows x 32064: top-k by radix 12 us, by bisection over counts 27 us
// ("Sampled decoding").  A row with top_k outside 1 .. n - 1 and top_p >= 1 runs neither search.
//
// Order of a greedy row: hx::arg_better (a NaN first, then the larger value, then the lower index).
//
// hx_sample_rows_constrained (logit_bias, min_tokens, min_p) is the same body — sampling_body.inc, included into both
// kernels — with two more steps: a row's (token, bias) entries are added to the staged row ahead of the penalties (1b),
// and min_p raises the top-k cut to the smallest z whose e reaches it, by one more block minimum over the registers (4b).
//
// hx_sample_rows_logprobs is the constrained body with a seventh step: when the draw is done a thread still holds its z,
// the block m, the cut and Z_S, so the log-probability of the chosen token under the distribution it was chosen from is
// (z - m) - logf(Z_S), and the K most likely alternatives are K block-argmax rounds over the registers — no second read
// of the row, no second launch.  A greedy row that is scored does not leave early: T' = 1 and S is the whole row.
//
// hx_sample_rows_masked (allowed_token_ids, guided_choice) is the scored body with a step 1a: a row that names one of
// the launch's token bitmasks (32 tokens per word, 1 = allowed) gets -inf at every token whose bit is clear, in the staged
// row and ahead of everything else, from one read of the mask's 4 KB — no LDS beyond the row's own.
//
// hx_sample_rows_resident_penalized is the resident body with a step 2L: a row's history is a prefix of its slot of a
// RESIDENT token log (tokens with repeats, appended by this kernel itself), counted per distinct token in the row's own
// LDS words (integer atomics) and penalised by hx::penalized_value in one rounding — what a captured decode step needs
// to penalise without the host ("Penalties from the captured step").
#include <math.h>

#include "hx_common.h"

namespace hx {

#define SMP_THREADS 1024
#define SMP_CHUNK 35                                    // elements a thread owns at most (odd)
#define SAMPLE_MAX_N HX_SAMPLE_MAX_N                     // 35840: 140 KiB of fp32 in LDS
static_assert(SAMPLE_MAX_N == SMP_THREADS * SMP_CHUNK, "the widest row is what 1024 threads own");
#define SMP_WAVES (SMP_THREADS / 64)

// ascending key of a non-NaN float (-0 and +0 share +0's key) and the value of a key
__device__ __forceinline__ uint32_t smp_key(float z) {
  const uint32_t b = __float_as_uint(z + 0.f);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float smp_val(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// word 0 of Philox4x32-10(counter = (offset_lo, offset_hi, 0, 0), key = (seed_lo, seed_hi))
__device__ __forceinline__ uint32_t smp_philox0(uint32_t c0, uint32_t c1, uint32_t k0, uint32_t k1) {
  uint32_t c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// the sum of all threads' s, the same bits in every thread: a wave tree, then the same tree over the sixteen wave sums
// (every wave runs it on the same sixteen values).  part: 16 words of LDS not in use by a reduction that other waves may still be reading (the callers alternate two).
__device__ __forceinline__ float smp_block_sum(float s, float* part) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  s = part[threadIdx.x & (SMP_WAVES - 1)];
#pragma unroll
  for (int off = SMP_WAVES / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// what the body names for its scores, in the kernels that give none (SCORED false: no statement that reads them is compiled)
#define SMP_NO_SCORES                                                                                  \
  constexpr bool SCORED = false;                                                                       \
  float* const logprobs = nullptr; int32_t* const top_ids = nullptr; float* const top_logprobs = nullptr; \
  const int32_t score_k = 0; const int32_t* const want = nullptr;
// and for its masks, in the kernels that take none (MASKED false: no statement that reads them is compiled)
#define SMP_NO_MASK                                                                                    \
  constexpr bool MASKED = false;                                                                       \
  const uint32_t* const allow_words = nullptr; const int32_t n_masks = 0; const int32_t* const mask_row = nullptr;

// and for its token log, in the kernels that keep none (LOGGED false: no statement that reads them is compiled)
#define SMP_NO_LOG                                                                                     \
  constexpr bool LOGGED = false;                                                                       \
  const int32_t* const penalty_params = nullptr; int32_t* const token_log = nullptr;                   \
  const int32_t log_slots = 0, log_cap = 0;
// log entries a thread holds in step 2L: 1024 threads x 4 = HX_SAMPLE_LOG_MAX
#define SMP_LOG_PER_THREAD 4
static_assert(HX_SAMPLE_LOG_MAX == SMP_THREADS * SMP_LOG_PER_THREAD, "the longest log prefix is what 1024 threads hold");

// the Philox counter of a row, as the body names it: in the four kernels that take the offset itself, words [6] and [7]
// of the row's record (`rec`, the body's own)
#define SMP_OFFSET_LO rec[6]
#define SMP_OFFSET_HI rec[7]

template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_kernel(
    int64_t* __restrict__ ids, float* __restrict__ cut_out, float* __restrict__ u_out, const u16* __restrict__ logits,
    int32_t n, int64_t ld, const int32_t* __restrict__ hist_ids, const int32_t* __restrict__ hist_counts,
    const int32_t* __restrict__ cu_hist, int32_t total, const float* __restrict__ penalties,
    const uint32_t* __restrict__ sample_params) {
  constexpr bool CONSTRAINED = false;
  SMP_NO_SCORES
  SMP_NO_MASK
  SMP_NO_LOG
  const int32_t* const bias_ids = nullptr; const float* const bias_values = nullptr; const int32_t* const cu_bias = nullptr;
  const int32_t bias_total = 0;
#include "sampling_body.inc"
}

// hx_sample_rows_constrained: the same body with a per-row bias table added to the staged row ahead of the penalties
// and the min_p cut (record word 3) between top-k and top-p.  The body is INCLUDED, as attn_decode_body.inc is (see
// attn_decode.hip for why not a __forceinline__ function): sample_rows_kernel keeps its device code byte for byte.
template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_constrained_kernel(
    int64_t* __restrict__ ids, float* __restrict__ cut_out, float* __restrict__ u_out, const u16* __restrict__ logits,
    int32_t n, int64_t ld, const int32_t* __restrict__ hist_ids, const int32_t* __restrict__ hist_counts,
    const int32_t* __restrict__ cu_hist, int32_t total, const float* __restrict__ penalties,
    const uint32_t* __restrict__ sample_params, const int32_t* __restrict__ bias_ids,
    const float* __restrict__ bias_values, const int32_t* __restrict__ cu_bias, int32_t bias_total) {
  constexpr bool CONSTRAINED = true;
  SMP_NO_SCORES
  SMP_NO_MASK
  SMP_NO_LOG
#include "sampling_body.inc"
}

// hx_sample_rows_logprobs: the constrained body with step 7 — the log-probability of the row's id under the distribution
// it was chosen from, and the K most likely alternatives of that distribution, out of the z and Z_S the draw has in
// registers.  SCORED is false in the two kernels above, which keep their device code byte for byte.
template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_logprobs_kernel(
    int64_t* __restrict__ ids, float* __restrict__ cut_out, float* __restrict__ u_out, const u16* __restrict__ logits,
    int32_t n, int64_t ld, const int32_t* __restrict__ hist_ids, const int32_t* __restrict__ hist_counts,
    const int32_t* __restrict__ cu_hist, int32_t total, const float* __restrict__ penalties,
    const uint32_t* __restrict__ sample_params, const int32_t* __restrict__ bias_ids,
    const float* __restrict__ bias_values, const int32_t* __restrict__ cu_bias, int32_t bias_total,
    float* __restrict__ logprobs, int32_t* __restrict__ top_ids, float* __restrict__ top_logprobs, int32_t score_k,
    const int32_t* __restrict__ want) {
  constexpr bool CONSTRAINED = true;
  constexpr bool SCORED = true;
  SMP_NO_MASK
  SMP_NO_LOG
#include "sampling_body.inc"
}

// hx_sample_rows_masked: the scored body with step 1a — a row that names a mask has every element whose bit is clear set
// to -inf in the staged row, ahead of the bias table; everything after that is the body as it stands, which handles -inf
// bans already.  Scoring is optional per launch here (logprobs null: no row is scored).  MASKED is false in the three
// kernels above, which keep their device code byte for byte.
template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_masked_kernel(
    int64_t* __restrict__ ids, float* __restrict__ cut_out, float* __restrict__ u_out, const u16* __restrict__ logits,
    int32_t n, int64_t ld, const int32_t* __restrict__ hist_ids, const int32_t* __restrict__ hist_counts,
    const int32_t* __restrict__ cu_hist, int32_t total, const float* __restrict__ penalties,
    const uint32_t* __restrict__ sample_params, const int32_t* __restrict__ bias_ids,
    const float* __restrict__ bias_values, const int32_t* __restrict__ cu_bias, int32_t bias_total,
    float* __restrict__ logprobs, int32_t* __restrict__ top_ids, float* __restrict__ top_logprobs, int32_t score_k,
    const int32_t* __restrict__ want, const uint32_t* __restrict__ allow_words, int32_t n_masks,
    const int32_t* __restrict__ mask_row) {
  constexpr bool CONSTRAINED = true;
  constexpr bool SCORED = true;
  constexpr bool MASKED = true;
  SMP_NO_LOG
#include "sampling_body.inc"
}

// hx_sample_rows_resident: sample_rows_kernel without a history (total is the constant 0: step 2 is not compiled), for
// records that STAY on the device across the steps of a captured decode graph.  Words [6] and [7] are a 64-bit
// offset_base and the counter is offset_base + positions[row], modulo 2^64 — a request's generated-token count minus its
// position is constant in decode, so no word of its record changes from step to step and the launch changes no state.
#undef SMP_OFFSET_LO
#undef SMP_OFFSET_HI
__device__ __forceinline__ uint64_t smp_resident_offset(const uint32_t* rec, int32_t position) {
  return (((uint64_t)rec[7] << 32) | (uint64_t)rec[6]) + (uint64_t)(int64_t)position;   // (sign-extended: a carry or a borrow)
}
#define SMP_OFFSET_LO ((uint32_t)smp_resident_offset(rec, positions[row]))
#define SMP_OFFSET_HI ((uint32_t)(smp_resident_offset(rec, positions[row]) >> 32))

template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_resident_kernel(
    int64_t* __restrict__ ids, float* __restrict__ cut_out, float* __restrict__ u_out, const u16* __restrict__ logits,
    int32_t n, int64_t ld, const uint32_t* __restrict__ sample_params, const int32_t* __restrict__ positions) {
  constexpr bool CONSTRAINED = false;
  SMP_NO_SCORES
  SMP_NO_MASK
  SMP_NO_LOG
  const int32_t* const bias_ids = nullptr; const float* const bias_values = nullptr; const int32_t* const cu_bias = nullptr;
  const int32_t bias_total = 0;
  const int32_t* const hist_ids = nullptr; const int32_t* const hist_counts = nullptr; const int32_t* const cu_hist = nullptr;
  const float* const penalties = nullptr;
  constexpr int32_t total = 0;
#include "sampling_body.inc"
}

// hx_sample_rows_resident_penalized: the resident kernel with step 2L — a row that names a slot of the resident token log
// is penalised over the slot's first L words (L the row's offset) and appends its id as word L.  LOGGED is false in the
// five kernels above, which keep their device code byte for byte.
template <typename T>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_resident_penalized_kernel(
    int64_t* __restrict__ ids, float* __restrict__ cut_out, float* __restrict__ u_out, const u16* __restrict__ logits,
    int32_t n, int64_t ld, const uint32_t* __restrict__ sample_params, const int32_t* __restrict__ positions,
    const int32_t* __restrict__ penalty_params, int32_t* token_log, int32_t log_slots, int32_t log_cap) {
  constexpr bool CONSTRAINED = false;
  constexpr bool LOGGED = true;
  SMP_NO_SCORES
  SMP_NO_MASK
  const int32_t* const bias_ids = nullptr; const float* const bias_values = nullptr; const int32_t* const cu_bias = nullptr;
  const int32_t bias_total = 0;
  const int32_t* const hist_ids = nullptr; const int32_t* const hist_counts = nullptr; const int32_t* const cu_hist = nullptr;
  const float* const penalties = nullptr;
  constexpr int32_t total = 0;
#include "sampling_body.inc"
}
#undef SMP_OFFSET_LO
#undef SMP_OFFSET_HI

}  // namespace hx

using namespace hx;

// What the four entries are called with.  hx_sample_rows comes with no bias table (bias_total 0); only
// hx_sample_rows_logprobs and hx_sample_rows_masked fill the score fields, only the latter the mask fields.
struct SampleArgs {
  int64_t* ids; float* cut_out; float* u_out;
  const void* logits; int64_t rows, n, ld;
  const int32_t* hist_ids; const int32_t* hist_counts; const int32_t* cu_hist; int64_t total; const float* penalties;
  const int32_t* bias_ids; const float* bias_values; const int32_t* cu_bias; int64_t bias_total;
  const void* sample_params;
  float* logprobs; int32_t* top_ids; float* top_logprobs; int top_k; const int32_t* want;
  int dtype; hipStream_t stream;
  const uint32_t* allow_words = nullptr; int64_t n_masks = 0; const int32_t* mask_row = nullptr;
};
enum SampleKernel { SMP_PLAIN, SMP_CONSTRAINED, SMP_SCORED, SMP_MASKED };

// The argument checks: top_k's range in front of everything for the scored entry, then shape, dtype, null pointers.  The
// masked entry is scored when it comes with logprobs: the scored entry's rules hold then, none of them otherwise.
static int sample_rows_check(SampleKernel which, const SampleArgs& a) {
  const bool scored = which == SMP_SCORED || (which == SMP_MASKED && a.logprobs);
  if (scored && (a.top_k < 0 || a.top_k > 20)) return HX_ERR_SHAPE;
  if (which == SMP_MASKED && (a.n_masks < 0 || a.n_masks > 0x7fffffff)) return HX_ERR_SHAPE;
  if (a.rows < 1 || a.n < 1 || a.ld < a.n || a.n > SAMPLE_MAX_N || a.rows > 0x7fffffff || a.total < 0 ||
      a.total > 0x7fffffff || a.bias_total < 0 || a.bias_total > 0x7fffffff)
    return HX_ERR_SHAPE;
  if (a.dtype != HX_F16 && a.dtype != HX_BF16) return HX_ERR_DTYPE;
  if (!a.ids || !a.logits || !a.sample_params ||
      (a.total > 0 && (!a.hist_ids || !a.hist_counts || !a.cu_hist || !a.penalties)) ||
      (a.bias_total > 0 && (!a.bias_ids || !a.bias_values || !a.cu_bias)))
    return HX_ERR_NULL;
  if (scored && (!a.logprobs || (a.top_k > 0 && (!a.top_ids || !a.top_logprobs)))) return HX_ERR_NULL;
  if (which == SMP_MASKED && (!a.mask_row || (a.n_masks > 0 && !a.allow_words))) return HX_ERR_NULL;
  return HX_OK;
}

// One workgroup per row, the row as fp32 in dynamic LDS (wider than 12288 elements: more than a launch gets unasked).
template <typename T>
static int launch_sample_rows(SampleKernel which, const SampleArgs& a) {
  const size_t lds = (size_t)((a.n + 7) / 8 * 8) * sizeof(float);
  const unsigned rows = (unsigned)a.rows;
  const u16* logits = (const u16*)a.logits;
  const uint32_t* params = (const uint32_t*)a.sample_params;
  const int32_t n = (int32_t)a.n, total = (int32_t)a.total, bias_total = (int32_t)a.bias_total;
  if (which == SMP_PLAIN)
    return launch_lds(sample_rows_kernel<T>, rows, SMP_THREADS, lds, a.stream, a.ids, a.cut_out, a.u_out, logits, n, a.ld,
                      a.hist_ids, a.hist_counts, a.cu_hist, total, a.penalties, params);
  if (which == SMP_CONSTRAINED)
    return launch_lds(sample_rows_constrained_kernel<T>, rows, SMP_THREADS, lds, a.stream, a.ids, a.cut_out, a.u_out, logits,
                      n, a.ld, a.hist_ids, a.hist_counts, a.cu_hist, total, a.penalties, params, a.bias_ids, a.bias_values,
                      a.cu_bias, bias_total);
  if (which == SMP_SCORED)
    return launch_lds(sample_rows_logprobs_kernel<T>, rows, SMP_THREADS, lds, a.stream, a.ids, a.cut_out, a.u_out, logits, n,
                      a.ld, a.hist_ids, a.hist_counts, a.cu_hist, total, a.penalties, params, a.bias_ids, a.bias_values,
                      a.cu_bias, bias_total, a.logprobs, a.top_ids, a.top_logprobs, (int32_t)a.top_k, a.want);
  const int32_t score_k = a.logprobs ? (int32_t)a.top_k : 0;      // (unscored: top_ids, top_logprobs and want are not read)
  return launch_lds(sample_rows_masked_kernel<T>, rows, SMP_THREADS, lds, a.stream, a.ids, a.cut_out, a.u_out, logits, n,
                    a.ld, a.hist_ids, a.hist_counts, a.cu_hist, total, a.penalties, params, a.bias_ids, a.bias_values,
                    a.cu_bias, bias_total, a.logprobs, a.top_ids, a.top_logprobs, score_k, a.logprobs ? a.want : nullptr,
                    a.allow_words, (int32_t)a.n_masks, a.mask_row);
}

// All four entries: the argument checks, then the launch by dtype.
static int sample_rows(SampleKernel which, const SampleArgs& a) {
  const int rc = sample_rows_check(which, a);
  if (rc != HX_OK) return rc;
  return a.dtype == HX_F16 ? launch_sample_rows<F16>(which, a) : launch_sample_rows<BF16>(which, a);
}

// The resident entry: hx_sample_rows' checks with total == 0, and the positions.  A row wider than 12288 elements needs
// the kernel's dynamic-LDS limit raised, which is no stream operation and may not happen while `stream` is being
// captured: it is raised — to the widest row, so one call serves every n — on every launch outside a capture, and a
// capture relies on such a launch having gone before (GraphedDecoder._capture runs the step twice first).
template <typename T>
static int launch_sample_rows_resident(const SampleArgs& a, const int32_t* positions) {
  const size_t lds = (size_t)((a.n + 7) / 8 * 8) * sizeof(float);
  if (lds > 48 * 1024) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(a.stream, &capturing);
    if (e != hipSuccess) return hip_rc(e);
    if (capturing == hipStreamCaptureStatusNone) {
      e = hipFuncSetAttribute((const void*)sample_rows_resident_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(SAMPLE_MAX_N * sizeof(float)));
      if (e != hipSuccess) return hip_rc(e);
    }
  }
  launcher(sample_rows_resident_kernel<T>, (unsigned)a.rows, SMP_THREADS, lds, a.stream)(
      a.ids, a.cut_out, a.u_out, (const u16*)a.logits, (int32_t)a.n, a.ld, (const uint32_t*)a.sample_params, positions);
  return check_launch();
}

extern "C" int hx_sample_rows_resident(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows,
                                       int64_t n, int64_t ld, const void* sample_params, const int32_t* positions,
                                       int dtype, hx_stream stream) {
  const SampleArgs a{ids, cut_out, u_out, logits, rows, n, ld, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                     nullptr, 0, sample_params, nullptr, nullptr, nullptr, 0, nullptr, dtype, (hipStream_t)stream};
  const int rc = sample_rows_check(SMP_PLAIN, a);
  if (rc != HX_OK) return rc;
  if (!positions) return HX_ERR_NULL;
  return dtype == HX_F16 ? launch_sample_rows_resident<F16>(a, positions) : launch_sample_rows_resident<BF16>(a, positions);
}

// The penalised resident entry: the resident entry's checks, the log's, and the same rule for the dynamic-LDS limit (the
// log takes no LDS: the launch asks for the row's alone).
template <typename T>
static int launch_sample_rows_resident_penalized(const SampleArgs& a, const int32_t* positions, const int32_t* penalty_params,
                                                 int32_t* token_log, int64_t log_slots, int64_t log_cap) {
  const size_t lds = (size_t)((a.n + 7) / 8 * 8) * sizeof(float);
  if (lds > 48 * 1024) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(a.stream, &capturing);
    if (e != hipSuccess) return hip_rc(e);
    if (capturing == hipStreamCaptureStatusNone) {
      e = hipFuncSetAttribute((const void*)sample_rows_resident_penalized_kernel<T>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SAMPLE_MAX_N * sizeof(float)));
      if (e != hipSuccess) return hip_rc(e);
    }
  }
  launcher(sample_rows_resident_penalized_kernel<T>, (unsigned)a.rows, SMP_THREADS, lds, a.stream)(
      a.ids, a.cut_out, a.u_out, (const u16*)a.logits, (int32_t)a.n, a.ld, (const uint32_t*)a.sample_params, positions,
      penalty_params, token_log, (int32_t)(log_slots > 0x7fffffff ? 0x7fffffff : log_slots), (int32_t)log_cap);
  return check_launch();
}

extern "C" int hx_sample_rows_resident_penalized(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows,
                                                 int64_t n, int64_t ld, const void* sample_params, const int32_t* positions,
                                                 const void* penalty_params, int32_t* token_log, int64_t log_slots,
                                                 int64_t log_cap, int dtype, hx_stream stream) {
  const SampleArgs a{ids, cut_out, u_out, logits, rows, n, ld, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                     nullptr, 0, sample_params, nullptr, nullptr, nullptr, 0, nullptr, dtype, (hipStream_t)stream};
  if (log_slots < 1 || log_cap < 1 || log_cap > HX_SAMPLE_LOG_MAX) return HX_ERR_SHAPE;
  const int rc = sample_rows_check(SMP_PLAIN, a);
  if (rc != HX_OK) return rc;
  if (!positions || !penalty_params || !token_log) return HX_ERR_NULL;
  return dtype == HX_F16
             ? launch_sample_rows_resident_penalized<F16>(a, positions, (const int32_t*)penalty_params, token_log, log_slots, log_cap)
             : launch_sample_rows_resident_penalized<BF16>(a, positions, (const int32_t*)penalty_params, token_log, log_slots, log_cap);
}

extern "C" int hx_sample_rows(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows, int64_t n,
                              int64_t ld, const int32_t* hist_ids, const int32_t* hist_counts, const int32_t* cu_hist,
                              int64_t total, const float* penalties, const void* sample_params, int dtype,
                              hx_stream stream) {
  return sample_rows(SMP_PLAIN, {ids, cut_out, u_out, logits, rows, n, ld, hist_ids, hist_counts, cu_hist, total, penalties,
                                 nullptr, nullptr, nullptr, 0, sample_params, nullptr, nullptr, nullptr, 0, nullptr, dtype,
                                 (hipStream_t)stream});
}

extern "C" int hx_sample_rows_constrained(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows,
                                          int64_t n, int64_t ld, const int32_t* hist_ids, const int32_t* hist_counts,
                                          const int32_t* cu_hist, int64_t total, const float* penalties,
                                          const int32_t* bias_ids, const float* bias_values, const int32_t* cu_bias,
                                          int64_t bias_total, const void* sample_params, int dtype, hx_stream stream) {
  return sample_rows(SMP_CONSTRAINED, {ids, cut_out, u_out, logits, rows, n, ld, hist_ids, hist_counts, cu_hist, total,
                                       penalties, bias_ids, bias_values, cu_bias, bias_total, sample_params, nullptr, nullptr,
                                       nullptr, 0, nullptr, dtype, (hipStream_t)stream});
}

extern "C" int hx_sample_rows_logprobs(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows, int64_t n,
                                       int64_t ld, const int32_t* hist_ids, const int32_t* hist_counts,
                                       const int32_t* cu_hist, int64_t total, const float* penalties,
                                       const int32_t* bias_ids, const float* bias_values, const int32_t* cu_bias,
                                       int64_t bias_total, const void* sample_params, float* logprobs, int32_t* top_ids,
                                       float* top_logprobs, int top_k, const int32_t* want, int dtype, hx_stream stream) {
  return sample_rows(SMP_SCORED, {ids, cut_out, u_out, logits, rows, n, ld, hist_ids, hist_counts, cu_hist, total, penalties,
                                  bias_ids, bias_values, cu_bias, bias_total, sample_params, logprobs, top_ids, top_logprobs,
                                  top_k, want, dtype, (hipStream_t)stream});
}

extern "C" int hx_sample_rows_masked(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows, int64_t n,
                                     int64_t ld, const int32_t* hist_ids, const int32_t* hist_counts, const int32_t* cu_hist,
                                     int64_t total, const float* penalties, const int32_t* bias_ids, const float* bias_values,
                                     const int32_t* cu_bias, int64_t bias_total, const void* sample_params, float* logprobs,
                                     int32_t* top_ids, float* top_logprobs, int top_k, const int32_t* want,
                                     const uint32_t* allow_words, int64_t n_masks, const int32_t* mask_row, int dtype,
                                     hx_stream stream) {
  return sample_rows(SMP_MASKED, {ids, cut_out, u_out, logits, rows, n, ld, hist_ids, hist_counts, cu_hist, total, penalties,
                                  bias_ids, bias_values, cu_bias, bias_total, sample_params, logprobs, top_ids, top_logprobs,
                                  top_k, want, dtype, (hipStream_t)stream, allow_words, n_masks, mask_row});
}
