// moe_experts.hip — the expert feed-forward half of a sparse MoE layer, for decode batches and prefill chunks:
//     router (softmax, greedy top-k)  ->  segments  ->  gate|up + silu*mul  ->  down  ->  combine (+ shared experts)
// replaces hydrainfer/model/deepseek_v3.py:61-93 (MoEGate.forward) and :124-155 (DeepseekV3MoE.moe_infer): a Python loop
// over the experts — index-gather + three library GEMMs each — around a tokens_per_expert.cpu() host synchronisation.
// Here nothing is read back, no launch shape depends on the routing, and the step captures into a hipGraph.
//
// THE TWO GEMMS (moe_gemm_kernel, the plan of gemm_skinny.hip with an expert dimension):
//   * grid = (output rows of the expert's weight / 64, E); 4 waves, each owns one 16-row group of the weight (for gate|up:
//     gate rows j and up rows I + j, two accumulators).  A workgroup first reads its expert's segment [off_e, off_e+1):
//     an expert with no rows returns before it issues a weight load — unrouted experts cost no bytes.
//   * the weight streams HBM -> VGPR with FULL-LINE loads (one instruction = 8 rows x 128 B, 16 instructions = 16 rows x
//     512 k per register buffer, non-temporal) and is transposed into the MFMA A layout through
//     the wave-private XOR-swizzled 2 KiB LDS image of gemm_skinny_kernel.
//   * B = the expert's token rows, GATHERED through the slot list into LDS (source row s / topk of x for gate|up, row s
//     of act for down; no permuted copy of x exists), one fragment per 16 rows: a weight fragment feeds rows/16 MFMAs
//     16x16x32; 16-row blocks past the segment's end are skipped.
//   * K is staged in LDS chunks (512 k; 1024 k for down below 64-row tiles; <= 67 KB) and the workgroup walks ALL of
//     K itself: gate|up needs the complete g before silu, and down then needs no slabs — one fp32 accumulation chain per
//     output, rounded once to T like nn.Linear.  Deterministic, no atomics.
//   * a segment longer than 64 rows is walked in 64-row tiles (prefill chunks), re-reading the weights once per tile.
// SEGMENTS (moe_segments_kernel): ONE small launch of one workgroup — counts, exclusive offsets and the slot list in
// LDS-integer-atomic order (order inside a group is free: a slot's result does not depend on its place).  Chosen over a
// scan in the GEMM prologues because it serves every n (prefill too) with one code path and keeps ~1400 GEMM workgroups
// from each repeating the same scan in front of their first weight load.
#include <cfloat>
#include "moe_gemm.h"

namespace {

using namespace hx;

// ---------------------------------------------------------------------------------------------------------------------
// a. router.  One 256-thread workgroup per token: x row -> LDS (fp32), wave w takes experts w, w + 4, ... (lanes stride
// over h, fp32 products and sums), then wave 0 runs softmax + iterative arg-max (the rule of topk_softmax_kernel: lower
// index wins ties, the chosen entry is cleared).  deepseek_v3.py:61-93, scoring_func = "softmax", topk_method = "greedy".
// ---------------------------------------------------------------------------------------------------------------------
template <typename TX, typename TW>
__global__ __launch_bounds__(256) void moe_gate_topk_kernel(float* __restrict__ weights, int32_t* __restrict__ ids,
                                                            const typename TX::storage* __restrict__ x,
                                                            const typename TW::storage* __restrict__ wr, int hidden,
                                                            int n_experts, int topk, int norm, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* xs = reinterpret_cast<float*>(smem);          // [hidden]
  float* logit = xs + hidden;                          // [kMaxE]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t token = blockIdx.x;
  for (int i = threadIdx.x; i < hidden; i += 256) xs[i] = TX::to_float(x[token * hidden + i]);
  __syncthreads();
  for (int e = w; e < n_experts; e += 4) {
    const typename TW::storage* row = wr + (int64_t)e * hidden;
    float acc = 0.f;
    for (int i = lane; i < hidden; i += 64) acc += xs[i] * TW::to_float(row[i]);
    acc = wave_sum(acc);
    if (lane == 0) logit[e] = acc;
  }
  __syncthreads();
  if (w != 0) return;
  constexpr int kPerLane = kMaxE / 64;
  float v[kPerLane];
  float mx = -FLT_MAX;
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) {
    const int e = lane + 64 * i;
    v[i] = e < n_experts ? logit[e] : -FLT_MAX;
    mx = fmaxf(mx, v[i]);
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) {
    const int e = lane + 64 * i;
    v[i] = e < n_experts ? expf(v[i] - mx) : 0.f;
    sum += v[i];
  }
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
#pragma unroll
  for (int i = 0; i < kPerLane; ++i) v[i] = (lane + 64 * i) < n_experts ? v[i] * inv : -FLT_MAX;
  float mine = 0.f, total = 0.f;      // lane k keeps the k-th weight
  int mine_id = 0;
  for (int k = 0; k < topk; ++k) {
    float best = -FLT_MAX;
    int col = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
      const int e = lane + 64 * i;
      if (e < n_experts && v[i] > best) { best = v[i]; col = e; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off, 64);
      const int oc = __shfl_xor(col, off, 64);
      if (ob > best || (ob == best && oc < col)) { best = ob; col = oc; }
    }
    if (lane == k) { mine = best; mine_id = col; }
    total += best;                   // k order, the order of topk_weight.sum(dim=-1)
#pragma unroll
    for (int i = 0; i < kPerLane; ++i)
      if (lane + 64 * i == col) v[i] = -10000.f;
  }
  if (lane < topk) {
#pragma clang fp contract(off)
    // deepseek_v3.py:88-92: renormalised only when top_k > 1
    const float wgt = (norm && topk > 1) ? mine / (total + 1e-20f) * scale : mine * scale;
    weights[token * topk + lane] = wgt;
    ids[token * topk + lane] = mine_id;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// b. segments.  seg = [ offsets E + 1 | counts E | slots n * topk ] (int32).  One workgroup; ids outside [0, E) are not
// routed (their slot appears in no group).  replaces deepseek_v3.py:125-130 (scatter_, argsort, .cpu()).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_segments_kernel(int32_t* __restrict__ seg, const int32_t* __restrict__ ids,
                                                           int n_slots, int n_experts) {
  __shared__ int32_t cnt[kMaxE];
  __shared__ int32_t cur[kMaxE];
  __shared__ int32_t scan[256];
  const int t = threadIdx.x;
  cnt[t] = 0;
  __syncthreads();
  for (int s = t; s < n_slots; s += 256) {
    const int e = ids[s];
    if (e >= 0 && e < n_experts) atomicAdd(&cnt[e], 1);
  }
  __syncthreads();
  const int32_t c = t < n_experts ? cnt[t] : 0;
  scan[t] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int32_t add = t >= off ? scan[t - off] : 0;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const int32_t excl = scan[t] - c;
  cur[t] = excl;
  if (t < n_experts) {
    seg[t] = excl;
    seg[n_experts + 1 + t] = c;
  }
  if (t == n_experts - 1) seg[n_experts] = scan[t];
  __syncthreads();
  int32_t* slots = seg + 2 * n_experts + 1;
  for (int s = t; s < n_slots; s += 256) {
    const int e = ids[s];
    if (e >= 0 && e < n_experts) slots[atomicAdd(&cur[e], 1)] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// c / d. the grouped GEMMs.  GU = 1: act[s, j] = T(silu(T(x_t . Wg_e[j])) * T(x_t . Wu_e[j])), K = hidden, N = inter,
//        weight [E, 2N, K];  GU = 0: y[s, c] = T(act_s . Wd_e[c]), K = inter, N = hidden, weight [E, N, K].
// Per LDS chunk of KL k a wave reads two weight STREAMS, both issued at the top of the chunk so that the second is in
// flight under the x staging and the first stream's MFMAs:
//   GU: stream 0 = gate rows, stream 1 = up rows, both over the chunk's KL k, one accumulator set each;
//   down: stream 0 / 1 = the first / second half of the chunk of the same rows, one accumulator set.
// Nothing is carried in registers from one chunk to the next but the accumulators (a refill issued under the MFMAs for
// the NEXT trip of a run-time loop is given fresh registers and copied at the back edge: 390 VGPRs); the latency of a
// chunk's first loads is covered by the other workgroups of the CU instead — LDS and registers leave room for 2 .. 8.
// MB = 16-row blocks of a tile = what min(n, 64) rows need — a function of n, not of the routing.  An expert holds at
// most n rows when a token's ids are distinct (every router's output); a longer segment is walked in tiles all the same.
// ---------------------------------------------------------------------------------------------------------------------
// The body is moe_gemm_body.inc, shared with moe_gemm_fp8w_kernel (moe_experts_fp8.hip); this is its 16-bit form: a load
// instruction is 8 rows x 64 k, a block goes through the image by wstream_block16.inc, there are no scales, and the x
// staging fetches all 16 MB rows of a tile.
#define HX_MOE_BLOCK_INC "wstream_block16.inc"
template <typename T, int MB, int GU>
__global__ __launch_bounds__(256, 2) void moe_gemm_kernel(u16* __restrict__ out, const u16* __restrict__ xin,
                                                       const u16* __restrict__ wgt, const int32_t* __restrict__ seg,
                                                       const int N, const int K, const int n_experts, const int n_slots,
                                                       const int topk) {
  using WElem = u16;
  using WVec = u16x8;
  constexpr int kKplLog2 = 6;
  constexpr bool kScaled = false, kSkipEmptyRows = false;
  const float* wsc = nullptr;
#include "moe_gemm_body.inc"
}
#undef HX_MOE_BLOCK_INC

struct Moe16 {
  template <typename T, int MB, int GU> static constexpr auto kernel() { return moe_gemm_kernel<T, MB, GU>; }
};

// ---------------------------------------------------------------------------------------------------------------------
// e. combine.  out[t, c] = T( float(T( sum_k w[t, k] * float(y[t topk + k, c]) )) + float(shared[t, c]) ): every product
// rounded to fp32 on its own, summed in k order (deepseek_v3.py:148-154: .type(f32).mul_(w).sum(dim=1).type(T)), then
// y + shared_experts(identity) in T (:120).  One thread per 8 columns.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void moe_combine_kernel(u16* __restrict__ out, const u16* __restrict__ y,
                                                          const float* __restrict__ weights, const u16* __restrict__ shared,
                                                          int64_t n_vec, int hidden, int topk) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_vec) return;
  const int vpr = hidden >> 3;
  const int64_t t = i / vpr;
  const int c0 = (int)(i - t * vpr) << 3;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int k = 0; k < topk; ++k) {
    const float wk = weights[t * topk + k];
    const u16x8 v = *reinterpret_cast<const u16x8*>(y + (t * topk + k) * hidden + c0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = T::to_float(v[j]) * wk;
      acc[j] = k ? acc[j] + p : p;
    }
  }
  u16x8 o;
  if (shared) {
    const u16x8 sv = *reinterpret_cast<const u16x8*>(shared + t * hidden + c0);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = T::from_float(round_to<T>(acc[j]) + T::to_float(sv[j]));
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = T::from_float(acc[j]);
  }
  *reinterpret_cast<u16x8*>(out + t * hidden + c0) = o;
}

template <typename TX>
int launch_gate(float* weights, int32_t* ids, const void* x, const void* wr, int64_t n, int64_t hidden, int64_t n_experts,
                int64_t topk, int w_dtype, int norm, float scale, hipStream_t stream) {
  const size_t lds = (size_t)(hidden + kMaxE) * sizeof(float);
  const typename TX::storage* xp = (const typename TX::storage*)x;
  if (w_dtype == HX_F32)
    return launch_lds(moe_gate_topk_kernel<TX, F32>, (unsigned)n, 256, lds, stream, weights, ids, xp, (const float*)wr,
                      (int)hidden, (int)n_experts, (int)topk, norm, scale);
  if (w_dtype != TX::kDtype) return HX_ERR_DTYPE;
  return launch_lds(moe_gate_topk_kernel<TX, TX>, (unsigned)n, 256, lds, stream, weights, ids, xp,
                    (const typename TX::storage*)wr, (int)hidden, (int)n_experts, (int)topk, norm, scale);
}

}  // namespace

using namespace hx;

extern "C" int64_t hx_moe_segments_elems(int64_t n_tokens, int64_t topk, int64_t n_experts) {
  if (n_tokens <= 0 || topk <= 0 || n_experts <= 0) return 0;
  return 2 * n_experts + 1 + n_tokens * topk;
}

extern "C" int hx_moe_gate_topk(float* topk_weights, int32_t* topk_ids, const void* x, const void* router_weight,
                                int64_t n_tokens, int64_t hidden, int64_t n_experts, int64_t topk, int x_dtype,
                                int weight_dtype, int scoring, int64_t n_group, int64_t topk_group, int norm_topk_prob,
                                float routed_scaling_factor, hx_stream stream) {
  if (!topk_weights || !topk_ids || !x || !router_weight) return HX_ERR_NULL;
  if (scoring != HX_MOE_SCORE_SOFTMAX || n_group > 1 || topk_group > 1) return HX_ERR_UNSUPPORTED;
  if (n_tokens <= 0 || hidden <= 0 || n_experts <= 0 || topk <= 0) return HX_ERR_SHAPE;
  if (n_experts > kMaxE || topk > kMaxTopk || topk > n_experts || hidden > 8192) return HX_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (x_dtype == HX_F16)
    return launch_gate<F16>(topk_weights, topk_ids, x, router_weight, n_tokens, hidden, n_experts, topk, weight_dtype,
                            norm_topk_prob, routed_scaling_factor, s);
  if (x_dtype == HX_BF16)
    return launch_gate<BF16>(topk_weights, topk_ids, x, router_weight, n_tokens, hidden, n_experts, topk, weight_dtype,
                             norm_topk_prob, routed_scaling_factor, s);
  return HX_ERR_DTYPE;
}

extern "C" int hx_moe_segments(int32_t* seg, const int32_t* topk_ids, int64_t n_tokens, int64_t topk, int64_t n_experts,
                               hx_stream stream) {
  if (!seg || !topk_ids) return HX_ERR_NULL;
  if (n_tokens <= 0 || topk <= 0 || n_experts <= 0 || n_experts > kMaxE || topk > kMaxTopk || n_tokens * topk > (int64_t)1 << 24)
    return HX_ERR_SHAPE;
  hx::launcher(moe_segments_kernel, 1, 256, 0, (hipStream_t)stream)(seg, topk_ids, (int)(n_tokens * topk), (int)n_experts);
  return check_launch();
}

extern "C" int hx_moe_gate_up_silu(void* act, const void* x, const void* w_gate_up, const int32_t* seg, int64_t n_tokens,
                                   int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter, int dtype,
                                   hx_stream stream) {
  if (int rc = moe_check_args(act, x, w_gate_up, nullptr, false, seg, n_tokens, topk, n_experts, hidden, inter, dtype)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const u16* w = (const u16*)w_gate_up;
  if (dtype == HX_F16) return launch_moe_gemm<Moe16, F16, 1>(act, x, seg, inter, hidden, n_experts, n_tokens * topk, topk, s, w);
  return launch_moe_gemm<Moe16, BF16, 1>(act, x, seg, inter, hidden, n_experts, n_tokens * topk, topk, s, w);
}

extern "C" int hx_moe_down(void* y, const void* act, const void* w_down, const int32_t* seg, int64_t n_tokens, int64_t topk,
                           int64_t n_experts, int64_t hidden, int64_t inter, int dtype, hx_stream stream) {
  if (int rc = moe_check_args(y, act, w_down, nullptr, false, seg, n_tokens, topk, n_experts, hidden, inter, dtype)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const u16* w = (const u16*)w_down;
  if (dtype == HX_F16) return launch_moe_gemm<Moe16, F16, 0>(y, act, seg, hidden, inter, n_experts, n_tokens * topk, topk, s, w);
  return launch_moe_gemm<Moe16, BF16, 0>(y, act, seg, hidden, inter, n_experts, n_tokens * topk, topk, s, w);
}

extern "C" int hx_moe_combine(void* out, const void* y, const float* topk_weights, const void* shared, int64_t n_tokens,
                              int64_t topk, int64_t hidden, int dtype, hx_stream stream) {
  if (!out || !y || !topk_weights) return HX_ERR_NULL;
  if (n_tokens <= 0 || topk <= 0 || hidden <= 0 || topk > kMaxTopk || hidden % 8) return HX_ERR_SHAPE;
  if (!aligned16(out) || !aligned16(y) || (shared && !aligned16(shared))) return HX_ERR_STRIDE;
  const int64_t n_vec = n_tokens * (hidden / 8);
  const unsigned blocks = (unsigned)((n_vec + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == HX_F16)
    hx::launcher(moe_combine_kernel<F16>, blocks, 256, 0, s)((u16*)out, (const u16*)y, topk_weights, (const u16*)shared, n_vec, (int)hidden, (int)topk);
  else if (dtype == HX_BF16)
    hx::launcher(moe_combine_kernel<BF16>, blocks, 256, 0, s)((u16*)out, (const u16*)y, topk_weights, (const u16*)shared, n_vec, (int)hidden, (int)topk);
  else
    return HX_ERR_DTYPE;
  return check_launch();
}
