// moe_experts_fp8.hip — the two grouped expert GEMMs of moe_experts.hip for FP8 block-scaled expert weights: the format
// DeepSeek-V3-family checkpoints publish (OCP float8_e4m3fn bytes, one fp32 scale per 128 x 128 block, `weight_scale_inv`:
// weight = float(q) * scale).  Weight-only: the activations stay fp16 / bf16 and the MFMA stays the 16-bit 16x16x32 one;
// what halves is the bytes a step streams, which is what these kernels' time is made of.
//
//     lin(row n of expert e, token row v) = T( sum_b scale[e, n / 128, b] * ( sum_{k in 128-block b} v[k] * q[e, n, k] ) )
//
// moe_gemm_fp8w_kernel IS moe_gemm_kernel's text (moe_gemm_body.inc: one workgroup = (expert, 64 weight rows), 4 waves x
// 16 rows, all of K, one rounding per linear; segments, tiles, x gather, chunk loop, epilogue) and shares its host side
// (moe_gemm.h: shape check, argument check, launch).  What differs is what this file hands to that text:
//   * a load instruction is 8 rows x 128 BYTES = 8 rows x one whole 128-k scale block; two of them fill the wave's 2 KiB
//     transpose image (wstream_image.inc, the same XOR swizzle) with 16 rows x 128 k, so an image holds exactly one
//     scale block;
//   * a block goes through the image by wstream_block_fp8.inc: the A fragment of MFMA step st is a ds_read_b64 (8 bytes =
//     k 32 st + 8 g .. + 7 of row r: the k of the 16-bit fragment, so the x image and its reads are unchanged) widened to
//     T (fp8_widen.h: exact for every finite e4m3 value, NaN bytes stay NaN); the four MFMA steps of a block accumulate
//     into a temporary (MB x f32x4) that starts at zero, and the block's scale — one scalar per (wave, block) — folds it
//     in with one fma(tmp, s, acc).  A weight is never rounded after it has been scaled;
//   * the scales [E, rows / 128, K / 128] are loaded with their blocks;
//   * the x staging fetches only the 16-row blocks of the tile that hold rows (kSkipEmptyRows).
// A second translation unit, so that the device code of moe_experts.hip does not move when this one changes.
#include "fp8_widen.h"
#include "moe_gemm.h"

namespace {

using namespace hx;

// GU = 1: act[s, j] = T(silu(T(lin_gate)) * T(lin_up)), K = hidden, N = inter, bytes [E, 2N, K], scales [E, 2N/128, K/128];
// GU = 0: y[s, c] = T(lin_down), K = inter, N = hidden, bytes [E, N, K], scales [E, N/128, K/128].
#define HX_MOE_BLOCK_INC "wstream_block_fp8.inc"
template <typename T, int MB, int GU>
__global__ __launch_bounds__(256, 2) void moe_gemm_fp8w_kernel(u16* __restrict__ out, const u16* __restrict__ xin,
                                                               const uint8_t* __restrict__ wgt,
                                                               const float* __restrict__ wsc,
                                                               const int32_t* __restrict__ seg, const int N, const int K,
                                                               const int n_experts, const int n_slots, const int topk) {
  using WElem = uint8_t;
  using WVec = u32x4;
  constexpr int kKplLog2 = 7;
  constexpr bool kScaled = true, kSkipEmptyRows = true;
#include "moe_gemm_body.inc"
}
#undef HX_MOE_BLOCK_INC

struct MoeFp8 {
  template <typename T, int MB, int GU> static constexpr auto kernel() { return moe_gemm_fp8w_kernel<T, MB, GU>; }
};

}  // namespace

using namespace hx;

extern "C" int hx_moe_gate_up_silu_fp8w(void* act, const void* x, const void* wq_gate_up, const float* w_scale,
                                        const int32_t* seg, int64_t n_tokens, int64_t topk, int64_t n_experts,
                                        int64_t hidden, int64_t inter, int dtype, hx_stream stream) {
  if (int rc = moe_check_args(act, x, wq_gate_up, w_scale, true, seg, n_tokens, topk, n_experts, hidden, inter, dtype)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* w = (const uint8_t*)wq_gate_up;
  if (dtype == HX_F16)
    return launch_moe_gemm<MoeFp8, F16, 1>(act, x, seg, inter, hidden, n_experts, n_tokens * topk, topk, s, w, w_scale);
  return launch_moe_gemm<MoeFp8, BF16, 1>(act, x, seg, inter, hidden, n_experts, n_tokens * topk, topk, s, w, w_scale);
}

extern "C" int hx_moe_down_fp8w(void* y, const void* act, const void* wq_down, const float* w_scale, const int32_t* seg,
                                int64_t n_tokens, int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter, int dtype,
                                hx_stream stream) {
  if (int rc = moe_check_args(y, act, wq_down, w_scale, true, seg, n_tokens, topk, n_experts, hidden, inter, dtype)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* w = (const uint8_t*)wq_down;
  if (dtype == HX_F16)
    return launch_moe_gemm<MoeFp8, F16, 0>(y, act, seg, hidden, inter, n_experts, n_tokens * topk, topk, s, w, w_scale);
  return launch_moe_gemm<MoeFp8, BF16, 0>(y, act, seg, hidden, inter, n_experts, n_tokens * topk, topk, s, w, w_scale);
}
