// moe_gemm.h — what the two grouped expert GEMM families (moe_gemm_kernel in moe_experts.hip: 16-bit weights;
// moe_gemm_fp8w_kernel in moe_experts_fp8.hip: FP8 block-scaled weights) share outside the kernel body
// (moe_gemm_body.inc): the limits, the chunking, and the host side — shape check, argument check, launch.
#pragma once
#include <algorithm>
#include "attn_common.h"

namespace hx {

constexpr int kMaxE = 256;       // routed experts
constexpr int kMaxTopk = 8;
constexpr int kTile = 64;        // token rows per tile

// The chunking of K, the same for every weight format (what a format changes is how many load instructions a stream's
// SK k are: moe_gemm_body.inc).
template <int MB, int GU>
struct MoeGemmCfg {
  static constexpr int KL = (GU || MB == 4) ? 512 : 1024;   // k per LDS chunk
  static constexpr int SK = GU ? KL : KL / 2;               // k per stream and chunk
  static constexpr int RS = KL * 2 + 32;                    // LDS row stride of the x image in bytes (B-fragment ds_read_b128: conflict free)
  static constexpr int kRows = MB * 16;                     // token rows per tile
  static constexpr size_t kLds = (size_t)kRows * RS + 4 * 2048 + 2 * kTile * 4;
};

// (hidden and inter in whole 128s: the scale block's edge, and what the 16-bit kernels ask for as well)
inline int moe_check_shape(int64_t n, int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter) {
  if (n <= 0 || topk <= 0 || n_experts <= 0 || hidden <= 0 || inter <= 0) return HX_ERR_SHAPE;
  if (n_experts > kMaxE || topk > kMaxTopk || hidden % 128 || inter % 128) return HX_ERR_SHAPE;
  if (n * topk > (int64_t)1 << 24 || n_experts * 2 * inter * hidden >= (int64_t)1 << 40) return HX_ERR_SHAPE;
  return HX_OK;
}

// The argument check of hx_moe_gate_up_silu / hx_moe_down (fp8w = false, w_scale unused) and of their _fp8w twins.
// The order of the last two is each family's own and part of its C ABI: the 16-bit entries report a misaligned pointer
// before a dtype they do not do, the FP8 entries the dtype first.
inline int moe_check_args(const void* out, const void* in, const void* weight, const float* w_scale, bool fp8w,
                          const int32_t* seg, int64_t n_tokens, int64_t topk, int64_t n_experts, int64_t hidden,
                          int64_t inter, int dtype) {
  if (!out || !in || !weight || (fp8w && !w_scale) || !seg) return HX_ERR_NULL;
  if (int rc = moe_check_shape(n_tokens, topk, n_experts, hidden, inter)) return rc;
  const int rc_dtype = (dtype != HX_F16 && dtype != HX_BF16) ? HX_ERR_DTYPE : HX_OK;
  const int rc_align = (!aligned16(out) || !aligned16(in) || !aligned16(weight) || (fp8w && ((uintptr_t)w_scale & 3u)))
                           ? HX_ERR_STRIDE : HX_OK;
  if (fp8w) return rc_dtype ? rc_dtype : rc_align;
  return rc_align ? rc_align : rc_dtype;
}

// One launch of family F (F::kernel<T, MB, GU>() = the kernel) over grid = (N / 64, E).  MB = 16-row blocks of a tile =
// what min(n tokens, 64) rows need.  `weight...` = the kernel's arguments between xin and seg: the weights, and their
// scales where the format has them.
template <typename F, typename T, int GU, typename... W>
int launch_moe_gemm(void* out, const void* xin, const int32_t* seg, int64_t N, int64_t K, int64_t n_experts,
                    int64_t n_slots, int64_t topk, hipStream_t stream, W... weight) {
  const dim3 grid((unsigned)(N / 64), (unsigned)n_experts);
  u16* o = (u16*)out;
  const u16* x = (const u16*)xin;
  const int mb = (int)((std::min<int64_t>(n_slots / topk, kTile) + 15) / 16);   // n tokens
  if (mb == 1)
    return launch_lds(F::template kernel<T, 1, GU>(), grid, 256, MoeGemmCfg<1, GU>::kLds, stream, o, x,
                      weight..., seg, (int)N, (int)K, (int)n_experts, (int)n_slots, (int)topk);
  if (mb == 2)
    return launch_lds(F::template kernel<T, 2, GU>(), grid, 256, MoeGemmCfg<2, GU>::kLds, stream, o, x,
                      weight..., seg, (int)N, (int)K, (int)n_experts, (int)n_slots, (int)topk);
  return launch_lds(F::template kernel<T, 4, GU>(), grid, 256, MoeGemmCfg<4, GU>::kLds, stream, o, x,
                    weight..., seg, (int)N, (int)K, (int)n_experts, (int)n_slots, (int)topk);
}

}  // namespace hx
