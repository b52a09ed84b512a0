// attn_decode_gqa.hip — paged decode attention for grouped-query models (n_heads > n_kv_heads,
// one new token per sequence).  Same entry as attn_decode.hip (mha_varlen_fwd with q_len == 1,
// flash_api.cpp:216-355 of the reference); chosen by hx_api when group > 1.
//
// Why a second kernel: attn_decode.hip gives every QUERY head its own workgroup, so a KV head is
// streamed `group` times (measured on MI355X, B=32 H=32 ctx 832: 73 us whether HK is 32 or 8 —
// 1.5 TB/s of unique bytes at group 4, 0.8 TB/s at group 7).  Here a workgroup owns one
// (sequence, KV head, key split) and the `group` query heads ride along as the 16 columns of the
// MFMA B operand, so every K / V byte is read once.
//
//   * grid = (n_kv_heads, batch, splits), 4 waves; wave w takes the 32-key tiles w, w+4, ... of
//     the split.  A tile goes HBM -> registers (whole 2D-byte rows, 4 rows per instruction; the
//     next tile's loads are in flight under the current tile's math; page ids are fetched one
//     tile ahead) -> a wave-private LDS image (row stride 2D+32 B) — no workgroup barrier in
//     the loop.
//   * S^T[key][head] = K . Q^T : A = K fragments from the image, B = Q^T of the group's heads
//     (columns >= group are zero).  Softmax per column as in attn_fwd.hip; P^T is the B operand
//     of O^T[dim][head] += V^T . P^T with V^T read by ds_read_b64_tr_b16.  P is rounded to T
//     before P.V like the prefill kernel (flash_fwd_kernel.h:878).
//   * the four waves' (m, l, O) states are merged through LDS; with splits > 1 the workgroup
//     writes per-head partials in the layout attn_decode_combine_kernel reads.
#include "attn_common.h"

namespace hx {
int launch_decode_combine(const AttnParams& p, int batch, int head_dim, int dtype, hipStream_t stream);
}

namespace {

using namespace hx;

constexpr int NW = 4;

// The kernel's body lives in attn_decode_gqa_body.inc and is INCLUDED into attn_decode_gqa_kernel (ALIBI = false) and
// attn_decode_gqa_alibi_kernel: the existing instantiations keep their names and their instruction streams (see
// attn_decode.hip for why it is textual inclusion and not a body function).
template <typename T, int D>
__global__ __launch_bounds__(NW * 64) void attn_decode_gqa_kernel(const AttnParams p) {
  constexpr bool ALIBI = false;
#include "attn_decode_gqa_body.inc"
}

// the same kernel with ALiBi slopes (AttnParams::alibi)
template <typename T, int D>
__global__ __launch_bounds__(NW * 64) void attn_decode_gqa_alibi_kernel(const AttnParams p) {
  constexpr bool ALIBI = true;
#include "attn_decode_gqa_body.inc"
}

template <typename T, int D>
int launch_gqa(const AttnParams& p, int batch, int dtype, hipStream_t stream) {
  constexpr int RS = 2 * D + 32;
  const size_t images = (size_t)NW * 2 * 32 * RS;
  const size_t merge = (size_t)(2 * NW * 16 + NW * D * 16) * sizeof(float);
  const size_t lds = images > merge ? images : merge;
  void (*const kernel)(const AttnParams) = p.alibi ? attn_decode_gqa_alibi_kernel<T, D> : attn_decode_gqa_kernel<T, D>;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return hip_rc(e);
  }
  dim3 grid(p.n_heads / p.group, batch, p.n_splits);
  hx::launcher(kernel, grid, NW * 64, lds, stream)(p);
  int rc = check_launch();
  if (rc || p.n_splits == 1) return rc;
  return launch_decode_combine(p, batch, D, dtype, stream);
}

}  // namespace

namespace hx {

bool decode_gqa_supported(int head_dim, int group) {
  return group > 1 && group <= 16 && (head_dim == 64 || head_dim == 128 || head_dim == 256);
}

// splits towards ~512 workgroups (8 waves per CU), but only while every wave keeps at least four
// 32-key tiles: below that the second launch (combine) costs more than the parallelism gains
// (measured, tools/bench_attn_decode_gqa.py: B=32 HK=8 ctx 832 one split 24 us, two 26 us)
int decode_gqa_pick_splits(int batch, int n_kv_heads, int max_seqlen_k, int requested) {
  if (requested >= 1) return requested > 128 ? 128 : requested;
  const int64_t base = (int64_t)batch * n_kv_heads;
  const int n_tiles = (max_seqlen_k + 31) / 32;
  int64_t want = (512 + base - 1) / base;
  int64_t cap = n_tiles / (4 * NW);
  if (cap < 1) cap = 1;
  int64_t s = want < cap ? want : cap;
  if (s > 64) s = 64;
  return (int)s;
}

int launch_attn_decode_gqa(const AttnParams& p, int batch, int head_dim, int dtype, hipStream_t stream) {
#define HX_GQA_CASE(TT, DD) case DD: return launch_gqa<TT, DD>(p, batch, dtype, stream);
  if (dtype == HX_F16) {
    switch (head_dim) { HX_GQA_CASE(F16, 64) HX_GQA_CASE(F16, 128) HX_GQA_CASE(F16, 256) }
  } else if (dtype == HX_BF16) {
    switch (head_dim) { HX_GQA_CASE(BF16, 64) HX_GQA_CASE(BF16, 128) HX_GQA_CASE(BF16, 256) }
  } else {
    return HX_ERR_DTYPE;
  }
#undef HX_GQA_CASE
  return HX_ERR_SHAPE;
}

}  // namespace hx
