// moe_experts_fp8.hip — the two grouped expert GEMMs of moe_experts.hip for FP8 block-scaled expert weights: the format
// DeepSeek-V3-family checkpoints publish (OCP float8_e4m3fn bytes, one fp32 scale per 128 x 128 block, `weight_scale_inv`:
// weight = float(q) * scale).  Weight-only: the activations stay fp16 / bf16 and the MFMA stays the 16-bit 16x16x32 one;
// what halves is the bytes a step streams, which is what these kernels' time is made of.
//
//     lin(row n of expert e, token row v) = T( sum_b scale[e, n / 128, b] * ( sum_{k in 128-block b} v[k] * q[e, n, k] ) )
//
// The plan is moe_gemm_kernel's (one workgroup = (expert, 64 weight rows), 4 waves x 16 rows, all of K, one rounding per
// linear, segments / tiles / x gather / epilogue word for word) with four differences:
//   * a load instruction is 8 rows x 128 BYTES = 8 rows x one whole 128-k scale block; two of them fill the wave's 2 KiB
//     transpose image with 16 rows x 128 k (the same XOR swizzle), so an image holds exactly one scale block;
//   * the A fragment of MFMA step st is a ds_read_b64 of the image (8 bytes = k 32 st + 8 g .. + 7 of row r: the k of the
//     16-bit kernel's fragment, so the x image and its reads are unchanged), widened to T by v_cvt_scalef32_pk_{bf16,f16}_fp8
//     with scale 1 — exact for every finite e4m3 value, NaN bytes stay NaN — two elements per instruction;
//   * the four MFMA steps of a block accumulate into a temporary (MB x f32x4) that starts at zero; the block's scale — one
//     scalar per (wave, block): a wave's 16 rows lie inside one 128-row block — folds it in with one fma(tmp, s, acc).
//     A weight is never rounded after it has been scaled.
//   * the x staging fetches only the 16-row blocks of the tile that hold rows (see xload).
// The device code of moe_experts.hip is not touched: this is a second translation unit that shares no text with it but
// the headers (the x staging and the epilogue are restated here rather than pulled into an .inc under that kernel).
#include <algorithm>
#include "attn_common.h"

namespace {

using namespace hx;

constexpr int kMaxE = 256;       // routed experts            (moe_experts.hip)
constexpr int kMaxTopk = 8;
constexpr int kTile = 64;        // token rows per tile
constexpr int kBlk = 128;        // the scale block's edge

// 8 e4m3 bytes -> 8 T, in byte order
template <typename T> struct Fp8Widen;
template <> struct Fp8Widen<BF16> {
  template <bool HI> static __device__ __forceinline__ uint32_t pk(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
  }
};
template <> struct Fp8Widen<F16> {
  template <bool HI> static __device__ __forceinline__ uint32_t pk(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
  }
};
template <typename T>
__device__ __forceinline__ u16x8 widen(u32x2 q) {
  const u32x4 o = {Fp8Widen<T>::template pk<false>(q[0]), Fp8Widen<T>::template pk<true>(q[0]),
                   Fp8Widen<T>::template pk<false>(q[1]), Fp8Widen<T>::template pk<true>(q[1])};
  return __builtin_bit_cast(u16x8, o);
}

// the chunking of MoeGemmCfg (moe_experts.hip), in scale blocks: KL k per LDS chunk, two streams of SK k, NB blocks each
template <int MB, int GU>
struct MoeFp8Cfg {
  static constexpr int KL = (GU || MB == 4) ? 512 : 1024;
  static constexpr int SK = GU ? KL : KL / 2;
  static constexpr int NB = SK / kBlk;                      // scale blocks per stream and chunk
  static constexpr int NJ = 2 * NB;                         // load instructions per stream and chunk (8 rows x 128 k each)
  static constexpr int RS = KL * 2 + 32;                    // LDS row stride of the x image in bytes
  static constexpr int kRows = MB * 16;
  static constexpr size_t kLds = (size_t)kRows * RS + 4 * 2048 + 2 * kTile * 4;
};

// GU = 1: act[s, j] = T(silu(T(lin_gate)) * T(lin_up)), K = hidden, N = inter, bytes [E, 2N, K], scales [E, 2N/128, K/128];
// GU = 0: y[s, c] = T(lin_down), K = inter, N = hidden, bytes [E, N, K], scales [E, N/128, K/128].
template <typename T, int MB, int GU>
__global__ __launch_bounds__(256, 2) void moe_gemm_fp8w_kernel(u16* __restrict__ out, const u16* __restrict__ xin,
                                                               const uint8_t* __restrict__ wq,
                                                               const float* __restrict__ wsc,
                                                               const int32_t* __restrict__ seg, const int N, const int K,
                                                               const int n_experts, const int n_slots, const int topk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = MoeFp8Cfg<MB, GU>;
  constexpr int KL = C::KL, SK = C::SK, NB = C::NB, NJ = C::NJ, RS = C::RS, kRows = C::kRows;
  constexpr int kCpr = KL / 8;                   // 16-byte pieces per LDS row of x
  constexpr int XPT = kRows * kCpr / 256;
  constexpr int XRND = XPT < 8 ? XPT : 8;
  const int e = blockIdx.y;
  // ---- the expert's segment, before anything else: no rows, no weight bytes and no scales
  int off = seg[e];
  int rows_e = seg[e + 1] - off;
  rows_e = min(max(rows_e, 0), n_slots);                 // (a foreign seg buffer cannot send the gather out of bounds)
  off = min(max(off, 0), n_slots - rows_e);
  if (rows_e == 0) return;
  const int32_t* slots = seg + 2 * n_experts + 1 + off;

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4, c = lane & 15;
  const int lrow = lane >> 3, lpiece = lane & 7;
  int32_t* srow = reinterpret_cast<int32_t*>(smem + kRows * RS + 4 * 2048);   // [64] source row of x per tile row
  int32_t* drow = srow + kTile;                                                 // [64] destination slot
  char* tl = smem + kRows * RS + w * 2048;        // wave-private transpose image: 16 rows x 128 e4m3 bytes
  const int wr_off0 = lrow * 128 + 16 * (lpiece ^ ((lrow >> 1) & 7));
  const int wr_off1 = (lrow + 8) * 128 + 16 * (lpiece ^ (((lrow + 8) >> 1) & 7));
  // 8-byte unit 4 st + g of row r: 16-byte piece 2 st + (g >> 1), swizzled like the writes, half g & 1
  const char* al = tl + r * 128 + 8 * (g & 1);
  const int a_sw = (r >> 1) & 7, a_p = g >> 1;
  const char* xl = smem + c * RS + g * 16;

  const int n0 = (blockIdx.x * 4 + w) << 4;       // the wave's 16 output rows: inside one 128-row scale block
  const int64_t wrows = GU ? 2 * (int64_t)N : (int64_t)N;
  const int KB = K / kBlk;
  const uint8_t* wbase = wq + ((int64_t)e * wrows + n0 + lrow) * K + 16 * lpiece;
  const float* sbase = wsc + ((int64_t)e * (wrows / kBlk) + (n0 >> 7)) * KB;
  const int n_it = (K + KL - 1) / KL;

  // weight load of stream s at LDS chunk `it`: instruction j covers rows 8 * (j & 1) + (lane >> 3) and the 128-byte
  // scale block j >> 1; blocks past K re-read a valid one (their MFMAs are skipped), and so do their scales
  auto load = [&](u32x4 (&buf)[NJ], float (&sc)[NB], int it, int s) {
    const int k0 = it * KL + (GU ? 0 : s * SK);
    const int last_cb = max(min((K - k0) >> 7, NB), 1) - 1;
    const int k0c = min(k0, K - kBlk);
    const uint8_t* wp = wbase + (GU ? (int64_t)s * N * K : 0) + k0c;
    const float* sp = sbase + (GU ? (int64_t)s * (N / kBlk) * KB : 0) + (k0c >> 7);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int cb = min(j >> 1, last_cb);
      buf[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (int64_t)(8 * (j & 1)) * K + kBlk * cb));
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) sc[b] = sp[min(b, last_cb)];
  };
  // pieces [j0, j0 + XRND) of this thread's share of the gathered rows of chunk `it` (always a valid address; rows past
  // the tile and k past K are zero-filled at the LDS write).  Piece j of all threads covers the kRpp rows from j * kRpp:
  // pieces past the tile's last 16-row block that holds rows (`xrows` = 16 nmb) are neither fetched nor written — no
  // MFMA reads those rows — so a tile of few rows does not stage 64 (unlike moe_gemm_kernel: at MB = 4 the staging of
  // 64 x KL of x per chunk is as many bytes as the chunk's fp8 weights).
  constexpr int kRpp = 256 / kCpr;
  auto xload = [&](u16x8 (&xr)[XRND], int it, int j0, int xrows) {
#pragma unroll
    for (int j = 0; j < XRND; ++j) {
      if ((j0 + j) * kRpp >= xrows) continue;
      const int i = threadIdx.x + (j0 + j) * 256;
      const int row = i / kCpr, k = it * KL + (i % kCpr) * 8;
      const int src = srow[row];
      const bool ok = src >= 0 && k < K;
      xr[j] = *reinterpret_cast<const u16x8*>(xin + (int64_t)(ok ? src : 0) * K + (ok ? k : 0));
    }
  };
  auto xstore = [&](const u16x8 (&xr)[XRND], int it, int j0, int xrows) {
#pragma unroll
    for (int j = 0; j < XRND; ++j) {
      if ((j0 + j) * kRpp >= xrows) continue;
      const int i = threadIdx.x + (j0 + j) * 256;
      const int row = i / kCpr, ch = i % kCpr;
      const bool ok = srow[row] >= 0 && it * KL + ch * 8 < K;
      *reinterpret_cast<u16x8*>(smem + row * RS + ch * 16) = ok ? xr[j] : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };

  for (int t0 = 0; t0 < rows_e; t0 += kRows) {
    const int rows = min(kRows, rows_e - t0);
    const int nmb = (rows + 15) >> 4;
    __syncthreads();                               // the previous tile's readers of srow / drow
    if (threadIdx.x < kTile) {
      int s = -1;
      if ((int)threadIdx.x < rows) s = min(max(slots[t0 + threadIdx.x], 0), n_slots - 1);
      drow[threadIdx.x] = s;
      srow[threadIdx.x] = s < 0 ? -1 : (GU ? s / topk : s);
    }
    __syncthreads();

    f32x4 acc[GU ? 2 : 1][MB];
#pragma unroll
    for (int a = 0; a < (GU ? 2 : 1); ++a)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) acc[a][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int it = 0; it < n_it; ++it) {
      u16x8 xr[XRND];
      u32x4 buf[2][NJ];
      float sc[2][NB];
      xload(xr, it, 0, nmb * 16);
      load(buf[0], sc[0], it, 0);
      load(buf[1], sc[1], it, 1);
      // keep the weight loads in flight under the x staging (moe_gemm_kernel)
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();                             // the previous chunk's B reads
      xstore(xr, it, 0, nmb * 16);
#pragma unroll
      for (int j0 = XRND; j0 < XPT; j0 += XRND) {
        xload(xr, it, j0, nmb * 16);
        xstore(xr, it, j0, nmb * 16);
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int k0 = it * KL + (GU ? 0 : s * SK);
        const int ncb = min(max((K - k0) >> 7, 0), NB);          // scale blocks of this stream inside K
        const char* xp = xl + (GU ? 0 : s * SK * 2);
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          if (cb < ncb) {
            *reinterpret_cast<u32x4*>(tl + wr_off0) = buf[s][2 * cb];
            *reinterpret_cast<u32x4*>(tl + wr_off1) = buf[s][2 * cb + 1];
            __builtin_amdgcn_wave_barrier();
            f32x4 tmp[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) tmp[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < 4; ++st) {
              const u16x8 af = widen<T>(*reinterpret_cast<const u32x2*>(al + 16 * ((2 * st + a_p) ^ a_sw)));
#pragma unroll
              for (int mb = 0; mb < MB; ++mb) {
                if (mb < nmb) {
                  const u16x8 xf = *reinterpret_cast<const u16x8*>(xp + mb * 16 * RS + (4 * cb + st) * 64);
                  tmp[mb] = Mfma<T>::mma(af, xf, tmp[mb]);
                }
              }
            }
            const float sv = sc[s][cb];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
              if (mb < nmb) {
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[GU ? s : 0][mb][i] = __builtin_fmaf(tmp[mb][i], sv, acc[GU ? s : 0][mb][i]);
              }
            }
            __builtin_amdgcn_wave_barrier();
          }
        }
      }
    }

    // ---- epilogue: acc[.][mb][i] = out^T[n0 + 4 g + i][tile row 16 mb + c]   (moe_gemm_kernel's, same rounding points)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int m = mb * 16 + c;
      if (mb < nmb && m < rows) {
        u16x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (GU) {
            const float gt = round_to<T>(acc[0][mb][i]);
            const float up = round_to<T>(acc[GU ? 1 : 0][mb][i]);
            const float a = round_to<T>(gt / (1.0f + __expf(-gt)));
            o[i] = T::from_float(a * up);
          } else {
            o[i] = T::from_float(acc[0][mb][i]);
          }
        }
        *reinterpret_cast<u16x4*>(out + (int64_t)drow[m] * N + n0 + 4 * g) = o;
      }
    }
  }
}

int check_shape(int64_t n, int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter) {
  if (n <= 0 || topk <= 0 || n_experts <= 0 || hidden <= 0 || inter <= 0) return HX_ERR_SHAPE;
  if (n_experts > kMaxE || topk > kMaxTopk || hidden % kBlk || inter % kBlk) return HX_ERR_SHAPE;
  if (n * topk > (int64_t)1 << 24 || n_experts * 2 * inter * hidden >= (int64_t)1 << 40) return HX_ERR_SHAPE;
  return HX_OK;
}

template <typename T, int GU>
int launch_moe_gemm_fp8w(void* out, const void* xin, const void* wq, const float* wsc, const int32_t* seg, int64_t N,
                         int64_t K, int64_t n_experts, int64_t n_slots, int64_t topk, hipStream_t stream) {
  const dim3 grid((unsigned)(N / 64), (unsigned)n_experts);
  u16* o = (u16*)out;
  const u16* x = (const u16*)xin;
  const uint8_t* w = (const uint8_t*)wq;
  const int mb = (int)((std::min<int64_t>(n_slots / topk, kTile) + 15) / 16);   // n tokens
  if (mb == 1)
    return launch_lds(moe_gemm_fp8w_kernel<T, 1, GU>, grid, 256, MoeFp8Cfg<1, GU>::kLds, stream, o, x, w, wsc, seg, (int)N,
                      (int)K, (int)n_experts, (int)n_slots, (int)topk);
  if (mb == 2)
    return launch_lds(moe_gemm_fp8w_kernel<T, 2, GU>, grid, 256, MoeFp8Cfg<2, GU>::kLds, stream, o, x, w, wsc, seg, (int)N,
                      (int)K, (int)n_experts, (int)n_slots, (int)topk);
  return launch_lds(moe_gemm_fp8w_kernel<T, 4, GU>, grid, 256, MoeFp8Cfg<4, GU>::kLds, stream, o, x, w, wsc, seg, (int)N,
                    (int)K, (int)n_experts, (int)n_slots, (int)topk);
}

}  // namespace

using namespace hx;

extern "C" int hx_moe_gate_up_silu_fp8w(void* act, const void* x, const void* wq_gate_up, const float* w_scale,
                                        const int32_t* seg, int64_t n_tokens, int64_t topk, int64_t n_experts,
                                        int64_t hidden, int64_t inter, int dtype, hx_stream stream) {
  if (!act || !x || !wq_gate_up || !w_scale || !seg) return HX_ERR_NULL;
  if (int rc = check_shape(n_tokens, topk, n_experts, hidden, inter)) return rc;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  if (!aligned16(act) || !aligned16(x) || !aligned16(wq_gate_up) || ((uintptr_t)w_scale & 3u)) return HX_ERR_STRIDE;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == HX_F16)
    return launch_moe_gemm_fp8w<F16, 1>(act, x, wq_gate_up, w_scale, seg, inter, hidden, n_experts, n_tokens * topk, topk, s);
  return launch_moe_gemm_fp8w<BF16, 1>(act, x, wq_gate_up, w_scale, seg, inter, hidden, n_experts, n_tokens * topk, topk, s);
}

extern "C" int hx_moe_down_fp8w(void* y, const void* act, const void* wq_down, const float* w_scale, const int32_t* seg,
                                int64_t n_tokens, int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter, int dtype,
                                hx_stream stream) {
  if (!y || !act || !wq_down || !w_scale || !seg) return HX_ERR_NULL;
  if (int rc = check_shape(n_tokens, topk, n_experts, hidden, inter)) return rc;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  if (!aligned16(y) || !aligned16(act) || !aligned16(wq_down) || ((uintptr_t)w_scale & 3u)) return HX_ERR_STRIDE;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == HX_F16)
    return launch_moe_gemm_fp8w<F16, 0>(y, act, wq_down, w_scale, seg, hidden, inter, n_experts, n_tokens * topk, topk, s);
  return launch_moe_gemm_fp8w<BF16, 0>(y, act, wq_down, w_scale, seg, hidden, inter, n_experts, n_tokens * topk, topk, s);
}
