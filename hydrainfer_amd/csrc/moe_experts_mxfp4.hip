// moe_experts_mxfp4.hip — the two grouped expert GEMMs of moe_experts.hip for MXFP4 expert weights: the OCP microscaling
// format (E2M1 elements, two per byte, element 2j in bits 0-3 of byte j; one E8M0 scale byte per 32 consecutive k,
// byte b = 2^(b - 127), 0xFF = NaN).  Weight-only: the activations stay fp16 / bf16 and the MFMA stays the 16-bit
// 16x16x32 one; what halves again is the bytes a step streams (0.53 B per weight against 1.0 for FP8).
//
//     lin(row n of expert e, token row v) = T( sum_g 2^(s[e, n, g] - 127) * ( sum_{k in 32-group g} v[k] * q[e, n, k] ) )
//
// The host plan is moe_gemm.h's (grid (N / 64, E), a workgroup = (expert, 64 weight rows) = 4 waves x 16 rows, all of K,
// MB = 1 / 2 / 4, the x image and its chunking), and the segment prologue, the x gather and the chunk loop follow
// moe_gemm_body.inc.  The weight path is this file's own — there is NO weight image in LDS:
//   * load: lane (c, g) = lane c + 16 g loads the 16 bytes = 32 k = ONE scale group g of the 128-k block of weight row
//     n0 + c.  One instruction of a wave is 16 rows x 64 B = 16 rows x 128 k, so K % 128 is the only condition;
//   * transpose in registers: an MFMA step sums over the k of all four lane quarters, so a step must be one scale
//     group.  The four lanes (c, 0..3) hold a 4 x 4 matrix of 32-bit words (piece g, word j); two v_permlane32_swap and
//     two v_permlane16_swap transpose it: afterwards word st of lane (c, g) is k 32 st + 8 g .. + 7 of row c — the k of
//     the 16-bit B fragment of step st, so the x image, its reads and their banks are those of the other two families;
//   * widen: v_cvt_scalef32_pk_{bf16,f16}_fp4 with scale 1, two elements per instruction, exact for all 16 codes;
//   * the weight is the MFMA's B operand (the x fragment is A): a lane's four accumulators are four TOKEN rows of ONE
//     weight row c, so a step has one scale per lane: the scale word (4 bytes = the block's four groups) of row c is
//     loaded by lane (c, *) with its weight piece and stays in a register.  Step st: tmp = mfma(x, w, 0), then
//     acc = fma(tmp, 2^(byte st - 127), acc) — exact for every byte 1..254 and both dtypes; the scale never touches a
//     weight before the MFMA, so no weight is rounded after it has been scaled;
//   * store: out[slot of token row 4 g + i][n0 + c], 16 lanes = 32 contiguous bytes per token row.
// A third translation unit, so that the device code of moe_experts.hip and moe_experts_fp8.hip does not move.
#include "moe_gemm.h"

namespace {

using namespace hx;

// 8 E2M1 nibbles of a word -> 8 T in nibble order (byte 0 low, byte 0 high, byte 1 low, ...)
template <typename T> struct Fp4Widen;
template <> struct Fp4Widen<BF16> {
  template <int B> static __device__ __forceinline__ uint32_t pk(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, B));
  }
};
template <> struct Fp4Widen<F16> {
  template <int B> static __device__ __forceinline__ uint32_t pk(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, B));
  }
};
template <typename T>
__device__ __forceinline__ u16x8 widen_fp4(uint32_t q) {
  const u32x4 o = {Fp4Widen<T>::template pk<0>(q), Fp4Widen<T>::template pk<1>(q), Fp4Widen<T>::template pk<2>(q),
                   Fp4Widen<T>::template pk<3>(q)};
  return __builtin_bit_cast(u16x8, o);
}

// E8M0 byte -> fp32: b << 23 is 2^(b - 127) for 1..254; byte 0 is the denormal 2^-127 and byte 255 a NaN — both are the
// mantissa's top bit on top of b << 23
__device__ __forceinline__ float e8m0(uint32_t b) {
  uint32_t bits = b << 23;
  if (((b + 1u) & 0xffu) < 2u) bits |= 0x00400000u;
  return __builtin_bit_cast(float, bits);
}

// (a, b) of the four lanes' word matrix: the lanes' upper half of a <-> the lower half of b (halves of 32 / of 16 lanes)
__device__ __forceinline__ void swap32(uint32_t& a, uint32_t& b) {
  const auto v = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = v[0]; b = v[1];
}
__device__ __forceinline__ void swap16(uint32_t& a, uint32_t& b) {
  const auto v = __builtin_amdgcn_permlane16_swap(a, b, false, false);
  a = v[0]; b = v[1];
}

// GU = 1: act[s, j] = T(silu(T(lin_gate)) * T(lin_up)), K = hidden, N = inter, bytes [E, 2N, K/2], scales [E, 2N, K/32];
// GU = 0: y[s, c] = T(lin_down), K = inter, N = hidden, bytes [E, N, K/2], scales [E, N, K/32].
template <typename T, int MB, int GU>
__global__ __launch_bounds__(256, 2) void moe_gemm_mxfp4w_kernel(u16* __restrict__ out, const u16* __restrict__ xin,
                                                                 const uint8_t* __restrict__ wgt,
                                                                 const uint8_t* __restrict__ wsc,
                                                                 const int32_t* __restrict__ seg, const int N, const int K,
                                                                 const int n_experts, const int n_slots, const int topk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = MoeGemmCfg<MB, GU>;
  constexpr int KL = C::KL, SK = C::SK, kRS = C::RS, kRows = C::kRows;
  constexpr int NB = SK / 128;                   // 128-k blocks = load instructions per stream and chunk
  constexpr int kCpr = KL / 8;                   // 16-byte pieces per LDS row of x
  constexpr int XPT = kRows * kCpr / 256;        // pieces per thread and chunk
  constexpr int XRND = XPT < 8 ? XPT : 8;        // ... fetched 8 at a time
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
  const int c = lane & 15, g = lane >> 4;
  int32_t* srow = reinterpret_cast<int32_t*>(smem + kRows * kRS + 4 * 2048);   // [64] source row of x per tile row
  int32_t* drow = srow + kTile;                                                 // [64] destination slot
  const char* xl = smem + c * kRS + g * 16;      // A fragment: token row c, k 8 g .. + 7 of a step

  const int n0 = (blockIdx.x * 4 + w) << 4;       // the wave's 16 output rows
  const int64_t wrows = GU ? 2 * (int64_t)N : (int64_t)N;
  const int64_t wrow = (int64_t)e * wrows + n0 + c;           // the lane's weight row (of stream 0)
  const uint8_t* wbase = wgt + wrow * (K >> 1) + 16 * g;      // its 16-byte piece = scale group g of a block
  const uint8_t* sbase = wsc + wrow * (K >> 5);               // its scale bytes: 4 per block
  const int n_it = (K + KL - 1) / KL;

  // weight load of stream s at LDS chunk `it`: instruction cb is the 128-k block cb (64 bytes of 16 rows) and the scale
  // word beside it the block's four group bytes; blocks past K re-read a valid one (their MFMAs are skipped)
  auto load = [&](u32x4 (&buf)[NB], uint32_t (&sc)[NB], int it, int s) {
    const int k0 = it * KL + (GU ? 0 : s * SK);
    const int last_cb = max(min((K - k0) >> 7, NB), 1) - 1;
    const int k0c = min(k0, K - 128);
    const uint8_t* wp = wbase + (GU ? (int64_t)s * N * (K >> 1) : 0) + (k0c >> 1);
    const uint8_t* sp = sbase + (GU ? (int64_t)s * N * (K >> 5) : 0) + (k0c >> 5);
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
      const int b = min(cb, last_cb);
      buf[cb] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + 64 * b));
      sc[cb] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(sp + 4 * b));
    }
  };
  // pieces [j0, j0 + XRND) of this thread's share of the gathered rows of chunk `it` (always a valid address; rows past
  // the tile and k past K are zero-filled at the LDS write).  Piece j of all threads covers the kRpp rows from j * kRpp;
  // pieces past the tile's last 16-row block that holds rows (`xrows` = 16 nmb) are neither fetched nor written.
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
      *reinterpret_cast<u16x8*>(smem + row * kRS + ch * 16) = ok ? xr[j] : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
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
      u32x4 buf[2][NB];
      uint32_t sc[2][NB];
      xload(xr, it, 0, nmb * 16);
      load(buf[0], sc[0], it, 0);
      load(buf[1], sc[1], it, 1);
      // keep the weight loads in flight under the x staging (hipcc sinks them below the LDS writes)
      __builtin_amdgcn_sched_barrier(0);
      __syncthreads();                             // the previous chunk's A reads
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
        const int ncb = min(max((K - k0) >> 7, 0), NB);   // blocks of this stream inside K
        const char* xp = xl + (GU ? 0 : s * SK * 2);
        f32x4 (&accb)[MB] = acc[GU ? s : 0];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          if (cb < ncb) {
            // (piece g, word j) -> (piece j, word g): bit 1 of g and j by the 32-lane swap, bit 0 by the 16-lane one
            uint32_t q0 = buf[s][cb][0], q1 = buf[s][cb][1], q2 = buf[s][cb][2], q3 = buf[s][cb][3];
            swap32(q0, q2);
            swap32(q1, q3);
            swap16(q0, q1);
            swap16(q2, q3);
            const uint32_t qs[4] = {q0, q1, q2, q3};
            const uint32_t sw = sc[s][cb];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
              const u16x8 wf = widen_fp4<T>(qs[st]);
              const float sv = e8m0((sw >> (8 * st)) & 0xffu);
#pragma unroll
              for (int mb = 0; mb < MB; ++mb) {
                if (mb < nmb) {
                  const u16x8 xf = *reinterpret_cast<const u16x8*>(xp + mb * 16 * kRS + (4 * cb + st) * 64);
                  const f32x4 tmp = Mfma<T>::mma(xf, wf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
                  for (int i = 0; i < 4; ++i) accb[mb][i] = __builtin_fmaf(tmp[i], sv, accb[mb][i]);
                }
              }
            }
          }
        }
      }
    }

    // ---- epilogue: acc[.][mb][i] = out[tile row 16 mb + 4 g + i][n0 + c]
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = mb * 16 + 4 * g + i;
        if (mb < nmb && m < rows) {
          u16 o;
          if (GU) {
            const float gt = round_to<T>(acc[0][mb][i]);
            const float up = round_to<T>(acc[GU ? 1 : 0][mb][i]);
            const float a = round_to<T>(gt / (1.0f + __expf(-gt)));
            o = T::from_float(a * up);
          } else {
            o = T::from_float(acc[0][mb][i]);
          }
          out[(int64_t)drow[m] * N + n0 + c] = o;
        }
      }
    }
  }
}

struct MoeMxfp4 {
  template <typename T, int MB, int GU> static constexpr auto kernel() { return moe_gemm_mxfp4w_kernel<T, MB, GU>; }
};

// moe_check_args with the FP8 family's order (dtype before alignment); of the scale it looks at the pointer only: not
// null and 4-byte aligned, which is what a block's scale word needs
inline int check(const void* out, const void* in, const void* weight, const uint8_t* w_scale, const int32_t* seg,
                 int64_t n_tokens, int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter, int dtype) {
  return moe_check_args(out, in, weight, reinterpret_cast<const float*>(w_scale), true, seg, n_tokens, topk, n_experts,
                        hidden, inter, dtype);
}

}  // namespace

using namespace hx;

extern "C" int hx_moe_gate_up_silu_mxfp4w(void* act, const void* x, const void* wq_gate_up, const uint8_t* w_scale,
                                          const int32_t* seg, int64_t n_tokens, int64_t topk, int64_t n_experts,
                                          int64_t hidden, int64_t inter, int dtype, hx_stream stream) {
  if (int rc = check(act, x, wq_gate_up, w_scale, seg, n_tokens, topk, n_experts, hidden, inter, dtype)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* w = (const uint8_t*)wq_gate_up;
  if (dtype == HX_F16)
    return launch_moe_gemm<MoeMxfp4, F16, 1>(act, x, seg, inter, hidden, n_experts, n_tokens * topk, topk, s, w, w_scale);
  return launch_moe_gemm<MoeMxfp4, BF16, 1>(act, x, seg, inter, hidden, n_experts, n_tokens * topk, topk, s, w, w_scale);
}

extern "C" int hx_moe_down_mxfp4w(void* y, const void* act, const void* wq_down, const uint8_t* w_scale, const int32_t* seg,
                                  int64_t n_tokens, int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter, int dtype,
                                  hx_stream stream) {
  if (int rc = check(y, act, wq_down, w_scale, seg, n_tokens, topk, n_experts, hidden, inter, dtype)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* w = (const uint8_t*)wq_down;
  if (dtype == HX_F16)
    return launch_moe_gemm<MoeMxfp4, F16, 0>(y, act, seg, hidden, inter, n_experts, n_tokens * topk, topk, s, w, w_scale);
  return launch_moe_gemm<MoeMxfp4, BF16, 0>(y, act, seg, hidden, inter, n_experts, n_tokens * topk, topk, s, w, w_scale);
}
