// gemm_fp8a.hip — the W8A8 prefill GEMM: e4m3 activations with one fp32 scale per (row, 128-k group) against FP8
// block-scaled weights (e4m3 bytes [N, K], one fp32 scale per 128 x 128 block, read in place), on the FP8 matrix
// instructions of gfx950 (v_mfma_f32_32x32x64_f8f6f4, both formats e4m3, no hardware scale).  Two launches:
//
//   hx_quant_fp8_group   s[m][g] = max(amax_{k in g} |x[m][k]|, 1e-10) / 448      q[m][k] = e4m3_rne(clamp(x / s, +-448))
//   hx_linear_fp8a       out[m][n] = T( sum over 128-k blocks b, in order, of
//                                       (xs[m][b] * ws[n / 128][b]) * ( sum_{k in b} xq[m][k] * wq[n][k] ) )
//
// The fp32 block scales are no powers of two, so they cannot ride the instruction's E8M0 operands: a block's 128 products
// go through two MFMAs into a temporary that starts at zero, and the temporary is folded into the running sum with one
// fma by s = xs * ws.  No split-K, no atomics, one rounding to T at the store.
//
// bf16 RESULTS RUN ON THE FP8 INSTRUCTION, fp16 RESULTS DO NOT.  Both FP8 matrix instructions of gfx950 (32x32x64_f8f6f4 and
// 32x32x16_fp8_fp8 give the same bits) align the products of 8 consecutive k to the largest of them and cut them 13 binary
// places below its leading bit before adding (profiles/linear_fp8a.md, Finding).  That is invisible under a bf16 rounding
// and 1.4 - 2.3 x the project's fp16 GEMM tolerance on outputs near zero.  So the F16 instantiations widen the staged
// bytes to fp16 (exact, fp8_widen.h), 8 bytes of each operand per step, and run four v_mfma_f32_32x32x16_f16 per 64 k:
// same tiles, same LDS images, same fold, the same k pairing (a lane's 32 bytes are cut into four runs of 8 for A and B
// alike), products and sums in fp32.  They are half as fast as the bf16 ones; the profile says what that costs.
//
// THE QUANTISER.  A wave takes (row, 512 k): 64 lanes x one 16-byte load of 8 elements, so 16 lanes hold a group.  The
// group maximum is an UNSIGNED INTEGER maximum of the |x| bit patterns (it orders non-negative floats as floats and puts
// every NaN above infinity, so a NaN in the group reaches the scale, as torch's amax does) over the 16 lanes by xor
// shuffles; x / s is the IEEE division; v_cvt_pk_fp8_f32 packs two values per instruction; a lane stores its 8 bytes at
// once.  No LDS.  The scales are written through two strides: the shim keeps them k-major ([K / 128][rows]), the order
// in which the GEMM reads them.
//
// THE GEMM.  256 threads own a 128 (n) x BM (m) output tile, BM = 128 or 64; a k-step is 128 k = one scale block, so the
// weight scale of a k-step is ONE scalar per workgroup and the activation scales are BM floats.  The two operand tiles of
// a k-step are staged as raw bytes in LDS, double-buffered: every thread has the next step's 16-byte global loads in
// flight in registers while the MFMAs of this step run, writes them into the other buffer afterwards, and one barrier per
// k-step separates the writes from their readers.  LDS rows are 128 bytes at a pitch of 144: the fragment read is a
// ds_read_b128 at the same column of 32 rows, and 36 r mod 64 = 4 (9 r mod 16) sends any 16 rows that differ mod 16 to
// 16 different bank quads.  The weight is the A operand (i = n), the activations the B operand (j = m): a lane's 16
// accumulators of a 32 x 32 tile then belong to ONE row m = lane % 32 — the fold needs one scale per lane and tile — and
// to four runs of four consecutive n (8 (r / 4) + 4 (lane / 32) + r % 4): an 8-byte store each.  A lane's 32 operand
// bytes are 32 consecutive k, the same k for A and B (k = 64 kk + 32 (lane / 32) + byte).  The four waves are 2 (n) x
// 2 (m); a wave owns 64 n x BM / 2 m as 2 x MW tiles.  Rows past M are staged as zero bytes with zero scales and never
// stored.  Workgroups are numbered so that the ones an XCD runs together are neighbours in an m-fastest walk of the
// tiles: they share weight tiles in that XCD's L2.
#include <cstring>
#include "fp8_widen.h"

namespace {

using namespace hx;

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kBlk = 128;                 // the scale block's edge = k per step = n per tile
constexpr int kPitch = kBlk + 16;         // LDS row pitch in bytes
constexpr int kGroupLanes = 16;           // lanes that hold one 128-k group in the quantiser
constexpr float kFp8Max = 448.f;

// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void quant_fp8_group_kernel(uint8_t* __restrict__ xq, float* __restrict__ xs,
                                                              const u16* __restrict__ x, const int M, const int K,
                                                              const int chunks, const int64_t ldx, const int64_t ldq,
                                                              const int64_t sx_row, const int64_t sx_grp) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // (row, 512-k chunk); uniform in a wave
  if (unit >= (int64_t)M * chunks) return;
  const int m = (int)(unit / chunks);
  const int k = ((int)(unit - (int64_t)m * chunks) << 9) + 8 * lane;
  const bool on = k < K;                                                   // whole 16-lane groups (K % 128 == 0)
  u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (on) v = *reinterpret_cast<const u16x8*>(x + (int64_t)m * ldx + k);
  float f[8];
  uint32_t top = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f[e] = T::to_float(v[e]);
    top = max(top, __builtin_bit_cast(uint32_t, f[e]) & 0x7fffffffu);
  }
#pragma unroll
  for (int off = kGroupLanes / 2; off > 0; off >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, off, kGroupLanes));
  const float s = __builtin_bit_cast(float, max(top, __builtin_bit_cast(uint32_t, 1e-10f))) / kFp8Max;
  float c[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float q = f[e] / s;
    c[e] = q != q ? q : fminf(fmaxf(q, -kFp8Max), kFp8Max);
  }
  u32x2 o;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(c[4 * h], c[4 * h + 1], 0, false);
    o[h] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c[4 * h + 2], c[4 * h + 3], w, true);
  }
  if (on) {
    *reinterpret_cast<u32x2*>(xq + (int64_t)m * ldq + k) = o;
    if ((lane & (kGroupLanes - 1)) == 0) xs[(int64_t)m * sx_row + (int64_t)(k >> 7) * sx_grp] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct Fp8aParams {
  const uint8_t* xq;
  const float* xs;
  const uint8_t* wq;
  const float* ws;          // [N / 128][K / 128]
  u16* out;
  int64_t ldq, sx_row, sx_grp, ldw, ldo;
  int32_t M, N, K, m_tiles, tiles;
};

// MW = 32-row m tiles per wave: the workgroup's tile is 128 n x 64 MW m
template <typename T, int MW>
__global__ __launch_bounds__(256, 2) void linear_fp8a_kernel(const Fp8aParams p) {
  constexpr int BM = 64 * MW;
  constexpr bool kWiden = std::is_same<T, F16>::value;     // fp16 results: 16-bit MFMAs over widened bytes (header comment)
  constexpr int kXPieces = BM / 32;                       // 16-byte pieces of the x tile per thread (the w tile: 4)
  constexpr int kBufBytes = (kBlk + BM) * kPitch + BM * 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = w & 1, wm = w >> 1;
  const int c = lane & 31, hi = lane >> 5;

  // the tile of this workgroup: hardware id -> XCD-contiguous logical id -> (n tile, m tile), m fastest
  const int id = blockIdx.x, xcd = id & 7, q8 = p.tiles >> 3, r8 = p.tiles & 7;
  const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (id >> 3);
  const int tn = logical / p.m_tiles, tm = logical - tn * p.m_tiles;
  const int n0 = tn * kBlk, m0 = tm * BM;
  const int KB = p.K >> 7;

  // staging map: piece i of a thread is row (tid >> 3) + 32 i, bytes 16 (tid & 7) .. + 15 of the k-step
  const int srow = tid >> 3, scol = (tid & 7) << 4;
  const uint8_t* wsrc = p.wq + (int64_t)(n0 + srow) * p.ldw + scol;
  const uint8_t* xsrc = p.xq + (int64_t)(m0 + srow) * p.ldq + scol;
  const float* wscale = p.ws + (int64_t)tn * KB;
  u32x4 gw[4], gx[kXPieces];
  float gs = 0.f;
  auto fetch = [&](int b) {
#pragma unroll
    for (int i = 0; i < 4; ++i) gw[i] = *reinterpret_cast<const u32x4*>(wsrc + (int64_t)(32 * i) * p.ldw + kBlk * b);
#pragma unroll
    for (int i = 0; i < kXPieces; ++i) {
      gx[i] = u32x4{0, 0, 0, 0};
      if (m0 + srow + 32 * i < p.M) gx[i] = *reinterpret_cast<const u32x4*>(xsrc + (int64_t)(32 * i) * p.ldq + kBlk * b);
    }
    if (tid < BM) gs = m0 + tid < p.M ? p.xs[(int64_t)(m0 + tid) * p.sx_row + (int64_t)b * p.sx_grp] : 0.f;
  };
  auto stage = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(buf + (srow + 32 * i) * kPitch + scol) = gw[i];
#pragma unroll
    for (int i = 0; i < kXPieces; ++i) *reinterpret_cast<u32x4*>(buf + (kBlk + srow + 32 * i) * kPitch + scol) = gx[i];
    if (tid < BM) *reinterpret_cast<float*>(buf + (kBlk + BM) * kPitch + 4 * tid) = gs;
  };

  f32x16 acc[2][MW];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int mt = 0; mt < MW; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nt][mt][r] = 0.f;

  fetch(0);
  stage(smem);
  __syncthreads();

  // fragment addresses inside a buffer: row of the tile = lane % 32, 32 bytes at 64 kk + 32 (lane / 32)
  const int a_off = (wn * 64 + c) * kPitch + 32 * hi;
  const int b_off = (kBlk + wm * 32 * MW + c) * kPitch + 32 * hi;
  const int s_off = (kBlk + BM) * kPitch + 4 * (wm * 32 * MW + c);
  auto frag = [](const char* at) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(at), up = *reinterpret_cast<const u32x4*>(at + 16);
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)up[0], (int)up[1], (int)up[2], (int)up[3]};
  };

  for (int b = 0; b < KB; ++b) {
    const char* cur = smem + (b & 1) * kBufBytes;
    const float sw = wscale[b];
    if (b + 1 < KB) fetch(b + 1);
    f32x16 tmp[2][MW];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      i32x8 fa[2], fb[MW];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) fa[nt] = frag(cur + a_off + nt * 32 * kPitch + 64 * kk);
#pragma unroll
      for (int mt = 0; mt < MW; ++mt) fb[mt] = frag(cur + b_off + mt * 32 * kPitch + 64 * kk);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int mt = 0; mt < MW; ++mt) {
          if (kk == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) tmp[nt][mt][r] = 0.f;
          }
          if constexpr (!kWiden)
            tmp[nt][mt] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[nt], fb[mt], tmp[nt][mt], 0, 0, 0, 0, 0, 0);
        }
      if constexpr (kWiden) {        // fp16: four 16-k steps over the lane's 32 bytes, 8 bytes of each operand widened per step
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f16x8 wa[2], wb[MW];
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            wa[nt] = __builtin_bit_cast(f16x8, widen<F16>(u32x2{(uint32_t)fa[nt][2 * j], (uint32_t)fa[nt][2 * j + 1]}));
#pragma unroll
          for (int mt = 0; mt < MW; ++mt)
            wb[mt] = __builtin_bit_cast(f16x8, widen<F16>(u32x2{(uint32_t)fb[mt][2 * j], (uint32_t)fb[mt][2 * j + 1]}));
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < MW; ++mt)
              tmp[nt][mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[nt], wb[mt], tmp[nt][mt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int mt = 0; mt < MW; ++mt) {
      const float s = *reinterpret_cast<const float*>(cur + s_off + 4 * 32 * mt) * sw;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][mt][r] = __builtin_fmaf(tmp[nt][mt][r], s, acc[nt][mt][r]);
    }
    if (b + 1 < KB) stage(smem + ((b + 1) & 1) * kBufBytes);
    __syncthreads();
  }

  // out[m][n0 + 64 wn + 32 nt + 8 rq + 4 hi .. + 3] = acc[nt][mt][4 rq .. 4 rq + 3], m = m0 + 32 MW wm + 32 mt + c
#pragma unroll
  for (int mt = 0; mt < MW; ++mt) {
    const int m = m0 + wm * 32 * MW + 32 * mt + c;
    if (m >= p.M) continue;
    u16* orow = p.out + (int64_t)m * p.ldo + n0 + wn * 64 + 4 * hi;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        u16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = T::from_float(acc[nt][mt][4 * rq + e]);
        *reinterpret_cast<u16x4*>(orow + 32 * nt + 8 * rq) = o;
      }
  }
}

int g_force_rows = 0;      // tuning: 0 = automatic, else the tile's rows (64 / 128)

// Rows of the output tile.  Two workgroups of either height are resident per CU (LDS), and a 64-row tile takes 2/3 of the
// time of a 128-row one (profiles/linear_fp8a.md: 336 against 255 us for the same 11008 x 4096 x 4096 product), so a
// launch costs its number of rounds over the 2 x CUs slots times 2 resp. 3: the cheaper height wins, ties go to 128 rows.
// Every one of the 24 measured (shape, M) points of the profile agrees with this rule.
int tile_rows(int64_t M, int64_t N) {
  if (g_force_rows == 64 || g_force_rows == 128) return g_force_rows;
  const int64_t slots = 2 * n_cus(), cols = N / kBlk;
  const int64_t r128 = ((M + 127) / 128 * cols + slots - 1) / slots, r64 = ((M + 63) / 64 * cols + slots - 1) / slots;
  return 2 * r64 < 3 * r128 ? 64 : 128;
}

template <typename T, int MW>
int launch_fp8a(Fp8aParams p, hipStream_t stream) {
  constexpr int BM = 64 * MW;
  p.m_tiles = (p.M + BM - 1) / BM;
  p.tiles = p.m_tiles * (p.N / kBlk);
  const size_t lds = 2 * ((size_t)(kBlk + BM) * kPitch + BM * 4);
  return launch_lds(linear_fp8a_kernel<T, MW>, dim3((unsigned)p.tiles), dim3(256), lds, stream, p);
}

}  // namespace

namespace hx {

int gemm_fp8a_set_option(const char* name, int value) {
  if (!strcmp(name, "fp8a_tile_rows")) { g_force_rows = value; return HX_OK; }
  return HX_ERR_UNSUPPORTED;
}

}  // namespace hx

using namespace hx;

extern "C" int hx_quant_fp8_group(void* xq, float* xs, const void* x, int64_t M, int64_t K, int64_t ldx, int64_t ldq,
                                  int64_t xs_row_stride, int64_t xs_group_stride, int dtype, hx_stream stream) {
  if (M <= 0 || K <= 0) return HX_ERR_SHAPE;
  if (!xq || !xs || !x) return HX_ERR_NULL;
  if (K % kBlk || M >= ((int64_t)1 << 31) || K >= ((int64_t)1 << 31) || ldx % 8 || ldx < K || ldq % 16 || ldq < K ||
      xs_row_stride <= 0 || xs_group_stride <= 0)
    return HX_ERR_SHAPE;
  if (!aligned16(x) || !aligned16(xq) || ((uintptr_t)xs & 3u)) return HX_ERR_STRIDE;
  const int chunks = (int)((K + 511) / 512);
  const int64_t blocks = (M * chunks + 3) / 4;
  if (blocks >= ((int64_t)1 << 31)) return HX_ERR_SHAPE;
  return dispatch_dtype16(dtype, [&](auto t) {
    launcher(quant_fp8_group_kernel<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream)(
        (uint8_t*)xq, xs, (const u16*)x, (int)M, (int)K, chunks, ldx, ldq, xs_row_stride, xs_group_stride);
    return check_launch();
  });
}

extern "C" int hx_linear_fp8a(void* out, const void* xq, const float* xs, const void* wq, const float* w_scale, int64_t M,
                              int64_t N, int64_t K, int64_t ldq, int64_t xs_row_stride, int64_t xs_group_stride, int64_t ldw,
                              int64_t ldo, int dtype, hx_stream stream) {
  if (M <= 0 || N <= 0 || K <= 0) return HX_ERR_SHAPE;
  if (!out || !xq || !xs || !wq || !w_scale) return HX_ERR_NULL;
  if (N % kBlk || K % kBlk || M >= ((int64_t)1 << 31) - kBlk || N >= ((int64_t)1 << 31) || K >= ((int64_t)1 << 31) || ldq % 16 ||
      ldq < K || ldw % 16 || ldw < K || ldo % 4 || ldo < N || xs_row_stride <= 0 || xs_group_stride <= 0 ||
      (M + 63) / 64 * (N / kBlk) >= ((int64_t)1 << 31))
    return HX_ERR_SHAPE;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  if (!aligned16(xq) || !aligned16(wq) || ((uintptr_t)xs & 3u) || ((uintptr_t)w_scale & 3u) || ((uintptr_t)out & 7u))
    return HX_ERR_STRIDE;
  Fp8aParams p;
  p.xq = (const uint8_t*)xq; p.xs = xs; p.wq = (const uint8_t*)wq; p.ws = w_scale; p.out = (u16*)out;
  p.ldq = ldq; p.sx_row = xs_row_stride; p.sx_grp = xs_group_stride; p.ldw = ldw; p.ldo = ldo;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.m_tiles = p.tiles = 0;
  const bool wide = tile_rows(M, N) == 128;
  return dispatch_dtype16(dtype, [&](auto t) {
    return wide ? launch_fp8a<decltype(t), 2>(p, (hipStream_t)stream) : launch_fp8a<decltype(t), 1>(p, (hipStream_t)stream);
  });
}
