// gemm_skinny_fp8.hip — the weight-streaming decode GEMM of gemm_skinny.hip (M <= 64 rows) for FP8 block-scaled weights: the
// format DeepSeek-V3-family checkpoints publish for every dense linear (OCP float8_e4m3fn bytes [N, K], one fp32 scale per
// 128 x 128 block, `weight_scale_inv`: weight = float(q) * scale).  Weight-only: x stays fp16 / bf16 and the MFMA the 16-bit
// 16x16x32 one; what halves is the bytes a step streams.
//
//     partial[s][m][n] = sum over 128-k blocks b of split s of scale[n / 128][b] * ( sum_{k in b} x[m][k] * float(q[n][k]) )
//     out[m][n]        = T( sum_s partial[s][m][n] )                                      (launch_slab_reduce, fixed order)
//
// The plan is gemm_skinny_kernel's — grid = (N tiles, K splits of <= 1024 k), the x slice staged once in LDS, every wave
// streaming whole 16-row groups with full-line non-temporal loads through its private XOR-swizzled 2 KiB transpose image,
// fp32 slabs for the slab reduce.  Shared with it as text: the x staging (gemm_skinny_x_load.inc / _store.inc: same
// image, same row stride) and the image's geometry (wstream_image.inc); shared with moe_gemm_fp8w_kernel
// (moe_experts_fp8.hip): the way of one scale block through the image (wstream_block_fp8.inc) and the widening
// (fp8_widen.h).  What is this kernel's own:
//   * a load instruction is 8 rows x 128 BYTES = 8 rows x one whole 128-k scale block; two of them fill the image with
//     16 rows x 128 k, so an image holds exactly one scale block (the block text widens a ds_read_b64 of it per MFMA step,
//     runs the block's four steps into a temporary that starts at zero and folds it into the running sum with one fma by
//     the block's scale: a weight is never rounded after it has been scaled);
//   * a register buffer is still 16 KiB and two are in flight; at one byte per weight a buffer is a whole (row group,
//     split): R row groups per wave are R buffers, and nothing is summed across buffers;
//   * a wave's 16 rows lie inside one 128-row scale block, so the scales of a (row group, split) are at most 8
//     wave-uniform floats: scalar loads, issued a whole buffer of work ahead of their use (the first buffer's with its
//     weight loads, the second's behind the x staging, so that they are not held in SGPRs across it).
// A translation unit of its own beside gemm_skinny.hip; it shares the split rule (gemm_skinny_splits), the workspace size
// and the slab reduce with it through their host entry points.
#include <cstring>
#include "attn_common.h"
#include "fp8_widen.h"

namespace hx {
int gemm_skinny_splits(int64_t K);
int launch_slab_reduce(const float* partial, void* out, int64_t M, int64_t N, int64_t ldo, int n_splits, int dtype,
                       hipStream_t stream);
}  // namespace hx

extern "C" int64_t hx_linear_decode_workspace_bytes(int64_t M, int64_t N, int64_t K);

namespace {

using namespace hx;

struct Fp8GemmParams {
  const void* x;
  const uint8_t* wq;
  const float* ws;   // [N / 128][K / 128]
  float* partial;    // [S][M][N]
  int64_t ldx;       // elements
  int64_t ldw;       // bytes
  int32_t M, N, K;
};

constexpr int kBlk = 128;                 // the scale block's edge
constexpr int kSplitK = 1024;             // k per split = one 16 KiB register buffer of 16 rows
constexpr int kNB = kSplitK / kBlk;       // scale blocks per buffer
constexpr int kNJ = 2 * kNB;              // load instructions per buffer (8 rows x 128 k each)
constexpr int kRS = kSplitK * 2 + 32;     // LDS row stride of the x image in bytes (gemm_skinny.hip's kRS)

// R = 16-row groups per wave (one register buffer each); NW = waves per workgroup.  Compile-time constants: the
// load / compute schedule is straight-line code (gemm_skinny_kernel).
template <typename T, int MB, int R, int NW>
__global__ __launch_bounds__(NW * 64) void gemm_skinny_fp8w_kernel(const Fp8GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int kThreads = NW * 64;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4, c = lane & 15;

  const int split = blockIdx.y;
  const int k0 = split * kSplitK;
  const int KR = min(kSplitK, p.K - k0);          // multiple of 256
  const int nblk = KR >> 7;                       // scale blocks of this split: 2 .. 8
  const int KB = p.K >> 7;
  const int n_rg_all = p.N >> 4;
  // wave's row groups: rg0 + j * NW, j < R (groups past the end are clamped for loads and skipped at the store)
  const int rg0 = blockIdx.x * (NW * R) + w;

  // ---- 1. x slice -> registers
  const u16* xb = reinterpret_cast<const u16*>(p.x) + k0;
  constexpr bool kNoXLoads = false;
#include "gemm_skinny_x_load.inc"

  // ---- 2. W prefetch.  Instruction j of a buffer covers rows 8 * (j & 1) + (lane >> 3) and the 128-byte scale block
  // j >> 1; lane & 7 selects the 16-byte piece.  Blocks past the split re-read its last one (their MFMAs are skipped), row
  // groups past N the last one (their stores are skipped); the scales follow their blocks.
  const int lrow = lane >> 3, lpiece = lane & 7;
  const uint8_t* wb = p.wq + k0 + 16 * lpiece;
  auto load = [&](u32x4 (&buf)[kNJ], int it) {
    const int n0 = min(rg0 + it * NW, n_rg_all - 1) << 4;
    const uint8_t* wp = wb + (int64_t)(n0 + lrow) * p.ldw;
#pragma unroll
    for (int j = 0; j < kNJ; ++j) {
      const int cb = min(j >> 1, nblk - 1);
      buf[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp + (int64_t)(8 * (j & 1)) * p.ldw + kBlk * cb));
    }
  };
  // the (at most 8) scales of row group `it` in this split: wave-uniform, scalar loads
  auto load_scales = [&](float (&sc)[kNB], int it) {
    const int n0 = min(rg0 + it * NW, n_rg_all - 1) << 4;
    const float* sp = p.ws + (int64_t)(n0 >> 7) * KB + (k0 >> 7);
#pragma unroll
    for (int b = 0; b < kNB; ++b) sc[b] = sp[min(b, nblk - 1)];
  };
  u32x4 buf[2][kNJ];
  float sc[2][kNB];
  load(buf[0], 0);
  if constexpr (R > 1) load(buf[1], 1);
  load_scales(sc[0], 0);
  // keep the weight prefetch in flight UNDER the x staging (gemm_skinny_kernel)
  __builtin_amdgcn_sched_barrier(0);

  // ---- 3. x slice -> LDS
#include "gemm_skinny_x_store.inc"
  __syncthreads();
  // the second buffer's scales: a whole buffer of work ahead of their use, and not held in SGPRs across the staging
  if constexpr (R > 1) load_scales(sc[1], 1);

  // the wave-private transpose images lie behind the x slice; an image holds 16 rows x 128 e4m3 bytes = one scale block
  char* images = smem + MB * 16 * kRS;
#include "wstream_image.inc"
  constexpr int nmb = MB;                        // every 16-row block of the x image takes part
  const char* xp = smem + c * kRS + g * 16;      // one buffer = the whole split: every buffer reads x from its first k

#pragma unroll
  for (int it = 0; it < R; ++it) {
    f32x4 acc[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const u32x4 (&wbuf)[kNJ] = buf[it & 1];
    const float (&wscale)[kNB] = sc[it & 1];
    f32x4 (&accb)[MB] = acc;
#pragma unroll
    for (int cb = 0; cb < kNB; ++cb) {
      if (cb < nblk) {
#include "wstream_block_fp8.inc"
      }
    }
    if (it + 2 < R) { load(buf[it & 1], it + 2); load_scales(sc[it & 1], it + 2); }
    const int rg = rg0 + it * NW;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int m = mb * 16 + c;
      if (m < p.M && rg < n_rg_all)
        *reinterpret_cast<f32x4*>(p.partial + ((int64_t)split * p.M + m) * p.N + (rg << 4) + 4 * g) = acc[mb];
    }
  }
}

// out[n][k] = T(float(q[n][k]) * scale[n / 128][k / 128]): one fp32 multiply, one rounding.  A thread takes 16 bytes of a
// row (inside one scale block) and writes two 16-byte pieces.
template <typename T>
__global__ __launch_bounds__(256) void dequant_fp8_block_kernel(u16* __restrict__ out, const uint8_t* __restrict__ wq,
                                                                const float* __restrict__ ws, const int64_t n_pieces,
                                                                const int K, const int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // 16-byte piece of the input
  if (i >= n_pieces) return;
  const int ppr = K >> 4;
  const int64_t n = i / ppr;
  const int k = (int)(i - n * ppr) << 4;
  const u32x4 q = *reinterpret_cast<const u32x4*>(wq + n * K + k);
  const float s = ws[(n >> 7) * (K >> 7) + (k >> 7)];
  u16* dst = out + n * ldo + k;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const u16x8 t = widen<T>(u32x2{q[2 * h], q[2 * h + 1]});    // exact
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = T::from_float(T::to_float(t[e]) * s);
    *reinterpret_cast<u16x8*>(dst + 8 * h) = o;
  }
}

int g_force_r = 0;       // tuning: 0 = automatic, else row groups per wave
int g_force_nw = 0;      // tuning: 0 = automatic, else waves per workgroup

bool fp8_supported(int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw) {
  return M >= 1 && M <= 64 && N > 0 && K > 0 && N % kBlk == 0 && K % 256 == 0 && N < ((int64_t)1 << 31) &&
         K < ((int64_t)1 << 31) && ldx % 8 == 0 && ldx >= K && ldw % 16 == 0 && ldw >= K;
}

// (waves, row groups per wave) of a launch.  units = (row group, split) pairs = 16 KiB buffers.  Few units: 4-wave
// workgroups with one buffer per wave, as many workgroups as the shape gives (the 16-bit kernel's choice up to ~1000
// workgroups).  More: two buffers per wave, so that a wave has its second 16 KiB in flight while it works on the first;
// from 4096 units on 8-wave workgroups (fewer x stagings per weight byte).  33 .. 64 rows: the x slice alone is 133 KB of
// LDS, one workgroup per CU — 8 waves as soon as 4-wave workgroups would outnumber the CUs four times.
// Built: MB 1 / 2: (4, 1) (4, 2) (8, 2); MB 4: (4, 1) (8, 1) (8, 2).
bool plan_cfg(int MB, int64_t N, int64_t K, int* nw, int* rpw) {
  const int64_t units = (N >> 4) * gemm_skinny_splits(K);
  if (MB < 4) {
    *nw = units > 4096 ? 8 : 4;
    *rpw = units > 1024 ? 2 : 1;
  } else {
    *nw = units > 1024 ? 8 : 4;
    *rpw = units > 2048 ? 2 : 1;
  }
  if (g_force_nw) *nw = g_force_nw;
  if (g_force_r) *rpw = g_force_r;
  if (MB < 4) return (*nw == 4 && (*rpw == 1 || *rpw == 2)) || (*nw == 8 && *rpw == 2);
  return (*nw == 4 && *rpw == 1) || (*nw == 8 && (*rpw == 1 || *rpw == 2));
}

template <typename T, int MB, int R, int NW>
int launch_cfg(const Fp8GemmParams& p, hipStream_t stream) {
  const int n_rg = p.N >> 4;
  const dim3 grid((unsigned)((n_rg + NW * R - 1) / (NW * R)), (unsigned)gemm_skinny_splits(p.K));
  const size_t lds = (size_t)MB * 16 * kRS + (size_t)NW * 2048;   // x slice + per-wave transpose images
  return launch_lds(gemm_skinny_fp8w_kernel<T, MB, R, NW>, grid, dim3(NW * 64), lds, stream, p);
}

template <typename T, int MB>
int launch_mb(const Fp8GemmParams& p, hipStream_t stream) {
  int nw = 0, rpw = 0;
  if (!plan_cfg(MB, p.N, p.K, &nw, &rpw)) return HX_ERR_UNSUPPORTED;   // a forced pair that is not built for these rows
  if constexpr (MB < 4) {
    if (nw == 8) return launch_cfg<T, MB, 2, 8>(p, stream);
    if (rpw == 2) return launch_cfg<T, MB, 2, 4>(p, stream);
    return launch_cfg<T, MB, 1, 4>(p, stream);
  } else {
    if (nw == 4) return launch_cfg<T, MB, 1, 4>(p, stream);
    if (rpw == 2) return launch_cfg<T, MB, 2, 8>(p, stream);
    return launch_cfg<T, MB, 1, 8>(p, stream);
  }
}

template <typename T>
int launch_t(const Fp8GemmParams& p, hipStream_t stream) {
  const int MB = (p.M + 15) / 16;
  if (MB == 1) return launch_mb<T, 1>(p, stream);
  if (MB == 2) return launch_mb<T, 2>(p, stream);
  return launch_mb<T, 4>(p, stream);
}

}  // namespace

namespace hx {

int gemm_fp8_set_option(const char* name, int value) {
  if (!strcmp(name, "gemm_fp8_rows_per_wave")) { g_force_r = value; return HX_OK; }
  if (!strcmp(name, "gemm_fp8_waves")) { g_force_nw = value; return HX_OK; }
  return HX_ERR_UNSUPPORTED;
}

}  // namespace hx

using namespace hx;

extern "C" int hx_linear_decode_fp8w(void* out, const void* x, const void* wq, const float* w_scale, int64_t M, int64_t N,
                                     int64_t K, int64_t ldx, int64_t ldw, int64_t ldo, void* workspace,
                                     int64_t workspace_bytes, int dtype, hx_stream stream) {
  if (M <= 0 || N <= 0 || K <= 0) return HX_ERR_SHAPE;
  if (!out || !x || !wq || !w_scale || !workspace) return HX_ERR_NULL;
  if (!fp8_supported(M, N, K, ldx, ldw) || ldo % 4 != 0 || ldo < N) return HX_ERR_SHAPE;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  if (workspace_bytes < hx_linear_decode_workspace_bytes(M, N, K)) return HX_ERR_WORKSPACE;
  if (!aligned16(x) || !aligned16(wq) || !aligned16(workspace) || ((uintptr_t)w_scale & 3u) || ((uintptr_t)out & 7u))
    return HX_ERR_STRIDE;
  Fp8GemmParams p;
  p.x = x; p.wq = (const uint8_t*)wq; p.ws = w_scale; p.partial = (float*)workspace; p.ldx = ldx; p.ldw = ldw;
  p.M = (int)M; p.N = (int)N; p.K = (int)K;
  hipStream_t s = (hipStream_t)stream;
  const int rc = dtype == HX_F16 ? launch_t<F16>(p, s) : launch_t<BF16>(p, s);
  if (rc) return rc;
  return launch_slab_reduce((const float*)workspace, out, M, N, ldo, gemm_skinny_splits(K), dtype, s);
}

// out[0] = waves per workgroup, out[1] = row groups per wave of the launch hx_linear_decode_fp8w(M, N, K) makes under the
// current options (host only).  HX_ERR_UNSUPPORTED: a forced pair that is not built for these rows.
extern "C" int hx_debug_linear_fp8_plan(int64_t M, int64_t N, int64_t K, int32_t* out) {
  if (!out) return HX_ERR_NULL;
  if (!fp8_supported(M, N, K, K, K)) return HX_ERR_SHAPE;
  const int MB = (int)((M + 15) / 16);
  int nw = 0, rpw = 0;
  const bool ok = plan_cfg(MB == 3 ? 4 : MB, N, K, &nw, &rpw);
  out[0] = nw; out[1] = rpw;
  return ok ? HX_OK : HX_ERR_UNSUPPORTED;
}

extern "C" int hx_dequant_fp8_block(void* out, const void* wq, const float* w_scale, int64_t N, int64_t K, int64_t ldo,
                                    int dtype, hx_stream stream) {
  if (N <= 0 || K <= 0) return HX_ERR_SHAPE;
  if (!out || !wq || !w_scale) return HX_ERR_NULL;
  if (N % kBlk || K % kBlk || K >= ((int64_t)1 << 31) || ldo % 8 != 0 || ldo < K) return HX_ERR_SHAPE;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  if (!aligned16(out) || !aligned16(wq) || ((uintptr_t)w_scale & 3u)) return HX_ERR_STRIDE;
  const int64_t n_pieces = N * K / 16;
  const unsigned blocks = (unsigned)((n_pieces + 255) / 256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == HX_F16)
    hx::launcher(dequant_fp8_block_kernel<F16>, blocks, 256, 0, s)((u16*)out, (const uint8_t*)wq, w_scale, n_pieces, (int)K, ldo);
  else
    hx::launcher(dequant_fp8_block_kernel<BF16>, blocks, 256, 0, s)((u16*)out, (const uint8_t*)wq, w_scale, n_pieces, (int)K, ldo);
  return check_launch();
}
