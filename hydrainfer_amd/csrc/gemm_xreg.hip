// gemm_xreg.hip — decode-batch (M <= 32) weight-streaming GEMM with the ACTIVATIONS IN REGISTERS:
//     partial[s][m][n] = sum_{k in split s} x[m][k] * W[n][k]         (fp32 slabs, usually ONE)
// the nn.Linear products of a decoder layer (hydrainfer/model/llama.py:24-27,48-50) at decode batch
// sizes.  gemm_skinny.hip keeps a 1024-wide slice of x in LDS, so K = 4096 needs 4 K-splits whose
// fp32 partial slabs (25 MB per 7B layer) cost 8.7 us of a 159 us layer in stores alone
// (tools/gemm_ablate.py) and force a reduce kernel behind every product.  Here:
//   * a workgroup is 4 waves and spans the WHOLE K of its split: wave w owns KW consecutive
//     k-steps (of 32) and keeps the x fragments of exactly those k-steps in registers (B operands:
//     KW * MB * 4 registers, 256 for K = 4096 at batch 32; one wave per SIMD, 512 registers each);
//   * the workgroup walks row groups rg = b, b + nb, b + 2 nb, ...; per row group a wave streams its
//     KW KiB of packed weight fragments (1 KiB contiguous per wave instruction, non-temporal)
//     through ceil(KW / 8) register buffers that are refilled for the NEXT row group as soon as they
//     are consumed: up to 32 KiB in flight per wave, 128 KiB per CU, no LDS and no barrier in the
//     loop;
//   * the four waves' partial tiles go to LDS; ONE barrier at the end of the workgroup's life, then
//     the tiles are summed in wave order (deterministic) and stored;
//   * waves start their k-steps at a workgroup-dependent rotation so that the fragments the chip
//     reads at one instant are spread over all memory channels (in lock-step they would sit
//     128 KiB apart).
// K <= 5120 needs no K-split at all (one slab); K = 11008 takes four (was 11), chosen per (N, K) so
// that every CU gets a workgroup (xreg_plan).
// Two extensions of the same kernel finish the operators around the product:
//   EPI = 1   gate|up + silu*mul: the packed gate and up row groups are interleaved, a workgroup owns
//             both halves of its columns and writes act = silu(gate) * up (hx_gate_up_silu_xreg);
//   NORM = 1  the add + RMSNorm that PRODUCES x runs inside the launch: the first M workgroups
//             compute one row each, publish x write-through and count themselves in; all workgroups
//             prefetch weights meanwhile, wait on their XCD's flag line, then load x.  Rows are
//             owned by whoever claims their state word first, and a workgroup that has waited 30 us
//             claims unstarted rows itself: progress needs ONE resident workgroup (hx_norm_*_xreg).
//             This hand-over is ONE text for both kernels, included into each: gemm_xreg_produce.inc (the
//             protocol is stated there) in front of the kernel's weight prefetch, gemm_xreg_wait.inc behind it.
// Activations between these launches are FRAGMENT-MAJOR (the order the B operands are loaded in;
// include/hydra_hip.h): row-major x makes every x load touch 16 cache lines for 16 bytes each.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <type_traits>
#include "attn_common.h"

namespace {

using namespace hx;

struct XregParams {
  const void* x;
  const void* w;        // packed: fragment (split s, row group rg, k-step j of the split) at KiB index
                        //         s*P*n_rg + rg*nks(s) + j,   P = 4*KW,  nks(s) = min(P, total_ks - s*P)
  float* partial;       // [S][M][N]
  int64_t ldx;
  int32_t M, N, K;
  int32_t stagger;      // bit 0: rotate the k-steps per workgroup; bit 1: test hook, NORM rows only via the rescue path
  int32_t x_packed;     // x is fragment-major: piece ((ks*MB + mb)*64 + lane) = x[16mb + (lane&15)][32ks + 8(lane>>4) ..+8]
  // NORM = 1: x is produced INSIDE the launch — workgroup r < M first computes row r of
  //   residual += (T) sum of the nm_splits slabs;  x = rms_norm(residual) * nm_weight   (hx_add_rms_norm_slabs)
  // and writes it fragment-major to `x` (write-through), the others prefetch weights meanwhile
  const float* nm_partial;   // [nm_splits][M][K]
  void* nm_residual;         // [M][K], in place
  const void* nm_weight;     // [K]
  uint32_t* sync;            // HX_XREG_SYNC_WORDS zeroed words: rows done, error word, one flag line per XCD, row states
  int32_t nm_splits;
  float nm_eps;
  void* act;            // EPI = 1: silu(gate)*up, fragment-major [inter/32][MB][64 lanes][8]
  int32_t interleaved;  // EPI = 0 over a gate|up packing (row groups gate, up, gate, ...): slab columns in [gate | up] order
  int32_t pk_P;         // wide kernel: k-steps per split of the PACKING (the launch's own splits are halves of those)
};

// KERNARG PRELOADING (round 5; Makefile: -mllvm -amdgpu-kernarg-preload-count=16).  A by-value struct parameter is read
// from the kernarg segment by s_loads at the kernel's start — a cold ~0.4 us round trip in front of the first address a
// wave can form, paid at every launch boundary (the math-free null layer got 0.39 us per launch faster with preloaded
// arguments, profiles/r5_kernarg_preload.md).  gfx950 can deliver the first 14 argument dwords in SGPRs WITH the wave,
// but only for scalar / pointer parameters: the kernels therefore take what their first loads need as leading
// scalars and the struct after them; the copy below lets the rest of the code keep reading `p.field`.
// The activations-in-registers kernels go further: NOTHING in front of their first loads comes from the struct.  Five pointer slots
// whose meaning depends on NORM (a norm-fused launch needs the producers' pointers first, x / partial / act late; a plain
// launch the other way round) and four packed integers — 14 dwords:
//   NORM = 0: p0 = w, p1 = x, p2 = partial, p3 = act            NORM = 1: p0 = w, p1 = nm_partial, p2 = nm_residual,
//                                                                          p3 = nm_weight, p4 = sync
//   a = N / 16 | grid.x << 16     b = K / 32 | M << 16 | x_packed << 24 | interleaved << 25
//   c = stagger | nm_splits << 8 | pk_P << 16 (wide kernel)       ldx (elements, < 2^31; NORM = 1: the bits of nm_eps instead)
struct XregHot {
  const void *p0, *p1, *p2, *p3, *p4;
  int32_t a, b, c, ldx;
};
template <int NORM>
inline bool xreg_hot(const XregParams& p, unsigned nb, XregHot* h) {
  if ((p.N >> 4) > 0xffff || nb > 0xffff || (p.K >> 5) > 0xffff || p.M > 255 || p.nm_splits > 255 || p.stagger > 255 ||
      p.pk_P > 0xffff || p.pk_P < 0 || p.ldx > 0x7fffffff || p.ldx < 0)
    return false;
  h->p0 = p.w;
  if (NORM) { h->p1 = p.nm_partial; h->p2 = p.nm_residual; h->p3 = p.nm_weight; h->p4 = p.sync; }
  else { h->p1 = p.x; h->p2 = p.partial; h->p3 = p.act; h->p4 = nullptr; }
  h->a = (int32_t)((uint32_t)(p.N >> 4) | (nb << 16));
  h->b = (int32_t)((uint32_t)(p.K >> 5) | ((uint32_t)p.M << 16) | ((uint32_t)(p.x_packed ? 1 : 0) << 24) | ((uint32_t)(p.interleaved ? 1 : 0) << 25));
  h->c = (int32_t)((uint32_t)p.stagger | ((uint32_t)p.nm_splits << 8) | ((uint32_t)p.pk_P << 16));
  h->ldx = NORM ? __builtin_bit_cast(int32_t, p.nm_eps) : (int32_t)p.ldx;      // (a norm-fused launch reads fragment-major x: no ldx)
  return true;
}

#define HX_XREG_HOT_SIG                                                                                             \
  const void* __restrict__ h_p0, const void* __restrict__ h_p1, const void* __restrict__ h_p2,                        \
      const void* __restrict__ h_p3, const void* __restrict__ h_p4, const int32_t h_a, const int32_t h_b,            \
      const int32_t h_c, const int32_t h_ldx
#define HX_XREG_UNPACK_HOT(NORM_)                                                                                   \
  XregParams p = p_in;                                                                                              \
  p.w = h_p0;                                                                                                       \
  if (NORM_) {                                                                                                      \
    p.nm_partial = reinterpret_cast<const float*>(h_p1); p.nm_residual = const_cast<void*>(h_p2); p.nm_weight = h_p3; \
    p.sync = reinterpret_cast<uint32_t*>(const_cast<void*>(h_p4));                                                  \
  } else {                                                                                                          \
    p.x = h_p1; p.partial = reinterpret_cast<float*>(const_cast<void*>(h_p2)); p.act = const_cast<void*>(h_p3);     \
  }                                                                                                                 \
  p.N = (h_a & 0xffff) << 4; p.K = (h_b & 0xffff) << 5; p.M = (h_b >> 16) & 0xff; p.x_packed = (h_b >> 24) & 1;     \
  p.interleaved = (h_b >> 25) & 1; p.stagger = h_c & 0xff; p.nm_splits = (h_c >> 8) & 0xff;                         \
  p.pk_P = (int32_t)((uint32_t)h_c >> 16);                                                                          \
  if (NORM_) p.nm_eps = __builtin_bit_cast(float, h_ldx);                                                           \
  else p.ldx = h_ldx;                                                                                               \
  const int h_nb = (int)((uint32_t)h_a >> 16);      /* gridDim.x (from the hidden arguments it would be one more s_load) */

__device__ __forceinline__ float silu_f32(float x) { return x / (1.0f + __expf(-x)); }

__device__ __attribute__((aligned(128))) u16 g_zero_line[64] = {0};

static_assert(HX_XREG_SYNC_WORDS >= 320 + 32, "sync area: word 0 arrivals, word 1 error, word 32*(1+xcc) the flag line of that XCD");
constexpr int kXAux = 16;     // cache policy of the x loads behind the hand-over: 16 = sc1 (past the XCD's L2); 0 = plain (L2 hits after
                              // an XCD's first reader) was measured again in round 5: first row group, kernel end and step unchanged — the
                              // 256 KiB per CU are bound by the CU's own 64 B/clk, not by where they come from
constexpr int kStateWord = 320;        // sync area: one ownership word per row (<= 32)
constexpr uint64_t kRescueTicks = 3000;   // 30 us of the 100 MHz clock (a normal wait is ~3 us)
constexpr int kMaxG = 16;

typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef unsigned int bu32x4 __attribute__((__vector_size__(16)));
__device__ __forceinline__ rsrc_t make_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}

// hx_add_rms_norm_slabs for ONE row by 256 threads, bit-identical to add_rms_norm_slab_kernel<T, MAXV, 512>:
// thread u plays its virtual threads u and u + 256 (same per-thread sums, same wave sums, same order of
// the eight wave sums).  x goes out fragment-major with sc1 (write-through) stores.
// OWNERSHIP: a row is computed by whoever first exchanges its state word 0 -> 1 (thread 0; the answer
// travels with the reduction barrier, so claiming costs no extra round trip); everybody else returns
// false without having stored anything — the residual is updated exactly once.
template <typename T, int MAXV, int MB, int KB = 6>      // KB: slab pieces requested per round trip (the wide kernel's down hands over 8)
__device__ __forceinline__ bool norm_row_256(const float* __restrict__ partial, int n_splits, int64_t slab_stride,
                                             u16* __restrict__ residual, const u16* __restrict__ weight, float eps,
                                             int hidden, int row, void* x_frag, uint32_t* state, float* red,
                                             int mb_layout = MB) {   // 16-row blocks of the fragment-major x: ceil(M / 16)
  const int tid = threadIdx.x;
  const int nvec = hidden / 8;
  uint32_t claimed = 1;
  if (tid == 0) claimed = __hip_atomic_exchange(state + row, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  u16x8* res_v = reinterpret_cast<u16x8*>(residual + (int64_t)row * hidden);
  const u16x8* w_v = reinterpret_cast<const u16x8*>(weight);
  float x[2 * MAXV][8];
  float ss[2] = {0.f, 0.f};
  u16x8 rr[2 * MAXV], ww[2 * MAXV], hh[2 * MAXV];
#pragma unroll
  for (int v = 0; v < 2; ++v)
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      const int i = min(tid + 256 * v + 512 * j, nvec - 1);
      rr[v * MAXV + j] = res_v[i];
      ww[v * MAXV + j] = w_v[i];
    }
#pragma unroll
  for (int v = 0; v < 2; ++v) {
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      const int i = tid + 256 * v + 512 * j;
      if (i < nvec) {
        // slab pieces: all loads of a batch of 6 splits before the first add, adds in split order
        // (norm_rope_act.hip slab_sum8)
        const float* pp = partial + (int64_t)row * hidden + i * 8;
        constexpr int kB = KB;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < n_splits; s0 += kB) {
          f32x4 pa[kB], pb[kB];
#pragma unroll
          for (int k = 0; k < kB; ++k) {
            const int sp = min(s0 + k, n_splits - 1);
            pa[k] = *reinterpret_cast<const f32x4*>(pp + sp * slab_stride);
            pb[k] = *reinterpret_cast<const f32x4*>(pp + sp * slab_stride + 4);
          }
#pragma unroll
          for (int k = 0; k < kB; ++k) {
            if (s0 + k == 0) { a = pa[0]; b = pb[0]; }
            else if (s0 + k < n_splits) { a += pa[k]; b += pb[k]; }
          }
        }
        const u16x8 r = rr[v * MAXV + j];
        u16x8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float sum = round_to<T>(round_to<T>(e < 4 ? a[e] : b[e - 4]) + T::to_float(r[e]));
          x[v * MAXV + j][e] = sum;
          h[e] = T::from_float(sum);
          ss[v] += sum * sum;
        }
        hh[v * MAXV + j] = h;
      }
    }
  }
  const float t0 = wave_sum(ss[0]), t1 = wave_sum(ss[1]);
  if ((tid & 63) == 0) {
    red[tid >> 6] = t0;
    red[4 + (tid >> 6)] = t1;
  }
  if (tid == 0) red[8] = claimed == 0u ? 1.f : 0.f;
  __syncthreads();
  const bool own = red[8] != 0.f;
  float total = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) total += red[k];
  const float inv = rsqrtf(total / (float)hidden + eps);
  if (own) {
    const rsrc_t xrs = make_rsrc(x_frag);      // (built here: x's pointer is not among the preloaded arguments)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
#pragma unroll
      for (int j = 0; j < MAXV; ++j) {
        const int i = tid + 256 * v + 512 * j;
        if (i < nvec) {
          res_v[i] = hh[v * MAXV + j];
          const u16x8 w = ww[v * MAXV + j];
          u16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            o[e] = T::from_float(round_to<T>(x[v * MAXV + j][e] * inv) * T::to_float(w[e]));
          // fragment-major piece ((i / 4) * MB + row / 16) * 64 + (i % 4) * 16 + row % 16
          const uint32_t piece = (uint32_t)((i >> 2) * mb_layout + (row >> 4)) * 64 + (i & 3) * 16 + (row & 15);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bu32x4, o), xrs, piece * 16, 0, 16);
        }
      }
    }
  }
  __syncthreads();   // red[] may be reused by the caller / the next row
  return own;
}

// EPI = 0: fp32 slabs.  EPI = 1 (one split only): the weight is a gate|up projection packed with its
// 16-row groups interleaved (group 2j = gate rows 16j.., group 2j+1 = up rows 16j..); a workgroup
// takes whole pairs and writes act = silu(gate) * up with the rounding of hx_silu_and_mul_slabs on the
// one-slab result (sum -> T, silu -> T, product -> T), fragment-major for the down projection.
template <typename T, int MB, int KW, int EPI = 0, int DBG = 0, int NORM = 0, int RM = 0>
__global__ __launch_bounds__(256) void gemm_xreg_kernel(HX_XREG_HOT_SIG, const XregParams p_in) {
  HX_XREG_UNPACK_HOT(NORM)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NBUF = (KW + 7) / 8;
  constexpr int P = 4 * KW;
  constexpr int mbl = MB;      // 16-row blocks of the fragment-major x
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  // Work is numbered from the END of the grid: row groups (pairs) are dealt round-robin, so the workgroups that go
  // short in the last, partial round are the FIRST ones of the grid — in a NORM launch the producers of x, which start
  // their own row groups ~3 us after everybody else (tools/xreg_timeline.py: with a full share they were the launch's
  // tail, 32.3 us against ~28 for the others in the 7B gate|up launch).  The same numbering in every form of the
  // kernel: the k-step rotation (stagger) follows it, and with it the summation order of a row group.
  const int split = blockIdx.y, nb = h_nb, b = nb - 1 - (int)blockIdx.x;
  const int total_ks = p.K >> 5;
  const int n_rg = p.N >> 4;
  const int ks0 = split * P;
  const int nks = min(P, total_ks - ks0);
  const int kw = max(0, min(KW, nks - w * KW));            // this wave's real k-steps
  // this workgroup's row groups (>= 1): rg_of(0), rg_of(1), ...
  const int G = EPI ? 2 * (((n_rg >> 1) - b + nb - 1) / nb) : (n_rg - b + nb - 1) / nb;
  auto rg_of = [&](int i) { return EPI ? 2 * (b + (i >> 1) * nb) + (i & 1) : b + i * nb; };
  const int j0 = (p.stagger & 1) ? (int)(((unsigned)b * 7u + (unsigned)w * 3u) % (unsigned)KW) : 0;
  // bit 3 of `stagger` (hx_debug_set_option("xreg_timeline", 1); NORM launches only): the first and the last workgroup
  // of the grid write 100 MHz time stamps of their phases into words 384.. of the sync area (tools/xreg_timeline.py)
  const int flat_id = blockIdx.y * nb + blockIdx.x;
  auto stamp = [&](int k) {
    if (NORM && (p.stagger & 8) && threadIdx.x == 0 && (flat_id == 0 || flat_id == (int)(nb * (NORM ? 1u : gridDim.y)) - 1))
      reinterpret_cast<unsigned long long*>(p.sync + 384 + (flat_id ? 32 : 0))[k] = __builtin_amdgcn_s_memrealtime();
  };
  stamp(0);

  // k-step of slot t: rot(t) = (j0 + t) mod KW; slots whose k-step is past the wave's range are
  // padding: x fragment zero, weight address clamped to a valid fragment
  auto rot = [&](int t) { const int r = j0 + t; return r >= KW ? r - KW : r; };
  // RM = 1: the weight is the ROW-MAJOR [N][K] tensor itself (the one the library prefill GEMMs read: an E/P/EPD node
  // then holds ONE copy).  The fragment of (row group, k-step) is then 16 rows x 64 bytes, lane (c, g) at row c, bytes
  // 16 g: the same elements in the same lanes as the packed fragment, so the sums are bit-identical.
  constexpr int64_t jstride = RM ? 32 : 512;
  const u16* wbase = RM ? reinterpret_cast<const u16*>(p.w) + (int64_t)c * p.K + 8 * g + (int64_t)ks0 * 32
                        : reinterpret_cast<const u16*>(p.w) + 8 * lane + ((int64_t)ks0 * n_rg) * 512;
  auto rg_off = [&](int rg) -> int64_t {
    if constexpr (!RM) return (int64_t)rg * nks * 512;
    else if (EPI || p.interleaved) return ((int64_t)(rg & 1) * (p.N >> 1) + (int64_t)(rg >> 1) * 16) * p.K;
    else return (int64_t)rg * 16 * p.K;
  };
  const int wave_k0 = min(w * KW, max(nks - 1, 0));
  auto frag_ptr = [&](int rg, int t) {
    const int r = rot(t);
    const int j = wave_k0 + (r < kw ? r : 0);
    return wbase + rg_off(rg) + j * jstride;
  };

  u16x8 buf[NBUF][8];
  auto load_buf = [&](int rg, int q) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (8 * q + j < KW) buf[q][j] = __builtin_nontemporal_load(reinterpret_cast<const u16x8*>(frag_ptr(rg, 8 * q + j)));
  };
  // x fragments of this wave's k-steps, in slot order.  Prologue order: for each block of 8 slots,
  // its x fragments, then its weight buffer — the first MFMAs need only the first block, so the
  // x broadcast (256 KiB per CU out of the XCD's L2, ~2 us chip-wide) overlaps the arrival of the
  // first weights instead of preceding it.  No use of a loaded value before the first MFMA
  // (padding slots read a zero line instead of being masked: a select on the loaded value made
  // hipcc wait for every earlier load after each of these).
  u16x8 xb[KW][MB];
  const u16* xp = reinterpret_cast<const u16*>(p.x) + 8 * g;
  const u16* zp = reinterpret_cast<const u16*>(g_zero_line) + 8 * g;
#include "gemm_xreg_load_x.inc"
  if (NORM) {
    constexpr int kNormMaxV = (KW + 31) / 32, kNormKB = 6;
    const int n_wg = nb;      // (a norm-fused launch has ONE split: gridDim.y == 1)
#include "gemm_xreg_produce.inc"
    stamp(1);
    // 2. everyone: weight prefetch (independent of x).  (Round 3, tools/xreg_timeline.py: a producer sees the flag 3 us
    //    later than the others — its first poll returns behind its own prefetch, loads return in order — but letting it
    //    poll first and request its weights afterwards only moves the wait: its first row group ends at 15 us either way.)
#pragma unroll
    for (int q = 0; q < NBUF; ++q) load_buf(rg_of(0), q);
    __builtin_amdgcn_sched_barrier(0);
#include "gemm_xreg_wait.inc"
    {      // 4. x
      const int &x_ks0 = ks0, &x_kw = kw;      // (by reference, here and in the wide kernel: as copies they change its SGPR spill lanes)
#include "gemm_xreg_load_x_norm.inc"
    }
    __builtin_amdgcn_sched_barrier(0);
  } else {
#pragma unroll
    for (int q = 0; q < NBUF; ++q) {
      load_x_block(q);
      load_buf(rg_of(0), q);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  f32x4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4* slot = reinterpret_cast<f32x4*>(smem) + (w * MB) * 64 + lane;   // + i*4*MB*64 + mb*64

  auto row_group = [&](int i, auto refill_tag) {
    constexpr bool REFILL = decltype(refill_tag)::value;
    const int rg_next = rg_of(i + 1);
#pragma unroll
    for (int q = 0; q < NBUF; ++q) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (8 * q + j < KW) {
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) acc[mb] = Mfma<T>::mma(buf[q][j], xb[8 * q + j][mb], acc[mb]);
        }
      }
      // refill behind this buffer's MFMAs (hoisted loads would need fresh registers: spills)
      __builtin_amdgcn_sched_barrier(0);
      if (REFILL) load_buf(rg_next, q);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      slot[(i * 4 * MB + mb) * 64] = acc[mb];
      acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  for (int i = 0; i < G - 1; ++i) { row_group(i, std::true_type{}); if (i < 6) stamp(3 + i); }
  row_group(G - 1, std::false_type{});
  stamp(10);
  if ((DBG & 2) && acc[0][0] != 123.25f) return;   // ablation: no reduction, no stores
  __syncthreads();

  // tile (i, mb) is summed by wave (i*MB + mb) % 4 over the four waves in order
  const f32x4* tiles = reinterpret_cast<const f32x4*>(smem) + lane;
  auto tile_sum = [&](int i, int mb) {
    f32x4 s = tiles[((i * 4 + 0) * MB + mb) * 64];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) s += tiles[((i * 4 + ww) * MB + mb) * 64];
    return s;
  };
  if (EPI == 0) {
    for (int pr = w; pr < G * MB; pr += 4) {
      const int i = pr / MB, mb = pr - i * MB;
      const f32x4 s = tile_sum(i, mb);
      const int m = mb * 16 + c;
      const int rg = rg_of(i);
      const int col = p.interleaved ? ((rg & 1) ? (p.N >> 1) : 0) + ((rg >> 1) << 4) : (rg << 4);
      if (m < p.M) *reinterpret_cast<f32x4*>(p.partial + ((int64_t)split * p.M + m) * p.N + col + 4 * g) = s;
    }
  } else {
    for (int pr = w; pr < (G >> 1) * MB; pr += 4) {
      const int ip = pr / MB, mb = pr - ip * MB;
      const f32x4 gt = tile_sum(2 * ip, mb), up = tile_sum(2 * ip + 1, mb);
      u16x4 r;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        r[e] = T::from_float(round_to<T>(silu_f32(round_to<T>(gt[e]))) * round_to<T>(up[e]));
      // act[m = 16mb + c][k = 16j + 4g + e], j = pair index: piece ((k/32)*MB + mb)*64 + ((k%32)/8)*16 + c, element k%8
      const int k = 16 * (b + ip * nb) + 4 * g;
      u16* dst = reinterpret_cast<u16*>(p.act) + ((((int64_t)(k >> 5) * MB + mb) * 64 + ((k & 31) >> 3) * 16 + c) << 3) + (k & 7);
      if (mb * 16 + c < p.M) *reinterpret_cast<u16x4*>(dst) = r;      // rows M .. of the last block stay as they are (like the slabs' and the wide kernel's)
    }
  }
  stamp(11);
}

// ------------------------------------------------------------------------------------------------------------
// The same kernel for decode batches of 33 .. 64 rows ("wide": MB = 4).  x for 64 rows is twice the registers, so a
// workgroup spans HALF of a packed K split (KW = half the packing's k-steps per wave: the SAME packed weights serve
// both batch ranges — no second copy) and writes twice the slabs; to keep 32 KiB per wave in flight a work unit is a
// PAIR of 16-row groups (two A fragments per k-step share the four x fragments).  The four waves' tiles are summed
// through LDS after every unit (one barrier per unit, two tile sets used alternately) — a share of up to 11 units
// would not fit LDS at 16 KiB each.  EPI = 0 only (silu*mul needs the whole K: hx_silu_and_mul_slabs behind it);
// NORM: the same hand-over text, with up to 64 producers.  Same k-step rotation and summation order per split.
// Round 5: (a) a launch split is HALF of a packing split in the general sense — split s = (packing split s / 2, half
// s % 2), the first half takes P = 4 KW k-steps, the second one what is left of the packing split (LLaVA-1.5-13B's down
// projection: 27 k-steps per wave in the packing -> halves of 14 and 13); (b) RG = row groups per work unit: 2 keeps
// 2 KW KiB per wave in flight; RG = 1 is for KW = 20 (13B's K = 5120: x for 64 rows is 320 registers, a second weight
// buffer set does not fit beside it).
// EPI = 1 (round 5; RG = 2, NORM = 1, a gate|up packing whose split is two halves): BOTH K halves in one workgroup, one
// after the other — x of the first half, all of the workgroup's units (their reduced tiles wait in LDS, 8 KiB per unit), x of
// the second half, the units again, and act = silu(gate) * up leaves from the epilogue with hx_silu_and_mul_slabs' order of
// summation and roundings.  No slabs, no silu*mul launch, nothing between workgroups; the weight stream runs on across
// the seam (the last unit of the first half refills with the first unit of the second).  gridDim.y == 1.
template <typename T, int KW, int NORM, int RG = 2, int EPI = 0>
__global__ __launch_bounds__(256) void gemm_xreg_wide_kernel(HX_XREG_HOT_SIG, const XregParams p_in) {
  HX_XREG_UNPACK_HOT(NORM)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int MB = 4, NBUF = (KW + 7) / 8, P = 4 * KW;
  static_assert(!EPI || (RG == 2 && NORM == 1), "the two-pass form: (gate, up) pairs, norm-fused");
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, c = lane & 15;
  const int split = EPI ? 0 : (int)blockIdx.y, nb = h_nb, b = nb - 1 - (int)blockIdx.x;
  const int total_ks = p.K >> 5;
  const int n_rg = p.N >> 4, n_un = n_rg / RG;
  // where the launch's split sits inside the packing
  const int sp = split >> 1, off_in = (split & 1) * P;
  const int nks_p = min(p.pk_P, total_ks - sp * p.pk_P);
  const int ks0 = sp * p.pk_P + off_in;
  const int nks = max(0, min(P, nks_p - off_in));
  const int kw = max(0, min(KW, nks - w * KW));
  const int G = (n_un - b + nb - 1) / nb;                  // this workgroup's units (>= 1): b, b + nb, ...
  const int mbl = (p.M + 15) >> 4;                         // 16-row blocks of the fragment-major x (3 for 33 .. 48 rows): the
                                                           // fourth MFMA column block then re-reads the third (rows >= M are never stored)
  const int j0 = (p.stagger & 1) ? (int)(((unsigned)b * 7u + (unsigned)w * 3u) % (unsigned)KW) : 0;
  const int flat_id = blockIdx.y * nb + blockIdx.x;
  auto stamp = [&](int k) {      // (xreg_timeline, as in the 32-row kernel: first and last workgroup of a norm-fused launch)
    if (NORM && (p.stagger & 8) && threadIdx.x == 0 && (flat_id == 0 || flat_id == (int)(nb * gridDim.y) - 1))
      reinterpret_cast<unsigned long long*>(p.sync + 384 + (flat_id ? 32 : 0))[k] = __builtin_amdgcn_s_memrealtime();
  };
  stamp(0);
  auto rot = [&](int t) { const int r = j0 + t; return r >= KW ? r - KW : r; };
  const u16* wbase = reinterpret_cast<const u16*>(p.w) + 8 * lane + ((int64_t)sp * p.pk_P * n_rg) * 512;
  const int wave_k0 = off_in + min(w * KW, max(nks - 1, 0));
  // what depends on the K half: first k-step, this wave's k-step count, its first k-step inside the packing split
  struct PassK { int ks0, kw, wk0; };
  const PassK pa{ks0, kw, wave_k0};
  const int nks_b = max(0, min(P, nks_p - P));                       // (EPI: the second half)
  const PassK pb{ks0 + P, max(0, min(KW, nks_b - w * KW)), P + min(w * KW, max(nks_b - 1, 0))};
  auto frag_ptr = [&](int rg, int t, const PassK& ps) {
    const int r = rot(t);
    return wbase + ((int64_t)rg * nks_p + ps.wk0 + (r < ps.kw ? r : 0)) * 512;
  };
  u16x8 buf[RG][NBUF][8];
  auto load_buf = [&](int unit, int q, const PassK& ps) {
#pragma unroll
    for (int h = 0; h < RG; ++h)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (8 * q + j < KW)
          buf[h][q][j] = __builtin_nontemporal_load(reinterpret_cast<const u16x8*>(frag_ptr(RG * unit + h, 8 * q + j, ps)));
  };
  auto unit_of = [&](int i) { return b + i * nb; };
  u16x8 xb[KW][MB];
  const u16* xp = reinterpret_cast<const u16*>(p.x) + 8 * g;
  const u16* zp = reinterpret_cast<const u16*>(g_zero_line) + 8 * g;
  constexpr int DBG = 0;      // (no ablation variants of this kernel)
#include "gemm_xreg_load_x.inc"
  if (NORM) {
    constexpr int kNormMaxV = (2 * KW + 31) / 32, kNormKB = 8;      // (the down projection hands over 8 slabs)
    const int n_wg = nb * (int)gridDim.y;
#include "gemm_xreg_produce.inc"
#pragma unroll
    for (int q = 0; q < NBUF; ++q) load_buf(unit_of(0), q, pa);
    __builtin_amdgcn_sched_barrier(0);
    stamp(1);      // (behind the prefetch here, in front of it in the 32-row kernel)
#include "gemm_xreg_wait.inc"
  }
  auto load_x_norm = [&](const PassK& ps) {      // the produced x of one K half
    const int &x_ks0 = ps.ks0, &x_kw = ps.kw;
#include "gemm_xreg_load_x_norm.inc"
  };
  if (NORM) {
    load_x_norm(pa);
    __builtin_amdgcn_sched_barrier(0);
  } else {
#pragma unroll
    for (int q = 0; q < NBUF; ++q) {
      load_x_block(q);
      load_buf(unit_of(0), q, pa);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  f32x4 acc[RG][MB];
#pragma unroll
  for (int h = 0; h < RG; ++h)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[h][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  // tile (set, row group h of the unit, wave, mb): 1 KiB each
  f32x4* tiles = reinterpret_cast<f32x4*>(smem) + lane;
  // one unit's MFMAs; behind every block of eight k-steps its buffers are requested again for (u_next, ps_next)
  auto mfma_unit = [&](auto refill_tag, int u_next, const PassK& ps_next) {
    constexpr bool REFILL = decltype(refill_tag)::value;
#pragma unroll
    for (int q = 0; q < NBUF; ++q) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (8 * q + j < KW) {
#pragma unroll
          for (int h = 0; h < RG; ++h)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) acc[h][mb] = Mfma<T>::mma(buf[h][q][j], xb[8 * q + j][mb], acc[h][mb]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (REFILL) load_buf(u_next, q, ps_next);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // the four waves' tiles of a unit summed in wave order: wave w ends up with tile (h, mb) = ((w + 4 k) >> 2, (w + 4 k) & 3)
  // in sum[k]; tile sets alternate, so one barrier per unit is enough (plain loads in flight survive it)
  auto reduce_unit = [&](int set, f32x4 (&sum)[RG]) {
#pragma unroll
    for (int h = 0; h < RG; ++h)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        tiles[(((set * RG + h) * 4 + w) * MB + mb) * 64] = acc[h][mb];
        acc[h][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RG; ++k) {
      const int tt = w + 4 * k, h = tt >> 2, mb = tt & 3;
      sum[k] = tiles[(((set * RG + h) * 4 + 0) * MB + mb) * 64];
#pragma unroll
      for (int ww = 1; ww < 4; ++ww) sum[k] += tiles[(((set * RG + h) * 4 + ww) * MB + mb) * 64];
    }
  };
  if constexpr (!EPI) {
    auto unit = [&](int i, auto refill_tag) {
      mfma_unit(refill_tag, unit_of(i + 1), pa);
      f32x4 sum[RG];
      reduce_unit(i & 1, sum);
#pragma unroll
      for (int k = 0; k < RG; ++k) {
        const int tt = w + 4 * k, h = tt >> 2, mb = tt & 3;
        const int rg = RG * unit_of(i) + h;
        const int col = p.interleaved ? ((rg & 1) ? (p.N >> 1) : 0) + ((rg >> 1) << 4) : (rg << 4);
        const int m = mb * 16 + c;
        if (m < p.M) *reinterpret_cast<f32x4*>(p.partial + ((int64_t)split * p.M + m) * p.N + col + 4 * g) = sum[k];
      }
    };
    for (int i = 0; i < G - 1; ++i) { unit(i, std::true_type{}); if (i < 6) stamp(3 + i); }
    unit(G - 1, std::false_type{});
  } else {
    // first K half: the units' reduced tiles go to LDS (wave-private pieces: the same wave adds the second half to them)
    f32x4* part = reinterpret_cast<f32x4*>(smem + 2 * RG * 4 * MB * 1024) + lane;
    int n_red = 0;
    for (int i = 0; i < G; ++i) {
      const bool seam = i + 1 == G;
      mfma_unit(std::true_type{}, seam ? unit_of(0) : unit_of(i + 1), seam ? pb : pa);
      f32x4 sum[RG];
      reduce_unit(n_red++ & 1, sum);
#pragma unroll
      for (int k = 0; k < RG; ++k) part[((i * RG + k) * 4 + w) * 64] = sum[k];
      if (i < 3) stamp(3 + i);
    }
    load_x_norm(pb);
    __builtin_amdgcn_sched_barrier(0);
    // second K half, then act[m][16 u + 4 g ..+4] = T(T(silu(T(g0 + g1))) * T(u0 + u1)); wave w holds row block w of both
    // the gate tile (k = 0) and the up tile (k = 1)
    auto finish = [&](int i, auto refill_tag) {
      mfma_unit(refill_tag, unit_of(i + 1), pb);
      f32x4 sum[RG];
      reduce_unit(n_red++ & 1, sum);
      f32x4 gt = part[((i * RG + 0) * 4 + w) * 64], up = part[((i * RG + 1) * 4 + w) * 64];
      gt += sum[0];
      up += sum[1];
      const int m = w * 16 + c;
      if (m < p.M) {
        u16x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          r[e] = T::from_float(round_to<T>(silu_f32(round_to<T>(gt[e]))) * round_to<T>(up[e]));
        // piece ((k / 32) * mbl + m / 16) * 64 + ((k % 32) / 8) * 16 + m % 16, element k % 8
        const int k = (unit_of(i) << 4) + 4 * g;
        u16* dst = reinterpret_cast<u16*>(p.act) + ((((int64_t)(k >> 5) * mbl + w) * 64 + ((k & 31) >> 3) * 16 + c) << 3) + (k & 7);
        *reinterpret_cast<u16x4*>(dst) = r;
      }
    };
    for (int i = 0; i < G - 1; ++i) { finish(i, std::true_type{}); if (i < 3) stamp(6 + i); }
    finish(G - 1, std::false_type{});
  }
  stamp(11);
}

// output piece i (16 bytes) of the packed tensor <- its source in the row-major weight
__global__ __launch_bounds__(256) void pack_xreg_kernel(u16* __restrict__ packed, const u16* __restrict__ w,
                                                        int64_t n_pieces, int total_ks, int n_rg, int64_t ldw, int P,
                                                        int interleave) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pieces) return;
  const int lane = (int)(i & 63);
  const int64_t blk = i >> 6;                                   // KiB index
  const int64_t per_split = (int64_t)P * n_rg;
  const int split = (int)(blk / per_split);
  const int ks0 = split * P;
  const int nks = min(P, total_ks - ks0);
  const int64_t rem = blk - (int64_t)ks0 * n_rg;
  const int64_t rg = rem / nks;
  const int s = ks0 + (int)(rem % nks);
  // interleave: packed group 2j = source group j (gate), 2j+1 = source group n_rg/2 + j (up)
  const int64_t srg = interleave ? (rg >> 1) + ((rg & 1) ? (n_rg >> 1) : 0) : rg;
  const u16* src = w + (16 * srg + (lane & 15)) * ldw + 32 * s + 8 * (lane >> 4);
  *reinterpret_cast<u16x8*>(packed + i * 8) = *reinterpret_cast<const u16x8*>(src);
}

int g_stagger = 1;
int g_no_producers = 0;   // test hook (xreg_no_producers): 1 = the norm-fused launches rely on the rescue path alone; 2 = no producers and no rescue: every such launch gives up (error word) after 2 ms
int g_dbg = 0;
int g_row_major = 0;   // EXPERIMENTS builds (xreg_row_major): every 32-row launch reads its weight argument as the row-major [N][K] tensor
int g_timeline = 0;      // diagnostic (xreg_timeline): phase time stamps of the NORM launches into their sync areas
int g_force_wgs = 0;     // tuning: cap on workgroups per launch (0 = the CU count)

int stagger_bits() {
  return (g_stagger ? 1 : 0) | (g_no_producers == 1 ? 2 : 0) | (g_no_producers == 2 ? 4 : 0) | (g_timeline ? 8 : 0) | (g_row_major ? 16 : 0);
}

// ---- what is built -------------------------------------------------------------------------------------------
// The instantiations of the two kernels by k-steps per wave (KW).  The plain product (EPI = 0, NORM = 0) is built
// for every row; `norm` / `silu`: NORM = 1 / EPI = 1 are built too (wide kernel: the silu epilogue only behind the
// norm).  round_kw, the dispatch below and the plan's predicates all read these tables — a new KW is one row.
struct XregBuilt { int kw; bool norm, silu; };
constexpr XregBuilt kNarrowBuilt[] = {{4, true, true},    {8, true, true},    {16, true, true},   {20, false, false}, {22, false, false},
                                      {27, false, false}, {29, false, false}, {32, true, true},   {40, true, true}};
constexpr XregBuilt kWideBuilt[] = {{2, true, false},   {4, true, false},   {8, true, false}, {10, false, false},
                                    {11, false, false}, {14, false, false}, {16, true, true}, {20, true, false}};
constexpr bool is_built(const XregBuilt& r, bool wide, int epi, int norm) {
  return (!norm || r.norm) && (!epi || (r.silu && (norm || !wide)));
}
template <size_t n>
const XregBuilt* find_built(const XregBuilt (&table)[n], int kw) {
  for (const XregBuilt& r : table) if (r.kw == kw) return &r;
  return nullptr;
}
int round_kw(int kw) {
  for (const XregBuilt& r : kNarrowBuilt) if (r.kw >= kw) return r.kw;
  return 0;
}
constexpr int wide_rg(int kw) { return kw == 20 ? 1 : 2; }      // row groups per work unit (the wide kernel's RG)

// ---- the plan: ONE description of a launch; every entry point answers from it -------------------------------
struct XregPlan {
  int64_t M = 0, N = 0, K = 0;
  bool gate_up = false;      // the packing: gate and up row groups interleaved (N = 2 * inter), never the extra split
  bool wide = false;         // the kernel: gemm_xreg_wide_kernel (<= 64 rows) over the same packing, else gemm_xreg_kernel (<= 32)
  bool valid = false;
  int S = 0, KW = 0;         // the launch: K splits (the slabs of a plain product) and k-steps per wave
  int pk_S = 0, pk_P = 0;    // the packing: its splits and k-steps per split (the wide kernel's splits are halves of those)
  const XregBuilt* built = nullptr;      // the table row of KW
};

// The packing's (splits, k-steps per wave): the fewest splits whose per-wave share fits the register budget
// (KW <= 40), or one more when fewer than 80 % of the CUs would get a workgroup and the extra split fills more (one
// workgroup per CU: K = 11008 with N = 4096 runs 192 workgroups at 3 splits, 256 at 4) without padding more than 4 %
// of the k-steps.  HX_XREG_S="K:S;K:S" overrides the split count per K (tuning).
// The wide kernel's launch split s = (packing split s / 2, half s % 2) with half the k-steps per wave.
XregPlan xreg_plan(int64_t M, int64_t N, int64_t K, bool gate_up, bool wide) {
  XregPlan pl;
  pl.M = M; pl.N = N; pl.K = K; pl.gate_up = gate_up; pl.wide = wide;
  if (M < 1 || M > (wide ? 64 : 32) || N <= 0 || K <= 0 || N % (wide ? 32 : 16) || K % 32) return pl;
  const int total_ks = (int)(K >> 5);
  const int n_rg = (int)(N >> 4);
  const int s0 = (total_ks + 159) / 160;   // KW <= 40
  auto kw_of = [&](int s) { return round_kw(((total_ks + s - 1) / s + 3) / 4); };
  auto wgs_of = [&](int s) {
    int nb = n_cus() / s;
    if (nb < 1) nb = 1;
    if (nb > n_rg) nb = n_rg;
    const int G = (n_rg + nb - 1) / nb;
    return s * ((n_rg + G - 1) / G);
  };
  int s = s0;
  if (!gate_up) {   // the fused gate|up epilogue needs ONE split: it never takes the extra one
    // padded k-steps (per cent over the real ones) of a split count: what the padding waves re-read
    auto waste_pct = [&](int sc) {
      const int kw = kw_of(sc);
      if (kw <= 0) return 1000;
      const int used = (total_ks + 4 * kw - 1) / (4 * kw);
      return used != sc ? 1000 : (int)(((int64_t)used * 4 * kw * 100) / total_ks) - 100;
    };
    const int w0 = waste_pct(s0), w1 = waste_pct(s0 + 1);
    if (w1 <= 4 && (w0 > 4 ||                                                   // K = 13824: 3 splits pad 11 %, 4 are exact
                    (wgs_of(s0) * 5 < n_cus() * 4 && wgs_of(s0 + 1) > wgs_of(s0))))   // K = 11008, N = 4096: 192 -> 256 workgroups
      s = s0 + 1;
  }
  static const char* env = getenv("HX_XREG_S");
  if (env) {
    const char* q = env;
    while (*q) {
      long k = 0, sv = 0;
      if (sscanf(q, "%ld:%ld", &k, &sv) == 2 && k == K && sv >= s0 && sv <= 16) s = (int)sv;
      const char* semi = strchr(q, ';');
      if (!semi) break;
      q = semi + 1;
    }
  }
  const int kwp = kw_of(s);
  if (kwp <= 0) return pl;
  pl.pk_P = 4 * kwp;
  pl.pk_S = (total_ks + pl.pk_P - 1) / pl.pk_P;      // the splits that actually hold data
  if (!wide) {
    pl.S = pl.pk_S; pl.KW = kwp;
    pl.built = find_built(kNarrowBuilt, kwp);
  } else {
    pl.KW = (kwp + 1) / 2;      // an odd packing count halves unevenly: 27 -> 14 + 13 (LLaVA-1.5-13B's down projection)
    pl.built = find_built(kWideBuilt, pl.KW);
    // only the last packing split can be partial, so the launch splits that hold k-steps are a prefix of their numbering
    for (int q = 0; q < pl.pk_S; ++q) pl.S += std::min(pl.pk_P, total_ks - q * pl.pk_P) > 4 * pl.KW ? 2 : 1;
  }
  pl.valid = pl.built != nullptr;
  return pl;
}

// Grid and dynamic LDS of the plan's launch (epi: with the silu epilogue) — what the launch uses, and what a
// predicate asks when the answer depends on the device's CU count.
struct XregGrid { int nb = 0, S = 0; size_t lds = 0; bool ok = false; };
XregGrid xreg_grid(const XregPlan& pl, bool epi) {
  XregGrid g;
  const int per_unit = pl.wide ? wide_rg(pl.KW) : epi ? 2 : 1;      // row groups per work unit (narrow: a gate/up pair)
  const int n_units = (int)(pl.N >> 4) / per_unit;
  if (!pl.valid || n_units < 1) return g;
  g.S = pl.wide && epi ? 1 : pl.S;                   // (wide silu: both K halves in one workgroup)
  g.nb = (!pl.wide && g_force_wgs > 0 ? g_force_wgs : n_cus()) / g.S;
  if (g.nb < 1) g.nb = 1;
  if (g.nb > n_units) g.nb = n_units;
  if (pl.wide) {
    g.lds = 2 * per_unit * 4 * 4 * 1024;             // two tile sets x RG row groups x four waves x MB tiles of 1 KiB
    if (epi) g.lds += (size_t)((n_units + g.nb - 1) / g.nb) * per_unit * 4 * 1024;      // + a unit's reduced tiles (first K half) per unit of a workgroup
    g.ok = g.lds <= 150 * 1024;      // (on a smaller or partitioned device the units per workgroup grow)
  } else {
    // the kernel derives its share from gridDim.x (ceil((n_units - b) / nb) units) and keeps one LDS tile set per
    // row group: a share past kMaxG row groups would index LDS beyond the allocation, so the grid grows instead
    // (more workgroups than CUs; they run in rounds)
    int G = (n_units + g.nb - 1) / g.nb;
    if (G * per_unit > kMaxG) {
      G = kMaxG / per_unit;
      g.nb = (n_units + G - 1) / G;
    }
    // (one workgroup per CU even when the last round is partial: its short shares go to the first workgroups of the
    // grid, which are the late starters of a NORM launch — see the kernel)
    g.lds = (size_t)G * per_unit * 4 * (size_t)((pl.M + 15) / 16) * 1024;
    g.ok = ((n_units + g.nb - 1) / g.nb) * per_unit <= kMaxG;
  }
  return g;
}

// ---- what a plan can do, each written once --------------------------------------------------------------------
int64_t slab_bytes(const XregPlan& pl) { return pl.valid ? (int64_t)pl.S * pl.M * pl.N * (int64_t)sizeof(float) : 0; }
// add + RMSNorm in the launch: K in ONE split of the packing, rows of <= 2048 (wide: 1024) x 8 elements
bool norm_ok(const XregPlan& pl) { return pl.valid && pl.built->norm && pl.pk_S == 1 && pl.K / 8 <= (pl.wide ? 1024 : 2048); }
// silu(gate) * up in the launch, <= 32 rows: the whole K in the workgroup
bool silu_ok(const XregPlan& pl) {
  return pl.valid && !pl.wide && pl.gate_up && pl.N % 64 == 0 && pl.built->silu && pl.S == 1 && xreg_grid(pl, true).ok;
}
// the same behind the norm at 33 .. 64 rows: one packing split of two full halves (K = 4096), and the LDS the launch would ask for
bool wide_silu_ok(const XregPlan& pl) {
  return norm_ok(pl) && pl.wide && pl.M > 32 && pl.gate_up && pl.N % 64 == 0 && pl.built->silu && pl.S == 2 &&
         pl.pk_P == 2 * 4 * pl.KW && xreg_grid(pl, true).ok;
}
// does a gate|up weight of the one-entry interface keep its halves interleaved?  (hx_decode_weight_plan and _pack)
bool dw_interleaved(int64_t N, int64_t K, int flags) {
  return (flags & HX_DW_GATE_UP) && N % 32 == 0 && silu_ok(xreg_plan(32, N, K, true, false));
}

// ---- launches --------------------------------------------------------------------------------------------------
// One launch of either kernel: its dynamic-LDS limit raised where the launch needs more than the default (per
// device, so not cached in a static), the hot arguments packed, the launch, its status.
template <int NORM, typename... P>
int launch_hot(void (*kernel)(P...), const XregParams& p, const XregGrid& g, hipStream_t stream) {
  if (g.lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
    if (e != hipSuccess) return hip_rc(e);
  }
  XregHot h;
  if (!xreg_hot<NORM>(p, (unsigned)g.nb, &h)) return HX_ERR_SHAPE;
  hx::launcher(kernel, dim3((unsigned)g.nb, (unsigned)g.S), 256, g.lds, stream)(h.p0, h.p1, h.p2, h.p3, h.p4, h.a, h.b, h.c, h.ldx, p);
  return check_launch();
}

template <typename T, int MB, int KW, int EPI, int NORM>
int launch_kw(const XregParams& p, const XregGrid& g, hipStream_t stream) {
  if (NORM && g.S != 1) return HX_ERR_SHAPE;
  if constexpr (EPI == 0 && NORM == 0 && MB == 2 && (KW == 32 || KW == 29)) if (g_dbg) {   // ablation variants (tools/bench_gemm_xreg.py OPTS=xreg_dbg=..)
    if (g_dbg == 1) return launch_hot<0>(gemm_xreg_kernel<T, MB, KW, 0, 1>, p, g, stream);
    if (g_dbg == 2) return launch_hot<0>(gemm_xreg_kernel<T, MB, KW, 0, 2>, p, g, stream);
    return launch_hot<0>(gemm_xreg_kernel<T, MB, KW, 0, 3>, p, g, stream);
  }
#if HX_EXPERIMENTS
  // measured and not taken (round 6, profiles/rejected.md): the same kernel over the ROW-MAJOR tensor — one weight copy
  // on a collocated node — streams 16 x 64-byte pieces per wave instruction and is 10-30 % slower (7B, 32 rows)
  if constexpr (MB == 2 && (KW == 32 || KW == 22 || KW == 29))
    if (p.stagger & 16) return launch_hot<NORM>(gemm_xreg_kernel<T, MB, KW, EPI, 0, NORM, 1>, p, g, stream);
#endif
  return launch_hot<NORM>(gemm_xreg_kernel<T, MB, KW, EPI, 0, NORM>, p, g, stream);
}

// f(integral_constant<i>) for the row i of `table` whose k-step count is kw; HX_ERR_SHAPE when there is none
template <size_t n, typename F, size_t... I>
int with_built_row(const XregBuilt (&table)[n], int kw, F&& f, std::index_sequence<I...>) {
  int rc = HX_ERR_SHAPE;
  (void)((table[I].kw == kw && ((rc = f(std::integral_constant<size_t, I>{})), true)) || ...);
  return rc;
}
template <size_t n, typename F>
int with_built_row(const XregBuilt (&table)[n], int kw, F&& f) { return with_built_row(table, kw, f, std::make_index_sequence<n>{}); }

template <typename T, int EPI, int NORM>
int launch_t(const XregParams& p, const XregPlan& pl, const XregGrid& g, hipStream_t stream) {
  if (pl.wide)
    return with_built_row(kWideBuilt, pl.KW, [&](auto i) -> int {
      constexpr XregBuilt r = kWideBuilt[decltype(i)::value];
      if constexpr (is_built(r, true, EPI, NORM)) return launch_hot<NORM>(gemm_xreg_wide_kernel<T, r.kw, NORM, wide_rg(r.kw), EPI>, p, g, stream);
      else return HX_ERR_SHAPE;
    });
  return with_built_row(kNarrowBuilt, pl.KW, [&](auto i) -> int {
    constexpr XregBuilt r = kNarrowBuilt[decltype(i)::value];
    if constexpr (!is_built(r, false, EPI, NORM)) return HX_ERR_SHAPE;
    else return pl.M <= 16 ? launch_kw<T, 1, r.kw, EPI, NORM>(p, g, stream) : launch_kw<T, 2, r.kw, EPI, NORM>(p, g, stream);
  });
}

// THE launch path: a plain product returns its slab count, the silu epilogue HX_OK (or either a negative HX_ERR_*)
template <int EPI, int NORM>
int xreg_launch(const XregParams& p, const XregPlan& pl, int dtype, hx_stream stream) {
  const XregGrid g = xreg_grid(pl, EPI);
  if (!g.ok) return HX_ERR_SHAPE;
  const int rc = dtype == HX_F16 ? launch_t<F16, EPI, NORM>(p, pl, g, (hipStream_t)stream)
                                 : launch_t<BF16, EPI, NORM>(p, pl, g, (hipStream_t)stream);
  return rc || EPI ? rc : pl.S;
}

// ---- arguments -------------------------------------------------------------------------------------------------
// the add + RMSNorm in front of a product (hx_add_rms_norm_slabs): what the four norm-fused entries take
struct NormIn {
  void* residual; const float* slabs; int32_t n_splits; const void* weight; float eps; void* x_frag; void* sync;
};

// Everything is zero / null but what the plan and the caller give.  Plain: x as passed; norm-fused: x is produced
// fragment-major INSIDE the launch.  partial or act is null (a plain product / the silu epilogue).
XregParams xreg_params(const XregPlan& pl, const void* packed, float* partial, void* act, const void* x, int64_t ldx,
                       int x_fragment_major, const NormIn* nm = nullptr) {
  XregParams p{};
  p.w = packed; p.partial = partial; p.act = act;
  p.M = (int)pl.M; p.N = (int)pl.N; p.K = (int)pl.K;
  p.stagger = stagger_bits();
  if (pl.wide) { p.interleaved = pl.gate_up ? 1 : 0; p.pk_P = pl.pk_P; }
  p.x = x; p.ldx = ldx; p.x_packed = x_fragment_major ? 1 : 0;
  if (nm) {
    p.x = nm->x_frag; p.ldx = pl.K; p.x_packed = 1;
    p.nm_partial = nm->slabs; p.nm_residual = nm->residual; p.nm_weight = nm->weight; p.sync = (uint32_t*)nm->sync;
    p.nm_splits = nm->n_splits; p.nm_eps = nm->eps;
  }
  return p;
}

// The checks of every launch entry in the ABI's order of precedence: a null pointer, the shape, the dtype, a
// misaligned pointer, the workspace.
int check_args(std::initializer_list<const void*> ptrs, bool shape_ok, int dtype, int64_t have_bytes = 0, int64_t need_bytes = 0) {
  for (const void* q : ptrs) if (!q) return HX_ERR_NULL;
  if (!shape_ok) return HX_ERR_SHAPE;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  for (const void* q : ptrs) if (!aligned16(q)) return HX_ERR_STRIDE;
  return have_bytes < need_bytes ? HX_ERR_WORKSPACE : HX_OK;
}
int check_norm_args(const void* out, const void* packed, const NormIn& nm, bool shape_ok, int dtype, int64_t have_bytes = 0,
                    int64_t need_bytes = 0) {
  return check_args({out, packed, nm.residual, nm.slabs, nm.weight, nm.x_frag, nm.sync}, nm.n_splits >= 1 && shape_ok, dtype,
                    have_bytes, need_bytes);
}

}  // namespace

namespace hx {
int xreg_set_option(const char* name, int value) {
  if (!strcmp(name, "xreg_stagger")) { g_stagger = value; return HX_OK; }
  if (!strcmp(name, "xreg_timeline")) { g_timeline = value ? 1 : 0; return HX_OK; }
  if (!strcmp(name, "xreg_wgs")) { g_force_wgs = value; return HX_OK; }
  if (!strcmp(name, "xreg_no_producers")) { g_no_producers = value; return HX_OK; }
  if (!strcmp(name, "xreg_dbg")) { g_dbg = value; return HX_OK; }
  if (!strcmp(name, "xreg_row_major")) { g_row_major = value ? 1 : 0; return HX_OK; }
  return HX_ERR_UNSUPPORTED;
}
}  // namespace hx

// ---- the plain product: <= 32 rows the narrow kernel, 33 .. 64 the wide one over the same packing ---------------
extern "C" int hx_linear_decode_xreg_supported(int64_t M, int64_t N, int64_t K) { return xreg_plan(M, N, K, false, M > 32).valid ? 1 : 0; }

extern "C" int hx_linear_decode_xreg_splits(int64_t N, int64_t K) {
  const XregPlan pl = xreg_plan(1, N, K, false, false);
  return pl.valid ? pl.S : HX_ERR_SHAPE;
}

extern "C" int64_t hx_linear_decode_xreg_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  return slab_bytes(xreg_plan(M, N, K, false, M > 32));
}

extern "C" int64_t hx_fragment_major_elems(int64_t rows, int64_t K) {
  if (rows <= 0 || K <= 0 || K % 32) return 0;
  return (rows + 15) / 16 * 16 * K;
}

extern "C" int hx_pack_decode_weight_xreg(void* packed, const void* weight, int64_t N, int64_t K, int64_t ldw,
                                          int interleave_halves, int dtype, hx_stream stream) {
  const XregPlan pl = xreg_plan(1, N, K, interleave_halves != 0, false);
  if (int rc = check_args({packed, weight}, pl.valid && ldw % 8 == 0 && !(interleave_halves && N % 32), dtype)) return rc;
  const int64_t n_pieces = N * K / 8;
  hx::launcher(pack_xreg_kernel, (unsigned)((n_pieces + 255) / 256), 256, 0, (hipStream_t)stream)(
      (u16*)packed, (const u16*)weight, n_pieces, (int)(K >> 5), (int)(N >> 4), ldw, pl.pk_P, interleave_halves ? 1 : 0);
  return check_launch();
}

extern "C" int hx_linear_decode_partial_xreg(float* partial, const void* x, const void* packed_weight,
                                             int64_t M, int64_t N, int64_t K, int64_t ldx, int x_fragment_major,
                                             int64_t partial_bytes, int dtype, hx_stream stream) {
  const XregPlan pl = xreg_plan(M, N, K, false, M > 32);
  if (int rc = check_args({partial, x, packed_weight}, pl.valid && (x_fragment_major || ldx % 8 == 0), dtype, partial_bytes, slab_bytes(pl))) return rc;
  return xreg_launch<0, 0>(xreg_params(pl, packed_weight, partial, nullptr, x, ldx, x_fragment_major), pl, dtype, stream);
}

// ---- gate|up + silu*mul in one launch (<= 32 rows) ---------------------------------------------------------------
extern "C" int hx_gate_up_silu_xreg_supported(int64_t M, int64_t inter, int64_t K) {
  return silu_ok(xreg_plan(M, 2 * inter, K, true, false)) ? 1 : 0;
}

extern "C" int hx_gate_up_silu_xreg(void* act, const void* x, const void* packed_gate_up, int64_t M,
                                    int64_t inter, int64_t K, int64_t ldx, int x_fragment_major, int dtype,
                                    hx_stream stream) {
  const XregPlan pl = xreg_plan(M, 2 * inter, K, true, false);
  if (int rc = check_args({act, x, packed_gate_up}, silu_ok(pl) && (x_fragment_major || ldx % 8 == 0), dtype)) return rc;
  return xreg_launch<1, 0>(xreg_params(pl, packed_gate_up, nullptr, act, x, ldx, x_fragment_major), pl, dtype, stream);
}

// ---- add + RMSNorm fused in front of the product (one launch instead of two) --------------------
extern "C" int hx_norm_xreg_supported(int64_t M, int64_t N, int64_t K, int gate_up) {
  if (gate_up) return hx_gate_up_silu_xreg_supported(M, N / 2, K);   // (a silu row of the table is a norm row, one split <= 5120 elements)
  return norm_ok(xreg_plan(M, N, K, false, M > 32)) ? 1 : 0;
}

extern "C" int hx_norm_linear_decode_xreg(float* partial, void* residual, const float* slabs_in, int32_t n_splits_in,
                                          const void* norm_weight, float epsilon, void* x_frag,
                                          const void* packed_weight, int64_t M, int64_t N, int64_t K, void* sync,
                                          int64_t partial_bytes, int dtype, hx_stream stream) {
  const NormIn nm{residual, slabs_in, n_splits_in, norm_weight, epsilon, x_frag, sync};
  const XregPlan pl = xreg_plan(M, N, K, false, M > 32);
  if (int rc = check_norm_args(partial, packed_weight, nm, norm_ok(pl), dtype, partial_bytes, slab_bytes(pl))) return rc;
  return xreg_launch<0, 1>(xreg_params(pl, packed_weight, partial, nullptr, nullptr, 0, 1, &nm), pl, dtype, stream);
}

extern "C" int hx_norm_gate_up_silu_xreg(void* act, void* residual, const float* slabs_in, int32_t n_splits_in,
                                         const void* norm_weight, float epsilon, void* x_frag,
                                         const void* packed_gate_up, int64_t M, int64_t inter, int64_t K, void* sync,
                                         int dtype, hx_stream stream) {
  const NormIn nm{residual, slabs_in, n_splits_in, norm_weight, epsilon, x_frag, sync};
  const XregPlan pl = xreg_plan(M, 2 * inter, K, true, false);
  if (int rc = check_norm_args(act, packed_gate_up, nm, silu_ok(pl) && norm_ok(pl), dtype)) return rc;
  return xreg_launch<1, 1>(xreg_params(pl, packed_gate_up, nullptr, act, nullptr, 0, 1, &nm), pl, dtype, stream);
}

// ---- the gate|up product WITHOUT the fused silu*mul, over the interleaved packing (batches of 33 .. 64 rows: x for
// 64 rows needs two K splits per workgroup, silu*mul the whole K) — the wide kernel at every row count, slabs in
// [gate | up] column order for hx_silu_and_mul_slabs.  Optionally with the add + RMSNorm in front.
extern "C" int hx_gate_up_xreg_supported(int64_t M, int64_t inter, int64_t K, int with_norm) {
  const XregPlan pl = xreg_plan(M, 2 * inter, K, true, true);
  return pl.valid && inter % 32 == 0 && (!with_norm || norm_ok(pl)) ? 1 : 0;
}

extern "C" int64_t hx_gate_up_xreg_workspace_bytes(int64_t M, int64_t inter, int64_t K) {
  return slab_bytes(xreg_plan(M, 2 * inter, K, true, true));
}

extern "C" int hx_gate_up_xreg(float* partial, const void* x, const void* packed_gate_up, int64_t M, int64_t inter, int64_t K,
                               int64_t ldx, int x_fragment_major, int64_t partial_bytes, int dtype, hx_stream stream) {
  const XregPlan pl = xreg_plan(M, 2 * inter, K, true, true);
  if (int rc = check_args({partial, x, packed_gate_up}, pl.valid && inter % 32 == 0 && (x_fragment_major || ldx % 8 == 0), dtype,
                          partial_bytes, slab_bytes(pl))) return rc;
  return xreg_launch<0, 0>(xreg_params(pl, packed_gate_up, partial, nullptr, x, ldx, x_fragment_major), pl, dtype, stream);
}

extern "C" int hx_norm_gate_up_xreg(float* partial, void* residual, const float* slabs_in, int32_t n_splits_in,
                                    const void* norm_weight, float epsilon, void* x_frag, const void* packed_gate_up,
                                    int64_t M, int64_t inter, int64_t K, void* sync, int64_t partial_bytes, int dtype,
                                    hx_stream stream) {
  const NormIn nm{residual, slabs_in, n_splits_in, norm_weight, epsilon, x_frag, sync};
  const XregPlan pl = xreg_plan(M, 2 * inter, K, true, true);
  if (int rc = check_norm_args(partial, packed_gate_up, nm, inter % 32 == 0 && norm_ok(pl), dtype, partial_bytes, slab_bytes(pl))) return rc;
  return xreg_launch<0, 1>(xreg_params(pl, packed_gate_up, partial, nullptr, nullptr, 0, 1, &nm), pl, dtype, stream);
}

// ---- the same with silu*mul in the launch (33 .. 64 rows): both K halves in one workgroup, no slabs ---------------
extern "C" int hx_gate_up_silu_wide_xreg_supported(int64_t M, int64_t inter, int64_t K) {
  return wide_silu_ok(xreg_plan(M, 2 * inter, K, true, true)) ? 1 : 0;
}

extern "C" int hx_norm_gate_up_silu_wide_xreg(void* act, void* residual, const float* slabs_in, int32_t n_splits_in,
                                              const void* norm_weight, float epsilon, void* x_frag,
                                              const void* packed_gate_up, int64_t M, int64_t inter, int64_t K, void* sync,
                                              int dtype, hx_stream stream) {
  const NormIn nm{residual, slabs_in, n_splits_in, norm_weight, epsilon, x_frag, sync};
  const XregPlan pl = xreg_plan(M, 2 * inter, K, true, true);
  if (int rc = check_norm_args(act, packed_gate_up, nm, wide_silu_ok(pl), dtype)) return rc;
  return xreg_launch<1, 1>(xreg_params(pl, packed_gate_up, nullptr, act, nullptr, 0, 1, &nm), pl, dtype, stream);
}

// ---- what a launch will be (tests pick a shape per instantiation with these; host only, nothing is launched) -------
extern "C" int hx_debug_xreg_plan(int64_t M, int64_t N, int64_t K, int gate_up, int wide, int epi, int32_t out[8]) {
  if (!out) return HX_ERR_NULL;
  const XregPlan pl = xreg_plan(M, N, K, gate_up != 0, wide != 0);
  const XregGrid g = xreg_grid(pl, epi != 0);
  out[0] = pl.wide ? 1 : 0;
  out[1] = pl.KW;
  out[2] = (int32_t)((M + 15) / 16);
  out[3] = g.S;
  out[4] = pl.pk_S;
  out[5] = g.nb * g.S;
  out[6] = (int32_t)g.lds;
  out[7] = pl.valid && g.ok ? 1 : 0;
  return HX_OK;
}

extern "C" int hx_debug_xreg_built(int wide, int index, int32_t out[3]) {
  if (!out) return HX_ERR_NULL;
  const XregBuilt* table = wide ? kWideBuilt : kNarrowBuilt;
  const int n = (int)(wide ? std::size(kWideBuilt) : std::size(kNarrowBuilt));
  if (index < 0 || index >= n) return HX_ERR_SHAPE;
  out[0] = table[index].kw;
  out[1] = table[index].norm ? 1 : 0;
  out[2] = table[index].silu ? 1 : 0;
  return HX_OK;
}

// ------------------------------------------------------------------------------------------------------------
// One entry for the decode-batch linear layer (include/hydra_hip.h "hx_decode_weight"): the caller describes the
// weight once, the library chooses the layout (activations-in-registers for <= 32 rows when the shape allows it,
// LDS-slice otherwise), packs it, and hx_linear_decode_ex dispatches on the descriptor.
// ------------------------------------------------------------------------------------------------------------
extern "C" int hx_decode_weight_plan(hx_decode_weight* w, int64_t N, int64_t K, int dtype, int max_rows, int flags) {
  if (!w) return HX_ERR_NULL;
  if (N <= 0 || K <= 0 || max_rows <= 0 || max_rows > 64) return HX_ERR_SHAPE;
  if (dtype != HX_F16 && dtype != HX_BF16) return HX_ERR_DTYPE;
  if (flags & ~(HX_DW_GATE_UP | HX_DW_FORCE_LDS_SLICE)) return HX_ERR_UNSUPPORTED;
  const bool force_lds = (flags & HX_DW_FORCE_LDS_SLICE) != 0;
  flags &= ~HX_DW_FORCE_LDS_SLICE;
  w->packed = nullptr;
  w->N = N; w->K = K; w->dtype = dtype; w->flags = flags; w->max_rows = max_rows;
  // the activations-in-registers layout serves <= 32 rows always, 33 .. 64 rows where the wide kernel can read the same
  // packing (a gate|up weight keeps its halves interleaved then: the plain product un-interleaves its slab columns)
  const bool xreg = !force_lds && xreg_plan(std::min(max_rows, 32), N, K, false, false).valid &&
                    (max_rows <= 32 || xreg_plan(max_rows, N, K, dw_interleaved(N, K, flags), true).valid);
  if (!xreg && (N % 16 || K % 256)) return HX_ERR_SHAPE;
  if ((flags & HX_DW_GATE_UP) && (!xreg || N % 32)) w->flags &= ~HX_DW_GATE_UP;   // no fused epilogue on this layout: halves stay in order
  w->layout = xreg ? HX_DW_XREG : HX_DW_LDS_SLICE;
  return HX_OK;
}

extern "C" int hx_decode_weight_pack(hx_decode_weight* w, void* packed, const void* weight, int64_t ldw, hx_stream stream) {
  if (!w || !packed || !weight) return HX_ERR_NULL;
  int rc;
  if (w->layout == HX_DW_XREG) {
    const bool inter = dw_interleaved(w->N, w->K, w->flags);
    if (!inter) w->flags &= ~HX_DW_GATE_UP;      // (K in more than one split: the plan kept the flag, the halves stay in order)
    rc = hx_pack_decode_weight_xreg(packed, weight, w->N, w->K, ldw, inter, w->dtype, stream);
  } else if (w->layout == HX_DW_LDS_SLICE) {
    rc = hx_pack_decode_weight(packed, weight, w->N, w->K, ldw, w->dtype, stream);
  } else {
    return HX_ERR_UNSUPPORTED;
  }
  if (rc == HX_OK) w->packed = packed;
  return rc;
}

extern "C" int64_t hx_linear_decode_ex_workspace_bytes(const hx_decode_weight* w, int64_t M) {
  if (!w || M <= 0) return 0;
  if (w->layout == HX_DW_XREG && (w->flags & HX_DW_GATE_UP)) return hx_gate_up_xreg_workspace_bytes(M, w->N / 2, w->K);
  return w->layout == HX_DW_XREG ? hx_linear_decode_xreg_workspace_bytes(M, w->N, w->K)
                                 : hx_linear_decode_workspace_bytes(M, w->N, w->K);
}

extern "C" int hx_linear_decode_ex(float* partial, int64_t partial_bytes, const void* x, int64_t ldx,
                                   int x_fragment_major, const hx_decode_weight* w, int64_t M, hx_stream stream) {
  if (!w || !w->packed) return HX_ERR_NULL;
  if (M > w->max_rows) return HX_ERR_SHAPE;
  if (w->layout == HX_DW_XREG) {
    if (w->flags & HX_DW_GATE_UP)     // interleaved halves: the fused hx_gate_up_silu_xreg, or this plain product (slabs [gate | up])
      return hx_gate_up_xreg(partial, x, w->packed, M, w->N / 2, w->K, ldx, x_fragment_major, partial_bytes, w->dtype, stream);
    return hx_linear_decode_partial_xreg(partial, x, w->packed, M, w->N, w->K, ldx, x_fragment_major, partial_bytes,
                                         w->dtype, stream);
  }
  if (x_fragment_major) return HX_ERR_STRIDE;                  // the LDS-slice kernel stages row-major x
  return hx_linear_decode_partial_packed(partial, x, w->packed, M, w->N, w->K, ldx, partial_bytes, w->dtype, stream);
}
