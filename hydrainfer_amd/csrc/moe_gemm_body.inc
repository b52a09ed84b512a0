// moe_gemm_body.inc — the body of a grouped expert GEMM, textually included ONCE into moe_gemm_kernel (moe_experts.hip,
// 16-bit weights) and into moe_gemm_fp8w_kernel (moe_experts_fp8.hip, FP8 block-scaled weights): the segment prologue,
// the tile set-up, the x gather, the chunk loop and the epilogue.  The plan is described in moe_experts.hip.
// Expects in scope: the kernel's parameters `out`, `xin`, `wgt` (const WElem*), `wsc` (the scales [E, rows / 128, K / 128];
// unused without kScaled), `seg`, N, K, n_experts, n_slots, topk; T, MB, GU; and the weight format:
//   WElem, WVec       a weight element and the 16 bytes of one lane of a load instruction (u16, u16x8 / uint8_t, u32x4)
//   kKplLog2          log2 of the k one load instruction covers per row: 128 bytes = 64 (16-bit) / 128 (FP8, = one
//                     scale block); two instructions fill the wave's transpose image: a BLOCK of 16 rows x that many k
//   kScaled           a block carries one fp32 scale per wave (a wave's 16 rows lie inside one 128-row scale block)
//   kSkipEmptyRows    the x staging fetches only the 16-row blocks of the tile that hold rows
//   HX_MOE_BLOCK_INC  the text that takes one block through the image (wstream_block16.inc / wstream_block_fp8.inc)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = MoeGemmCfg<MB, GU>;
  constexpr int KL = C::KL, SK = C::SK, kRS = C::RS, kRows = C::kRows;
  constexpr int kKpl = 1 << kKplLog2;
  constexpr int NB = SK / kKpl;                  // blocks per stream and chunk
  constexpr int NJ = 2 * NB;                     // load instructions per stream and chunk
  constexpr int kCpr = KL / 8;                   // 16-byte pieces per LDS row of x
  constexpr int XPT = kRows * kCpr / 256;        // pieces per thread and chunk
  constexpr int XRND = XPT < 8 ? XPT : 8;        // ... fetched 8 at a time
  const int e = blockIdx.y;
  // ---- the expert's segment, before anything else: no rows, no weight bytes (and no scales)
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
  int32_t* srow = reinterpret_cast<int32_t*>(smem + kRows * kRS + 4 * 2048);   // [64] source row of x per tile row
  int32_t* drow = srow + kTile;                                                 // [64] destination slot
  char* images = smem + kRows * kRS;              // the wave-private transpose images lie behind the x image
#include "wstream_image.inc"
  const char* xl = smem + c * kRS + g * 16;

  const int n0 = (blockIdx.x * 4 + w) << 4;       // the wave's 16 output rows
  const int64_t wrows = GU ? 2 * (int64_t)N : (int64_t)N;
  [[maybe_unused]] const int KB = K / 128;
  const WElem* wbase = wgt + ((int64_t)e * wrows + n0 + lrow) * K + (int)(16 / sizeof(WElem)) * lpiece;
  [[maybe_unused]] const float* sbase = kScaled ? wsc + ((int64_t)e * (wrows / 128) + (n0 >> 7)) * KB : nullptr;
  const int n_it = (K + KL - 1) / KL;

  // weight load of stream s at LDS chunk `it`: instruction j covers rows 8 * (j & 1) + (lane >> 3) and the 128-byte
  // block j >> 1; blocks past K re-read a valid one (their MFMAs are skipped), and so do their scales
  auto load = [&](WVec (&buf)[NJ], [[maybe_unused]] float (&sc)[NB], int it, int s) {
    const int k0 = it * KL + (GU ? 0 : s * SK);
    const int last_cb = max(min((K - k0) >> kKplLog2, NB), 1) - 1;
    const int k0c = min(k0, K - kKpl);
    const WElem* wp = wbase + (GU ? (int64_t)s * N * K : 0) + k0c;
    [[maybe_unused]] const float* sp = kScaled ? sbase + (GU ? (int64_t)s * (N / 128) * KB : 0) + (k0c >> 7) : nullptr;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int cb = min(j >> 1, last_cb);
      buf[j] = __builtin_nontemporal_load(reinterpret_cast<const WVec*>(wp + (int64_t)(8 * (j & 1)) * K + kKpl * cb));
    }
    if constexpr (kScaled) {
#pragma unroll
      for (int b = 0; b < NB; ++b) sc[b] = sp[min(b, last_cb)];
    }
  };
  // pieces [j0, j0 + XRND) of this thread's share of the gathered rows of chunk `it` (always a valid address; rows past
  // the tile and k past K are zero-filled at the LDS write).  Piece j of all threads covers the kRpp rows from j * kRpp.
  // kSkipEmptyRows: pieces past the tile's last 16-row block that holds rows (`xrows` = 16 nmb) are neither fetched nor
  // written — no MFMA reads those rows — so a tile of few rows does not stage 64 (at MB = 4 the staging of 64 x KL of x
  // per chunk is as many bytes as the chunk's fp8 weights).
  constexpr int kRpp = 256 / kCpr;
  auto xload = [&](u16x8 (&xr)[XRND], int it, int j0, int xrows) {
#pragma unroll
    for (int j = 0; j < XRND; ++j) {
      if (kSkipEmptyRows && (j0 + j) * kRpp >= xrows) continue;
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
      if (kSkipEmptyRows && (j0 + j) * kRpp >= xrows) continue;
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
      WVec buf[2][NJ];
      float sc[2][NB];
      xload(xr, it, 0, nmb * 16);
      load(buf[0], sc[0], it, 0);
      load(buf[1], sc[1], it, 1);
      // keep the weight loads in flight under the x staging (gemm_skinny_kernel: hipcc sinks them below the LDS writes)
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
        const int ncb = min(max((K - k0) >> kKplLog2, 0), NB);   // blocks of this stream inside K
        const char* xp = xl + (GU ? 0 : s * SK * 2);
        const WVec (&wbuf)[NJ] = buf[s];
        [[maybe_unused]] const float (&wscale)[NB] = sc[s];
        f32x4 (&accb)[MB] = acc[GU ? s : 0];
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) {
          if (cb < ncb) {
#include HX_MOE_BLOCK_INC
          }
        }
      }
    }

    // ---- epilogue: acc[.][mb][i] = out^T[n0 + 4 g + i][tile row 16 mb + c]
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
