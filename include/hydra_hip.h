/*
 * hydra_hip.h — C ABI of libhydra_hip.so: the MI355X (gfx950) implementation of
 * HydraInfer's attention + paged-KV operator surface (`hydrainfer._C.*`).
 *
 * Every entry point is `extern "C"`, takes raw device pointers, element
 * counts/strides (in ELEMENTS unless the name says bytes) and a hipStream_t
 * passed as `void*`, launches asynchronously on that stream, never
 * synchronises, never allocates, and returns 0 or a negative hx_status.
 * No torch types cross this boundary.  `hx_strerror` maps a status to text.
 *
 * Each function cites the reference interface it replaces
 * (paths relative to the dongxianzhe/hydrainfer tree).
 */
#ifndef HYDRA_HIP_H
#define HYDRA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: hx_attn_args.flags (was `reserved`) gates the local-window fields — a zero-filled tail of the struct means
 * "no softcap, no window"; launch plans; hx_decode_advance takes a stride; experiments moved to
 * hydra_hip_experimental.h */
#define HX_ABI_VERSION 3

typedef enum hx_dtype {
  HX_F32 = 0,
  HX_F16 = 1,
  HX_BF16 = 2,
} hx_dtype;

typedef enum hx_status {
  HX_OK = 0,
  HX_ERR_DTYPE = -1,       /* dtype not supported by this op                */
  HX_ERR_SHAPE = -2,       /* size / divisibility constraint violated       */
  HX_ERR_STRIDE = -3,      /* layout (contiguity / alignment) unsupported   */
  HX_ERR_NULL = -4,        /* required pointer is NULL                      */
  HX_ERR_UNSUPPORTED = -5, /* feature of the reference op not implemented   */
  HX_ERR_WORKSPACE = -6,   /* workspace too small                           */
  HX_ERR_HIP = -7,         /* a HIP runtime call failed (see hx_last_hip_error) */
  HX_ERR_HANDLE = -8,      /* bad IPC handle                                */
} hx_status;

typedef void* hx_stream; /* hipStream_t */

int hx_abi_version(void);
const char* hx_strerror(int status);
/* hipError_t of the most recent HX_ERR_HIP on this thread (0 if none). */
int hx_last_hip_error(void);
/* Tuning knobs for A/B measurements in one process (not part of the reference surface):
 * "decode_waves" = 4|8 waves per decode-attention workgroup, "decode_nt" = 0|1 non-temporal
 * K/V loads, "decode_small_lo" / "decode_small_hi" = range of (sequence, head) pair counts served
 * by the 8-wave no-split form, "fwd_row_blocks" = 0(auto)|1|2 query row blocks per wave,
 * "fwd_key_units" = 0(auto)|1|2 32-key units per tile and "fwd_xcd_remap" = 0|1 XCD-aware
 * workgroup numbering in the prefill kernel, "fwd_persistent" = 0|1(auto)|2 one workgroup per
 * (sequence, query tile, head) item | persistent workgroups where the launcher expects a gain |
 * persistent workgroups wherever their tables fit, "fwd_priority" = -1(auto)|0|1 and
 * "fwd_seq_group" = 0(auto)|1|2|4, "fwd_units" = -1(auto)|0|1 for the persistent form (equal
 * priorities or priority to the workgroup of a CU with more left to do; sequences per deal group;
 * single tiles or units of a sequence's k-th longest and k-th shortest tile),
 * "gemm_rows_per_wave" / "gemm_waves" / "gemm_slab_nt" for the decode GEMM — results are
 * identical for every setting of these.  "decode_gqa" = 0|1 selects the per-query-head or the
 * grouped-query decode kernel for n_heads > n_kv_heads (both within the stated tolerance; the
 * grouped kernel rounds P to T before P.V like the prefill kernel). */
int hx_debug_set_option(const char* name, int value);

/* ------------------------------------------------------------------------
 * Paged cache scatter.
 * replaces: csrc/kernel/kv_cache_kernels/kv_cache_kernels.cu:60-95 (set_kv_cache)
 *           hydrainfer/_C/kernel/kv_cache_kernels/__init__.pyi:5-10
 * cache[slot / block_size, slot % block_size, h, d] = src[token, h, d] for K and V.
 * keys/values: [n_tokens, n_kv_heads, head_dim], last two dims contiguous, row
 * stride k_stride / v_stride elements.  Caches: [n_blocks, block_size, n_kv_heads,
 * head_dim] with block stride cache_block_stride elements (rows inside a block
 * contiguous).  Bit-exact copy; slots < 0 are skipped.
 * ---------------------------------------------------------------------- */
int hx_set_kv_cache(const int32_t* slot_ids, const void* keys, const void* values,
                    void* key_cache, void* value_cache,
                    int64_t n_tokens, int64_t n_kv_heads, int64_t head_dim,
                    int64_t block_size, int64_t k_stride, int64_t v_stride,
                    int64_t kcache_block_stride, int64_t vcache_block_stride,
                    int dtype, hx_stream stream);

/* replaces: csrc/kernel/cache_kernels/cache_kernels.cu:55-83 (set_image_cache)
 *           hydrainfer/_C/kernel/cache_kernels/__init__.pyi:4-7 */
int hx_set_image_cache(const int32_t* slot_ids, const void* image_tokens, void* image_cache,
                       int64_t n_tokens, int64_t n_heads, int64_t head_dim,
                       int64_t block_size, int64_t token_stride, int64_t cache_block_stride,
                       int dtype, hx_stream stream);

/* ------------------------------------------------------------------------
 * replaces: csrc/kernel/norm/rms_norm.cu:43-63 (rms_norm)
 *           hydrainfer/_C/kernel/norm/__init__.pyi:4-9
 * out[r,i] = (T)(x[r,i] * rsqrt(mean_i(x[r,:]^2) + eps)) * w[i]   (T arithmetic for
 * the weight multiply, fp32 reduction) — rounding points of rms_norm.cu:39.
 * out/input contiguous [rows, hidden]; dtype f32/f16/bf16 (bf16 is an extension).
 * ---------------------------------------------------------------------- */
int hx_rms_norm(void* out, const void* input, const void* weight, float epsilon,
                int64_t rows, int64_t hidden, int dtype, hx_stream stream);

/* Extension: h = residual + x written back to `residual`,
 * out = rms_norm(h).  Same rounding as add-then-hx_rms_norm. */
int hx_add_rms_norm(void* out, void* residual, const void* x, const void* weight,
                    float epsilon, int64_t rows, int64_t hidden, int dtype, hx_stream stream);

/* ------------------------------------------------------------------------
 * replaces: csrc/kernel/position_embedding/rope.cu:82-117 (apply_rotary_pos_emb)
 *           hydrainfer/_C/kernel/position_embedding/__init__.pyi:5-11
 * In-place rotation of query [n_tokens, n_heads, head_dim] and key
 * [n_tokens, n_kv_heads, head_dim] (row strides q_stride / k_stride elements, last two
 * dims contiguous).  cos_sin: [max_positions, 2, rotary_dim/2] in the tensors' dtype.
 * x' = x*c - y*s ; y' = x*s + y*c, every operation rounded to T (rope.cu:22-27).
 * interleaved ? (x,y)=(2i,2i+1) : (i, i+rotary_dim/2).
 * ---------------------------------------------------------------------- */
int hx_apply_rotary_pos_emb(void* query, void* key, const int32_t* positions,
                            const void* cos_sin, int64_t n_tokens, int64_t n_heads,
                            int64_t n_kv_heads, int64_t head_dim, int64_t rotary_dim,
                            int64_t q_stride, int64_t k_stride, int interleaved,
                            int dtype, hx_stream stream);

/* Extension: apply_rotary_pos_emb (NeoX layout) on query/key in place AND
 * set_kv_cache(slot_ids, key, value) in one launch — the two consecutive calls of
 * hydrainfer/model/model_forward.py:78-83 + hydrainfer/layer/causal_attention.py:401-403.
 * Bit-identical to the two separate ops.  Vector path only (dims multiples of 16 bytes). */
int hx_rope_set_kv_cache(void* query, void* key, const void* value, const int32_t* positions,
                         const void* cos_sin, const int32_t* slot_ids, void* key_cache,
                         void* value_cache, int64_t n_tokens, int64_t n_heads, int64_t n_kv_heads,
                         int64_t head_dim, int64_t rotary_dim, int64_t q_stride, int64_t k_stride,
                         int64_t v_stride, int64_t block_size, int64_t kcache_block_stride,
                         int64_t vcache_block_stride, int dtype, hx_stream stream);

/* ------------------------------------------------------------------------
 * replaces: csrc/kernel/activation/activation.cu:52-56 (silu)
 *           hydrainfer/_C/kernel/activation/__init__.pyi:3-4
 * out[r,i] = (T)(x / (1 + exp(-x))) computed in fp32; input rows strided by
 * in_stride elements, out contiguous [rows, n].
 * ---------------------------------------------------------------------- */
int hx_silu(void* out, const void* input, int64_t rows, int64_t n, int64_t in_stride,
            int dtype, hx_stream stream);

/* Extension: out = (T)silu(gate) * up in T arithmetic, i.e. exactly
 * `silu(gate_proj(h)) * up_proj(h)` of hydrainfer/model/model_forward.py:36. */
int hx_silu_and_mul(void* out, const void* gate, const void* up, int64_t rows, int64_t n,
                    int64_t gate_stride, int64_t up_stride, int dtype, hx_stream stream);

/* Extensions for the vision tower (CLIP ViT; round 6): the reference runs these as separate torch ops, at 577 x 1024 each
 * a ~5 us launch-bound kernel.
 * hx_quick_gelu: out = x * sigmoid(1.702 x) — hydrainfer/layer/activation.py:17-22 (QuickGELU) — with its three T
 *   roundings (scaled copy, sigmoid, product); input rows strided by in_stride elements, out contiguous [rows, n];
 *   n and in_stride multiples of 8 (4 for fp32).
 * hx_add_layer_norm: residual[r,:] += x[r,:] (one T rounding, in place); out[r,:] = (T)((h - mean) * rstd * weight + bias),
 *   moments in fp32 over the T-rounded h, biased variance — `h = h + y; x = nn.LayerNorm(h)` of the encoder layer
 *   (hydrainfer/model/clip.py: CLIPEncoderLayer.forward) in one pass.  x == NULL: plain layer norm of `residual`
 *   (left untouched).  Contiguous rows, hidden % 8 == 0 (4 for fp32), hidden <= 8192 (4096 for fp32). */
int hx_quick_gelu(void* out, const void* input, int64_t rows, int64_t n, int64_t in_stride, int dtype, hx_stream stream);
int hx_add_layer_norm(void* out, void* residual, const void* x, const void* weight, const void* bias, float epsilon,
                      int64_t rows, int64_t hidden, int dtype, hx_stream stream);

/* ------------------------------------------------------------------------
 * Extension: decode-batch linear layer  out[M,N] = x[M,K] @ weight[N,K]^T  (M <= 64) as a
 * weight-streaming HIP kernel — the nn.Linear calls of hydrainfer/model/llama.py:24-27,48-50
 * at decode batch sizes.  fp32 accumulation, split-K partials summed in a fixed order.
 * Constraints: N % 16 == 0, K % 256 == 0, f16/bf16.  workspace >=
 * hx_linear_decode_workspace_bytes(M, N, K).  Strides in elements.
 * ---------------------------------------------------------------------- */
int64_t hx_linear_decode_workspace_bytes(int64_t M, int64_t N, int64_t K);
int hx_linear_decode(void* out, const void* x, const void* weight, int64_t M, int64_t N,
                     int64_t K, int64_t ldx, int64_t ldw, int64_t ldo, void* workspace,
                     int64_t workspace_bytes, int dtype, hx_stream stream);
/* ONE ENTRY for the decode-batch linear layer with pre-packed weights (what a maintainer binds; the layout-specific
 * entry points further down are what it dispatches to and what the fused decode layer of hydrainfer_amd/model uses).
 *   hx_decode_weight w;
 *   hx_decode_weight_plan(&w, N, K, dtype, max_rows, flags);      // host only: picks the layout for batches <= max_rows
 *   hx_decode_weight_pack(&w, packed_dev, weight, ldw, stream);   // once, at model load; packed_dev: N*K elements
 *   n_slabs = hx_linear_decode_ex(partial, bytes, x, ldx, 0, &w, M, stream);          // every step: partial[s][M][N] fp32
 * followed by a slab consumer (hx_add_rms_norm_slabs, hx_silu_and_mul_slabs, hx_decode_attention_fused, or a plain
 * sum).  layout: activations-in-registers (HX_DW_XREG: max_rows <= 32 and hx_linear_decode_xreg_supported) else
 * LDS-slice (HX_DW_LDS_SLICE: N % 16 == 0, K % 256 == 0, max_rows <= 64).  HX_DW_GATE_UP marks a [gate; up] weight:
 * on the XREG layout its halves are interleaved for hx_gate_up_silu_xreg / hx_norm_gate_up_silu_xreg (flag kept in
 * w->flags; hx_linear_decode_ex refuses such a packing), otherwise the flag is cleared and the rows stay in order.
 * x may be fragment-major (see hx_linear_decode_partial_xreg) on the XREG layout only.
 * Replaces: torch.nn.functional.linear of hydrainfer/model/llama.py:24-27,48-50 at decode batch sizes. */
typedef struct hx_decode_weight {
  const void* packed;   /* device, N*K elements; set by hx_decode_weight_pack */
  int64_t N, K;
  int32_t dtype;        /* HX_F16 | HX_BF16 */
  int32_t layout;       /* HX_DW_* chosen by hx_decode_weight_plan */
  int32_t flags;
  int32_t max_rows;
} hx_decode_weight;
#define HX_DW_LDS_SLICE 0
#define HX_DW_XREG 1
#define HX_DW_GATE_UP 1
#define HX_DW_FORCE_LDS_SLICE 2   /* plan flag only (not kept in w->flags): the LDS-slice layout whatever the batch range — the
                                   * consumer hands over ROW-major activations (the o projection behind the attention output) */
int hx_decode_weight_plan(hx_decode_weight* w, int64_t N, int64_t K, int dtype, int max_rows, int flags);
int hx_decode_weight_pack(hx_decode_weight* w, void* packed, const void* weight, int64_t ldw, hx_stream stream);
int64_t hx_linear_decode_ex_workspace_bytes(const hx_decode_weight* w, int64_t M);
int hx_linear_decode_ex(float* partial, int64_t partial_bytes, const void* x, int64_t ldx, int x_fragment_major,
                        const hx_decode_weight* w, int64_t M, hx_stream stream);
/* Same GEMM, but the fp32 split-K slabs partial[s][M][N] are left for a fused consumer.
 * Returns the number of slabs (>= 1) or a negative hx_status. */
int hx_linear_decode_partial(float* partial, const void* x, const void* weight, int64_t M,
                             int64_t N, int64_t K, int64_t ldx, int64_t ldw,
                             int64_t partial_bytes, int dtype, hx_stream stream);
/* The same GEMM on weights PACKED for streaming: hx_pack_decode_weight copies weight [N, K] (row
 * stride ldw elements) into packed [N*K], where the 1 KiB block (n/16, k/32) holds at lane
 * l = (r = l & 15, g = l >> 4) the 8 elements weight[16*(n/16) + r][32*(k/32) + 8g .. + 8] — the
 * MFMA A operand of that (row group, k-step) — and the blocks are ordered [K split of 1024][row
 * group][k-step in split].  The kernel then reads each (row group, K split) as one contiguous run,
 * adjacent to its neighbours' (the fastest read shape on MI355X, tools/bench_stream.py), and needs
 * no transpose.  Results are bit-identical to hx_linear_decode_partial.  N % 16 == 0, K % 256 == 0. */
int hx_pack_decode_weight(void* packed, const void* weight, int64_t N, int64_t K, int64_t ldw,
                          int dtype, hx_stream stream);
int hx_linear_decode_partial_packed(float* partial, const void* x, const void* packed_weight,
                                    int64_t M, int64_t N, int64_t K, int64_t ldx,
                                    int64_t partial_bytes, int dtype, hx_stream stream);
/* The decode-batch linear layer over an FP8 block-scaled weight (csrc/gemm_skinny_fp8.hip): the format DeepSeek-V3-family
 * checkpoints publish for their dense linears.  wq [N, K]: one byte per element, OCP float8_e4m3fn (a byte 0x7F / 0xFF is
 * a NaN weight), row stride ldw BYTES (a multiple of 16, >= K), 16-byte aligned; w_scale: contiguous fp32 [N / 128, K / 128]
 * (`weight_scale_inv`: weight = float(q) * scale, one scale per 128 x 128 block).  Weight-only: x [M, K] (row stride ldx
 * elements, a multiple of 8) and out [M, N] (row stride ldo elements, a multiple of 4) are T = `dtype` (HX_F16 / HX_BF16).
 * M 1 .. 64, N % 128 == 0, K % 256 == 0; workspace >= hx_linear_decode_workspace_bytes(M, N, K), 16-byte aligned.
 *   out[m][n] = T( sum over splits s (of 1024 k, in order) of
 *                  sum over the 128-k blocks b of split s (in order) of
 *                  w_scale[n / 128][b] * ( sum_{k in b} float(x[m][k]) * float(q[n][k]) ) )
 * — every sum an fp32 sum of exact products (MFMA accumulation inside a block), a block's scale applied to that block's
 * fp32 partial sum with ONE fma into the split's running sum, ONE rounding to T (in the slab reduce, deterministic, no
 * atomics); a weight is never rounded after it has been scaled.  Nothing outside [N, K] of wq (row gaps included) and
 * nothing outside w_scale reaches a result.
 * Status as hx_linear_decode: non-positive sizes and the shape / stride rules HX_ERR_SHAPE, NULL (w_scale included)
 * HX_ERR_NULL, fp32 HX_ERR_DTYPE, a small workspace HX_ERR_WORKSPACE, misaligned bases HX_ERR_STRIDE; nothing is launched
 * on a refusal.  "gemm_fp8_waves" / "gemm_fp8_rows_per_wave" (hx_debug_set_option; 0 = automatic) force the launch's
 * waves per workgroup / 16-row groups per wave — results are identical for every built pair; a pair that is not built for
 * the batch's row blocks is HX_ERR_UNSUPPORTED.  hx_debug_linear_fp8_plan (host only) writes the (waves, row groups per
 * wave) the launch of (M, N, K) makes under the current options into out[0..1].
 * hx_dequant_fp8_block: out[n][k] = T(float(q[n][k]) * w_scale[n / 128][k / 128]) — one fp32 multiply, one rounding — for the
 * library GEMM of batches above 64 rows.  wq contiguous [N, K], N % 128 == 0, K % 128 == 0; out row stride ldo elements
 * (a multiple of 8, >= K), 16-byte aligned. */
int hx_linear_decode_fp8w(void* out, const void* x, const void* wq, const float* w_scale, int64_t M, int64_t N, int64_t K,
                          int64_t ldx, int64_t ldw, int64_t ldo, void* workspace, int64_t workspace_bytes, int dtype,
                          hx_stream stream);
int hx_debug_linear_fp8_plan(int64_t M, int64_t N, int64_t K, int32_t* out);
int hx_dequant_fp8_block(void* out, const void* wq, const float* w_scale, int64_t N, int64_t K, int64_t ldo, int dtype,
                         hx_stream stream);
/* Step-edge fusions of a decode loop (extensions, bit-identical to the ops they replace).
 * hx_embed_rms_norm: h_out[r] = table[ids[r]] (torch.nn.functional.embedding; ids int32 or int64, out-of-range
 * ids clamp) and x_out[r] = rms_norm(h_out[r]) * weight, one launch (hydrainfer/model/llama.py:80-83 + layer/norm.py).
 * hx_argmax_rows: out[r] = argmax(logits[r, :n]) with torch.argmax's rule (NaN largest, ties to the smallest
 * index): the greedy sampler of hydrainfer/model/llama.py:99-104. */
int hx_embed_rms_norm(void* h_out, void* x_out, const void* ids, int ids_are_int64, const void* table,
                      const void* weight, float epsilon, int64_t rows, int64_t hidden, int64_t vocab,
                      int dtype, hx_stream stream);
int hx_argmax_rows(int64_t* out, const void* logits, int64_t rows, int64_t n, int64_t ld, int dtype,
                   hx_stream stream);
/* hx_logprob_rows: per-token log-probabilities of a step, one launch (extension; added WITHOUT raising HX_ABI_VERSION:
 * nothing that existed changed).  Stands in for the greedy sampler of hydrainfer/model/llama.py:99-104 followed by
 * torch.log_softmax(logits.float(), -1) and torch.topk.  logits: fp16 / bf16 [rows, n], row stride ld elements.  Per row:
 *   ids[r]            the greedy token, bit-identical to hx_argmax_rows (NaN largest, ties to the smallest index);
 *   logprobs[r]       logits[r, ids[r]] - logsumexp(logits[r, :n]), all arithmetic in fp32;
 *   top_ids[r, :K], top_logprobs[r, :K]  (dense [rows, K], K = top_k in 0..20) the K largest entries ordered by value
 *                     descending, then index ascending (a NaN before every number); entries past n: id -1, logprob -inf.
 * A -inf logit has logprob -inf and leaves the rest of its row alone; a row that holds a NaN has every logprob NaN.
 * top_ids / top_logprobs may be NULL when top_k == 0.  rows < 1, n < 1, ld < n, top_k outside 0..20: HX_ERR_SHAPE;
 * fp32: HX_ERR_DTYPE; a missing pointer: HX_ERR_NULL — nothing is launched. */
int hx_logprob_rows(int64_t* ids, float* logprobs, int32_t* top_ids, float* top_logprobs, const void* logits,
                    int64_t rows, int64_t n, int64_t ld, int top_k, int dtype, hx_stream stream);
/* hx_token_logprob_rows: the log-probability of a GIVEN token per row — prompt log-probabilities, one launch over the
 * logits of a prefill chunk (extension; added WITHOUT raising HX_ABI_VERSION: nothing that existed changed).  Replaces no
 * reference interface: the reference's models end in torch.argmax (hydrainfer/model/llama.py:99-104) and score nothing;
 * it stands in for torch.log_softmax(logits.float(), -1).gather(-1, targets), a comparison count and torch.topk.
 * logits: fp16 / bf16 [rows, n], row stride ld elements; targets: int32 [rows] on the device.  Per row with
 * t = targets[r] in 0 .. n-1:
 *   logprobs[r]       logits[r, t] - logsumexp(logits[r, :n]), all arithmetic in fp32 (the model's raw softmax);
 *   ranks[r]          the number of entries that come before (logits[r, t], t) in hx_logprob_rows' order (a NaN first,
 *                     then the larger value, then the lower index): exact; 0 means t is hx_argmax_rows' id;
 *   top_ids[r, :K], top_logprobs[r, :K]  exactly what hx_logprob_rows writes, entries past n included.
 * A row with t < 0 or t >= n is not scored and not read: logprobs NaN, ranks -1, top_ids -1, top_logprobs -inf — rows
 * that only sample ride along in the same logits at no cost.  A -inf target has logprob -inf; a row that holds a NaN or
 * a +inf, or nothing but -inf, has every logprob NaN (as log_softmax gives).  top_ids / top_logprobs may be NULL when
 * top_k == 0.  rows < 1, n < 1, ld < n, top_k outside 0..20: HX_ERR_SHAPE; fp32: HX_ERR_DTYPE; a missing pointer
 * (targets and ranks included): HX_ERR_NULL — nothing is launched.
 * hx_token_logprob_rows_ex: A MEASUREMENT HOOK, NO STABILITY PROMISE — the same with the kernel form named, so that
 * tools/bench_token_logprobs.py and the tests can run both; products call hx_token_logprob_rows, and the forms or this
 * entry may go when the choice is settled.  form: 0 — the form kept per top_k class, what hx_token_logprob_rows runs;
 * 1 — one pass straight from global memory; 2 — the row staged in LDS first (rows wider than 65536 elements: form 1).
 * Another value: HX_ERR_SHAPE.  Results of the forms agree in ranks and ids bit for bit.  With top_k > 0 forms 0 and 2
 * repeat hx_logprob_rows' sum term for term in its order, so every log-probability equals its bit for bit (tested); form
 * 1 too where the logits are 16-byte aligned with ld % 8 == 0 (elsewhere its threads own other elements and the order
 * of the sum differs).  With top_k == 0 the forms agree to fp32 rounding of the sum. */
int hx_token_logprob_rows(float* logprobs, int32_t* ranks, int32_t* top_ids, float* top_logprobs, const void* logits,
                          const int32_t* targets, int64_t rows, int64_t n, int64_t ld, int top_k, int dtype,
                          hx_stream stream);
int hx_token_logprob_rows_ex(float* logprobs, int32_t* ranks, int32_t* top_ids, float* top_logprobs, const void* logits,
                             const int32_t* targets, int64_t rows, int64_t n, int64_t ld, int top_k, int dtype, int form,
                             hx_stream stream);
/* hx_penalized_argmax_rows: greedy sampling under frequency, presence and repetition penalties, one launch and one read
 * of the logits (extension; added WITHOUT raising HX_ABI_VERSION: nothing that existed changed).  Steps 1-2 of
 * hydrainfer/sampling/logits_processor.py:65-72 followed by the argmax of hydrainfer/model/llama.py:99-104; steps 3-5
 * there (temperature, top-k, top-p) never move the largest entry.  logits: fp16 / bf16 [rows, n], row stride ld elements,
 * n <= 262144 (2^18: the row's bitmap in LDS, 32 KiB).  The history is a CSR — the reference's unique_token_ids /
 * unique_token_counts / unique_token_lens without the padding: row r owns hist_ids[j], hist_counts[j] for
 * cu_hist[r] <= j < cu_hist[r + 1] (cu_hist int32 [rows + 1], its values are held inside [0, total] by the kernel), the
 * ids of a row pairwise distinct.  penalties: fp32 [rows, 3] = (frequency f, presence p, repetition r) per row.
 * For a history entry (t, c) of row r, with x = (float)logits[r, t], each operation rounded to fp32 on its own, in the
 * reference's order (bit-identical to torch's fp32 result):
 *     s = x - (float)c * f;   s = s - (c > 0 ? p : 0);   s = s < 0 ? s * r : s / r
 * every other element keeps its value.  ids[r]: the index of the first element in the order of hx_argmax_rows (a NaN
 * first, then the larger value, then the lower index) — a row with an empty history gives hx_argmax_rows' answer bit for
 * bit.  scores_out (fp32 [total], may be NULL): s of every history entry, in CSR order (the reference's `score`).
 * An entry with t < 0 or t >= n is ignored: nothing is read for it, and its scores_out entry is NaN.  A token that
 * appears twice in one row breaks the contract: the row's answer uses one of the two values, nothing is read or written
 * out of bounds.  total == 0 is legal and returns HX_OK: every row is plain argmax, cu_hist is still read (all zeros),
 * hist_ids / hist_counts may be NULL.  rows < 1, n < 1, ld < n, n > 262144, total < 0: HX_ERR_SHAPE; fp32:
 * HX_ERR_DTYPE; ids, logits, cu_hist or penalties NULL, or hist_ids / hist_counts NULL with total > 0: HX_ERR_NULL —
 * nothing is launched. */
int hx_penalized_argmax_rows(int64_t* ids, float* scores_out, const void* logits, int64_t rows, int64_t n, int64_t ld,
                             const int32_t* hist_ids, const int32_t* hist_counts, const int32_t* cu_hist, int64_t total,
                             const float* penalties, int dtype, hx_stream stream);
/* hx_sample_rows: seeded sampled decoding — penalties, temperature, top-k, top-p and the draw in one launch and one read
 * of the logits (extension: the reference's models end in torch.argmax; added WITHOUT raising HX_ABI_VERSION).  logits:
 * fp16 / bf16 [rows, n], row stride ld elements, n <= HX_SAMPLE_MAX_N (the row as fp32 in LDS).  The history arguments are
 * hx_penalized_argmax_rows'; with total == 0 no row is penalised and hist_ids, hist_counts, cu_hist and penalties may
 * all be NULL.  sample_params: one 32-byte record per row, eight 32-bit words:
 *     [0] temperature T (fp32)   [1] top_p (fp32)   [2] top_k (int32)   [3] 0
 *     [4] seed, low word   [5] seed, high word   [6] offset, low word   [7] offset, high word
 * offset: the index of the token being generated (0 for the first).  Per row:
 *   u = (Philox4x32-10(counter = (offset_lo, offset_hi, 0, 0), key = (seed_lo, seed_hi))[0] >> 8) * 2^-24, in [0, 1).
 *   s_i: the penalised value of hx_penalized_argmax_rows (float(x_i) outside the history).
 *   Greedy row — T == 0 (or not > 0): ids[r] is hx_penalized_argmax_rows' id bit for bit; no draw.  Degenerate row — a
 *   NaN in the row, or a largest z that is not finite: the same id.
 *   z_i = s_i / T, one correctly rounded fp32 division.
 *   top-k: K = n if top_k <= 0 or top_k >= n, else top_k; v_K = the K-th largest z counting multiplicity; every
 *   z_i >= v_K is kept (tied values stand or fall together).
 *   top-p: skipped if top_p >= 1 (v* = v_K).  Else, with m = max z, e_i = expf(z_i - m), Z_K = sum of e over {z >= v_K},
 *   A(v) = sum of e over {z > v}: v* = the smallest value of the row with v* >= v_K and A(v*) <= top_p * Z_K.
 *   draw: over S = {i : z_i >= v*} in INDEX order, the first i whose inclusive running sum of e exceeds u * Z_S (Z_S the
 *   sum over S); the last element of S if rounding leaves none.
 * Sums are fp32: per thread over the elements it owns, then a wave tree and the wave sums in order.  The same (row,
 * record) gives the same token whatever else is in the batch.  cut_out, u_out (fp32 [rows], may be NULL): v* and u; a
 * greedy or degenerate row gets NaN and its u.  rows < 1, n < 1, ld < n, n > HX_SAMPLE_MAX_N, total < 0: HX_ERR_SHAPE;
 * fp32: HX_ERR_DTYPE; ids, logits or sample_params NULL, or a history pointer NULL with total > 0: HX_ERR_NULL —
 * nothing is launched. */
#define HX_SAMPLE_MAX_N 35840
int hx_sample_rows(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows, int64_t n, int64_t ld,
                   const int32_t* hist_ids, const int32_t* hist_counts, const int32_t* cu_hist, int64_t total,
                   const float* penalties, const void* sample_params, int dtype, hx_stream stream);
/* hx_sample_rows_resident: hx_sample_rows without a history (its total == 0 case) for records that stay RESIDENT on the
 * device, as a captured decode step needs them (extension; added WITHOUT raising HX_ABI_VERSION: nothing that existed
 * changed).  One difference: words [6] and [7] of a record are not the offset but a 64-bit two's-complement offset_base,
 * and row r draws with
 *     offset = offset_base + (int64)positions[r]        modulo 2^64 (the carry into the high word included)
 * positions: int32 [rows], the step's position array.  In decode a request's position and its generated-token count both
 * grow by one per step, so offset_base = n_out - position is constant for the life of the request: a record written once
 * stays valid step after step, and the launch changes no state (a discarded or replayed step desynchronises nothing).
 * Words [0..5] are hx_sample_rows'; word [3] is ignored.  ids, cut_out and u_out are bit for bit what hx_sample_rows
 * gives for the same logits with total == 0 and a record that carries that offset — greedy rows (T == 0), degenerate
 * rows and NULL cut_out / u_out included.  Errors: hx_sample_rows' rules; positions NULL: HX_ERR_NULL — nothing is
 * launched.  A row wider than 12288 elements needs the kernel's dynamic-LDS limit raised: every call outside a stream
 * capture does that; a call on a capturing stream does not (it is no stream operation), so one call outside a capture
 * must have gone before on this device. */
int hx_sample_rows_resident(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows, int64_t n,
                            int64_t ld, const void* sample_params, const int32_t* positions, int dtype, hx_stream stream);
/* hx_sample_rows_resident_penalized: hx_sample_rows_resident with frequency / presence / repetition penalties over a
 * RESIDENT token log that the kernel both reads and appends to, so that a captured decode step penalises without the host
 * (extension; added WITHOUT raising HX_ABI_VERSION: nothing that existed changed).  token_log: int32 [log_slots,
 * log_cap], on the device.  penalty_params: int32 [rows, 4] = frequency, presence, repetition (fp32 bits) and the row's
 * log slot s.  With rec the row's record, L = offset_base(rec) + (int64)positions[r] — the 64-bit sum that is the Philox
 * offset, a request's generated-token count:
 *   Row without a slot (s < 0 or s >= log_slots): ids, cut_out and u_out are hx_sample_rows_resident's bit for bit; the
 *   log is neither read nor written.
 *   Row with a slot: its history is the multiset token_log[s][0 .. L'), L' = min(max(L, 0), log_cap).  ids, cut_out and
 *   u_out are bit for bit what hx_sample_rows gives for the same logits, the CSR of that multiset's (distinct ids,
 *   counts), the same three penalties and a record that carries offset L — greedy rows (hx_penalized_argmax_rows' id) and
 *   degenerate rows included.  A log entry outside [0, n) is ignored.  Then, if 0 <= L < log_cap, token_log[s][L] =
 *   (int32)ids[r]; otherwise nothing is written.
 * Nothing outside token_log[s][0 .. log_cap) is read or written.  The launch is IDEMPOTENT: it reads words [0, L) and
 * writes word [L] alone, so a step that is replayed, or whose sample is later dropped, desynchronises nothing — the next
 * step of the row overwrites word [L] or reads what a replay wrote again.  Two rows of one launch that name the same slot
 * break the contract (one of them wins word [L]); nothing goes out of bounds.
 * HX_SAMPLE_LOG_MAX: the log takes NO LDS beside the row (a 140 KiB row at n = HX_SAMPLE_MAX_N leaves under 19 KiB of the
 * 160 KiB, too little for a (token, count) table of 2048 entries at a sane load): the count of token t is built in the
 * row's own word t, whose value the log entries naming t hold in registers meanwhile.  The bound is those registers —
 * 4 entries for each of the 1024 threads.
 * Errors: hx_sample_rows_resident's rules; penalty_params or token_log NULL: HX_ERR_NULL; log_slots < 1, log_cap < 1 or
 * log_cap > HX_SAMPLE_LOG_MAX: HX_ERR_SHAPE — nothing is launched.  The dynamic-LDS rule of hx_sample_rows_resident holds
 * unchanged (for this kernel: one call outside a capture must have gone before). */
#define HX_SAMPLE_LOG_MAX 4096
int hx_sample_rows_resident_penalized(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows, int64_t n,
                                      int64_t ld, const void* sample_params, const int32_t* positions,
                                      const void* penalty_params, int32_t* token_log, int64_t log_slots, int64_t log_cap,
                                      int dtype, hx_stream stream);
/* hx_sample_rows_constrained: hx_sample_rows with a per-row logit bias table and a min_p cut, still one launch and one
 * read of the logits (extension; added WITHOUT raising HX_ABI_VERSION: nothing that existed changed).  Everything
 * hx_sample_rows documents holds word for word, with two additions.
 * The bias table is a CSR like the history: row r owns (bias_ids[j], bias_values[j]) for cu_bias[r] <= j < cu_bias[r + 1]
 * (cu_bias int32 [rows + 1], its values are held inside [0, bias_total] by the kernel; bias_values fp32), the ids of a
 * row pairwise distinct.  For a bias entry (t, b) of row r, after the row is staged as fp32 and BEFORE the penalties:
 *     x_t = (float)logits[r, t] + b          one fp32 addition
 * and the penalised value s_t of a history entry, with everything downstream, is computed from that x_t (a token may be
 * in both tables).  b = -inf bans the token: its value stays -inf through the penalties (r > 0) and it is in no kept
 * set.  An entry with t < 0 or t >= n is ignored: nothing is read or written for it.  A token that appears twice in one
 * row's table breaks the contract: the row uses one of the sums, nothing is read or written out of bounds.  A row whose
 * every element is banned has a largest z that is not finite: hx_sample_rows' degenerate row (the greedy id — index 0 —
 * and cut NaN).  bias_total == 0 is legal: bias_ids, bias_values and cu_bias may then be NULL.
 * min_p is word [3] of the row's record, as fp32 (hx_sample_rows keeps ignoring that word).  Off when not > 0 (a NaN
 * included); ignored on greedy and degenerate rows; a value above 1 acts as 1.  With m = max z and e_i = expf(z_i - m):
 *     M = {i : e_i >= min_p},   v_M = min z over M,   v_K' = max(v_K, v_M)
 * and top-p and the draw use v_K' wherever hx_sample_rows uses v_K: Z_K is the sum of e over {z >= v_K'}, v* >= v_K', and
 * with top_p >= 1, v* = v_K'.  The kept set is a threshold set on z: tied values stand or fall together.
 * A greedy row (T == 0) rides through: bias, then penalties, then the id in hx_argmax_rows' order.
 * Errors: hx_sample_rows' rules; bias_total < 0 or > 0x7fffffff: HX_ERR_SHAPE; bias_ids, bias_values or cu_bias NULL
 * with bias_total > 0: HX_ERR_NULL — nothing is launched. */
int hx_sample_rows_constrained(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows, int64_t n,
                               int64_t ld, const int32_t* hist_ids, const int32_t* hist_counts, const int32_t* cu_hist,
                               int64_t total, const float* penalties, const int32_t* bias_ids, const float* bias_values,
                               const int32_t* cu_bias, int64_t bias_total, const void* sample_params, int dtype,
                               hx_stream stream);
/* hx_sample_rows_logprobs: hx_sample_rows_constrained that also SCORES the token it chose, under the distribution it
 * chose it from, still one launch and one read of the logits (extension; added WITHOUT raising HX_ABI_VERSION: nothing
 * that existed changed).  ids, cut_out and u_out are hx_sample_rows_constrained's bit for bit, whatever want and top_k.
 * want: int32 [rows], may be NULL (every row is scored).  logprobs fp32 [rows]; top_ids int32 / top_logprobs fp32, dense
 * [rows, top_k], top_k in 0..20 (both may be NULL with top_k == 0).  Per row r:
 *   want[r] < 0 — not scored: logprobs[r] NaN, top_ids -1, top_logprobs NaN; the row does what it does in
 *   hx_sample_rows_constrained and nothing more (a greedy row leaves before the selection).
 *   Scored: T' = T if T > 0, else 1; z_i = s_i / T' (s: the biased, penalised value); m = max z; e_i = expf(z_i - m).
 *   The kept set S is {z_i >= v*} for a sampled row and every index for a greedy one (which ignores top_k, top_p and
 *   min_p, as its choice does).  Z_S: the fp32 sum of e over S — for a sampled row the very value the draw was made
 *   against, for a greedy row the same reduction over the whole row.
 *       lp_i = (z_i - m) - logf(Z_S)   for i in S,   -inf outside S
 *   logprobs[r] = lp of ids[r], always finite (a greedy row: -logf(Z_S)).  top_ids[r, :top_k]: the first top_k indices
 *   in the order (larger z, then lower index) — hx_argmax_rows' order — each with its lp: -inf when it lies outside S,
 *   but named all the same; entries past n: id -1, -inf.
 *   Scored and degenerate (a NaN in the row, or a largest z that is not finite): the id as in hx_sample_rows, logprobs[r]
 *   NaN, top_ids -1, top_logprobs NaN.
 * Errors: hx_sample_rows_constrained's rules; top_k outside 0..20: HX_ERR_SHAPE; logprobs NULL, or top_ids / top_logprobs
 * NULL with top_k > 0: HX_ERR_NULL — nothing is launched. */
int hx_sample_rows_logprobs(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows, int64_t n,
                            int64_t ld, const int32_t* hist_ids, const int32_t* hist_counts, const int32_t* cu_hist,
                            int64_t total, const float* penalties, const int32_t* bias_ids, const float* bias_values,
                            const int32_t* cu_bias, int64_t bias_total, const void* sample_params, float* logprobs,
                            int32_t* top_ids, float* top_logprobs, int top_k, const int32_t* want, int dtype,
                            hx_stream stream);
/* hx_sample_rows_masked: hx_sample_rows_logprobs under per-row TOKEN MASKS (allowed_token_ids, guided_choice), still one
 * launch and one read of the logits (extension; added WITHOUT raising HX_ABI_VERSION: nothing that existed changed).
 * allow_words: uint32 [n_masks, words], words = (n + 31) / 32 — the bitmask format grammar engines exchange: bit t & 31 of
 * word t >> 5 of a mask is set when token t may be chosen; bits at positions >= n in the last word are ignored.
 * mask_row: int32 [rows], the index of the row's mask in allow_words; a value < 0 or >= n_masks: the row is unmasked and
 * nothing of allow_words is read for it.  Step 1a, after the row is staged as fp32 and BEFORE the bias table: every
 * element of a masked row whose bit is clear becomes -inf (a bias entry on such a token keeps it -inf: biases are
 * finite or -inf).  The mask's words are read from global memory once per row; no LDS is added.
 * Scoring is optional per launch as well as per row: with logprobs == NULL no row is scored, and top_ids, top_logprobs,
 * top_k and want are not read.
 * The contract:
 *   A masked row gives, bit for bit, the ids, cut_out, u_out, logprobs, top_ids and top_logprobs that
 *   hx_sample_rows_logprobs gives for the same row with -inf written into the logits at the masked positions; with
 *   logprobs == NULL the ids, cut_out and u_out of hx_sample_rows_constrained.
 *   An unmasked row gives exactly what those entries give for it.
 *   A row whose surviving elements are all -inf is hx_sample_rows' degenerate row: id 0, cut NaN.  That id may lie
 *   OUTSIDE the mask: the kernel does not special-case it, the caller must not let it happen (a mask with no bit set
 *   below n; a mask whose every token is banned by a -inf bias).
 * Errors: with logprobs != NULL hx_sample_rows_logprobs' rules, else hx_sample_rows_constrained's; n_masks < 0 or
 * > 0x7fffffff: HX_ERR_SHAPE; mask_row NULL, or allow_words NULL with n_masks > 0: HX_ERR_NULL — nothing is launched. */
int hx_sample_rows_masked(int64_t* ids, float* cut_out, float* u_out, const void* logits, int64_t rows, int64_t n,
                          int64_t ld, const int32_t* hist_ids, const int32_t* hist_counts, const int32_t* cu_hist,
                          int64_t total, const float* penalties, const int32_t* bias_ids, const float* bias_values,
                          const int32_t* cu_bias, int64_t bias_total, const void* sample_params, float* logprobs,
                          int32_t* top_ids, float* top_logprobs, int top_k, const int32_t* want,
                          const uint32_t* allow_words, int64_t n_masks, const int32_t* mask_row, int dtype,
                          hx_stream stream);
/* The same product for M <= 32 with the activations held in REGISTERS (csrc/gemm_xreg.hip): a
 * workgroup spans the whole K of its split, so K <= 4096 needs ONE slab (no K split) and K = 11008
 * three instead of eleven — the fp32 slab traffic of a decode layer drops from 25 MB to 6.5 MB.
 * The weight must be packed by hx_pack_decode_weight_xreg (same 1 KiB fragment format as
 * hx_pack_decode_weight, blocks ordered [K split][row group][k-step in split] with the split size
 * this kernel chooses for K; interleave_halves != 0 alternates the 16-row groups of the two halves
 * of N — gate and up of a fused gate|up weight — for hx_gate_up_silu_xreg).
 * x is row-major [M, K] (row stride ldx) or, with x_fragment_major != 0, FRAGMENT-MAJOR: the 16-byte
 * piece ((k/32) * MB + m/16) * 64 + ((k%32)/8) * 16 + m%16, MB = ceil(M/16), holds x[m][8*(k/8) .. +8]
 * — the MFMA B operands in the order the kernel loads them (buffer: hx_fragment_major_elems(M, K)
 * elements; rows M .. 16*MB-1 are never read for a stored result).  hx_add_rms_norm_slabs_ex /
 * hx_silu_and_mul_slabs_ex / hx_gate_up_silu_xreg produce that layout.
 * hx_linear_decode_partial_xreg returns the number of slabs written (>= 1) or a negative HX_ERR_*.
 * Accumulation order differs from hx_linear_decode_partial (per-wave k ranges, then the four waves
 * in order): deterministic, not bit-identical to it.  N % 16 == 0, K % 32 == 0.
 * hx_gate_up_silu_xreg: act = silu(x Wg^T) * (x Wu^T) in one launch for K with a single split
 * (hx_gate_up_silu_xreg_supported), act fragment-major [inter]; rounding exactly as
 * hx_linear_decode_partial_xreg -> hx_silu_and_mul_slabs (bit-identical, tested); like that form it leaves rows
 * M .. 16*MB-1 of act as they were.
 * Replaces: torch.nn.functional.linear at decode batch sizes and silu(gate) * up
 * (hydrainfer/model/llama.py:24-27,48-50, model_forward.py:36). */
int hx_linear_decode_xreg_supported(int64_t M, int64_t N, int64_t K);
int hx_linear_decode_xreg_splits(int64_t N, int64_t K);
int64_t hx_linear_decode_xreg_workspace_bytes(int64_t M, int64_t N, int64_t K);
int64_t hx_fragment_major_elems(int64_t rows, int64_t K);
int hx_pack_decode_weight_xreg(void* packed, const void* weight, int64_t N, int64_t K, int64_t ldw,
                               int interleave_halves, int dtype, hx_stream stream);
int hx_linear_decode_partial_xreg(float* partial, const void* x, const void* packed_weight,
                                  int64_t M, int64_t N, int64_t K, int64_t ldx, int x_fragment_major,
                                  int64_t partial_bytes, int dtype, hx_stream stream);
/* hx_add_rms_norm_slabs FUSED IN FRONT of the product (one launch instead of two): workgroup r < M of
 * the GEMM grid first computes row r of
 *     residual += (T) sum of the n_splits_in slabs of slabs_in [n_splits_in][M][K];  x = rms_norm(residual) * norm_weight
 * (bit-identical to hx_add_rms_norm_slabs_ex with fragment-major output), writes it to x_frag
 * (hx_fragment_major_elems(M, K) elements, a scratch the caller may read afterwards) and counts itself
 * in at `sync`; all workgroups prefetch their weights meanwhile, wait for the last row, then load x.
 * sync: HX_XREG_SYNC_WORDS int32 words, ZERO before the launch, one area per launch in flight (word 1
 * is set if a workgroup gave up waiting after 1 s — never expected).  Needs K in one split of the packing
 * (hx_norm_xreg_supported; M <= 32 for the gate|up + silu*mul form, M <= 64 for the plain product).  slabs_in must not alias the outputs.  Results equal
 * hx_add_rms_norm_slabs_ex + hx_linear_decode_partial_xreg resp. hx_gate_up_silu_xreg bit for bit. */
#define HX_XREG_SYNC_WORDS 512
int hx_norm_xreg_supported(int64_t M, int64_t N, int64_t K, int gate_up);
int hx_norm_linear_decode_xreg(float* partial, void* residual, const float* slabs_in, int32_t n_splits_in,
                               const void* norm_weight, float epsilon, void* x_frag,
                               const void* packed_weight, int64_t M, int64_t N, int64_t K, void* sync,
                               int64_t partial_bytes, int dtype, hx_stream stream);
int hx_norm_gate_up_silu_xreg(void* act, void* residual, const float* slabs_in, int32_t n_splits_in,
                              const void* norm_weight, float epsilon, void* x_frag,
                              const void* packed_gate_up, int64_t M, int64_t inter, int64_t K, void* sync,
                              int dtype, hx_stream stream);
/* Batches of 33 .. 64 rows (the reference's linear layers have no batch limit: hydrainfer/model/llama.py:24-27,48-50):
 * hx_linear_decode_partial_xreg and hx_norm_linear_decode_xreg take M <= 64 — above 32 rows a workgroup spans HALF of a
 * packed K split (x for 64 rows fills the registers at half the k-steps) over the SAME packing, so the slab count doubles
 * (2 for K <= 4096) and no second copy of the weights is needed; hx_*_supported / _workspace_bytes answer per M.  The
 * gate|up product then comes WITHOUT the fused silu*mul (it needs the whole K): hx_gate_up_xreg / hx_norm_gate_up_xreg
 * multiply by the interleaved gate|up packing and write fp32 slabs [n_splits][M][2*inter] in plain [gate | up] column
 * order for hx_silu_and_mul_slabs; they return the slab count (any M <= 64). */
int hx_gate_up_xreg_supported(int64_t M, int64_t inter, int64_t K, int with_norm);
int64_t hx_gate_up_xreg_workspace_bytes(int64_t M, int64_t inter, int64_t K);
int hx_gate_up_xreg(float* partial, const void* x, const void* packed_gate_up, int64_t M, int64_t inter, int64_t K,
                    int64_t ldx, int x_fragment_major, int64_t partial_bytes, int dtype, hx_stream stream);
int hx_norm_gate_up_xreg(float* partial, void* residual, const float* slabs_in, int32_t n_splits_in,
                         const void* norm_weight, float epsilon, void* x_frag, const void* packed_gate_up,
                         int64_t M, int64_t inter, int64_t K, void* sync, int64_t partial_bytes, int dtype,
                         hx_stream stream);
/* hx_norm_gate_up_silu_wide_xreg (round 5): the norm-fused gate|up product of 33 .. 64 rows WITH silu * mul — one launch
 * and no slabs instead of hx_norm_gate_up_xreg + hx_silu_and_mul_slabs.  A workgroup does BOTH K halves of its (gate, up)
 * row-group pairs one after the other (x of the first half, all its units — their reduced tiles wait in LDS —, x of the
 * second half, the units again) and writes act (fragment-major, ceil(M / 16) row blocks, as hx_silu_and_mul_slabs_ex with
 * out_fragment_major) with the same order of summation and the same roundings: bit-identical to the two-launch form.
 * Supported where the packing's one split is two full halves of 16 k-steps per wave (K = 4096: LLaVA-1.5-7B). */
int hx_gate_up_silu_wide_xreg_supported(int64_t M, int64_t inter, int64_t K);
int hx_norm_gate_up_silu_wide_xreg(void* act, void* residual, const float* slabs_in, int32_t n_splits_in,
                                   const void* norm_weight, float epsilon, void* x_frag,
                                   const void* packed_gate_up, int64_t M, int64_t inter, int64_t K, void* sync,
                                   int dtype, hx_stream stream);
int hx_gate_up_silu_xreg_supported(int64_t M, int64_t inter, int64_t K);
int hx_gate_up_silu_xreg(void* act, const void* x, const void* packed_gate_up, int64_t M,
                         int64_t inter, int64_t K, int64_t ldx, int x_fragment_major, int dtype,
                         hx_stream stream);
/* What a launch of the activations-in-registers kernels WILL BE, answered on the host from the plan and the
 * instantiation tables the launches themselves read (tests choose their shapes with it; nothing is launched).
 * hx_debug_xreg_plan: the launch of M rows over a [N, K] weight — gate_up: the interleaved gate|up packing (N = 2 *
 *   inter); wide: the 33 .. 64-row kernel (which hx_gate_up_xreg runs at every row count); epi: with the silu*mul
 *   epilogue.  out[0] kernel (0 = 32-row kernel, 1 = wide kernel), out[1] k-steps per wave (the instantiation), out[2]
 *   16-row blocks of x, out[3] K splits of the launch (the slabs of a plain product), out[4] splits of the packing,
 *   out[5] workgroups, out[6] dynamic LDS bytes, out[7] 1 if the shape has a built instantiation and a grid, else 0
 *   (the other words are then what the plan got to).  Whether NORM / EPI are built for it: the *_supported entries.
 * hx_debug_xreg_built: row `index` of the 32-row (wide = 0) or the wide kernel's table of built instantiations:
 *   out[0] k-steps per wave, out[1] 1 if built with the norm in front, out[2] 1 if built with the silu*mul epilogue
 *   (wide kernel: behind the norm only).  index past the end (or negative): HX_ERR_SHAPE.
 * out == NULL: HX_ERR_NULL. */
int hx_debug_xreg_plan(int64_t M, int64_t N, int64_t K, int gate_up, int wide, int epi, int32_t out[8]);
int hx_debug_xreg_built(int wide, int index, int32_t out[3]);
/* Slab consumers: sum the n_splits slabs in order, round once to T (the projection's output
 * rounding), then behave exactly like hx_add_rms_norm / hx_silu_and_mul on that tensor.
 * partial: [n_splits][rows][hidden] resp. [n_splits][rows][2*inter] (gate | up columns). */
int hx_add_rms_norm_slabs(void* out, void* residual, const float* partial, int32_t n_splits,
                          const void* weight, float epsilon, int64_t rows, int64_t hidden,
                          int dtype, hx_stream stream);
int hx_silu_and_mul_slabs(void* out, const float* partial, int32_t n_splits, int64_t rows,
                          int64_t inter, int dtype, hx_stream stream);
/* The same two consumers with the output optionally FRAGMENT-MAJOR (see hx_linear_decode_partial_xreg;
 * hidden resp. inter % 32 == 0): values bit-identical to the row-major form. */
int hx_add_rms_norm_slabs_ex(void* out, void* residual, const float* partial, int32_t n_splits,
                             const void* weight, float epsilon, int64_t rows, int64_t hidden,
                             int dtype, int out_fragment_major, hx_stream stream);
int hx_silu_and_mul_slabs_ex(void* out, const float* partial, int32_t n_splits, int64_t rows,
                             int64_t inter, int dtype, int out_fragment_major, hx_stream stream);

/* ------------------------------------------------------------------------
 * Variable-length attention forward, dense or paged.
 * replaces: csrc/kernel/flash_attn/flash_api.cpp:216-355 (mha_varlen_fwd)
 *           hydrainfer/_C/kernel/flash_attn/__init__.pyi:23-40
 *
 * out, q : [n_tokens, n_heads, head_dim], row strides o_row_stride / q_row_stride,
 *          head stride = head_dim (heads contiguous).
 * dense  : block_table == NULL; k, v: [total_k, n_kv_heads, head_dim] with
 *          kv_row_stride / kv_head_stride.
 * paged  : block_table != NULL (flat int32 [sum blocks]) with cu_block_lens int32
 *          [batch+1]; k, v: [n_blocks, block_size, n_kv_heads, head_dim] with
 *          kv_block_stride / kv_row_stride / kv_head_stride; block_size % 16 == 0.
 * cu_seqlens_q / cu_seqlens_k: int32 [batch+1] (device).
 * causal != 0: key j visible to query i iff j <= i + (kv_len - q_len)
 *          (bottom-right aligned; reference mask.h:173-193, window (-1,0)).
 * softcap, local windows and ALiBi slopes: see the tail of hx_attn_args (flags & HX_ATTN_LOCAL_WINDOW,
 *          flags & HX_ATTN_ALIBI).
 * workspace: device scratch of at least hx_mha_varlen_fwd_workspace_bytes() bytes
 * (used for split-KV partials; may be NULL when that returns 0).
 * ---------------------------------------------------------------------- */
typedef struct hx_attn_args {
  void* out;
  const void* q;
  const void* k;
  const void* v;
  const int32_t* cu_seqlens_q;
  const int32_t* cu_seqlens_k;
  const int32_t* block_table;   /* NULL => dense */
  const int32_t* cu_block_lens; /* required iff block_table */
  int32_t batch;
  int32_t n_heads;
  int32_t n_kv_heads;
  int32_t head_dim;
  int32_t block_size;    /* paged only */
  int32_t max_seqlen_q;
  int32_t max_seqlen_k;
  int32_t total_q;       /* rows of q */
  int64_t q_row_stride;
  int64_t o_row_stride;
  int64_t k_block_stride, k_row_stride, k_head_stride;
  int64_t v_block_stride, v_row_stride, v_head_stride;
  float softmax_scale;
  int32_t causal;
  int32_t dtype;         /* HX_F16 | HX_BF16 */
  int32_t num_splits;    /* 0 = choose automatically, 1 = never split */
  void* workspace;
  int64_t workspace_bytes;
  /* flash_api.cpp:93-111.  softcap > 0: scores = softcap * tanh(q.k * softmax_scale / softcap)
   * before masking; 0 = off.  Local attention only when flags & HX_ATTN_LOCAL_WINDOW: query row i (of
   * q_len rows, kv_len keys) sees keys [i + kv_len - q_len - window_left, i + kv_len - q_len + window_right]
   * (mask.h:173-193); a negative bound = unbounded on that side; `causal` must be 0 then (causal IS the
   * window (-1, 0)).  Without the flag window_left / window_right are ignored, so an all-zero tail of
   * the struct (the usual C initialisation) means "no softcap, no window". */
  float softcap;
  int32_t window_left;
  int32_t window_right;
  int32_t flags;         /* HX_ATTN_* bits; unknown bits -> HX_ERR_UNSUPPORTED */
  /* ALiBi (flash_api.cpp:197-214), read only when flags & HX_ATTN_ALIBI: fp32 slopes on the device, [n_heads]
   * (alibi_batch_stride = 0) or [batch, n_heads] (alibi_batch_stride = elements between two sequences' vectors,
   * >= 0); the pointer must be 4-byte aligned and softmax_scale > 0.  Sequence b, head h, query row i (of q_len rows)
   * and key j (of kv_len keys):
   *   score(i, j) = f(q_i.k_j * softmax_scale) - alibi_slopes[b * alibi_batch_stride + h] * |i + kv_len - q_len - j|
   * with f the soft cap above (or the identity): the bias is added after the cap and before the masks.  Under a
   * causal mask the reference adds slope * j instead (mask.h:157-158), a constant per row apart: the same softmax.
   * hx_decode_attention_fused answers the flag with HX_ERR_UNSUPPORTED (it fuses RoPE; ALiBi models have none).
   * These two fields were appended WITHOUT raising HX_ABI_VERSION (still 3): a zero-filled tail keeps meaning "off",
   * and a caller detects the feature by the flag itself — a library built before it answers the unknown flag bit
   * with HX_ERR_UNSUPPORTED and never reads past `flags`. */
  const float* alibi_slopes;
  int64_t alibi_batch_stride;
} hx_attn_args;
#define HX_ATTN_LOCAL_WINDOW 1
#define HX_ATTN_ALIBI 2

int64_t hx_mha_varlen_fwd_workspace_bytes(const hx_attn_args* args);
int hx_mha_varlen_fwd(const hx_attn_args* args, hx_stream stream);

/* Extension (SURVEY §8f-2 taken to the end): one launch for the three consecutive steps of a
 * decode layer — apply_rotary_pos_emb(q, k) (NeoX, rotary_dim == head_dim), set_kv_cache(slots,
 * k, v) and the paged attention itself (hydrainfer/model/model_forward.py:78-84 +
 * hydrainfer/layer/causal_attention.py:401-406).  `args` is an all-decode batch (q_len 1) whose
 * cu_seqlens_k already counts the new token; args->q, k_new, v_new are UN-rotated; the kernel
 * rotates in registers (same T-arithmetic rounding), attends with the new token taken from
 * registers and appends its rotated key / value to the cache at new_cache_slots.
 * Results are bit-identical to the three separate ops. */
typedef struct hx_fused_decode_args {
  const void* k_new;          /* [batch, n_kv_heads, head_dim] */
  const void* v_new;          /* [batch, n_kv_heads, head_dim] */
  int64_t k_new_row_stride;
  int64_t v_new_row_stride;
  const int32_t* positions;   /* [batch] */
  const void* cos_sin;        /* [max_pos, 2, head_dim/2] in the tensors' dtype */
  const int32_t* new_cache_slots; /* [batch] */
  int32_t rotary_dim;
  int32_t interleaved;
  /* optional: take q / k_new / v_new from the split-K slabs of the fused qkv projection
   * ([qkv_splits][batch][(n_heads + 2*n_kv_heads) * head_dim] fp32, hx_linear_decode_partial);
   * args->q, k_new, v_new are then ignored */
  const float* qkv_partial;
  int32_t qkv_splits;
  /* optional (may be NULL): the batch's RANK DESCRIPTOR, int32 [1 + batch] on the device — [0] = 1 when the batch is
   * ragged, [1 + r] = the sequence with the r-th most keys (hx_decode_rank / hx_decode_advance_ranked /
   * hx_step_head_args.rank_desc write it).  With it a big ragged batch is laid over the CUs in length-ranked snake
   * order (same results bit for bit, csrc/attn_decode.hip RANKED); without it: the static (head, sequence) grid. */
  const int32_t* rank_desc;
} hx_fused_decode_args;
int hx_decode_attention_fused(const hx_attn_args* args, const hx_fused_decode_args* fused,
                              hx_stream stream);

/* ------------------------------------------------------------------------
 * Cache-block migration between GPUs / processes.
 * replaces: csrc/data_transfer/block_migration.cpp:55-59 (get_ipc_mem_handle),
 *           :69-80 (register_ipc_mem_handle), :194-245 (migrate_blocks)
 *           hydrainfer/_C/data_transfer/block_migration/__init__.pyi:6-18
 * ---------------------------------------------------------------------- */
#define HX_IPC_HANDLE_BYTES 64
/* Writes the 64-byte hipIpcMemHandle_t of the allocation containing dev_ptr and the
 * byte offset of dev_ptr inside it. */
int hx_ipc_get_mem_handle(const void* dev_ptr, uint8_t handle_out[HX_IPC_HANDLE_BYTES],
                          int64_t* offset_out);
/* Opens (or returns the cached mapping of) a peer handle.  Mappings are cached by
 * handle bytes for the life of the process: the reference re-opens per call
 * (block_migration.cpp:213-215) which HIP rejects for an already-open handle. */
int hx_ipc_open_mem_handle(const uint8_t handle[HX_IPC_HANDLE_BYTES], void** dev_ptr_out);
int hx_ipc_close_all(void);

/* dst[l, t, dst_table[i]] = src[l, t, src_table[i]] for every layer l, token-kind t
 * (k/v) and i < n_pairs, as ONE gather-copy kernel per <=HX_MIGRATE_MAX_PAIRS pairs.
 * Pools are contiguous 6-D (n_layers, n_tokens, n_blocks, block_size, n_heads, head_size);
 * block_bytes = block_size*n_heads*head_size*itemsize (multiple of 16).
 * src may be an IPC-mapped peer pointer (xGMI read) or a local pointer. */
#define HX_MIGRATE_MAX_PAIRS 448
int hx_migrate_blocks(const int32_t* src_table_host, const int32_t* dst_table_host,
                      int64_t n_pairs, const void* src_pool, void* dst_pool,
                      int64_t n_layers, int64_t n_tokens, int64_t src_n_blocks,
                      int64_t dst_n_blocks, int64_t block_bytes, hx_stream stream);

/* Pack / unpack selected blocks to / from a contiguous staging buffer
 * [n_layers, n_tokens, n_pairs, block_bytes] — the RCCL send/recv path
 * (replaces the per-(block,layer,k/v) P2POp list of
 * hydrainfer/memory/communication.py:57-74). */
int hx_pack_blocks(const int32_t* table_host, int64_t n_pairs, const void* pool, void* staging,
                   int64_t n_layers, int64_t n_tokens, int64_t n_blocks, int64_t block_bytes,
                   hx_stream stream);
int hx_unpack_blocks(const int32_t* table_host, int64_t n_pairs, const void* staging, void* pool,
                     int64_t n_layers, int64_t n_tokens, int64_t n_blocks, int64_t block_bytes,
                     hx_stream stream);

/* The same three copies over pools whose (layer, k/v) PLANES are not back to back: plane p of a pool starts
 * p * plane_bytes past the pool's base and holds n_blocks blocks contiguously (plane_bytes >= n_blocks * block_bytes,
 * multiple of 16; n_planes = n_layers * n_tokens).  The entries above are these with plane_bytes = n_blocks * block_bytes —
 * the reference's contiguous 6-D tensor (hydrainfer/memory/token_cache_manger.py:65).
 * Why a pool would want spare bytes between planes (round 5, tools/probes/attn_placement.py): K and V of one
 * (block, token, head) are read by the same wave at the same time, and in the contiguous pool they lie n_blocks *
 * block_bytes apart — a large power-of-two multiple — so both land on the same HBM channel; with the V plane an odd
 * multiple of 256 bytes further on, decode attention of 64 sequences runs 5 % faster, the 64-row decode step 3 %, the
 * 13B step 1 % (hydrainfer_amd/memory/kv_pool.py allocates pools that way; the plane stride travels with the pool's
 * IPC handle). */
int hx_migrate_blocks_planes(const int32_t* src_table_host, const int32_t* dst_table_host,
                             int64_t n_pairs, const void* src_pool, void* dst_pool, int64_t n_planes,
                             int64_t src_n_blocks, int64_t dst_n_blocks, int64_t src_plane_bytes,
                             int64_t dst_plane_bytes, int64_t block_bytes, hx_stream stream);
int hx_pack_blocks_planes(const int32_t* table_host, int64_t n_pairs, const void* pool, void* staging,
                          int64_t n_planes, int64_t n_blocks, int64_t pool_plane_bytes, int64_t block_bytes,
                          hx_stream stream);
int hx_unpack_blocks_planes(const int32_t* table_host, int64_t n_pairs, const void* staging, void* pool,
                            int64_t n_planes, int64_t n_blocks, int64_t pool_plane_bytes, int64_t block_bytes,
                            hx_stream stream);

/* ------------------------------------------------------------------------
 * Decode-step metadata advance: device-resident equivalent of one
 * AttentionParametersBuilder pass for an all-decode batch
 * (hydrainfer/layer/causal_attention.py:147-168).  For every sequence b:
 *   positions[b] += stride; kv_len[b] += stride; cu_seqlens_k = prefix-sum(kv_len);
 *   new_cache_slots[b] = block_table[cu_block_lens[b] + pos/bs]*bs + pos%bs.
 * stride = 1 is the reference's step; a benchmark that samples the generation's contexts at a fixed spacing
 * uses a larger one.  Lets a whole decode step live inside one hipGraph / launch plan.
 * hx_decode_feed_ids: the step's input ids with one step of look-ahead (engine/graph_decode.py): row r takes the
 * token the PREVIOUS launch sampled for row src[r] (prev, int64, still on the device) when src[r] >= 0, else the
 * host-written ids[r].  hx_collect_errors: out[0] = OR over i < n_areas of areas[i * stride_words + word], OR
 * extra[0] if given — the give-up words of a step's in-kernel hand-overs folded into ONE word that travels to the
 * host with the step's tokens.
 * ---------------------------------------------------------------------- */
int hx_decode_advance(int32_t* positions, int32_t* kv_lens, int32_t* cu_seqlens_k,
                      int32_t* new_cache_slots, const int32_t* block_table,
                      const int32_t* cu_block_lens, int32_t batch, int32_t block_size,
                      int32_t stride, hx_stream stream);
/* hx_decode_advance that also leaves the advanced batch's rank descriptor (hx_fused_decode_args.rank_desc) in rank_desc
 * (int32 [1 + batch]); hx_decode_rank: the descriptor alone, from cu_seqlens_k (int32 [batch + 1]).  A batch of more
 * than 256 sequences is declared even ([0] = 0).  The engine's host-built steps write the same words from the host
 * (hydrainfer_amd/layer/causal_attention.py::decode_rank_descriptor). */
int hx_decode_advance_ranked(int32_t* positions, int32_t* kv_lens, int32_t* cu_seqlens_k,
                             int32_t* new_cache_slots, const int32_t* block_table,
                             const int32_t* cu_block_lens, int32_t batch, int32_t block_size,
                             int32_t stride, int32_t* rank_desc, hx_stream stream);
int hx_decode_rank(const int32_t* cu_seqlens_k, int32_t batch, int32_t* rank_desc, hx_stream stream);
/* hx_decode_step_head: everything a decode step does before its first GEMM as ONE launch — hx_embed_rms_norm for
 * `rows` rows (each id optionally replaced by the previous launch's sample like hx_decode_feed_ids: feed_src /
 * feed_prev, both or neither; fed_out, if given, receives the ids used), hx_memset_zero of zero_bytes at zero_ptr
 * (the hand-over areas of the step's norm-fused launches; 0 = none) and hx_decode_advance for `batch` sequences
 * (0 = none).  The three parts touch disjoint memory; each is bit-identical to the separate call. */
typedef struct hx_step_head_args {
  void* h_out;               /* [rows, hidden] embedding rows */
  void* x_out;               /* [rows, hidden] rms_norm(h_out) * weight */
  const void* ids;           /* [rows] int32 or int64 */
  const int32_t* feed_src;   /* [rows] or NULL */
  const int64_t* feed_prev;  /* previous launch's samples, or NULL */
  int64_t* fed_out;          /* [rows] or NULL */
  const void* table;         /* [vocab, hidden] */
  const void* weight;        /* [hidden] */
  void* zero_ptr;            /* 16-byte aligned, or NULL */
  int64_t zero_bytes;        /* multiple of 4 */
  int32_t* positions;        /* hx_decode_advance arguments (batch = 0: unused) */
  int32_t* kv_lens;
  int32_t* cu_seqlens_k;
  int32_t* new_cache_slots;
  const int32_t* block_table;
  const int32_t* cu_block_lens;
  int64_t rows, hidden, vocab;
  float epsilon;
  int32_t ids_are_int64;
  int32_t dtype;             /* HX_F16 | HX_BF16 */
  int32_t batch, block_size, stride;
  int32_t* rank_desc;        /* NULL, or int32 [1 + batch]: the advanced batch's rank descriptor (hx_decode_advance_ranked) */
} hx_step_head_args;
int hx_decode_step_head(const hx_step_head_args* args, hx_stream stream);
/* hx_stage_decode: a decode step's integer inputs into the engine's RESIDENT device buffer (engine/graph_decode.py) —
 * the step's head (ids, positions, slots, cumulative lengths, table offsets, rank descriptor: head_words words, copied to
 * dst[0 ..)) and the block-table DELTAS behind it: staging[head_words] = n_runs, then per run [dst word offset] [count]
 * [count values].  A sequence's table stays where it is on the device; a step writes only the block ids that are new
 * (the reference rebuilds and re-copies every table every step: hydrainfer/engine/parameters_builder.py:46-97).
 * staging: host memory the device can read (pinned); dst_words bounds every write. */
int hx_stage_decode(void* dst, int64_t dst_words, const void* staging, int32_t head_words, hx_stream stream);
int hx_decode_feed_ids(int64_t* out, const int32_t* ids, const int32_t* src, const int64_t* prev,
                       int32_t n, hx_stream stream);
int hx_collect_errors(uint32_t* out, const uint32_t* areas, int32_t n_areas, int64_t stride_words,
                      int32_t word, const uint32_t* extra, hx_stream stream);
/* hx_copy_words2: dst0[0 .. n0) = src0[..], dst1[0 .. n1) = src1[..] (32-bit words, 4-byte aligned, n1 may be 0) as ONE
 * kernel launch.  Any of the four pointers may be host-mapped pinned memory (hipHostMalloc / torch pin_memory): this is how
 * the engine's decode loop moves a step's few hundred integers in and its sampled tokens out (engine/graph_decode.py) —
 * a hipMemcpyAsync between two graph launches cost the stream ~40-120 us of idle time per copy on this ROCm (round 5,
 * rocprofv3 trace of the serving leg: three copyBuffer launches per step with 9 / 0 / 123 us in front of them); a kernel
 * is just the next packet in the queue.  Results written to pinned memory are visible to the host once an event recorded
 * behind the launch has completed (the reference's step does a blocking .tolist(), hydrainfer/engine/executor.py). */
int hx_copy_words2(void* dst0, const void* src0, int32_t n0_words, void* dst1, const void* src1, int32_t n1_words,
                   hx_stream stream);

/* ------------------------------------------------------------------------
 * Launch plans: record the launches of a fixed sequence of hx_* calls once, replay them with one
 * native loop — the role of the hipGraph in the reference's unfinished
 * hydrainfer/model_runner/cuda_graph_model_runner.py:1-72.  Between hx_plan_begin and hx_plan_end every hx_* entry
 * point called on the recording thread appends its kernel launches (hx_memset_zero included) to the plan instead of
 * executing them; nothing runs, no stream is touched.  hx_plan_launch issues them on a stream, in order, with the
 * recorded arguments (pointers are recorded by value: the buffers must stay allocated and in place, like a graph's).
 * One recording per thread at a time; a plan may be replayed from any thread.  hx_plan_size: recorded launches.
 * ---------------------------------------------------------------------- */
typedef struct hx_plan hx_plan;
int hx_plan_begin(hx_plan** plan);
int hx_plan_end(hx_plan* plan);
int hx_plan_size(const hx_plan* plan);
int hx_plan_launch(const hx_plan* plan, hx_stream stream);
int hx_plan_destroy(hx_plan* plan);
/* memset(p, 0, bytes) on the stream as a kernel launch; recordable in a plan, capturable in a hipGraph. */
int hx_memset_zero(void* p, int64_t bytes, hx_stream stream);
/* Measurement aid (SURVEY §8d "measured streaming ceiling"; no reference counterpart): reads `bytes` bytes at p
 * once, the way the weight-streaming kernels of this library read — 1 KiB contiguous per wave instruction,
 * non-temporal, ONE 8 KiB chunk (eight 1 KiB loads) in flight per wave, consumed before the next eight are requested,
 * 512 workgroups of 4 waves — and does nothing with them.  bench.py times it to report the read rate this GPU reaches
 * in this run beside the 8 TB/s vendor peak.  bytes % 8192 == 0, p 16-byte aligned; sink: one float the kernel never
 * writes (keeps the loads alive). */
int hx_measure_read_stream(const void* p, int64_t bytes, float* sink, hx_stream stream);
/* Measurement aids for the "null layer" (round 5; tools/null_layer.py, bench.py `whole_step.null_step`): the decode
 * layer's launches with the arithmetic, the activations and the hand-overs removed — what ANY design that runs a layer
 * as the same number of launches over the same bytes can reach on this GPU.
 *   hx_measure_read_grid   the kernel of hx_measure_read_stream over `n_workgroups` workgroups (the real grid of the
 *                          weight-streaming launch it stands in for: 256 = one per CU);
 *   hx_measure_paged_read  the decode attention kernel's read pattern and grid — (head, sequence) workgroups of 4
 *                          waves, wave w owns the 16-key tiles w, w + 4, ..., a tile = one page of the paged cache
 *                          (block_size 16): this head's 256 B (head_bytes) of 16 K rows and 16 V rows at a pitch of
 *                          row_bytes, pages looked up in `table` (n_seq rows of table_stride int32), two tiles in
 *                          flight per wave — nothing computed, nothing written.  head_bytes must be 256.
 * Both record into launch plans like every other launch. */
int hx_measure_read_grid(const void* p, int64_t bytes, int n_workgroups, float* sink, hx_stream stream);
int hx_measure_paged_read(const void* kbase, const void* vbase, const int32_t* table, int64_t table_stride, int n_seq,
                          int n_heads, int tiles, int64_t page_bytes, int64_t row_bytes, int head_bytes, float* sink,
                          hx_stream stream);

/* ------------------------------------------------------------------------
 * MoE routing / permutation ops (named in north_star; no production caller in the reference).
 * replaces: csrc/kernel/moe/moe_kernel.h:6-39, moe_kernels_pybind.cpp:7-15
 *           hydrainfer/_C/kernel/moe/__init__.pyi:4-145
 * ---------------------------------------------------------------------- */
/* gating_logits f32 [n_tokens, n_experts] -> topk_weights f32 / topk_indices i32
 * [n_tokens, topk]: softmax over experts then iterative arg-max, lower index wins ties
 * (topk_softmax_kernel.cu:108-180).  n_experts <= 1024 (any value, not only powers of 2). */
int hx_topk_softmax(const float* gating_logits, float* topk_weights, int32_t* topk_indices,
                    int64_t n_tokens, int64_t n_experts, int64_t topk, hx_stream stream);
/* DeepSeek-V3 routing (grouped_topk_sigmoid_kernel.cu:15-181): score = sigmoid(logit);
 * choice = score + bias; drop (n_groups - topk_group) groups ranked by the sum of their two
 * largest choices (ties: higher group dropped first); top-k over the kept experts by choice
 * (ties: lower expert); weights = score of the chosen experts, NOT renormalised;
 * scaling_factor is accepted and, like the reference (:180), not applied. */
int hx_grouped_topk_sigmoid(const float* gating_logits, const float* correction_bias,
                            float* topk_weights, int32_t* topk_indices, int64_t n_tokens,
                            int64_t n_experts, int64_t n_groups, int64_t topk_group,
                            int64_t topk, float scaling_factor, hx_stream stream);
/* row_id_map i32 [topk, n_tokens] from a STABLE sort of the flattened topk_indices by expert
 * (permutation_index_kernel.cu:39-77): the element with flat index f = t*topk + k that lands at
 * sorted position p gives row_id_map[k*n_tokens + t] = p. */
int64_t hx_moe_sort_workspace_bytes(int64_t n_tokens, int64_t topk);
int hx_moe_row_id_map_from_indices(const int32_t* topk_indices, int32_t* row_id_map,
                                   int64_t n_tokens, int64_t topk, void* workspace,
                                   int64_t workspace_bytes, hx_stream stream);
/* row_id_map i32 [n_experts, n_tokens] from a boolean routing map [n_tokens, n_experts]
 * (permutation_mask_kernel.cu:43-130): running count in expert-major, token-minor order where
 * routed, -1 elsewhere.  workspace >= 4*n_experts bytes. */
int hx_moe_row_id_map_from_mask(const uint8_t* routing_map, int32_t* row_id_map,
                                int64_t n_tokens, int64_t n_experts, void* workspace,
                                int64_t workspace_bytes, hx_stream stream);
/* permuted[row_id_map[r*n_tokens + t], :] = tokens[t, :] for every map row r with entry >= 0
 * (n_rows = topk for an index map, n_experts for a mask map). */
int hx_moe_permute(const void* tokens, void* permuted, const int32_t* row_id_map,
                   int64_t n_tokens, int64_t n_rows, int64_t dim, int dtype, hx_stream stream);
/* out[t,:] = sum_r probs[t,r] * permuted[row_id_map[r*n_tokens + t], :] over entries >= 0,
 * product and running sum in T arithmetic like the reference's frag_sum
 * (permutation_index_kernel.cu:146-160); probs has the tokens' dtype, [n_tokens, n_rows],
 * NULL = weight 1. */
int hx_moe_unpermute(const void* permuted, void* out, const int32_t* row_id_map,
                     const void* probs, int64_t n_tokens, int64_t n_rows, int64_t dim,
                     int dtype, hx_stream stream);
/* out[t,:] = sum_k in[t,k,:] with the reference's arithmetic (align_block_kernel.cu:172-188,242-272): topk in {2,3,4,8} —
 * topk_sum_kernel's instantiations — keep the running sum in T (every partial sum rounded), any other topk accumulates in
 * fp32 and rounds once (torch::sum_out). */
int hx_moe_sum_out(const void* in, void* out, int64_t n_tokens, int64_t topk, int64_t dim,
                   int dtype, hx_stream stream);

/* ------------------------------------------------------------------------
 * Sparse MoE feed-forward (csrc/moe_experts.hip): router, segments, grouped expert GEMMs, combine.
 * replaces: hydrainfer/model/deepseek_v3.py:61-93 (MoEGate.forward), :114-121 (DeepseekV3MoE.forward),
 *           :124-155 (moe_infer: a Python loop over experts around a tokens_per_expert.cpu() host sync)
 * n tokens, E <= 256 routed experts, topk <= 8, hidden h and expert intermediate I multiples of 128, T = fp16 / bf16;
 * stacked contiguous weights w_gate_up [E, 2I, h] (gate rows, then up rows) and w_down [E, h, I]; slot s = t * topk + k.
 * No entry synchronises or reads anything back; every grid depends on (E, I, h, n, topk) only, so a step captures into
 * a hipGraph; results are deterministic (no floating-point atomics).
 * ---------------------------------------------------------------------- */
#define HX_MOE_SCORE_SOFTMAX 0
#define HX_MOE_SCORE_SIGMOID 1
/* deepseek_v3.py:61-93 with scoring_func = "softmax", topk_method = "greedy": logits[t, e] = sum_h float(x[t, h]) *
 * float(router_weight[e, h]) in fp32 (router_weight [E, h] in x's dtype or fp32), fp32 softmax over the experts, top-k
 * with ties to the lower index (the rule of hx_topk_softmax), weights = w / (sum_k w + 1e-20) * routed_scaling_factor
 * when norm_topk_prob and topk > 1 (:88), else w * routed_scaling_factor.  topk_weights f32 / topk_ids i32 [n, topk].
 * scoring != HX_MOE_SCORE_SOFTMAX or group-limited routing (n_group > 1 or topk_group > 1): HX_ERR_UNSUPPORTED —
 * hx_grouped_topk_sigmoid is the entry for that. */
int hx_moe_gate_topk(float* topk_weights, int32_t* topk_ids, const void* x, const void* router_weight,
                     int64_t n_tokens, int64_t hidden, int64_t n_experts, int64_t topk, int x_dtype,
                     int weight_dtype, int scoring, int64_t n_group, int64_t topk_group, int norm_topk_prob,
                     float routed_scaling_factor, hx_stream stream);
/* deepseek_v3.py:125-130 (scatter_, argsort, .cpu()) on the device, one small launch: seg (int32,
 * hx_moe_segments_elems() elements) = [ exclusive offsets E + 1 | per-expert row counts E | the n * topk slots grouped
 * by expert ].  Order inside a group is unspecified (a slot's result does not depend on its place); an id outside
 * [0, E) puts its slot in no group, and the rows of that slot are then written by neither GEMM. */
int64_t hx_moe_segments_elems(int64_t n_tokens, int64_t topk, int64_t n_experts);
int hx_moe_segments(int32_t* seg, const int32_t* topk_ids, int64_t n_tokens, int64_t topk, int64_t n_experts,
                    hx_stream stream);
/* deepseek_v3.py:138-140 with GateUpDownMLP, first half: for every routed slot s = (t, k), e = topk_ids[t, k]:
 * act[s, j] = T(float(T(silu(float(g)))) * float(u)), g = T(sum_h x[t, h] * Wg_e[j, h]), u = T(sum_h x[t, h] * Wu_e[j, h])
 * (fp32 accumulation, one rounding, as nn.Linear).  x [n, h], act [n * topk, I] in slot order: no permuted copy of x. */
int hx_moe_gate_up_silu(void* act, const void* x, const void* w_gate_up, const int32_t* seg, int64_t n_tokens,
                        int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter, int dtype, hx_stream stream);
/* ... second half (down_proj): y[s, c] = T(sum_j act[s, j] * Wd_e[c, j]), y [n * topk, h]. */
int hx_moe_down(void* y, const void* act, const void* w_down, const int32_t* seg, int64_t n_tokens, int64_t topk,
                int64_t n_experts, int64_t hidden, int64_t inter, int dtype, hx_stream stream);
/* deepseek_v3.py:148-154 and :120: out[t, c] = T( float(T( sum_k topk_weights[t, k] * float(y[t * topk + k, c]) )) +
 * float(shared[t, c]) ), products and sum in fp32, k order; shared [n, h] (the shared experts' output) may be NULL:
 * out = T(sum). */
int hx_moe_combine(void* out, const void* y, const float* topk_weights, const void* shared, int64_t n_tokens,
                   int64_t topk, int64_t hidden, int dtype, hx_stream stream);
/* The two grouped GEMMs over FP8 block-scaled expert weights (csrc/moe_experts_fp8.hip): the format DeepSeek-V3-family
 * checkpoints publish.  wq_gate_up [E, 2I, h] / wq_down [E, h, I]: one byte per element, OCP float8_e4m3fn (a byte 0x7F /
 * 0xFF is a NaN weight), contiguous, 16-byte aligned; w_scale fp32 [E, 2I/128, h/128] resp. [E, h/128, I/128]
 * (`weight_scale_inv`: weight = float(q) * scale, one scale per 128 x 128 block; gate rows then up rows, scales too).
 * Weight-only: x / act / y stay T = `dtype` (HX_F16 / HX_BF16), seg is hx_moe_segments' output.  With
 *   lin(row n of expert e, token row v) = T( sum_b w_scale[e, n / 128, b] * ( sum_{k in 128-block b} float(v[k]) * float(q[e, n, k]) ) )
 * — the inner sums fp32 MFMA accumulation of exact products, a block's scale multiplying the block's fp32 partial sum in
 * fp32 (one fma into the running sum), ONE rounding to T at the end, no weight ever rounded to T after scaling — act and
 * y are what hx_moe_gate_up_silu / hx_moe_down define with lin in place of their dot products: the same silu * mul
 * rounding points, the same slot order, the same grids; an expert with no rows reads no weight bytes and no scales.
 * Status as the 16-bit entries: NULL (w_scale included) HX_ERR_NULL, the shape rules HX_ERR_SHAPE, fp32 HX_ERR_DTYPE;
 * nothing is launched on a refusal. */
int hx_moe_gate_up_silu_fp8w(void* act, const void* x, const void* wq_gate_up, const float* w_scale, const int32_t* seg,
                             int64_t n_tokens, int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter, int dtype,
                             hx_stream stream);
int hx_moe_down_fp8w(void* y, const void* act, const void* wq_down, const float* w_scale, const int32_t* seg,
                     int64_t n_tokens, int64_t topk, int64_t n_experts, int64_t hidden, int64_t inter, int dtype,
                     hx_stream stream);

/* ------------------------------------------------------------------------
 * Focal image-token pruning without a score tensor (csrc/focal_prune.hip).
 * replaces: hydrainfer/layer/token_prunning.py:5-37 (focal_prunning) fed with the pre-softmax scaled logits of
 *           hydrainfer/layer/multihead_attention.py:59-62 (`attention_scores`, a view of `score` taken before the softmax)
 * Per image, N = tokens_per_image - skip_leading tokens, H heads, head dim D:
 *   S_h[i, j] = (q[i,h,:] * scale) . k[j,h,:];  A = mean_h S_h;  s1[j] = mean_i A[i, j];  s2[i] = mean_j A[i, j]
 *   sig = var(s1) > var(s2) ? s1 : s2  (unbiased variance);  'rank': keep the n tokens of largest sig;  'row': g = sqrt(N),
 *   keep all tokens of the n / g grid rows with the largest sum of sig;  ties go to the lower index;  ids ascending.
 * Every reduction is linear in S, so s1 / s2 come from q and k directly (column sums, then one dot product per token):
 * no N x N tensor, no host synchronisation.  All three are deterministic (no floating-point atomics, fixed summation
 * order), record into launch plans and capture into hipGraphs.
 *
 * hx_focal_significance (token_prunning.py:17-21 over multihead_attention.py:59-62): q, k [n_images * tokens_per_image,
 *   n_heads, head_dim] f16 / bf16, heads contiguous, row strides in elements (multiples of 8, 16-byte aligned bases);
 *   the first skip_leading tokens of every image (CLIP's CLS: 1) take no part, neither as query nor as key.  s1, s2: fp32
 *   [n_images, N].  head_dim % 8 == 0, n_heads * head_dim <= 8192, N <= 4096.  workspace: at least
 *   hx_focal_significance_workspace_bytes(n_images, n_heads, head_dim) bytes, 4-byte aligned.
 * hx_focal_select (token_prunning.py:22-35): n_keep int32 [n_images] ON THE DEVICE (clamped to 0 .. N); ids_out int32
 *   [n_images, N]: the first n_keep[b] entries of row b are the kept ids in ascending order, the rest -1.  strategy
 *   HX_FOCAL_ROW needs a square N (HX_ERR_SHAPE) and keeps n_keep[b] / g whole rows (the caller, who knows the counts,
 *   refuses n % g != 0).  Variances in fp32, two passes; var(s1) == var(s2) or NaN -> s2.
 * hx_focal_gather (token_prunning.py:36): out[b, r, :] = tokens[b, ids[b, r], :] for r < n_keep[b], bit-exact 16-byte
 *   copies; rows r >= n_keep[b] (and ids outside 0 .. N-1) are not written.  tokens and out hold N rows per image at
 *   row strides token_row_stride / out_row_stride elements; hidden * itemsize and both strides multiples of 16 bytes.
 * ---------------------------------------------------------------------- */
#define HX_FOCAL_RANK 0
#define HX_FOCAL_ROW 1
int64_t hx_focal_significance_workspace_bytes(int64_t n_images, int64_t n_heads, int64_t head_dim);
int hx_focal_significance(float* s1, float* s2, const void* q, const void* k, int64_t n_images,
                          int64_t tokens_per_image, int64_t skip_leading, int64_t n_heads, int64_t head_dim,
                          int64_t q_row_stride, int64_t k_row_stride, float scale, void* workspace,
                          int64_t workspace_bytes, int dtype, hx_stream stream);
int hx_focal_select(int32_t* ids_out, const float* s1, const float* s2, const int32_t* n_keep,
                    int64_t n_images, int64_t N, int strategy, hx_stream stream);
int hx_focal_gather(void* out, const void* tokens, const int32_t* ids, const int32_t* n_keep,
                    int64_t n_images, int64_t N, int64_t hidden, int64_t token_row_stride,
                    int64_t out_row_stride, int dtype, hx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* HYDRA_HIP_H */
