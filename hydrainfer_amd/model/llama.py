"""Llama decoder (the language half of LLaVA-1.5) — the caller of the hot path.

Mirrors hydrainfer/model/llama.py:21-104 + hydrainfer/model/model_forward.py:39-105:
    h = h + o_proj(Attn(rope(q_proj, k_proj), v_proj)) ; h = h + down(silu(gate) * up)
with pre-RMSNorm, greedy argmax inside the model (llama.py:99-104), last-layer token
selection for prefill (model_forward.py:101-103).

MI355X-first differences (all rounding-neutral with respect to the reference's unfused ops):
  * q/k/v and gate/up weights are stored fused ([3h, h] and [2i, h]) so a layer is 4 library
    GEMMs instead of 7; `from_reference_state_dict` builds them from the reference's names.
  * residual-add + RMSNorm, RoPE (in place on the qkv buffer), set_kv_cache + attention and
    silu*mul each run as one HIP launch.
GEMMs are plain library GEMMs (torch.matmul -> hipBLASLt); everything else is libhydra_hip."""
import os
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch
from torch import Tensor

from hydrainfer_amd._C.kernel.activation import silu_and_mul, silu_and_mul_slabs
from hydrainfer_amd._C.kernel.norm import (StepHead, add_rms_norm, add_rms_norm_slabs, argmax_rows, decode_step_head,
                                             embed_rms_norm, embed_rms_norm_supported, logprob_rows, rms_norm)
from hydrainfer_amd._C.kernel.position_embedding import rope_set_kv_cache
from hydrainfer_amd.layer.causal_attention import AttentionParameters
from hydrainfer_amd._C.kernel.flash_attn import decode_attention_fused, mha_varlen_fwd
from hydrainfer_amd._C.kernel import gemm as hip_gemm
from hydrainfer_amd import _lib, launch_plan
from hydrainfer_amd.model.decode_plan import Dims, Layouts, StepPlan, mlp_xreg_ok, plan_layouts, resolve, wide_ok


@dataclass
class LlamaShape:
    hidden_size: int
    intermediate_size: int
    num_hidden_layers: int
    num_attention_heads: int
    num_key_value_heads: int
    head_dim: int
    vocab_size: int
    rms_norm_eps: float = 1e-5
    rope_theta: float = 10000.0
    max_position_embeddings: int = 4096


# SURVEY.md §8 model constants
LLAVA_1_5_7B = LlamaShape(4096, 11008, 32, 32, 32, 128, 32064)
LLAVA_1_5_13B = LlamaShape(5120, 13824, 40, 40, 40, 128, 32064)


@dataclass
class LanguageModelParameters:
    """hydrainfer/model/parameters.py:21-29 (fields used by the language model)."""
    attention_params: List[AttentionParameters]
    all_sequences_decode: bool
    selected_token_ids: Optional[Tensor] = None  # int64 index tensor on the device
    image_row_index: Optional[Tensor] = None     # int64 rows of the batch that are image tokens (host knows them:
                                                 # spares the nonzero() sync of a boolean-mask assignment)
    step_head: Optional[StepHead] = None         # decode loops: metadata advance / look-ahead feed folded into the step's
                                                 # first launch (hx_decode_step_head); the model runs it or raises


def build_cos_sin(shape: LlamaShape, dtype: torch.dtype, device) -> Tensor:
    inv = 1.0 / torch.pow(shape.rope_theta,
                          torch.arange(0, shape.head_dim, 2, dtype=torch.float) / shape.head_dim)
    t = torch.arange(shape.max_position_embeddings, dtype=torch.float)
    freqs = torch.einsum("i,j->ij", t, inv)
    cs = torch.cat([freqs.cos()[:, None, :], freqs.sin()[:, None, :]], dim=1)
    return cs.to(dtype).to(device)


class LlamaForCausalLM:
    """Weights live in fused device tensors; `state` maps fused names to tensors."""

    # FP8 block-scaled dense linears (state[key] float8_e4m3fn + state[key + "_scale"]): only a subclass whose decode
    # step runs on the general path offers them (model/deepseek_moe.py) — the in-register decode plan packs 16-bit weights
    fp8_dense = False

    def __init__(self, shape: LlamaShape, dtype: torch.dtype, device, state: Dict[str, Tensor]):
        self.shape, self.dtype, self.device = shape, dtype, torch.device(device)
        self.state = state
        if not self.fp8_dense:
            fp8 = sorted(k for k, v in state.items() if k.endswith("_scale") or v.dtype == torch.float8_e4m3fn)
            if fp8:
                raise ValueError(f"{type(self).__name__}: FP8 block-scaled weights ({', '.join(fp8[:4])}{', ...' if len(fp8) > 4 else ''}) "
                                 "are not supported by this model's decode plan, which packs 16-bit weights; "
                                 "DeepseekMoeForCausalLM runs them")
        self.fp8_scratch: Optional[Tensor] = None   # T [elements of the largest FP8 dense weight]: linear()'s dequantised copy
        self.cos_sin = build_cos_sin(shape, dtype, self.device)
        self.q_size = shape.num_attention_heads * shape.head_dim
        self.kv_size = shape.num_key_value_heads * shape.head_dim
        self.dims = Dims(shape.hidden_size, shape.intermediate_size, self.q_size, self.q_size + 2 * self.kv_size, shape.num_hidden_layers)
        # decode batches (<= 64 rows) stream the weights through the HIP kernel; larger
        # batches (prefill) use the library GEMM
        self.use_hip_gemm = True
        # decode steps: RoPE + cache append + attention as one launch.  Grouped-query models take
        # three launches instead (GEMM reduce, RoPE + append, attention): the fused kernel gives
        # every query head its own workgroup, the unfused entry picks attn_decode_gqa.hip, which
        # reads each KV head once (3x faster at group 4 and more than pays for the two launches)
        self.fuse_decode_attention = (shape.head_dim in (64, 128, 256)
                                      and shape.num_key_value_heads == shape.num_attention_heads)
        # decode GEMMs stream PACKED copies of the weights (MFMA-fragment order, contiguous 1 KiB
        # reads: csrc/gemm_skinny.hip gemm_packed_kernel); the row-major tensors stay for the
        # prefill GEMMs (library).  288 GB of HBM: the second copy of a 7B / 13B model is 13 / 26 GB.
        self.use_packed = True
        self.packed: Dict[str, Tensor] = {}
        # decode batches of <= 32 rows: the MLP runs on the activations-in-registers GEMM
        # (csrc/gemm_xreg.hip) — gate|up + silu*mul in ONE launch that needs no K split, down with 3
        # slabs instead of 11; the activations travel between these launches in MFMA-fragment order.
        # 7 launches per layer, -7.5 us per 7B layer (tools/bench_layer_xreg.py).
        self.use_xreg = True
        # qkv of layers >= 1 on the same kernel (its x comes fragment-major from the previous layer's
        # add+norm; the attention prologue then reads 1 slab instead of 4): -45 us per 7B step
        self.xreg_qkv = os.environ.get("HX_XREG_QKV", "1") == "1"
        # the two add+norm launches of a layer run INSIDE the gate|up and qkv launches (the first 32
        # workgroups produce x while all prefetch weights; in-kernel hand-over): 5 launches per layer
        self.fuse_norm = os.environ.get("HX_FUSE_NORM", "1") == "1"
        # batches of 33 .. 64 rows on the same layout (the wide kernel: 6 launches per layer, no LDS-slice copies)
        self.use_wide = os.environ.get("HX_WIDE", "1") == "1"
        # ... with silu * mul inside the norm + gate|up launch (round 5: both K halves in one workgroup, no slabs)
        self.use_wide_silu = os.environ.get("HX_WIDE_SILU", "1") == "1"
        self.sample_out: Optional[Tensor] = None   # int64 [rows]: forward() writes the sampled ids here (decode loops)
        self.xreg_sync: Optional[Tensor] = None   # [L, 2, XREG_SYNC_WORDS] of the last step (word 1 = wait gave up)
        self.packed_x: Dict[str, Tensor] = {}
        self.dw: Dict[str, "hip_gemm.DecodeWeight"] = {}       # descriptors of the packed copies (xreg layout)
        self.dw_lds: Dict[str, "hip_gemm.DecodeWeight"] = {}   # ... (LDS-slice layout)
        self.decode_layouts: Optional[Layouts] = None          # what pack_decode_weights built (None: nothing yet)
        # decode-side weight layouts are built ONCE, by prepare_decode (engine build / runner construction), for
        # the largest decode batch the owner will ever run — never in the middle of serving
        self.decode_rows_prepared = 0
        self.decode_only = False                   # row-major decoder weights dropped (D-role node)

    # ------------------------------------------------------------------ decode-side weight layouts
    def prepare_decode(self, max_rows: int = 64, keep_row_major: bool = True) -> None:
        """Builds every packed layout a decode batch of <= max_rows rows can need, now (model load, before the
        KV pool is sized): the activations-in-registers layout for gate|up, down and qkv of layers >= 1 (<= 32
        rows), the LDS-slice layout for o and layer 0's qkv — and for all four projections when max_rows > 32
        (batches of 33..64 rows run on that kernel).  keep_row_major=False is for nodes that never prefill
        (parallel.epd_roles: "D"): the row-major decoder weights — only the library prefill GEMMs read them —
        are released, ONE copy of the weights stays resident.  Reference: one nn.Linear weight per projection
        (hydrainfer/model/llama.py:24-27,48-50)."""
        max_rows = min(int(max_rows), 64)
        if max_rows > self.decode_rows_prepared and not self.decode_only:
            self.pack_decode_weights(all_lds_slice=max_rows > 32 and not self._wide_ok(max_rows))
            self.decode_rows_prepared = max_rows
        if not keep_row_major and not self.decode_only and len(set(self.packed) | set(self.packed_x)) == 4 * self.shape.num_hidden_layers:
            for l in range(self.shape.num_hidden_layers):
                for n in ("wqkv", "wo", "wgu", "wdown"):
                    w = self.state[f"l{l}.{n}"]
                    # shape / stride / dtype carrier without storage: anything that tries to read it fails loudly
                    self.state[f"l{l}.{n}"] = torch.empty_strided(w.shape, w.stride(), dtype=w.dtype, device="meta")
            self.decode_only = True

    def weight_bytes_resident(self) -> int:
        """Bytes of HBM the weights occupy in all their layouts (row-major + packed copies)."""
        tensors = [v for v in self.state.values() if v.device.type != "meta"]
        tensors += list(self.packed.values()) + list(self.packed_x.values())
        return sum(t.numel() * t.element_size() for t in tensors)

    def release(self) -> None:
        """Drops every weight tensor (bench.py frees the 7B model before its 13B leg)."""
        self.state, self.packed, self.packed_x, self.dw, self.dw_lds = {}, {}, {}, {}, {}
        self.xreg_sync = self.decode_layouts = self.fp8_scratch = None

    def handover_failed(self) -> bool:
        """True if an in-kernel hand-over of the last decode step gave up waiting (word 1 of a norm-fused
        launch's sync area): that step's activations are garbage.
        One small D2H sync — callers on the hot path fold the flag into their token copy instead
        (engine/graph_decode.py)."""
        bad = False
        if self.xreg_sync is not None:
            bad = bool(int(self.xreg_sync[:, :, 1].abs().sum()) != 0)
        return bad

    def handover_error_word(self) -> Optional[Tensor]:
        """int32 scalar tensor on the device, nonzero iff a hand-over of the step just enqueued gave up; None when
        the step had no in-kernel hand-over.  Enqueued on the current stream (capturable)."""
        if self.xreg_sync is not None:
            return self.xreg_sync[:, :, 1].abs().sum().to(torch.int32)
        return None

    def pack_decode_weights(self, all_lds_slice: bool = False) -> None:
        """Builds the packed copies that decode_plan.plan_layouts names (prepare_decode calls this; never during a capture)
        through the library's one decode-weight entry (gemm.DecodeWeight) and records them in decode_layouts, which the step
        plan reads.  all_lds_slice: batches of 33..64 rows are announced that the wide kernel cannot take."""
        L = self.shape.num_hidden_layers
        ok = self.use_hip_gemm and all(self.state[f"l{l}.{p}"].stride(1) == 1 for l in range(L) for p in ("wqkv", "wo", "wgu", "wdown"))
        lay = plan_layouts(self.dims, self.dtype, self if ok else None, all_lds_slice, self.decode_layouts)
        for key in lay.xreg_keys(L):
            if key not in self.packed_x:
                dw = hip_gemm.DecodeWeight(self.state[key], max_rows=32, gate_up=key.endswith("wgu"))
                assert dw.layout == "xreg"
                self.dw[key], self.packed_x[key] = dw, dw.packed
        for key in sorted(lay.lds_slice - set(self.packed)):     # row-major x in (o, layer 0's qkv) / 13B-like shapes
            dw = hip_gemm.DecodeWeight(self.state[key], max_rows=64, lds_slice=True)
            assert dw.layout == "lds_slice"
            self.dw_lds[key], self.packed[key] = dw, dw.packed
        # how gate|up is packed: from here on the descriptor's answer (before: the predicate hx_decode_weight_plan decides by)
        self.decode_layouts = replace(lay, gu_interleaved=self.dw["l0.wgu"].interleaved) if lay.mlp_xreg else lay

    def _new_sync(self, device) -> Tensor:
        return torch.empty((self.shape.num_hidden_layers, 2, hip_gemm.XREG_SYNC_WORDS), dtype=torch.int32, device=device)

    def _layouts(self) -> Layouts:
        return self.decode_layouts or plan_layouts(self.dims, self.dtype)

    def _xreg_mlp_ok(self, n: int) -> bool:
        return self._wide_ok(n) if n > 32 else mlp_xreg_ok(self.dims, n, self.dtype)

    def _wide_ok(self, n: int) -> bool:
        """Batches of 33 .. 64 rows on the activations-in-registers layout (LLaVA-1.5-7B and -13B; other shapes stay on
        LDS-slice copies)."""
        return wide_ok(self.dims, n, self.dtype, self, self._layouts().gu_interleaved)

    def _partial(self, x: Tensor, key: str, ws: Tensor) -> int:
        """split-K slabs of x @ state[key]^T into ws; packed weights when available."""
        dw = self.dw_lds.get(key)
        if dw is not None:
            return hip_gemm.linear_decode_ex(x, dw, ws)
        if self.decode_only:
            raise RuntimeError(f"decode-only model: no packed layout of {key} for {x.shape[0]} rows (prepare_decode("
                               f"max_rows={self.decode_rows_prepared}) was called) and the row-major weight is released")
        return hip_gemm.linear_decode_partial(x, self.state[key], ws)

    def linear(self, x: Tensor, w: Tensor, scale: Optional[Tensor] = None) -> Tensor:
        """x @ w^T.  scale given: w is FP8 block-scaled bytes (float8_e4m3fn, one fp32 scale per 128 x 128 block).  Up to
        64 rows run on csrc/gemm_skinny_fp8.hip, which applies a block's scale to the block's fp32 partial sum and never
        rounds a scaled weight.  Larger batches (prefill) dequantise the weight into the model's scratch tensor
        (hx_dequant_fp8_block) and call the library GEMM: they multiply by T(q * s), a scaled weight ROUNDED to T — at
        most half an ulp of T per weight away from what decode multiplies by."""
        if w.device.type == "meta":
            raise RuntimeError("decode-only model (prepare_decode(keep_row_major=False)): prefill / row-major GEMMs "
                               "are not available on this node")
        if scale is not None:
            if not self.fp8_dense:
                raise ValueError(f"{type(self).__name__}.linear: FP8 block-scaled weights are not supported by this model")
            if self.use_hip_gemm and hip_gemm.fp8_supported(x, w, scale):
                return hip_gemm.linear_decode_fp8(x, w, scale)
            return torch.matmul(x, self._dequantised(w, scale, x.dtype).t())
        if self.use_hip_gemm and x.shape[0] <= 64 and hip_gemm.supported(x, w):
            return hip_gemm.linear_decode(x, w)
        return torch.matmul(x, w.t())

    def _dequantised(self, w: Tensor, scale: Tensor, dtype: torch.dtype) -> Tensor:
        """T(q * s) of an FP8 weight as a [N, K] view of ONE scratch tensor: sized to the largest FP8 2-d weight of the
        state, allocated at first use, reused by every call in stream order (its reader is the GEMM that follows)."""
        buf = self.fp8_scratch
        if buf is None or buf.dtype != dtype or buf.numel() < w.numel():
            n = max([v.numel() for v in self.state.values() if v.dim() == 2 and v.dtype == torch.float8_e4m3fn] + [w.numel()])
            buf = self.fp8_scratch = torch.empty(n, dtype=dtype, device=w.device)
        return hip_gemm.dequant_fp8_block(w, scale, dtype, out=buf[:w.numel()].view(w.shape))

    # ------------------------------------------------------------------ construction
    @classmethod
    def random_init(cls, shape: LlamaShape, dtype: torch.dtype, device, seed: int = 0,
                    std: float = 0.02) -> "LlamaForCausalLM":
        """N(0, std) linears/embeddings, norm weights 1 (SURVEY.md §8d synthetic weights)."""
        g = torch.Generator(device=device).manual_seed(seed)
        h, i, L = shape.hidden_size, shape.intermediate_size, shape.num_hidden_layers
        q, kv = shape.num_attention_heads * shape.head_dim, shape.num_key_value_heads * shape.head_dim

        def w(*size):
            return (torch.randn(size, generator=g, device=device, dtype=torch.float32) * std).to(dtype)

        st: Dict[str, Tensor] = {"embed": w(shape.vocab_size, h), "lm_head": w(shape.vocab_size, h),
                                 "norm": torch.ones(h, dtype=dtype, device=device)}
        for l in range(L):
            st[f"l{l}.wqkv"] = w(q + 2 * kv, h)
            st[f"l{l}.wo"] = w(h, q)
            st[f"l{l}.wgu"] = w(2 * i, h)
            st[f"l{l}.wdown"] = w(h, i)
            st[f"l{l}.norm1"] = torch.ones(h, dtype=dtype, device=device)
            st[f"l{l}.norm2"] = torch.ones(h, dtype=dtype, device=device)
        return cls(shape, dtype, device, st)

    @classmethod
    def from_reference_state_dict(cls, shape: LlamaShape, sd: Dict[str, Tensor], dtype, device,
                                  prefix: str = "") -> "LlamaForCausalLM":
        """Names of hydrainfer/model/llama.py (== HF Llama): model.layers.N.self_attn.q_proj.weight ..."""
        def t(name):
            return sd[prefix + name].to(dtype).to(device)
        st = {"embed": t("model.embed_tokens.weight"), "lm_head": t("lm_head.weight"),
              "norm": t("model.norm.weight")}
        for l in range(shape.num_hidden_layers):
            p = f"model.layers.{l}."
            st[f"l{l}.wqkv"] = torch.cat([t(p + "self_attn.q_proj.weight"), t(p + "self_attn.k_proj.weight"),
                                          t(p + "self_attn.v_proj.weight")], dim=0).contiguous()
            st[f"l{l}.wo"] = t(p + "self_attn.o_proj.weight")
            st[f"l{l}.wgu"] = torch.cat([t(p + "mlp.gate_proj.weight"), t(p + "mlp.up_proj.weight")],
                                        dim=0).contiguous()
            st[f"l{l}.wdown"] = t(p + "mlp.down_proj.weight")
            st[f"l{l}.norm1"] = t(p + "input_layernorm.weight")
            st[f"l{l}.norm2"] = t(p + "post_attention_layernorm.weight")
        return cls(shape, dtype, device, st)

    def to_reference_state_dict(self) -> Dict[str, Tensor]:
        """Unfused CPU copy under the reference's parameter names (consumed by the oracle)."""
        s, q, kv, i = self.state, self.q_size, self.kv_size, self.shape.intermediate_size
        sd = {"model.embed_tokens.weight": s["embed"].cpu(), "lm_head.weight": s["lm_head"].cpu(),
              "model.norm.weight": s["norm"].cpu()}
        for l in range(self.shape.num_hidden_layers):
            p = f"model.layers.{l}."
            wqkv, wgu = s[f"l{l}.wqkv"].cpu(), s[f"l{l}.wgu"].cpu()
            sd[p + "self_attn.q_proj.weight"] = wqkv[:q]
            sd[p + "self_attn.k_proj.weight"] = wqkv[q:q + kv]
            sd[p + "self_attn.v_proj.weight"] = wqkv[q + kv:]
            sd[p + "self_attn.o_proj.weight"] = s[f"l{l}.wo"].cpu()
            sd[p + "mlp.gate_proj.weight"] = wgu[:i]
            sd[p + "mlp.up_proj.weight"] = wgu[i:]
            sd[p + "mlp.down_proj.weight"] = s[f"l{l}.wdown"].cpu()
            sd[p + "input_layernorm.weight"] = s[f"l{l}.norm1"].cpu()
            sd[p + "post_attention_layernorm.weight"] = s[f"l{l}.norm2"].cpu()
        return sd

    def weight_bytes(self) -> int:
        """Bytes a decode step must stream: all linears + lm_head (embedding gather ignored),
        the `W` term of SURVEY.md §8d."""
        n = sum(v.numel() for k, v in self.state.items() if k != "embed" and v.dim() == 2)
        return n * self.state["lm_head"].element_size()

    # ------------------------------------------------------------------ forward
    def embed(self, input_ids: Tensor) -> Tensor:
        return torch.nn.functional.embedding(input_ids, self.state["embed"])

    def _decode_plan(self, n: int, dtype) -> dict:
        """Which launches a decode step of n rows is made of: the six flags of the resolved plan."""
        return resolve(self.dims, n, dtype, self, self._layouts()).flags()

    def _step_plan(self, n: int, dtype) -> StepPlan:
        """The plan of the step about to run.  Resolved per step and never cached (fuse_norm is cleared at run time after
        a hand-over gave up), before the step's first launch, which zeroes the hand-over areas the plan asks for."""
        if n > self.decode_rows_prepared and not self.decode_only:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"decode batch of {n} rows captured before prepare_decode(max_rows >= {n})")
            self.prepare_decode(max_rows=64)     # a caller that never announced its batch size (unit tests, ad-hoc scripts)
        return resolve(self.dims, n, dtype, self, self._layouts())

    def _decode_hidden_hip_gemm(self, h: Tensor, position_ids: Tensor, model_params: LanguageModelParameters, plan: StepPlan,
                                x0: Optional[Tensor] = None, sync: Optional[Tensor] = None) -> Tensor:
        """All-decode step of <= 64 rows on the weight-streaming HIP GEMMs and their fused slab consumers.  A layer is five
        stages — qkv, attention + o, norm2 + gate|up + silu*mul, down, close (residual add + the next norm) — each run in
        the variant `plan` names: five to eight launches, listed per plan in tests/decode_arms.py::SEQUENCES.  Nothing is
        decided here.  Same rounding points as the unfused path."""
        sh, n, last = self.shape, h.shape[0], self.shape.num_hidden_layers - 1
        f32 = lambda k: torch.empty(k, dtype=torch.float32, device=h.device)
        frag = lambda K: torch.empty(hip_gemm.fragment_major_elems(n, K), dtype=h.dtype, device=h.device)
        ws = f32(plan.ws)
        b = SimpleNamespace(n=n, h=h, x=x0, ws=ws, ws_q=f32(plan.ws_q) if plan.ws_q else ws, ws_gu=f32(plan.ws_gu) if plan.ws_gu else ws,
                            xf=frag(sh.hidden_size) if plan.xf else None, sync=sync,
                            actf=frag(sh.intermediate_size) if plan.actf or plan.actf_w else None)
        if plan.sync and sync is None:   # the caller did not come through the step head, whose launch zeroes the areas
            b.sync = self._new_sync(h.device)
            _lib.memset_zero(b.sync)
        if plan.sync:
            self.xreg_sync = b.sync
        if x0 is None:                   # else the first layer's norm came with the embedding gather
            b.x = torch.empty_like(h)
            rms_norm(b.x, h, self.state["l0.norm1"], sh.rms_norm_eps)
        s_qkv = None
        for l in range(last + 1):
            s_qkv = self._stage_qkv(plan.qkv if l else "rowmajor", l, b, s_qkv)
            s_o = self._stage_attention_o(l, b, s_qkv, position_ids, model_params.attention_params[l])
            act = self._stage_mlp_in(plan.mlp, l, b, s_o)
            s_dn = self._stage_down(plan.down, l, b, act)
            s_qkv = self._stage_close(plan.close if l < last else "rowmajor", l, b, s_dn)
        return b.x

    def _stage_qkv(self, variant: str, l: int, b, handed: Optional[int]) -> int:
        """Slabs of x @ wqkv^T in b.ws_q; returns their count."""
        key, hid = f"l{l}.wqkv", self.shape.hidden_size
        if variant == "handover":
            return handed
        if variant == "ex":
            return hip_gemm.linear_decode_ex(b.xf, self.dw[key], b.ws_q, frag_shape=(b.n, hid))
        if variant == "wide":
            return hip_gemm.linear_decode_partial_xreg(b.xf, self.packed_x[key], self.q_size + 2 * self.kv_size, b.ws_q, frag_shape=(b.n, hid))
        return self._partial(b.x, key, b.ws_q)

    def _stage_attention_o(self, l: int, b, s_qkv: int, position_ids: Tensor, ap: AttentionParameters) -> int:
        """[slab reduce + RoPE + cache append + attention], then the slabs of o @ wo^T in b.ws; returns their count."""
        H, HK, D = self.shape.num_attention_heads, self.shape.num_key_value_heads, self.shape.head_dim
        kc, vc = ap.kv_cache.get_kv_cache()
        o = torch.empty((b.n, H, D), dtype=b.h.dtype, device=b.h.device)
        # q / k_new / v_new arguments are shape carriers here: the kernel reads the slabs
        decode_attention_fused(o, o, o[:, :HK], o[:, :HK], kc, vc, position_ids, self.cos_sin,
                               ap.new_cache_slots, ap.q_cu_seq_lens, ap.kv_cu_seq_lens, ap.block_tables,
                               ap.cu_blocks_lens, ap.kv_max_seq_len, D ** -0.5, 0, b.ws_q, s_qkv, ap.decode_rank)
        return self._partial(o.view(b.n, self.q_size), f"l{l}.wo", b.ws)

    def _stage_mlp_in(self, variant: str, l: int, b, s_o: int) -> Tensor:
        """h += o; x = norm2(h); returns silu(x Wg^T) * (x Wu^T) as the down stage reads it: row-major for "slabs", else
        fragment-major.  The "norm_" variants produce x inside the gate|up launch (hand-over area b.sync[l, 0])."""
        n, h, ws, xf, nw, eps = b.n, b.h, b.ws, b.xf, self.state[f"l{l}.norm2"], self.shape.rms_norm_eps
        hid, inter = self.shape.hidden_size, self.shape.intermediate_size
        if variant == "slabs":
            add_rms_norm_slabs(b.x, h, ws, s_o, nw, eps)
            s_gu = self._partial(b.x, f"l{l}.wgu", ws)
            return silu_and_mul_slabs(ws, s_gu, n, inter, h.dtype)
        pgu = self.packed_x[f"l{l}.wgu"]
        if variant == "norm_silu":
            hip_gemm.norm_gate_up_silu_xreg(h, ws, s_o, nw, eps, xf, pgu, inter, b.actf, b.sync[l, 0])
            return b.actf
        if variant == "norm_wide_silu":     # 33 .. 64 rows, both K halves in one workgroup: no slabs
            hip_gemm.norm_gate_up_silu_wide_xreg(h, ws, s_o, nw, eps, xf, pgu, inter, b.actf, b.sync[l, 0])
            return b.actf
        if variant == "norm_wide":
            s_gu = hip_gemm.norm_gate_up_xreg(h, ws, s_o, nw, eps, xf, pgu, inter, b.ws_gu, b.sync[l, 0])
            return silu_and_mul_slabs(b.ws_gu, s_gu, n, inter, h.dtype, fragment_major=True)
        add_rms_norm_slabs(xf, h, ws, s_o, nw, eps, fragment_major=True)
        if variant == "silu":
            hip_gemm.gate_up_silu_xreg(xf, pgu, inter, b.actf, frag_shape=(n, hid))
            return b.actf
        if variant == "wide":
            s_gu = hip_gemm.gate_up_xreg(xf, pgu, inter, b.ws_gu, frag_shape=(n, hid))
        else:   # "plain" (b.ws_gu is ws), "wide_plain": halves in order, the plain product already gives [gate | up] columns
            s_gu = hip_gemm.linear_decode_partial_xreg(xf, pgu, 2 * inter, b.ws_gu, frag_shape=(n, hid))
        return silu_and_mul_slabs(b.ws_gu, s_gu, n, inter, h.dtype, fragment_major=True)

    def _stage_down(self, variant: str, l: int, b, act: Tensor) -> int:
        """Slabs of act @ wdown^T in b.ws; returns their count."""
        key, inter = f"l{l}.wdown", self.shape.intermediate_size
        if variant == "ex":
            return hip_gemm.linear_decode_ex(act, self.dw[key], b.ws, frag_shape=(b.n, inter))
        if variant == "wide":
            return hip_gemm.linear_decode_partial_xreg(act, self.packed_x[key], self.shape.hidden_size, b.ws, frag_shape=(b.n, inter))
        return self._partial(act, key, b.ws)

    def _stage_close(self, variant: str, l: int, b, s_dn: int) -> Optional[int]:
        """h += down; x = the next layer's first norm of h (after the last layer: the final norm).  "handover": the same
        launch also writes the next layer's qkv slabs and returns their count."""
        nxt = self.state[f"l{l + 1}.norm1" if l + 1 < self.shape.num_hidden_layers else "norm"]
        if variant == "handover":
            return hip_gemm.norm_linear_decode_xreg(b.h, b.ws, s_dn, nxt, self.shape.rms_norm_eps, b.xf, self.packed_x[f"l{l + 1}.wqkv"],
                                                    self.q_size + 2 * self.kv_size, b.ws_q, b.sync[l, 1])
        if variant == "fm":
            return add_rms_norm_slabs(b.xf, b.h, b.ws, s_dn, nxt, self.shape.rms_norm_eps, fragment_major=True)
        return add_rms_norm_slabs(b.x, b.h, b.ws, s_dn, nxt, self.shape.rms_norm_eps)

    def _decode_fast_path(self, n: int, dtype, model_params: LanguageModelParameters) -> bool:
        sh = self.shape
        return bool(self.use_hip_gemm and model_params.all_sequences_decode and self.fuse_decode_attention
                    and n <= 64 and dtype in (torch.float16, torch.bfloat16)
                    and sh.hidden_size % 256 == 0 and sh.intermediate_size % 256 == 0)

    def step_head_supported(self, n_rows: int) -> bool:
        """True if forward() of an all-decode batch of n_rows token ids runs LanguageModelParameters.step_head."""
        t = self.state["embed"]
        return bool(n_rows <= 64 and t.is_cuda and t.dtype in (torch.float16, torch.bfloat16) and t.is_contiguous()
                    and t.shape[1] % 8 == 0 and t.shape[1] <= 8192)

    def _mlp(self, l: int, x: Tensor) -> Tensor:
        """Layer l's feed-forward on the general path: down(silu(gate(x)) * up(x)).  A subclass with another MLP
        (model/deepseek_moe.py) overrides this."""
        inter = self.shape.intermediate_size
        gu = self.linear(x, self.state[f"l{l}.wgu"], self.state.get(f"l{l}.wgu_scale"))
        act = silu_and_mul(gu[:, :inter], gu[:, inter:])
        return self.linear(act, self.state[f"l{l}.wdown"], self.state.get(f"l{l}.wdown_scale"))

    def forward_hidden(self, input_ids_or_embeds: Tensor, position_ids: Tensor,
                       model_params: LanguageModelParameters) -> Tensor:
        sh, st = self.shape, self.state
        x0 = sync = None
        head = model_params.step_head
        is_ids = input_ids_or_embeds.dtype in (torch.int32, torch.int64)
        n, dtype = input_ids_or_embeds.shape[0], st["embed"].dtype if is_ids else input_ids_or_embeds.dtype
        plan = self._step_plan(n, dtype) if self._decode_fast_path(n, dtype, model_params) else None
        if is_ids:
            ids = input_ids_or_embeds
            if model_params.all_sequences_decode and ids.dim() == 1 and n <= 64 and embed_rms_norm_supported(ids, st["embed"]):
                # decode step: embedding gather + the first layer's norm + the zeroing of the hand-over areas of the
                # step's norm-fused launches + the caller's metadata advance / look-ahead feed: ONE launch
                if plan is not None and plan.sync:
                    sync = self._new_sync(ids.device)
                h, x0 = decode_step_head(ids, st["embed"], st["l0.norm1"], sh.rms_norm_eps, zero=sync, head=head)
                head = None
            else:
                h = self.embed(ids)
        else:
            h = input_ids_or_embeds
        if head is not None:
            raise RuntimeError("LanguageModelParameters.step_head needs the decode fast path (<= 64 rows of token ids, "
                               "fp16 / bf16 embedding table): the caller must run its advance / feed itself")
        if not h.is_contiguous():
            h = h.contiguous()
        if plan is not None:
            return self._decode_hidden_hip_gemm(h, position_ids, model_params, plan, x0, sync)
        n = h.shape[0]
        H, HK, D = sh.num_attention_heads, sh.num_key_value_heads, sh.head_dim
        q_size, kv_size = self.q_size, self.kv_size
        eps = sh.rms_norm_eps
        L = sh.num_hidden_layers

        if x0 is not None:
            x = x0
        else:
            x = torch.empty_like(h)
            rms_norm(x, h, st["l0.norm1"], eps)
        for l in range(L):
            ap = model_params.attention_params[l]
            qkv = self.linear(x, st[f"l{l}.wqkv"], st.get(f"l{l}.wqkv_scale"))
            q = qkv[:, :q_size].view(n, H, D)
            k = qkv[:, q_size:q_size + kv_size].view(n, HK, D)
            v = qkv[:, q_size + kv_size:].view(n, HK, D)
            kc, vc = ap.kv_cache.get_kv_cache()
            o = torch.empty((n, H, D), dtype=h.dtype, device=h.device)
            if model_params.all_sequences_decode and self.fuse_decode_attention:
                # RoPE + cache append + paged attention, one launch
                decode_attention_fused(o, q, k, v, kc, vc, position_ids, self.cos_sin,
                                       ap.new_cache_slots, ap.q_cu_seq_lens, ap.kv_cu_seq_lens,
                                       ap.block_tables, ap.cu_blocks_lens, ap.kv_max_seq_len, D ** -0.5,
                                       rank_desc=ap.decode_rank)
            else:
                # RoPE in place + append k/v to the paged cache, one launch; then attention
                rope_set_kv_cache(q, k, v, position_ids, self.cos_sin, D, ap.new_cache_slots, kc, vc)
                mha_varlen_fwd(o, q, kc, vc, ap.q_cu_seq_lens, ap.kv_cu_seq_lens, ap.block_tables,
                               ap.cu_blocks_lens, None, ap.q_max_seq_len, ap.kv_max_seq_len,
                               D ** -0.5, 0, -1, 0, 0)
            a = self.linear(o.view(n, q_size), st[f"l{l}.wo"], st.get(f"l{l}.wo_scale"))
            # h += a ; x = norm2(h)
            add_rms_norm(x, h, a, st[f"l{l}.norm2"], eps)
            if (not model_params.all_sequences_decode) and l == L - 1 \
                    and model_params.selected_token_ids is not None:
                # last layer of a prefill: only sampled tokens go through the MLP
                h = h[model_params.selected_token_ids].contiguous()
                x = x[model_params.selected_token_ids].contiguous()
            m = self._mlp(l, x)
            nxt = st[f"l{l + 1}.norm1"] if l + 1 < L else st["norm"]
            if x.shape != h.shape:
                x = torch.empty_like(h)
            add_rms_norm(x, h, m, nxt, eps)   # h += m ; x = next norm (final norm after last layer)
        return x

    def forward_logits(self, input_ids_or_embeds, position_ids, model_params) -> Tensor:
        x = self.forward_hidden(input_ids_or_embeds, position_ids, model_params)
        w = self.state["lm_head"]
        if launch_plan.current() is None:
            return torch.matmul(x, w.t())
        # a launch plan is being recorded: the library GEMM is a host-side step of the plan between two native
        # launch segments, writing into a buffer of the plan's pool
        logits = torch.empty((x.shape[0], w.shape[0]), dtype=x.dtype, device=x.device)
        launch_plan.host_op(lambda: torch.matmul(x, w.t(), out=logits))
        return logits

    def forward(self, input_ids_or_embeds, position_ids, model_params) -> Tensor:
        """Returns sampled token ids (greedy), like the reference model."""
        logits = self.forward_logits(input_ids_or_embeds, position_ids, model_params)
        if logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype in (torch.float16, torch.bfloat16):
            # one 4 us launch (the library reduction: 15 us); straight into the caller's next-input buffer if it set one
            out = self.sample_out if (self.sample_out is not None and self.sample_out.shape == (logits.shape[0],)) else None
            return argmax_rows(logits, out)
        return torch.argmax(logits, dim=-1)

    def forward_logprobs(self, input_ids_or_embeds, position_ids, model_params, top_k: int = 0, out=None):
        """forward() for a step whose requests asked for log-probabilities: the same logits, then ONE launch that gives
        the greedy ids (the same rule as forward's, so the tokens do not change), their log-softmax values and the top_k
        alternatives — (ids, logprobs, top_ids, top_logprobs) of _C.kernel.norm.logprob_rows, views of one buffer (`out`).
        Eager only: not part of the launch plan or the captured graphs."""
        logits = self.forward_logits(input_ids_or_embeds, position_ids, model_params)
        return logprob_rows(logits, top_k, out)

    def forward_penalized(self, input_ids_or_embeds, position_ids, model_params, hist_ids, hist_counts, cu_hist, penalties,
                          out=None):
        """forward() for a step with a request under frequency / presence / repetition penalties: the same logits, then
        ONE launch (sampling.penalized_argmax_rows) in place of argmax_rows — row r's (token, count) table is the CSR slice
        cu_hist[r] .. cu_hist[r + 1], a row with an empty table gets forward()'s id.  Eager only: not part of the launch
        plan or the captured graphs."""
        from hydrainfer_amd.sampling import penalized_argmax_rows
        logits = self.forward_logits(input_ids_or_embeds, position_ids, model_params)
        return penalized_argmax_rows(logits, hist_ids, hist_counts, cu_hist, penalties, out)

    def forward_sampled(self, input_ids_or_embeds, position_ids, model_params, sample_params, hist_ids=None, hist_counts=None,
                        cu_hist=None, penalties=None, out=None):
        """forward() for a step with a sampled request (temperature > 0): the same logits, then ONE launch
        (sampling.sample_rows) in place of argmax_rows — row r's record is sample_params[r], a row with temperature 0
        gets forward_penalized()'s id.  Eager only: not part of the launch plan or the captured graphs."""
        from hydrainfer_amd.sampling import sample_rows
        logits = self.forward_logits(input_ids_or_embeds, position_ids, model_params)
        return sample_rows(logits, sample_params, hist_ids, hist_counts, cu_hist, penalties, out)

    def forward_constrained(self, input_ids_or_embeds, position_ids, model_params, sample_params, bias_ids, bias_values,
                            cu_bias, hist_ids=None, hist_counts=None, cu_hist=None, penalties=None, out=None):
        """forward() for a step with a constrained request (logit_bias, min_tokens, min_p): the same logits, then ONE
        launch (sampling.sample_rows_constrained) — forward_sampled() with the rows' bias tables added ahead of the
        penalties and min_p in the records.  Eager only: not part of the launch plan or the captured graphs."""
        from hydrainfer_amd.sampling import sample_rows_constrained
        logits = self.forward_logits(input_ids_or_embeds, position_ids, model_params)
        return sample_rows_constrained(logits, sample_params, bias_ids, bias_values, cu_bias, hist_ids, hist_counts, cu_hist,
                                       penalties, out)

    def forward_scored(self, input_ids_or_embeds, position_ids, model_params, sample_params, bias_ids, bias_values,
                       cu_bias, hist_ids=None, hist_counts=None, cu_hist=None, penalties=None, *, top_k: int, want=None,
                       out=None):
        """forward_constrained() for a step with a request that asked for the scores of the PROCESSED distribution
        (logprobs_mode = "processed_logprobs"): the same logits, then ONE launch (sampling.sample_rows_logprobs) that
        gives forward_constrained()'s ids and, for the rows with want >= 0, the log-probability of each id under the
        distribution it was chosen from and the top_k alternatives — (ids, logprobs, top_ids, top_logprobs), views of
        one buffer (`out`) in logprob_rows' layout.  Eager only: not part of the launch plan or the captured graphs."""
        from hydrainfer_amd.sampling import sample_rows_logprobs
        logits = self.forward_logits(input_ids_or_embeds, position_ids, model_params)
        return sample_rows_logprobs(logits, sample_params, bias_ids, bias_values, cu_bias, hist_ids, hist_counts, cu_hist,
                                    penalties, top_k=top_k, want=want, out=out)

    __call__ = forward
