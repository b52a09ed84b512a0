"""DeepSeek-MoE-shaped decoder: the language model of DeepSeek-VL2 (hydrainfer/model/deepseek_v3.py:158-246) — the Llama
decoder of model/llama.py whose MLP is, from layer `first_k_dense_replace` on, a sparse MoE block (:191).

Attention is the parent's: the reference's DeepseekV3Attention (:158-182) is plain RoPE MHA / GQA.  The MoE layers run on
layer/moe.py (csrc/moe_experts.hip); the step has no host synchronisation, so the model runs unchanged under
LlavaLanguageModel in the eager executor, the hipGraph decoder and the cohort.  The in-register decode plan of the dense
model (model/decode_plan.py) is switched off: its launch sequences hard-wire the dense MLP."""
from dataclasses import dataclass
from typing import Dict

import torch
from torch import Tensor

from hydrainfer_amd._C.kernel.moe.experts import FP8, quantize_fp8_block
from hydrainfer_amd.layer.moe import SparseMoE
from hydrainfer_amd.model.llama import LanguageModelParameters, LlamaForCausalLM, LlamaShape


@dataclass
class MoeShape(LlamaShape):
    n_routed_experts: int = 64
    num_experts_per_tok: int = 6
    moe_intermediate_size: int = 1408
    n_shared_experts: int = 2
    first_k_dense_replace: int = 1
    norm_topk_prob: bool = False
    routed_scaling_factor: float = 1.0


class DeepseekMoeForCausalLM(LlamaForCausalLM):
    """state: the parent's names for attention, norms, embeddings and the dense layers; for a sparse layer l
    l{l}.moe.router [E, h], l{l}.moe.wgu [E, 2I, h], l{l}.moe.wdown [E, h, I], l{l}.moe.sgu [2 I_s, h], l{l}.moe.sdown.
    FP8 block-scaled routed experts (layer/moe.py): wgu / wdown are float8_e4m3fn and l{l}.moe.wgu_scale [E, 2I/128, h/128],
    l{l}.moe.wdown_scale [E, h/128, I/128] (fp32) stand beside them.
    FP8 block-scaled dense linears (the published DeepSeek-V3 format of every other linear; csrc/gemm_skinny_fp8.hip): any
    of l{l}.wqkv / wo / wgu / wdown and l{l}.moe.sgu / sdown may be float8_e4m3fn [N, K] with an fp32 [N/128, K/128] scale
    under the same name + "_scale" (wqkv_scale: the q, k and v scales concatenated, so q_size and kv_size must be
    multiples of 128; wgu_scale: gate then up).  Embeddings, lm_head, norms and the router stay T.  Steps of <= 64 rows
    never round a scaled weight; larger batches (prefill) multiply by T(q * s) (LlamaForCausalLM.linear)."""

    fp8_dense = True
    DENSE_KEYS = ("wqkv", "wo", "wgu", "wdown")

    def __init__(self, shape: MoeShape, dtype: torch.dtype, device, state: Dict[str, Tensor]):
        super().__init__(shape, dtype, device, state)
        for l in range(shape.num_hidden_layers):
            for n in self.DENSE_KEYS:
                self._check_fp8(f"l{l}.{n}")
        self.moe: Dict[int, SparseMoE] = {}
        for l in range(shape.first_k_dense_replace, shape.num_hidden_layers):
            s = lambda n: state.get(f"l{l}.moe.{n}")
            self.moe[l] = SparseMoE(s("router"), s("wgu"), s("wdown"), s("sgu"), s("sdown"), shape.num_experts_per_tok,
                                    shape.norm_topk_prob, shape.routed_scaling_factor, linear=self.linear,
                                    w_gate_up_scale=s("wgu_scale"), w_down_scale=s("wdown_scale"),
                                    shared_gate_up_scale=s("sgu_scale"), shared_down_scale=s("sdown_scale"))

    def _check_fp8(self, key: str) -> None:
        """A dense weight of the state and its scale: both or neither, of the format's dtypes and shapes."""
        w, sc = self.state.get(key), self.state.get(key + "_scale")
        if w is None or (sc is None and w.dtype != FP8):
            if sc is not None:
                raise ValueError(f"{key}_scale without {key}")
            return
        if sc is None:
            raise KeyError(f"{key}_scale: {key} is float8_e4m3fn and needs its block scales")
        if (w.dtype != FP8 or w.dim() != 2 or w.shape[0] % 128 or w.shape[1] % 128 or sc.dtype != torch.float32
                or tuple(sc.shape) != (w.shape[0] // 128, w.shape[1] // 128)):
            raise ValueError(f"{key}: an FP8 dense weight is float8_e4m3fn [N, K], N and K multiples of 128, with "
                             f"{key}_scale fp32 [N/128, K/128]")
        if key.endswith("wqkv") and (self.q_size % 128 or self.kv_size % 128):
            raise ValueError(f"{key}_scale: q_size {self.q_size} and kv_size {self.kv_size} must be multiples of 128 (the q, k "
                             "and v scales are concatenated by rows)")
        if key.endswith("wgu") and self.shape.intermediate_size % 128:
            raise ValueError(f"{key}_scale: intermediate_size {self.shape.intermediate_size} must be a multiple of 128")

    # ------------------------------------------------------------------ the MLP hook and the decode plan
    def _mlp(self, l: int, x: Tensor) -> Tensor:
        return self.moe[l](x) if l in self.moe else super()._mlp(l, x)

    def _decode_fast_path(self, n: int, dtype, model_params: LanguageModelParameters) -> bool:
        return False

    def prepare_decode(self, max_rows: int = 64, keep_row_major: bool = True) -> None:
        """Nothing to build: the step runs on the row-major weights (dense layers: csrc/gemm_skinny.hip; experts:
        csrc/moe_experts.hip, which streams the stacked tensors as they are).  keep_row_major=False is accepted and
        ignored — there is no second layout that could stay in their place."""
        self.decode_rows_prepared = max(self.decode_rows_prepared, min(int(max_rows), 64))

    def pack_decode_weights(self, all_lds_slice: bool = False) -> None:
        return None

    def release(self) -> None:
        super().release()
        self.moe = {}

    def quantize_experts(self) -> "DeepseekMoeForCausalLM":
        """The routed experts of every sparse layer to FP8 block-scaled bytes (SparseMoE.quantize_experts); the state
        holds the bytes and the scales afterwards, the 16-bit tensors are dropped.  Idempotent."""
        for l, m in self.moe.items():
            m.quantize_experts()
            self.state[f"l{l}.moe.wgu"], self.state[f"l{l}.moe.wdown"] = m.w_gate_up, m.w_down
            self.state[f"l{l}.moe.wgu_scale"], self.state[f"l{l}.moe.wdown_scale"] = m.w_gate_up_scale, m.w_down_scale
        return self

    def quantize_dense(self) -> "DeepseekMoeForCausalLM":
        """The dense linears (attention projections, the dense layers' MLP) and the shared experts to FP8 block-scaled
        bytes; the state holds the bytes and the scales afterwards, the 16-bit tensors are dropped.  The routed experts
        are quantize_experts()'s.  Embeddings, lm_head, norms and routers stay T.  Idempotent."""
        if self.q_size % 128 or self.kv_size % 128:
            raise ValueError(f"quantize_dense: q_size {self.q_size} and kv_size {self.kv_size} must be multiples of 128")
        for l in range(self.shape.num_hidden_layers):
            for n in self.DENSE_KEYS:
                key = f"l{l}.{n}"
                if key in self.state and key + "_scale" not in self.state:
                    self.state[key], self.state[key + "_scale"] = quantize_fp8_block(self.state[key])
                    self._check_fp8(key)
            m = self.moe.get(l)
            if m is not None and m.shared_gate_up is not None:
                m.quantize_shared()
                self.state[f"l{l}.moe.sgu"], self.state[f"l{l}.moe.sdown"] = m.shared_gate_up, m.shared_down
                self.state[f"l{l}.moe.sgu_scale"], self.state[f"l{l}.moe.sdown_scale"] = m.shared_gate_up_scale, m.shared_down_scale
        return self

    # ------------------------------------------------------------------ construction
    @classmethod
    def random_init(cls, shape: MoeShape, dtype: torch.dtype, device, seed: int = 0, std: float = 0.02,
                    router_std: float = 0.2, expert_std: float = None, expert_dtype: str = None,
                    dense_dtype: str = None) -> "DeepseekMoeForCausalLM":
        """N(0, std) linears and embeddings, N(0, router_std) routers, N(0, expert_std or std) routed and shared experts.
        expert_dtype="fp8": the same draw, then quantize_experts(); dense_dtype="fp8": then quantize_dense()."""
        if expert_dtype not in (None, "fp8"):
            raise ValueError(f"random_init: expert_dtype {expert_dtype!r} (None or 'fp8')")
        if dense_dtype not in (None, "fp8"):
            raise ValueError(f"random_init: dense_dtype {dense_dtype!r} (None or 'fp8')")
        g = torch.Generator(device=device).manual_seed(seed)
        h, L = shape.hidden_size, shape.num_hidden_layers
        q, kv = shape.num_attention_heads * shape.head_dim, shape.num_key_value_heads * shape.head_dim
        E, I, Is = shape.n_routed_experts, shape.moe_intermediate_size, shape.moe_intermediate_size * shape.n_shared_experts

        def w(*size, s=std):
            return (torch.randn(size, generator=g, device=device, dtype=torch.float32) * s).to(dtype)

        st: Dict[str, Tensor] = {"embed": w(shape.vocab_size, h), "lm_head": w(shape.vocab_size, h),
                                 "norm": torch.ones(h, dtype=dtype, device=device)}
        for l in range(L):
            st[f"l{l}.wqkv"] = w(q + 2 * kv, h)
            st[f"l{l}.wo"] = w(h, q)
            if l < shape.first_k_dense_replace:
                st[f"l{l}.wgu"] = w(2 * shape.intermediate_size, h)
                st[f"l{l}.wdown"] = w(h, shape.intermediate_size)
            else:
                st[f"l{l}.moe.router"] = w(E, h, s=router_std)
                es = std if expert_std is None else expert_std
                st[f"l{l}.moe.wgu"] = w(E, 2 * I, h, s=es)
                st[f"l{l}.moe.wdown"] = w(E, h, I, s=es)
                if Is:
                    st[f"l{l}.moe.sgu"] = w(2 * Is, h, s=es)
                    st[f"l{l}.moe.sdown"] = w(h, Is, s=es)
            st[f"l{l}.norm1"] = torch.ones(h, dtype=dtype, device=device)
            st[f"l{l}.norm2"] = torch.ones(h, dtype=dtype, device=device)
        model = cls(shape, dtype, device, st)
        if expert_dtype == "fp8":
            model.quantize_experts()
        return model.quantize_dense() if dense_dtype == "fp8" else model

    @classmethod
    def from_reference_state_dict(cls, shape: MoeShape, sd: Dict[str, Tensor], dtype, device,
                                  prefix: str = "") -> "DeepseekMoeForCausalLM":
        """Names of hydrainfer/model/deepseek_v3.py: model.layers.N.mlp.experts.E.gate_proj.weight, ...mlp.gate.weight,
        ...mlp.shared_experts.*; dense layers and attention as in the parent.  Experts published as float8_e4m3fn with
        ...weight_scale_inv are taken as they are: neither the bytes nor the scales are cast to `dtype`.  The same holds
        for the attention projections, the dense layers' MLP and the shared experts (the published DeepSeek-V3 format of
        every linear but lm_head and the router): a float8_e4m3fn weight without its ...weight_scale_inv is a KeyError that
        names the scale — never a cast of the raw e4m3 values — and projections that are fused here (q / k / v, gate / up)
        must agree in dtype."""
        def t(name):
            v = sd[prefix + name]
            if v.dtype == FP8:
                raise ValueError(f"{prefix + name} is float8_e4m3fn: only the linears of the decoder layers may be")
            return v.to(dtype).to(device)

        def fused(key, names):
            """st[key] (and st[key + "_scale"]) from the projections `names`, concatenated by rows."""
            ws = [sd[prefix + n] for n in names]
            kinds = {w.dtype == FP8 for w in ws}
            if len(kinds) != 1:
                raise ValueError(f"{', '.join(prefix + n for n in names)}: float8_e4m3fn and 16-bit projections cannot be fused")
            if not kinds.pop():
                st[key] = torch.cat([w.to(dtype).to(device) for w in ws], dim=0).contiguous()
                return
            scales = []
            for n in names:
                sn = prefix + n[:-len("weight")] + "weight_scale_inv"
                if sn not in sd:
                    raise KeyError(f"{sn}: {prefix + n} is float8_e4m3fn and needs its block scales")
                scales.append(sd[sn].to(device))
            # float8 tensors are concatenated through their bytes
            st[key] = torch.cat([w.to(device).view(torch.uint8) for w in ws], dim=0).contiguous().view(FP8)
            st[key + "_scale"] = torch.cat(scales, dim=0).contiguous()

        st = {"embed": t("model.embed_tokens.weight"), "lm_head": t("lm_head.weight"), "norm": t("model.norm.weight")}
        for l in range(shape.num_hidden_layers):
            p = f"model.layers.{l}."
            fused(f"l{l}.wqkv", [p + f"self_attn.{n}_proj.weight" for n in "qkv"])
            fused(f"l{l}.wo", [p + "self_attn.o_proj.weight"])
            if l < shape.first_k_dense_replace:
                fused(f"l{l}.wgu", [p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"])
                fused(f"l{l}.wdown", [p + "mlp.down_proj.weight"])
            else:
                m = SparseMoE.from_reference_state_dict(prefix + p + "mlp.", sd, shape.num_experts_per_tok, dtype=dtype,
                                                        device=device)
                st[f"l{l}.moe.router"], st[f"l{l}.moe.wgu"], st[f"l{l}.moe.wdown"] = m.router_weight, m.w_gate_up, m.w_down
                if m.experts_fp8:
                    st[f"l{l}.moe.wgu_scale"], st[f"l{l}.moe.wdown_scale"] = m.w_gate_up_scale, m.w_down_scale
                if m.shared_gate_up is not None:
                    st[f"l{l}.moe.sgu"], st[f"l{l}.moe.sdown"] = m.shared_gate_up, m.shared_down
                if m.shared_fp8:
                    st[f"l{l}.moe.sgu_scale"], st[f"l{l}.moe.sdown_scale"] = m.shared_gate_up_scale, m.shared_down_scale
            st[f"l{l}.norm1"] = t(p + "input_layernorm.weight")
            st[f"l{l}.norm2"] = t(p + "post_attention_layernorm.weight")
        return cls(shape, dtype, device, st)

    def to_reference_state_dict(self) -> Dict[str, Tensor]:
        s, q, kv, i = self.state, self.q_size, self.kv_size, self.shape.intermediate_size
        sd = {"model.embed_tokens.weight": s["embed"].cpu(), "lm_head.weight": s["lm_head"].cpu(),
              "model.norm.weight": s["norm"].cpu()}
        for l in range(self.shape.num_hidden_layers):
            p = f"model.layers.{l}."
            def split(key, names, rows):
                """The row ranges of state[key] under `names`; FP8: the scales' row ranges beside them, bit for bit."""
                w, sc, at = s[key].cpu(), s.get(key + "_scale"), 0
                for n, r in zip(names, rows):
                    sd[p + n + ".weight"] = w[at:at + r]
                    if sc is not None:
                        sd[p + n + ".weight_scale_inv"] = sc.cpu()[at // 128:(at + r) // 128]
                    at += r
            split(f"l{l}.wqkv", [f"self_attn.{n}_proj" for n in "qkv"], [q, kv, kv])
            split(f"l{l}.wo", ["self_attn.o_proj"], [s[f"l{l}.wo"].shape[0]])
            if l in self.moe:
                sd.update(self.moe[l].to_reference_state_dict(p + "mlp."))
            else:
                split(f"l{l}.wgu", ["mlp.gate_proj", "mlp.up_proj"], [i, i])
                split(f"l{l}.wdown", ["mlp.down_proj"], [s[f"l{l}.wdown"].shape[0]])
            sd[p + "input_layernorm.weight"] = s[f"l{l}.norm1"].cpu()
            sd[p + "post_attention_layernorm.weight"] = s[f"l{l}.norm2"].cpu()
        return sd

    # ------------------------------------------------------------------ byte models
    def weight_bytes(self, n_tokens: int = 1) -> int:
        """Bytes a decode step of n_tokens rows must stream at most: every dense linear, router and shared expert, the
        lm_head, and per sparse layer min(E, n_tokens * topk) routed experts (the distinct experts a step can hit) — at
        one byte per element plus 4 bytes per 128 x 128 block where the layer's experts are FP8 block-scaled, and the same
        for every dense linear or shared expert that is."""
        sh, es = self.shape, self.state["lm_head"].element_size()
        total = sum(v.numel() * (4 if k.endswith("_scale") else 1 if v.dtype == FP8 else es)
                    for k, v in self.state.items() if k != "embed" and v.dim() == 2)
        hit = min(sh.n_routed_experts, n_tokens * sh.num_experts_per_tok)
        per_expert = 3 * sh.hidden_size * sh.moe_intermediate_size
        for m in self.moe.values():
            total += hit * (per_expert + 4 * per_expert // (128 * 128) if m.experts_fp8 else per_expert * es)
        return total

    def weight_bytes_resident(self) -> int:
        """Bytes of HBM the weights occupy: one layout of everything, all experts included."""
        return sum(t.numel() * t.element_size() for t in self.state.values() if t.device.type != "meta")
