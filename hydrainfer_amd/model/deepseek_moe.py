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
    l{l}.moe.wdown_scale [E, h/128, I/128] (fp32) stand beside them."""

    def __init__(self, shape: MoeShape, dtype: torch.dtype, device, state: Dict[str, Tensor]):
        super().__init__(shape, dtype, device, state)
        self.moe: Dict[int, SparseMoE] = {}
        for l in range(shape.first_k_dense_replace, shape.num_hidden_layers):
            s = lambda n: state.get(f"l{l}.moe.{n}")
            self.moe[l] = SparseMoE(s("router"), s("wgu"), s("wdown"), s("sgu"), s("sdown"), shape.num_experts_per_tok,
                                    shape.norm_topk_prob, shape.routed_scaling_factor, linear=self.linear,
                                    w_gate_up_scale=s("wgu_scale"), w_down_scale=s("wdown_scale"))

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

    # ------------------------------------------------------------------ construction
    @classmethod
    def random_init(cls, shape: MoeShape, dtype: torch.dtype, device, seed: int = 0, std: float = 0.02,
                    router_std: float = 0.2, expert_std: float = None, expert_dtype: str = None) -> "DeepseekMoeForCausalLM":
        """N(0, std) linears and embeddings, N(0, router_std) routers, N(0, expert_std or std) routed and shared experts.
        expert_dtype="fp8": the same draw, then quantize_experts()."""
        if expert_dtype not in (None, "fp8"):
            raise ValueError(f"random_init: expert_dtype {expert_dtype!r} (None or 'fp8')")
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
        return model.quantize_experts() if expert_dtype == "fp8" else model

    @classmethod
    def from_reference_state_dict(cls, shape: MoeShape, sd: Dict[str, Tensor], dtype, device,
                                  prefix: str = "") -> "DeepseekMoeForCausalLM":
        """Names of hydrainfer/model/deepseek_v3.py: model.layers.N.mlp.experts.E.gate_proj.weight, ...mlp.gate.weight,
        ...mlp.shared_experts.*; dense layers and attention as in the parent.  Experts published as float8_e4m3fn with
        ...weight_scale_inv are taken as they are: neither the bytes nor the scales are cast to `dtype`."""
        def t(name):
            return sd[prefix + name].to(dtype).to(device)
        st = {"embed": t("model.embed_tokens.weight"), "lm_head": t("lm_head.weight"), "norm": t("model.norm.weight")}
        for l in range(shape.num_hidden_layers):
            p = f"model.layers.{l}."
            st[f"l{l}.wqkv"] = torch.cat([t(p + "self_attn.q_proj.weight"), t(p + "self_attn.k_proj.weight"),
                                          t(p + "self_attn.v_proj.weight")], dim=0).contiguous()
            st[f"l{l}.wo"] = t(p + "self_attn.o_proj.weight")
            if l < shape.first_k_dense_replace:
                st[f"l{l}.wgu"] = torch.cat([t(p + "mlp.gate_proj.weight"), t(p + "mlp.up_proj.weight")], dim=0).contiguous()
                st[f"l{l}.wdown"] = t(p + "mlp.down_proj.weight")
            else:
                m = SparseMoE.from_reference_state_dict(prefix + p + "mlp.", sd, shape.num_experts_per_tok, dtype=dtype,
                                                        device=device)
                st[f"l{l}.moe.router"], st[f"l{l}.moe.wgu"], st[f"l{l}.moe.wdown"] = m.router_weight, m.w_gate_up, m.w_down
                if m.experts_fp8:
                    st[f"l{l}.moe.wgu_scale"], st[f"l{l}.moe.wdown_scale"] = m.w_gate_up_scale, m.w_down_scale
                if m.shared_gate_up is not None:
                    st[f"l{l}.moe.sgu"], st[f"l{l}.moe.sdown"] = m.shared_gate_up, m.shared_down
            st[f"l{l}.norm1"] = t(p + "input_layernorm.weight")
            st[f"l{l}.norm2"] = t(p + "post_attention_layernorm.weight")
        return cls(shape, dtype, device, st)

    def to_reference_state_dict(self) -> Dict[str, Tensor]:
        s, q, kv, i = self.state, self.q_size, self.kv_size, self.shape.intermediate_size
        sd = {"model.embed_tokens.weight": s["embed"].cpu(), "lm_head.weight": s["lm_head"].cpu(),
              "model.norm.weight": s["norm"].cpu()}
        for l in range(self.shape.num_hidden_layers):
            p = f"model.layers.{l}."
            wqkv = s[f"l{l}.wqkv"].cpu()
            sd[p + "self_attn.q_proj.weight"] = wqkv[:q]
            sd[p + "self_attn.k_proj.weight"] = wqkv[q:q + kv]
            sd[p + "self_attn.v_proj.weight"] = wqkv[q + kv:]
            sd[p + "self_attn.o_proj.weight"] = s[f"l{l}.wo"].cpu()
            if l in self.moe:
                sd.update(self.moe[l].to_reference_state_dict(p + "mlp."))
            else:
                wgu = s[f"l{l}.wgu"].cpu()
                sd[p + "mlp.gate_proj.weight"] = wgu[:i]
                sd[p + "mlp.up_proj.weight"] = wgu[i:]
                sd[p + "mlp.down_proj.weight"] = s[f"l{l}.wdown"].cpu()
            sd[p + "input_layernorm.weight"] = s[f"l{l}.norm1"].cpu()
            sd[p + "post_attention_layernorm.weight"] = s[f"l{l}.norm2"].cpu()
        return sd

    # ------------------------------------------------------------------ byte models
    def weight_bytes(self, n_tokens: int = 1) -> int:
        """Bytes a decode step of n_tokens rows must stream at most: every dense linear, router and shared expert, the
        lm_head, and per sparse layer min(E, n_tokens * topk) routed experts (the distinct experts a step can hit) — at
        one byte per element plus 4 bytes per 128 x 128 block where the layer's experts are FP8 block-scaled."""
        sh, es = self.shape, self.state["lm_head"].element_size()
        total = es * sum(v.numel() for k, v in self.state.items() if k != "embed" and v.dim() == 2)
        hit = min(sh.n_routed_experts, n_tokens * sh.num_experts_per_tok)
        per_expert = 3 * sh.hidden_size * sh.moe_intermediate_size
        for m in self.moe.values():
            total += hit * (per_expert + 4 * per_expert // (128 * 128) if m.experts_fp8 else per_expert * es)
        return total

    def weight_bytes_resident(self) -> int:
        """Bytes of HBM the weights occupy: one layout of everything, all experts included."""
        return sum(t.numel() * t.element_size() for t in self.state.values() if t.device.type != "meta")
