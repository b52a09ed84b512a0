"""Sparse MoE feed-forward block — mirrors DeepseekV3MoE (hydrainfer/model/deepseek_v3.py:95-155): softmax / greedy
router, routed experts, shared experts.

MI355X-first differences (rounding-neutral with respect to the reference's ops, tests/moe_block_ref.py):
  * the routed experts' weights are STACKED ([E, 2I, h] gate rows then up rows, [E, h, I]) and run as two grouped
    weight-streaming launches (csrc/moe_experts.hip) instead of a Python loop of index-gather + three GEMMs per expert;
  * nothing is read back to the host (the reference's tokens_per_expert.cpu(), :130): the block captures into a hipGraph;
  * the shared experts' gate and up projections are one fused [2 I_s, h] GEMM;
  * the routed experts may be held as FP8 block-scaled bytes (float8_e4m3fn + one fp32 scale per 128 x 128 block, the
    published DeepSeek-V3 format: csrc/moe_experts_fp8.hip) — opt-in, by quantize_experts() or by handing over such a state
    dict — and so may the shared experts (quantize_shared(); csrc/gemm_skinny_fp8.hip through the dense ops); the router
    stays in T.
HIP only: the router, the segments, both expert GEMMs and the combine are libhydra_hip launches; there is no fallback."""
from typing import Callable, Dict, Optional

import torch
from torch import Tensor

from hydrainfer_amd._C.kernel.activation import silu_and_mul
from hydrainfer_amd._C.kernel.moe import experts as moe_experts


def _dense_linear(x: Tensor, w: Tensor, scale: Optional[Tensor] = None) -> Tensor:
    """x @ w^T on the dense ops of the decoder: the weight-streaming HIP GEMM at decode sizes, the library GEMM above.
    scale given: w is FP8 block-scaled bytes — the FP8 decode GEMM, or above 64 rows the library GEMM over T(q * s)
    (LlamaForCausalLM.linear, which keeps one scratch tensor for that copy; here it is a fresh one)."""
    from hydrainfer_amd._C.kernel import gemm as hip_gemm
    if scale is not None:
        if hip_gemm.fp8_supported(x, w, scale):
            return hip_gemm.linear_decode_fp8(x, w, scale)
        return torch.matmul(x, hip_gemm.dequant_fp8_block(w, scale, x.dtype).t())
    if x.shape[0] <= 64 and hip_gemm.supported(x, w):
        return hip_gemm.linear_decode(x, w)
    return torch.matmul(x, w.t())


class SparseMoE:
    def __init__(self, router_weight: Tensor, w_gate_up: Tensor, w_down: Tensor, shared_gate_up: Optional[Tensor],
                 shared_down: Optional[Tensor], num_experts_per_tok: int, norm_topk_prob: bool = False,
                 routed_scaling_factor: float = 1.0, linear: Optional[Callable[..., Tensor]] = None,
                 w_gate_up_scale: Optional[Tensor] = None, w_down_scale: Optional[Tensor] = None,
                 shared_gate_up_scale: Optional[Tensor] = None, shared_down_scale: Optional[Tensor] = None):
        """linear(x, w, scale=None): the dense x @ w^T; it is handed a scale only for FP8 shared experts."""
        E, two_i, h = w_gate_up.shape
        if w_down.shape != (E, h, two_i // 2) or router_weight.shape != (E, h):
            raise ValueError("SparseMoE: router_weight [E, h], w_gate_up [E, 2I, h], w_down [E, h, I]")
        if (w_gate_up_scale is None) != (w_down_scale is None):
            raise ValueError("SparseMoE: fp8 experts need the scales of both weights")
        if w_gate_up_scale is not None and (
                w_gate_up.dtype != moe_experts.FP8 or w_down.dtype != moe_experts.FP8
                or w_gate_up_scale.shape != (E, two_i // 128, h // 128) or w_down_scale.shape != (E, h // 128, two_i // 256)):
            raise ValueError("SparseMoE: fp8 experts are float8_e4m3fn with scales [E, 2I/128, h/128] and [E, h/128, I/128]")
        self.w_gate_up_scale, self.w_down_scale = w_gate_up_scale, w_down_scale
        if (shared_gate_up is None) != (shared_down is None):
            raise ValueError("SparseMoE: the shared experts need both weights")
        if (shared_gate_up_scale is None) != (shared_down_scale is None):
            raise ValueError("SparseMoE: fp8 shared experts need the scales of both weights")
        if shared_gate_up_scale is not None:
            if shared_gate_up is None:
                raise ValueError("SparseMoE: shared expert scales without shared experts")
            for w, sc, name in ((shared_gate_up, shared_gate_up_scale, "shared_gate_up"), (shared_down, shared_down_scale, "shared_down")):
                if (w.dtype != moe_experts.FP8 or w.dim() != 2 or sc.dtype != torch.float32
                        or tuple(sc.shape) != (w.shape[0] // 128, w.shape[1] // 128) or w.shape[0] % 128 or w.shape[1] % 128):
                    raise ValueError(f"SparseMoE: fp8 {name} is float8_e4m3fn [N, K] with an fp32 scale [N/128, K/128]")
            if shared_gate_up.shape[0] % 256:
                raise ValueError("SparseMoE: fp8 shared experts need an intermediate size that is a multiple of 128")
        elif shared_gate_up is not None and moe_experts.FP8 in (shared_gate_up.dtype, shared_down.dtype):
            raise ValueError("SparseMoE: float8_e4m3fn shared experts need their block scales (shared_gate_up_scale, shared_down_scale)")
        self.router_weight, self.w_gate_up, self.w_down = router_weight, w_gate_up, w_down
        self.shared_gate_up, self.shared_down = shared_gate_up, shared_down
        self.shared_gate_up_scale, self.shared_down_scale = shared_gate_up_scale, shared_down_scale
        self.num_experts_per_tok, self.norm_topk_prob = int(num_experts_per_tok), bool(norm_topk_prob)
        self.routed_scaling_factor = float(routed_scaling_factor)
        self.linear = linear or _dense_linear
        self.last_topk_ids: Optional[Tensor] = None      # [n, topk] int32 of the last forward (tests, statistics)

    @property
    def n_experts(self) -> int:
        return self.w_gate_up.shape[0]

    @property
    def experts_fp8(self) -> bool:
        return self.w_gate_up_scale is not None

    def quantize_experts(self) -> "SparseMoE":
        """The routed experts to FP8 block-scaled bytes, in place; the 16-bit tensors are dropped.  Idempotent."""
        if not self.experts_fp8:
            self.w_gate_up, self.w_gate_up_scale = moe_experts.quantize_fp8_block(self.w_gate_up)
            self.w_down, self.w_down_scale = moe_experts.quantize_fp8_block(self.w_down)
        return self

    @property
    def shared_fp8(self) -> bool:
        return self.shared_gate_up_scale is not None

    def quantize_shared(self) -> "SparseMoE":
        """The shared experts to FP8 block-scaled bytes, in place; the 16-bit tensors are dropped.  Idempotent."""
        if self.shared_gate_up is not None and not self.shared_fp8:
            if self.shared_gate_up.shape[0] % 256:
                raise ValueError("quantize_shared: the shared experts' intermediate size must be a multiple of 128")
            self.shared_gate_up, self.shared_gate_up_scale = moe_experts.quantize_fp8_block(self.shared_gate_up)
            self.shared_down, self.shared_down_scale = moe_experts.quantize_fp8_block(self.shared_down)
        return self

    def shared_experts(self, x: Tensor) -> Optional[Tensor]:
        """DeepseekV3MLP of intermediate size I * n_shared_experts (:110-112) on the dense ops."""
        if self.shared_gate_up is None:
            return None
        inter = self.shared_gate_up.shape[0] // 2
        if self.shared_fp8:
            gu = self.linear(x, self.shared_gate_up, self.shared_gate_up_scale)
            return self.linear(silu_and_mul(gu[:, :inter], gu[:, inter:]), self.shared_down, self.shared_down_scale)
        gu = self.linear(x, self.shared_gate_up)
        return self.linear(silu_and_mul(gu[:, :inter], gu[:, inter:]), self.shared_down)

    def forward(self, x: Tensor) -> Tensor:
        if x.dim() != 2:
            raise ValueError("SparseMoE.forward: x must be [n_tokens, hidden]")
        if not x.is_contiguous():
            x = x.contiguous()
        w, ids = moe_experts.gate_topk(x, self.router_weight, self.num_experts_per_tok, self.norm_topk_prob,
                                       self.routed_scaling_factor)
        self.last_topk_ids = ids
        shared = self.shared_experts(x)
        if shared is not None and not shared.is_contiguous():
            shared = shared.contiguous()
        return moe_experts.experts_forward(x, self.w_gate_up, self.w_down, w, ids, shared, self.w_gate_up_scale,
                                           self.w_down_scale)

    __call__ = forward

    @classmethod
    def from_reference_state_dict(cls, prefix: str, sd: Dict[str, Tensor], num_experts_per_tok: int,
                                  norm_topk_prob: bool = False, routed_scaling_factor: float = 1.0, dtype=None, device=None,
                                  linear=None) -> "SparseMoE":
        """prefix: up to and including "mlp." — reads {prefix}experts.{e}.{gate,up,down}_proj.weight, {prefix}gate.weight
        and {prefix}shared_experts.{gate,up,down}_proj.weight (absent: no shared experts).  Experts published as
        float8_e4m3fn come with {...}_proj.weight_scale_inv ([N / 128, K / 128] fp32): bytes and scales are stacked as they
        are (gate before up, the scales too), nothing is dequantised and `dtype` does not apply to them.  The same holds
        for shared experts published as float8_e4m3fn: a missing ...weight_scale_inv is a KeyError that names it, gate and
        up projections of different dtypes are refused."""
        def t(name, cast=True):
            v = sd[prefix + name]
            return v.to(dtype=(dtype if cast else None) or v.dtype, device=device or v.device)
        n_e = 0
        while f"{prefix}experts.{n_e}.gate_proj.weight" in sd:
            n_e += 1
        if n_e == 0:
            raise KeyError(f"no {prefix}experts.0.gate_proj.weight in the state dict")
        fp8 = {sd[f"{prefix}experts.{e}.{p}_proj.weight"].dtype == moe_experts.FP8
               for e in range(n_e) for p in ("gate", "up", "down")}
        if len(fp8) != 1:
            raise ValueError(f"{prefix}experts: float8_e4m3fn and 16-bit expert weights in one layer")
        fp8 = fp8.pop()
        gus = downs = None

        def stack(suffix):
            # float8 tensors are stacked through their bytes (torch.cat / stack of float8 is not everywhere available)
            def b(name):
                v = t(name, not fp8)
                return v.view(torch.uint8) if v.dtype == moe_experts.FP8 else v
            gu = torch.stack([torch.cat([b(f"experts.{e}.gate_proj.{suffix}"), b(f"experts.{e}.up_proj.{suffix}")], dim=0)
                              for e in range(n_e)]).contiguous()
            dn = torch.stack([b(f"experts.{e}.down_proj.{suffix}") for e in range(n_e)]).contiguous()
            return (gu.view(moe_experts.FP8), dn.view(moe_experts.FP8)) if gu.dtype == torch.uint8 else (gu, dn)
        wgu, wdown = stack("weight")
        if fp8:
            gus, downs = stack("weight_scale_inv")
        sgu = sdown = sgus = sdowns = None
        if prefix + "shared_experts.gate_proj.weight" in sd:
            s_fp8 = {p: sd[f"{prefix}shared_experts.{p}_proj.weight"].dtype == moe_experts.FP8 for p in ("gate", "up", "down")}
            if s_fp8["gate"] != s_fp8["up"]:
                raise ValueError(f"{prefix}shared_experts: gate_proj and up_proj differ in dtype (one is float8_e4m3fn)")
            if s_fp8["gate"] != s_fp8["down"]:
                raise ValueError(f"{prefix}shared_experts: float8_e4m3fn and 16-bit projections in one layer")
            if s_fp8["gate"]:
                def q(p):
                    name = f"{prefix}shared_experts.{p}_proj.weight_scale_inv"
                    if name not in sd:
                        raise KeyError(f"{name}: the float8_e4m3fn weight beside it needs its block scales")
                    return (t(f"shared_experts.{p}_proj.weight", False).view(torch.uint8),
                            sd[name].to(device=device or sd[name].device))
                (qg, sg), (qu, su), (qd, sdn) = q("gate"), q("up"), q("down")
                sgu = torch.cat([qg, qu], dim=0).contiguous().view(moe_experts.FP8)
                sdown = qd.contiguous().view(moe_experts.FP8)
                sgus, sdowns = torch.cat([sg, su], dim=0).contiguous(), sdn.contiguous()
            else:
                sgu = torch.cat([t("shared_experts.gate_proj.weight"), t("shared_experts.up_proj.weight")], dim=0).contiguous()
                sdown = t("shared_experts.down_proj.weight").contiguous()
        return cls(t("gate.weight").contiguous(), wgu, wdown, sgu, sdown, num_experts_per_tok, norm_topk_prob,
                   routed_scaling_factor, linear, gus, downs, sgus, sdowns)

    def to_reference_state_dict(self, prefix: str) -> Dict[str, Tensor]:
        inter = self.w_gate_up.shape[1] // 2
        sd = {prefix + "gate.weight": self.router_weight.cpu()}
        wgu, wdown = self.w_gate_up.cpu(), self.w_down.cpu()
        for e in range(self.n_experts):
            sd[f"{prefix}experts.{e}.gate_proj.weight"] = wgu[e, :inter]
            sd[f"{prefix}experts.{e}.up_proj.weight"] = wgu[e, inter:]
            sd[f"{prefix}experts.{e}.down_proj.weight"] = wdown[e]
        if self.experts_fp8:
            gus, downs = self.w_gate_up_scale.cpu(), self.w_down_scale.cpu()
            for e in range(self.n_experts):
                sd[f"{prefix}experts.{e}.gate_proj.weight_scale_inv"] = gus[e, :inter // 128]
                sd[f"{prefix}experts.{e}.up_proj.weight_scale_inv"] = gus[e, inter // 128:]
                sd[f"{prefix}experts.{e}.down_proj.weight_scale_inv"] = downs[e]
        if self.shared_gate_up is not None:
            si = self.shared_gate_up.shape[0] // 2
            sgu = self.shared_gate_up.cpu()
            sd[prefix + "shared_experts.gate_proj.weight"] = sgu[:si]
            sd[prefix + "shared_experts.up_proj.weight"] = sgu[si:]
            sd[prefix + "shared_experts.down_proj.weight"] = self.shared_down.cpu()
            if self.shared_fp8:
                sgus = self.shared_gate_up_scale.cpu()
                sd[prefix + "shared_experts.gate_proj.weight_scale_inv"] = sgus[:si // 128]
                sd[prefix + "shared_experts.up_proj.weight_scale_inv"] = sgus[si // 128:]
                sd[prefix + "shared_experts.down_proj.weight_scale_inv"] = self.shared_down_scale.cpu()
        return sd
