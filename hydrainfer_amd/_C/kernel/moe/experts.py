"""The expert feed-forward half of a sparse MoE layer (csrc/moe_experts.hip): router, segments, the two grouped expert
GEMMs and the combine.  No counterpart in hydrainfer._C: the reference runs this as a Python loop over the experts around
a host synchronisation (hydrainfer/model/deepseek_v3.py:61-93, :124-155).  No call here synchronises or reads back."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from hydrainfer_amd import _lib

SCORE_SOFTMAX, SCORE_SIGMOID = 0, 1
_SCORING = {"softmax": SCORE_SOFTMAX, "sigmoid": SCORE_SIGMOID}


def _rows(t: Tensor, name: str, dtype=None) -> Tensor:
    if t.dim() != 2 or not t.is_contiguous():
        raise _lib.HydraHipError(f"{name} must be a contiguous 2-d tensor")
    if dtype is not None and t.dtype != dtype:
        raise _lib.HydraHipError(f"{name} must be {dtype}")
    return t


def gate_topk(x: Tensor, router_weight: Tensor, topk: int, norm_topk_prob: bool, routed_scaling_factor: float = 1.0,
              scoring_func: str = "softmax", n_group: int = 1, topk_group: int = 1) -> Tuple[Tensor, Tensor]:
    """MoEGate.forward (deepseek_v3.py:61-93), softmax + greedy: (topk_weights f32, topk_ids i32), both [n, topk]."""
    _lib.require_gpu(x, router_weight)
    _rows(x, "x"); _rows(router_weight, "router_weight")
    if scoring_func not in _SCORING:
        raise _lib.HydraHipError(f"gate_topk: unknown scoring function {scoring_func!r}")
    n, h = x.shape
    E = router_weight.shape[0]
    if router_weight.shape[1] != h:
        raise _lib.HydraHipError("gate_topk: router_weight must be [n_experts, hidden]")
    w = torch.empty((n, topk), dtype=torch.float32, device=x.device)
    ids = torch.empty((n, topk), dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().hx_moe_gate_topk(w.data_ptr(), ids.data_ptr(), x.data_ptr(), router_weight.data_ptr(), n, h, E,
                                           int(topk), _lib.dtype_code(x), _lib.dtype_code(router_weight),
                                           _SCORING[scoring_func], int(n_group), int(topk_group), int(bool(norm_topk_prob)),
                                           float(routed_scaling_factor), _lib.current_stream()), "moe gate_topk")
    return w, ids


def segments(topk_ids: Tensor, n_experts: int, out: Optional[Tensor] = None) -> Tensor:
    """int32 [offsets E + 1 | counts E | slots n * topk]: the slots s = t * topk + k grouped by expert."""
    _lib.require_gpu(topk_ids, out)
    _rows(topk_ids, "topk_ids", torch.int32)
    n, topk = topk_ids.shape
    elems = _lib.lib().hx_moe_segments_elems(n, topk, int(n_experts))
    if out is None:
        out = torch.empty(elems, dtype=torch.int32, device=topk_ids.device)
    elif out.dtype != torch.int32 or out.numel() < elems or not out.is_contiguous():
        raise _lib.HydraHipError(f"segments: out must be contiguous int32 with >= {elems} elements")
    _lib.check(_lib.lib().hx_moe_segments(out.data_ptr(), topk_ids.data_ptr(), n, topk, int(n_experts),
                                          _lib.current_stream()), "moe segments")
    return out


def _expert_weights(w_gate_up: Optional[Tensor], w_down: Optional[Tensor], dtype) -> Tuple[int, int, int]:
    E = h = inter = 0
    if w_gate_up is not None:
        if w_gate_up.dim() != 3 or not w_gate_up.is_contiguous() or w_gate_up.dtype != dtype or w_gate_up.shape[1] % 2:
            raise _lib.HydraHipError("w_gate_up must be contiguous [E, 2I, h] in the activations' dtype")
        E, inter, h = w_gate_up.shape[0], w_gate_up.shape[1] // 2, w_gate_up.shape[2]
    if w_down is not None:
        if w_down.dim() != 3 or not w_down.is_contiguous() or w_down.dtype != dtype:
            raise _lib.HydraHipError("w_down must be contiguous [E, h, I] in the activations' dtype")
        E, h, inter = w_down.shape
    return E, h, inter


def gate_up_silu(x: Tensor, w_gate_up: Tensor, seg: Tensor, topk: int, out: Optional[Tensor] = None) -> Tensor:
    """act [n * topk, I] in slot order: silu(x_t Wg_e^T) * (x_t Wu_e^T) for every routed slot (t, k), e = its expert."""
    _lib.require_gpu(x, w_gate_up, seg, out)
    _rows(x, "x")
    E, h, inter = _expert_weights(w_gate_up, None, x.dtype)
    n = x.shape[0]
    if x.shape[1] != h or seg.dtype != torch.int32 or seg.numel() < 2 * E + 1 + n * topk:
        raise _lib.HydraHipError("gate_up_silu: x [n, h], seg from segments(topk_ids, E)")
    if out is None:
        out = torch.empty((n * topk, inter), dtype=x.dtype, device=x.device)
    elif out.shape != (n * topk, inter) or out.dtype != x.dtype or not out.is_contiguous():
        raise _lib.HydraHipError("gate_up_silu: out must be contiguous [n * topk, I]")
    _lib.check(_lib.lib().hx_moe_gate_up_silu(out.data_ptr(), x.data_ptr(), w_gate_up.data_ptr(), seg.data_ptr(), n, int(topk),
                                              E, h, inter, _lib.dtype_code(x), _lib.current_stream()), "moe gate_up_silu")
    return out


def down(act: Tensor, w_down: Tensor, seg: Tensor, topk: int, out: Optional[Tensor] = None) -> Tensor:
    """y [n * topk, h] in slot order: act_s Wd_e^T."""
    _lib.require_gpu(act, w_down, seg, out)
    _rows(act, "act")
    E, h, inter = _expert_weights(None, w_down, act.dtype)
    slots = act.shape[0]
    if act.shape[1] != inter or slots % topk or seg.dtype != torch.int32 or seg.numel() < 2 * E + 1 + slots:
        raise _lib.HydraHipError("down: act [n * topk, I], seg from segments(topk_ids, E)")
    if out is None:
        out = torch.empty((slots, h), dtype=act.dtype, device=act.device)
    elif out.shape != (slots, h) or out.dtype != act.dtype or not out.is_contiguous():
        raise _lib.HydraHipError("down: out must be contiguous [n * topk, h]")
    _lib.check(_lib.lib().hx_moe_down(out.data_ptr(), act.data_ptr(), w_down.data_ptr(), seg.data_ptr(), slots // topk, int(topk),
                                      E, h, inter, _lib.dtype_code(act), _lib.current_stream()), "moe down")
    return out


def combine(y: Tensor, topk_weights: Tensor, shared: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """out[t] = T(T(sum_k w[t, k] * y[t * topk + k]) + shared[t]) (fp32 products and sum, k order); shared may be None."""
    _lib.require_gpu(y, topk_weights, shared, out)
    _rows(y, "y"); _rows(topk_weights, "topk_weights", torch.float32)
    n, topk = topk_weights.shape
    h = y.shape[1]
    if y.shape[0] != n * topk:
        raise _lib.HydraHipError("combine: y must be [n * topk, h]")
    if shared is not None and (shared.shape != (n, h) or shared.dtype != y.dtype or not shared.is_contiguous()):
        raise _lib.HydraHipError("combine: shared must be contiguous [n, h] in y's dtype")
    if out is None:
        out = torch.empty((n, h), dtype=y.dtype, device=y.device)
    elif out.shape != (n, h) or out.dtype != y.dtype or not out.is_contiguous():
        raise _lib.HydraHipError("combine: out must be contiguous [n, h]")
    _lib.check(_lib.lib().hx_moe_combine(out.data_ptr(), y.data_ptr(), topk_weights.data_ptr(),
                                         shared.data_ptr() if shared is not None else None, n, topk, h, _lib.dtype_code(y),
                                         _lib.current_stream()), "moe combine")
    return out


def experts_forward(x: Tensor, w_gate_up: Tensor, w_down: Tensor, topk_weights: Tensor, topk_ids: Tensor,
                    shared: Optional[Tensor] = None) -> Tensor:
    """moe_infer (deepseek_v3.py:124-155) + the shared experts' term (:120): segments, gate|up + silu*mul, down, combine."""
    topk = topk_ids.shape[1]
    seg = segments(topk_ids, w_gate_up.shape[0])
    act = gate_up_silu(x, w_gate_up, seg, topk)
    y = down(act, w_down, seg, topk)
    return combine(y, topk_weights, shared)
