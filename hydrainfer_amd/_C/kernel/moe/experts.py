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


FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0          # the largest finite e4m3fn value
BLOCK = 128              # edge of a scale block


def _blocks(t: Tensor) -> Tensor:
    """[..., N, K] -> [..., N / 128, 128, K / 128, 128] view."""
    if t.dim() < 2 or t.shape[-2] % BLOCK or t.shape[-1] % BLOCK:
        raise _lib.HydraHipError("fp8 block scaling: [..., N, K] with N and K multiples of 128")
    return t.reshape(*t.shape[:-2], t.shape[-2] // BLOCK, BLOCK, t.shape[-1] // BLOCK, BLOCK)


def quantize_fp8_block(w: Tensor, scale: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(q float8_e4m3fn [..., N, K], scale f32 [..., N / 128, K / 128]) with w ~ float(q) * scale: the published
    `weight_scale_inv` format.  scale = amax(block) / 448 (1 for an all-zero block) unless given.  Load-time work in plain
    torch, any device."""
    wb = _blocks(w.float())
    if scale is None:
        amax = wb.abs().amax(dim=(-3, -1))
        scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    elif scale.shape != wb.shape[:-4] + (wb.shape[-4], wb.shape[-2]):
        raise _lib.HydraHipError("quantize_fp8_block: scale must be [..., N / 128, K / 128]")
    scale = scale.to(torch.float32)
    q = (wb / scale[..., :, None, :, None]).to(FP8).reshape(w.shape)
    return q.contiguous(), scale.contiguous()


def dequantize_fp8_block(q: Tensor, scale: Tensor) -> Tensor:
    """fp32 float(q) * scale of its block (exact: 4 x 24 significant bits)."""
    if q.dtype == torch.uint8:
        q = q.view(FP8)
    return (_blocks(q.float()) * scale.float()[..., :, None, :, None]).reshape(q.shape)


def _expert_weights(w_gate_up: Optional[Tensor], w_down: Optional[Tensor], dtype, scale: Optional[Tensor] = None
                    ) -> Tuple[int, int, int]:
    """(E, h, I) of the one weight given.  With a scale the weight is e4m3 bytes (float8_e4m3fn or uint8) and the scale
    fp32 [E, rows / 128, cols / 128] on its device; without one it is in the activations' dtype."""
    w, name, layout = (w_gate_up, "w_gate_up", "[E, 2I, h]") if w_gate_up is not None else (w_down, "w_down", "[E, h, I]")
    if scale is None:
        if w.dtype in (FP8, torch.uint8):
            raise _lib.HydraHipError(f"{name} holds fp8 bytes: it needs its block scales ({name}_scale)")
        kind, ok = "in the activations' dtype", w.dtype == dtype
    else:
        kind, ok = "of float8_e4m3fn (or uint8) bytes when a scale is given", w.dtype in (FP8, torch.uint8)
    if w.dim() != 3 or not w.is_contiguous() or not ok or (w_gate_up is not None and w.shape[1] % 2):
        raise _lib.HydraHipError(f"{name} must be contiguous {layout} {kind}")
    if scale is not None:
        if w.shape[1] % BLOCK or w.shape[2] % BLOCK:
            raise _lib.HydraHipError(f"{name}: fp8 block scaling needs rows and columns that are multiples of 128")
        want = (w.shape[0], w.shape[1] // BLOCK, w.shape[2] // BLOCK)
        if (scale.dtype != torch.float32 or tuple(scale.shape) != want or not scale.is_contiguous()
                or scale.device != w.device):
            raise _lib.HydraHipError(f"{name}_scale must be contiguous fp32 {list(want)} on the weight's device")
    if w_gate_up is not None:
        return w.shape[0], w.shape[2], w.shape[1] // 2
    return w.shape[0], w.shape[1], w.shape[2]


def gate_up_silu(x: Tensor, w_gate_up: Tensor, seg: Tensor, topk: int, out: Optional[Tensor] = None,
                 w_gate_up_scale: Optional[Tensor] = None) -> Tensor:
    """act [n * topk, I] in slot order: silu(x_t Wg_e^T) * (x_t Wu_e^T) for every routed slot (t, k), e = its expert.
    w_gate_up_scale given: w_gate_up is fp8 bytes with one scale per 128 x 128 block (hx_moe_gate_up_silu_fp8w)."""
    _lib.require_gpu(x, w_gate_up, seg, out, w_gate_up_scale)
    _rows(x, "x")
    E, h, inter = _expert_weights(w_gate_up, None, x.dtype, w_gate_up_scale)
    n = x.shape[0]
    if x.shape[1] != h or seg.dtype != torch.int32 or seg.numel() < 2 * E + 1 + n * topk:
        raise _lib.HydraHipError("gate_up_silu: x [n, h], seg from segments(topk_ids, E)")
    if out is None:
        out = torch.empty((n * topk, inter), dtype=x.dtype, device=x.device)
    elif out.shape != (n * topk, inter) or out.dtype != x.dtype or not out.is_contiguous():
        raise _lib.HydraHipError("gate_up_silu: out must be contiguous [n * topk, I]")
    if w_gate_up_scale is not None:
        _lib.check(_lib.lib().hx_moe_gate_up_silu_fp8w(out.data_ptr(), x.data_ptr(), w_gate_up.data_ptr(),
                                                       w_gate_up_scale.data_ptr(), seg.data_ptr(), n, int(topk), E, h, inter,
                                                       _lib.dtype_code(x), _lib.current_stream()), "moe gate_up_silu_fp8w")
        return out
    _lib.check(_lib.lib().hx_moe_gate_up_silu(out.data_ptr(), x.data_ptr(), w_gate_up.data_ptr(), seg.data_ptr(), n, int(topk),
                                              E, h, inter, _lib.dtype_code(x), _lib.current_stream()), "moe gate_up_silu")
    return out


def down(act: Tensor, w_down: Tensor, seg: Tensor, topk: int, out: Optional[Tensor] = None,
         w_down_scale: Optional[Tensor] = None) -> Tensor:
    """y [n * topk, h] in slot order: act_s Wd_e^T.  w_down_scale given: fp8 bytes and block scales (hx_moe_down_fp8w)."""
    _lib.require_gpu(act, w_down, seg, out, w_down_scale)
    _rows(act, "act")
    E, h, inter = _expert_weights(None, w_down, act.dtype, w_down_scale)
    slots = act.shape[0]
    if act.shape[1] != inter or slots % topk or seg.dtype != torch.int32 or seg.numel() < 2 * E + 1 + slots:
        raise _lib.HydraHipError("down: act [n * topk, I], seg from segments(topk_ids, E)")
    if out is None:
        out = torch.empty((slots, h), dtype=act.dtype, device=act.device)
    elif out.shape != (slots, h) or out.dtype != act.dtype or not out.is_contiguous():
        raise _lib.HydraHipError("down: out must be contiguous [n * topk, h]")
    if w_down_scale is not None:
        _lib.check(_lib.lib().hx_moe_down_fp8w(out.data_ptr(), act.data_ptr(), w_down.data_ptr(), w_down_scale.data_ptr(),
                                               seg.data_ptr(), slots // topk, int(topk), E, h, inter, _lib.dtype_code(act),
                                               _lib.current_stream()), "moe down_fp8w")
        return out
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
                    shared: Optional[Tensor] = None, w_gate_up_scale: Optional[Tensor] = None,
                    w_down_scale: Optional[Tensor] = None) -> Tensor:
    """moe_infer (deepseek_v3.py:124-155) + the shared experts' term (:120): segments, gate|up + silu*mul, down, combine.
    The scales select the fp8 block-scaled launches, each linear on its own."""
    topk = topk_ids.shape[1]
    seg = segments(topk_ids, w_gate_up.shape[0])
    act = gate_up_silu(x, w_gate_up, seg, topk, w_gate_up_scale=w_gate_up_scale)
    y = down(act, w_down, seg, topk, w_down_scale=w_down_scale)
    return combine(y, topk_weights, shared)
