"""What a decode step of <= 64 rows launches, decided once, on the host.  `plan_layouts` is the one statement of which
packed weight layouts exist; `resolve` names the variant of every stage of a layer for one step.  Both are pure in their
arguments and the host support queries of _C.kernel.gemm (no tensor, no device).  `sw` is anything that carries the A/B
switches of LlamaForCausalLM as attributes.  tests/decode_arms.py::SEQUENCES lists the launches of every plan."""
from collections import namedtuple
from dataclasses import dataclass
from typing import FrozenSet, Optional

import torch

from hydrainfer_amd._C.kernel import gemm as hip_gemm

HALF = (torch.float16, torch.bfloat16)
Dims = namedtuple("Dims", "hidden inter q_size qkv_n layers")


@dataclass(frozen=True)
class Layouts:
    """The packed layouts pack_decode_weights has built (before it ran: none, and how it would pack gate|up)."""
    mlp_xreg: bool = False                   # gate|up and down of every layer in the activations-in-registers layout
    qkv_xreg: bool = False                   # qkv of layers >= 1 in that layout
    gu_interleaved: bool = False             # gate|up halves interleaved (for the silu*mul epilogue), not in order
    lds_slice: FrozenSet[str] = frozenset()  # state keys with an LDS-slice copy

    def xreg_keys(self, layers: int) -> list:
        return ([f"l{l}.{p}" for l in range(layers) for p in ("wgu", "wdown")] if self.mlp_xreg else []) + \
               ([f"l{l}.wqkv" for l in range(1, layers)] if self.qkv_xreg else [])


def mlp_xreg_ok(d: Dims, n: int, dtype) -> bool:
    """gate|up and down of n <= 32 rows on the activations-in-registers kernel."""
    return bool(dtype in HALF and d.inter % 32 == 0 and d.hidden % 32 == 0
                and hip_gemm.xreg_supported(n, 2 * d.inter, d.hidden, dtype) and hip_gemm.xreg_supported(n, d.hidden, d.inter, dtype))


def qkv_xreg_ok(d: Dims, n: int, dtype) -> bool:
    return hip_gemm.xreg_supported(n, d.qkv_n, d.hidden, dtype)


def wide_ok(d: Dims, n: int, dtype, sw, gu_interleaved: bool) -> bool:
    """33 .. 64 rows on the <= 32-row packing (the wide kernel: no second copy): gate|up, down and qkv must all be
    supported.  hx_gate_up_xreg reads the INTERLEAVED packing; halves packed in order take the plain wide product."""
    gu = (hip_gemm.gate_up_xreg_supported(n, d.inter, d.hidden, dtype) if gu_interleaved
          else hip_gemm.xreg_supported(n, 2 * d.inter, d.hidden, dtype))
    return bool(32 < n <= 64 and sw.use_wide and sw.use_xreg and sw.xreg_qkv and mlp_xreg_ok(d, 32, dtype) and gu
                and hip_gemm.xreg_supported(n, d.hidden, d.inter, dtype) and qkv_xreg_ok(d, n, dtype) and qkv_xreg_ok(d, 32, dtype))


def plan_layouts(d: Dims, dtype, sw=None, all_lds_slice: bool = False, have: Optional[Layouts] = None) -> Layouts:
    """The layouts to have after packing on top of `have` (sw None: nothing is packed).  o and layer 0's qkv only take the
    LDS-slice layout (o: the x broadcast of the other kernel would dominate; layer 0's qkv: its x comes row-major from
    the embedding launch); the rest get an LDS-slice copy where they have no activations-in-registers one, or all_lds_slice."""
    have = have or Layouts(gu_interleaved=hip_gemm.gate_up_silu_supported(32, d.inter, d.hidden, dtype))
    if sw is None or not (sw.use_packed and dtype in HALF):
        return have
    mlp = have.mlp_xreg or bool(sw.use_xreg and mlp_xreg_ok(d, 32, dtype))
    qkv = have.qkv_xreg if have.mlp_xreg else bool(mlp and sw.xreg_qkv and d.layers > 1 and qkv_xreg_ok(d, 32, dtype))
    xreg = Layouts(mlp, qkv).xreg_keys(d.layers)
    nk = {"wqkv": (d.qkv_n, d.hidden), "wo": (d.hidden, d.q_size), "wgu": (2 * d.inter, d.hidden), "wdown": (d.hidden, d.inter)}
    lds = {f"l{l}.{p}" for l in range(d.layers) for p, (N, K) in nk.items()
           if (all_lds_slice or f"l{l}.{p}" not in xreg) and N % 16 == 0 and K % 256 == 0}
    return Layouts(mlp, qkv, have.gu_interleaved, have.lds_slice | lds)


@dataclass(frozen=True)
class StepPlan:
    """The variant of each stage of a layer (LlamaForCausalLM._stage_* say what each launches) and the floats of the
    step's slab buffers.  Layer 0's qkv and the last layer's close are always "rowmajor"."""
    qkv: str        # layers >= 1: "rowmajor" | "ex" | "wide" | "handover" (the previous layer's close wrote it)
    mlp: str        # "slabs" | "silu" | "plain" | "norm_silu" | "wide" | "wide_plain" | "norm_wide" | "norm_wide_silu"
    down: str       # "rowmajor" | "ex" | "wide"
    close: str      # "rowmajor" | "fm" | "handover"
    ws: int
    ws_q: Optional[int] = None      # qkv slabs of their own: the hand-over reads the down slabs in ws while it writes them
    ws_gu: Optional[int] = None     # gate|up slabs of the wide product (the norm-fused form reads the o slabs in ws meanwhile)
    xf = property(lambda s: s.mlp != "slabs")                        # fragment-major x
    actf = property(lambda s: s.mlp in ("silu", "norm_silu"))        # fragment-major activation of the fused <= 32-row launch
    actf_w = property(lambda s: s.mlp == "norm_wide_silu")           # ... of the wide one
    nf_gu = property(lambda s: s.mlp.startswith("norm_"))
    sync = property(lambda s: s.nf_gu or s.close == "handover")      # a hand-over area per norm-fused launch

    def flags(self) -> dict:
        """The six flags LlamaForCausalLM._decode_plan reports."""
        return {"xreg": self.xf, "fused": self.actf, "nf_gu": self.nf_gu, "nf_qkv": self.close == "handover",
                "wide": self.down == "wide", "wide_silu": self.actf_w}


def resolve(d: Dims, n: int, dtype, sw, lay: Layouts) -> StepPlan:
    """The plan of a decode step of n <= 64 rows."""
    g, hid, inter = hip_gemm, d.hidden, d.inter
    # qkv and an un-fused gate|up on the activations-in-registers kernel also land in ws where no norm-fused launch
    # gives them a buffer of their own (two slabs each at 33 .. 64 rows)
    ws = max(g.workspace_floats(n, d.qkv_n, hid), g.workspace_floats(n, hid, d.q_size), g.workspace_floats(n, 2 * inter, hid),
             g.workspace_floats(n, hid, inter), g.xreg_workspace_floats(n, hid, inter),
             g.xreg_workspace_floats(n, d.qkv_n, hid), g.xreg_workspace_floats(n, 2 * inter, hid))
    wide, il = n > 32, lay.gu_interleaved
    if not (sw.use_xreg and lay.mlp_xreg and (wide_ok(d, n, dtype, sw, il) if wide else mlp_xreg_ok(d, n, dtype))):
        return StepPlan("rowmajor", "slabs", "rowmajor", "rowmajor", ws)
    nf_qkv = sw.fuse_norm and lay.qkv_xreg and g.norm_xreg_supported(n, d.qkv_n, hid, dtype)
    close = "handover" if nf_qkv else "fm" if lay.qkv_xreg else "rowmajor"
    qkv = {"handover": "handover", "fm": "wide" if wide else "ex", "rowmajor": "rowmajor"}[close]
    ws_q = max(g.xreg_workspace_floats(n, d.qkv_n, hid), g.workspace_floats(n, d.qkv_n, hid)) if nf_qkv else None
    if not wide:
        fused = g.gate_up_silu_supported(n, inter, hid, dtype)
        nf_gu = sw.fuse_norm and fused and g.norm_xreg_supported(n, 2 * inter, hid, dtype, gate_up=True)
        return StepPlan(qkv, "norm_silu" if nf_gu else "silu" if fused else "plain", "ex", close, ws, ws_q)
    nf_gu = sw.fuse_norm and il and g.gate_up_xreg_supported(n, inter, hid, dtype, with_norm=True)
    if nf_gu and sw.use_wide_silu and g.gate_up_silu_wide_supported(n, inter, hid, dtype):
        return StepPlan(qkv, "norm_wide_silu", "wide", close, ws, ws_q)
    ws_gu = g.gate_up_xreg_workspace_floats(n, inter, hid) if il else g.xreg_workspace_floats(n, 2 * inter, hid)
    return StepPlan(qkv, "norm_wide" if nf_gu else "wide" if il else "wide_plain", "wide", close, ws, ws_q, ws_gu)
