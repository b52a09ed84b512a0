"""FP8 block-scaled expert weights restated in pure torch on the CPU (no GPU), shared by tests/test_moe_fp8_cpu.py (which
proves the properties of the inputs) and tests/test_gpu_moe_fp8.py (which runs them through csrc/moe_experts_fp8.hip).
Builds on tests/moe_block_ref.py, which it imports and does not change.

THE CONTRACT (include/hydra_hip.h, hx_moe_gate_up_silu_fp8w / hx_moe_down_fp8w):
    lin(row n of expert e, token row v) = T( sum_b scale[e, n / 128, b] * ( sum_{k in 128-block b} v[k] * q[e, n, k] ) )
fp32 sums of exact products, the scale applied to a block's fp32 partial sum, one rounding to T; a weight is never
rounded to T after scaling.  The rest is moe_block_ref's restatement with lin in place of its dot products, so the
expected tensors are its "exact" mode run on the DEQUANTISED weights float(q) * scale held in fp32 (they are exact there:
4 x 24 significant bits): float64 sums, rounded to T where the kernels round.

EXACT PAIRING (fp8_pairing): moe_block_ref.build_pairing's case with the weights stored as e4m3 bytes and a seeded
power-of-two scale from PAIRING_SCALES per (expert, 128 x 128 block).  The bytes are the case's weights DIVIDED by their
block's scale (grid values j / 4 over 1/4 .. 4 stay 4-bit numbers between 2^-4 and 15, the gate's 32 becomes 8 .. 128:
all on the e4m3 grid), so the dequantised weights are the case's own — a block met with another block's scale is off by
a power of two — and the expected tensors are the 16-bit test's.  Unrouted experts: 0x7F bytes (NaN) and NaN scales.
What is new for exactness is the sum over one 128-k block BEFORE its scale, which runs over the bytes: their maximum is
15 and their quantum 2^-4 (pairing_block_bound); once scaled, a block's sum is a partial sum of the 16-bit case, whose
bounds build_pairing asserts.

FINE SCALES (fine_case): one product per output.  x (resp. act) rows are one-hot with value 3, gate bytes 32 with scale 1
(silu(96) == 96), up / down bytes random grid values with scales (1 + m 2^-12) 2^e, m in 0 .. 4095, e in -3 .. 3: every
product 3 q s has at most 6 + 13 = 19 significant bits, so its fp32 value is exact and the result is the float64 value
rounded to T at the contract's rounding points.  The mutant (round_weight=True) rounds q * s to T first."""
import functools
from dataclasses import dataclass

import torch

from tests import gemm_exact as G
from tests import moe_block_ref as R

FP8 = torch.float8_e4m3fn
BLK = 128
NAN_BYTE = 0x7F
PAIRING_SCALES = (0.25, 0.5, 1.0, 2.0, 4.0)


def to_bytes(w: torch.Tensor) -> torch.Tensor:
    """uint8 e4m3 bytes of values that are exactly representable (asserted)."""
    q = w.to(FP8)
    assert torch.equal(q.float(), w.float()), "a value is not on the e4m3 grid"
    return q.view(torch.uint8)


def expand(scale: torch.Tensor) -> torch.Tensor:
    """[..., N / 128, K / 128] -> [..., N, K]."""
    return scale.repeat_interleave(BLK, dim=-2).repeat_interleave(BLK, dim=-1)


def dequant(q_bytes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """fp32 float(q) * scale, exact."""
    return q_bytes.view(FP8).float() * expand(scale)


# ---------------------------------------------------------------------------------------------------------------------
# exact pairing
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Fp8Pairing:
    p: R.Pairing
    qgu: torch.Tensor           # uint8 [E, 2I, h]; unrouted experts NAN_BYTE
    qdown: torch.Tensor         # uint8 [E, h, I]
    sgu: torch.Tensor           # fp32 [E, 2I / 128, h / 128]; unrouted experts NaN
    sdown: torch.Tensor         # fp32 [E, h / 128, I / 128]
    wgu: torch.Tensor           # fp32 dequantised (routed experts; NaN elsewhere)
    wdown: torch.Tensor


@functools.lru_cache(maxsize=8)
def fp8_pairing(case: R.PairingCase) -> Fp8Pairing:
    p = R.build_pairing(case)
    n_e, h, inter = case.E, case.h, case.I
    g = torch.Generator().manual_seed(9100 + 7 * n_e + h + inter)
    choices = torch.tensor(PAIRING_SCALES)
    sgu = choices[torch.randint(0, len(choices), (n_e, 2 * inter // BLK, h // BLK), generator=g)]
    sdown = choices[torch.randint(0, len(choices), (n_e, h // BLK, inter // BLK), generator=g)]
    qgu = to_bytes(torch.nan_to_num(p.wgu, nan=0.0) / expand(sgu))
    qdown = to_bytes(torch.nan_to_num(p.wdown, nan=0.0) / expand(sdown))
    qgu[~p.routed] = NAN_BYTE
    qdown[~p.routed] = NAN_BYTE
    sgu[~p.routed] = float("nan")
    sdown[~p.routed] = float("nan")
    return Fp8Pairing(p, qgu, qdown, sgu, sdown, dequant(qgu, sgu), dequant(qdown, sdown))


def pairing_block_bound() -> float:
    """The largest magnitude, in quanta, of a sum over one 128-k block of the down GEMM before its scale: act = 32 u is a
    multiple of 8 with |act| <= 120 (build_pairing), a byte a multiple of 1/4 / max scale with |q| <= 3.75 / min scale.
    (A gate / up block holds one product.)  Asserted below 2^24."""
    smax, smin = max(PAIRING_SCALES), min(PAIRING_SCALES)
    return G.assert_exact(BLK, R.GATE_VALUE * G.LEVELS * G.STEP, G.LEVELS * G.STEP / smin, 8 * G.STEP * G.STEP / smax)


def pairing_act(f: Fp8Pairing, T) -> torch.Tensor:
    """act [n * topk, I] in T: 32 * (the dequantised up weight at the token's k), exactly."""
    p, case = f.p, f.p.case
    flat, ks = p.ids.reshape(-1), p.x.argmax(dim=1)
    return torch.stack([R.GATE_VALUE * f.wgu[int(flat[s]), case.I:, int(ks[s // case.topk])] for s in range(flat.numel())]).to(T)


def pairing_y(f: Fp8Pairing, T) -> torch.Tensor:
    return R.expert_rows(f.p.x.to(T), f.p.ids, f.wgu, f.wdown, "exact")


def pairing_out(f: Fp8Pairing, T, shared: bool = True) -> torch.Tensor:
    return R.combine(pairing_y(f, T), f.p.w, f.p.shared.to(T) if shared else None, "exact")


# ---------------------------------------------------------------------------------------------------------------------
# fine scales: one product per output
# ---------------------------------------------------------------------------------------------------------------------
FINE_N, FINE_TOPK, FINE_E, FINE_H, FINE_I = 5, 2, 4, 640, 256
FINE_VALUE = 3.0
FINE_KS = (5, 200, 300, 511, 639)            # one k per 128-block of h; 511 | 639 sit on either side of the 512-k chunk


@dataclass
class FineCase:
    x: torch.Tensor             # [n, h] fp32 holder: FINE_VALUE at FINE_KS[t]
    act_in: torch.Tensor        # [n * topk, I]: FINE_VALUE at js[s] (the down launch's own input)
    js: torch.Tensor            # [n * topk]
    ids: torch.Tensor           # [n, topk] int32
    qgu: torch.Tensor           # uint8 [E, 2I, h]
    qdown: torch.Tensor
    sgu: torch.Tensor           # fp32 [E, 2I / 128, h / 128]: 1 for the gate rows
    sdown: torch.Tensor


def _fine_scales(shape, g) -> torch.Tensor:
    m = torch.randint(0, 4096, shape, generator=g).double()
    e = torch.randint(-3, 4, shape, generator=g).double()
    s = ((1 + m * 2.0 ** -12) * 2.0 ** e).float()
    assert torch.equal(s.double(), (1 + m * 2.0 ** -12) * 2.0 ** e)
    return s


@functools.lru_cache(maxsize=1)
def fine_case() -> FineCase:
    n, topk, n_e, h, inter = FINE_N, FINE_TOPK, FINE_E, FINE_H, FINE_I
    g = torch.Generator().manual_seed(4242)
    x = G.one_hot_rows(FINE_KS, h) * FINE_VALUE
    ids = torch.stack([torch.randperm(n_e, generator=g)[:topk] for _ in range(n)]).to(torch.int32)
    js = torch.randint(0, inter, (n * topk,), generator=g)
    js[0], js[1], js[2] = 0, 127, 128                       # both k-blocks of the down GEMM and their border
    act_in = torch.zeros((n * topk, inter))
    act_in[torch.arange(n * topk), js] = FINE_VALUE
    up = G.grid_values((n_e, inter, h), 51)
    qgu = to_bytes(torch.cat([torch.full((n_e, inter, h), R.GATE_VALUE), up], dim=1))
    qdown = to_bytes(G.grid_values((n_e, h, inter), 52))
    sgu = torch.cat([torch.ones((n_e, inter // BLK, h // BLK)), _fine_scales((n_e, inter // BLK, h // BLK), g)], dim=1)
    sdown = _fine_scales((n_e, h // BLK, inter // BLK), g)
    return FineCase(x, act_in, js, ids, qgu, qdown, sgu, sdown)


def _scaled(q_col: torch.Tensor, s_col: torch.Tensor, T, round_weight: bool) -> torch.Tensor:
    """T(3 * q * s) in float64 — or, the mutant, T(3 * T(q * s))."""
    w = q_col.double() * s_col.double()
    if round_weight:
        w = w.to(T).double()
    return (FINE_VALUE * w).to(T)


def fine_act(c: FineCase, T, round_weight: bool = False) -> torch.Tensor:
    """act [n * topk, I]: g = T(3 * 32) = 96, a = T(silu(96)) = 96, u = T(3 q s), act = T(96 u)."""
    inter = FINE_I
    flat = c.ids.reshape(-1).long()
    sgu = expand(c.sgu)
    rows = []
    for s in range(flat.numel()):
        e, k = int(flat[s]), FINE_KS[s // FINE_TOPK]
        u = _scaled(c.qgu[e, inter:, k].view(FP8).float(), sgu[e, inter:, k], T, round_weight)
        rows.append((FINE_VALUE * R.GATE_VALUE * u.double()).to(T))
    return torch.stack(rows)


def fine_y(c: FineCase, T, round_weight: bool = False) -> torch.Tensor:
    """y [n * topk, h] of the down launch fed with act_in: T(3 q s)."""
    flat = c.ids.reshape(-1).long()
    sdown = expand(c.sdown)
    return torch.stack([_scaled(c.qdown[int(flat[s]), :, int(c.js[s])].view(FP8).float(), sdown[int(flat[s]), :, int(c.js[s])],
                                T, round_weight) for s in range(flat.numel())])


# ---------------------------------------------------------------------------------------------------------------------
# published names
# ---------------------------------------------------------------------------------------------------------------------
def published(sd, quantize):
    """A reference-named state dict whose ...experts.{e}.{gate,up,down}_proj.weight are float8_e4m3fn with
    ...weight_scale_inv beside them (quantize: hydrainfer_amd's quantize_fp8_block); everything else as it is."""
    out = {}
    for k, v in sd.items():
        if ".experts." in "." + k and k.endswith("_proj.weight") and "shared_experts" not in k:
            q, s = quantize(v)
            out[k], out[k[:-len("weight")] + "weight_scale_inv"] = q, s
        else:
            out[k] = v
    return out


def dequantised_sd(sd, T):
    """The inverse, for the CPU oracle: expert weights float(q) * scale, cast to T (the oracle's F.linear takes one
    dtype; the cast moves a weight by at most half an ulp of T, far inside the logit tolerances it is used with)."""
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_scale_inv"):
            continue
        if v.dtype == FP8:
            out[k] = dequant(v.view(torch.uint8), sd[k[:-len("weight")] + "weight_scale_inv"]).to(T)
        else:
            out[k] = v
    return out
