"""MXFP4 expert weights restated in pure torch on the CPU, shared by tests/test_moe_mxfp4_cpu.py and
tests/test_gpu_moe_mxfp4.py (which runs the cases through csrc/moe_experts_mxfp4.hip).  Builds on tests/moe_block_ref.py,
which it imports and does not change.

THE CONTRACT (include/hydra_hip.h, hx_moe_gate_up_silu_mxfp4w / hx_moe_down_mxfp4w):
    lin(row n of expert e, token row v) = T( sum_g 2^(s[e, n, g] - 127) * ( sum_{k in 32-group g} v[k] * q[e, n, k] ) )
fp32 sums of exact products, one rounding to T, no weight rounded after scaling.  The expected tensors are
moe_block_ref's "exact" restatement (float64 sums, rounded to T where the kernels round) over the weights of
dequantize_mxfp4, which are exact in fp32 here.

EXACT PAIRING (mx_pairing): moe_block_ref.build_pairing's tokens, routing and shared term; every weight nibble and every
scale byte seeded.  Gate rows dequantise to 32 everywhere (silu(32) == 32) but through a seeded (code, byte) pair per
group — 0.5 * 2^6, 1 * 2^5, 2 * 2^4 or 4 * 2^3 — up elements are any of the 16 codes with scales 2^-5 .. 2^-3 and down
elements any code with scales 2^-3 .. 2^-1, so an element met with another group's scale, or the other nibble of its
byte, is another number.  act = 32 u is a multiple of 1/2 with |act| <= 24; a down sum of I products |w| <= 3 of quantum
1/32 stays an fp32 number (asserted).  Unrouted experts hold scale byte 0xFF: NaN weights.

WIDE SCALES (wide_case): one product per output.  Group g of K carries the scale exponent WIDE_EXP[g] (+ a seeded -1 / 0
/ +1 per row), from 2^-24 to 2^15; the token that is one-hot in group g has the power of two x = 2^-WIDE_EXP[g], clamped
to fp16's normal range, so every expected value T(x * q * 2^e) is a normal number of both types although 0.5 * 2^-25 and
6 * 2^15 are not fp16 numbers: a kernel that rounded the scaled weight to T would be caught."""
import functools
from dataclasses import dataclass

import torch

from hydrainfer_amd._C.kernel.moe.experts import dequantize_mxfp4
from tests import gemm_exact as G
from tests import moe_block_ref as R

NAN_BYTE = 0xFF
GATE_PAIRS = ((1, 133), (2, 132), (4, 131), (6, 130))      # (E2M1 code, scale byte): 0.5 * 2^6 = 1 * 2^5 = 2 * 2^4 = 4 * 2^3 = 32
UP_BYTES, DOWN_BYTES = (122, 123, 124), (124, 125, 126)


def pack(codes: torch.Tensor) -> torch.Tensor:
    """uint8 [..., K] codes 0..15 -> [..., K / 2] bytes: element 2j in bits 0-3, 2j + 1 in bits 4-7."""
    c = codes.to(torch.uint8).reshape(*codes.shape[:-1], codes.shape[-1] // 2, 2)
    return c[..., 0] | (c[..., 1] << 4)


def _rand(shape, choices, g) -> torch.Tensor:
    return torch.tensor(choices, dtype=torch.uint8)[torch.randint(0, len(choices), shape, generator=g)]


@dataclass
class MxPairing:
    p: R.Pairing
    qgu: torch.Tensor           # uint8 [E, 2I, h / 2]
    qdown: torch.Tensor         # uint8 [E, h, I / 2]
    sgu: torch.Tensor           # uint8 [E, 2I, h / 32]; unrouted experts NAN_BYTE
    sdown: torch.Tensor         # uint8 [E, h, I / 32]
    wgu: torch.Tensor           # fp32 dequantised (NaN in the unrouted experts)
    wdown: torch.Tensor


@functools.lru_cache(maxsize=8)
def mx_pairing(case: R.PairingCase) -> MxPairing:
    p = R.build_pairing(case)
    n_e, h, inter = case.E, case.h, case.I
    g = torch.Generator().manual_seed(9400 + 7 * n_e + h + inter)
    pair = torch.randint(0, len(GATE_PAIRS), (n_e, inter, h // 32), generator=g)
    pairs = torch.tensor(GATE_PAIRS, dtype=torch.uint8)
    gate_codes = pairs[pair][..., 0].repeat_interleave(32, dim=-1)
    qgu = pack(torch.cat([gate_codes, torch.randint(0, 16, (n_e, inter, h), generator=g).to(torch.uint8)], dim=1))
    sgu = torch.cat([pairs[pair][..., 1], _rand((n_e, inter, h // 32), UP_BYTES, g)], dim=1)
    qdown = pack(torch.randint(0, 16, (n_e, h, inter), generator=g))
    sdown = _rand((n_e, h, inter // 32), DOWN_BYTES, g)
    sgu[~p.routed] = NAN_BYTE
    sdown[~p.routed] = NAN_BYTE
    wgu, wdown = dequantize_mxfp4(qgu, sgu), dequantize_mxfp4(qdown, sdown)
    assert bool((wgu[p.routed][:, :inter] == R.GATE_VALUE).all()) and bool(torch.isnan(wgu[~p.routed]).all())
    G.assert_exact(inter, R.GATE_VALUE * 6 * 2.0 ** -3, 6 * 2.0 ** -1, R.GATE_VALUE * 0.5 * 2.0 ** -5 * 0.5 * 2.0 ** -3)
    return MxPairing(p, qgu, qdown, sgu, sdown, wgu, wdown)


def pairing_act(f: MxPairing, T) -> torch.Tensor:
    """act [n * topk, I] in T: 32 * (the dequantised up weight at the token's k), exactly."""
    p, case = f.p, f.p.case
    flat, ks = p.ids.reshape(-1), p.x.argmax(dim=1)
    return torch.stack([R.GATE_VALUE * f.wgu[int(flat[s]), case.I:, int(ks[s // case.topk])] for s in range(flat.numel())]).to(T)


def pairing_y(f: MxPairing, T) -> torch.Tensor:
    return R.expert_rows(f.p.x.to(T), f.p.ids, f.wgu, f.wdown, "exact")


def pairing_out(f: MxPairing, T) -> torch.Tensor:
    return R.combine(pairing_y(f, T), f.p.w, f.p.shared.to(T), "exact")


# ---------------------------------------------------------------------------------------------------------------------
# wide scales: one product per output
# ---------------------------------------------------------------------------------------------------------------------
WIDE_N, WIDE_TOPK, WIDE_E, WIDE_H, WIDE_I = 16, 2, 4, 256, 256
WIDE_EXP = (-24, -19, -13, -6, 0, 4, 8, 15)          # the scale exponent of the eight 32-k groups of K = 256
NONZERO = (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15)


def _x_exp(group: int) -> int:
    return max(-14, min(14, -WIDE_EXP[group]))


@dataclass
class WideCase:
    x: torch.Tensor             # [n, h] fp32 holder: 2^_x_exp(group) at ks[t]
    ks: torch.Tensor            # [n]: two k per group, at different words and nibbles of the group's 16 bytes
    act_in: torch.Tensor        # [n * topk, I]: the down launch's own input, one-hot at js[s]
    js: torch.Tensor            # [n * topk]
    ids: torch.Tensor           # [n, topk] int32
    qgu: torch.Tensor
    qdown: torch.Tensor
    sgu: torch.Tensor
    sdown: torch.Tensor


@functools.lru_cache(maxsize=1)
def wide_case() -> WideCase:
    n, topk, n_e, h, inter = WIDE_N, WIDE_TOPK, WIDE_E, WIDE_H, WIDE_I
    g = torch.Generator().manual_seed(4343)
    ks = torch.tensor([32 * (t // 2) + (5, 30)[t % 2] for t in range(n)])
    ids = torch.stack([torch.randperm(n_e, generator=g)[:topk] for _ in range(n)]).to(torch.int32)
    js = torch.tensor([32 * (s % 8) + (0, 9, 22, 31)[s // 8] for s in range(n * topk)])
    x = torch.zeros((n, h))
    x[torch.arange(n), ks] = torch.tensor([2.0 ** _x_exp(int(k) // 32) for k in ks])
    act_in = torch.zeros((n * topk, inter))
    act_in[torch.arange(n * topk), js] = torch.tensor([2.0 ** _x_exp(int(j) // 32) for j in js])
    base = torch.tensor([127 + e for e in WIDE_EXP])
    # gate: x * 4 * 2^(3 - x's exponent) = 32 whatever the group
    gate_s = torch.tensor([130 - _x_exp(gr) for gr in range(8)]).expand(n_e, inter, 8)
    up_s = base + torch.randint(-1, 2, (n_e, inter, h // 32), generator=g)
    qgu = pack(torch.cat([torch.full((n_e, inter, h), 6), _rand((n_e, inter, h), NONZERO, g)], dim=1))
    sgu = torch.cat([gate_s, up_s], dim=1).to(torch.uint8)
    qdown = pack(_rand((n_e, h, inter), NONZERO, g))
    sdown = (base + torch.randint(-1, 2, (n_e, h, inter // 32), generator=g)).to(torch.uint8)
    w = dequantize_mxfp4(qgu, sgu, torch.float64)[:, inter:]
    assert int((w.to(torch.float16).double() != w).sum()) > 0 and int(up_s.min()) <= 103 and int(up_s.max()) >= 135
    return WideCase(x, ks, act_in, js, ids, qgu, qdown, sgu.contiguous(), sdown.contiguous())


def _normal(v: torch.Tensor, T) -> bool:
    return bool(((v.abs() >= torch.finfo(T).tiny) & (v.abs() <= torch.finfo(T).max)).all())


def wide_act(c: WideCase, T) -> torch.Tensor:
    """act [n * topk, I]: g = T(x * 4 * 2^eg) = 32 = T(silu(g)), u = T(x * q * 2^e), act = T(32 u); all normal numbers of T."""
    w = dequantize_mxfp4(c.qgu, c.sgu, torch.float64)
    flat = c.ids.reshape(-1).long()
    rows = []
    for s in range(flat.numel()):
        t = s // WIDE_TOPK
        col = w[int(flat[s]), :, int(c.ks[t])] * c.x[t, c.ks[t]].double()
        assert bool((col[:WIDE_I] == R.GATE_VALUE).all()) and _normal(col[WIDE_I:], T)
        u = col[WIDE_I:].to(T)
        assert torch.equal(u.double(), col[WIDE_I:])
        rows.append((R.GATE_VALUE * u.double()).to(T))
    return torch.stack(rows)


def wide_y(c: WideCase, T) -> torch.Tensor:
    """y [n * topk, h] of the down launch fed with act_in: T(x * q * 2^e)."""
    w = dequantize_mxfp4(c.qdown, c.sdown, torch.float64)
    flat = c.ids.reshape(-1).long()
    rows = [w[int(flat[s]), :, int(c.js[s])] * c.act_in[s, c.js[s]].double() for s in range(flat.numel())]
    assert all(_normal(r, T) for r in rows)
    return torch.stack(rows).to(T)


def dequantised_sd(sd, T):
    """A reference-named state dict with MXFP4 experts, for the CPU oracle: packed weights as element * scale cast to T
    (exact for bf16; fp16 moves a weight by at most half an ulp, far inside the logit tolerances it is used with)."""
    out = {}
    for k, v in sd.items():
        if k.endswith("weight_scale"):
            continue
        out[k] = dequantize_mxfp4(v, sd[k + "_scale"]).to(T) if v.dtype == torch.uint8 else v
    return out
