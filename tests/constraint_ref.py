"""The reference the token-constraint tests measure against (include/hydra_hip.h: hx_sample_rows_constrained), on the CPU:
- `biased_row`: the fp32 row after the bias table, by torch CPU fp32 addition — the kernel's x_t bit for bit;
- `check_row_constrained`: sampling_ref.check_row over the biased row, extended with the min_p rule;
- `reference_sample_constrained`: the float64 sampler of the contract.

The min_p margin.  M = {i : e_i >= min_p} is decided by the kernel on e = expf(z - m) in fp32; fp32 expf plus the rounding
of z - m deviates from float64 by about 1e-5 relative for |z - m| <= ~100, so an element whose float64 e lies within
DELTA = sampling_ref.DELTA (1e-4, the project's acceptance margin) RELATIVE to min_p may fall on either side: every kept z
has e >= min_p * (1 - DELTA), every z below the cut has e <= min_p * (1 + DELTA) unless top-k or top-p explains the cut.
Both follow from: the cut passes sampling_ref's check 2 from SOME v_K' = max(v_K, v_M) whose v_M is a value of the row
inside that band."""
import math

import numpy as np
import torch

from tests import penalty_ref
from tests import sampling_ref as ref

DELTA = ref.DELTA


def biased_row(x: torch.Tensor, ids, values) -> torch.Tensor:
    """fp32 [n]: float(x) with values[j] added at ids[j] (one fp32 addition each; ids outside the row are ignored)."""
    row = x.float().clone()
    for t, b in zip(ids, values):
        if 0 <= int(t) < row.numel():
            row[int(t)] = row[int(t)] + torch.tensor(float(b), dtype=torch.float32)
    return row


def min_p_band(z: np.ndarray, min_p: float):
    """(lo, hi): v_M computed with min_p * (1 - DELTA) and with min_p * (1 + DELTA) — the kernel's v_M lies in [lo, hi].
    min_p <= 1, so the maximum (e = 1) is in the first set; the second may be empty: then hi is the maximum."""
    e = np.exp(z.astype(np.float64) - np.float64(z.max()))
    lo = z[e >= min_p * (1 - DELTA)].min()
    above = z[e >= min_p * (1 + DELTA)]
    return lo, (above.min() if above.size else z.max())


def check_cut_from(z: np.ndarray, vk, top_p: float, cut, what="") -> None:
    """sampling_ref.check_cut with the base cut given (v_K' in place of v_K)."""
    cut = np.float32(cut)
    assert np.any(z == cut), f"{what}: the cut {cut!r} is no value of the row"
    assert cut >= vk, f"{what}: the cut {cut!r} lies below v_K' = {vk!r}"
    if top_p >= 1:
        assert cut == vk, f"{what}: top_p >= 1 but the cut {cut!r} != v_K' = {vk!r}"
        return
    e = np.exp(z.astype(np.float64) - np.float64(z.max()))
    zk = e[z >= vk].sum()
    a = e[z > cut].sum()
    assert a <= (top_p + DELTA) * zk, f"{what}: A(v*) / Z_K = {a / zk!r} above top_p = {top_p} + {DELTA}"
    if cut > vk:
        below = z[z < cut].max()
        a = e[z > below].sum()
        assert a > (top_p - DELTA) * zk, f"{what}: A(v') / Z_K = {a / zk!r} for the next value below the cut: it would do"


def check_cut_constrained(z: np.ndarray, top_k: int, top_p: float, min_p: float, cut, what="") -> None:
    assert z.dtype == np.float32
    cut = np.float32(cut)
    vk = ref.kth_largest(z, top_k)
    e = np.exp(z.astype(np.float64) - np.float64(z.max()))
    kept = e[z >= cut]
    assert kept.size and kept.min() >= min_p * (1 - DELTA), \
        f"{what}: a kept element has e = {kept.min() if kept.size else None!r} < min_p = {min_p} (1 - {DELTA})"
    lo, hi = min_p_band(z, min_p)
    candidates = sorted(set(np.unique(z[(z >= lo) & (z <= hi)]).tolist()) | {float(hi)})
    errors = []
    for vm in candidates:
        try:
            check_cut_from(z, max(vk, np.float32(vm)), top_p, cut, what)
            return
        except AssertionError as err:
            errors.append(str(err))
    raise AssertionError(f"{what}: the cut {cut!r} follows from no v_M in [{lo!r}, {hi!r}] (min_p = {min_p}): " + "; ".join(errors))


def check_row_constrained(x: torch.Tensor, bias_ids, bias_values, ids, counts, penalties, record, token: int, cut: float,
                          u: float, what="") -> str:
    """One row of a constrained launch.  record: (temperature, top_p, top_k, seed, offset[, min_p]).  Returns 'greedy',
    'degenerate' or 'sampled'."""
    xb = biased_row(x, bias_ids, bias_values)
    min_p = record[5] if len(record) > 5 else 0.0
    if not min_p > 0:
        return ref.check_row(xb, ids, counts, penalties, tuple(record[:5]), token, cut, u, what)
    temperature, top_p, top_k, seed, offset = record[:5]
    assert np.float32(u).view(np.uint32) == ref.uniform(seed, offset).view(np.uint32), f"{what}: u {u!r} != Philox's"
    s, z = ref.scaled_row(xb, ids, counts, penalties, temperature if temperature > 0 else 1.0)
    if temperature <= 0 or ref.is_degenerate(z):
        want = penalty_ref.argmax_in_order(s)
        assert token == want and math.isnan(cut), f"{what}: greedy / degenerate row gave {token} (cut {cut!r}), want {want}"
        return "greedy" if temperature <= 0 else "degenerate"
    z = z.numpy()
    check_cut_constrained(z, top_k, top_p, min(min_p, 1.0), cut, what)
    ref.check_draw(z, cut, u, token, what)
    return "sampled"


def reference_sample_constrained(z: np.ndarray, top_k: int, top_p: float, min_p: float, u: float):
    """(token, cut) of the contract with float64 sums and a float64 e: sampling_ref.reference_sample from v_K'."""
    vk = ref.kth_largest(z, top_k)
    e = np.exp(z.astype(np.float64) - np.float64(z.max()))
    if min_p > 0:
        vk = max(vk, z[e >= min(min_p, 1.0)].min())
    cut = vk
    if top_p < 1:
        zk = e[z >= vk].sum()
        cut = min(v for v in np.unique(z[z >= vk]) if e[z > v].sum() <= top_p * zk)
    s = np.where(z >= cut, e, 0.0)
    c = np.cumsum(s)
    over = np.nonzero((c > float(u) * s.sum()) & (z >= cut))[0]
    return int(over[0]) if over.size else int(np.nonzero(z >= cut)[0][-1]), np.float32(cut)
