"""The reference the sampling tests measure against (include/hydra_hip.h: hx_sample_rows), on the CPU:
- Philox4x32-10 in numpy integers and the uniform number made from its first word;
- z, the scaled logits, by torch CPU fp32 arithmetic — the penalised row of tests/penalty_ref.py, then ONE division:
  the kernel's z bit for bit, so v_K is exact and a cut can be looked up in the row;
- float64 versions of A(v), Z_K and the index-order CDF, and the two acceptance checks built on them: `check_cut`
  (the top-k / top-p cut) and `check_draw` (the token against u).  DELTA is the issue's 1e-4: the kernel compares a
  handful of fp32 sums of non-negative terms, each accumulated per thread and then combined by a tree; emulated on the
  CPU that deviates from float64 by about 1e-6 of the total."""
import math

import numpy as np
import torch

from tests import penalty_ref

DELTA = 1e-4
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four 32-bit words, key: two -> the four output words (Random123's philox4x32_R(10, ...))."""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed: int, offset: int) -> np.float32:
    """u of a (seed, offset): the top 24 bits of the first word, in [0, 1)."""
    w = philox4x32_10((offset & MASK, offset >> 32, 0, 0), (seed & MASK, seed >> 32))[0]
    return np.float32(w >> 8) * np.float32(2.0 ** -24)


def scaled_row(x: torch.Tensor, ids, counts, penalties, temperature: float):
    """(s, z): the penalised fp32 row of penalty_ref and z = s / T in torch CPU fp32 (one division, as logits.div_)."""
    s = penalty_ref.penalized_row(x, ids, counts, *penalties)[0]
    return s, s / torch.tensor(temperature, dtype=torch.float32)


def is_degenerate(z: torch.Tensor) -> bool:
    """a NaN in the row, or a largest value that is not finite: the row is sampled greedily"""
    return bool(torch.isnan(z).any()) or not math.isfinite(float(z.max()))


def kth_largest(z: np.ndarray, top_k: int):
    n = z.size
    k = n if top_k <= 0 or top_k >= n else top_k
    return np.sort(z)[n - k]


def check_cut(z: np.ndarray, top_k: int, top_p: float, cut: float, what="") -> None:
    """z: fp32 [n], the row.  The issue's check 2."""
    assert z.dtype == np.float32
    cut = np.float32(cut)
    vk = kth_largest(z, top_k)
    assert np.any(z == cut), f"{what}: the cut {cut!r} is no value of the row"
    assert cut >= vk, f"{what}: the cut {cut!r} lies below v_K = {vk!r}"
    if top_p >= 1:
        assert cut == vk, f"{what}: top_p >= 1 but the cut {cut!r} != v_K = {vk!r}"
        return
    e = np.exp(z.astype(np.float64) - np.float64(z.max()))
    zk = e[z >= vk].sum()
    a = e[z > cut].sum()
    assert a <= (top_p + DELTA) * zk, f"{what}: A(v*) / Z_K = {a / zk!r} above top_p = {top_p} + {DELTA}"
    if cut > vk:
        below = z[z < cut].max()
        a = e[z > below].sum()
        assert a > (top_p - DELTA) * zk, f"{what}: A(v') / Z_K = {a / zk!r} for the next value below the cut: it would do"


def check_draw(z: np.ndarray, cut: float, u: float, token: int, what="") -> None:
    """The issue's check 3: the token lies in S(v*), and u inside its slice of the index-order CDF, +- DELTA."""
    cut = np.float32(cut)
    assert 0 <= token < z.size and z[token] >= cut, f"{what}: token {token} is not in S"
    e = np.where(z >= cut, np.exp(z.astype(np.float64) - np.float64(z.max())), 0.0)
    total = e.sum()
    incl = e[:token + 1].sum() / total
    excl = e[:token].sum() / total
    assert excl - DELTA <= float(u) <= incl + DELTA, f"{what}: u = {u!r} outside [{excl!r}, {incl!r}] of token {token}"


def check_row(x: torch.Tensor, ids, counts, penalties, record, token: int, cut: float, u: float, what="") -> str:
    """One row of a launch against everything above.  record: (temperature, top_p, top_k, seed, offset).  Returns
    'greedy', 'degenerate' or 'sampled'."""
    temperature, top_p, top_k, seed, offset = record
    assert np.float32(u).view(np.uint32) == uniform(seed, offset).view(np.uint32), f"{what}: u {u!r} != Philox's {uniform(seed, offset)!r}"
    s, z = scaled_row(x, ids, counts, penalties, temperature if temperature > 0 else 1.0)
    if temperature <= 0 or is_degenerate(z):
        want = penalty_ref.argmax_in_order(s)
        assert token == want and math.isnan(cut), f"{what}: greedy / degenerate row gave {token} (cut {cut!r}), want {want}"
        return "greedy" if temperature <= 0 else "degenerate"
    z = z.numpy()
    check_cut(z, top_k, top_p, cut, what)
    check_draw(z, cut, u, token, what)
    return "sampled"


def reference_sample(z: np.ndarray, top_k: int, top_p: float, u: float):
    """(token, cut) of the contract with float64 sums — what a kernel with exact sums would give; the checks above accept
    it (test_sampling_cpu.py), and a kernel whose fp32 sums stay within DELTA of these."""
    vk = kth_largest(z, top_k)
    e = np.exp(z.astype(np.float64) - np.float64(z.max()))
    cut = vk
    if top_p < 1:
        zk = e[z >= vk].sum()
        cut = min(v for v in np.unique(z[z >= vk]) if e[z > v].sum() <= top_p * zk)
    s = np.where(z >= cut, e, 0.0)
    c = np.cumsum(s)
    over = np.nonzero((c > float(u) * s.sum()) & (z >= cut))[0]
    return int(over[0]) if over.size else int(np.nonzero(z >= cut)[0][-1]), np.float32(cut)
