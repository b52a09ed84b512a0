"""Decode-GEMM inputs whose answer is known exactly (pure torch, no GPU), shared by tests/test_gemm_exact_cpu.py (which
proves the inputs order-independent and the probe list complete) and tests/test_gpu_gemm_instantiations.py (which runs
them through every built kernel of csrc/gemm_xreg.hip and the LDS-slice family of csrc/gemm_skinny.hip).

EXACT INPUTS.  x and w are drawn from {j * step : |j| <= 15} with `step` a power of two (1/4 unless a test says
otherwise): exact in fp16 and bf16.  Every product is an integer multiple of the quantum step_x * step_w, every partial
sum of K of them has magnitude <= K * max|x| * max|w|, and as long as that is below 2^24 quanta every such sum is an
fp32 number: fp32 accumulation is exact in ANY order — whatever the k order, the split count, the per-workgroup
rotation of the k-steps or the MFMA's internal order.  exactness_bound() computes the figure and problem() asserts it
for whatever it generates.  The reference is x.double() @ w.double().t() on the CPU; comparisons are torch.equal on the
float64 sum of the slabs.

POISON AND GUARD.  poisoned(n) is a float32 buffer of n used elements filled with NaN followed by GUARD floats holding
SENTINEL; checked() asserts that the used part holds no NaN any more and that the tail is untouched.

STRIDED OPERANDS.  strided(t, pad) is a [:, :cols] view of a (rows, cols + pad) buffer whose gap columns hold `fill`.

ONE-HOT PROBES.  Row m of x is the unit vector at k_m, so row m of the product is column k_m of w, exactly.
probe_ks() lists the k that sit on a boundary of the kernels' k decomposition (split_ranges / wave_ranges below restate
it from the kernel comments: a launch split is 4 waves x KW k-steps of 32; the wide kernel's splits are the halves of the
packing's)."""
import functools
from typing import List, Tuple

import torch

LEVELS = 15                 # |j| <= LEVELS
STEP = 0.25
GUARD = 4096                # floats behind the used part of a workspace
SENTINEL = 12288.0          # exact in fp32, fp16 and bf16

# the candidate shapes of tests/test_gpu_gemm_instantiations.py: it picks, per instantiation, the cheapest (N, K) of
# N_VALUES (GU_N_VALUES for a gate|up weight: N = 2 * inter, inter % 32 == 0) x K_VALUES whose plan is that instantiation
N_VALUES = (96, 1056, 1104, 3072, 4128, 6144)
GU_N_VALUES = (192, 3072, 4160, 8256)       # (8256: 258 gate/up pairs over 256 workgroups)
K_VALUES = (512, 1024, 2048, 2560, 2816, 3456, 3584, 4096, 4128, 5120, 11008, 13824)
# LDS-slice family (csrc/gemm_skinny.hip), with the (waves, row groups per wave) its dispatch chooses by itself from
# units = N / 16 * splits (a split is 1024 of K) at <= 32 rows / at 33 .. 64 rows
LDS_SHAPES = (
    (1056, 2816),       # 198 units, a short last split: 4 x 1 / 4 x 1
    (48, 256),          # a single short split: 4 x 1 / 4 x 1
    (96, 11008),        # 11 splits: 8 x 2 / 4 x 2
    (65552, 256),       # 4097 units (> 4096), a ragged last workgroup: 8 x 3 / 8 x 3
    (5504, 2816),       # 1032 units: 4 x 1 / 8 x 1 (the 33 .. 64-row form's own choice)
)


def exactness_bound(K: int, max_x: float, max_w: float, quantum: float) -> float:
    """The largest magnitude, in quanta, that a sum of K products can reach."""
    return K * max_x * max_w / quantum


def assert_exact(K: int, max_x: float, max_w: float, quantum: float) -> float:
    b = exactness_bound(K, max_x, max_w, quantum)
    assert b < 2 ** 24, f"K={K} |x|<={max_x} |w|<={max_w} quantum={quantum}: {b} quanta, not below 2^24 — fp32 sums would round"
    return b


def grid_values(shape, seed: int, step: float = STEP) -> torch.Tensor:
    """float32 tensor of j * step, j uniform in -LEVELS .. LEVELS."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-LEVELS, LEVELS + 1, shape, generator=g, dtype=torch.int32).to(torch.float32) * step


class Problem:
    def __init__(self, x: torch.Tensor, w: torch.Tensor, x_step: float, w_step: float):
        K = x.shape[1]
        assert w.shape[1] == K
        self.x, self.w, self.quantum = x, w, x_step * w_step
        # every value a multiple of its step (so every product one of the quantum), and the bound: checked, not assumed
        assert torch.equal((x / x_step).round() * x_step, x) and torch.equal((w / w_step).round() * w_step, w)
        self.bound = assert_exact(K, x.abs().max().item(), w.abs().max().item(), self.quantum)
        self.ref = x.double() @ w.double().t()


@functools.lru_cache(maxsize=6)
def problem(M: int, N: int, K: int, seed: int = 0, x_step: float = STEP, w_step: float = STEP) -> Problem:
    """x [M, K], w [N, K] (float32 holders of values exact in fp16 / bf16) and ref = x @ w^T in float64.  Rows :m of x
    and of ref are the problem of m rows.  Cached: a reference is computed once and shared; do not write into it."""
    x = grid_values((M, K), 1000003 * seed + 7 * K + M, x_step)
    w = grid_values((N, K), 1000003 * seed + 13 * K + N + 1, w_step)
    return Problem(x, w, x_step, w_step)


def poisoned(used: int, device) -> torch.Tensor:
    buf = torch.empty(used + GUARD, dtype=torch.float32, device=device)
    buf[:used] = float("nan")
    buf[used:] = SENTINEL
    return buf


def checked(buf: torch.Tensor, used: int, what: str = "") -> torch.Tensor:
    """The used part of a poisoned(used) buffer after a launch: fully written, nothing written behind it."""
    assert buf.numel() == used + GUARD
    n_nan = int(torch.isnan(buf[:used]).sum())
    assert n_nan == 0, f"{what}: {n_nan} of {used} workspace floats were never written (first at {int(torch.isnan(buf[:used]).nonzero()[0])})"
    assert bool((buf[used:] == SENTINEL).all()), f"{what}: the guard behind the workspace was written"
    return buf[:used]


def strided(t: torch.Tensor, pad: int, fill: float = float("nan")) -> torch.Tensor:
    """A [:, :cols] view, equal to t, of a (rows, cols + pad) buffer whose other columns hold `fill`."""
    rows, cols = t.shape
    buf = torch.full((rows, cols + pad), fill, dtype=t.dtype, device=t.device)
    buf[:, :cols] = t
    return buf[:, :cols]


def gaps_hold(view: torch.Tensor, pad: int, fill: float) -> bool:
    """Do the gap columns of a strided(.., pad, fill) view still hold `fill`?"""
    rows, cols = view.shape
    whole = torch.as_strided(view, (rows, cols + pad), (cols + pad, 1))
    return bool((whole[:, cols:] == fill).all())


# ---- the k decomposition of the activations-in-registers kernels (csrc/gemm_xreg.hip), in k-steps of 32 ----------
def split_ranges(K: int, kw: int, wide: bool = False, pk_P: int = 0) -> List[Tuple[int, int]]:
    """(first k-step, k-steps) of every launch split.  Narrow kernel: split s starts at 4 * kw * s.  Wide kernel: the
    packing's split q starts at pk_P * q (pk_P: k-steps per split of the packing); its first half is 4 * kw k-steps, the
    second what is left of it — launch splits 2q and 2q + 1."""
    total, P = K // 32, 4 * kw
    out = []
    if not wide:
        for s0 in range(0, total, P):
            out.append((s0, min(P, total - s0)))
        return out
    assert pk_P in (2 * P, 2 * P - 4), (kw, pk_P)       # an odd packing count halves unevenly (27 -> 14 + 13)
    for q0 in range(0, total, pk_P):
        n = min(pk_P, total - q0)
        out.append((q0, min(P, n)))
        if n > P:
            out.append((q0 + P, n - P))
    return out


def wave_ranges(K: int, kw: int, wide: bool = False, pk_P: int = 0) -> List[Tuple[int, int, int, int]]:
    """(split, wave, first k-step, k-steps >= 1): wave v of a split owns its k-steps v * kw .. v * kw + kw - 1, as far
    as the split has them (the rest is padding)."""
    out = []
    for s, (s0, n) in enumerate(split_ranges(K, kw, wide, pk_P)):
        for v in range(4):
            a, b = s0 + v * kw, min(s0 + v * kw + kw, s0 + n)
            if a < b:
                out.append((s, v, a, b - a))
    return out


def probe_ks(K: int, kw: int, wide: bool = False, pk_P: int = 0) -> List[int]:
    """The k of the one-hot probes: 0, 31, 32, the first and the last k of every wave's share (which holds both sides of
    every split boundary), the first and last k of the last real k-step before the padding, K - 1."""
    ks = {0, 31, 32, K - 32, K - 1}
    for _, _, a, n in wave_ranges(K, kw, wide, pk_P):
        ks.add(32 * a)
        ks.add(32 * (a + n) - 1)
    return sorted(k for k in ks if 0 <= k < K)


def one_hot_rows(ks, K: int) -> torch.Tensor:
    x = torch.zeros((len(ks), K), dtype=torch.float32)
    x[torch.arange(len(ks)), torch.tensor(list(ks))] = 1.0
    return x
