"""FP8 block-scaled dense linears restated in pure torch on the CPU (no GPU), shared by tests/test_linear_fp8_cpu.py (which
proves the properties of the inputs), tests/test_gpu_linear_fp8.py (which runs them through csrc/gemm_skinny_fp8.hip) and
tests/test_gpu_moe_model_fp8_dense.py.  Builds on tests/gemm_exact.py and tests/moe_fp8_ref.py, which it does not change.

THE CONTRACT (include/hydra_hip.h, hx_linear_decode_fp8w):
    out[m][n] = T( sum over splits s of sum over 128-k blocks b of s of scale[n / 128][b] * ( sum_{k in b} x[m][k] * q[n][k] ) )
fp32 sums of exact products, a block's scale applied to the block's fp32 partial sum with one fma, one rounding to T; a
weight is never rounded after it has been scaled.

EXACT CASE (exact_case): x from gemm_exact.grid_values (j / 4, |j| <= 15); the dequantised weights are grid values too and
the bytes are those values DIVIDED by their block's power-of-two scale PAIRING_SCALES[(3 nb + kb) % 5] (to_bytes asserts
they lie on the e4m3 grid): every block differs from its neighbours in both directions, so a block met with another
block's scale is off by a power of two (neighbour_mutant).  The sum over one block of the bytes and the scaled running
sums stay below 2^24 quanta (asserted), so every fp32 sum is exact in any order and the answer is the float64 product.

FINE SCALES (fine_case): one product per output.  Row m of x is 3 at k_m, the bytes are random grid values, the scales
(1 + m 2^-12) 2^e: every product 3 q s has at most 6 + 13 = 19 significant bits, so the result is the float64 value
rounded once to T.  The mutant rounds q * s to T first.  The k_m sit on the boundaries of the k decomposition (fine_ks)."""
import functools
from dataclasses import dataclass

import torch

from tests import gemm_exact as G
from tests import moe_fp8_ref as F8

FP8, BLK, NAN_BYTE = F8.FP8, F8.BLK, F8.NAN_BYTE
SPLIT_K = 1024                  # k per launch split (csrc/gemm_skinny.hip: 32 k-steps of 32)
MAX_ROWS = 64


def pairing_scales(N: int, K: int, shift: int = 0) -> torch.Tensor:
    """fp32 [N / 128, K / 128]: PAIRING_SCALES[(3 nb + kb + shift) % 5]."""
    nb, kb = torch.arange(N // BLK)[:, None], torch.arange(K // BLK)[None, :]
    return torch.tensor(F8.PAIRING_SCALES)[(3 * nb + kb + shift) % len(F8.PAIRING_SCALES)]


@dataclass
class ExactCase:
    x: torch.Tensor             # [64, K] fp32 holder of grid values; rows :M are the problem of M rows
    q: torch.Tensor             # uint8 [N, K]
    scale: torch.Tensor         # fp32 [N / 128, K / 128]
    ref: torch.Tensor           # float64 [64, N]
    block_bound: float
    sum_bound: float


@functools.lru_cache(maxsize=8)
def exact_case(N: int, K: int) -> ExactCase:
    x = G.grid_values((MAX_ROWS, K), 7 * K + 11)
    w = G.grid_values((N, K), 13 * K + N + 5)
    scale = pairing_scales(N, K)
    q = F8.to_bytes(w / F8.expand(scale))
    smax, smin = max(F8.PAIRING_SCALES), min(F8.PAIRING_SCALES)
    # one block of the bytes, before its scale: |q| <= 15 / 4 / smin, a multiple of 1 / 4 / smax
    block_bound = G.assert_exact(BLK, G.LEVELS * G.STEP, G.LEVELS * G.STEP / smin, G.STEP * G.STEP / smax)
    # the scaled running sums: partial sums of x . w, whose quantum is 1 / 16
    sum_bound = G.assert_exact(K, G.LEVELS * G.STEP, G.LEVELS * G.STEP, G.STEP * G.STEP)
    assert float(q.view(FP8).float().abs().max()) <= G.LEVELS * G.STEP / smin
    return ExactCase(x, q, scale, x.double() @ w.double().t(), block_bound, sum_bound)


def neighbour_mutant(c: ExactCase) -> torch.Tensor:
    """The answer of a kernel that meets every block with its k-neighbour's scale."""
    N, K = c.q.shape
    return c.x.double() @ F8.dequant(c.q, pairing_scales(N, K, shift=1)).double().t()


# ---------------------------------------------------------------------------------------------------------------------
FINE_VALUE = 3.0


def fine_ks(K: int):
    """0, 127, 128, 255, 256, 1023, 1024, the first and the last k of the (short) last split, K - 1."""
    last0 = (K - 1) // SPLIT_K * SPLIT_K
    return sorted({k for k in (0, 127, 128, 255, 256, 1023, 1024, last0, K - 1) if 0 <= k < K})


@dataclass
class FineCase:
    ks: tuple
    x: torch.Tensor             # [len(ks), K]: FINE_VALUE at ks[m]
    q: torch.Tensor             # uint8 [N, K]
    scale: torch.Tensor


@functools.lru_cache(maxsize=2)
def fine_case(N: int = 256, K: int = 2816) -> FineCase:
    g = torch.Generator().manual_seed(777 + K)
    ks = tuple(fine_ks(K))
    q = F8.to_bytes(G.grid_values((N, K), 61))
    return FineCase(ks, G.one_hot_rows(ks, K) * FINE_VALUE, q, F8._fine_scales((N // BLK, K // BLK), g))


def fine_out(c: FineCase, T, round_weight: bool = False) -> torch.Tensor:
    """[len(ks), N]: T(3 q s) in float64 — or, the mutant, T(3 T(q s))."""
    w = c.q.view(FP8).float().double() * F8.expand(c.scale).double()
    if round_weight:
        w = w.to(T).double()
    return torch.stack([(FINE_VALUE * w[:, k]).to(T) for k in c.ks])


# ---------------------------------------------------------------------------------------------------------------------
def contract_fp32(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, T) -> torch.Tensor:
    """The contract in fp32 on the CPU: per 128-k block an fp32 dot product, its scale, an fp32 running sum in block
    order; one rounding to T.  (The order inside a block is torch's, not the MFMA's: a restatement for tolerances.)"""
    xf, qf = x.to(T).float(), q.view(FP8).float()
    acc = torch.zeros((x.shape[0], q.shape[0]), dtype=torch.float32)
    for b in range(q.shape[1] // BLK):
        part = xf[:, b * BLK:(b + 1) * BLK] @ qf[:, b * BLK:(b + 1) * BLK].t()
        acc = torch.addcmul(acc, part, scale[:, b].repeat_interleave(BLK)[None, :])
    return acc.to(T)


def rounded_weight_product(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, T) -> torch.Tensor:
    """The mutant of the random-input test: the float64 product over T(q * s)."""
    return x.to(T).double() @ F8.dequant(q, scale).to(T).double().t()


def tolerance(ref: torch.Tensor, T) -> torch.Tensor:
    """tests/test_gpu_ops.py::test_linear_decode_matches_fp32_reference's: 2^-7 (bf16) / 2^-10 (fp16) x max(|ref|, 0.05)."""
    return (2.0 ** -7 if T == torch.bfloat16 else 2.0 ** -10) * ref.abs().clamp_min(0.05)


# ---------------------------------------------------------------------------------------------------------------------
def published_full(sd, quantize):
    """A reference-named state dict in the fully published format: every ..._proj.weight (attention, dense MLP, routed and
    shared experts) float8_e4m3fn with ...weight_scale_inv beside it (quantize: hydrainfer_amd's quantize_fp8_block);
    embeddings, lm_head, norms and the router (mlp.gate.weight) as they are."""
    out = {}
    for k, v in sd.items():
        if k.endswith("_proj.weight"):
            q, s = quantize(v)
            out[k], out[k[:-len("weight")] + "weight_scale_inv"] = q, s
        else:
            out[k] = v
    return out
