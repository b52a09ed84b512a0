"""W8A8 (csrc/gemm_fp8a.hip) restated in pure torch on the CPU, for tests/test_gpu_linear_fp8a.py.  Builds on
tests/gemm_exact.py, tests/moe_fp8_ref.py and tests/linear_fp8_ref.py, which it does not change.

THE CONTRACT (include/hydra_hip.h): hx_quant_fp8_group gives, per (row, 128-k group), s = max(amax |x|, 1e-10) / 448 and
q = e4m3_rne(clamp(x / s, -448, 448)); hx_linear_fp8a gives
    out[m][n] = T( sum over 128-k blocks b of (xs[m][b] * ws[n / 128][b]) * ( sum_{k in b} xq[m][k] * wq[n][k] ) ).

EXACT ROWS (exact_rows): linear_fp8_ref.exact_case's weight with its x turned into bytes: row m is the case's row
(m + m // 64) % 64 — rows 64 apart differ — divided by the power-of-two scale 2^((m + 2 b) % 4 - 1) of its (row, group), so
neighbouring rows and neighbouring groups have different scales and a row or group met with another's is off by a power
of two.  x bytes are multiples of 1/16 up to 7.5, weight bytes multiples of 1/16 up to 15: a block's sum stays below 2^24
quanta (asserted), every scale product is a power of two and the scaled running sums are exact_case's (asserted there), so
every fp32 sum is exact in any order and the answer is the float64 product rounded once."""
import torch

from tests import gemm_exact as G
from tests import linear_fp8_ref as L8
from tests import moe_fp8_ref as F8

FP8, BLK = F8.FP8, F8.BLK


def quant_group(x: torch.Tensor):
    """(uint8 bytes [M, K], fp32 scales [M, K / 128]) of x: the contract's expression, in fp32."""
    M, K = x.shape
    g = x.float().view(M, K // BLK, BLK)
    s = g.abs().amax(dim=-1).clamp(min=1e-10) / 448.0
    return (g / s[..., None]).clamp(-448, 448).to(FP8).view(torch.uint8).view(M, K), s


def dequant_rows(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """float64 [M, K]: float(q) * s of its (row, group)."""
    return q.view(FP8).double() * s.double().repeat_interleave(BLK, dim=1)


def exact_rows(c: L8.ExactCase, M: int):
    """(bytes [M, K], scales [M, K / 128], float64 answer [M, N]) of M rows over exact_case c."""
    K = c.x.shape[1]
    m = torch.arange(M)
    rows = (m + m // L8.MAX_ROWS) % L8.MAX_ROWS
    s = 2.0 ** ((m[:, None] + 2 * torch.arange(K // BLK)[None, :]) % 4 - 1).float()
    G.assert_exact(BLK, G.LEVELS * G.STEP / 0.5, G.LEVELS * G.STEP / min(F8.PAIRING_SCALES), (G.STEP / 4) * (G.STEP / max(F8.PAIRING_SCALES)))
    return F8.to_bytes(c.x[rows] / s.repeat_interleave(BLK, dim=1)), s, c.ref[rows]


PROBE_X = 1.5                                # the one nonzero activation of a probe row (byte 0x3C)


def probe_weight(N: int, K: int) -> torch.Tensor:
    """uint8 [N, K]: row n holds the 252 finite nonzero e4m3 bytes in order, rotated by 7 n — distinct over any 252
    consecutive k, so the product of row m (one-hot at k = m) names the k the kernel paired it with."""
    table = torch.tensor([b for b in range(256) if b & 0x7F not in (0, 0x7F)], dtype=torch.uint8)
    return table[(torch.arange(K)[None, :] + 7 * torch.arange(N)[:, None]) % table.numel()]
