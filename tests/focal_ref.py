"""Torch restatement of focal image-token pruning (test infrastructure; runs on CPU or GPU tensors).

The rule (per image; N patch tokens after `skip_leading` leading tokens are dropped from rows and columns, H heads, head dim
D, scale = 1 / sqrt(D)) — this restatement MATERIALISES the scores the way the reference's attention fallback does:

    S_h[i, j] = (float(q[i, h, :]) * scale) . float(k[j, h, :])          fp32 bmm (fp64 in the float64 variant)
    A         = mean_h S_h
    s1[j]     = mean_i A[i, j]          s2[i] = mean_j A[i, j]
    sig       = s1 if var(s1) > var(s2) else s2                          torch.var: unbiased
    'rank'    : keep the n tokens of largest sig
    'row'     : g = sqrt(N); r[y] = sum of sig over grid row y; keep all tokens of the n / g rows of largest r
    output    = tokens[ascending sorted kept ids, :]

Exact ties go to the lower index (a STABLE descending sort); 'row' needs n % g == 0; 1 <= n <= N."""
import math
from typing import List, Sequence, Tuple, Union

import torch
from torch import Tensor


def scores(q: Tensor, k: Tensor, skip_leading: int = 0, dtype: torch.dtype = torch.float32) -> Tensor:
    """q, k [B, T, H, D] -> S [B, H, N, N] in `dtype` (float32: the reference's arithmetic; float64: the yardstick)."""
    D = q.shape[-1]
    scale = 1.0 / math.sqrt(D)
    qs = q[:, skip_leading:].to(dtype).transpose(1, 2) * scale
    ks = k[:, skip_leading:].to(dtype).transpose(1, 2)
    return torch.matmul(qs, ks.transpose(-1, -2))


def significance_from_scores(S: Tensor) -> Tuple[Tensor, Tensor]:
    """S [B, H, N, N] -> (s1, s2) [B, N]."""
    A = S.mean(dim=1)
    return A.mean(dim=1), A.mean(dim=2)


def significance(q: Tensor, k: Tensor, skip_leading: int = 0, dtype: torch.dtype = torch.float32) -> Tuple[Tensor, Tensor]:
    return significance_from_scores(scores(q, k, skip_leading, dtype))


def choose(s1: Tensor, s2: Tensor) -> Tensor:
    """One image: the significance vector the rule ranks by."""
    return s1 if torch.var(s1).item() > torch.var(s2).item() else s2


def select_one(s1: Tensor, s2: Tensor, n: int, strategy: str) -> Tensor:
    """One image: the ascending kept ids (int64)."""
    N = s1.shape[0]
    assert 1 <= n <= N
    sig = choose(s1, s2)
    if strategy == "rank":
        order = torch.sort(sig, descending=True, stable=True).indices
        kept = order[:n]
    else:
        assert strategy == "row"
        g = math.isqrt(N)
        assert g * g == N and n % g == 0
        r = sig.reshape(g, g).sum(dim=-1)
        rows = torch.sort(r, descending=True, stable=True).indices[: n // g]
        kept = torch.arange(N, device=sig.device).reshape(g, g)[rows].reshape(-1)
    return torch.sort(kept).values


def select(s1: Tensor, s2: Tensor, n: Union[int, Sequence[int]], strategy: str) -> List[Tensor]:
    B = s1.shape[0]
    counts = [n] * B if isinstance(n, int) else list(n)
    return [select_one(s1[b], s2[b], counts[b], strategy) for b in range(B)]


def padded_ids(ids: List[Tensor], N: int) -> Tensor:
    """The kernel's id layout: int32 [B, N], the kept ids first, -1 behind them."""
    out = torch.full((len(ids), N), -1, dtype=torch.int32)
    for b, t in enumerate(ids):
        out[b, : t.numel()] = t.to(torch.int32).cpu()
    return out


def cut_gap(s1: Tensor, s2: Tensor, n: int) -> float:
    """One image, 'rank': the gap between the n-th and the (n+1)-th largest significance (inf when n == N)."""
    sig = torch.sort(choose(s1, s2), descending=True).values
    return float("inf") if n >= sig.numel() else (sig[n - 1] - sig[n]).item()


def focal_prunning(tokens: Tensor, q: Tensor, k: Tensor, n: Union[int, Sequence[int]], strategy: str, skip_leading: int = 0,
                   dtype: torch.dtype = torch.float32) -> Tuple[List[Tensor], List[Tensor]]:
    """(kept rows per image, kept ids per image)."""
    s1, s2 = significance(q, k, skip_leading, dtype)
    ids = select(s1, s2, n, strategy)
    return [tokens[b, ids[b]] for b in range(tokens.shape[0])], ids
