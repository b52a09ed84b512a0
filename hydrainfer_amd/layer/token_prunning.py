"""Focal image-token pruning — hydrainfer/layer/token_prunning.py:5-37 (the module keeps the reference's name and
spelling) on the HIP path.

The rule keeps, per image, the `n` tokens of largest significance, where the significance is the column mean (token as a
key, s1) or the row mean (token as a query, s2) of the head-averaged attention scores, whichever has the larger variance.
The scores the reference hands to it are the PRE-softmax scaled logits (multihead_attention.py:59-62), so both means are
linear in q and k and `focal_prunning_qk` gets them without the [B, H, N, N] tensor (hx_focal_significance); the selection
(hx_focal_select) and the gather (hx_focal_gather) stay on the device, with no host synchronisation: the whole path
captures into a hipGraph.  `focal_prunning` keeps the reference's signature over materialised scores.

Defined here where the reference leaves it open: exact ties go to the lower index; 'row' needs a square token count and
n a multiple of its root; 1 <= n <= N; n == N returns the tokens unchanged."""
import math
from typing import Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from hydrainfer_amd import _lib

_STRATEGY = {"rank": _lib.HX_FOCAL_RANK, "row": _lib.HX_FOCAL_ROW}


def _strategy_code(strategy: str) -> int:
    try:
        return _STRATEGY[strategy]
    except KeyError:
        raise ValueError(f"focal pruning strategy {strategy!r}: 'rank' or 'row'")


def check_counts(counts: Sequence[int], n_tokens: int, strategy: str) -> None:
    """The limits on host-known counts (the kernels clamp; they cannot raise)."""
    _strategy_code(strategy)
    g = math.isqrt(n_tokens)
    if strategy == "row" and g * g != n_tokens:
        raise ValueError(f"strategy 'row': {n_tokens} tokens are not a square grid")
    for n in counts:
        if not 1 <= n <= n_tokens:
            raise ValueError(f"n_output_tokens {n} outside 1..{n_tokens}")
        if strategy == "row" and n % g != 0:
            raise ValueError(f"strategy 'row': n_output_tokens {n} is not a multiple of the grid side {g}")


def keep_counts(n_output_tokens: Union[int, Sequence[int], Tensor], n_images: int, n_tokens: int, strategy: str,
                device) -> Tuple[Tensor, Optional[int]]:
    """(int32 device tensor [n_images], largest count or None when only the device knows).  A device tensor is taken as it
    is — no synchronisation, so its content cannot be checked: the kernels clamp it to 0..N."""
    if isinstance(n_output_tokens, Tensor) and n_output_tokens.is_cuda:
        if n_output_tokens.dtype != torch.int32 or n_output_tokens.shape != (n_images,) or not n_output_tokens.is_contiguous():
            raise ValueError("n_output_tokens on the device: a contiguous int32 tensor [n_images]")
        _strategy_code(strategy)
        return n_output_tokens, None
    if isinstance(n_output_tokens, Tensor):
        n_output_tokens = n_output_tokens.tolist()
    counts = [int(n_output_tokens)] * n_images if isinstance(n_output_tokens, int) else [int(n) for n in n_output_tokens]
    if len(counts) != n_images:
        raise ValueError(f"{len(counts)} counts for {n_images} images")
    check_counts(counts, n_tokens, strategy)
    t = torch.tensor(counts, dtype=torch.int32)
    if torch.device(device).type == "cuda":
        t = t.pin_memory().to(device, non_blocking=True)
    return t, max(counts) if counts else 0


def focal_significance(q: Tensor, k: Tensor, n_images: int, tokens_per_image: int, n_heads: int, head_dim: int,
                       skip_leading: int = 0, scale: Optional[float] = None) -> Tuple[Tensor, Tensor]:
    """(s1, s2), fp32 [n_images, tokens_per_image - skip_leading], from q and k [n_images * tokens_per_image, n_heads *
    head_dim] (any row stride: views of a fused qkv product)."""
    _lib.require_gpu(q, k)
    q2 = q.reshape(n_images * tokens_per_image, -1) if q.dim() != 2 else q
    k2 = k.reshape(n_images * tokens_per_image, -1) if k.dim() != 2 else k
    width = n_heads * head_dim
    if q2.shape != (n_images * tokens_per_image, width) or k2.shape != q2.shape or q2.dtype != k2.dtype:
        raise _lib.HydraHipError(f"focal_significance: q {tuple(q.shape)} / k {tuple(k.shape)} are not "
                                 f"[{n_images} * {tokens_per_image}, {n_heads} * {head_dim}] of one dtype")
    if q2.stride(1) != 1 or k2.stride(1) != 1:
        raise _lib.HydraHipError("focal_significance: heads and head dim must be contiguous")
    n = tokens_per_image - skip_leading
    l = _lib.lib()
    s = torch.empty((2, n_images, n), dtype=torch.float32, device=q.device)
    ws_bytes = l.hx_focal_significance_workspace_bytes(n_images, n_heads, head_dim)
    ws = torch.empty((max(ws_bytes, 4) // 4,), dtype=torch.float32, device=q.device)
    _lib.check(l.hx_focal_significance(s[0].data_ptr(), s[1].data_ptr(), q2.data_ptr(), k2.data_ptr(), n_images,
                                       tokens_per_image, skip_leading, n_heads, head_dim, q2.stride(0), k2.stride(0),
                                       scale if scale is not None else 1.0 / math.sqrt(head_dim), ws.data_ptr(), ws_bytes,
                                       _lib.dtype_code(q2), _lib.current_stream()), "focal_significance")
    return s[0], s[1]


def focal_select(s1: Tensor, s2: Tensor, n_keep: Tensor, strategy: str = "rank") -> Tensor:
    """ids int32 [n_images, N]: the kept ids of image b ascending in the first n_keep[b] entries, -1 behind them."""
    _lib.require_gpu(s1, s2, n_keep)
    if s1.dim() != 2 or s1.shape != s2.shape or s1.dtype != torch.float32 or s2.dtype != torch.float32:
        raise _lib.HydraHipError("focal_select: s1, s2 are fp32 [n_images, N]")
    if n_keep.dtype != torch.int32 or n_keep.shape != (s1.shape[0],):
        raise _lib.HydraHipError("focal_select: n_keep is int32 [n_images]")
    s1, s2, n_keep = (t if t.is_contiguous() else t.contiguous() for t in (s1, s2, n_keep))
    ids = torch.empty(s1.shape, dtype=torch.int32, device=s1.device)
    _lib.check(_lib.lib().hx_focal_select(ids.data_ptr(), s1.data_ptr(), s2.data_ptr(), n_keep.data_ptr(), s1.shape[0],
                                          s1.shape[1], _strategy_code(strategy), _lib.current_stream()), "focal_select")
    return ids


def focal_gather(tokens: Tensor, ids: Tensor, n_keep: Tensor) -> Tensor:
    """out [B, N, hidden] with out[b, r] = tokens[b, ids[b, r]] for r < n_keep[b]; the rows behind are left unwritten."""
    _lib.require_gpu(tokens, ids, n_keep)
    if tokens.dim() != 3 or ids.shape != tokens.shape[:2] or ids.dtype != torch.int32 or not ids.is_contiguous():
        raise _lib.HydraHipError("focal_gather: tokens [B, N, hidden], ids int32 [B, N]")
    B, N, hidden = tokens.shape
    if tokens.stride(2) != 1 or (B > 1 and tokens.stride(0) != N * tokens.stride(1)):
        tokens = tokens.contiguous()
    out = torch.empty((B, N, hidden), dtype=tokens.dtype, device=tokens.device)
    _lib.check(_lib.lib().hx_focal_gather(out.data_ptr(), tokens.data_ptr(), ids.data_ptr(), n_keep.data_ptr(), B, N, hidden,
                                          tokens.stride(1), hidden, _lib.dtype_code(tokens), _lib.current_stream()),
               "focal_gather")
    return out


def focal_prunning_qk(tokens: Tensor, q: Tensor, k: Tensor, n_output_tokens, strategy: str = "rank", skip_leading: int = 0,
                      n_heads: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The fused path.  tokens [B, N, hidden]; q, k [B, N + skip_leading, n_heads, head_dim] (or [B, N + skip_leading,
    n_heads * head_dim] with n_heads given) of the attention whose scores rank the tokens; n_output_tokens an int, a
    per-image list / host tensor, or an int32 device tensor [B].  Returns (pruned [B, max n, hidden] — image b's kept
    tokens in its first n_b rows, the rows behind them unwritten; max n = N when only the device knows the counts —,
    ids int32 [B, N], -1 behind the kept ones)."""
    B, N, _ = tokens.shape
    if q.dim() == 4:
        n_heads, head_dim = q.shape[2], q.shape[3]
        q, k = q.flatten(2), k.flatten(2)
    elif n_heads is None:
        raise ValueError("q, k without a head axis need n_heads")
    else:
        head_dim = q.shape[-1] // n_heads
    if q.shape[0] != B or q.shape[1] != N + skip_leading:
        raise ValueError(f"q {tuple(q.shape)} does not belong to tokens {tuple(tokens.shape)} with skip_leading = {skip_leading}")
    n_keep, n_max = keep_counts(n_output_tokens, B, N, strategy, tokens.device)
    s1, s2 = focal_significance(q.reshape(B * (N + skip_leading), -1), k.reshape(B * (N + skip_leading), -1), B,
                                N + skip_leading, n_heads, head_dim, skip_leading)
    ids = focal_select(s1, s2, n_keep, strategy)
    out = focal_gather(tokens, ids, n_keep)
    return (out if n_max is None else out[:, :n_max]), ids


def focal_prunning(tokens: Tensor, scores: Tensor, n_output_tokens: int, strategy: str) -> Tensor:
    """token_prunning.py:5-37 with the reference's signature: tokens [B, N, hidden], materialised scores [B, H, N, N].
    The two means are torch reductions (plumbing: the tensor exists already); selection and gather are the HIP launches."""
    assert tokens.dim() == 3 and scores.dim() == 4
    B, N, _ = tokens.shape
    assert scores.shape[0] == B and scores.shape[2] == N and scores.shape[3] == N
    n_keep, n_max = keep_counts(n_output_tokens, B, N, strategy, tokens.device)
    a = scores.float().mean(dim=1)
    ids = focal_select(a.mean(dim=1), a.mean(dim=2), n_keep, strategy)
    return focal_gather(tokens, ids, n_keep)[:, :n_max]
