"""fp32 torch restatement of attention with ALiBi slopes, for tests/test_alibi_cpu.py and tests/test_gpu_alibi.py
(test infrastructure only; oracle/ops.py::_attend has no ALiBi and stays as it is).

ALiBi is NOT in the reference's torch handlers, so parity is unpinned for it — like softcap and windows in `_attend`,
this restates the CUDA kernel's semantics (flash_api.cpp:197-214, mask.h:112-190, alibi.h): for sequence b, head h, query
row i of lq rows and key j of lk keys

    score(i, j) = f(q_i . k_j * softmax_scale) - slope[b, h] * |i + lk - lq - j|

with f the soft cap `softcap * tanh(x / softcap)` or the identity.  The bias is added AFTER the cap (the reference
divides the slope by its scale_softmax, which is the cap when one is set: flash_fwd_kernel.h:244) and BEFORE the masks.
Under a causal mask the reference adds slope * j instead (mask.h:157-158): a constant per row apart, the same softmax.
Rows that see no key give zeros."""
from typing import List, Optional

import torch
from torch import Tensor


def attend_alibi(q: Tensor, k: Tensor, v: Tensor, sm_scale: float, causal: bool, slopes: Optional[Tensor],
                 softcap: float = 0.0, window: Optional[tuple] = None) -> Tensor:
    """q [Lq, H, D]; k, v [Lk, HK, D]; slopes fp32 [H] or None.  Everything in fp32."""
    q, k, v = q.float(), k.float(), v.float()
    group = q.shape[1] // k.shape[1]
    k = k.repeat_interleave(group, dim=1)
    v = v.repeat_interleave(group, dim=1)
    scores = torch.einsum("qhd,khd->hqk", q, k) * sm_scale
    if softcap > 0:
        scores = softcap * torch.tanh(scores / softcap)
    lq, lk = q.shape[0], k.shape[0]
    x = torch.arange(lk)[None, None, :]
    y = torch.arange(lq)[None, :, None]
    if slopes is not None:
        scores = scores - slopes.float()[:, None, None] * (y + (lk - lq) - x).abs().float()
    if causal:
        scores = scores.masked_fill((x - y) > (lk - lq), float("-inf"))
    if window is not None and (window[0] >= 0 or window[1] >= 0):
        left = window[0] if window[0] >= 0 else lk
        right = window[1] if window[1] >= 0 else lk
        d = x - y - (lk - lq)
        scores = scores.masked_fill((d > right) | (d < -left), float("-inf"))
    p = torch.softmax(scores, dim=-1)
    p = torch.nan_to_num(p, nan=0.0)
    return torch.einsum("hqk,khd->qhd", p, v)


def _slopes_of(slopes: Optional[Tensor], b: int) -> Optional[Tensor]:
    if slopes is None:
        return None
    return slopes[b] if slopes.dim() == 2 else slopes


def paged_attention_alibi(q: Tensor, kc: Tensor, vc: Tensor, cu_q: Tensor, cu_k: Tensor, block_table: Tensor,
                          cu_blocks: Tensor, slopes: Optional[Tensor], causal: bool = True, softcap: float = 0.0,
                          window: Optional[tuple] = None) -> Tensor:
    """Paged form: kc, vc [n_blocks, block_size, HK, D]; flat block table.  slopes [H] or [batch, H].  Returns fp32."""
    bs = kc.shape[1]
    out = torch.zeros(q.shape, dtype=torch.float32)
    for b in range(cu_q.numel() - 1):
        q0, q1 = int(cu_q[b]), int(cu_q[b + 1])
        lk = int(cu_k[b + 1]) - int(cu_k[b])
        pages = block_table[int(cu_blocks[b]): int(cu_blocks[b + 1])].long()
        k = kc[pages].reshape(-1, *kc.shape[2:])[:lk]
        v = vc[pages].reshape(-1, *vc.shape[2:])[:lk]
        assert k.shape[0] == lk and pages.numel() == (lk + bs - 1) // bs
        out[q0:q1] = attend_alibi(q[q0:q1], k, v, 1.0 / q.shape[-1] ** 0.5, causal, _slopes_of(slopes, b), softcap, window)
    return out


def dense_attention_alibi(q: Tensor, k: Tensor, v: Tensor, cu_q: Tensor, cu_k: Tensor, slopes: Optional[Tensor],
                          causal: bool = False, softcap: float = 0.0, window: Optional[tuple] = None) -> Tensor:
    out = torch.zeros(q.shape, dtype=torch.float32)
    for b in range(cu_q.numel() - 1):
        q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
        out[q0:q1] = attend_alibi(q[q0:q1], k[k0:k1], v[k0:k1], 1.0 / q.shape[-1] ** 0.5, causal, _slopes_of(slopes, b),
                                  softcap, window)
    return out


def closed_form_q0(v: Tensor, slopes: Tensor) -> Tensor:
    """With q = 0 every dot product vanishes: head h's output over keys 0..lk-1 is sum_j w_j v_j with
    w_j ~ exp(-slope_h * (lk - 1 - j)).  Worked out directly in float64, independent of attend_alibi.
    v [lk, H, D]; slopes [H] -> [H, D] float64."""
    lk = v.shape[0]
    dist = torch.arange(lk - 1, -1, -1, dtype=torch.float64)                  # lk - 1 - j
    w = torch.exp(-slopes.double()[:, None] * dist[None, :])                   # [H, lk]
    w = w / w.sum(dim=1, keepdim=True)
    return torch.einsum("hj,jhd->hd", w, v.double())


def random_paged(batch: int, H: int, HK: int, D: int, kv_lens: List[int], q_lens: List[int], dt, block_size: int = 16,
                 seed: int = 0, extra_blocks: int = 7):
    """Random q, a shuffled paged cache and the control arrays (CPU tensors)."""
    g = torch.Generator().manual_seed(seed)
    n_blocks = sum((l + block_size - 1) // block_size for l in kv_lens) + extra_blocks
    kc = torch.randn((n_blocks, block_size, HK, D), generator=g).to(dt)
    vc = torch.randn((n_blocks, block_size, HK, D), generator=g).to(dt)
    perm = torch.randperm(n_blocks, generator=g).tolist()
    tables, cu_b, cu_q, cu_k, used = [], [0], [0], [0], 0
    for ql, kl in zip(q_lens, kv_lens):
        nb = (kl + block_size - 1) // block_size
        tables += perm[used: used + nb]
        used += nb
        cu_b.append(cu_b[-1] + nb)
        cu_q.append(cu_q[-1] + ql)
        cu_k.append(cu_k[-1] + kl)
    q = torch.randn((cu_q[-1], H, D), generator=g).to(dt)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    return q, kc, vc, i32(cu_q), i32(cu_k), i32(tables), i32(cu_b)


def ragged_lens(batch: int, lo: int, hi: int, seed: int) -> List[int]:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (batch,), generator=g).tolist()


# the first GPU case of tests/test_gpu_alibi.py (the one that must fail without the feature): shared with the CPU test
# that shows, on the restatement alone, that ignoring the slopes cannot pass it
FIRST_CASE = dict(batch=8, H=32, HK=32, D=128, lo=1, hi=1000, seed=20)
