"""The reference the penalty tests measure against: steps 1-2 of the reference's process_logits
(hydrainfer/sampling/logits_processor.py:65-72) restated in torch fp32, one row at a time, and the argmax under the
kernel's order (a NaN first, then the larger value, then the lower index).  tests/golden/g14_penalties.npz holds what the
reference's own function gave for a few dozen rows; test_penalties_cpu.py holds this file to it exactly."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_penalties.npz")


def penalized_scores(x: torch.Tensor, ids, counts, f: float, p: float, r: float) -> torch.Tensor:
    """fp32 [len(ids)]: the penalised values of the entries (ids, counts) of one row; x: the row as fp32.  Every
    operation is a separate fp32 torch op, in the reference's order."""
    ids = torch.as_tensor(ids, dtype=torch.int64)
    counts = torch.as_tensor(counts, dtype=torch.int32)
    f, p, r = (torch.tensor(v, dtype=torch.float32) for v in (f, p, r))
    score = x.float()[ids].clone()
    score = score - counts * f
    score = score - (counts > 0) * p
    return torch.where(score < 0, score * r, score / r)


def argmax_in_order(row: torch.Tensor) -> int:
    """The first element of an fp32 row under (NaN first, larger value, lower index)."""
    nan = torch.isnan(row)
    if bool(nan.any()):
        return int(torch.nonzero(nan)[0])
    return int(torch.nonzero(row == row.max())[0])


def penalized_row(x: torch.Tensor, ids, counts, f: float, p: float, r: float):
    """(penalised fp32 row, scores of the entries, greedy id).  Entries whose id lies outside the row are ignored: their
    score is NaN, as the kernel reports them."""
    row = x.float().clone()
    ids_t = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
    counts_t = torch.as_tensor(counts, dtype=torch.int32).reshape(-1)
    ok = (ids_t >= 0) & (ids_t < row.numel())
    scores = torch.full((ids_t.numel(),), float("nan"), dtype=torch.float32)
    if bool(ok.any()):
        scores[ok] = penalized_scores(row, ids_t[ok], counts_t[ok], f, p, r)
        row[ids_t[ok]] = scores[ok]
    return row, scores, argmax_in_order(row)


def penalized_batch(logits: torch.Tensor, hist_ids, hist_counts, cu_hist, penalties):
    """(ids int64 [rows], scores fp32 [total]) for a CSR batch, row by row."""
    hist_ids, hist_counts, cu = (torch.as_tensor(t).reshape(-1).tolist() for t in (hist_ids, hist_counts, cu_hist))
    pen = torch.as_tensor(penalties, dtype=torch.float32).reshape(-1, 3).tolist()
    out, scores = [], []
    for r in range(logits.shape[0]):
        a, b = cu[r], cu[r + 1]
        _, s, i = penalized_row(logits[r], hist_ids[a:b], hist_counts[a:b], *pen[r])
        out.append(i)
        scores.append(s)
    return torch.tensor(out, dtype=torch.int64), torch.cat(scores) if scores else torch.zeros(0)


def bf16_from_bits(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits.astype(np.int32) << 16).view(torch.float32).to(torch.bfloat16)


def load_golden():
    """The fixture as a list of rows: dict(n, logits bf16 [n], ids, counts, penalties (f, p, r), scores fp32 (the
    reference's penalised history entries), best (the reference row's argmax in the kernel's order), max (its value))."""
    z = np.load(GOLDEN)
    rows, lo, ho = [], 0, 0
    for r, n in enumerate(z["n"].tolist()):
        h = int(z["hist_len"][r])
        rows.append(dict(n=n, logits=bf16_from_bits(z["logits_bits"][lo:lo + n]),
                         ids=z["hist_ids"][ho:ho + h].tolist(), counts=z["hist_counts"][ho:ho + h].tolist(),
                         penalties=tuple(float(v) for v in z["penalties"][r]),
                         scores=torch.from_numpy(z["scores"][ho:ho + h].copy()),
                         best=int(z["argmax"][r]), max=float(z["max"][r]), raw_best=int(z["raw_argmax"][r])))
        lo, ho = lo + n, ho + h
    return rows
