"""The reference the processed-logprob tests measure against (include/hydra_hip.h: hx_sample_rows_logprobs), on the CPU.
tests/constraint_ref.py / sampling_ref.py / penalty_ref.py give a row's z = s / T' bit for bit as fp32 (`row_z`);
`reference_logprobs` is the float64 log-softmax of that z over the kept set S and the K first indices in the order
(larger z, then lower index) — a two-key sort, as in tests/logprob_ref.py, whose ATOL and assert_logprobs_close hold the
kernel's fp32 results to it."""
import math

import numpy as np
import torch

from tests import constraint_ref as cref
from tests import sampling_ref as ref


def row_z(x: torch.Tensor, bias, hist, penalties, record) -> np.ndarray:
    """fp32 [n]: the z of one row of a launch — x: the row's 16-bit logits, bias: None or (ids, values), hist: None or a
    PenaltyHistory, record: (temperature, ...).  A greedy row (temperature not > 0) is scaled by T' = 1."""
    b_ids, b_values = ([], []) if bias is None else (np.asarray(bias[0]).tolist(), np.asarray(bias[1]).tolist())
    xb = cref.biased_row(x, b_ids, b_values)
    t = record[0] if record[0] > 0 else 1.0
    return ref.scaled_row(xb, list(hist.ids) if hist else [], list(hist.counts) if hist else [], penalties, t)[1].numpy()


def reference_logprobs(z: np.ndarray, cut, top_k: int):
    """z: fp32 [n] without a NaN and with a finite maximum; cut: the sampled row's v* (S = {z >= cut}), None for a greedy
    row (S: everything).  Returns (lp float64 [n]: the log-softmax of z over S, -inf outside; top_ids int64 [top_k];
    top_lp float64 [top_k]); entries past n: id -1, -inf."""
    assert z.dtype == np.float32 and z.ndim == 1 and not np.isnan(z).any() and math.isfinite(float(z.max()))
    n = z.size
    z64 = z.astype(np.float64)
    kept = np.ones(n, dtype=bool) if cut is None else z >= np.float32(cut)
    assert kept.any(), "the kept set is empty"
    m = z64.max()
    with np.errstate(divide="ignore"):
        lp = np.where(kept, (z64 - m) - math.log(np.exp(z64[kept] - m).sum()), -math.inf)
    order = np.lexsort((np.arange(n), -z64))[:top_k]              # last key first: z descending, then index ascending
    top_ids = np.full(top_k, -1, dtype=np.int64)
    top_lp = np.full(top_k, -math.inf)
    top_ids[:len(order)] = order
    top_lp[:len(order)] = lp[order]
    return lp, top_ids, top_lp
