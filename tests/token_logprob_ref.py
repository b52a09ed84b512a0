"""Reference for the prompt log-probability tests (test_gpu_token_logprobs.py, test_gpu_prompt_logprobs_engine.py,
test_prompt_logprobs_cpu.py): tests/logprob_ref.reference for the top lists, the float64 log-softmax of the SAME 16-bit
logits gathered at the given ids, and the rank from the same two-key sort — a NaN in front of every number, value
descending, index ascending: the rank of token t is its position in that order, an integer with one answer even in rows
full of exact ties."""
import math

import numpy as np
import torch

from tests.logprob_ref import ATOL, assert_logprobs_close, reference  # noqa: F401  (re-exported for the tests)


def token_reference(logits: torch.Tensor, targets, top_k: int):
    """(logprobs float64 [rows], ranks int64 [rows], top_ids int64 [rows, K], top_logprobs float64 [rows, K]) of a
    [rows, n] tensor of any float dtype and one id per row; a row whose id is outside 0..n-1 is not scored: NaN, -1,
    ids -1, -inf."""
    x = logits.detach().cpu().to(torch.float64)
    rows, n = x.shape
    t = torch.as_tensor(targets, dtype=torch.int64).reshape(rows)
    scored = (t >= 0) & (t < n)
    _, _, top_ids, top_lp = reference(x, top_k)
    lsm = torch.log_softmax(x, dim=-1)
    lp = lsm.gather(1, t.clamp(0, n - 1)[:, None])[:, 0]
    v = x.numpy()
    nan = np.isnan(v)
    key = np.where(nan, 0.0, v)
    idx = np.arange(n)
    ranks = torch.full((rows,), -1, dtype=torch.int64)
    for r in range(rows):
        if bool(scored[r]):
            order = np.lexsort((idx, -key[r], ~nan[r]))           # the key of logprob_ref.reference
            ranks[r] = int(np.nonzero(order == int(t[r]))[0][0])
    lp = torch.where(scored, lp, torch.full_like(lp, math.nan))
    top_ids = torch.where(scored[:, None], top_ids, torch.full_like(top_ids, -1))
    top_lp = torch.where(scored[:, None], top_lp, torch.full_like(top_lp, -math.inf))
    return lp, ranks, top_ids, top_lp


def self_test():
    """A row of exact ties: the rank of index i among equal values is i; a larger value in front of them all; a NaN in
    front of that."""
    x = torch.full((1, 9), 1.5, dtype=torch.float16)
    for i in (0, 4, 8):
        lp, rk, top_ids, top_lp = token_reference(x, [i], 3)
        assert int(rk[0]) == i and abs(float(lp[0]) + math.log(9)) < 1e-12 and top_ids[0].tolist() == [0, 1, 2]
    x[0, 6] = 2.0
    assert int(token_reference(x, [6], 0)[1][0]) == 0 and int(token_reference(x, [0], 0)[1][0]) == 1
    assert int(token_reference(x, [7], 0)[1][0]) == 7       # 6 in front, then 0..5
    x[0, 8] = math.nan
    lp, rk, _, _ = token_reference(x, [8], 0)
    assert int(rk[0]) == 0 and math.isnan(float(lp[0])) and int(token_reference(x, [6], 0)[1][0]) == 1
    lp, rk, top_ids, top_lp = token_reference(x, [9], 2)    # outside: not scored
    assert math.isnan(float(lp[0])) and int(rk[0]) == -1 and top_ids[0].tolist() == [-1, -1]
    assert top_lp[0].tolist() == [-math.inf, -math.inf]
