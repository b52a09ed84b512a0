"""Reference for the per-token log-probability tests (test_gpu_logprobs*.py, test_logprobs_cpu.py): float64
log-softmax on the CPU of the SAME 16-bit logits the kernel read, and the top-K order by a two-key sort — value
descending (a NaN in front of every number, as torch.argmax ranks it), then index ascending.  torch.topk leaves the
order of equal values open, so it is no oracle for rows of 16-bit logits, which are full of exact ties."""
import math

import numpy as np
import torch

ATOL = 1e-4     # fp32 sum of <= 1e5 terms in (0, 1] (~1e-5 relative, so ~1e-5 in the log) + the fp32 result's rounding


def reference(logits: torch.Tensor, top_k: int):
    """(ids int64 [rows], logprobs float64 [rows], top_ids int64 [rows, K], top_logprobs float64 [rows, K]) of a
    [rows, n] tensor of any float dtype; entries past n: id -1, logprob -inf."""
    x = logits.detach().cpu().to(torch.float64)
    rows, n = x.shape
    lsm = torch.log_softmax(x, dim=-1).numpy()
    v = x.numpy()
    nan = np.isnan(v)
    key = np.where(nan, 0.0, v)
    idx = np.broadcast_to(np.arange(n), v.shape)
    k = max(top_k, 1)
    top_ids = np.full((rows, k), -1, dtype=np.int64)
    top_lp = np.full((rows, k), -math.inf)
    for r in range(rows):
        order = np.lexsort((idx[r], -key[r], ~nan[r]))[:k]        # last key first: NaNs, then value desc, then index asc
        top_ids[r, :len(order)] = order
        top_lp[r, :len(order)] = lsm[r, order]
    return (torch.from_numpy(top_ids[:, 0].copy()), torch.from_numpy(top_lp[:, 0].copy()),
            torch.from_numpy(top_ids[:, :top_k].copy()), torch.from_numpy(top_lp[:, :top_k].copy()))


def assert_logprobs_close(got: torch.Tensor, want: torch.Tensor, what: str = "", atol: float = ATOL) -> float:
    """got (fp32, any device) against want (float64): within atol where want is finite, -inf where it is -inf, NaN
    where it is NaN.  Returns the largest finite error."""
    got, want = got.detach().cpu().to(torch.float64).reshape(-1), want.reshape(-1)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    nan, ninf = torch.isnan(want), want == -math.inf
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN logprobs differ from the reference's"
    assert torch.equal(got == -math.inf, ninf), f"{what}: -inf logprobs differ from the reference's"
    fin = ~(nan | ninf)
    err = float((got[fin] - want[fin]).abs().max()) if bool(fin.any()) else 0.0
    assert err <= atol, f"{what}: max |logprob - float64 reference| = {err:.3e} > {atol}"
    return err
