"""GPU: hx_sample_rows_logprobs (csrc/sampling.hip, sampling_body.inc with SCORED) through sampling.sample_rows_logprobs —
exact answers first.  Logits and biases are multiples of 1/8 in [-8, 8].  ids, cut_out and u_out must be
hx_sample_rows_constrained's bit for bit whatever `want` and K are; the scores are held to tests/sample_logprob_ref.py
(float64) within logprob_ref.ATOL, with the kept set S taken from the cut that the parity check has just proved to be
the existing kernel's.  Every result buffer is pre-filled with a sentinel: a slot that was not written shows."""
import math

import numpy as np
import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd._C.kernel.norm import argmax_rows, logprob_rows_bytes
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, SAMPLE_MAX_N, PenaltyHistory, pack_constrained_step,
                                     sample_rows_logprobs)
from tests import logprob_ref
from tests import sample_logprob_ref as sref
from tests.test_gpu_constraints import DEV, DTYPES, IDS, eighths, launch_c, misaligned, random_table, same

pytestmark = pytest.mark.gpu

NEG = -math.inf
SENTINEL_BYTE = 0x5A          # ids 0x5a5a5a5a5a5a5a5a, top_ids 0x5a5a5a5a, floats 1.5e16: none is a result
WORST = [0.0]                 # the largest |fp32 - float64| seen in this run


def launch_s(logits, entries, k, want=None):
    """-> ((ids, cut, u), logprobs, top_ids, top_logprobs) on the host; want: None or a list of ints, one per row"""
    tables = pack_constrained_step(entries).to_device(DEV)
    rows = logits.shape[0]
    cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2))
    out = torch.full((logprob_rows_bytes(rows, k),), SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    w = None if want is None else torch.tensor(want, dtype=torch.int32, device=DEV)
    ids, lp, top_ids, top_lp = sample_rows_logprobs(logits, *tables, top_k=k, want=w, out=out, cut_out=cut, u_out=u)
    assert ids.dtype == torch.int64 and ids.shape == (rows,) and top_ids.shape == (rows, k) and top_lp.shape == (rows, k)
    assert ids.data_ptr() == out.data_ptr()
    return (ids.cpu(), cut.cpu(), u.cpu()), lp.cpu(), top_ids.cpu(), top_lp.cpu()


def assert_fill(lp, top_ids, top_lp, r, what):
    assert math.isnan(float(lp[r])) and bool((top_ids[r] == -1).all()) and bool(torch.isnan(top_lp[r]).all()), (what, r)


def check_scores(x, entries, base, got, k, want, degenerate=(), what=""):
    """got: launch_s' result; base: hx_sample_rows_constrained's (ids, cut, u) for the same rows.  Rows with want < 0 and
    the scored `degenerate` rows carry the fill values, every other row the reference's scores."""
    triple, lp, top_ids, top_lp = got
    assert same(triple, base), f"{what}: ids / cut_out / u_out differ from hx_sample_rows_constrained's"
    ids, cut, _ = base
    for r, (hist, pen, rec, bias) in enumerate(entries):
        if (want is not None and want[r] < 0) or r in degenerate:
            assert_fill(lp, top_ids, top_lp, r, what)
            continue
        z = sref.row_z(x[r], bias, hist, pen, rec)
        greedy = not rec[0] > 0
        assert greedy == math.isnan(float(cut[r])), (what, r)
        ref_lp, ref_ids, ref_top = sref.reference_logprobs(z, None if greedy else float(cut[r]), k)
        tag = f"{what} row {r} {rec}"
        assert top_ids[r].tolist() == ref_ids.tolist(), tag
        err = logprob_ref.assert_logprobs_close(top_lp[r], torch.from_numpy(ref_top), tag)
        chosen = int(ids[r])
        assert math.isfinite(float(lp[r])), tag
        err = max(err, logprob_ref.assert_logprobs_close(lp[r:r + 1], torch.from_numpy(ref_lp[chosen:chosen + 1]), tag + " (chosen)"))
        WORST[0] = max(WORST[0], err)
        n_kept = int(np.isfinite(ref_lp).sum())                   # |S| (a banned token that no cut removed has p = 0)
        assert int(torch.isfinite(top_lp[r]).sum()) == min(n_kept, k), tag
        if n_kept <= k:
            assert abs(float(top_lp[r].double().exp().sum()) - 1.0) <= logprob_ref.ATOL, tag
    print(f"{what}: largest |logprob - float64 reference| so far {WORST[0]:.3e}")


def mixed_entries(rows, n, g, seed0):
    """greedy, sampled top-k + bias, sampled top-p + penalties, sampled min_p, greedy + bias + penalties — in turn"""
    out = []
    for r in range(rows):
        seed, kind = (1 << 33) + 977 * seed0 + r, r % 5
        hist = PenaltyHistory(torch.randint(0, n, (12,), generator=g).tolist())
        table = random_table(n, 9, g)
        if kind == 0:
            out.append((None, NO_PENALTIES, (0.0, 0.5, 3, seed, r), None))           # (greedy: top_p / top_k ignored)
        elif kind == 1:
            out.append((None, NO_PENALTIES, (1.0, 1.0, max(1, min(5, n - 1)), seed, r), table))
        elif kind == 2:
            out.append((hist, (0.375, 0.25, 1.5), (0.5, 0.9, 0, seed, r), None))
        elif kind == 3:
            out.append((None, NO_PENALTIES, (2.0, 0.75, 50, seed, r, 0.125), table))
        else:
            out.append((hist, (0.25, 0.5, 2.0), (0.0, 1.0, 0, seed, r, 0.5), table))
    return out


def want_variants(rows):
    return [None, [-1] * rows, [(-1 if r % 2 else r) for r in range(rows)]]


@pytest.mark.parametrize("n,rows", [(1, 1), (7, 2), (1000, 3), (1024, 4), (1025, 5), (4099, 5), (12288, 5), (12296, 5), (32064, 5), (SAMPLE_MAX_N, 3)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_parity_and_scores(dtype, n, rows):
    g = torch.Generator().manual_seed(4000 + n)
    x = eighths((rows, n), g).to(dtype)
    entries = mixed_entries(rows, n, g, n)
    xd = x.to(DEV)
    base = launch_c(xd, entries)
    for k in (0, 1, 20):
        for want in want_variants(rows):
            check_scores(x, entries, base, launch_s(xd, entries, k, want), k, want, what=f"n={n} K={k} want={want}")
    check_scores(x, entries, base, launch_s(misaligned(xd), entries, 20, None), 20, None, what=f"n={n} misaligned")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_degenerate_rows(dtype):
    """a NaN, all -inf (every token banned) and a +inf, sampled and greedy, beside two ordinary rows"""
    n, rows = 1000, 6
    g = torch.Generator().manual_seed(21)
    x = eighths((rows, n), g).to(dtype)
    x[0, 17] = math.nan
    x[2, 900] = math.inf
    x[5, 3] = math.nan
    every = (np.arange(n, dtype=np.int32), np.full(n, -np.inf, np.float32))
    entries = [(None, NO_PENALTIES, (1.0, 0.9, 0, 11, 0), None), (None, NO_PENALTIES, (0.0, 1.0, 0, 12, 1), every),
               (None, NO_PENALTIES, (0.7, 1.0, 5, 13, 2), None), (None, NO_PENALTIES, (1.0, 0.9, 0, 14, 3), None),
               (None, NO_PENALTIES, GREEDY_RECORD, None), (None, NO_PENALTIES, GREEDY_RECORD, None)]
    xd = x.to(DEV)
    base = launch_c(xd, entries)
    assert base[0].tolist()[:3] == [17, 0, 900] and int(base[0][5]) == 3 and bool(torch.isnan(base[1][[0, 1, 2, 4, 5]]).all())
    for k in (0, 1, 20):
        for want in want_variants(rows):
            check_scores(x, entries, base, launch_s(xd, entries, k, want), k, want, degenerate=(0, 1, 2, 5),
                         what=f"degenerate K={k} want={want}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_unique_maximum(dtype):
    """top_k = 1 in the record, a unique maximum: S is that one token, its probability 1"""
    n, k = 1025, 5
    g = torch.Generator().manual_seed(23)
    x = eighths((2, n), g).clamp(max=6.0)
    x[0, 700] = x[1, 1024] = 7.5
    x = x.to(dtype)
    entries = [(None, NO_PENALTIES, (0.5, 1.0, 1, 5 + r, r), None) for r in range(2)]
    (ids, cut, _), lp, top_ids, top_lp = launch_s(x.to(DEV), entries, k)
    assert ids.tolist() == [700, 1024] and cut.tolist() == [15.0, 15.0]
    for r in range(2):
        assert float(lp[r]) == 0.0 and float(top_lp[r, 0]) == 0.0 and bool((top_lp[r, 1:] == NEG).all())
        assert top_ids[r].tolist() == sref.reference_logprobs(sref.row_z(x[r], None, None, NO_PENALTIES, entries[r][2]), 15.0, k)[1].tolist()


@pytest.mark.parametrize("j", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_ties(dtype, j):
    """the 2^j largest entries tied, top_k = 2^j in the record and 2^j alternatives: each has probability 2^-j"""
    n, c = 4099, 1 << j
    g = torch.Generator().manual_seed(25 + j)
    row = eighths((n,), g).clamp(max=5.0)
    where = sorted(torch.randperm(n, generator=g)[:c].tolist())
    row[where] = 6.25
    x = row.to(dtype).reshape(1, n)
    (ids, _, _), lp, top_ids, top_lp = launch_s(x.to(DEV), [(None, NO_PENALTIES, (1.0, 1.0, c, 77, j), None)], c)
    assert top_ids[0].tolist() == where and int(ids[0]) in where
    bits = top_lp[0].view(torch.int32)
    assert bool((bits == bits[0]).all()) and int(lp.view(torch.int32)[0]) == int(bits[0])
    exact = int(torch.tensor(-math.log(c), dtype=torch.float32).view(torch.int32))
    assert abs(int(bits[0]) - exact) <= 2, (float(top_lp[0, 0]), -math.log(c))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_short_row_and_ban(dtype):
    """n = 7, K = 20: every token is named, the banned one last with -inf; entries past n: id -1, -inf"""
    x = torch.tensor([[1.0, 3.0, 2.0, 3.0, -1.0, 0.5, 2.5]] * 2).to(dtype)
    ban = (np.asarray([1], np.int32), np.asarray([-np.inf], np.float32))
    entries = [(None, NO_PENALTIES, (1.0, 1.0, 0, 9, 0), ban), (None, NO_PENALTIES, GREEDY_RECORD, ban)]
    (ids, _, _), lp, top_ids, top_lp = launch_s(x.to(DEV), entries, 20)
    for r in range(2):
        assert top_ids[r].tolist() == [3, 6, 2, 0, 5, 4, 1] + [-1] * 13
        assert bool(torch.isfinite(top_lp[r, :6]).all()) and bool((top_lp[r, 6:] == NEG).all())
        assert abs(float(top_lp[r, :6].double().exp().sum()) - 1.0) <= logprob_ref.ATOL
        assert float(lp[r]) == float(top_lp[r, top_ids[r].tolist().index(int(ids[r]))])
    assert int(ids[1]) == 3
    # tokens that the truncation dropped are still named, in z order, with -inf: top_k = 2 keeps the two 3.0s
    entries = [(None, NO_PENALTIES, (1.0, 1.0, 2, 9, 0), None)]
    _, lp, top_ids, top_lp = launch_s(x[:1].to(DEV), entries, 4)
    assert top_ids[0].tolist() == [1, 3, 6, 2] and bool(torch.isfinite(top_lp[0, :2]).all()) and top_lp[0, 2:].tolist() == [NEG, NEG]


@pytest.mark.parametrize("n", [1000, 32064])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_random_rows_against_float64(dtype, n):
    g = torch.Generator().manual_seed(n + 1)
    recs = [(t, p, k, (1 << 36) + j, j, mp) for j, (mp, k, p, t) in enumerate(
        (mp, k, p, t) for mp in (0.0, 0.1) for k in (0, 12) for p in (1.0, 0.9) for t in (0.7, 1.5))]
    recs += [GREEDY_RECORD, (0.0, 0.9, 50, 3, 1, 0.5)]
    rows = len(recs)
    x = (torch.randn(rows, n, generator=g) * 3).to(dtype)
    entries = []
    for r, rec in enumerate(recs):
        hist = PenaltyHistory(torch.randint(0, n, (25,), generator=g).tolist()) if r % 3 == 0 and r < rows - 2 else None
        entries.append((hist, (0.3, 0.2, 1.7) if hist is not None else NO_PENALTIES, rec, random_table(n, 16 if r % 2 else 0, g)))
    xd = x.to(DEV)
    base = launch_c(xd, entries)
    got = launch_s(xd, entries, 20)
    check_scores(x, entries, base, got, 20, None, what=f"random n={n}")
    # the greedy row without bias entries or penalties: the raw log-softmax, and argmax_rows' id
    r = rows - 2
    assert entries[r][3][0].size == 0 and int(got[0][0][r]) == int(argmax_rows(xd[r:r + 1])[0])
    _, raw_lp, raw_ids, raw_top = logprob_ref.reference(x[r:r + 1], 20)
    assert got[2][r].tolist() == raw_ids[0].tolist()
    logprob_ref.assert_logprobs_close(got[3][r], raw_top[0], "greedy row against the raw log-softmax")
    logprob_ref.assert_logprobs_close(got[1][r:r + 1], raw_lp, "greedy row's id against the raw log-softmax")
    # twice the same, and a row alone gives what it gave in the batch
    again = launch_s(xd, entries, 20)
    assert same(again[0], got[0]) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again[1:], got[1:]))
    alone = launch_s(xd[3:4], entries[3:4], 20)
    assert all(torch.equal(a.view(torch.int32), b[3:4].view(torch.int32)) for a, b in zip(alone[1:], got[1:]))


def test_errors_leave_everything_untouched():
    rows, n, k = 2, 16, 3
    logits = torch.zeros((rows, n), dtype=torch.float16, device=DEV)
    step = pack_constrained_step([(PenaltyHistory([3, 4]), (1.0, 0.0, 1.0), GREEDY_RECORD, (np.asarray([5], np.int32), np.asarray([1.0], np.float32))),
                                  (None, NO_PENALTIES, GREEDY_RECORD, None)])
    sp, bi, bv, cb, hi, hc, cu, pen = step.to_device(DEV)
    out = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    lp = torch.full((rows,), 7.0, device=DEV)
    tids = torch.full((rows, k), -7, dtype=torch.int32, device=DEV)
    tlp = torch.full((rows, k), 7.0, device=DEV)
    want = torch.zeros(rows, dtype=torch.int32, device=DEV)
    f = _lib.lib().hx_sample_rows_logprobs
    ok = [out.data_ptr(), None, None, logits.data_ptr(), rows, n, n, hi.data_ptr(), hc.data_ptr(), cu.data_ptr(), 2,
          pen.data_ptr(), bi.data_ptr(), bv.data_ptr(), cb.data_ptr(), 1, sp.data_ptr(), lp.data_ptr(), tids.data_ptr(),
          tlp.data_ptr(), k, want.data_ptr(), _lib.HX_F16, _lib.current_stream()]
    SHAPE, DTYPE, NULL = -2, -1, -4
    cases = [((4, 0), SHAPE), ((5, 0), SHAPE), ((6, n - 1), SHAPE), ((5, SAMPLE_MAX_N + 1), SHAPE), ((10, -1), SHAPE),
             ((10, 1 << 31), SHAPE), ((15, -1), SHAPE), ((15, 1 << 31), SHAPE), ((20, -1), SHAPE), ((20, 21), SHAPE),
             ((22, _lib.HX_F32), DTYPE)]
    cases += [((at, None), NULL) for at in (0, 3, 16, 7, 8, 9, 11, 12, 13, 14, 17, 18, 19)]
    for (at, v), code in cases:
        args = list(ok)
        args[at] = v
        if (at, v) == (5, SAMPLE_MAX_N + 1):
            args[6] = v
        assert f(*args) == code, (at, v)
    torch.cuda.synchronize()
    assert out.tolist() == [-7, -7] and lp.tolist() == [7.0, 7.0] and bool((tids == -7).all()) and bool((tlp == 7.0).all())
    # K = 0 with the two alternative pointers NULL, want NULL, no tables: legal
    args = list(ok)
    for at in (7, 8, 9, 11, 12, 13, 14, 18, 19, 21):
        args[at] = None
    args[10] = args[15] = args[20] = 0
    assert f(*args) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0] and lp.tolist() == [pytest.approx(-math.log(n), abs=1e-6)] * 2 and bool((tids == -7).all())


def test_wrapper_refuses_malformed_arguments():
    logits = torch.zeros((2, 16), dtype=torch.float16, device=DEV)
    step = pack_constrained_step([(None, NO_PENALTIES, GREEDY_RECORD, (np.asarray([5, 6], np.int32), np.asarray([1.0, 2.0], np.float32))),
                                  (None, NO_PENALTIES, GREEDY_RECORD, None)])
    tables = step.to_device(DEV)
    E = _lib.HydraHipError
    w = torch.zeros(2, dtype=torch.int32, device=DEV)
    for bad in (lambda: sample_rows_logprobs(logits, *tables, top_k=21), lambda: sample_rows_logprobs(logits, *tables, top_k=-1),
                lambda: sample_rows_logprobs(logits, *tables, top_k=True),
                lambda: sample_rows_logprobs(logits, *tables, top_k=1, want=w.long()),
                lambda: sample_rows_logprobs(logits, *tables, top_k=1, want=w[:1]),
                lambda: sample_rows_logprobs(logits, *tables, top_k=1, out=torch.empty(7, dtype=torch.uint8, device=DEV)),
                lambda: sample_rows_logprobs(logits.float(), *tables, top_k=1),
                lambda: sample_rows_logprobs(logits, tables[0], tables[1], tables[2][:1], tables[3], top_k=1)):
        with pytest.raises(E):
            bad()
    with pytest.raises(E, match="CPU tensor"):
        sample_rows_logprobs(logits, *tables, top_k=1, want=w.cpu())
    with pytest.raises(TypeError):
        sample_rows_logprobs(logits, *tables)                                  # top_k is required, by keyword
    ids, lp, top_ids, top_lp = sample_rows_logprobs(logits, *tables, top_k=2, want=w)
    assert ids.tolist() == [6, 0] and top_ids.tolist() == [[6, 5], [0, 1]]
