"""GPU: hx_sample_rows_constrained (csrc/sampling.hip, sampling_body.inc) — exact answers first.  Logits and biases are
multiples of 1/8 in [-8, 8]: float(x) + b is then representable in fp16 and bf16 (asserted on the CPU before every
launch), so the constrained launch on (logits, bias table) must equal hx_sample_rows on the pre-biased logits BIT FOR BIT
in ids, cut_out and u_out.  min_p, which hx_sample_rows does not have, is held to tests/constraint_ref.py."""
import math

import numpy as np
import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, SAMPLE_MAX_N, PenaltyHistory, pack_constrained_step,
                                     pack_sample_records, pack_sample_step, sample_rows, sample_rows_constrained)
from tests import constraint_ref as cref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
NO_BIAS = (np.zeros(0, np.int32), np.zeros(0, np.float32))


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    """two (ids, cut, u) triples, bit for bit (a cut may be NaN)"""
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def launch_c(logits, entries):
    """entries: (PenaltyHistory or None, penalties, record, (bias ids, bias values) or None) per row -> (ids, cut, u)"""
    tables = pack_constrained_step(entries).to_device(DEV)
    rows = logits.shape[0]
    cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2))
    ids = sample_rows_constrained(logits, *tables, cut_out=cut, u_out=u)
    assert ids.dtype == torch.int64 and ids.shape == (rows,)
    return ids.cpu(), cut.cpu(), u.cpu()


def launch_plain(logits, entries):
    """hx_sample_rows on the same rows: the entries' first three elements, five-word records"""
    sp, hi, hc, cu, pen = pack_sample_step([(h, p, tuple(rec[:5])) for h, p, rec, *_ in entries]).to_device(DEV)
    rows = logits.shape[0]
    cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2))
    ids = sample_rows(logits, sp, hi, hc, cu, pen, cut_out=cut, u_out=u)
    return ids.cpu(), cut.cpu(), u.cpu()


def eighths(shape, g):
    return torch.randint(-64, 65, shape, generator=g).float() / 8


def random_table(n, count, g):
    """`count` distinct ids of the row (at most n), biases that are multiples of 1/8 in [-8, 8]"""
    count = min(count, n)
    ids = torch.randperm(n, generator=g)[:count].to(torch.int32).numpy()
    return ids, eighths((count,), g).numpy()


def pre_biased(x, tables, dtype):
    """the logits with every row's table added, on the CPU, and the proof that nothing was rounded"""
    want = x.float().clone()
    for r, (ids, values) in enumerate(tables):
        want[r] = cref.biased_row(x[r], ids.tolist(), values.tolist())
    out = want.to(dtype)
    finite = torch.isfinite(want)
    assert torch.equal(out.float()[finite], want[finite]) and torch.equal(torch.isinf(out), ~finite), "float(x) + b is not representable"
    return out


def misaligned(logits):
    """the same rows behind a base that is not 16-byte aligned and a row stride that is no multiple of 8"""
    rows, n = logits.shape
    ld = n + 3 if (n + 3) % 8 else n + 5
    store = torch.zeros(rows * ld + 8, dtype=logits.dtype, device=DEV)
    view = store[1:1 + rows * ld].view(rows, ld)[:, :n]
    view.copy_(logits)
    assert view.stride(0) % 8 != 0 and view.data_ptr() % 16 != 0
    return view


def mixed_records(rows, n, seed0):
    """greedy, top-k only, top-p only, both — in turn"""
    kinds = [(0.0, 1.0, 0), (1.0, 1.0, max(1, min(5, n - 1))), (0.7, 0.9, 0), (1.5, 0.5, 50)]
    return [kinds[r % 4] + ((1 << 33) + seed0 * 131 + r, r) for r in range(rows)]


@pytest.mark.parametrize("n", [1, 7, 8, 1023, 1025, 12288, 12296, 32064, SAMPLE_MAX_N])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_equals_sample_rows_on_pre_biased_logits(dtype, n):
    """8 rows with 0, 1, 300 and 1500 entries (the last: the strided entry loop beyond 1024 threads), once with greedy /
    top-k / top-p / both falling on one order of the counts and once on the other; both load paths"""
    g = torch.Generator().manual_seed(1000 + n)
    rows = 8
    x = eighths((rows, n), g).to(dtype)
    assert torch.equal(x.float() * 8, (x.float() * 8).round())
    for shift in (0, 1):
        counts = [(0, 1, 300, 1500)[(r + (r // 4) * shift) % 4] for r in range(rows)]
        tables = [random_table(n, c, g) for c in counts]
        recs = mixed_records(rows, n, n + shift)
        entries = [(None, NO_PENALTIES, rec, t) for rec, t in zip(recs, tables)]
        want = launch_plain(pre_biased(x, tables, dtype).to(DEV), entries)
        got = launch_c(x.to(DEV), entries)
        assert same(got, want), (n, shift, got, want)
        assert same(launch_c(misaligned(x.to(DEV)), entries), want), (n, shift, "misaligned")
    assert bool(torch.isnan(want[1][0::4]).all()) and (n < 2 or not bool(torch.isnan(want[1][1::4]).any()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bias_comes_before_the_penalties(dtype):
    """history and bias tables share tokens: the penalised value starts from x + b"""
    n, rows = 1025, 8
    g = torch.Generator().manual_seed(7)
    x = eighths((rows, n), g).to(dtype)
    tables, entries = [], []
    for r, rec in enumerate(mixed_records(rows, n, 3)):
        ids, values = random_table(n, 40, g)
        shared = ids[:20].tolist()
        hist = PenaltyHistory(shared + shared[:7] + torch.randint(0, n, (10,), generator=g).tolist())
        # the row's maximum is in both tables: a bias of +8 puts it on top, the penalties act on the sum
        top = int(x[r].float().argmax())
        if top not in ids.tolist():
            ids, values = np.append(ids, np.int32(top)), np.append(values, np.float32(8.0))
        hist.append(top)
        tables.append((ids, values))
        entries.append((hist, (0.375, 0.25, 1.5), rec, (ids, values)))
    want = launch_plain(pre_biased(x, tables, dtype).to(DEV), entries)
    got = launch_c(x.to(DEV), entries)
    assert same(got, want)
    # and it is not what the other order gives: penalising float(x) and adding b afterwards moves a greedy row's value
    unbiased = launch_plain(x.to(DEV), entries)
    assert not torch.equal(unbiased[0], want[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bans(dtype):
    n, rows = 1025, 64
    g = torch.Generator().manual_seed(9)
    base = eighths((n,), g).clamp(max=5.0)
    top5 = [100, 200, 300, 400, 1024]
    base[top5] = torch.tensor([8.0, 7.5, 7.0, 6.5, 6.0])
    base[[17, 600]] = 5.5                                   # what is left on top once the five are gone
    x = base.to(dtype).expand(rows, n).contiguous()
    for banned in ([100], top5):
        table = (np.asarray(banned, np.int32), np.full(len(banned), -np.inf, np.float32))
        recs = [(0.0, 1.0, 0, 5, 0)] + [(1.0, 1.0, 0, (1 << 34) + 7 * r, r) for r in range(1, rows)]     # one greedy row, 63 seeds
        entries = [(None, NO_PENALTIES, rec, table) for rec in recs]
        got = launch_c(x.to(DEV), entries)
        assert not set(got[0].tolist()) & set(banned)
        assert int(got[0][0]) == (200 if banned == [100] else 17)
        written = x.clone()
        written[:, banned] = -math.inf
        assert same(got, launch_plain(written.to(DEV), entries))
        assert same(got, launch_plain(pre_biased(x, [table] * rows, dtype).to(DEV), entries))
        # top_k = 1 on a sampled row: the best of what is left, for every seed
        entries = [(None, NO_PENALTIES, (1.0, 1.0, 1, 99 + r, r), table) for r in range(rows)]
        ids, cut, _ = launch_c(x.to(DEV), entries)
        assert set(ids.tolist()) <= ({200} if banned == [100] else {17, 600}) and set(cut.tolist()) == {7.5 if banned == [100] else 5.5}
    # a ban under a history entry stays a ban: -inf through the penalties
    entries = [(PenaltyHistory([100, 100]), (-2.0, -2.0, 0.5), (1.0, 1.0, 0, 3 + r, r), (np.asarray([100], np.int32), np.asarray([-np.inf], np.float32)))
               for r in range(rows)]
    assert 100 not in launch_c(x.to(DEV), entries)[0].tolist()
    # every token of the row banned: the degenerate row — id 0 and cut NaN, greedy or sampled
    small = eighths((2, 8), g).to(dtype).to(DEV)
    every = (np.arange(8, dtype=np.int32), np.full(8, -np.inf, np.float32))
    ids, cut, _ = launch_c(small, [(None, NO_PENALTIES, (0.0, 1.0, 0, 1, 0), every), (None, NO_PENALTIES, (1.0, 0.9, 3, 1, 0, 0.5), every)])
    assert ids.tolist() == [0, 0] and bool(torch.isnan(cut).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rows_are_independent(dtype):
    """only some rows have entries or min_p: the others get hx_sample_rows' ids, cut and u bit for bit; twice the same"""
    n, rows = 32064, 12
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(rows, n, generator=g) * 3).to(dtype).to(DEV)
    recs = mixed_records(rows, n, 5)
    entries = []
    for r, rec in enumerate(recs):
        hist = PenaltyHistory(torch.randint(0, n, (30,), generator=g).tolist()) if r % 2 else None
        pen = (0.3, 0.2, 1.7) if hist is not None else NO_PENALTIES
        if r % 3 == 0:
            entries.append((hist, pen, rec, random_table(n, 300, g)))
        elif r % 3 == 1:
            entries.append((hist, pen, rec + (0.3,), None))
        else:
            entries.append((hist, pen, rec, None if r % 2 else NO_BIAS))
    got = launch_c(x, entries)
    want = launch_plain(x, entries)
    free = [r for r in range(rows) if r % 3 == 2] + [r for r in range(rows) if r % 3 == 1 and recs[r][0] == 0.0]   # (greedy rows ignore min_p)
    assert same([t[free] for t in got], [t[free] for t in want])
    assert not torch.equal(got[0], want[0]), "the constrained rows were meant to differ"
    assert same(launch_c(x, entries), got)
    # every row on its own gives what it gave in the batch
    for r in (0, 1, 5):
        assert same(launch_c(x[r:r + 1], [entries[r]]), [t[r:r + 1] for t in got])
    # no bias entries at all (bias_total == 0, null pointers) and no min_p: hx_sample_rows
    none = [(h, p, rec[:5], None) for h, p, rec, _ in entries]
    assert same(launch_c(x, none), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_entries_outside_the_row_are_ignored(dtype):
    n, rows = 1025, 4
    g = torch.Generator().manual_seed(13)
    x = eighths((rows, n), g).to(dtype).to(DEV)
    recs = mixed_records(rows, n, 9)
    clean, dirty = [], []
    for r in range(rows):
        ids, values = random_table(n, 20, g)
        clean.append((ids, values))
        at = [0, 7, 20, 22]
        dirty.append((np.insert(ids, [0, 7, 20, 20], np.asarray([-1, n, n + 5, -(1 << 31)], np.int32)),
                      np.insert(values, [0, 7, 20, 20], np.asarray([8.0, -8.0, np.inf, -np.inf], np.float32))))
        assert len(dirty[-1][0]) == 24 and at
    a = launch_c(x, [(None, NO_PENALTIES, rec, t) for rec, t in zip(recs, clean)])
    b = launch_c(x, [(None, NO_PENALTIES, rec, t) for rec, t in zip(recs, dirty)])
    assert same(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_min_p_off_and_exact(dtype):
    n, rows = 1025, 9
    g = torch.Generator().manual_seed(15)
    x = (torch.randn(rows, n, generator=g) * 3).to(dtype).to(DEV)
    recs = [(1.0, 1.0, 0), (0.7, 0.9, 0), (1.5, 0.5, 50)] * 3
    recs = [rec + ((1 << 35) + r, r) for r, rec in enumerate(recs)]
    want = launch_plain(x, [(None, NO_PENALTIES, rec, None) for rec in recs])
    for off in (0.0, -0.0, -0.5, math.nan, -math.inf):
        assert same(launch_c(x, [(None, NO_PENALTIES, rec + (off,), None) for rec in recs]), want), off
    # min_p = 1: only the row's maxima are left, the cut is m
    y = x.clone()
    y[:, 77] = y[:, 900] = 12.0
    ids, cut, _ = launch_c(y, [(None, NO_PENALTIES, rec + (1.0,), None) for rec in recs])
    m = [12.0 / rec[0] for rec in recs]
    assert set(ids.tolist()) == {77, 900} and cut.tolist() == [float(np.float32(12.0) / np.float32(rec[0])) for rec in recs], (ids, cut, m)
    # an exact case: e = 1, 1, e^-1, e^-2, ... at T = 1 — min_p = 0.3 keeps down to z = 2, min_p = 0.1 down to z = 1;
    # top_k = 2 cuts higher than min_p = 0.1, min_p = 0.3 higher than top_k = 5
    row = torch.full((n,), -4.0)
    row[[3, 500, 1024, 8, 9]] = torch.tensor([3.0, 3.0, 2.0, 1.0, 0.0])
    z = row.to(dtype).to(DEV).expand(6, n).contiguous()
    recs = [(1.0, 1.0, 0, 5, 0, 0.3), (1.0, 1.0, 0, 5, 1, 0.1), (1.0, 1.0, 2, 5, 2, 0.1), (1.0, 1.0, 5, 5, 3, 0.3),
            (0.0, 1.0, 0, 5, 4, 0.3), (1.0, 1.0, 0, 5, 5, 1e-30)]
    ids, cut, _ = launch_c(z, [(None, NO_PENALTIES, rec, None) for rec in recs])
    assert cut[:4].tolist() == [2.0, 1.0, 3.0, 2.0] and math.isnan(float(cut[4])) and float(cut[5]) == -4.0
    assert int(ids[4]) == 3 and set(ids[:4].tolist()) <= {3, 500, 1024, 8}


@pytest.mark.parametrize("n", [1000, 32064])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_min_p_random_rows(dtype, n):
    """min_p x top-k x top-p x temperature on random rows, with bias tables and histories beside: every row against
    constraint_ref (the float64 e within DELTA of min_p, relatively); greedy rows ignore min_p"""
    g = torch.Generator().manual_seed(n)
    recs = [(t, p, k, (1 << 36) + j, j, mp) for j, (mp, k, p, t) in enumerate(
        (mp, k, p, t) for mp in (0.01, 0.1, 0.5) for k in (0, 50) for p in (1.0, 0.9) for t in (0.7, 1.5))]
    recs += [(0.0, 0.9, 50, 3, 0, 0.5), (0.0, 1.0, 0, 3, 1, 0.01)]
    rows = len(recs)
    x = (torch.randn(rows, n, generator=g) * 3).to(dtype)
    entries = []
    for r, rec in enumerate(recs):
        hist = PenaltyHistory(torch.randint(0, n, (25,), generator=g).tolist()) if r % 3 == 0 else None
        ids, values = random_table(n, 16 if r % 2 else 0, g)
        entries.append((hist, (0.3, 0.2, 1.7) if hist is not None else NO_PENALTIES, rec, (ids, values)))
    ids, cut, u = launch_c(x.to(DEV), entries)
    kinds = []
    for r, (h, pen, rec, (b_ids, b_values)) in enumerate(entries):
        kinds.append(cref.check_row_constrained(x[r], b_ids.tolist(), b_values.tolist(), list(h.ids) if h else [],
                                                list(h.counts) if h else [], pen, rec, int(ids[r]), float(cut[r]),
                                                np.float32(u[r].item()), f"n={n} row {r} {rec}"))
    assert kinds == ["sampled"] * (rows - 2) + ["greedy"] * 2
    # min_p did cut: without it the kept set of the top_p = 1, top_k = 0 rows is the whole row
    wide = [r for r, rec in enumerate(recs) if rec[0] > 0 and rec[1] == 1.0 and rec[2] == 0]
    zmin = [float((cref.biased_row(x[r], *[t.tolist() for t in entries[r][3]])).min()) for r in wide]
    assert wide and all(float(cut[r]) > lo / recs[r][0] for r, lo in zip(wide, zmin))
    # greedy rows ignore min_p: the same rows and tables without it, bit for bit
    last = [(h, p, rec[:5], b) for h, p, rec, b in entries[-2:]]
    assert same(launch_c(x[-2:].to(DEV), last), [t[-2:] for t in (ids, cut, u)])


def test_errors_leave_ids_untouched():
    rows, n = 2, 16
    logits = torch.zeros((rows, n), dtype=torch.float16, device=DEV)
    step = pack_constrained_step([(PenaltyHistory([3, 4]), (1.0, 0.0, 1.0), GREEDY_RECORD, (np.asarray([5], np.int32), np.asarray([1.0], np.float32))),
                                  (None, NO_PENALTIES, GREEDY_RECORD, None)])
    sp, bi, bv, cb, hi, hc, cu, pen = step.to_device(DEV)
    out = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    f = _lib.lib().hx_sample_rows_constrained
    ok = [out.data_ptr(), None, None, logits.data_ptr(), rows, n, n, hi.data_ptr(), hc.data_ptr(), cu.data_ptr(), 2,
          pen.data_ptr(), bi.data_ptr(), bv.data_ptr(), cb.data_ptr(), 1, sp.data_ptr(), _lib.HX_F16, _lib.current_stream()]
    SHAPE, DTYPE, NULL = -2, -1, -4
    cases = [((4, 0), SHAPE), ((5, 0), SHAPE), ((6, n - 1), SHAPE), ((5, SAMPLE_MAX_N + 1), SHAPE), ((10, -1), SHAPE),
             ((10, 1 << 31), SHAPE), ((15, -1), SHAPE), ((15, 1 << 31), SHAPE), ((17, _lib.HX_F32), DTYPE)]
    cases += [((at, None), NULL) for at in (0, 3, 16, 7, 8, 9, 11, 12, 13, 14)]
    for (at, v), code in cases:
        args = list(ok)
        args[at] = v
        if (at, v) == (5, SAMPLE_MAX_N + 1):
            args[6] = v
        assert f(*args) == code, (at, v)
    torch.cuda.synchronize()
    assert out.tolist() == [-7, -7]
    # total == 0 and bias_total == 0 with every table pointer NULL: legal
    args = list(ok)
    for at in (7, 8, 9, 11, 12, 13, 14):
        args[at] = None
    args[10] = args[15] = 0
    assert f(*args) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0]
    assert sample_rows_constrained(logits, sp, bi, bv, cb, hi, hc, cu, pen).tolist() == [5, 0]


def test_wrapper_refuses_malformed_tensors():
    logits = torch.zeros((2, 16), dtype=torch.float16, device=DEV)
    step = pack_constrained_step([(PenaltyHistory([3, 4]), (1.0, 0.0, 1.0), GREEDY_RECORD, (np.asarray([5, 6], np.int32), np.asarray([1.0, 2.0], np.float32))),
                                  (None, NO_PENALTIES, GREEDY_RECORD, None)])
    sp, bi, bv, cb, hi, hc, cu, pen = step.to_device(DEV)
    E = _lib.HydraHipError
    call = sample_rows_constrained
    for bad in (lambda: call(logits.float(), sp, bi, bv, cb), lambda: call(logits[0], sp, bi, bv, cb),
                lambda: call(logits.t(), sp, bi, bv, cb), lambda: call(logits, sp[:1], bi, bv, cb),
                lambda: call(logits, sp.float(), bi, bv, cb),
                lambda: call(logits, sp, bi.float(), bv, cb),                        # bias_ids must be int32
                lambda: call(logits, sp, bi, bv.view(torch.int32), cb),              # bias_values fp32
                lambda: call(logits, sp, bi, bv[:1], cb),                            # as many values as ids
                lambda: call(logits, sp, bi, bv, cb[:2]),                            # cu_bias [rows + 1]
                lambda: call(logits, sp, bi, bv, cb.long()),
                lambda: call(logits, sp, torch.zeros(4, dtype=torch.int32, device=DEV)[::2], bv, cb),     # non-contiguous
                lambda: call(logits, sp, bi, bv, torch.zeros(6, dtype=torch.int32, device=DEV)[::2]),
                lambda: call(logits, sp, bi, bv, cb, hi, hc, cu),                    # three of the four history tables
                lambda: call(logits, sp, bi, bv, cb, hi, hc, cu[:2], pen),
                lambda: call(logits, sp, bi, bv, cb, out=torch.empty(2, dtype=torch.int32, device=DEV)),
                lambda: call(logits, sp, bi, bv, cb, cut_out=torch.empty(3, device=DEV)),
                lambda: call(logits, sp, bi, bv, cb, u_out=torch.empty(2, dtype=torch.float64, device=DEV)),
                lambda: call(torch.zeros((1, SAMPLE_MAX_N + 1), dtype=torch.bfloat16, device=DEV), sp[:1], bi, bv, cb[:2])):
        with pytest.raises(E):
            bad()
    with pytest.raises(E, match="CPU tensor"):
        call(logits, sp, bi.cpu(), bv, cb)
    with pytest.raises(E, match="CPU tensor"):
        call(logits, sp, bi, bv, cb.cpu())
    assert call(logits, sp, bi, bv, cb, hi, hc, cu, pen).tolist() == [6, 0]
