"""GPU: hx_sample_rows (csrc/sampling.hip) against tests/sampling_ref.py — every row of every launch is checked on its
own: u bit for bit against the numpy Philox, the cut v* against the float64 A(v) / Z_K (check 2 of sampling_ref), the
token against the float64 index-order CDF (check 3), greedy and degenerate rows against the penalised argmax.  Every
launch asks for cut_out / u_out; shapes are the smallest at which a branch of the kernel can go wrong."""
import itertools
import math

import numpy as np
import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, SAMPLE_MAX_N, PenaltyHistory, pack_penalty_step,
                                     pack_sample_records, pack_sample_step, penalized_argmax_rows, sample_rows)
from tests import sampling_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
TEMPS, TOP_PS = (0.7, 1.0, 1.5), (1e-6, 0.5, 0.9, 1.0)
SEEDS = ((1 << 32) + 7, (1 << 40) + 3, (1 << 63) - 1, 0x9E3779B97F4A7C15 >> 1, 5)
OFFSETS = (0, 1, (1 << 32) + 5)


def launch(logits, entries, tables=True, diagnostics=True):
    """entries: (PenaltyHistory or None, penalties, record) per row -> (ids, cut, u) on the host."""
    sp, hi, hc, cu, pen = pack_sample_step(entries).to_device(DEV)
    rows = logits.shape[0]
    cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2)) if diagnostics else (None, None)
    ids = sample_rows(logits, sp, *((hi, hc, cu, pen) if tables else ()), cut_out=cut, u_out=u)
    assert ids.dtype == torch.int64 and ids.shape == (rows,)
    return (ids.cpu(), cut.cpu(), u.cpu()) if diagnostics else ids.cpu()


def verify(logits, entries, ids, cut, u, tag=""):
    """every row against sampling_ref; returns the rows' kinds"""
    host = logits.cpu()
    kinds = []
    for r, (h, pen, rec) in enumerate(entries):
        kinds.append(ref.check_row(host[r], list(h.ids) if h else [], list(h.counts) if h else [], pen, rec, int(ids[r]),
                                   float(cut[r]), np.float32(u[r].item()), f"{tag} row {r} {rec}"))
    return kinds


def plain(records):
    return [(None, NO_PENALTIES, rec) for rec in records]


def grid_records(n, seed0=1):
    """T x top_k x top_p, every row its own seed and offset"""
    recs = []
    for j, (t, k, p) in enumerate(itertools.product(TEMPS, (0, 1, 5, 50, n, n + 1), TOP_PS)):
        recs.append((t, p, k, SEEDS[j % len(SEEDS)] ^ (seed0 * 977 + j), OFFSETS[j % 3] + j // 3))
    return recs


def randn3(rows, n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, n, generator=g) * 3).to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_u_is_philox(dtype):
    recs = [(1.0, 1.0, 0, s, o) for s in SEEDS for o in OFFSETS] + [(0.0, 1.0, 0, s, 3) for s in SEEDS]   # greedy rows get their u too
    logits = randn3(len(recs), 64, dtype, 1)
    ids, cut, u = launch(logits, plain(recs), tables=False)
    for r, rec in enumerate(recs):
        assert np.float32(u[r].item()).view(np.uint32) == ref.uniform(rec[3], rec[4]).view(np.uint32), rec
        assert 0.0 <= float(u[r]) < 1.0
    assert len({float(v) for v in u}) == len(recs)
    verify(logits, plain(recs), ids, cut, u)


@pytest.mark.parametrize("n", [1, 7, 8, 1023, 1025, 12288, 12296, 32064, SAMPLE_MAX_N])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_parameter_grid(dtype, n):
    """72 rows of randn * 3 in one launch, each with its own (T, top_k, top_p, seed, offset)"""
    recs = grid_records(n, n)
    logits = randn3(len(recs), n, dtype, n)
    ids, cut, u = launch(logits, plain(recs), tables=False)
    kinds = verify(logits, plain(recs), ids, cut, u, f"n={n}")
    assert kinds == ["sampled"] * len(recs)
    if n >= 1023:
        assert len({int(i) for i in ids}) > 10, "the draws hardly differ"
    # the ids do not depend on the diagnostics being asked for
    assert torch.equal(launch(logits, plain(recs), tables=False, diagnostics=False), ids)


@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_counts_and_the_scalar_read_path(dtype, rows):
    """rows in {1, 3, 64}, each once from a contiguous tensor and once from a view whose row stride is no multiple of 8
    and whose base is not 16-byte aligned (the non-vector read): the same answers"""
    n = 1025
    recs = grid_records(n, rows)[:rows] if rows <= 3 else grid_records(n, rows)[4:4 + rows]
    logits = randn3(rows, n, dtype, 100 + rows)
    ids, cut, u = launch(logits, plain(recs), tables=False)
    verify(logits, plain(recs), ids, cut, u, f"rows={rows}")
    ld = n + 3
    store = torch.zeros(rows * ld + 8, dtype=dtype, device=DEV)
    view = store[1:1 + rows * ld].view(rows, ld)[:, :n]
    view.copy_(logits)
    assert view.stride(0) % 8 != 0 and view.data_ptr() % 16 != 0
    ids2, cut2, u2 = launch(view, plain(recs), tables=False)
    assert torch.equal(ids2, ids) and torch.equal(cut2.view(torch.int32), cut.view(torch.int32)) and torch.equal(u2, u)


def test_the_widest_row_and_one_more():
    logits = torch.zeros((1, SAMPLE_MAX_N + 1), dtype=torch.bfloat16, device=DEV)
    sp = torch.from_numpy(pack_sample_records([(1.0, 1.0, 0, 1, 0)])).to(DEV)
    with pytest.raises(_lib.HydraHipError):
        sample_rows(logits, sp)
    out = torch.empty(1, dtype=torch.int64, device=DEV)
    assert _lib.lib().hx_sample_rows(out.data_ptr(), None, None, logits.data_ptr(), 1, SAMPLE_MAX_N + 1, SAMPLE_MAX_N + 1,
                                     None, None, None, 0, None, sp.data_ptr(), _lib.HX_BF16, _lib.current_stream()) == -2
    assert SAMPLE_MAX_N >= 32064


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_many_draws(dtype):
    """4096 rows of the same content, k = 4, p = 1, every seed and offset different: every draw is checked on its own,
    and all four kept tokens occur"""
    n, rows = 1025, 4096
    row = (torch.randn(n, generator=torch.Generator().manual_seed(5)) * 3).clamp(max=6.0)
    kept = {10: 9.0, 500: 8.5, 1000: 8.75, 1024: 8.25}
    for i, v in kept.items():
        row[i] = v
    logits = row.to(dtype).to(DEV).expand(rows, n).contiguous()
    recs = [(1.0, 1.0, 4, (1 << 33) + 1000003 * r, r * 7 + (r % 5) * (1 << 32)) for r in range(rows)]
    ids, cut, u = launch(logits, plain(recs), tables=False)
    host = logits[0].cpu()
    z = host.float().numpy()
    assert set(cut.tolist()) == {8.25}
    us = set()
    for r, rec in enumerate(recs):
        assert np.float32(u[r].item()).view(np.uint32) == ref.uniform(rec[3], rec[4]).view(np.uint32)
        ref.check_cut(z, 4, 1.0, float(cut[r]), f"row {r}")
        ref.check_draw(z, float(cut[r]), float(u[r]), int(ids[r]), f"row {r}")
        us.add(float(u[r]))
    assert len(us) > 4000
    counts = {i: int((ids == i).sum()) for i in kept}
    assert sum(counts.values()) == rows and min(counts.values()) > 300, counts


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_greedy_rows_alone_and_mixed(dtype):
    """T = 0 rows give penalized_argmax_rows' ids bit for bit — alone, beside sampled rows, with and without history"""
    n, rows = 1025, 12
    logits = randn3(rows, n, dtype, 21)
    logits[4, 77] = logits[4, 900] = logits[4].max() + 1          # a tie at the top: the lower index
    hists = [PenaltyHistory([int(logits[r].argmax()), 5, 5, 9]) if r % 3 == 0 else None for r in range(rows)]
    pens = [(1.5, 0.5, 1.3) if h is not None else NO_PENALTIES for h in hists]
    want = penalized_argmax_rows(logits, *pack_penalty_step(list(zip(hists, pens))).to_device(DEV)).cpu()
    all_greedy = [(h, p, (0.0, 0.5, 3, 11 + r, r)) for r, (h, p) in enumerate(zip(hists, pens))]
    ids, cut, u = launch(logits, all_greedy)
    assert torch.equal(ids, want) and bool(torch.isnan(cut).all())
    assert verify(logits, all_greedy, ids, cut, u) == ["greedy"] * rows
    assert int(ids[4]) == 77
    mixed = [(h, p, (0.0, 1.0, 0, 3, r) if r % 2 else (0.9, 0.9, 20, (1 << 35) + r, r)) for r, (h, p) in enumerate(zip(hists, pens))]
    ids, cut, u = launch(logits, mixed)
    kinds = verify(logits, mixed, ids, cut, u)
    assert kinds == ["sampled", "greedy"] * (rows // 2)
    assert torch.equal(ids[1::2], want[1::2])
    # the same row gives the same token whatever else is in the batch
    alone = launch(logits[4:5], [mixed[4]])
    assert int(alone[0][0]) == int(ids[4]) and float(alone[1][0]) == float(cut[4])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cases(dtype):
    n = 1025
    g = torch.Generator().manual_seed(8)
    base = (torch.randn(n, generator=g) * 3).clamp(max=5.0)
    rows, recs, expect = [], [], []

    def add(row, rec, in_set=None):
        rows.append(row.clone())
        recs.append(rec)
        expect.append(in_set)
    # top_k = 1 with a unique maximum: the argmax for every u
    uniq = base.clone()
    uniq[321] = 9.0
    for o in range(8):
        add(uniq, (1.5, 1.0, 1, (1 << 34) + 1, o), {321})
    # a constant row keeps everything
    for o in range(4):
        add(torch.full((n,), -2.5), (0.7, 0.9, 0, 99, o))
        add(torch.zeros(n), (1.0, 0.5, 7, 98, o))
    # tied maxima with top_k = 1 or top_p = 1e-6: one of the tied indices
    tied = base.clone()
    tied[[4, 400, 1024]] = 8.0
    for o in range(6):
        add(tied, (1.0, 1.0, 1, 5, o), {4, 400, 1024})
        add(tied, (0.7, 1e-6, 0, 6, o), {4, 400, 1024})
    # degenerate rows: all -inf gives 0, a NaN the first NaN's index, a +inf its index
    add(torch.full((n,), -math.inf), (1.0, 0.9, 5, 1, 0), {0})
    nan = base.clone()
    nan[[700, 30]] = math.nan
    add(nan, (1.0, 0.9, 5, 1, 1), {30})
    inf = base.clone()
    inf[[600, 601]] = math.inf
    add(inf, (0.7, 1.0, 0, 1, 2), {600})
    logits = torch.stack(rows).to(dtype).to(DEV)
    ids, cut, u = launch(logits, plain(recs), tables=False)
    kinds = verify(logits, plain(recs), ids, cut, u)
    assert kinds[-3:] == ["degenerate"] * 3 and set(kinds[:-3]) == {"sampled"}
    for r, allowed in enumerate(expect):
        assert allowed is None or int(ids[r]) in allowed, (r, recs[r], int(ids[r]))
    const = [int(ids[r]) for r, rec in enumerate(recs) if rec[3] in (98, 99)]
    assert len(set(const)) > 2, "a constant row keeps everything: eight draws on one token"
    assert {int(ids[r]) for r, rec in enumerate(recs) if rec[3] in (5, 6)} == {4, 400, 1024}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_three_finite_places_over_256_offsets(dtype):
    n = 1023
    row = torch.full((n,), -math.inf)
    row[[3, 511, 1022]] = torch.tensor([1.0, 2.0, 1.5])
    logits = row.to(dtype).to(DEV).expand(256, n).contiguous()
    for k, p in ((0, 1.0), (0, 0.999), (2, 1.0)):
        recs = [(1.0, p, k, 1 << 50, o) for o in range(256)]
        ids, cut, u = launch(logits, plain(recs), tables=False)
        assert verify(logits, plain(recs), ids, cut, u) == ["sampled"] * 256
        assert {int(i) for i in ids} == ({3, 511, 1022} if k == 0 else {511, 1022})


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_penalties(dtype):
    n, rows = 1025, 64
    base = (torch.randn(n, generator=torch.Generator().manual_seed(13)) * 2).clamp(max=4.0)
    base[[100, 200, 300, 400]] = torch.tensor([9.0, 8.0, 7.5, 7.0])
    logits = base.to(dtype).to(DEV).expand(rows, n).contiguous()
    # token 100 was generated five times: frequency 1.5 takes it from 9 to 1.5, out of the top_k = 3 nucleus; the ids
    # n + 7 and -1 lie outside the row and are ignored
    h = PenaltyHistory([100] * 5 + [n + 7, 17])
    bad = PenaltyHistory([-1])
    entries = [(h, (1.5, 0.0, 1.0), (1.0, 1.0, 3, 77, o)) for o in range(rows - 2)]
    entries += [(bad, (1.0, 1.0, 2.0), (1.0, 1.0, 3, 77, 0)), (None, NO_PENALTIES, (1.0, 1.0, 3, 77, 0))]
    ids, cut, u = launch(logits, entries)
    assert verify(logits, entries, ids, cut, u) == ["sampled"] * rows
    assert {int(i) for i in ids[:rows - 2]} == {200, 300, 400} and set(cut[:rows - 2].tolist()) == {7.0}
    assert float(cut[-1]) == 7.5 and int(ids[-1]) in (100, 200, 300) and int(ids[-2]) == int(ids[-1])
    # the same call twice; another offset, another u
    again = launch(logits, entries)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(again, (ids, cut, u)))
    assert len({float(v) for v in u[:rows - 2]}) == rows - 2
    # empty histories beside total == 0 (no tables at all)
    recs = [e[2] for e in entries]
    empty = [(PenaltyHistory() if r % 2 else None, (1.0, 1.0, 2.0), rec) for r, rec in enumerate(recs)]
    a, b = launch(logits, empty), launch(logits, plain(recs), tables=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # a repetition penalty on a sampled row with top_p: checked like every row
    g = torch.Generator().manual_seed(14)
    rnd = randn3(8, n, dtype, 15)
    entries = [(PenaltyHistory(torch.randint(0, n, (40,), generator=g).tolist()), (0.3, 0.2, 1.7), (0.7, 0.9, 50, 1 << 36, r))
               for r in range(8)]
    ids, cut, u = launch(rnd, entries)
    assert verify(rnd, entries, ids, cut, u) == ["sampled"] * 8


def test_wrapper_refuses_bad_arguments():
    logits = torch.zeros((2, 16), dtype=torch.float16, device=DEV)
    sp = torch.from_numpy(pack_sample_records([GREEDY_RECORD] * 2)).to(DEV)
    hi, hc, cu, pen = pack_penalty_step([(PenaltyHistory([3, 4]), (1.0, 0.0, 1.0)), (None, NO_PENALTIES)]).to_device(DEV)
    assert sample_rows(logits, sp, hi, hc, cu, pen).tolist() == [0, 0]
    E = _lib.HydraHipError
    with pytest.raises(E):
        sample_rows(logits.float(), sp)
    with pytest.raises(E):
        sample_rows(logits[0], sp)
    with pytest.raises(E):
        sample_rows(logits.t(), sp)
    with pytest.raises(E):
        sample_rows(logits, sp[:1])
    with pytest.raises(E):
        sample_rows(logits, sp.float())
    with pytest.raises(E):
        sample_rows(logits, torch.zeros((2, 16), dtype=torch.int32, device=DEV)[:, ::2])
    with pytest.raises(E):
        sample_rows(logits, sp, hi, hc, cu)                                  # three of the four tables
    with pytest.raises(E):
        sample_rows(logits, sp, hi, hc, cu[:2], pen)
    with pytest.raises(E):
        sample_rows(logits, sp, hi, hc, cu, pen.t().contiguous().t())        # non-contiguous
    with pytest.raises(E):
        sample_rows(logits, sp, torch.zeros(4, dtype=torch.int32, device=DEV)[::2], hc, cu, pen)
    with pytest.raises(E):
        sample_rows(logits, sp, out=torch.empty(2, dtype=torch.int32, device=DEV))
    with pytest.raises(E):
        sample_rows(logits, sp, out=torch.empty(3, dtype=torch.int64, device=DEV))
    with pytest.raises(E):
        sample_rows(logits, sp, cut_out=torch.empty(3, device=DEV))
    with pytest.raises(E):
        sample_rows(logits, sp, u_out=torch.empty(2, dtype=torch.float64, device=DEV))
    with pytest.raises(E, match="CPU tensor"):
        sample_rows(logits, sp.cpu())
