"""GPU: hx_sample_rows_resident_penalized (csrc/sampling.hip) against hx_sample_rows.  A row that names a slot of the
resident token log is penalised over the slot's first L words — L = offset_base + position — and writes its id as word L.
For the same logits, the CSR (distinct ids, counts) of that prefix built HERE on the host, the same penalties and a record
that carries L as its explicit offset, hx_sample_rows gives the ids, the cut and u that the new launch must give BIT FOR
BIT (int32 views, NaN cuts included).  A launch holds a penalised greedy row, a penalised row with top-k and top-p, a row
without a slot (hx_sample_rows_resident's, bit for bit) and a penalised row with a temperature only; the prefixes are a
small pool with repeats and the ids -1 and n among them, one token L times, and L distinct tokens.  The log is compared as
a WHOLE table after every launch: word L of a row's slot changed, nothing else — sentinel slots lie between the rows'."""
from collections import Counter

import numpy as np
import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd.sampling import (SAMPLE_LOG_MAX, SAMPLE_MAX_N, pack_penalty_records, pack_resident_records,
                                     pack_sample_records, sample_rows, sample_rows_resident,
                                     sample_rows_resident_penalized)
from tests import penalty_ref
from tests import sampling_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
HX_ERR_DTYPE, HX_ERR_SHAPE, HX_ERR_NULL = -1, -2, -4
SENTINEL = -12345
LOG_CAP, LOG_SLOTS = 2048, 8
# (temperature, top_p, top_k, seed) per row, None = greedy; the penalties; the slots (odd: the even ones are sentinels)
SAMPLING = [None, (0.8, 0.9, 20, (1 << 40) + 3), (1.1, 0.8, 50, 5), (0.9, 1.0, 0, (1 << 63) - 1)]
PENALTIES = [(0.7, 0.5, 1.3), (0.4, 0.0, 1.0), None, (0.0, 0.6, 1.2)]
SLOTS = [1, 3, -1, 5]
POSITIONS = [7, 300, 2, 1500]


def prefixes(n, L, g):
    """row 0: a pool of eight tokens with repeats, the ids -1 and n among them; row 1: one token L times; row 3: L distinct"""
    pool = torch.randint(0, n, (8,), generator=g).tolist()
    mixed = [pool[i] for i in torch.randint(0, 8, (L,), generator=g).tolist()]
    if L >= 2:
        mixed[0] = mixed[1]                     # (L = 2: a repeated token)
    if L >= 4:
        mixed[2], mixed[L - 1] = -1, n
    one = [int(torch.randint(0, n, (1,), generator=g))] * L
    perm = torch.randperm(n, generator=g).tolist()
    distinct = (perm + perm)[:L]                # (pairwise distinct while L <= n; a second round of them past that)
    return [mixed, one, None, distinct]


def make_log(n, prefix, g, cap=LOG_CAP, slots=SLOTS, n_slots=LOG_SLOTS):
    """the table: sentinel slots, and in a row's slot its prefix followed by valid tokens that the launch must not read"""
    log = torch.full((n_slots, cap), SENTINEL, dtype=torch.int32)
    for s, p in zip(slots, prefix):
        if s >= 0:
            log[s] = torch.randint(0, n, (cap,), generator=g, dtype=torch.int32)
            k = min(len(p), cap)
            log[s, :k] = torch.tensor(p[:k], dtype=torch.int32)
    return log


def reference(logits, sampling, penalties, prefix, Ls, cap=LOG_CAP):
    """hx_sample_rows over the CSR of each row's prefix [0, min(max(L, 0), cap)) and the explicit offset L mod 2^64 ->
    (ids, cut, u as int32 views on the host, the rows' (ids, counts))"""
    rows = logits.shape[0]
    tables = []
    for p, L in zip(prefix, Ls):
        c = Counter(p[:min(max(L, 0), cap)]) if p is not None else {}
        tables.append((list(c), list(c.values())))
    cu = np.cumsum([0] + [len(t[0]) for t in tables]).astype(np.int32)
    hist_ids = torch.tensor([t for ids, _ in tables for t in ids], dtype=torch.int32, device=DEV)
    hist_counts = torch.tensor([c for _, counts in tables for c in counts], dtype=torch.int32, device=DEV)
    pen = torch.tensor([p if p is not None else (0.0, 0.0, 1.0) for p in penalties], dtype=torch.float32, device=DEV)
    recs = [(0.0, 1.0, 0, 0, L % (1 << 64)) if s is None else s + (L % (1 << 64),) for s, L in zip(sampling, Ls)]
    cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2))
    ids = sample_rows(logits, torch.from_numpy(pack_sample_records(recs)).to(DEV), hist_ids, hist_counts,
                      torch.from_numpy(cu).to(DEV), pen, cut_out=cut, u_out=u)
    return [t.cpu().view(torch.int32) for t in (ids, cut, u)], tables, recs


def launch(logits, sampling, penalties, slots, Ls, positions, log):
    """the new launch -> (ids, cut, u as int32 views on the host); `log` (a device tensor) is updated in place"""
    rows = logits.shape[0]
    records = [None if s is None and p is None else (s or (0.0, 1.0, 0, 0)) + (L - pos,)
               for s, p, L, pos in zip(sampling, penalties, Ls, positions)]
    resident = torch.from_numpy(pack_resident_records(records)).to(DEV)
    pen = torch.from_numpy(pack_penalty_records([None if p is None else p + (s,) for p, s in zip(penalties, slots)])).to(DEV)
    pos = torch.tensor(positions, dtype=torch.int32, device=DEV)
    cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2))
    ids = sample_rows_resident_penalized(logits, resident, pos, pen, log, cut_out=cut, u_out=u)
    return [t.cpu().view(torch.int32) for t in (ids, cut, u)], (resident, pos)


def padded(host, pad):
    rows, n = host.shape
    wide = torch.zeros(rows, n + pad, dtype=host.dtype)
    wide[:, :n] = host
    return wide.to(DEV)[:, :n]


@pytest.mark.parametrize("n", [1000, 32064])               # the scalar staging path (ld % 8 != 0); the product's vocabulary
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bit_for_bit_with_sample_rows_over_the_log_prefix(dtype, n):
    g = torch.Generator().manual_seed(n)
    logits = padded((torch.randn(4, n, generator=g) * 3).to(dtype), 8 if n == 32064 else 3)
    host = logits.cpu()
    checked = set()
    for L in (0, 1, 2, 63, 64, 65, 1023, 1024, 1025):
        prefix = prefixes(n, L, g)
        before = make_log(n, prefix, g)
        log = before.to(DEV)
        Ls = [L, L, 9, L]                       # (row 2 has no slot: its offset is just a number)
        want, tables, recs = reference(logits, SAMPLING, PENALTIES, prefix, Ls)
        got, (resident, pos) = launch(logits, SAMPLING, PENALTIES, SLOTS, Ls, POSITIONS, log)
        for name, a, b in zip(("ids", "cut", "u"), got, want):
            assert torch.equal(a, b), f"L {L} {name}: {a.tolist()} != sample_rows {b.tolist()}"
        ids = got[0].view(torch.int64)
        # the row without a slot: hx_sample_rows_resident's, bit for bit
        c, uu = (torch.full((4,), 7.0, device=DEV) for _ in range(2))
        plain = sample_rows_resident(logits, resident, pos, cut_out=c, u_out=uu)
        assert int(ids[2]) == int(plain[2]) and int(got[1][2]) == int(c.cpu().view(torch.int32)[2]) \
            and int(got[2][2]) == int(uu.cpu().view(torch.int32)[2])
        # the write: word L of each row's slot, nothing else in the whole table
        after = before.clone()
        for r, s in enumerate(SLOTS):
            if s >= 0:
                after[s, L] = int(ids[r])
        assert torch.equal(log.cpu(), after), f"L {L}: the log differs outside word L of the rows' slots"
        # a second identical launch: the same ids, the same table
        again, _ = launch(logits, SAMPLING, PENALTIES, SLOTS, Ls, POSITIONS, log)
        assert all(torch.equal(a, b) for a, b in zip(again, got)) and torch.equal(log.cpu(), after)
        # the independent reference: a greedy and a sampled row, at a short and a long prefix
        if L in (65, 1025):
            cut, u = got[1].view(torch.float32), got[2].view(torch.float32)
            for r in (0, 1):
                kind = ref.check_row(host[r], tables[r][0], tables[r][1], PENALTIES[r], recs[r], int(ids[r]), float(cut[r]),
                                     np.float32(u[r].item()), f"L {L} row {r}")
                assert kind == ("greedy" if r == 0 else "sampled")
                checked.add(kind)
    assert checked == {"greedy", "sampled"}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_only_the_frequency_term_decides(dtype):
    """tokens a > b, x_a = 8, x_b = 7.5, everything else below 4; the log holds a three times and b twice, f = 0.5:
    8 - 1.5 = 7.5 - 1.0, a tie that the lower index b wins — a count of a that is one short gives a, one of b that is one
    long gives a"""
    n, a, b = 1000, 700, 300
    g = torch.Generator().manual_seed(5)
    host = torch.randn(4, n, generator=g).clamp(max=3.0)
    host[0, a], host[0, b] = 8.0, 7.5
    logits = padded(host.to(dtype), 3)
    prefix = [[a, b, a, b, a], [a] * 5, None, [1, 2, 3, 4, 5]]
    penalties = [(0.5, 0.0, 1.0)] + PENALTIES[1:]
    before = make_log(n, prefix, g)
    log = before.to(DEV)
    Ls = [5, 5, 9, 5]
    want, tables, recs = reference(logits, SAMPLING, penalties, prefix, Ls)
    got, _ = launch(logits, SAMPLING, penalties, SLOTS, Ls, POSITIONS, log)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert int(got[0].view(torch.int64)[0]) == b
    assert penalty_ref.penalized_row(logits.cpu()[0], tables[0][0], tables[0][1], *penalties[0])[2] == b
    assert int(log[1, 5]) == b
    # one occurrence of a fewer: a wins
    log = make_log(n, [[a, b, a, b, 7], [a] * 5, None, [1, 2, 3, 4, 5]], g).to(DEV)
    got, _ = launch(logits, SAMPLING, penalties, SLOTS, Ls, POSITIONS, log)
    assert int(got[0].view(torch.int64)[0]) == a


@pytest.mark.parametrize("L", [-1, 64, 70], ids=["before_the_log", "at_the_cap", "past_the_cap"])
def test_outside_the_log_nothing_is_written(L):
    """log_cap = 64: L = -1 has an empty history (and the offset 2^64 - 1), L = 64 and 70 the whole row; none of them
    writes, and no word of the table changes — sentinel slots on both sides of every row's"""
    n, cap = 1000, 64
    g = torch.Generator().manual_seed(100 + L)
    logits = padded((torch.randn(4, n, generator=g) * 3).to(torch.bfloat16), 3)
    prefix = prefixes(n, 80, g)
    before = make_log(n, prefix, g, cap=cap)
    log = before.to(DEV)
    Ls = [L, L, 9, L]
    want, _, _ = reference(logits, SAMPLING, PENALTIES, prefix, Ls, cap=cap)
    got, _ = launch(logits, SAMPLING, PENALTIES, SLOTS, Ls, POSITIONS, log)
    for name, a, b in zip(("ids", "cut", "u"), got, want):
        assert torch.equal(a, b), f"{name}: {a.tolist()} != sample_rows {b.tolist()}"
    assert torch.equal(log.cpu(), before)
    if L == -1:
        assert np.float32(got[2].view(torch.float32)[1].item()).view(np.uint32) == \
            ref.uniform(SAMPLING[1][3], (1 << 64) - 1).view(np.uint32)
    # a slot past the table is no slot: nothing is read or written, the rows are the resident launch's
    got, (resident, pos) = launch(logits, SAMPLING, PENALTIES, [LOG_SLOTS, -5, -1, 1 << 30], [3, 3, 9, 3], POSITIONS, log)
    plain = sample_rows_resident(logits, resident, pos)
    assert got[0].view(torch.int64).tolist() == plain.tolist() and torch.equal(log.cpu(), before)


def test_errors_launch_nothing():
    rows, n = 2, 64
    logits = torch.zeros(rows, n, dtype=torch.bfloat16, device=DEV)
    sp = torch.from_numpy(pack_resident_records([(1.0, 1.0, 0, 1, 0)] * rows)).to(DEV)
    pen = torch.from_numpy(pack_penalty_records([(0.5, 0.5, 1.2, 0), (0.5, 0.5, 1.2, 1)])).to(DEV)
    pos = torch.zeros(rows, dtype=torch.int32, device=DEV)
    log = torch.full((2, 16), SENTINEL, dtype=torch.int32, device=DEV)
    ids = torch.full((rows,), -77, dtype=torch.int64, device=DEV)
    cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2))
    fn, stream = _lib.lib().hx_sample_rows_resident_penalized, _lib.current_stream()

    def call(rows_=rows, n_=n, ld=n, positions=pos.data_ptr(), penalty=pen.data_ptr(), token_log=log.data_ptr(), slots=2,
             cap=16, dtype=_lib.HX_BF16, sample_params=sp.data_ptr()):
        return fn(ids.data_ptr(), cut.data_ptr(), u.data_ptr(), logits.data_ptr(), rows_, n_, ld, sample_params, positions,
                  penalty, token_log, slots, cap, dtype, stream)
    assert call(positions=None) == HX_ERR_NULL
    assert call(penalty=None) == HX_ERR_NULL
    assert call(token_log=None) == HX_ERR_NULL
    assert call(sample_params=None) == HX_ERR_NULL
    assert call(slots=0) == HX_ERR_SHAPE
    assert call(cap=0) == HX_ERR_SHAPE
    assert call(cap=SAMPLE_LOG_MAX + 1) == HX_ERR_SHAPE
    assert call(n_=SAMPLE_MAX_N + 1, ld=SAMPLE_MAX_N + 1) == HX_ERR_SHAPE
    assert call(rows_=0) == HX_ERR_SHAPE
    assert call(dtype=_lib.HX_F32) == HX_ERR_DTYPE
    torch.cuda.synchronize()
    assert ids.tolist() == [-77] * rows and cut.tolist() == [7.0] * rows and u.tolist() == [7.0] * rows
    assert (log == SENTINEL).all()
    assert SAMPLE_LOG_MAX >= 2048
    assert call() == 0
    torch.cuda.synchronize()
    assert all(0 <= t < n for t in ids.tolist()) and log[:, 0].tolist() == ids.tolist() and (log[:, 1:] == SENTINEL).all()
    # the shim refuses what the entry would
    with pytest.raises(_lib.HydraHipError):
        sample_rows_resident_penalized(logits, sp, pos, pen[:, :3].contiguous(), log)
    with pytest.raises(_lib.HydraHipError):
        sample_rows_resident_penalized(logits, sp, pos, pen, log.long())
    with pytest.raises(_lib.HydraHipError):
        sample_rows_resident_penalized(logits, sp, pos, pen, torch.zeros(2, SAMPLE_LOG_MAX + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.HydraHipError):
        sample_rows_resident_penalized(logits, sp, pos.long(), pen, log)


def test_captured_at_the_product_vocabulary():
    """n = 32064 needs 125 KiB of dynamic LDS: the limit is raised by a launch outside the capture; the captured launch
    replays step after step, each one reading what the one before appended"""
    n, L0 = 32064, 3
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(4, n, generator=g) * 3).to(torch.bfloat16).to(DEV)
    prefix = prefixes(n, L0, g)
    log = make_log(n, prefix, g).to(DEV)
    start = log.clone()
    records = [(s or (0.0, 1.0, 0, 0)) + (L0 - p,) for s, p in zip(SAMPLING, POSITIONS)]
    resident = torch.from_numpy(pack_resident_records(records)).to(DEV)
    pen = torch.from_numpy(pack_penalty_records([None if p is None else p + (s,) for p, s in zip(PENALTIES, SLOTS)])).to(DEV)
    pos = torch.tensor(POSITIONS, dtype=torch.int32, device=DEV)
    ids = torch.zeros(4, dtype=torch.int64, device=DEV)
    cut, u = (torch.zeros(4, device=DEV) for _ in range(2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sample_rows_resident_penalized(logits, resident, pos, pen, log, out=ids, cut_out=cut, u_out=u)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sample_rows_resident_penalized(logits, resident, pos, pen, log, out=ids, cut_out=cut, u_out=u)
    log.copy_(start)
    for step in range(3):
        pos.copy_(torch.tensor([p + step for p in POSITIONS], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        L = L0 + step
        want, _, _ = reference(logits, SAMPLING, PENALTIES, prefix, [L, L, L, L])
        for a, b in zip((ids, cut, u), want):
            assert torch.equal(a.cpu().view(torch.int32), b), f"step {step}"
        for r, s in enumerate(SLOTS):
            if s >= 0:
                assert int(log[s, L]) == int(ids[r])
                prefix[r] = prefix[r] + [int(ids[r])]
