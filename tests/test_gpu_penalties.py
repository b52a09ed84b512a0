"""GPU: hx_penalized_argmax_rows / hydrainfer_amd.sampling.penalized_argmax_rows — greedy ids under frequency, presence
and repetition penalties in one launch — against tests/penalty_ref.py (the fp32 restatement of the reference's
process_logits steps 1-2, itself held to the reference's output by test_penalties_cpu.py) and against the reference's own
numbers in tests/golden/g14_penalties.npz."""
import math

import pytest
import torch

from tests import penalty_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
NAN = math.nan


def _ops():
    from hydrainfer_amd._C.kernel.norm import argmax_rows
    from hydrainfer_amd.sampling import penalized_argmax_rows
    return argmax_rows, penalized_argmax_rows


def _csr(hists):
    """hists: per row a list of (token, count).  -> (hist_ids, hist_counts, cu_hist) int32 on the host."""
    ids = [t for h in hists for t, _ in h]
    counts = [c for h in hists for _, c in h]
    cu = [0]
    for h in hists:
        cu.append(cu[-1] + len(h))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return i32(ids), i32(counts), i32(cu)


def _run(logits, hists, penalties, scores=True):
    """(ids, scores) of the op on the host; logits: a device tensor (possibly a strided view)."""
    _, op = _ops()
    hist_ids, hist_counts, cu = _csr(hists)
    pen = torch.tensor(penalties, dtype=torch.float32).reshape(-1, 3)
    s = torch.full((hist_ids.numel(),), -77.0, dtype=torch.float32, device="cuda") if scores else None
    ids = op(logits, hist_ids.cuda(), hist_counts.cuda(), cu.cuda(), pen.cuda(), scores_out=s)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int64 and ids.shape == (logits.shape[0],)
    return ids.cpu(), (s.cpu() if scores else None)


def _same_bits(a, b):
    """fp32 tensors equal bit for bit, any NaN counting as equal to any NaN (payloads are not part of the contract)."""
    a, b = a.float().cpu(), b.float().cpu()
    return a.shape == b.shape and bool((torch.isnan(a) == torch.isnan(b)).all()) \
        and torch.equal(torch.nan_to_num(a, nan=0.0).view(torch.int32), torch.nan_to_num(b, nan=0.0).view(torch.int32))


def _check_against_ref(x, hists, penalties, what, views=None):
    want_ids, want_scores = ref.penalized_batch(x, *_csr(hists), penalties)
    for name, v in (views or {"contiguous": x.cuda()}).items():
        ids, scores = _run(v, hists, penalties)
        assert torch.equal(ids, want_ids), f"{what} {name}: ids {ids.tolist()} != {want_ids.tolist()}"
        assert _same_bits(scores, want_scores), f"{what} {name}: scores differ from the restatement"
    return want_ids, want_scores


def _views(x):
    """x on the device as a contiguous tensor, a strided view (ld > n, ld % 8 == 0, 16-byte aligned: the vector path with
    its n % 8 tail) and a view 2 bytes off a 16-byte boundary (the scalar path); what lies past n would win if read."""
    rows, n = x.shape
    ld = (n + 7) // 8 * 8 + 8
    wide = torch.full((rows, ld), 9.0e3, dtype=x.dtype, device="cuda")
    wide[:, :n] = x
    flat = torch.full((rows * ld + 8,), 9.0e3, dtype=x.dtype, device="cuda")
    off = flat[1:1 + rows * ld].view(rows, ld)
    off[:, :n] = x
    assert wide.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 2
    return {"contiguous": x.cuda(), "strided": wide[:, :n], "unaligned": off[:, :n]}


# ------------------------------------------------------------------------------------------------ empty histories
@pytest.mark.parametrize("n", [1, 7, 8, 63, 1000, 32064, 40000])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_empty_histories_equal_argmax_rows(n, dt):
    """No history: the id is hx_argmax_rows' bit for bit — random rows and a row of equal values, a row with a NaN, a
    row of -inf; contiguous, strided and unaligned logits; with total == 0 (NULL history pointers) and with the empty
    rows inside a batch whose last row has a history."""
    argmax_rows, op = _ops()
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(77 + n)
    special = torch.stack([torch.full((n,), 1.5), (4.0 * torch.randn(n, generator=g)), torch.full((n,), -math.inf)])
    special[1, n // 2] = NAN
    for x in ((4.0 * torch.randn((3, n), generator=g)).to(dtype), special.to(dtype)):
        for name, v in _views(x).items():
            want = argmax_rows(v)
            ids, _ = _run(v, [[], [], []], [(0.5, 0.25, 2.0), (0, 0, 1), (-1.0, 2.0, 0.5)], scores=False)
            assert torch.equal(ids, want.cpu()), f"{dt} n={n} {name}: total == 0"
            ids, _ = _run(v, [[], [], [(0, 1)]], [(0.5, 0.25, 2.0)] * 3)
            assert torch.equal(ids[:2], want.cpu()[:2]), f"{dt} n={n} {name}: empty rows beside a full one"
    assert special[0].to(dtype).unique().numel() == 1 and int(argmax_rows(special.to(dtype).cuda())[1]) == n // 2


# ------------------------------------------------------------------------------------------------ exact answers
def _grid_row(n, fill=-8.0, **at):
    x = torch.full((n,), fill)
    for k, v in at.items():
        x[int(k[1:])] = v
    return x


@pytest.mark.parametrize("n", [16, 1000])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_answers(n, dt):
    """Logits on a 0.25 grid, penalties in {+-0.5, 0.25, 0}, repetition in {0.5, 1, 2, 4}, counts 1..8: every operation
    is exact in fp32, so ids and scores are the restatement's bit for bit whatever the compiler contracts."""
    cases = [
        # the raw winner penalised below the runner-up: (8 - 2 * 0.5 - 0.5) / 2 = 3.25 < 6
        ("winner falls", _grid_row(n, i3=8.0, i5=6.0), [(3, 2)], (0.5, 0.5, 2.0), 5, [3.25]),
        # a negative logit is MULTIPLIED by r: -1 * 4 = -4 < -2
        ("negative times r", _grid_row(n, i2=-1.0, i9=-2.0), [(2, 1)], (0.0, 0.0, 4.0), 9, [-4.0]),
        # ... and with r < 1 a negative logit rises: -4 * 0.5 = -2 > -3
        ("negative times r < 1", _grid_row(n, i2=-4.0, i9=-3.0), [(2, 1)], (0.0, 0.0, 0.5), 2, [-2.0]),
        # a penalised value ties an unpenalised one: the lower index wins, whichever of the two it is
        ("tie, penalised first", _grid_row(n, i4=8.0, i11=3.5), [(4, 2)], (0.25, 0.5, 2.0), 4, [3.5]),
        ("tie, penalised last", _grid_row(n, i4=3.5, i11=8.0), [(11, 2)], (0.25, 0.5, 2.0), 4, [3.5]),
        # count 0: neither frequency nor presence (8 - 0 - 0), repetition all the same: 8 / 2 = 4 < 5
        ("count 0", _grid_row(n, i6=8.0, i1=5.0), [(6, 0)], (0.5, 0.5, 2.0), 1, [4.0]),
        # negative penalties promote: 1 + 4 * 0.5 + 0.5 = 3.5 > 3
        ("promotion", _grid_row(n, i2=1.0, i7=3.0), [(2, 4)], (-0.5, -0.5, 1.0), 2, [3.5]),
        # a penalised NaN stays a NaN and wins; of two NaNs the lower index; a penalised finite beside a plain NaN
        ("penalised NaN", _grid_row(n, i4=NAN, i7=9.0), [(4, 3)], (0.5, 0.25, 2.0), 4, [NAN]),
        ("two NaNs", _grid_row(n, i4=NAN, i9=NAN), [(9, 1)], (0.5, 0.25, 2.0), 4, [NAN]),
        ("plain NaN", _grid_row(n, i4=7.0, i9=NAN), [(4, 8)], (0.5, 0.25, 4.0), 9, [0.6875]),
        # every entry of the row in the history
        ("whole row", torch.arange(n, dtype=torch.float32) * 0.25 - 2.0, [(t, 1 + t % 8) for t in range(n)],
         (0.25, -0.5, 2.0), None, None),
    ]
    x = torch.stack([c[1] for c in cases]).to(DTYPES[dt])
    hists, pens = [c[2] for c in cases], [c[3] for c in cases]
    want_ids, want_scores = _check_against_ref(x, hists, pens, f"{dt} n={n}", _views(x))
    at = 0
    for (name, _, h, _, wid, ws), got in zip(cases, want_ids.tolist()):
        if wid is not None:
            assert got == wid, f"{name}: the restatement itself gives {got}, worked out by hand {wid}"
            assert _same_bits(want_scores[at:at + len(h)], torch.tensor(ws)), name
        at += len(h)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_answers_random_grid(dt):
    """The same exact arithmetic over random rows full of ties (65 distinct values in a 1000 / 32064-wide row)."""
    g = torch.Generator().manual_seed(11)
    pick = lambda vals: vals[int(torch.randint(0, len(vals), (1,), generator=g))]
    for n, rows in ((1000, 8), (32064, 4)):
        x = (torch.randint(-32, 33, (rows, n), generator=g) * 0.25).to(DTYPES[dt])
        hists, pens = [], []
        for r in range(rows):
            h = int(torch.randint(0, 301, (1,), generator=g)) if r else 300
            toks = torch.randperm(n, generator=g)[:h].tolist()
            top = torch.nonzero(x[r] == x[r].max()).flatten().tolist()[:5]       # the raw winners go into the history
            toks = list(dict.fromkeys(top + toks))[:max(h, len(top))] if r % 2 == 0 else toks
            hists.append([(t, int(torch.randint(1, 9, (1,), generator=g))) for t in toks])
            pens.append((pick([0.5, -0.5, 0.25, 0.0]), pick([0.5, -0.5, 0.25, 0.0]), pick([0.5, 1.0, 2.0, 4.0])))
        want_ids, _ = _check_against_ref(x, hists, pens, f"{dt} n={n}")
        raw = x.float().argmax(-1)
        assert int((want_ids != raw).sum()) >= 1, "no penalty changed a token: the case shows nothing"


# ------------------------------------------------------------------------------------------------ the reference's numbers
def _ulp(m: float) -> float:
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 else 2.0 ** -149


def test_golden_fixture():
    """Every row of g14_penalties.npz (the reference's process_logits, row by row).  The issue's acceptance bound is 4
    fp32 ulps of the largest intermediate magnitude (|x| + c |f| + |p|) max(r, 1/r) per entry; the kernel keeps its
    operations uncontracted and its division correctly rounded, and on an MI355X every score came out bit-equal to the
    reference, so the test asks for EQUALITY: scores bit for bit, ids the reference's argmax."""
    rows = ref.load_golden()
    n_scores = 0
    for n in sorted({r["n"] for r in rows}):
        group = [r for r in rows if r["n"] == n]
        x = torch.stack([r["logits"] for r in group])
        hists = [list(zip(r["ids"], r["counts"])) for r in group]
        ids, scores = _run(x.cuda(), hists, [r["penalties"] for r in group])
        at = 0
        for k, r in enumerate(group):
            h = len(r["ids"])
            got = scores[at:at + h]
            at += h
            f, p, rep = r["penalties"]
            worst, row_bound = 0.0, 0.0
            for j in range(h):
                m = (abs(float(r["logits"][r["ids"][j]])) + r["counts"][j] * abs(f) + abs(p)) * max(rep, 1.0 / rep)
                err = abs(float(got[j]) - float(r["scores"][j]))
                worst, row_bound = max(worst, err / _ulp(m)), max(row_bound, 4 * _ulp(m))
                assert err <= 4 * _ulp(m), f"n={n} row {k} entry {j}: {float(got[j])!r} vs {float(r['scores'][j])!r}"
            # the reference's value at the id the kernel chose, against the reference's maximum
            chosen = int(ids[k])
            value = float(r["scores"][r["ids"].index(chosen)]) if chosen in r["ids"] else float(r["logits"][chosen])
            assert abs(value - r["max"]) <= row_bound, f"n={n} row {k}: id {chosen}"
            print(f"n={n} h={h}: worst score error {worst:.2f} ulp, id {chosen} (reference {r['best']}, raw {r['raw_best']})")
            assert _same_bits(got, r["scores"]), f"n={n} row {k}: scores not bit-equal to the reference"
            assert chosen == r["best"], f"n={n} row {k}: id {chosen}, the reference's argmax is {r['best']}"
            n_scores += h
    assert n_scores > 1000


# ------------------------------------------------------------------------------------------------ bounds
def test_outputs_are_written_inside_their_bounds():
    """The C entry point on outputs with canaries all round; history ids of -1 and n are ignored (NaN in scores_out, the
    answer of the same row without them); a history longer than the workgroup (3000 entries at n = 32064); a batch
    mixing empty and full histories."""
    from hydrainfer_amd import _lib
    rows, n, pad = 5, 32064, 64
    g = torch.Generator().manual_seed(5)
    x = (4.0 * torch.randn((rows + 1, n), generator=g)).to(torch.bfloat16)
    top = x.float().topk(40, dim=-1).indices
    long = list(dict.fromkeys(top[1].tolist() + torch.randperm(n, generator=g)[:3000].tolist()))[:3000]
    clean = [[], [(t, 1 + i % 8) for i, t in enumerate(long)], [(t, 2) for t in top[2].tolist()], [],
             [(int(top[4, 0]), 3)]]
    dirty = [list(h) for h in clean]
    dirty[2] = [(-1, 5)] + dirty[2][:7] + [(n, 1)] + dirty[2][7:] + [(n + 1000, 2), (-(2 ** 31), 1), (2 ** 31 - 1, 1)]
    dirty[3] = [(n, 4), (-1, 4)]
    pens = [(0.5, 0.5, 2.0), (1.0, 0.25, 1.5), (1.0, 0.0, 1.5), (0.5, 0.5, 2.0), (0.0, 3.0, 1.0)]
    want_ids, want_scores = ref.penalized_batch(x[:rows], *_csr(dirty), pens)
    clean_ids, _ = ref.penalized_batch(x[:rows], *_csr(clean), pens)
    assert torch.equal(want_ids, clean_ids) and want_ids[0] == top[0, 0] and want_ids[3] == top[3, 0]
    assert all(int(want_ids[r]) != int(top[r, 0]) for r in (1, 2, 4)), "the full histories must move their rows' tokens"
    hist_ids, hist_counts, cu = (t.cuda() for t in _csr(dirty))
    total = hist_ids.numel()
    bufs = {"ids": torch.full((rows + 2 * pad,), -77, dtype=torch.int64, device="cuda"),
            "scores": torch.full((total + 2 * pad,), -77.0, dtype=torch.float32, device="cuda")}
    xd, pen = x.cuda(), torch.tensor(pens, dtype=torch.float32).cuda()
    _lib.check(_lib.lib().hx_penalized_argmax_rows(
        bufs["ids"][pad:].data_ptr(), bufs["scores"][pad:].data_ptr(), xd.data_ptr(), rows, n, xd.stride(0),
        hist_ids.data_ptr(), hist_counts.data_ptr(), cu.data_ptr(), total, pen.data_ptr(), _lib.HX_BF16,
        _lib.current_stream()), "penalized_argmax_rows")
    torch.cuda.synchronize()
    for name, b, inner in (("ids", bufs["ids"], rows), ("scores", bufs["scores"], total)):
        assert bool((b[:pad] == -77).all()) and bool((b[pad + inner:] == -77).all()), f"{name}: canary overwritten"
    assert torch.equal(bufs["ids"][pad:pad + rows].cpu(), want_ids)
    got = bufs["scores"][pad:pad + total].cpu()
    assert _same_bits(got, want_scores) and int(torch.isnan(got).sum()) == 7
    # scores_out NULL: nothing but ids is written; a cu_hist that points past `total` is held inside it
    bufs["ids"].fill_(-77)
    bad_cu = cu.clone()
    bad_cu[-1] = total + 100000
    _lib.check(_lib.lib().hx_penalized_argmax_rows(
        bufs["ids"][pad:].data_ptr(), None, xd.data_ptr(), rows, n, xd.stride(0), hist_ids.data_ptr(),
        hist_counts.data_ptr(), bad_cu.data_ptr(), total, pen.data_ptr(), _lib.HX_BF16, _lib.current_stream()),
        "penalized_argmax_rows")
    torch.cuda.synchronize()
    assert torch.equal(bufs["ids"][pad:pad + rows].cpu(), want_ids)
    assert bool((bufs["ids"][:pad] == -77).all()) and bool((bufs["ids"][pad + rows:] == -77).all())


def test_refusals_launch_nothing():
    from hydrainfer_amd import _lib
    _, op = _ops()
    good = torch.zeros((2, 16), dtype=torch.float16, device="cuda")
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    pen = torch.tensor([[0.5, 0.5, 2.0]] * 2, device="cuda")
    args = (i32(3), i32(1), i32(0, 1, 1), pen)
    assert op(good, *args).tolist() == [0, 0]
    for bad in ((good.float(),) + args, (good[0],) + args, (good.t(),) + args, (good.cpu(),) + args,
                (good, i32(3).long(), i32(1), i32(0, 1, 1), pen), (good, i32(3), i32(1, 1), i32(0, 1, 1), pen),
                (good, i32(3), i32(1), i32(0, 1), pen), (good, i32(3), i32(1), i32(0, 1, 1), pen[:1]),
                (good, i32(3), i32(1), i32(0, 1, 1), pen.double()), (good, i32(3), i32(1), i32(0, 1, 1).cpu(), pen)):
        with pytest.raises(_lib.HydraHipError):
            op(*bad)
    with pytest.raises(_lib.HydraHipError):
        op(good, *args, out=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(_lib.HydraHipError):
        op(good, *args, scores_out=torch.zeros(2, dtype=torch.float32, device="cuda"))
    with pytest.raises(_lib.HydraHipError):
        op(torch.zeros((1, (1 << 18) + 8), dtype=torch.float16, device="cuda"), i32(3), i32(1), i32(0, 1), pen[:1])
    # the C entry point itself: an error code for every bad argument, and the outputs keep their canaries
    out = torch.full((64,), -77, dtype=torch.int64, device="cuda")
    f = _lib.lib().hx_penalized_argmax_rows
    s, p, q, F16 = _lib.current_stream(), out.data_ptr(), good.data_ptr(), _lib.HX_F16
    h, c, cu, pn = (t.data_ptr() for t in args)
    assert f(p, p, q, 0, 16, 16, h, c, cu, 1, pn, F16, s) == -2 and f(p, p, q, 2, 0, 16, h, c, cu, 1, pn, F16, s) == -2
    assert f(p, p, q, 2, 16, 8, h, c, cu, 1, pn, F16, s) == -2 and f(p, p, q, 2, 16, 16, h, c, cu, -1, pn, F16, s) == -2
    assert f(p, p, q, 1, (1 << 18) + 1, 1 << 19, h, c, cu, 1, pn, F16, s) == -2
    assert f(p, p, q, 2, 16, 16, h, c, cu, 1, pn, _lib.HX_F32, s) == -1
    assert f(None, p, q, 2, 16, 16, h, c, cu, 1, pn, F16, s) == -4 and f(p, p, None, 2, 16, 16, h, c, cu, 1, pn, F16, s) == -4
    assert f(p, p, q, 2, 16, 16, None, c, cu, 1, pn, F16, s) == -4 and f(p, p, q, 2, 16, 16, h, None, cu, 1, pn, F16, s) == -4
    assert f(p, p, q, 2, 16, 16, h, c, None, 1, pn, F16, s) == -4 and f(p, p, q, 2, 16, 16, h, c, cu, 1, None, F16, s) == -4
    torch.cuda.synchronize()
    assert bool((out == -77).all())
    # total == 0 with NULL history pointers is legal: plain argmax
    zero_cu = i32(0, 0, 0)
    assert f(p, None, q, 2, 16, 16, None, None, zero_cu.data_ptr(), 0, pn, F16, s) == 0
    torch.cuda.synchronize()
    assert out[:2].tolist() == [0, 0] and bool((out[2:] == -77).all())


def test_widest_row():
    """n = 2^18, the widest row the bitmap takes: the last element, penalised and not."""
    n = 1 << 18
    x = torch.zeros((2, n), dtype=torch.float16)
    x[:, n - 1] = 4.0
    x[:, 5] = 3.0
    ids, scores = _run(x.cuda(), [[(n - 1, 2)], [(5, 1)]], [(0.5, 0.5, 2.0)] * 2)
    assert ids.tolist() == [5, n - 1] and scores.tolist() == [1.25, 1.0]
