"""GPU: hx_token_logprob_rows / _C.kernel.norm.token_logprob_rows — the log-probability of a GIVEN token per row, its
rank and the row's top-K list in one launch — against the float64 reference of tests/token_logprob_ref.py.  Ranks and
ids are exact (the order is part of the contract); log-probabilities are held to logprob_ref.ATOL.  Every case runs the
form the entry point picks and both forms by name (hx_token_logprob_rows_ex): the pass from global memory and the row
staged in LDS."""
import math

import pytest
import torch

from tests.token_logprob_ref import assert_logprobs_close, token_reference

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
KS = (0, 1, 5, 20)
FORMS = (0, 1, 2)
POISON = -77


def _ops():
    from hydrainfer_amd._C.kernel.norm import logprob_rows, token_logprob_rows
    return logprob_rows, token_logprob_rows


def _views(x):
    """The same logits as a contiguous tensor, a strided view (ld > n, ld % 8 == 0, 16-byte aligned: the vector path,
    with its n % 8 tail) and a view with ld > n whose base is one element off a 16-byte boundary (the scalar path)."""
    rows, n = x.shape
    ld = (n + 7) // 8 * 8 + 8
    wide = torch.full((rows, ld), 9.0e3, dtype=x.dtype, device="cuda")        # what lies past n would win if it were read
    wide[:, :n] = x
    flat = torch.full((rows * ld + 8,), 9.0e3, dtype=x.dtype, device="cuda")
    off = flat[1:1 + rows * ld].view(rows, ld)
    off[:, :n] = x
    assert wide.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 2
    return {"contiguous": x.cuda(), "strided": wide[:, :n], "unaligned": off[:, :n]}


def _check(logits, targets, top_k, ref, what, form=0):
    _, token_logprob_rows = _ops()
    lp, ranks, top_ids, top_lp = token_logprob_rows(logits, targets, top_k, form=form)
    torch.cuda.synchronize()
    rows = logits.shape[0]
    assert lp.dtype == torch.float32 and lp.shape == (rows,) and ranks.dtype == torch.int32 and ranks.shape == (rows,)
    assert top_ids.dtype == torch.int32 and top_ids.shape == (rows, top_k)
    assert top_lp.dtype == torch.float32 and top_lp.shape == (rows, top_k)
    r_lp, r_ranks, r_top_ids, r_top_lp = ref
    assert torch.equal(ranks.cpu().long(), r_ranks), f"{what}: ranks differ from the reference"
    assert torch.equal(top_ids.cpu().long(), r_top_ids[:, :top_k]), f"{what}: top ids / their order differ"
    e1 = assert_logprobs_close(lp, r_lp, what)
    e2 = assert_logprobs_close(top_lp, r_top_lp[:, :top_k], what + " (top)")
    return max(e1, e2)


def _targets(rows, n, g):
    """Random ids; row 0 asks for id 0, the last row for id n - 1, and of three or more rows the second is not scored."""
    t = torch.randint(0, n, (rows,), generator=g, dtype=torch.int32)
    t[0] = 0
    t[rows - 1] = n - 1
    if rows >= 3:
        t[1] = -1 if n % 2 else n
    return t


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1023, 1025, 24576, 24584, 32064, 65536, 65537])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_shape_grid(n, dt):
    """n: below / at / past a 16-byte piece, below / past one piece per thread, a staged row of exactly 48 KiB and the
    first past it, which needs the kernel's dynamic LDS limit raised (24576, 24584), the vocabulary, the widest row that
    is staged in LDS and the first that is not; rows 1, 3, 70; K 0, 1, 5, 20 (K > n for the small ones); three layouts;
    three forms."""
    worst = 0.0
    for rows in (1, 3, 70):
        g = torch.Generator().manual_seed(1000 * rows + n)
        x = (4.0 * torch.randn((rows, n), generator=g)).to(DTYPES[dt])
        t = _targets(rows, n, g)
        ref = token_reference(x, t, max(KS))
        td = t.cuda()
        for name, v in _views(x).items():
            for k in KS:
                for form in FORMS:
                    worst = max(worst, _check(v, td, k, ref, f"{dt} n={n} rows={rows} K={k} {name} form={form}", form))
    print(f"{dt} n={n}: max |logprob error| {worst:.2e}")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_ties_and_nans(dt):
    """Rows drawn from 5 distinct 16-bit values: every rank and every top entry is decided by the index.  Then the same
    rows with NaNs sprinkled in: a NaN comes before every number."""
    n, rows = 32064, 6
    g = torch.Generator().manual_seed(11)
    vals = torch.tensor([0.25, -3.0, 2.5, 2.484375, -math.inf]).to(DTYPES[dt])
    x = vals[torch.randint(0, 5, (rows, n), generator=g)]
    x[1, :9000] = vals[1]                       # the largest value's first occurrences lie deep in the row
    t = torch.randint(0, n, (rows,), generator=g, dtype=torch.int32)
    t[2] = int((x[2] == vals[2]).nonzero()[0])  # the greedy id itself
    t[3] = int((x[3] == vals[4]).nonzero()[-1])  # the last -inf: the largest rank there is, or nearly
    x[4, [5, 20000, 32063]] = math.nan
    x[5, 31000] = math.nan
    t[5] = 31000                                # a NaN target: rank 0
    ref = token_reference(x, t, 20)
    assert int(ref[1][2]) == 0 and int(ref[1][5]) == 0 and int(ref[1][3]) > n // 2 and float(ref[0][3]) == -math.inf
    assert bool(torch.isnan(ref[0][4:]).all())
    for k in KS:
        for form in FORMS:
            _check(x.cuda(), t.cuda(), k, ref, f"{dt} five values K={k} form={form}", form)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_edge_rows(dt):
    """Rows of all -inf, rows with one +inf, targets at 0, n - 1, a -inf entry and a NaN entry; ordinary rows between
    them must not notice."""
    n, dtype = 1025, DTYPES[dt]
    g = torch.Generator().manual_seed(3)
    noise = lambda: (4.0 * torch.randn(n, generator=g)).to(dtype)
    x = torch.stack([noise(), torch.full((n,), -math.inf, dtype=dtype), noise(), noise(), noise(), noise(), noise(),
                     torch.full((n,), -math.inf, dtype=dtype), noise()])
    x[3, 500] = math.inf                        # one +inf, asked for itself
    x[4, 500] = math.inf                        # one +inf, a finite entry asked for
    x[5, 77] = -math.inf                        # a -inf target in an ordinary row
    x[6, 900] = math.nan                        # a NaN target
    x[7, [5, 1000]] = torch.tensor([1.0, 2.0]).to(dtype)      # -inf except two entries
    t = torch.tensor([0, 3, n - 1, 500, 7, 77, 900, 1000, 0], dtype=torch.int32)
    ref = token_reference(x, t, 5)
    assert math.isnan(float(ref[0][1])) and math.isnan(float(ref[0][3])) and math.isnan(float(ref[0][4]))
    assert float(ref[0][5]) == -math.inf and math.isnan(float(ref[0][6])) and int(ref[1][6]) == 0
    assert abs(float(ref[0][7]) - (2 - math.log(math.e + math.e ** 2))) < 1e-9 and int(ref[1][7]) == 0
    for k in (0, 5):
        for form in FORMS:
            _check(x.cuda(), t.cuda(), k, ref, f"{dt} edge rows K={k} form={form}", form)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_greedy_targets_have_rank_zero_and_the_same_top_lists(dt):
    logprob_rows, token_logprob_rows = _ops()
    g = torch.Generator().manual_seed(17)
    x = (4.0 * torch.randn((9, 32064), generator=g)).to(DTYPES[dt]).cuda()
    x[2] = 1.5                                  # ties everywhere
    for k in (0, 5, 20):
        ids, lp, top_ids, top_lp = logprob_rows(x, k)
        for form in FORMS:
            t_lp, ranks, t_top_ids, t_top_lp = token_logprob_rows(x, ids.to(torch.int32), k, form=form)
            assert bool((ranks == 0).all()), f"{dt} K={k} form={form}: the greedy id does not have rank 0"
            assert torch.equal(t_top_ids, top_ids), f"{dt} K={k} form={form}: top ids differ from logprob_rows'"
            if k:
                # K > 0 repeats hx_logprob_rows' sum term for term, in every form: bit for bit, not merely close
                assert torch.equal(t_top_lp, top_lp), f"{dt} K={k} form={form}: top logprobs differ from logprob_rows'"
                assert torch.equal(t_lp, lp), f"{dt} K={k} form={form}: the greedy id's logprob differs from logprob_rows'"
            else:
                assert float((t_lp - lp).abs().max()) <= 1e-4      # K = 0: the online sum, another order of summation


def test_unscored_rows_and_bounds():
    """The C entry point on poisoned buffers with guard tails all round: rows whose target is -1 or n get the defined
    sentinels, rows past `rows` and entries past rows * K stay untouched."""
    from hydrainfer_amd import _lib
    rows, n, k, pad = 6, 1000, 7, 64
    x = torch.randn((rows + 2, n), generator=torch.Generator().manual_seed(5)).half().cuda()
    t = torch.tensor([3, -1, n, 999, -5, 0, 1, 1], dtype=torch.int32)
    for form in FORMS:
        bufs = {"lp": torch.full((rows + 2 * pad,), float(POISON), dtype=torch.float32, device="cuda"),
                "ranks": torch.full((rows + 2 * pad,), POISON, dtype=torch.int32, device="cuda"),
                "top_ids": torch.full((rows * k + 2 * pad,), POISON, dtype=torch.int32, device="cuda"),
                "top_lp": torch.full((rows * k + 2 * pad,), float(POISON), dtype=torch.float32, device="cuda")}
        ptr = {name: b[pad:].data_ptr() for name, b in bufs.items()}
        td = t.cuda()
        _lib.check(_lib.lib().hx_token_logprob_rows_ex(ptr["lp"], ptr["ranks"], ptr["top_ids"], ptr["top_lp"], x.data_ptr(),
                                                       td.data_ptr(), rows, n, x.stride(0), k, _lib.HX_F16, form,
                                                       _lib.current_stream()), "token_logprob_rows")
        torch.cuda.synchronize()
        for name, b in bufs.items():
            inner = rows * (k if name.startswith("top") else 1)
            assert bool((b[:pad] == POISON).all()) and bool((b[pad + inner:] == POISON).all()), f"{name}: guard overwritten"
        ref = token_reference(x[:rows], t[:rows], k)
        lp = bufs["lp"][pad:pad + rows].cpu()
        ranks = bufs["ranks"][pad:pad + rows].cpu()
        top_ids = bufs["top_ids"][pad:pad + rows * k].view(rows, k).cpu()
        top_lp = bufs["top_lp"][pad:pad + rows * k].view(rows, k).cpu()
        for r in (1, 2, 4):
            assert math.isnan(float(lp[r])) and int(ranks[r]) == -1
            assert top_ids[r].tolist() == [-1] * k and top_lp[r].tolist() == [-math.inf] * k
        assert torch.equal(ranks.long(), ref[1]) and torch.equal(top_ids.long(), ref[2])
        assert_logprobs_close(lp, ref[0], "guarded run")
        assert_logprobs_close(top_lp, ref[3], "guarded run (top)")
        # K = 0: the top buffers are not touched at all (and may be NULL)
        for name in ("top_ids", "top_lp"):
            bufs[name].fill_(POISON)
        _lib.check(_lib.lib().hx_token_logprob_rows_ex(ptr["lp"], ptr["ranks"], None, None, x.data_ptr(), td.data_ptr(), rows,
                                                       n, x.stride(0), 0, _lib.HX_F16, form, _lib.current_stream()),
                   "token_logprob_rows")
        torch.cuda.synchronize()
        assert bool((bufs["top_ids"] == POISON).all()) and bool((bufs["top_lp"] == POISON).all())


def test_refusals_launch_nothing():
    from hydrainfer_amd import _lib
    _, token_logprob_rows = _ops()
    good = torch.zeros((2, 16), dtype=torch.float16, device="cuda")
    tg = torch.zeros(2, dtype=torch.int32, device="cuda")
    for bad, t, k in ((good.float(), tg, 0), (good[0], tg, 0), (good, tg, 21), (good, tg, -1), (good.cpu(), tg, 0),
                      (good.t(), tg, 0), (good, tg.long(), 0), (good, tg[:1], 0), (good, tg.cpu(), 0), (good, tg, True)):
        with pytest.raises(_lib.HydraHipError):
            token_logprob_rows(bad, t, k)
    # the C entry points themselves: an error code for every bad argument, and the outputs keep their poison
    out = torch.full((64,), POISON, dtype=torch.int64, device="cuda")
    f, fx = _lib.lib().hx_token_logprob_rows, _lib.lib().hx_token_logprob_rows_ex
    s, p, q, t = _lib.current_stream(), out.data_ptr(), good.data_ptr(), tg.data_ptr()
    assert f(p, p, p, p, q, t, 2, 16, 16, 21, _lib.HX_F16, s) == -2 and f(p, p, p, p, q, t, 2, 16, 16, -1, _lib.HX_F16, s) == -2
    assert f(p, p, p, p, q, t, 0, 16, 16, 1, _lib.HX_F16, s) == -2 and f(p, p, p, p, q, t, 2, 0, 16, 1, _lib.HX_F16, s) == -2
    assert f(p, p, p, p, q, t, 2, 16, 8, 1, _lib.HX_F16, s) == -2
    assert f(p, p, p, p, q, t, 2, 16, 16, 1, _lib.HX_F32, s) == -1
    assert f(p, p, p, p, q, None, 2, 16, 16, 1, _lib.HX_F16, s) == -4 and f(p, None, p, p, q, t, 2, 16, 16, 1, _lib.HX_F16, s) == -4
    assert f(None, p, p, p, q, t, 2, 16, 16, 1, _lib.HX_F16, s) == -4 and f(p, p, None, p, q, t, 2, 16, 16, 1, _lib.HX_F16, s) == -4
    assert f(p, p, p, p, None, t, 2, 16, 16, 1, _lib.HX_F16, s) == -4
    assert fx(p, p, p, p, q, t, 2, 16, 16, 1, _lib.HX_F16, 3, s) == -2 and fx(p, p, p, p, q, t, 2, 16, 16, 1, _lib.HX_F16, -1, s) == -2
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


def test_packed_result_is_one_buffer():
    """The four results share one allocation: one copy brings a step's prompt scores to the host."""
    from hydrainfer_amd._C.kernel.norm import (token_logprob_rows, token_logprob_rows_bytes, token_logprob_rows_packed,
                                               token_logprob_rows_views)
    g = torch.Generator().manual_seed(9)
    x = torch.randn((3, 500), generator=g).to(torch.bfloat16).cuda()
    t = torch.tensor([4, -1, 499], dtype=torch.int32, device="cuda")
    res = token_logprob_rows(x, t, 4)
    host = token_logprob_rows_views(token_logprob_rows_packed(res[0], 4).cpu(), 3, 4)
    assert math.isnan(float(host[0][1])) and int(host[1][1]) == -1
    for a, b in zip(res, host):
        assert torch.equal(torch.nan_to_num(a.cpu().double(), nan=7.0), torch.nan_to_num(b.double(), nan=7.0))
    big = torch.zeros(64 + token_logprob_rows_bytes(3, 4), dtype=torch.uint8, device="cuda")
    res2 = token_logprob_rows(x, t, 4, out=big[64:])
    assert res2[0].data_ptr() == big.data_ptr() + 64 and torch.equal(res[1], res2[1]) and torch.equal(res[2], res2[2])
    assert torch.equal(res[3], res2[3]) and torch.equal(torch.nan_to_num(res[0], nan=7.0), torch.nan_to_num(res2[0], nan=7.0))
    assert bool((big[:64] == 0).all())
