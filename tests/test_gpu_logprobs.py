"""GPU: hx_logprob_rows / _C.kernel.norm.logprob_rows — greedy id, its log-softmax value and the top-K alternatives of
every row in one launch — against the float64 reference of tests/logprob_ref.py.  Ids are exact (the tie rule is part of
the contract); log-probabilities are held to 1e-4 (logprob_ref.ATOL: the fp32 sum's error bound with an order of
magnitude of margin, a hundred times below 16-bit arithmetic)."""
import math

import pytest
import torch

from tests.logprob_ref import assert_logprobs_close, reference

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
KS = (0, 1, 5, 20)


def _ops():
    from hydrainfer_amd._C.kernel.norm import argmax_rows, logprob_rows
    return argmax_rows, logprob_rows


def _views(rows, n, dtype, seed):
    """The same random logits as a contiguous tensor, a strided view (ld > n, ld % 8 == 0, 16-byte aligned: the vector
    path, with its n % 8 tail) and a view whose base is 2 bytes off a 16-byte boundary (the scalar path)."""
    g = torch.Generator().manual_seed(seed)
    x = (4.0 * torch.randn((rows, n), generator=g)).to(dtype)
    ld = (n + 7) // 8 * 8 + 8
    wide = torch.full((rows, ld), 9.0e3, dtype=dtype, device="cuda")          # what lies past n would win if it were read
    wide[:, :n] = x
    flat = torch.full((rows * ld + 8,), 9.0e3, dtype=dtype, device="cuda")
    off = flat[1:1 + rows * ld].view(rows, ld)
    off[:, :n] = x
    assert wide.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 2
    return x, {"contiguous": x.cuda(), "strided": wide[:, :n], "unaligned": off[:, :n]}


def _check(logits, top_k, ref, what):
    argmax_rows, logprob_rows = _ops()
    ids, lp, top_ids, top_lp = logprob_rows(logits, top_k)
    torch.cuda.synchronize()
    rows = logits.shape[0]
    assert ids.dtype == torch.int64 and ids.shape == (rows,) and lp.dtype == torch.float32 and lp.shape == (rows,)
    assert top_ids.dtype == torch.int32 and top_ids.shape == (rows, top_k)
    assert top_lp.dtype == torch.float32 and top_lp.shape == (rows, top_k)
    r_ids, r_lp, r_top_ids, r_top_lp = ref
    assert torch.equal(ids.cpu(), r_ids), f"{what}: greedy ids differ from the reference"
    assert torch.equal(ids, argmax_rows(logits)), f"{what}: ids differ from argmax_rows"
    assert torch.equal(top_ids.cpu().long(), r_top_ids[:, :top_k]), f"{what}: top ids / their order differ"
    if top_k:
        assert torch.equal(top_ids[:, 0].long(), ids), f"{what}: top_ids[:, 0] is not the greedy id"
    e1 = assert_logprobs_close(lp, r_lp, what)
    e2 = assert_logprobs_close(top_lp, r_top_lp[:, :top_k], what + " (top)")
    return max(e1, e2)


@pytest.mark.parametrize("n", [1, 7, 8, 63, 1000, 24576, 24584, 32064, 40000, 100000])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_shape_grid(n, dt):
    """n: below / at / past a 16-byte piece, a staged row of exactly 48 KiB and the first past it, which needs the
    kernel's dynamic LDS limit raised (24576, 24584), one trip of the load loop (32064), two (40000), a row that does
    not fit in LDS (100000); rows 1, 3, 33; K 0, 1, 5, 20 (K > n for the small ones); three layouts."""
    worst = 0.0
    for rows in (1, 3, 33):
        x, views = _views(rows, n, DTYPES[dt], seed=1000 * rows + n)
        ref = reference(x, max(KS))
        for name, v in views.items():
            for k in KS:
                worst = max(worst, _check(v, k, ref, f"{dt} n={n} rows={rows} K={k} {name}"))
    print(f"{dt} n={n}: max |logprob error| {worst:.2e}")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_ties(dt):
    _, logprob_rows = _ops()
    n = 32064
    flat = torch.full((2, n), 1.5, dtype=DTYPES[dt], device="cuda")
    ids, lp, top_ids, top_lp = logprob_rows(flat, 20)
    assert ids.tolist() == [0, 0] and top_ids.tolist() == [list(range(20))] * 2
    assert float((top_lp.double() + math.log(n)).abs().max()) <= 1e-4 and float((lp.double() + math.log(n)).abs().max()) <= 1e-4
    # four distinct values repeated over the row: every one of the top 20 is decided by the index
    g = torch.Generator().manual_seed(7)
    vals = torch.tensor([0.25, -3.0, 2.5, 2.484375]).to(DTYPES[dt])     # (distinct in both formats)
    x = vals[torch.randint(0, 4, (3, n), generator=g)]
    x[1, :9000] = vals[1]                       # the largest value's first occurrences lie deep in the row
    ref = reference(x, 20)
    for k in KS:
        _check(x.cuda(), k, ref, f"{dt} four values K={k}")
    assert bool((x[torch.arange(3)[:, None], ref[2]] == vals[2]).all()) and int(ref[2][1, 0]) >= 9000


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_answers(dt):
    _, logprob_rows = _ops()
    n, j, dtype = 32064, 12345, DTYPES[dt]
    g = torch.Generator().manual_seed(3)
    noise = lambda: (4.0 * torch.randn(n, generator=g)).to(dtype)
    # rows 0, 2, 4, 6: ordinary rows around the special ones — they must not notice their neighbours
    x = torch.stack([noise(), torch.zeros(n, dtype=dtype), noise(), torch.full((n,), -math.inf, dtype=dtype), noise(),
                     noise(), noise()])
    x[1, j] = 40.0                                             # one-hot
    finite = [5, 4000, 32063]
    x[3, finite] = torch.tensor([1.0, 2.0, 1.0]).to(dtype)     # -inf except m = 3 entries
    x[5, 777] = math.nan                                       # one NaN
    ids, lp, top_ids, top_lp = logprob_rows(x.cuda(), 5)
    ids, lp, top_ids, top_lp = ids.cpu(), lp.cpu().double(), top_ids.cpu(), top_lp.cpu().double()
    # one-hot: logprob = -log(1 + (n - 1) e^-40), the others -40 more
    lse = math.log1p((n - 1) * math.exp(-40.0))
    assert ids[1] == j and abs(lp[1] + lse) <= 1e-4
    assert top_ids[1].tolist() == [j, 0, 1, 2, 3] and float((top_lp[1, 1:] + 40.0 + lse).abs().max()) <= 1e-4
    # three finite entries 1, 2, 1: softmax over them alone, everything else -inf
    z = math.log(2 * math.e + math.e ** 2)
    assert ids[3] == 4000 and top_ids[3].tolist() == [4000, 5, 32063, 0, 1]
    assert float((top_lp[3, :3] - torch.tensor([2 - z, 1 - z, 1 - z], dtype=torch.float64)).abs().max()) <= 1e-4
    assert top_lp[3, 3:].tolist() == [-math.inf, -math.inf] and abs(lp[3] - (2 - z)) <= 1e-4
    # a NaN: the id is its position, every logprob of the row NaN
    assert ids[5] == 777 and top_ids[5, 0] == 777 and math.isnan(lp[5]) and bool(torch.isnan(top_lp[5]).all())
    # the neighbours
    ref = reference(x, 5)
    for r in (0, 2, 4, 6):
        assert ids[r] == ref[0][r] and torch.equal(top_ids[r].long(), ref[2][r])
        assert_logprobs_close(top_lp[r], ref[3][r], f"{dt} neighbour row {r}")
        assert_logprobs_close(lp[r:r + 1], ref[1][r:r + 1], f"{dt} neighbour row {r}")


def test_outputs_are_written_inside_their_bounds():
    """The C entry point on buffers with canaries all round: rows past `rows` and entries past rows * K stay untouched,
    and so does the logits' tail."""
    from hydrainfer_amd import _lib
    rows, n, k, pad = 5, 1000, 7, 64
    x = torch.randn((rows + 2, n), generator=torch.Generator().manual_seed(5)).half().cuda()
    bufs = {"ids": torch.full((rows + 2 * pad,), -77, dtype=torch.int64, device="cuda"),
            "lp": torch.full((rows + 2 * pad,), -77.0, dtype=torch.float32, device="cuda"),
            "top_ids": torch.full((rows * k + 2 * pad,), -77, dtype=torch.int32, device="cuda"),
            "top_lp": torch.full((rows * k + 2 * pad,), -77.0, dtype=torch.float32, device="cuda")}
    ptr = {name: b[pad:].data_ptr() for name, b in bufs.items()}
    _lib.check(_lib.lib().hx_logprob_rows(ptr["ids"], ptr["lp"], ptr["top_ids"], ptr["top_lp"], x.data_ptr(), rows, n,
                                          x.stride(0), k, _lib.HX_F16, _lib.current_stream()), "logprob_rows")
    torch.cuda.synchronize()
    ref = reference(x[:rows], k)
    for name, b in bufs.items():
        inner = rows * (k if name.startswith("top") else 1)
        assert bool((b[:pad] == -77).all()) and bool((b[pad + inner:] == -77).all()), f"{name}: canary overwritten"
    assert torch.equal(bufs["ids"][pad:pad + rows].cpu(), ref[0])
    assert torch.equal(bufs["top_ids"][pad:pad + rows * k].view(rows, k).cpu().long(), ref[2])
    assert_logprobs_close(bufs["top_lp"][pad:pad + rows * k], ref[3], "canary run")
    # K = 0: the top buffers are not touched at all (and may be NULL)
    for name in ("top_ids", "top_lp"):
        bufs[name].fill_(-77)
    _lib.check(_lib.lib().hx_logprob_rows(ptr["ids"], ptr["lp"], None, None, x.data_ptr(), rows, n, x.stride(0), 0,
                                          _lib.HX_F16, _lib.current_stream()), "logprob_rows")
    torch.cuda.synchronize()
    assert bool((bufs["top_ids"] == -77).all()) and bool((bufs["top_lp"] == -77.0).all())


def test_refusals_launch_nothing():
    from hydrainfer_amd import _lib
    _, logprob_rows = _ops()
    good = torch.zeros((2, 16), dtype=torch.float16, device="cuda")
    for bad, k in ((good.float(), 0), (good[0], 0), (good, 21), (good, -1), (good.cpu(), 0), (good.t(), 0)):
        with pytest.raises(_lib.HydraHipError):
            logprob_rows(bad, k)
    # the C entry point itself: an error code for every bad argument, and the outputs keep their canaries
    out = torch.full((64,), -77, dtype=torch.int64, device="cuda")
    f = _lib.lib().hx_logprob_rows
    s, p, q = _lib.current_stream(), out.data_ptr(), good.data_ptr()
    assert f(p, p, p, p, q, 2, 16, 16, 21, _lib.HX_F16, s) == -2 and f(p, p, p, p, q, 2, 16, 16, -1, _lib.HX_F16, s) == -2
    assert f(p, p, p, p, q, 0, 16, 16, 1, _lib.HX_F16, s) == -2 and f(p, p, p, p, q, 2, 0, 16, 1, _lib.HX_F16, s) == -2
    assert f(p, p, p, p, q, 2, 16, 8, 1, _lib.HX_F16, s) == -2
    assert f(p, p, p, p, q, 2, 16, 16, 1, _lib.HX_F32, s) == -1
    assert f(None, p, p, p, q, 2, 16, 16, 1, _lib.HX_F16, s) == -4 and f(p, p, None, p, q, 2, 16, 16, 1, _lib.HX_F16, s) == -4
    assert f(p, p, p, p, None, 2, 16, 16, 1, _lib.HX_F16, s) == -4
    torch.cuda.synchronize()
    assert bool((out == -77).all())


def test_packed_result_is_one_buffer():
    """The four results share one allocation: one copy brings a step's scores to the host."""
    from hydrainfer_amd._C.kernel.norm import logprob_rows, logprob_rows_bytes, logprob_rows_packed, logprob_rows_views
    x = torch.randn((3, 500), generator=torch.Generator().manual_seed(9)).to(torch.bfloat16).cuda()
    res = logprob_rows(x, 4)
    host = logprob_rows_views(logprob_rows_packed(res[0], 4).cpu(), 3, 4)
    for a, b in zip(res, host):
        assert torch.equal(a.cpu(), b)
    big = torch.zeros(64 + logprob_rows_bytes(3, 4), dtype=torch.uint8, device="cuda")
    res2 = logprob_rows(x, 4, out=big[64:])
    assert res2[0].data_ptr() == big.data_ptr() + 64 and all(torch.equal(a, b) for a, b in zip(res, res2))
    assert bool((big[:64] == 0).all())
