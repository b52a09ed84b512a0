"""GPU: hx_sample_rows_masked (csrc/sampling.hip, sampling_body.inc with MASKED) through sampling.sample_rows_masked.
Exactness first, with no tolerance: a masked launch must give, bit for bit, what hx_sample_rows_logprobs (scored) and
hx_sample_rows_constrained (unscored) give for the same rows with -inf written into the logits at the masked positions.
Then what holds whatever the library computes: a one-token mask returns that token, an id lies inside its mask, the scores
are the float64 log-softmax over the allowed set (tests/mask_ref.py).  Every result buffer is pre-filled with a sentinel."""
import math

import numpy as np
import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd._C.kernel.norm import logprob_rows_bytes
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, SAMPLE_MAX_N, PenaltyHistory, pack_constrained_step,
                                     pack_mask_words, pack_masked_step, sample_rows_masked)
from tests import mask_ref
from tests.test_gpu_constraints import DEV, DTYPES, IDS, bits, eighths, launch_c, misaligned, same
from tests.test_gpu_sample_logprobs import SENTINEL_BYTE, launch_s

pytestmark = pytest.mark.gpu

NEG = -math.inf
ATOL = 1e-4                   # the bound the project holds hx_sample_rows_logprobs' scores to


def launch_m(logits, entries, masks, mask_row, k, want=None):
    """entries: pack_constrained_step's; masks: a list of uint32 word arrays; mask_row: one int per row.  k None: the
    unscored launch -> (ids, cut, u); else -> ((ids, cut, u), logprobs, top_ids, top_logprobs), all on the host."""
    sp, bi, bv, cb, hi, hc, cu, pen = pack_constrained_step(entries).to_device(DEV)
    rows, n = logits.shape
    words = (n + 31) // 32
    allow = torch.from_numpy(np.stack(masks).view(np.int32) if masks else np.zeros((0, words), np.int32)).to(DEV)
    mr = torch.tensor(mask_row, dtype=torch.int32, device=DEV)
    cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2))
    if k is None:
        ids = sample_rows_masked(logits, sp, bi, bv, cb, allow, mr, hi, hc, cu, pen, cut_out=cut, u_out=u)
        assert ids.dtype == torch.int64 and ids.shape == (rows,)
        return ids.cpu(), cut.cpu(), u.cpu()
    out = torch.full((logprob_rows_bytes(rows, k),), SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    w = None if want is None else torch.tensor(want, dtype=torch.int32, device=DEV)
    ids, lp, top_ids, top_lp = sample_rows_masked(logits, sp, bi, bv, cb, allow, mr, hi, hc, cu, pen, top_k=k, want=w,
                                                  out=out, cut_out=cut, u_out=u)
    assert ids.data_ptr() == out.data_ptr() and top_ids.shape == (rows, k) and top_lp.shape == (rows, k)
    return (ids.cpu(), cut.cpu(), u.cpu()), lp.cpu(), top_ids.cpu(), top_lp.cpu()


def same_scores(a, b):
    """two launch_s / launch_m results (scored), bit for bit"""
    return same(a[0], b[0]) and all(torch.equal(bits(x), bits(y)) for x, y in zip(a[1:], b[1:]))


def banned_logits(x, masks, mask_row):
    """the logits with -inf written where a row's mask leaves a token out (rows whose index names no mask: as they are)"""
    out = x.clone()
    n = x.shape[1]
    for r, j in enumerate(mask_row):
        if 0 <= j < len(masks):
            keep = torch.zeros(n, dtype=torch.bool)
            keep[mask_ref.allowed_of(masks[j].tolist(), n)] = True
            out[r, ~keep] = NEG
    return out


def mixed_case(n, g):
    """Eight rows in one launch: unmasked (-1); an index >= n_masks (unmasked); two rows sharing a mask, sampled and
    greedy; a one-token mask; a mask of all tokens; a row with history penalties and a bias entry on an allowed token; a
    row whose top_k exceeds its allowed count.  -> (entries, masks, mask_row, allowed sets by mask)"""
    perm = lambda count: sorted(torch.randperm(n, generator=g)[:max(1, min(count, n))].tolist())
    sets = [perm((n + 1) // 2), perm(1), list(range(n)), perm((n + 2) // 3), perm(3)]
    masks = [pack_mask_words(s, n) for s in sets]
    seed = (1 << 35) + 31 * n
    tk = max(1, min(5, n - 1))
    hist = PenaltyHistory(torch.randint(0, n, (12,), generator=g).tolist() + sets[3][:2])
    bias = (np.asarray([sets[3][0]], np.int32), np.asarray([2.5], np.float32))         # on an allowed token
    entries = [(None, NO_PENALTIES, (1.0, 0.9, 0, seed, 0), None),
               (None, NO_PENALTIES, GREEDY_RECORD, None),
               (None, NO_PENALTIES, (0.5, 0.75, 0, seed + 2, 2), None),
               (None, NO_PENALTIES, GREEDY_RECORD, None),
               (None, NO_PENALTIES, (1.0, 1.0, 0, seed + 4, 4), None),
               (None, NO_PENALTIES, (2.0, 1.0, tk, seed + 5, 5, 0.125), None),
               (hist, (0.375, 0.25, 1.5), (1.5, 0.9, 0, seed + 6, 6), bias),
               (None, NO_PENALTIES, (1.0, 1.0, min(50, n - 1) if n > 4 else 0, seed + 7, 7), None)]
    mask_row = [-1, len(masks) + 3, 0, 0, 1, 2, 3, 4]
    return entries, masks, mask_row, sets


@pytest.mark.parametrize("n", [31, 33, 100, 4104, 32064, SAMPLE_MAX_N])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_equals_the_siblings_on_banned_logits(dtype, n):
    """n = 31: less than one word; 33: a one-bit tail word; 100: n % 8 != 0, the scalar staging tail; 4104 behind a row
    stride of n + 3: the unaligned, non-vector path; 32064: the vocabulary; SAMPLE_MAX_N: the widest row."""
    g = torch.Generator().manual_seed(7000 + n)
    x = eighths((8, n), g).to(dtype)
    entries, masks, mask_row, _ = mixed_case(n, g)
    place = misaligned if n == 4104 else (lambda t: t)
    xd, xb = place(x.to(DEV)), place(banned_logits(x, masks, mask_row).to(DEV))
    if n == 4104:
        assert xd.stride(0) == n + 3
    # garbage in the bits at and above n of every mask's last word: ignored
    dirty = [m.copy() for m in masks]
    if n % 32:
        for m in dirty:
            m[-1] |= np.uint32((0xffffffff << (n % 32)) & 0xffffffff)
    base = launch_c(xb, entries)
    for these in (masks, dirty):
        assert same(launch_m(xd, entries, these, mask_row, None), base), f"n={n}: unscored, against hx_sample_rows_constrained"
    for k, want in ((0, None), (3, [0, -1, 0, 0, -1, 0, 0, 0]), (20, None), (20, [-1, 0, -1, 0, 0, -1, 0, 0])):
        ref = launch_s(xb, entries, k, want)
        assert same(ref[0], base)
        for these in (masks, dirty):
            assert same_scores(launch_m(xd, entries, these, mask_row, k, want), ref), f"n={n} K={k} want={want}"
    # and the ids themselves, whatever the siblings say: inside the mask
    ids = base[0].tolist()
    for r, j in enumerate(mask_row):
        if 0 <= j < len(masks):
            assert (int(masks[j][ids[r] >> 5]) >> (ids[r] & 31)) & 1, (n, r)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_no_mask_at_all_is_the_sibling(dtype):
    """n_masks = 0 (allow_words NULL) and every index out of range: the scored and the constrained launch, bit for bit"""
    n = 1000
    g = torch.Generator().manual_seed(5)
    x = eighths((8, n), g).to(dtype).to(DEV)
    entries, _, _, _ = mixed_case(n, g)
    for mask_row in ([-1] * 8, [0, 1, 2, 3, 1 << 30, -(1 << 31), 7, -2]):
        assert same(launch_m(x, entries, [], mask_row, None), launch_c(x, entries))
        assert same_scores(launch_m(x, entries, [], mask_row, 5, [0, -1] * 4), launch_s(x, entries, 5, [0, -1] * 4))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ids_stay_inside_their_masks_over_64_seeds(dtype):
    """eight launches of eight rows, 64 seeds: a one-token mask returns that token; every masked row's id is allowed"""
    n = 1000
    g = torch.Generator().manual_seed(17)
    x = (torch.randn(8, n, generator=g) * 3).to(dtype).to(DEV)
    sets = [[777], sorted(torch.randperm(n, generator=g)[:4].tolist()), sorted(torch.randperm(n, generator=g)[:500].tolist())]
    masks = [pack_mask_words(s, n) for s in sets]
    mask_row = [0, 0, 0, 1, 1, 2, 2, 0]
    seen = set()
    for launch in range(8):
        entries = [(None, NO_PENALTIES, (1.0 + 0.5 * (r % 3), 1.0, 0, (1 << 36) + 8 * launch + r, launch), None)
                   for r in range(8)]
        ids = launch_m(x, entries, masks, mask_row, None)[0].tolist()
        for r, t in enumerate(ids):
            assert t in sets[mask_row[r]], (launch, r, t)
        assert [ids[r] for r in (0, 1, 2, 7)] == [777] * 4
        seen.update(ids[3:5])
    assert len(seen) > 1, "64 seeds over four allowed tokens drew one token only"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scores_are_the_log_softmax_over_the_allowed_set(dtype):
    """T = 1, top_k = 0, top_p = 1, no penalties: logprobs and top_logprobs against float64 (tests/mask_ref.py) within
    1e-4; with fewer allowed tokens than K the alternatives run on into disallowed tokens, which carry -inf"""
    n, k = 32064, 20
    g = torch.Generator().manual_seed(23)
    x = (torch.randn(4, n, generator=g) * 3).to(dtype)
    sets = [sorted(torch.randperm(n, generator=g)[:c].tolist()) for c in (4, 1, 1000, n // 2)]
    masks = [pack_mask_words(s, n) for s in sets]
    entries = [(None, NO_PENALTIES, (1.0, 1.0, 0, (1 << 37) + r, r), None) for r in range(4)]
    (ids, _, _), lp, top_ids, top_lp = launch_m(x.to(DEV), entries, masks, [0, 1, 2, 3], k)
    worst = 0.0
    for r in range(4):
        ref = mask_ref.masked_log_softmax(x[r].float().numpy(), sets[r])
        assert int(ids[r]) in sets[r]
        worst = max(worst, abs(float(lp[r]) - ref[int(ids[r])]))
        inside = 0
        for t, v in zip(top_ids[r].tolist(), top_lp[r].tolist()):
            assert 0 <= t < n
            if t in sets[r]:
                inside += 1
                worst = max(worst, abs(v - ref[t]))
            else:
                assert v == NEG, f"row {r}: the disallowed token {t} is named with {v}"
        assert inside == min(k, len(sets[r])), r
        # the alternatives come most likely first: the allowed ones lead
        assert all(t in sets[r] for t in top_ids[r].tolist()[:inside])
    print(f"largest |logprob - float64 log-softmax over the allowed set| {worst:.3e}")
    assert worst <= ATOL


def test_errors_leave_everything_untouched():
    rows, n, k = 2, 40, 3
    logits = torch.zeros((rows, n), dtype=torch.float16, device=DEV)
    step = pack_constrained_step([(PenaltyHistory([3, 4]), (1.0, 0.0, 1.0), GREEDY_RECORD, (np.asarray([5], np.int32), np.asarray([1.0], np.float32))),
                                  (None, NO_PENALTIES, GREEDY_RECORD, None)])
    sp, bi, bv, cb, hi, hc, cu, pen = step.to_device(DEV)
    out = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    lp = torch.full((rows,), 7.0, device=DEV)
    tids = torch.full((rows, k), -7, dtype=torch.int32, device=DEV)
    tlp = torch.full((rows, k), 7.0, device=DEV)
    want = torch.zeros(rows, dtype=torch.int32, device=DEV)
    allow = torch.from_numpy(pack_mask_words([9, 33], n).view(np.int32).reshape(1, 2)).to(DEV)
    mr = torch.tensor([0, -1], dtype=torch.int32, device=DEV)
    f = _lib.lib().hx_sample_rows_masked
    ok = [out.data_ptr(), None, None, logits.data_ptr(), rows, n, n, hi.data_ptr(), hc.data_ptr(), cu.data_ptr(), 2,
          pen.data_ptr(), bi.data_ptr(), bv.data_ptr(), cb.data_ptr(), 1, sp.data_ptr(), lp.data_ptr(), tids.data_ptr(),
          tlp.data_ptr(), k, want.data_ptr(), allow.data_ptr(), 1, mr.data_ptr(), _lib.HX_F16, _lib.current_stream()]
    SHAPE, DTYPE, NULL = -2, -1, -4
    # hx_sample_rows_logprobs' rules (scoring is asked for), then the three of the masks
    cases = [((4, 0), SHAPE), ((5, 0), SHAPE), ((6, n - 1), SHAPE), ((5, SAMPLE_MAX_N + 1), SHAPE), ((10, -1), SHAPE),
             ((10, 1 << 31), SHAPE), ((15, -1), SHAPE), ((15, 1 << 31), SHAPE), ((20, -1), SHAPE), ((20, 21), SHAPE),
             ((25, _lib.HX_F32), DTYPE), ((23, -1), SHAPE)]
    cases += [((at, None), NULL) for at in (0, 3, 16, 7, 8, 9, 11, 12, 13, 14, 18, 19, 22, 24)]
    for (at, v), code in cases:
        args = list(ok)
        args[at] = v
        if (at, v) == (5, SAMPLE_MAX_N + 1):
            args[6] = v
        assert f(*args) == code, (at, v)
    # without scores the constrained entry's rules are left: a top_k out of range is not looked at, the mask rules stay
    for (at, v), code in (((23, -1), SHAPE), ((24, None), NULL), ((22, None), NULL), ((5, 0), SHAPE), ((16, None), NULL)):
        args = list(ok)
        args[17] = None
        args[at] = v
        assert f(*args) == code, ("unscored", at, v)
    torch.cuda.synchronize()
    assert out.tolist() == [-7, -7] and lp.tolist() == [7.0, 7.0] and bool((tids == -7).all()) and bool((tlp == 7.0).all())
    # legal: unscored with top_ids, top_logprobs and want NULL and a top_k that would be out of range; n_masks = 0 with
    # allow_words NULL
    args = list(ok)
    for at in (17, 18, 19, 21):
        args[at] = None
    args[20] = 21
    assert f(*args) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [9, 0] and lp.tolist() == [7.0, 7.0] and bool((tids == -7).all()) and bool((tlp == 7.0).all())
    args = list(ok)
    args[22], args[23] = None, 0
    assert f(*args) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [5, 0] and bool((tids[:, 0] != -7).all())        # (unmasked: row 0's bias puts token 5 on top)


def test_wrapper_refuses_malformed_arguments():
    n = 40
    logits = torch.zeros((2, n), dtype=torch.float16, device=DEV)
    step = pack_masked_step([(None, NO_PENALTIES, GREEDY_RECORD, None, 0, pack_mask_words([9], n)),
                             (None, NO_PENALTIES, GREEDY_RECORD, None, -1, None)])
    *tables, want = step.to_device(DEV)
    ids, lp, _, _ = sample_rows_masked(logits, *tables, top_k=2, want=want)
    assert ids.tolist() == [9, 0] and lp[0].item() == 0.0 and math.isnan(lp[1].item())
    assert sample_rows_masked(logits, *tables).tolist() == [9, 0]
    E = _lib.HydraHipError
    sp, bi, bv, cb, allow, mr, hi, hc, cu, pen = tables
    call = lambda allow=allow, mr=mr, **kw: sample_rows_masked(logits, sp, bi, bv, cb, allow, mr, hi, hc, cu, pen, **kw)
    for bad in (lambda: call(top_k=21), lambda: call(top_k=True), lambda: call(want=want),
                lambda: call(allow=allow[:, :1]), lambda: call(allow=allow.float()), lambda: call(allow=allow.view(-1)),
                lambda: call(allow=allow.cpu()), lambda: call(mr=mr.long()), lambda: call(mr=mr[:1]),
                lambda: call(top_k=1, want=want.long())):
        with pytest.raises(E):
            bad()
