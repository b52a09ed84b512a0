"""No GPU: every case tests/test_gpu_moe_branches.py runs is shown, on the oracle, to be SOUND (the oracle's output passes
the case's own checker) and SENSITIVE (the output of a subtly wrong kernel — the mutants of tests/moe_cases.py — is
refused by the very assertion the GPU file applies).  The case lists live in tests/moe_cases.py: what is proven here is
what runs."""
import numpy as np
import pytest
import torch

from oracle import moe
from tests import moe_cases as M

ALL_UNPERMUTE = M.UNPERMUTE_CASES + M.UNPERMUTE_SPLIT_CASES + M.UNPERMUTE_LOOP_CASES
ALL_TOPK = [c for e in M.TOPK_EXPERTS for c in M.topk_cases(e)]


def _refused(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def test_case_lists_cover_what_the_issue_names():
    cs = M.UNPERMUTE_CASES
    for dt in M.DTYPES:
        idx = [c for c in cs if c.form == "index" and c.dt == dt]
        assert {c.n_rows for c in idx} == set(range(1, 10))
        assert {c.dim for c in idx} == {8, 64, 2056, 36} and {c.n_tokens for c in idx} == {1, 5, 300}
        msk = [c for c in cs if c.form == "mask" and c.dt == dt]
        assert {c.dim for c in msk} >= {8, 64, 2056, 36} and {c.n_tokens for c in msk} == {1, 5, 300}
        assert {c.n_rows for c in msk} >= {257, 320} and {c.full_expert for c in msk} == {False, True}
        valid = torch.cat([M.unpermute(c).n_valid for c in msk if c.n_rows <= 60])
        assert set(valid.tolist()) >= set(range(0, 9)), "uneven masks must give every count from 0 to 2 * topk"
    assert {(c.form, c.dt) for c in M.UNPERMUTE_SPLIT_CASES} == {(f, d) for f in ("index", "mask") for d in ("fp16", "bf16")}
    assert all(c.dim == 7168 and c.n_tokens <= 8 for c in M.UNPERMUTE_SPLIT_CASES)
    assert all(c.n_tokens >= 1024 and c.dim // 8 > 256 and c.dt != "fp32" for c in M.UNPERMUTE_LOOP_CASES)
    assert M.SUM_OUT_LOOP_SHAPE[0] >= 1024 and M.SUM_OUT_LOOP_SHAPE[2] // 8 > 256
    assert [n * k for n, k in M.SORT_SHAPES] == [1024, 1025, 32768, 1048576, 1048584]
    assert {c.n_experts for c in ALL_TOPK} == {5, 60, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024}
    for e in M.TOPK_EXPERTS:
        ks = {c.topk for c in M.topk_cases(e)}
        assert ks == ({1, min(8, e)} | ({e} if e <= 65 else set()))
        assert {(c.n_tokens, c.ties > 0, c.ninf) for c in M.topk_cases(e)} == {(n, t, f) for n in (1, 6) for t, f in
                                                                               ((False, False), (True, False), (True, True))}


def test_uneven_masks_have_the_edges_and_respect_the_row_budget():
    for n, e, topk in ((1, 4, 2), (5, 8, 4), (300, 16, 4), (257, 60, 4), (300, 257, 4)):
        for full in (False, True):
            m = M.uneven_mask(n, e, topk, M._gen(1, n, e, full), full)
            assert int(m.sum()) <= n * topk
            assert (m.sum(dim=0) == 0).any(), "an expert with no tokens"
            if full:
                assert (m.sum(dim=0) == n).any(), "an expert that takes every token"
            else:
                assert (m.sum(dim=1) == 0).any(), "a token routed nowhere"
            if n >= 257:
                assert (m.sum(dim=1) > topk).any(), "a token with more than topk experts"


@pytest.mark.parametrize("case", ALL_UNPERMUTE, ids=[c.name for c in ALL_UNPERMUTE])
def test_unpermute_case_is_sound(case):
    b = M.unpermute(case)
    out = M.kernel_arithmetic(b.x, b.row_map, b.probs)
    assert not torch.isnan(out.float()).any(), "NaN at an unrouted position reached the oracle's output"
    M.check_unpermute(b, out)
    if case.form == "mask":
        assert torch.isnan(b.probs.float()[(b.row_map < 0).t()]).all() and (b.probs.float()[(b.row_map >= 0).t()] > 0).all()


def test_unpermute_mutants_are_refused():
    """Every applicable mutant fails the checker on at least 90 % of the cases it applies to; "map order reversed" (the
    same terms, other two-byte roundings — often invisible at a few rows) on at least one two-byte case per form."""
    table = {name: [0, 0] for name, _ in M.UNPERMUTE_MUTANTS}
    reversed_seen = set()
    for case in ALL_UNPERMUTE:
        b = M.unpermute(case)
        for name, mutate in M.UNPERMUTE_MUTANTS:
            out = mutate(b)
            if out is None:
                continue
            hit = _refused(M.check_unpermute, b, out)
            table[name][0] += 1
            table[name][1] += hit
            if hit and name == "map order reversed":
                reversed_seen.add((case.form, case.dt))
    print("unpermute mutants (applies, refused):", table)
    for name, (applies, refused) in table.items():
        assert applies >= 20, f"{name}: applies to {applies} cases only"
        if name == "map order reversed":
            assert reversed_seen >= {(f, d) for f in ("index", "mask") for d in ("fp16", "bf16")}, reversed_seen
        else:
            assert refused >= 0.9 * applies, f"{name}: refused on {refused} of {applies} cases"


@pytest.mark.parametrize("dtype", [torch.float, torch.half, torch.bfloat16])
def test_old_assertion_accepts_mispaired_weights_and_the_new_checker_refuses_them(dtype):
    """The finding restated: on copies of the token (what tests/test_gpu_moe.py::test_permute_index unpermutes) flipped
    probabilities pass its allclose(out, tokens, 1e-2) — the result is token * sum(probs) however the weights are
    paired — while on distinct rows the same flip is refused, off by more than 1 on most elements."""
    dt = {torch.float: "fp32", torch.half: "fp16", torch.bfloat16: "bf16"}[dtype]
    n_tokens, dim, n_experts, topk = 300, 64, 16, 4
    g = torch.Generator().manual_seed(n_tokens + dim + n_experts + topk)
    tokens = torch.randn((n_tokens, dim), generator=g).to(dtype)
    gating = torch.randn((n_tokens, n_experts), generator=g).to(dtype)
    weights, indices = gating.float().topk(topk, dim=-1)
    probs = weights.softmax(dim=-1).to(dtype)
    p_ref, sorted_ref, row_map = moe.permute_index(tokens, indices.to(torch.int32))
    out_ref = moe.unpermute_index(p_ref, sorted_ref, probs, n_tokens, topk)
    flipped = moe.unpermute_rows(p_ref, row_map, probs.flip(1))
    assert not torch.equal(probs, probs.flip(1))
    assert torch.allclose(flipped.float(), out_ref.float(), atol=1e-2, rtol=1e-2)         # today's two assertions
    assert torch.allclose(tokens.float(), flipped.float(), atol=1e-2, rtol=1e-2)
    b = M.unpermute(M.UnpermuteCase("index", dt, n_tokens, dim, topk, topk))
    wrong = M.mut_flip_probs(b)
    M.check_unpermute(b, M.kernel_arithmetic(b.x, b.row_map, b.probs))
    with pytest.raises(AssertionError):
        M.check_unpermute(b, wrong)
    right = M.kernel_arithmetic(b.x, b.row_map, b.probs).float()
    assert float(((wrong.float() - right).abs() > 0.1).float().mean()) > 0.5


def test_map_checker_refuses_an_unstable_sort_and_a_wrong_copy():
    for n_tokens, topk, n_experts in ((128, 8, 8), (205, 5, 256), (7, 3, 4)):
        tokens, ids, permuted, row_map = M.index_case(n_tokens, topk, n_experts, 8, "fp16")
        M.check_rows(permuted, row_map, permuted, row_map, "oracle")
        swapped = M.mut_unstable_sort(ids, row_map)
        assert swapped is not None and sorted(swapped.reshape(-1).tolist()) == list(range(n_tokens * topk))
        assert _refused(M.check_rows, permuted, swapped, permuted, row_map, "unstable sort")
        assert _refused(M.check_rows, permuted.roll(1, 0), row_map, permuted, row_map, "rows shifted")
    tokens, routing, permuted, row_map = M.mask_case(257, 60, 4, 8, "fp16", True)
    padded = torch.cat([permuted, torch.full((257 * 4 - permuted.shape[0], 8), float("nan"), dtype=permuted.dtype)])
    M.check_rows(padded, row_map, permuted, row_map, "rows past the total are not compared")
    assert int((row_map >= 0).sum()) == permuted.shape[0] and torch.equal(tokens[2], permuted[int(row_map[:, 2].max())])


@pytest.mark.parametrize("case", ALL_TOPK, ids=[c.name for c in ALL_TOPK])
def test_topk_case_is_sound(case):
    b = M.build_topk(case)                                   # asserts the 1 % separation of the oracle's probabilities
    w, i = M.oracle_topk(b)
    M.check_topk(b, w, i)
    lt = b.logits.gather(1, b.indices.long())
    assert bool((lt[:, 1:] <= lt[:, :-1]).all())
    same = lt[:, 1:] == lt[:, :-1]
    assert bool((b.indices[:, 1:] > b.indices[:, :-1])[same].all()), "lower index first among equals"
    if case.ties:
        assert bool((b.logits == b.logits.max(dim=1, keepdim=True).values).sum(dim=1).ge(2).all()), "the row maximum is tied"
    if case.ninf:
        assert int(torch.isinf(b.logits).sum()) > 0


def test_topk_mutants_are_refused():
    applies = refused = 0
    with_ties = [c for c in ALL_TOPK if c.ties]
    for case in with_ties:
        b = M.build_topk(case)
        wrong = M.mut_ties_higher(b)
        if wrong is None:
            continue
        applies += 1
        refused += _refused(M.check_topk, b, *wrong)
        w, i = M.oracle_topk(b)
        assert _refused(M.check_topk, b, w * (1 + 3e-5), i), "a weight 3e-5 off must be refused"
    print(f"topk_softmax: ties-to-the-higher-index applies to {applies} of {len(with_ties)} tie cases, refused on {refused}")
    assert applies >= 0.9 * len(with_ties) and refused >= 0.9 * applies


def test_sum_out_inputs_are_what_their_bars_assume():
    for dt in M.DTYPES:
        exact, positive = M.sum_out_inputs(3, 16, 264, dt)
        assert torch.equal((exact.double() * 16).round() / 16, exact.double()) and float(exact.abs().max()) <= 64
        a = exact.double().sum(dim=1)
        assert torch.equal(moe.sum_out(exact).double(), a.to(M.DTYPES[dt]).double()), "every order gives the one correct rounding"
        assert torch.equal(moe.sum_out(exact.flip(1)), moe.sum_out(exact))
        assert bool((positive >= 0).all()) and float(positive.float().mean()) > 10


@pytest.mark.parametrize("cfg", M.GROUPED_CASES)
def test_grouped_cases_oracle_equals_the_lane_emulator(cfg):
    from tests.moe_lane_emulator import grouped_topk_sigmoid_lanes, tie_heavy_inputs
    n_experts, n_groups, topk_group, topk = cfg
    logits, bias = tie_heavy_inputs(n_experts, M.GROUPED_TOKENS, 7 + n_experts + n_groups)
    lt = torch.from_numpy(logits)
    w, i = moe.grouped_topk_sigmoid(lt, torch.from_numpy(bias), n_groups, topk_group, topk)
    assert all(len(set(r)) == topk and max(r) < n_experts for r in i.tolist())
    if M.emulator_accepts(n_groups):
        scores = (1.0 / (1.0 + torch.exp(-lt))).numpy()
        w_emu, i_emu = grouped_topk_sigmoid_lanes(scores, bias, n_groups, topk_group, topk)
        assert np.array_equal(i.numpy(), i_emu) and np.allclose(w.numpy(), w_emu, rtol=1e-6, atol=1e-7)
    else:
        assert cfg == (1024, 64, 8, 8)
