"""CPU: the restatement of the sparse MoE block (tests/moe_block_ref.py) is the reference's DeepseekV3MoE, the pairing
cases are exact and refuse the mutants, and the new kernels were compiled without scratch (no GPU needed)."""
import os
import sys

import pytest
import torch

from tests import moe_block_ref as R
from tests.golden.generate_goldens import REFERENCE, import_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_CASES = [(dt, norm, n) for dt in R.DTYPES for norm in (False, True) for n in R.N_VALUES]


def _hold_to_reference(out, ids, ref_out, ref_ids, what):
    """Bit-equal where the reference's top-k came in the restatement's k order, within one ulp of T elsewhere (the fp32
    sum over k in another order)."""
    assert torch.equal(ids.sort(dim=1).values, ref_ids.sort(dim=1).values), f"{what}: other experts than the reference's"
    same_order = (ids == ref_ids).all(dim=1)
    assert torch.equal(out[same_order], ref_out[same_order]), f"{what}: differs from the reference in the reference's k order"
    d = R.ulp_distance(out, ref_out)
    assert int(d.max()) <= 1, f"{what}: {int(d.max())} ulp from the reference"


@pytest.mark.parametrize("dt,norm,n", BLOCK_CASES, ids=[R.fixture_key(*c) for c in BLOCK_CASES])
def test_restatement_is_the_stored_reference(dt, norm, n):
    c = R.block_case(dt, norm, n)
    wr, wgu, wdown, sgu, sdown = R.stacked(R.block_weights(dt))
    out, ids, _ = R.block(c.x, wr, wgu, wdown, sgu, sdown, R.TOPK, norm, R.SCALE, "T")
    _hold_to_reference(out, ids, c.ref_out, c.ref_ids, R.fixture_key(dt, norm, n))
    # the fixture's two conditions, re-measured
    _, _, p = R.route(c.x, wr, R.TOPK, norm, R.SCALE)
    top = p.sort(dim=-1, descending=True).values
    assert float((top[:, R.TOPK - 1] - top[:, R.TOPK]).min()) >= R.MIN_GAP * 0.99
    y64, _, _ = R.block(c.x, wr, wgu, wdown, sgu, sdown, R.TOPK, norm, R.SCALE, "f64", ids=c.ref_ids)
    ratio = R.error_ratio(c.ref_out, y64, R.TOL[dt])
    assert ratio <= 1.0 and abs(ratio - c.ref_ratio) < 1e-6


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "hydrainfer")), reason="needs a checkout of the reference")
@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_restatement_is_the_reference_module(dt):
    """The reference's own module, imported and run here on fresh inputs (not the fixture's)."""
    from tests.golden.generate_moe_block_golden import reference_moe
    import_reference()
    wr, wgu, wdown, sgu, sdown = R.stacked(R.block_weights(dt))
    x = torch.randn((37, R.H), generator=torch.Generator().manual_seed(5)).to(R.DTYPES[dt])
    with torch.no_grad():
        for norm in (False, True):
            moe = reference_moe(dt, norm)
            ref_ids, _ = moe.gate(x)
            out, ids, _ = R.block(x, wr, wgu, wdown, sgu, sdown, R.TOPK, norm, R.SCALE, "T")
            _hold_to_reference(out, ids, moe(x), ref_ids.to(torch.int32), f"{dt} norm={norm}")


def test_the_three_modes_agree_where_they_must():
    """ "exact" is "T" with float64 sums: on the fixture's inputs they differ by rounding only (<= 2 ulp after three
    chained roundings), and "f64" is within the tolerance of both."""
    c = R.block_case("bf16", True, 5)
    wr, wgu, wdown, sgu, sdown = R.stacked(R.block_weights("bf16"))
    a, ids, w = R.block(c.x, wr, wgu, wdown, sgu, sdown, R.TOPK, True, R.SCALE, "T")
    b, _, _ = R.block(c.x, wr, wgu, wdown, sgu, sdown, R.TOPK, True, R.SCALE, "exact", ids=ids, w=w)
    y64, _, _ = R.block(c.x, wr, wgu, wdown, sgu, sdown, R.TOPK, True, R.SCALE, "f64", ids=ids)
    assert int(R.ulp_distance(a, b).max()) <= 2
    assert R.error_ratio(a, y64, R.TOL["bf16"]) <= 1 and R.error_ratio(b, y64, R.TOL["bf16"]) <= 1


# ---------------------------------------------------------------------------------------------------------------------
# pairing cases
# ---------------------------------------------------------------------------------------------------------------------
def test_silu_of_the_gate_value_is_exact():
    assert R.silu_of_gate_is_exact()


@pytest.mark.parametrize("case", R.PAIRING_CASES, ids=[c.name for c in R.PAIRING_CASES])
@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_pairing_case_is_exact(case, dt):
    """The expected value does not depend on the summation order: the "exact" restatement (float64 sums) equals the "T"
    one (torch's fp32 accumulation) bit for bit, and again with every K axis reversed; the case's shape is what the
    issue's table says (every expert / one expert / past the 64-row tile ...)."""
    T = R.DTYPES[dt]
    p = R.build_pairing(case)          # asserts the fp32 exactness bounds (gemm_exact.assert_exact)
    want = R.pairing_expected(p, T)
    assert not torch.isnan(want).any()
    y = R.expert_rows(p.x.to(T), p.ids, p.wgu.to(T), p.wdown.to(T), "T")
    assert torch.equal(R.combine(y, p.w, p.shared.to(T), "T"), want)
    wgu_rev = torch.cat([p.wgu[:, :case.I].flip(1), p.wgu[:, case.I:].flip(1)], dim=1).flip(2)       # h and I reversed
    rev = R.expert_rows(p.x.flip(1).to(T), p.ids, wgu_rev.to(T), p.wdown.flip(2).to(T), "T")
    assert torch.equal(R.combine(rev, p.w, p.shared.to(T), "T"), want)
    counts = torch.bincount(p.ids.reshape(-1).long(), minlength=case.E)
    if case.routing == "one":
        assert sorted(counts.tolist())[-2:] == [0, case.n] and int((counts == 0).sum()) == case.E - 1
    if case.name == "two-experts-70-rows":
        assert counts.tolist() == [70, 70]
    if case.name == "every-expert-one-row":
        assert counts.tolist() == [1] * 8
    # a token's experts are distinct, the one-hot columns too
    assert all(len(set(r)) == case.topk for r in p.ids.tolist())
    assert p.x.sum(dim=0).max() == 1 and bool((p.x.sum(dim=1) == 1).all())


@pytest.mark.parametrize("case", R.PAIRING_CASES, ids=[c.name for c in R.PAIRING_CASES])
def test_pairing_case_refuses_the_mutants(case):
    T = torch.bfloat16
    p = R.build_pairing(case)
    want = R.pairing_expected(p, T)
    applied = 0
    for mutant in ("swap_k", "next_expert", "token_mod"):
        got = R.pairing_expected(p, T, **{mutant: True})
        if got is None:
            continue
        if mutant == "token_mod" and (case.topk == 1 or case.n == 1):
            assert torch.equal(got, want)       # s % n == s / topk when topk == 1 or n == 1: not a mutant there
            continue
        applied += 1
        assert not torch.equal(got, want), f"{case.name}: the checker cannot tell the {mutant} mutant"
    assert applied >= 1
    assert not torch.equal(R.pairing_expected(p, T, shared=False), want)


def test_every_mutant_is_refused_somewhere():
    T = torch.bfloat16
    for mutant in ("swap_k", "next_expert", "token_mod"):
        hits = 0
        for case in R.PAIRING_CASES:
            p = R.build_pairing(case)
            got = R.pairing_expected(p, T, **{mutant: True})
            hits += got is not None and not torch.equal(got, R.pairing_expected(p, T))
        assert hits >= 3, mutant


def test_tiny_model_inputs_are_sound():
    """tests/test_gpu_moe_model.py: on its seeded tiny model the routed experts move the logits by more than 4
    tolerances (the logits' own scale is ~1 and the bf16 tolerance 0.15: a wrong expert cannot hide inside it), and every
    routing decision that reaches a logit has the fixture's routing gap (a logit summed in another order picks the same
    experts)."""
    from tests import test_gpu_moe_model as TM
    for dname, tol in TM.LOGIT_TOL.items():
        ref = TM.cpu_run(dname)
        assert ref["moved"] > 4 * tol, (dname, ref["moved"])
        assert ref["gap"] >= R.MIN_GAP, (dname, ref["gap"])
        print(dname, "moved", ref["moved"], "gap", ref["gap"])


# ---------------------------------------------------------------------------------------------------------------------
# resources
# ---------------------------------------------------------------------------------------------------------------------
def test_moe_expert_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    new = [r for r in kernel_table.kernels() if r["name"].startswith(("moe_gemm_kernel<", "moe_gate_topk_kernel<",
                                                                      "moe_segments_kernel", "moe_combine_kernel<"))]
    assert len(new) == 12 + 4 + 1 + 2, sorted(r["name"] for r in new)
    for r in new:
        assert r.get("private_segment_fixed_size", 0) == 0 and r.get("vgpr_spill_count", 0) == 0, r
        assert r.get("sgpr_spill_count", 0) == 0 and r.get("wavefront_size") == 64, r
