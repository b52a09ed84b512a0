"""CPU: every host-side answer of the activations-in-registers decode GEMMs (csrc/gemm_xreg.hip) equals the pinned
table tests/golden/xreg_plan_table.json (tests/golden/generate_xreg_plan_table.py): supported / splits / slab counts
of the eight planning entries over 8 x 14 x 178 shapes, hx_decode_weight_plan's (status, layout, flags), and the
status of each launch entry for one argument defect.  Packed weights, workspaces and the launch sequence of the decode
step all depend on these answers; no device is needed for any of them (256 CUs are assumed without one)."""
import json

import pytest
import torch

from hydrainfer_amd import _lib
from tests.golden import generate_xreg_plan_table as G


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        return json.load(f)


def test_the_table_is_not_constant(golden):
    """A generator that recorded nothing would pass the comparison: every predicate answers both ways on the grid,
    split counts 1 .. 4 occur, and both layouts are planned."""
    want = G.decode(golden)
    assert len(want) == len(G.N_VALUES) * len(G.k_values()) == 14 * 178
    points = [a for per_m, _, _ in want.values() for a in per_m]
    assert len(points) == 8 * 14 * 178
    for i, name in enumerate(G.POINT_FIELDS):
        seen = {a[i] for a in points}
        if name.endswith("_slabs"):
            assert {0, 1, 2} <= seen, (name, seen)
        else:
            assert seen == {0, 1}, (name, seen)
    supported = sum(a[0] for a in points) / len(points)
    assert 0.7 < supported < 0.9, supported
    assert {s for _, s, _ in want.values()} == {-2, 1, 2, 3, 4}
    plans = {a for _, _, p in want.values() for a in p}
    assert {(0, _lib.HX_DW_LDS_SLICE, 0), (0, _lib.HX_DW_XREG, 0), (0, _lib.HX_DW_XREG, _lib.HX_DW_GATE_UP)} <= plans
    assert any(rc < 0 for rc, _, _ in plans)


def test_planning_answers_equal_the_pinned_table(golden):
    want = G.decode(golden)
    got = G.sweep(_lib.lib())
    assert got.keys() == want.keys()
    wrong = []
    for (N, K), (per_m, splits, plans) in want.items():
        g_m, g_splits, g_plans = got[(N, K)]
        for M, a, b in zip(G.M_VALUES, per_m, g_m):
            wrong += [f"{f}(M={M}, N={N}, K={K}): {y}, pinned {x}" for f, x, y in zip(G.POINT_FIELDS, a, b) if x != y]
        if splits != g_splits:
            wrong.append(f"hx_linear_decode_xreg_splits(N={N}, K={K}): {g_splits}, pinned {splits}")
        for (r, fl), a, b in zip(((r, fl) for r in G.PLAN_ROWS for fl in G.PLAN_FLAGS), plans, g_plans):
            if a != b:
                wrong.append(f"hx_decode_weight_plan(N={N}, K={K}, max_rows={r}, flags={fl}): {b}, pinned {a}")
    assert not wrong, f"{len(wrong)} answers differ, the first: {wrong[:8]}"


# With a device, a regression that let one of these calls through would launch a kernel on the fake pointers; without
# one the launch only returns an error and the test fails harmlessly.
@pytest.mark.skipif(torch.cuda.is_available(), reason="defective calls on fake pointers: only where nothing can launch")
def test_one_defect_per_call_gives_the_pinned_status(golden):
    want = golden["arg_checks"]
    entries = {name.split(":")[0] for name in want}
    assert len(entries) == 9 and {-1, -2, -3, -4, -6} == set(want.values())
    for e in entries:      # null pointer, unsupported shape, bad dtype code, misaligned pointer (and, where the entry takes one, a short workspace)
        assert {f"{e}:null", f"{e}:shape", f"{e}:dtype", f"{e}:misaligned"} <= set(want), e
    assert sum(name.endswith(":workspace") for name in want) == 5
    assert G.arg_check_statuses(_lib.lib()) == want
