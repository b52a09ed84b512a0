"""No GPU: what tests/test_gpu_decode_arms.py rests on, shown on the oracle and the host planning queries.
SOUND: the T oracle's own distance E_T from the fp32 oracle — the unit of the GPU file's bar — is non-zero and a few
ulps of T, for every shape, n in {1, 17, 33, 64} and both dtypes.  SENSITIVE: every kept mutant of the oracle (one row's
stale hand-over, rows 16 / 17 swapped, a skipped residual add, the wrong final-norm weight, K written one slot early)
misses the fp32 oracle by more than 10 x that bar; tests/decode_arms.py says where a mutant is dropped and why.
SHAPES: through the host queries alone (256 CUs assumed without a device) every arm of ARMS still plans what the table
says at every row count it runs, so a changed `supported` predicate that moves a shape to another arm fails here and
names the arm that lost its shape."""
import math

import pytest
import torch

from tests import decode_arms as A

SOUND = [(s, n, d) for s in A.SHAPES for d in A.DTYPES for n in (1, 17, 33, 64)]


def _ulp(dname: str, magnitude: float) -> float:
    return 2.0 ** (math.floor(math.log2(magnitude)) - {"fp16": 10, "bf16": 7}[dname])


@pytest.mark.parametrize("dname", list(A.DTYPES))
def test_hooked_oracle_is_the_oracle(dname):
    c = A.case("A", 33, dname)
    for T in (A.DTYPES[dname], torch.float32):
        l0, k0, p0 = A.reference(c, T)
        l1, k1, p1 = A.reference(c, T, A.HookedOracle)
        assert torch.equal(l0, l1) and torch.equal(p0, p1)
        assert not torch.equal(p0, c.pool.to(T))


def test_case_is_what_the_gpu_file_assumes():
    for n in A.LOW_ROWS + A.HIGH_ROWS + (A.GENERIC_ROWS,):
        c = A.case("A", n, "fp16")
        assert len(c.ctx) == n and 1 <= min(c.ctx) and max(c.ctx) <= A.MAX_CTX
        assert set(c.ctx) >= set([17, 16, 1][:n])
        blocks = [b for t in c.tables for b in t]
        assert all(len(t) == (k + A.BS - 1) // A.BS for t, k in zip(c.tables, c.ctx))
        assert len(set(blocks)) == len(blocks) and c.pool.shape[2] == len(blocks) + 3      # three unreferenced pages
        if n >= 16:
            assert blocks != sorted(blocks) and c.ctx != sorted(c.ctx)
        assert len(set(c.slots.tolist())) == n
        m = c.meta()
        assert m.kv_cu_seq_lens[-1] == sum(c.ctx) and m.cu_blocks_lens[-1] == len(blocks)
    c = A.case("A", 17, "fp16")
    perm = torch.randperm(17, generator=torch.Generator().manual_seed(17)).tolist()
    cp = c.permuted(perm)
    assert cp.slots.tolist() == c.slots[perm].tolist() and cp.ids.tolist() == c.ids[perm].tolist()
    assert cp.pool is c.pool
    # a permuted step is the same step: the oracle's logits permute, its pool does not change
    l0, _, p0 = A.reference(c, torch.float16)
    l1, _, p1 = A.reference(cp, torch.float16)
    assert torch.equal(l1, l0[perm]) and torch.equal(p0, p1)


@pytest.mark.parametrize("shape,n,dname", SOUND, ids=[f"{s}-{n}-{d}" for s, n, d in SOUND])
def test_bar_is_sound_and_mutants_are_caught(shape, n, dname):
    c = A.case(shape, n, dname)
    lt, kt, pt = A.reference(c, A.DTYPES[dname])
    l32, k32, p32 = A.reference(c, torch.float32)
    e_l, e_k = (lt - l32).abs().max().item(), (kt - k32).abs().max().item()
    # non-zero (the two oracles do round differently) and small: three layers of a few roundings each stay within 8 ulps
    # of T at the largest magnitude (measured: at most 2.6)
    assert 0 < e_l <= 8 * _ulp(dname, l32.abs().max().item()), e_l
    assert 0 < e_k <= 8 * _ulp(dname, k32.abs().max().item()), e_k
    # the oracle writes the n x 3 rows and nothing else
    keep = torch.ones(c.pool.shape[2] * A.BS, dtype=torch.bool)
    keep[c.slots.long()] = False
    flat = lambda p: p.reshape(A.LAYERS, 2, -1, *p.shape[4:])
    assert torch.equal(flat(pt)[:, :, keep], flat(c.pool)[:, :, keep])
    assert torch.equal(flat(p32)[:, :, keep], flat(c.pool.float())[:, :, keep])
    bar_l, bar_k = A.BAR_FACTOR[dname] * e_l, A.BAR_FACTOR[dname] * e_k
    kept = []
    for M in A.MUTANTS:
        if not A.mutant_applies(M, c):
            continue
        lm, km, _ = A.reference(c, torch.float32, M)
        margin = max((lm - l32).abs().max().item() / bar_l, (km - k32).abs().max().item() / bar_k)
        print(f"\nMUTANT {shape} {n} {dname} {M.__name__}: misses by {margin:.1f} x the bar")
        assert margin > A.MUTANT_MARGIN, f"{M.__name__} misses the fp32 oracle by only {margin:.1f} x the bar"
        kept.append(M.__name__)
    assert {"StaleHandover", "KeyOneSlotEarly"} <= set(kept) or (n == 1 and max(c.ctx) == 1)
    assert dname != "fp16" or len(kept) == len(A.MUTANTS) - (n < 18)


def test_dropped_mutants_are_listed_not_run():
    names = {M.__name__ for M in A.MUTANTS}
    assert all(m in names and d in A.DTYPES and set(s) <= set(A.SHAPES) for (m, d), s in A.DROPPED.items())
    assert not any(d == "fp16" for _, d in A.DROPPED)


@pytest.mark.parametrize("arm", A.ARMS, ids=[a.name for a in A.ARMS])
def test_shape_still_reaches_its_arm(arm):
    for n in arm.rows():
        got = A.host_plan(arm.shape, arm.sw, n)
        if n > 64:
            assert got is None
            continue
        want = A.PLAN_OF[arm.family(n)]
        assert got == want, (f"arm {arm.name} lost its shape {A.SHAPES[arm.shape]} at {n} rows: the host queries now plan "
                             f"{got}, the table says {arm.family(n)} = {want}")
    # what tells the ':fm' qkv launches of layers >= 1 from LDS-slice ones
    lds_qkv = {"lds8", "rowmajor8", "xreg6_gu_lds_qkv", "xreg7_lds_qkv"}
    for fam in (arm.low, arm.high):
        if fam is not None and fam not in lds_qkv:
            assert A.host_qkv_packed(arm.shape, arm.sw), (arm.name, fam)


def test_the_table_is_the_issue_s_table():
    """The five shapes answer the queries the way each row of the table needs, query by query."""
    from hydrainfer_amd import _lib
    l = _lib.lib()
    for key, (hid, inter, _) in A.SHAPES.items():
        for n in A.LOW_ROWS:      # every shape runs its MLP and its qkv on the narrow kernel
            assert l.hx_linear_decode_xreg_supported(n, 2 * inter, hid) == 1 and l.hx_linear_decode_xreg_supported(n, hid, inter) == 1
            assert l.hx_linear_decode_xreg_supported(n, 3 * hid, hid) == 1
            assert (l.hx_gate_up_silu_xreg_supported(n, inter, hid) == 1) == (key != "C"), (key, n)
            assert (l.hx_norm_xreg_supported(n, 2 * inter, hid, 1) == 1) == (key != "C"), (key, n)
            assert (l.hx_norm_xreg_supported(n, 3 * hid, hid, 0) == 1) == (key in "ADE"), (key, n)
        for n in A.HIGH_ROWS:
            wide = (l.hx_gate_up_xreg_supported(n, inter, hid, 0) == 1 and l.hx_linear_decode_xreg_supported(n, hid, inter) == 1
                    and l.hx_linear_decode_xreg_supported(n, 3 * hid, hid) == 1)
            assert wide == (key != "D"), (key, n)
            if wide:
                assert (l.hx_gate_up_xreg_supported(n, inter, hid, 1) == 1) == (key != "C"), (key, n)
                assert (l.hx_gate_up_silu_wide_xreg_supported(n, inter, hid) == 1) == (key == "E"), (key, n)


def test_arms_table_is_consistent():
    assert set(A.PLAN_OF) == set(A.SEQUENCES) - {"generic"}
    assert {a.family(n) for a in A.ARMS for n in a.rows()} == set(A.SEQUENCES)          # no family without an arm
    assert {a.shape for a in A.ARMS if a.generic} == set(A.SHAPES)
    launches = {f: [len(s) for s in seq] for f, seq in A.SEQUENCES.items()}
    assert launches["lds8"] == launches["rowmajor8"] == [8, 8, 8]
    assert launches["xreg7"] == [7, 7, 7] and launches["xreg5"] == [6, 5, 5]      # layer 0's qkv is a launch of its own
    assert launches["wide6"] == [7, 6, 6] and launches["wide5"] == [6, 5, 5] and launches["xreg8_silu"] == [8, 8, 8]
    for f, seq in A.SEQUENCES.items():
        assert all(s.count(A.ATT) == 1 for s in seq)
        if f != "generic":
            assert seq[2][-1] == A.NORM, f      # the final norm lands row-major
            p = A.PLAN_OF[f]
            assert (A.NLX in seq[0]) == p["nf_qkv"] and (A.NGUSW in seq[1]) == p["wide_silu"]
            assert any(x in seq[1] for x in (A.NGUS, A.NGU, A.NGUSW)) == p["nf_gu"]
    for a, b, rows in A.FAMILIES_BIT_IDENTICAL:
        assert A.ARM[a].shape == A.ARM[b].shape and all(A.ARM[a].family(n) and A.ARM[b].family(n) for n in rows)


def test_spy_wraps_every_call_site_and_restores():
    from hydrainfer_amd import _lib
    from hydrainfer_amd.model import llama
    sites = A.call_sites()
    gemm_sites = sites - {"add_rms_norm_slabs", "silu_and_mul_slabs", "decode_attention_fused", "rms_norm"}
    assert gemm_sites <= set(A.GEMM_WRAPPERS) and len(gemm_sites) >= 9, gemm_sites
    before = (llama.hip_gemm.linear_decode_ex, llama.rms_norm, _lib.memset_zero)
    with A.spy() as seen:
        assert llama.hip_gemm.linear_decode_ex is not before[0] and llama.rms_norm is not before[1]
        assert _lib.memset_zero is not before[2] and list(seen) == []
    assert (llama.hip_gemm.linear_decode_ex, llama.rms_norm, _lib.memset_zero) == before


# ---------------------------------------------------------------------------------------------------------------------
# the resolved step plan (hydrainfer_amd/model/decode_plan.py) and a dry run of the layer body, both without a device
# ---------------------------------------------------------------------------------------------------------------------
_dry_states = {}


def _dry_model(arm, dname):
    """The arm's three-layer model on uninitialised CPU tensors (no launch reads them) after what prepare_decode(64)
    would do without packing anything: the layout record of decode_plan.plan_layouts — the statement pack_decode_weights
    packs by — and a placeholder in the layout dicts for every key the record names."""
    from hydrainfer_amd.model.decode_plan import plan_layouts
    from hydrainfer_amd.model.llama import LlamaForCausalLM
    dt, sh = A.DTYPES[dname], A.llama_shape(arm.shape)
    if (arm.shape, dname) not in _dry_states:
        hid, inter = sh.hidden_size, sh.intermediate_size
        sizes = {"wqkv": (3 * hid, hid), "wo": (hid, hid), "wgu": (2 * inter, hid), "wdown": (hid, inter), "norm1": (hid,), "norm2": (hid,)}
        st = {f"l{l}.{k}": torch.empty(s, dtype=dt) for l in range(A.LAYERS) for k, s in sizes.items()}
        st.update(embed=torch.zeros((A.VOCAB, hid), dtype=dt), lm_head=torch.zeros((A.VOCAB, hid), dtype=dt), norm=torch.empty(hid, dtype=dt))
        _dry_states[(arm.shape, dname)] = st
    model = LlamaForCausalLM(sh, dt, "cpu", dict(_dry_states[(arm.shape, dname)]))
    arm.sw.apply(model)
    lay = plan_layouts(model.dims, dt, arm.sw, all_lds_slice=not model._wide_ok(64))        # as prepare_decode(64) asks
    for k in lay.xreg_keys(A.LAYERS):
        model.packed_x[k] = model.dw[k] = object()
    for k in lay.lds_slice:
        model.packed[k] = model.dw_lds[k] = object()
    model.decode_layouts, model.decode_rows_prepared = lay, 64
    return model


DRY = [(a, d) for a in A.ARMS for d in A.DTYPES]


@pytest.mark.parametrize("arm,dname", DRY, ids=[f"{a.name}-{d}" for a, d in DRY])
def test_resolver_plans_what_the_table_says(arm, dname):
    """decode_plan.resolve on the arm's switches and the layout record of its shape: the six flags are the table's and
    the independent restatement's (host_plan), the record is host_qkv_packed's, at every row count the arm runs."""
    from hydrainfer_amd.model.decode_plan import resolve
    model = _dry_model(arm, dname)
    lay = model.decode_layouts
    assert lay.qkv_xreg == A.host_qkv_packed(arm.shape, arm.sw)
    assert set(lay.lds_slice) >= {f"l{l}.wo" for l in range(A.LAYERS)} | {"l0.wqkv"} or not arm.sw.use_packed
    # a second (LDS-slice) copy of a projection exactly where 64 rows cannot run on the activations-in-registers one
    xk = set(lay.xreg_keys(A.LAYERS))
    assert bool(set(lay.lds_slice) & xk) == (bool(xk) and not model._wide_ok(64))
    for n in arm.rows():
        if n <= 64:
            plan = resolve(model.dims, n, A.DTYPES[dname], arm.sw, lay)
            assert plan.flags() == A.PLAN_OF[arm.family(n)] == A.host_plan(arm.shape, arm.sw, n), (arm.name, n, plan)
            assert plan.flags() == model._decode_plan(n, A.DTYPES[dname])
            assert (plan.ws_q is not None) == plan.flags()["nf_qkv"] and plan.xf == plan.flags()["xreg"]
            assert (plan.ws_gu is not None) == (plan.flags()["wide"] and not plan.flags()["wide_silu"])


@pytest.mark.parametrize("arm,dname", DRY, ids=[f"{a.name}-{d}" for a, d in DRY])
def test_dry_run_of_the_layer_body(arm, dname):
    """The real forward_logits on the "embeds" feed with every launch wrapper stubbed (tests/decode_arms.py::dry_stubs):
    the layer body assembles the arm's launch sequence, layer by layer, and zeroes a hand-over area of its own exactly
    where the plan has a hand-over."""
    model = _dry_model(arm, dname)
    heads = A.SHAPES[arm.shape][2]
    for n in arm.rows():
        if n > 64:
            continue
        c = A.Case(arm.shape, dname, n, torch.zeros(n, dtype=torch.int64), [1] * n, [[i] for i in range(n)],
                   torch.empty((A.LAYERS, 2, n, A.BS, heads, A.HEAD_DIM), dtype=A.DTYPES[dname]))
        logits, seen = A.device_step(model, c, "cpu", c.pool, "embeds", stubs=A.dry_stubs())
        fam, plan = arm.family(n), model._step_plan(n, A.DTYPES[dname])
        assert logits.shape == (n, A.VOCAB)
        for l in range(A.LAYERS):
            assert seen.layer(l) == A.SEQUENCES[fam][l], f"layer {l} of {arm.name} at {n} rows"
        assert plan.sync == (A.PLAN_OF[fam]["nf_gu"] or A.PLAN_OF[fam]["nf_qkv"])
        assert seen.layer(A.HEAD) == (["memset_zero", "rms_norm"] if plan.sync else ["rms_norm"])
        assert (model.xreg_sync is not None) == plan.sync
        model.xreg_sync = None


def test_the_layer_body_decides_nothing():
    """The body and its stage functions read the plan: no switch, no packed_x membership, no support query."""
    import inspect
    for f in A.decode_layer_functions():
        src = inspect.getsource(f)
        for banned in ("in self.packed_x", "_gu_interleaved", "_supported(", "self.use_", "self.fuse_norm", "self.xreg_qkv"):
            assert banned not in src, (f.__name__, banned)
