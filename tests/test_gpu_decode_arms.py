"""-m gpu: every launch sequence ("arm") LlamaForCausalLM._decode_hidden_hip_gemm can choose, run as a three-layer model
on the smallest shape that reaches it (tests/decode_arms.py: ARMS), at 1 / 16 / 17 / 32 rows or 33 / 48 / 64 rows, both
dtypes, plus the generic loop at 65 rows once per shape.  Per case:
  a. the arm is the arm: model._decode_plan equals the table, the spied launch list equals the arm's per layer;
  b. logits and the written KV rows within BAR_FACTOR x E_T of the fp32 oracle (E_T = the T oracle's own distance from
     it), every other element of the pool bit-identical to the input pool, no hand-over gave up;
  d. the same requests in another order: the same logits rows, permuted, and the same pool, bit for bit;
  e. int64 ids, int32 ids and embeddings give the same bits (the first two zero the sync areas in the step head: no
     memset_zero launch; the third zeroes a fresh area: exactly one, where the plan has a hand-over);
  f. the step a second time on a restored pool gives the same bits.
Then: (c) arms that differ only by fusions proven bit-identical at operator level agree bit for bit; one representative
per launch family through DecodeRunner under the eager, hipGraph and launch-plan executors; and, last, the coverage gate:
every launch-wrapper call site of the decode layer and every plan of ARMS was reached in this run.
Run with -s for the ARM-RATIO lines (error / E_T per case), which profiles/decode_arm_tests.md records."""
import pytest
import torch

from tests import decode_arms as A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_models, _refs = {}, {}
_seen_names, _plans_run, _families_run = set(), [], set()


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    for m in _models.values():
        m.release()
    _models.clear()
    _refs.clear()
    torch.cuda.empty_cache()


def _model(arm: A.Arm, dname: str):
    key = (arm.shape, dname, arm.sw)
    if key not in _models:
        _models[key] = A.build_model(arm.shape, dname, arm.sw, DEV)
    return _models[key]


def _ref(shape: str, n: int, dname: str):
    """(case, fp32 logits, fp32 KV rows, E_T of the logits, E_T of the KV rows): computed once, never written."""
    key = (shape, n, dname)
    if key not in _refs:
        c = A.case(shape, n, dname)
        lt, kt, _ = A.reference(c, A.DTYPES[dname])
        l32, k32, _ = A.reference(c, torch.float32)
        e_l, e_k = (lt - l32).abs().max().item(), (kt - k32).abs().max().item()
        assert e_l > 0 and e_k > 0
        _refs[key] = (c, l32, k32, e_l, e_k)
    return _refs[key]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _run(model, c, pool0_d, feed="int64"):
    pool = pool0_d.clone()
    logits, seen = A.device_step(model, c, DEV, pool, feed)
    _seen_names.update(seen.names())
    return logits, pool, seen


CASES = [(a.name, n, d) for a in A.ARMS for d in A.DTYPES for n in a.rows()]


@pytest.mark.parametrize("arm_name,n,dname", CASES, ids=[f"{a}-{n}-{d}" for a, n, d in CASES])
def test_arm(arm_name, n, dname):
    arm = A.ARM[arm_name]
    fam, dt = arm.family(n), A.DTYPES[dname]
    model = _model(arm, dname)
    c, l32, k32, e_l, e_k = _ref(arm.shape, n, dname)
    pool0 = c.pool.to(DEV)

    # ---- a. the arm is the arm
    nf = False
    if n <= 64:
        plan = model._decode_plan(n, dt)
        assert plan == A.PLAN_OF[fam], f"{arm_name} at {n} rows plans {plan}: the shape no longer reaches {fam}"
        nf = plan["nf_gu"] or plan["nf_qkv"]
        _plans_run.append(plan)
    _families_run.add(fam)
    logits, pool, seen = _run(model, c, pool0)
    torch.cuda.synchronize()
    assert seen.layer(A.HEAD) == (["decode_step_head"] if n <= 64 else ["rms_norm"])
    for l in range(A.LAYERS):
        assert seen.layer(l) == A.SEQUENCES[fam][l], f"layer {l} of {arm_name} at {n} rows"
    assert {k for _, k in seen} == {A.HEAD, 0, 1, 2}
    assert (model.xreg_sync is not None) or not nf
    assert not model.handover_failed()

    # ---- b. against the high-precision reference
    got_l = logits.float().cpu()
    got_k = A.written_rows(c, pool).float().cpu()
    assert torch.isfinite(got_l).all() and torch.isfinite(got_k).all()
    r_l, r_k = (got_l - l32).abs().max().item() / e_l, (got_k - k32).abs().max().item() / e_k
    print(f"\nARM-RATIO {arm_name} {n} {dname} {fam} E_T {e_l:.3e} {e_k:.3e} ratio {r_l:.3f} {r_k:.3f}")
    assert r_l <= A.BAR_FACTOR[dname], f"logits {r_l:.2f} x E_T ({e_l:.3e}) from the fp32 oracle"
    assert r_k <= A.BAR_FACTOR[dname], f"written KV rows {r_k:.2f} x E_T ({e_k:.3e}) from the fp32 oracle"
    keep = torch.ones(pool.shape[2] * A.BS, dtype=torch.bool, device=DEV)
    keep[c.slots.long().to(DEV)] = False
    flat = lambda p: _bits(p).reshape(A.LAYERS, 2, -1, *p.shape[4:])
    assert torch.equal(flat(pool)[:, :, keep], flat(pool0)[:, :, keep]), "a cache row the step does not own changed"
    assert not torch.equal(flat(pool)[:, :, ~keep], flat(pool0)[:, :, ~keep])

    # ---- f. twice in the same process
    logits2, pool2, seen2 = _run(model, c, pool0)
    assert list(seen2) == list(seen)
    assert _same_bits(logits2, logits) and _same_bits(pool2, pool), "the second run of the same step differs"

    # ---- e. both ways into the step
    assert "memset_zero" not in seen.names()
    logits3, pool3, seen3 = _run(model, c, pool0, "int32")
    assert list(seen3) == list(seen)
    assert _same_bits(logits3, logits) and _same_bits(pool3, pool), "int32 ids differ from int64 ids"
    logits4, pool4, seen4 = _run(model, c, pool0, "embeds")
    assert seen4.layer(A.HEAD) == (["memset_zero"] if nf else []) + ["rms_norm"]
    assert [x for x in seen4 if x[1] != A.HEAD] == [x for x in seen if x[1] != A.HEAD]
    assert _same_bits(logits4, logits) and _same_bits(pool4, pool), "embeddings differ from token ids"
    assert not model.handover_failed()

    # ---- d. row order does not matter
    if n > 1:
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).tolist()
        assert perm != list(range(n))
        logits5, pool5, seen5 = _run(model, c.permuted(perm), pool0)
        assert list(seen5) == list(seen)
        assert _same_bits(logits5, logits[torch.tensor(perm, device=DEV)]), "logits depend on the order of the requests"
        assert _same_bits(pool5, pool), "the pool depends on the order of the requests"
        assert not model.handover_failed()


TWINS = [(a, b, n, d) for a, b, rows in A.FAMILIES_BIT_IDENTICAL for d in A.DTYPES for n in rows]


@pytest.mark.parametrize("arm_name,twin_name,n,dname", TWINS, ids=[f"{a}=={b}-{n}-{d}" for a, b, n, d in TWINS])
def test_arms_of_one_family_are_bit_identical(arm_name, twin_name, n, dname):
    """c. Arms that differ only by fusions the operator tests prove bit-identical give the same logits and pool."""
    arm, twin = A.ARM[arm_name], A.ARM[twin_name]
    assert arm.shape == twin.shape and arm.family(n) != twin.family(n)
    c = _ref(arm.shape, n, dname)[0]
    pool0 = c.pool.to(DEV)
    la, pa, sa = _run(_model(arm, dname), c, pool0)
    lb, pb, sb = _run(_model(twin, dname), c, pool0)
    for l in range(A.LAYERS):
        assert sa.layer(l) == A.SEQUENCES[arm.family(n)][l] and sb.layer(l) == A.SEQUENCES[twin.family(n)][l]
    assert _same_bits(la, lb), f"{arm_name} and {twin_name} give different logits at {n} rows"
    assert _same_bits(pa, pb), f"{arm_name} and {twin_name} give different pools at {n} rows"


EXECUTOR_ARMS = ["A", "A-no_fuse_norm", "B", "C", "D", "E", "E-no_wide_silu", "A-no_xreg"]


@pytest.mark.parametrize("rows", [5, 33])
@pytest.mark.parametrize("arm_name", EXECUTOR_ARMS)
def test_executors_agree(arm_name, rows):
    """A 12-token prompt and 24 steps (contexts 13 .. 36: two block boundaries) through DecodeRunner: eager launches,
    the captured hipGraph and the launch plan give the same tokens and the same pool, bit for bit; no hand-over gave up.
    bf16, the benchmark's dtype (the dtype dispatch of every arm is in test_arm)."""
    from hydrainfer_amd.model.runner import DecodeRunner, RunnerConfig
    arm = A.ARM[arm_name]
    model = _model(arm, "bf16")
    plan = model._decode_plan(rows, torch.bfloat16)
    fam = arm.family(rows) or A.ARM[arm.shape].family(rows)       # a switch that is not read at these rows: the shape's default
    assert plan == A.PLAN_OF[fam]
    prompts = torch.randint(5, 2000, (rows, 12), generator=torch.Generator().manual_seed(0)).to(DEV)
    outs = []
    for use_graph, executor in ((False, "graph"), (True, "graph"), (True, "plan")):
        r = DecodeRunner(model, RunnerConfig(batch=rows, prompt_len=12, n_generate=32, use_graph=use_graph,
                                             executor=executor), seed=4)
        r.prefill(prompts)
        for _ in range(24):
            r.step()
        torch.cuda.synchronize()
        assert not model.handover_failed()
        if use_graph:
            assert r.graph is not None and r.executor_used == executor
        outs.append((r.generated(), r.pool.clone()))
        del r
    assert outs[0][0].shape == (25, rows)
    for toks, pool in outs[1:]:
        assert torch.equal(toks, outs[0][0]), "an executor sampled other tokens than the eager launches"
        assert _same_bits(pool, outs[0][1]), "an executor left another KV pool than the eager launches"


def test_coverage_gate():
    """Last: every launch wrapper named in the decode layer's source was seen by a spy in this run, every family of
    launch sequences and every distinct plan of ARMS was run.  A new call site without an arm that reaches it fails here.
    (Meaningful after the whole file has run: a selection that leaves arms out fails it.)"""
    sites = A.call_sites()
    assert sites - {"add_rms_norm_slabs", "silu_and_mul_slabs", "decode_attention_fused", "rms_norm"} <= set(A.GEMM_WRAPPERS), \
        "a launch wrapper the spy does not wrap"
    assert len(sites) >= 13, sites
    missing = sites - _seen_names
    assert not missing, f"call sites of the decode layer no arm reached: {sorted(missing)}"
    want_fams = {a.family(n) for a in A.ARMS for n in a.rows()}
    assert want_fams == set(A.SEQUENCES) and _families_run == want_fams, want_fams ^ _families_run
    freeze = lambda p: tuple(sorted(p.items()))
    want = {freeze(p) for p in A.PLAN_OF.values()}
    assert {freeze(p) for p in _plans_run} == want
