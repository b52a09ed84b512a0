"""No GPU: every case tests/test_gpu_attention_probes.py runs is shown, on the oracle, to be SOUND (the precondition
holds — the target leads every other visible key by MIN_GAP_LOG2 — and the oracle returns V[t] bit for bit; poisoned
pools leave the oracle finite and unchanged) and SENSITIVE (the same case with a mask moved by one key is refused by
the very assertion the GPU file applies).  The case lists live in tests/attn_probe.py: what is proven here is what runs."""
import pytest
import torch

from tests import attn_probe as A

IDS = [c.name for _, c in A.ALL_CASES]
CASES = [c for _, c in A.ALL_CASES]


def test_case_lists_cover_what_the_issue_names():
    cs = CASES
    assert {c.D for c in cs} >= {32, 64, 96, 128, 256} and {c.bs for c in cs} >= {0, 16, 32, 64}
    assert {c.dt for c in cs} == {"fp16", "bf16"}
    assert {c.window for c in cs if c.window} == set(A.WINDOWS)
    assert {(c.H, c.HK) for c in A.GQA_DECODE} >= {(8, 4), (28, 4), (16, 1)}
    lens = {l for c in A.PER_HEAD_DECODE + A.GQA_DECODE for l in c.kv_lens}
    assert lens >= set(A.EDGE_LENS)
    for group in (A.PER_HEAD_DECODE, A.GQA_DECODE):
        ts = {t for c in group if c.aim == "targets" for t in c.targets}
        assert ts >= set(A.TILE_EDGES) | set(A.split_edges(1500)) | {0}
        for bs in (16, 32, 64):
            assert any(c.bs == bs and {bs - 1, bs} <= set(c.targets) for c in group if c.aim == "targets"), bs
    assert all(len(c.kv_lens) <= 32 and max(c.kv_lens) <= 4096 for c in cs)
    assert all(c.H <= 8 or (c.H, c.HK) in ((32, 32), (28, 4), (16, 1)) for c in cs)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_probe_is_sound(case):
    p = A.probe(case)
    out = A.oracle(p)
    assert torch.isfinite(out.float()).all()
    if case.exact:
        gap = A.min_gap_log2(p)
        assert gap >= A.MIN_GAP_LOG2, f"{case.name}: gap {gap:.1f} log2 units"
        assert torch.equal(out, p.expected), "the oracle does not return V[t] bit for bit"
    A.check(p, out)
    if case.bs > 0:
        for kind in A.POISONS:
            kc, vc = A.poisoned(p, kind)
            assert not torch.isfinite(kc.float()).all()
            assert not torch.isfinite(kc[0].float()).any(), "physical block 0 must be poisoned: no table may hold it"
            o2 = A.oracle(p, kc=kc, vc=vc)
            assert torch.equal(o2.view(torch.int16), out.view(torch.int16)), kind
            A.check(p, o2)


@pytest.mark.parametrize("case", A.FUSED_DECODE, ids=[c.name for c in A.FUSED_DECODE])
def test_fused_probe_is_sound(case):
    """The fused form of the case (last key out of the cache, in as k_new / v_new; RoPE at position kv_len - 1): the
    precondition on the oracle's rotated q against the cache as stored, V[t] bit for bit, and poison-proof."""
    p = A.probe(case)
    fi = A.fused_inputs(p)
    out, qr, kc, vc = A.fused_oracle(p, fi)
    gap = A.min_gap_log2(p, q=qr, kc=kc)
    assert gap >= A.MIN_GAP_LOG2, f"{case.name}: gap {gap:.1f} log2 units"
    assert torch.equal(out, p.expected)
    written = ~A.addressed_mask(p, drop_last=True) & A.addressed_mask(p)
    assert int(written.sum()) == len(case.kv_lens)
    assert not torch.equal(fi[3][written], kc[written]), "the decoy in the slot to be written must differ from the new key"
    for kind in A.POISONS:
        pk, pv = A.poisoned(p, kind, drop_last=True, kc=fi[3], vc=fi[4])
        assert not torch.isfinite(pk[written].float()).any()
        o2, _, kc2, vc2 = A.fused_oracle(p, fi, kc=pk, vc=pv)
        assert torch.equal(o2, out)
        assert torch.equal(kc2[written].view(torch.int16), kc[written].view(torch.int16))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_probe_is_sensitive(case):
    """Every mutation that applies to the case must be refused by check(); no case may be without one."""
    p = A.probe(case)
    caught = []
    for name, mutate in A.MUTATIONS:
        out = mutate(p)
        if out is None:
            continue
        with pytest.raises(AssertionError):
            A.check(p, out, what=f"{case.name} [{name}]")
        caught.append(name)
    assert caught, f"{case.name}: no mutation applies"
