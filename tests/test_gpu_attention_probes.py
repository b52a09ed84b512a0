"""GPU: the attention kernels on inputs whose answer is known exactly (tests/attn_probe.py; each case is proven sound
and sensitive on the oracle by tests/test_attn_probe_cpu.py).

Part A — one-hot probes: the output must be V[target] bit for bit (torch.equal, no tolerance) on every kernel path.
Part B — trap keys just past the end of a sequence, in physical block 0 and in an unreferenced page (ATTN_TOL against the
oracle; a leak lands near 64), and every case again on a pool whose unaddressed slots are NaN, then +inf in K and the
largest finite value in V: finite, bit-identical to the clean-pool run of the same kernel, and still right.  One engine
run on a NaN pool against one on a zero pool.

Every test prints how many probe launches it checked."""
import math

import pytest
import torch

from tests import attn_probe as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_DEFAULTS = {"decode_gqa": 1, "fwd_mfma32": 1, "fwd_persistent": 1, "fwd_units": -1, "fwd_seq_group": 0,
             "fwd_row_blocks": 0, "fwd_key_units": 0, "decode_hpw4": 0}


class _options:
    """hx_debug_set_option for the block, defaults restored on the way out."""

    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        from hydrainfer_amd import _lib
        for k, v in self.opts.items():
            _lib.check(_lib.lib().hx_debug_set_option(k.encode(), v), f"option {k}")

    def __exit__(self, *exc):
        from hydrainfer_amd import _lib
        for k in self.opts:
            _lib.lib().hx_debug_set_option(k.encode(), _DEFAULTS[k])


def _launch(p, kc, vc, num_splits=0):
    """mha_varlen_fwd on the probe with the given pool (device tensors); `out` starts as NaN so an unwritten row shows."""
    from hydrainfer_amd._C.kernel.flash_attn import mha_varlen_fwd
    c = p.case
    d = lambda t: None if t is None else t.to(DEV)
    qd = p.q.to(DEV)
    out = torch.full_like(qd, float("nan"))
    if c.window is not None:
        wl, wr = c.window
    else:
        wl, wr = (-1, 0) if c.causal else (-1, -1)
    mha_varlen_fwd(out, qd, kc, vc, d(p.cu_q), d(p.cu_k), d(p.bt), d(p.cu_b), d(p.slopes), p.max_q, p.max_k,
                   1.0 / math.sqrt(c.D), c.softcap, wl, wr, num_splits)
    torch.cuda.synchronize()
    return out


def _clean_and_poisoned(p, what, num_splits=0):
    """The probe on the clean pool, then on the two poisoned pools: each checked, the poisoned ones bit-identical to the
    clean one.  Returns the number of launches checked."""
    clean = _launch(p, p.kc.to(DEV), p.vc.to(DEV), num_splits)
    A.check(p, clean, what=f"{what}, clean pool")
    if p.case.bs == 0:
        return 1
    for kind in A.POISONS:
        kc, vc = A.poisoned(p, kind)
        out = _launch(p, kc.to(DEV), vc.to(DEV), num_splits)
        A.check(p, out, what=f"{what}, pool poisoned with {kind}")
        assert torch.equal(out.view(torch.int16), clean.view(torch.int16)), f"{what}: {kind} in unaddressed slots changes the bits"
    return 3


def _sweep(cases, what, splits=(0,)):
    n = 0
    for case in cases:
        p = A.probe(case)
        for s in splits:
            n += _clean_and_poisoned(p, f"{what}: {case.name} splits={s}", s)
    return n


def test_per_head_decode():
    """attn_decode.hip, decode_gqa = 0: 4-wave and (32 x 32 heads x 8 sequences) 8-wave forms, every split setting."""
    from hydrainfer_amd import _lib
    with _options(decode_gqa=0):
        n = _sweep(A.PER_HEAD_DECODE, "per-head decode", A.SPLITS)
        n += _sweep(A.RANDOM_DECODE, "per-head decode", (0, 3))
        if _lib.has_experiments():
            with _options(decode_hpw4=1):
                n += _sweep([c for c in A.PER_HEAD_DECODE if c.H == c.HK], "four-heads decode", (1,))
    print(f"probe launches checked, per-head decode: {n}")


def test_gqa_decode():
    """attn_decode_gqa.hip: head pairs (8, 4), (28, 4), (16, 1), every split setting."""
    n = _sweep(A.GQA_DECODE, "gqa decode", A.SPLITS) + _sweep(A.RANDOM_DECODE, "gqa decode", (0, 3))
    print(f"probe launches checked, grouped-query decode: {n}")


def test_alibi_decode_and_prefill():
    n = _sweep(A.ALIBI_DECODE, "alibi gqa/auto decode", (0, 1, 4))
    with _options(decode_gqa=0):
        n += _sweep(A.ALIBI_DECODE, "alibi per-head decode", (0, 1, 4))
    n += _sweep(A.ALIBI_PREFILL, "alibi general kernel")
    print(f"probe launches checked, ALiBi: {n}")


def _fused(p, fi, kc, vc, form, splits):
    from hydrainfer_amd._C.kernel.flash_attn import decode_attention_fused, decode_rank
    c = p.case
    q, k_new, v_new, _, _, pos, cs, slots = fi
    d = lambda t: t.to(DEV)
    B = len(c.kv_lens)
    out = torch.full((B, c.H, c.D), float("nan"), dtype=q.dtype, device=DEV)
    kcd, vcd = d(kc).clone(), d(vc).clone()
    kw = {}
    qd, kd, vd = d(q), d(k_new), d(v_new)
    if form == "rank_desc":
        kw["rank_desc"] = decode_rank(d(p.cu_k))
    elif form == "slabs":          # two fp32 slabs of half the value each: their sum is exact
        row = torch.cat([q.reshape(B, -1), k_new.reshape(B, -1), v_new.reshape(B, -1)], dim=1).float() / 2
        kw["qkv_partial"], kw["qkv_splits"] = d(torch.stack([row, row]).contiguous()), 2
        qd, kd, vd = torch.zeros_like(qd), torch.zeros_like(kd), torch.zeros_like(vd)      # shape carriers only
    decode_attention_fused(out, qd, kd, vd, kcd, vcd, d(pos), d(cs), d(slots), d(p.cu_q), d(p.cu_k), d(p.bt), d(p.cu_b),
                           p.max_k, 1.0 / math.sqrt(c.D), splits, **kw)
    torch.cuda.synchronize()
    return out, kcd.cpu(), vcd.cpu()


def test_fused_decode():
    """decode_attention_fused plain, with a rank descriptor and from qkv slabs; the target is the new token in one pass
    and a cached key in the other.  On the poisoned pools the slot to be written is poisoned too; afterwards the caches
    equal the input caches bit for bit except the one written slot per sequence, which holds the oracle's
    apply_rotary_pos_emb + set_kv_cache result."""
    n = 0
    i16 = lambda t: t.view(torch.int16)
    for case in A.FUSED_DECODE:
        p = A.probe(case)
        fi = A.fused_inputs(p)
        _, _, kc_ref, vc_ref = A.fused_oracle(p, fi)
        written = ~A.addressed_mask(p, drop_last=True) & A.addressed_mask(p)
        for form in ("plain", "rank_desc", "slabs"):
            for splits in (0, 1, 3):
                what = f"fused {form}: {case.name} splits={splits}"
                clean = None
                for kind in ("clean",) + A.POISONS:
                    kc, vc = (fi[3], fi[4]) if kind == "clean" else A.poisoned(p, kind, drop_last=True, kc=fi[3], vc=fi[4])
                    out, kca, vca = _fused(p, fi, kc, vc, form, splits)
                    A.check(p, out, what=f"{what}, {kind} pool")
                    assert torch.equal(i16(kca)[~written], i16(kc)[~written]) and torch.equal(i16(vca)[~written], i16(vc)[~written]), \
                        f"{what}, {kind} pool: a slot other than the new token's changed"
                    assert torch.equal(i16(kca)[written], i16(kc_ref)[written]) and torch.equal(i16(vca)[written], i16(vc_ref)[written]), \
                        f"{what}, {kind} pool: the written slot differs from the oracle's RoPE + set_kv_cache"
                    if clean is None:
                        clean = out
                    assert torch.equal(i16(out), i16(clean)), f"{what}: {kind} in unaddressed slots changes the bits"
                    n += 1
    print(f"probe launches checked, fused decode: {n}")


@pytest.mark.parametrize("keys", [1, 2])
@pytest.mark.parametrize("rows", [1, 2])
def test_prefill_16x16x32(rows, keys):
    with _options(fwd_mfma32=0, fwd_row_blocks=rows, fwd_key_units=keys):
        n = _sweep(A.PREFILL + A.PREFILL_D256 + list(A.RANDOM_PREFILL), f"16x16x32 rows={rows} keys={keys}")
    print(f"probe launches checked, 16x16x32 prefill rows={rows} keys={keys}: {n}")


@pytest.mark.parametrize("mode", ["item", "tiles", "units", "g4", "auto"])
def test_prefill_32x32x16(mode):
    opts = {"item": dict(fwd_persistent=0), "tiles": dict(fwd_persistent=2, fwd_units=0),
            "units": dict(fwd_persistent=2, fwd_units=1, fwd_seq_group=1), "g4": dict(fwd_persistent=2, fwd_seq_group=4),
            "auto": {}}[mode]
    with _options(**opts):
        n = _sweep(A.PREFILL + list(A.RANDOM_PREFILL), f"32x32x16 {mode}")
    print(f"probe launches checked, 32x32x16 prefill {mode}: {n}")


def test_general_kernel_head_dims_32_and_96():
    n = _sweep(A.GENERAL + A.PREFILL_D256 + list(A.RANDOM_GENERAL), "general kernel")
    print(f"probe launches checked, general kernel (D = 32, 96, 256; soft-cap; random window): {n}")


def test_dense_layout():
    n = _sweep(A.DENSE, "dense")
    with _options(fwd_persistent=2):
        n += _sweep(A.DENSE, "dense, persistent")
    with _options(fwd_mfma32=0):
        n += _sweep(A.DENSE, "dense, 16x16x32")
    print(f"probe launches checked, dense layout: {n}")


def test_windows():
    n = _sweep(A.WINDOW, "window")
    print(f"probe launches checked, windows: {n}")


# ---------------------------------------------------------------------------------------------------------------------
# B3: the stale pool as the product meets it
# ---------------------------------------------------------------------------------------------------------------------
def _fill_pools(cluster, value):
    for node in cluster.nodes:
        t = node.kv_cache_block_manager.cache_tensor
        flat = torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())     # the plane skew included
        flat.fill_(value)
    torch.cuda.synchronize()


@pytest.mark.parametrize("graph_decode", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dname", ["fp16", "bf16"])
def test_engine_on_a_nan_pool_generates_the_tokens_of_a_zero_pool(dname, graph_decode):
    from tests import test_engine_e2e as E
    from tests.engine_util import run_trace
    from tests.golden import cases as C
    dt = C.DTYPES[dname]
    tokens = []
    for value in (float("nan"), 0.0):
        reqs = E.trace_requests()
        cluster, _, _ = E.hip_cluster(dt, dname, ["EPD"], True, graph_decode=graph_decode)
        _fill_pools(cluster, value)
        rcbs = run_trace(cluster, E.creator(), reqs)
        torch.cuda.synchronize()
        tokens.append([list(r.output_token_ids) for r in rcbs])
    assert all(len(t) > 0 for t in tokens[0])
    for i, (a, b) in enumerate(zip(*tokens)):
        assert a == b, f"request {i}: NaN pool {a}, zero pool {b}"
