"""GPU: the kernels of hydrainfer_amd/csrc/moe_experts.hip fed with topk_ids / topk_weights directly, the fused router, and
SparseMoE.forward against the reference fixture (inputs and expected values: tests/moe_block_ref.py, proven on the CPU by
tests/test_moe_block_cpu.py).

1. exact pairing: one-hot tokens, gate weights 32, grid-valued up / down weights per expert, power-of-two routing weights,
   NaN weights in the unrouted experts, NaN-poisoned outputs with a guard tail — torch.equal to the float64 restatement.
   Which kernel instantiation a case launches (MB = 16-row blocks of a tile = ceil(min(n, 64) / 16) -> 1, 2 or 4):
     every-expert-one-row    moe_gemm_kernel<T, 1, 1> / <T, 1, 0>   one row per expert, one K chunk
     odd-multiples-e72       <T, 1, *>   h = 1280: three 512-k chunks, the last one half full; I = 896: one 1024-k down
                             chunk whose second stream is three quarters full; 72 experts, most of them empty
     two-row-blocks          <T, 2, *>   two 1024-k down chunks, the last one an eighth full
     full-tile-one-expert    <T, 4, *>   64 rows of one expert, seven empty experts
     minimum-sizes           <T, 4, *>   33 tokens, h = I = 128
     two-experts-70-rows     <T, 4, *>   70 rows per expert: a second tile of 6 rows; two K chunks in both GEMMs
2. router: exact logits with deliberate ties, E in {8, 64, 72}, with and without norm_topk_prob; refusals.
3. the block: |out - y64| <= 2 tol (1 + |y64|), the same bound against the reference's stored output, the reference's
   experts as sets."""
import pytest
import torch

from tests import gemm_exact as G
from tests import moe_block_ref as R
from tests import moe_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _poisoned(rows: int, cols: int, T):
    """[rows, cols] view of a NaN-filled T buffer followed by G.GUARD sentinels."""
    buf = torch.empty(rows * cols + G.GUARD, dtype=T, device=DEV)
    buf[:rows * cols] = float("nan")
    buf[rows * cols:] = G.SENTINEL
    return buf, buf[:rows * cols].view(rows, cols)


def _checked(buf, view, what):
    used = view.numel()
    n_nan = int(torch.isnan(buf[:used]).sum())
    assert n_nan == 0, f"{what}: {n_nan} of {used} elements are NaN (never written, or computed from an unrouted expert)"
    assert bool((buf[used:] == G.SENTINEL).all()), f"{what}: the guard behind the output was written"
    return view


@pytest.mark.parametrize("case", R.PAIRING_CASES, ids=[c.name for c in R.PAIRING_CASES])
@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_exact_pairing(case, dt):
    from hydrainfer_amd._C.kernel.moe import experts as K
    T = R.DTYPES[dt]
    p = R.build_pairing(case)
    n, topk, n_e, h, inter = case.n, case.topk, case.E, case.h, case.I
    x, wgu, wdown = p.x.to(T).to(DEV), p.wgu.to(T).to(DEV), p.wdown.to(T).to(DEV)
    ids, w, shared = p.ids.to(DEV), p.w.to(DEV), p.shared.to(T).to(DEV)

    # segments: offsets / counts of the bincount, and the slot list a grouping of 0 .. n * topk - 1 by expert
    seg_buf = torch.full((2 * n_e + 1 + n * topk + 64,), -7, dtype=torch.int32, device=DEV)
    seg = K.segments(ids, n_e, out=seg_buf).cpu()
    counts = torch.bincount(p.ids.reshape(-1).long(), minlength=n_e)
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])
    assert seg[:n_e + 1].tolist() == offsets.tolist() and seg[n_e + 1:2 * n_e + 1].tolist() == counts.tolist()
    assert bool((seg[2 * n_e + 1 + n * topk:] == -7).all()), "segments wrote behind its output"
    slots = seg[2 * n_e + 1:2 * n_e + 1 + n * topk]
    flat = p.ids.reshape(-1)
    for e in range(n_e):
        group = slots[offsets[e]:offsets[e + 1]].long()
        assert sorted(group.tolist()) == (flat == e).nonzero()[:, 0].tolist(), f"expert {e}: wrong slots"

    # gate|up + silu * mul: act[s, j] = 32 * Wu_e[j, k_t], exactly
    act_buf, act = _poisoned(n * topk, inter, T)
    K.gate_up_silu(x, wgu, seg_buf, topk, out=act)
    _checked(act_buf, act, "act")
    ks = p.x.argmax(dim=1)
    want_act = torch.stack([R.GATE_VALUE * p.wgu[int(flat[s]), inter:, int(ks[s // topk])] for s in range(n * topk)]).to(T)
    assert torch.equal(act.cpu(), want_act), "act: a slot was paired with another token or another expert's weights"

    y_buf, y = _poisoned(n * topk, h, T)
    K.down(act, wdown, seg_buf, topk, out=y)
    _checked(y_buf, y, "y")
    want_y = R.expert_rows(p.x.to(T), p.ids, p.wgu.to(T), p.wdown.to(T), "exact")
    assert torch.equal(y.cpu(), want_y), "y: down paired a slot with another expert"

    for with_shared in (True, False):
        out_buf, out = _poisoned(n, h, T)
        K.combine(y, w, shared if with_shared else None, out=out)
        _checked(out_buf, out, "out")
        assert torch.equal(out.cpu(), R.pairing_expected(p, T, shared=with_shared)), f"combine (shared={with_shared})"
    # the one-call form, fresh buffers
    assert torch.equal(K.experts_forward(x, wgu, wdown, w, ids, shared).cpu(), R.pairing_expected(p, T))


ROUTER_CASES = [M.TopkCase(6, E, k, ties) for E in (8, 64, 72) for k in sorted({1, 3, min(8, E)}) for ties in (0, 2)]


@pytest.mark.parametrize("case", ROUTER_CASES, ids=[c.name for c in ROUTER_CASES])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "bf16-f32router"])
def test_router_exact_logits_and_ties(case, dt):
    """x[t] is one-hot at column t and router_weight[e, t] = logits[t, e] of moe_cases.build_topk (distinct multiples of
    0.25 with deliberate ties at lanes l, l + 64 and across lanes; exact in both types): the fp32 logits are exact, the
    indices the stable descending argsort, the weights the float64 formula at WEIGHT_RTOL."""
    from hydrainfer_amd._C.kernel.moe import experts as K
    T = R.DTYPES[dt.split("-")[0]]
    b = M.build_topk(case)
    n, n_e, topk, h = case.n_tokens, case.n_experts, case.topk, 128
    wr = G.grid_values((n_e, h), 3 + n_e)
    wr[:, :n] = b.logits.t()
    assert torch.equal(wr.to(T).float(), wr)
    x = G.one_hot_rows(list(range(n)), h).to(T).to(DEV)
    wr_dev = (wr if dt.endswith("f32router") else wr.to(T)).to(DEV)
    for norm, scale in ((False, 1.0), (True, 1.0), (True, 2.5), (False, 0.5)):
        w, ids = K.gate_topk(x, wr_dev, topk, norm, scale)
        assert torch.equal(ids.cpu(), b.indices), f"{case.name} norm={norm}: indices differ from the stable argsort"
        want = b.weights / (b.weights.sum(dim=1, keepdim=True) + 1e-20) * scale if (norm and topk > 1) else b.weights * scale
        torch.testing.assert_close(w.cpu().double(), want, rtol=M.WEIGHT_RTOL, atol=0)


def test_router_and_experts_refuse_what_they_do_not_do():
    from hydrainfer_amd import _lib
    from hydrainfer_amd._C.kernel.moe import experts as K
    x = torch.zeros((2, 128), dtype=torch.bfloat16, device=DEV)
    wr = torch.zeros((8, 128), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.HydraHipError, match="not supported|unsupported"):
        K.gate_topk(x, wr, 2, False, scoring_func="sigmoid")
    with pytest.raises(_lib.HydraHipError, match="not supported|unsupported"):
        K.gate_topk(x, wr, 2, False, n_group=4, topk_group=2)
    with pytest.raises(_lib.HydraHipError):
        K.gate_topk(x, wr, 9, False)                                   # topk > 8
    with pytest.raises(_lib.HydraHipError):
        K.gate_topk(x, wr.half(), 2, False)                            # router in another two-byte type than x
    ids = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    seg = K.segments(ids, 8)
    bad = torch.zeros((8, 2 * 96, 128), dtype=torch.bfloat16, device=DEV)      # I = 96: not a multiple of 128
    with pytest.raises(_lib.HydraHipError):
        K.gate_up_silu(x, bad, seg, 2)
    with pytest.raises(_lib.HydraHipError):
        K.segments(ids, 257)                                           # more than 256 experts


BLOCK_CASES = [(dt, norm, n) for dt in R.DTYPES for norm in (False, True) for n in R.N_VALUES]


@pytest.mark.parametrize("dt,norm,n", BLOCK_CASES, ids=[R.fixture_key(*c) for c in BLOCK_CASES])
def test_block_against_the_fixture(dt, norm, n):
    from hydrainfer_amd.layer.moe import SparseMoE
    c = R.block_case(dt, norm, n)
    sd = R.block_weights(dt)
    moe = SparseMoE.from_reference_state_dict("", sd, R.TOPK, norm, R.SCALE, device=DEV)
    out = moe.forward(c.x.to(DEV)).cpu()
    ids = moe.last_topk_ids.cpu()
    assert torch.equal(ids.sort(dim=1).values, c.ref_ids.sort(dim=1).values), "other experts than the reference's"
    wr, wgu, wdown, sgu, sdown = R.stacked(sd)
    y64, _, _ = R.block(c.x, wr, wgu, wdown, sgu, sdown, R.TOPK, norm, R.SCALE, "f64", ids=ids)
    tol = R.TOL[dt]
    ratio, ratio_ref = R.error_ratio(out, y64, tol), R.error_ratio(out, c.ref_out.double(), tol)
    print(f"{R.fixture_key(dt, norm, n)}: ratio to float64 {ratio:.3f} (the reference's own {c.ref_ratio:.3f}), "
          f"to the reference's output {ratio_ref:.3f}; bound 2")
    assert ratio <= 2.0 and ratio_ref <= 2.0
