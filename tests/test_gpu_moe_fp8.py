"""GPU: the FP8 block-scaled expert GEMMs of hydrainfer_amd/csrc/moe_experts_fp8.hip, SparseMoE and DeepseekMoeForCausalLM
on quantised experts (inputs and expected values: tests/moe_fp8_ref.py, proven on the CPU by tests/test_moe_fp8_cpu.py).

1. exact pairing: tests/test_gpu_moe_experts.py's construction (one-hot tokens, gate 32, grid up / down weights, NaN in
   the unrouted experts, NaN-poisoned outputs with guard tails) with the weights stored as e4m3 bytes and a seeded
   power-of-two scale per (expert, 128 x 128 block); unrouted experts hold 0x7F bytes and NaN scales.  torch.equal to
   the float64 restatement over the dequantised weights: pins expert <-> weight <-> scale-block pairing in every
   instantiation (moe_gemm_fp8w_kernel<T, MB, GU>, MB = 1 / 2 / 4 as listed there), chunk border and partial chunk.
2. fine scales: one product 3 q s per output, scales with 13 significant bits — torch.equal to the float64 value rounded
   at the contract's rounding points; a kernel that rounded q s to T first would differ (asserted on the CPU).
3. the block on quantize_experts() against the float64 block over the dequantised weights, at the 16-bit block's bound
   and tolerance (only the arithmetic is judged, not the quantisation).
4. the tiny model, the engine (eager = graphed tokens) and OfflineInferenceEngine on quantised experts.
5. the Python shim's refusals."""
import pytest
import torch

from tests import moe_block_ref as R
from tests import moe_fp8_ref as F8
from tests import test_gpu_moe_model as MM
from tests.golden import cases as C
from tests.test_gpu_moe_experts import _checked, _poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP8 = torch.float8_e4m3fn


@pytest.mark.parametrize("case", R.PAIRING_CASES, ids=[c.name for c in R.PAIRING_CASES])
@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_exact_pairing_fp8(case, dt):
    from hydrainfer_amd._C.kernel.moe import experts as K
    T = R.DTYPES[dt]
    f = F8.fp8_pairing(case)
    p = f.p
    n, topk, n_e, h, inter = case.n, case.topk, case.E, case.h, case.I
    x, ids, w, shared = p.x.to(T).to(DEV), p.ids.to(DEV), p.w.to(DEV), p.shared.to(T).to(DEV)
    qgu, qdown = f.qgu.to(DEV).view(FP8), f.qdown.to(DEV)            # float8 and uint8 holders are both accepted
    sgu, sdown = f.sgu.to(DEV), f.sdown.to(DEV)
    seg = K.segments(ids, n_e)

    act_buf, act = _poisoned(n * topk, inter, T)
    K.gate_up_silu(x, qgu, seg, topk, out=act, w_gate_up_scale=sgu)
    _checked(act_buf, act, "act")
    assert torch.equal(act.cpu(), F8.pairing_act(f, T)), "act: a slot met another token, expert or scale block"

    y_buf, y = _poisoned(n * topk, h, T)
    K.down(act, qdown, seg, topk, out=y, w_down_scale=sdown)
    _checked(y_buf, y, "y")
    assert torch.equal(y.cpu(), F8.pairing_y(f, T)), "y: down paired a slot with another expert or scale block"

    for with_shared in (True, False):
        out_buf, out = _poisoned(n, h, T)
        K.combine(y, w, shared if with_shared else None, out=out)
        _checked(out_buf, out, "out")
        assert torch.equal(out.cpu(), F8.pairing_out(f, T, shared=with_shared)), f"combine (shared={with_shared})"
    one_call = K.experts_forward(x, qgu, qdown.view(FP8), w, ids, shared, w_gate_up_scale=sgu, w_down_scale=sdown)
    assert torch.equal(one_call.cpu(), F8.pairing_out(f, T))


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_fine_scales_one_product_per_output(dt):
    from hydrainfer_amd._C.kernel.moe import experts as K
    T = R.DTYPES[dt]
    c = F8.fine_case()
    n, topk, n_e, h, inter = F8.FINE_N, F8.FINE_TOPK, F8.FINE_E, F8.FINE_H, F8.FINE_I
    seg = K.segments(c.ids.to(DEV), n_e)
    act_buf, act = _poisoned(n * topk, inter, T)
    K.gate_up_silu(c.x.to(T).to(DEV), c.qgu.to(DEV), seg, topk, out=act, w_gate_up_scale=c.sgu.to(DEV))
    _checked(act_buf, act, "act")
    want = F8.fine_act(c, T)
    diff = int((act.cpu() != want).sum())
    assert diff == 0, f"act: {diff} of {want.numel()} elements differ from T(96 T(3 q s)) (the scaled weight was rounded?)"
    # the down launch on its own: one-hot act rows of value 3
    y_buf, y = _poisoned(n * topk, h, T)
    K.down(c.act_in.to(T).to(DEV), c.qdown.to(DEV), seg, topk, out=y, w_down_scale=c.sdown.to(DEV))
    _checked(y_buf, y, "y")
    want = F8.fine_y(c, T)
    diff = int((y.cpu() != want).sum())
    assert diff == 0, f"y: {diff} of {want.numel()} elements differ from T(3 q s)"


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_a_nan_byte_is_a_nan_weight(dt):
    """0x7F in one up row and 0xFF in one down row of a routed expert: that output of every slot of the expert is NaN
    (0 * NaN is NaN, so the one-hot rows do not hide it), and nothing else is."""
    from hydrainfer_amd._C.kernel.moe import experts as K
    T = R.DTYPES[dt]
    c = F8.fine_case()
    n, topk, n_e, h, inter = F8.FINE_N, F8.FINE_TOPK, F8.FINE_E, F8.FINE_H, F8.FINE_I
    e0, j0, c0 = int(c.ids[0, 0]), 77, 300
    qgu, qdown = c.qgu.clone(), c.qdown.clone()
    qgu[e0, inter + j0, F8.FINE_KS[0]] = 0x7F            # the k token 0 is one-hot at
    qdown[e0, c0, int(c.js[0])] = 0xFF                   # the j slot 0's act row is one-hot at
    seg = K.segments(c.ids.to(DEV), n_e)
    act = K.gate_up_silu(c.x.to(T).to(DEV), qgu.to(DEV), seg, topk, w_gate_up_scale=c.sgu.to(DEV)).cpu()
    y = K.down(c.act_in.to(T).to(DEV), qdown.to(DEV), seg, topk, w_down_scale=c.sdown.to(DEV)).cpu()
    want_act, want_y = F8.fine_act(c, T), F8.fine_y(c, T)
    of_e0 = c.ids.reshape(-1) == e0
    assert 0 < int(of_e0.sum()) < n * topk
    nan_act = torch.zeros_like(want_act, dtype=torch.bool)
    nan_act[of_e0, j0] = True
    nan_y = torch.zeros_like(want_y, dtype=torch.bool)
    nan_y[of_e0, c0] = True
    assert torch.equal(torch.isnan(act), nan_act) and torch.equal(act[~nan_act], want_act[~nan_act])
    assert torch.equal(torch.isnan(y), nan_y) and torch.equal(y[~nan_y], want_y[~nan_y])


BLOCK_CASES = [(dt, norm, n) for dt in R.DTYPES for norm in (False, True) for n in R.N_VALUES]


@pytest.mark.parametrize("dt,norm,n", BLOCK_CASES, ids=[R.fixture_key(*c) for c in BLOCK_CASES])
def test_quantised_block_against_the_fixture_inputs(dt, norm, n):
    from hydrainfer_amd._C.kernel.moe import experts as K
    from hydrainfer_amd.layer.moe import SparseMoE
    c = R.block_case(dt, norm, n)
    sd = R.block_weights(dt)
    moe = SparseMoE.from_reference_state_dict("", sd, R.TOPK, norm, R.SCALE, device=DEV).quantize_experts()
    assert moe.experts_fp8 and moe.w_gate_up.dtype == FP8 and moe.router_weight.dtype == R.DTYPES[dt]
    out = moe.forward(c.x.to(DEV)).cpu()
    ids = moe.last_topk_ids.cpu()
    assert torch.equal(ids.sort(dim=1).values, c.ref_ids.sort(dim=1).values), "other experts than the reference's"
    wr, _, _, sgu, sdown = R.stacked(sd)
    wgu = K.dequantize_fp8_block(moe.w_gate_up.cpu(), moe.w_gate_up_scale.cpu())
    wdown = K.dequantize_fp8_block(moe.w_down.cpu(), moe.w_down_scale.cpu())
    y64, _, _ = R.block(c.x, wr, wgu, wdown, sgu, sdown, R.TOPK, norm, R.SCALE, "f64", ids=ids)
    ratio = R.error_ratio(out, y64, R.TOL[dt])
    print(f"fp8 {R.fixture_key(dt, norm, n)}: ratio to float64 over the dequantised weights {ratio:.3f}; bound 2")
    assert ratio <= 2.0


def _quantised_model(dname):
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    dt = C.DTYPES[dname]
    return DeepseekMoeForCausalLM.from_reference_state_dict(MM.moe_shape(), MM.reference_sd(dname), dt,
                                                            torch.device(DEV)).quantize_experts()


def _cpu_logits(dname, sd):
    """MM._cpu_pass on a given state dict: the CPU model's logits per step, following its own greedy tokens."""
    from oracle.model import OracleAttnMeta
    dt, shape = C.DTYPES[dname], MM.moe_shape()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    model = R.oracle_moe_model(shape, sd, dt)
    pool = MM._pool(dt, shape.num_hidden_layers)
    logits, toks = [], []
    gen = MM._steps()
    m = next(gen)
    for s in range(1 + C.TINY_DECODE_STEPS):
        meta = OracleAttnMeta(i32(m["cu_q"]), i32(m["cu_k"]), i32(m["slots"]), i32(m["bt"]), i32(m["cu_b"]))
        lg = model.forward_logits(i32(m["ids"]), i32(m["pos"]), meta, [(pool[l, 0], pool[l, 1]) for l in range(pool.shape[0])],
                                  torch.tensor(m["sel"]) if m["prefill"] else None).float()
        logits.append(lg)
        toks.append(lg.argmax(-1).tolist())
        if s < C.TINY_DECODE_STEPS:
            m = gen.send(toks[-1])
    return torch.stack(logits), toks


@pytest.mark.parametrize("dname", list(MM.LOGIT_TOL))
def test_quantised_model_matches_the_cpu_composition(dname):
    from hydrainfer_amd.layer.causal_attention import AttentionParametersBuilder
    from hydrainfer_amd.memory.kv_cache import KVCache
    from hydrainfer_amd.model.llama import LanguageModelParameters
    dt, dev, shape = C.DTYPES[dname], torch.device(DEV), MM.moe_shape()
    model = _quantised_model(dname)
    assert model.state["l1.moe.wgu"].dtype == FP8 and model.moe[1].experts_fp8
    want_all, toks = _cpu_logits(dname, F8.dequantised_sd(model.to_reference_state_dict(), dt))
    pool = MM._pool(dt, shape.num_hidden_layers).to(dev)
    tol = MM.LOGIT_TOL[dname]
    gen = MM._steps()
    m = next(gen)
    worst = 0.0
    for s in range(1 + C.TINY_DECODE_STEPS):
        b = AttentionParametersBuilder(shape.num_attention_heads, shape.num_key_value_heads, shape.head_dim, MM.BS, dev)
        for ql, kl, sl, tb in m["per"]:
            b.add_request(ql, kl, sl, tb)
        for l in range(shape.num_hidden_layers):
            b.add_kv_cache(KVCache(pool[l, 0], pool[l, 1]))
        params = LanguageModelParameters(attention_params=b.build_attention_parameters(), all_sequences_decode=not m["prefill"],
                                         selected_token_ids=torch.tensor(m["sel"], device=dev) if m["prefill"] else None)
        got = model.forward_logits(torch.tensor(m["ids"], dtype=torch.int64, device=dev),
                                   torch.tensor(m["pos"], dtype=torch.int32, device=dev), params).float().cpu()
        err = float((got - want_all[s]).abs().max())
        worst = max(worst, err)
        assert err <= tol, f"step {s}: logits max abs err {err} > {tol}"
        if s < C.TINY_DECODE_STEPS:
            m = gen.send(toks[s])                 # both sides follow the CPU's tokens
    print(f"fp8 {dname}: worst logit error {worst:.4f} (tolerance {tol})")


def _quantised_cluster(dname, graph_decode):
    cluster, n_img_tok = MM._engine_cluster(dname, graph_decode)
    lm = cluster.nodes[0].executor.fill_executor.language_model.language_model
    lm.quantize_experts()                          # before the first step: nothing has been captured yet
    assert lm.moe[1].experts_fp8
    return cluster, n_img_tok


def test_engine_eager_and_graphed_decode_give_the_same_tokens_fp8():
    from hydrainfer_amd.engine import InstructionCreator
    from tests.engine_util import run_trace
    outs, decoder = [], None
    for graph_decode in (False, True):
        cluster, n_img_tok = _quantised_cluster("bf16", graph_decode)
        creator = InstructionCreator(image_token_id=C.TINY_IMAGE_TOKEN_ID, n_image_tokens_per_image=n_img_tok, block_size=MM.BS,
                                     ignore_eos=True)
        rcbs = run_trace(cluster, creator, MM._trace())
        torch.cuda.synchronize()
        outs.append([r.output_token_ids for r in rcbs])
        if graph_decode:
            decoder = cluster.nodes[0].executor.fill_executor.graph_decoder
    assert all(len(t) == want for t, want in zip(outs[0], (9, 7, 8)))
    assert outs[0] == outs[1]
    assert decoder is not None and len(decoder.graphs) > 0 and decoder.launches > 0, "no decode step was replayed from a capture"


def test_offline_engine_serves_the_quantised_model():
    from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
    from hydrainfer_amd.engine.offline import OfflineInferenceEngine, OfflineRequest
    from tests.engine_util import run_trace
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (7 + 9 * i,), generator=g).tolist() for i in range(3)]
    cluster, n_img_tok = _quantised_cluster("fp16", False)
    creator = InstructionCreator(image_token_id=C.TINY_IMAGE_TOKEN_ID, n_image_tokens_per_image=n_img_tok, block_size=MM.BS, ignore_eos=True)
    eager = run_trace(cluster, creator, [(0, TokenRequest(request_id=i, token_ids=p, pixel_values=None, image_size=(0, 0), image_hash=0,
                                                           sampling_params=SamplingParameters(max_tokens=6))) for i, p in enumerate(prompts)])
    node = cluster.nodes[0].executor
    eng = OfflineInferenceEngine(node.fill_executor.language_model, node.image_embed_executor.vision_model, torch.float16, DEV,
                                 max_running_requests=4, token_budgets=64, max_context=256, warm_up=False)
    got = eng.generate([OfflineRequest(p, None, max_tokens=6) for p in prompts])
    assert [r.output_token_ids for r in got] == [r.output_token_ids for r in eager]
    assert all(len(r.output_token_ids) == 6 for r in got)


def test_python_shim_refuses_what_does_not_fit():
    from hydrainfer_amd import _lib
    from hydrainfer_amd._C.kernel.moe import experts as K
    T = torch.bfloat16
    x = torch.zeros((2, 256), dtype=T, device=DEV)
    ids = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    seg = K.segments(ids, 4)
    q = torch.zeros((4, 256, 256), dtype=torch.uint8, device=DEV)
    s = torch.ones((4, 2, 2), dtype=torch.float32, device=DEV)
    K.gate_up_silu(x, q, seg, 2, w_gate_up_scale=s)                                        # the form that is accepted
    for bad in (s[:, :1].contiguous(), torch.ones((4, 2, 3), device=DEV), s.double(), s.to(T), s.cpu(),
                torch.ones((4, 2, 4), device=DEV)[:, :, ::2]):
        with pytest.raises(_lib.HydraHipError):
            K.gate_up_silu(x, q, seg, 2, w_gate_up_scale=bad)
    with pytest.raises(_lib.HydraHipError):
        K.gate_up_silu(x, torch.zeros((4, 256, 256), dtype=T, device=DEV), seg, 2, w_gate_up_scale=s)   # bf16 weights with a scale
    with pytest.raises(_lib.HydraHipError):
        K.gate_up_silu(x, q.view(FP8), seg, 2)                                                          # fp8 weights without one
    act = torch.zeros((4, 128), dtype=T, device=DEV)
    qd = torch.zeros((4, 256, 128), dtype=torch.uint8, device=DEV)
    sd = torch.ones((4, 2, 1), dtype=torch.float32, device=DEV)
    K.down(act, qd.view(FP8), seg, 2, w_down_scale=sd)
    for bad in (torch.ones((4, 1, 2), device=DEV), sd.half(), sd.cpu()):
        with pytest.raises(_lib.HydraHipError):
            K.down(act, qd, seg, 2, w_down_scale=bad)
    with pytest.raises(_lib.HydraHipError):
        K.down(act, torch.zeros((4, 256, 128), dtype=T, device=DEV), seg, 2, w_down_scale=sd)
    with pytest.raises(_lib.HydraHipError):
        K.down(act, qd, seg, 2)
    with pytest.raises(_lib.HydraHipError):
        K.experts_forward(x, q, qd, torch.ones((2, 2), device=DEV), ids, w_gate_up_scale=s)              # down's scale is missing
