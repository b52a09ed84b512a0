"""GPU: the MXFP4 expert GEMMs of hydrainfer_amd/csrc/moe_experts_mxfp4.hip, SparseMoE and DeepseekMoeForCausalLM on
MXFP4 experts (inputs and expected values: tests/moe_mxfp4_ref.py).

1. exact pairing over moe_block_ref.PAIRING_CASES (moe_gemm_mxfp4w_kernel<T, MB, GU>, MB = 1 / 2 / 4 as listed in
   tests/test_gpu_moe_experts.py): torch.equal to the float64 restatement over dequantize_mxfp4 — pins expert, row,
   nibble order and scale group.
2. wide scales, 2^-25 .. 2^16, one product per output, both launches: torch.equal to T(x * q * 2^e).
3. a 0xFF scale byte is a NaN weight for its row, and for nothing else.
4. the block on quantize_experts("mxfp4") against the float64 block over the dequantised weights, at the 16-bit bound.
5. the tiny model, the engine (eager = graphed tokens) and OfflineInferenceEngine on MXFP4 experts.
6. the Python shim's refusals."""
import pytest
import torch

from tests import moe_block_ref as R
from tests import moe_mxfp4_ref as MX
from tests import test_gpu_moe_model as MM
from tests.golden import cases as C
from tests.test_gpu_moe_experts import _checked, _poisoned
from tests.test_gpu_moe_fp8 import _cpu_logits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", R.PAIRING_CASES, ids=[c.name for c in R.PAIRING_CASES])
@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_exact_pairing_mxfp4(case, dt):
    from hydrainfer_amd._C.kernel.moe import experts as K
    T = R.DTYPES[dt]
    f = MX.mx_pairing(case)
    p = f.p
    n, topk, n_e, h, inter = case.n, case.topk, case.E, case.h, case.I
    x, ids, w, shared = p.x.to(T).to(DEV), p.ids.to(DEV), p.w.to(DEV), p.shared.to(T).to(DEV)
    qgu, qdown, sgu, sdown = f.qgu.to(DEV), f.qdown.to(DEV), f.sgu.to(DEV), f.sdown.to(DEV)
    seg = K.segments(ids, n_e)

    act_buf, act = _poisoned(n * topk, inter, T)
    K.gate_up_silu(x, qgu, seg, topk, out=act, w_gate_up_scale=sgu)
    _checked(act_buf, act, "act")
    assert torch.equal(act.cpu(), MX.pairing_act(f, T)), "act: a slot met another token, expert, nibble or scale group"

    y_buf, y = _poisoned(n * topk, h, T)
    K.down(act, qdown, seg, topk, out=y, w_down_scale=sdown)
    _checked(y_buf, y, "y")
    assert torch.equal(y.cpu(), MX.pairing_y(f, T)), "y: down paired a slot with another expert, nibble or scale group"

    one_call = K.experts_forward(x, qgu, qdown, w, ids, shared, w_gate_up_scale=sgu, w_down_scale=sdown)
    assert torch.equal(one_call.cpu(), MX.pairing_out(f, T))


def _wide_launches(T, sgu=None, sdown=None):
    from hydrainfer_amd._C.kernel.moe import experts as K
    c = MX.wide_case()
    n, topk = MX.WIDE_N, MX.WIDE_TOPK
    seg = K.segments(c.ids.to(DEV), MX.WIDE_E)
    act_buf, act = _poisoned(n * topk, MX.WIDE_I, T)
    K.gate_up_silu(c.x.to(T).to(DEV), c.qgu.to(DEV), seg, topk, out=act, w_gate_up_scale=(c.sgu if sgu is None else sgu).to(DEV))
    y_buf, y = _poisoned(n * topk, MX.WIDE_H, T)
    K.down(c.act_in.to(T).to(DEV), c.qdown.to(DEV), seg, topk, out=y, w_down_scale=(c.sdown if sdown is None else sdown).to(DEV))
    return (act_buf, act), (y_buf, y)


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_wide_scales_one_product_per_output(dt):
    T = R.DTYPES[dt]
    (act_buf, act), (y_buf, y) = _wide_launches(T)
    _checked(act_buf, act, "act")
    _checked(y_buf, y, "y")
    c = MX.wide_case()
    for got, want, what in ((act.cpu(), MX.wide_act(c, T), "act = T(32 T(x q 2^e))"), (y.cpu(), MX.wide_y(c, T), "y = T(x q 2^e)")):
        diff = int((got != want).sum())
        assert diff == 0, f"{diff} of {want.numel()} elements differ from {what} (the scaled weight was rounded?)"


@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_a_nan_scale_byte_is_a_nan_weight(dt):
    """0xFF in one group of one up row and of one down row of a routed expert: that output of every slot of the expert
    is NaN (0 * NaN is NaN, so the one-hot rows do not hide it), and nothing else is."""
    T = R.DTYPES[dt]
    c = MX.wide_case()
    e0, j0, c0 = int(c.ids[0, 0]), 77, 200
    sgu, sdown = c.sgu.clone(), c.sdown.clone()
    sgu[e0, MX.WIDE_I + j0, 3] = MX.NAN_BYTE
    sdown[e0, c0, 6] = MX.NAN_BYTE
    (_, act), (_, y) = _wide_launches(T, sgu, sdown)
    act, y = act.cpu(), y.cpu()
    want_act, want_y = MX.wide_act(c, T), MX.wide_y(c, T)
    of_e0 = c.ids.reshape(-1) == e0
    assert 0 < int(of_e0.sum()) < MX.WIDE_N * MX.WIDE_TOPK
    nan_act = torch.zeros_like(want_act, dtype=torch.bool)
    nan_act[of_e0, j0] = True
    nan_y = torch.zeros_like(want_y, dtype=torch.bool)
    nan_y[of_e0, c0] = True
    assert torch.equal(torch.isnan(act), nan_act) and torch.equal(act[~nan_act], want_act[~nan_act])
    assert torch.equal(torch.isnan(y), nan_y) and torch.equal(y[~nan_y], want_y[~nan_y])


BLOCK_CASES = [(dt, norm, n) for dt in R.DTYPES for norm in (False, True) for n in R.N_VALUES]


@pytest.mark.parametrize("dt,norm,n", BLOCK_CASES, ids=[R.fixture_key(*c) for c in BLOCK_CASES])
def test_mxfp4_block_against_the_fixture_inputs(dt, norm, n):
    from hydrainfer_amd._C.kernel.moe import experts as K
    from hydrainfer_amd.layer.moe import SparseMoE
    c = R.block_case(dt, norm, n)
    sd = R.block_weights(dt)
    moe = SparseMoE.from_reference_state_dict("", sd, R.TOPK, norm, R.SCALE, device=DEV).quantize_experts("mxfp4")
    assert moe.experts_mxfp4 and not moe.experts_fp8 and moe.w_gate_up.shape == (R.E, 2 * R.I, R.H // 2)
    out = moe.forward(c.x.to(DEV)).cpu()
    ids = moe.last_topk_ids.cpu()
    assert torch.equal(ids.sort(dim=1).values, c.ref_ids.sort(dim=1).values), "other experts than the reference's"
    wr, _, _, sgu, sdown = R.stacked(sd)
    wgu = K.dequantize_mxfp4(moe.w_gate_up.cpu(), moe.w_gate_up_scale.cpu())
    wdown = K.dequantize_mxfp4(moe.w_down.cpu(), moe.w_down_scale.cpu())
    y64, _, _ = R.block(c.x, wr, wgu, wdown, sgu, sdown, R.TOPK, norm, R.SCALE, "f64", ids=ids)
    ratio = R.error_ratio(out, y64, R.TOL[dt])
    print(f"mxfp4 {R.fixture_key(dt, norm, n)}: ratio to float64 over the dequantised weights {ratio:.3f}; bound 2")
    assert ratio <= 2.0


@pytest.mark.parametrize("dname", list(MM.LOGIT_TOL))
def test_mxfp4_model_matches_the_cpu_composition(dname):
    from hydrainfer_amd.layer.causal_attention import AttentionParametersBuilder
    from hydrainfer_amd.memory.kv_cache import KVCache
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    from hydrainfer_amd.model.llama import LanguageModelParameters
    dt, dev, shape = C.DTYPES[dname], torch.device(DEV), MM.moe_shape()
    model = DeepseekMoeForCausalLM.from_reference_state_dict(shape, MM.reference_sd(dname), dt, dev).quantize_experts("mxfp4")
    assert model.state["l1.moe.wgu"].dtype == torch.uint8 and model.moe[1].experts_mxfp4
    want_all, toks = _cpu_logits(dname, MX.dequantised_sd(model.to_reference_state_dict(), dt))
    pool = MM._pool(dt, shape.num_hidden_layers).to(dev)
    gen = MM._steps()
    m = next(gen)
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
        assert err <= MM.LOGIT_TOL[dname], f"step {s}: logits max abs err {err} > {MM.LOGIT_TOL[dname]}"
        if s < C.TINY_DECODE_STEPS:
            m = gen.send(toks[s])                 # both sides follow the CPU's tokens


def _mxfp4_cluster(dname, graph_decode):
    cluster, n_img_tok = MM._engine_cluster(dname, graph_decode)
    lm = cluster.nodes[0].executor.fill_executor.language_model.language_model
    lm.quantize_experts("mxfp4")                   # before the first step: nothing has been captured yet
    assert lm.moe[1].experts_mxfp4
    return cluster, n_img_tok


def test_engine_eager_and_graphed_decode_give_the_same_tokens_mxfp4():
    from hydrainfer_amd.engine import InstructionCreator
    from tests.engine_util import run_trace
    outs, decoder = [], None
    for graph_decode in (False, True):
        cluster, n_img_tok = _mxfp4_cluster("bf16", graph_decode)
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


def test_offline_engine_serves_the_mxfp4_model():
    from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
    from hydrainfer_amd.engine.offline import OfflineInferenceEngine, OfflineRequest
    from tests.engine_util import run_trace
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (7 + 9 * i,), generator=g).tolist() for i in range(3)]
    cluster, n_img_tok = _mxfp4_cluster("fp16", False)
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
    T, u8 = torch.bfloat16, dict(dtype=torch.uint8, device=DEV)
    x = torch.zeros((2, 256), dtype=T, device=DEV)
    ids = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    seg = K.segments(ids, 4)
    q, s = torch.zeros((4, 256, 128), **u8), torch.full((4, 256, 8), 127, **u8)
    qd, sd = torch.zeros((4, 256, 64), **u8), torch.full((4, 256, 4), 127, **u8)
    act = K.gate_up_silu(x, q, seg, 2, w_gate_up_scale=s)                                  # the forms that are accepted
    K.down(act, qd, seg, 2, w_down_scale=sd)
    refused = [lambda bad=bad: K.gate_up_silu(x, q, seg, 2, w_gate_up_scale=bad)           # a scale of the wrong shape or dtype
               for bad in (s[:, :, :4].contiguous(), s[:, :128].contiguous(), s.to(torch.int8), s.to(T), s.cpu(), None)]
    refused += [lambda bad=bad: K.down(act, qd, seg, 2, w_down_scale=bad) for bad in (sd[:, :, :2].contiguous(), sd.to(torch.int32), None)]
    refused += [lambda: K.gate_up_silu(torch.zeros((2, 382), dtype=T, device=DEV), torch.zeros((4, 256, 191), **u8), seg, 2,
                                       w_gate_up_scale=torch.full((4, 256, 11), 127, **u8)),   # an odd K / 2
                lambda: K.experts_forward(x, q, qd, torch.ones((2, 2), device=DEV), ids, w_gate_up_scale=s)]
    for call in refused:
        with pytest.raises(_lib.HydraHipError):
            call()
