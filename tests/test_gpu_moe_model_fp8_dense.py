"""GPU: DeepseekMoeForCausalLM with EVERY linear of the decoder layers FP8 block-scaled — the fully published DeepSeek-V3
format: attention projections, the dense layer's MLP, routed and shared experts float8_e4m3fn with weight_scale_inv;
embeddings, lm_head, norms and the router 16-bit — loaded from such a state dict (tests/linear_fp8_ref.published_full).

The tiny model is tests/test_gpu_moe_model.py's.  The prompts here are 50 and 23 tokens: the prefill is 73 rows, so the
attention projections and the dense MLP run the dequantise + library GEMM path (above 64 rows) and the decode steps — and
the prefill's last layer, which sees the two selected rows only — the FP8 decode GEMM.  The CPU side is the oracle on
moe_fp8_ref.dequantised_sd(...): float(q) * scale cast to T."""
import pytest
import torch

from tests import linear_fp8_ref as L8
from tests import moe_block_ref as R
from tests import moe_fp8_ref as F8
from tests import test_gpu_moe_model as MM
from tests.golden import cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP8 = F8.FP8
PROMPTS = (50, 23)
FP8_KEYS = ("l0.wqkv", "l0.wo", "l0.wgu", "l0.wdown", "l1.wqkv", "l1.wo", "l1.moe.sgu", "l1.moe.sdown", "l1.moe.wgu", "l1.moe.wdown")


def _published_sd(dname):
    from hydrainfer_amd._C.kernel.moe.experts import quantize_fp8_block
    return L8.published_full(MM.reference_sd(dname), quantize_fp8_block)


def _steps():
    """MM._steps with this file's prompts: the prefill of both (73 rows), then TINY_DECODE_STEPS decode steps."""
    BS = MM.BS
    tables, nxt = [], C.TINY_BLOCKS - 1
    for p in PROMPTS:
        n = (p + C.TINY_DECODE_STEPS + BS - 1) // BS
        tables.append([nxt - j for j in range(n)][::-1])
        nxt -= n
    g = torch.Generator().manual_seed(811)
    new = [torch.randint(0, C.TINY_LLAMA["vocab_size"], (p,), generator=g).tolist() for p in PROMPTS]
    lens = [0, 0]
    for _ in range(1 + C.TINY_DECODE_STEPS):
        ids, pos, sel, slots, bt, cu_q, cu_k, cu_b, per = [], [], [], [], [], [0], [0], [0], []
        for r, n in enumerate(new):
            sl = [tables[r][p // BS] * BS + p % BS for p in range(lens[r], lens[r] + len(n))]
            pos += list(range(lens[r], lens[r] + len(n)))
            lens[r] += len(n)
            t = tables[r][: (lens[r] + BS - 1) // BS]
            per.append((len(n), lens[r], sl, t))
            slots += sl; bt += t; ids += n
            cu_q.append(cu_q[-1] + len(n)); cu_k.append(cu_k[-1] + lens[r]); cu_b.append(cu_b[-1] + len(t))
            sel.append(cu_q[-1] - 1)
        nxt_tok = yield dict(ids=ids, pos=pos, sel=sel, slots=slots, bt=bt, cu_q=cu_q, cu_k=cu_k, cu_b=cu_b, per=per,
                             prefill=len(ids) > 2)
        new = [[int(nxt_tok[0])], [int(nxt_tok[1])]]


def _cpu_logits(dname, sd):
    from oracle.model import OracleAttnMeta
    dt, shape = C.DTYPES[dname], MM.moe_shape()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    model = R.oracle_moe_model(shape, sd, dt)
    pool = MM._pool(dt, shape.num_hidden_layers)
    logits, toks = [], []
    gen = _steps()
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
def test_published_model_matches_the_cpu_composition(dname):
    from hydrainfer_amd._C.kernel import gemm
    from hydrainfer_amd.layer.causal_attention import AttentionParametersBuilder
    from hydrainfer_amd.memory.kv_cache import KVCache
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    from hydrainfer_amd.model.llama import LanguageModelParameters
    dt, dev, shape = C.DTYPES[dname], torch.device(DEV), MM.moe_shape()
    sd = _published_sd(dname)
    model = DeepseekMoeForCausalLM.from_reference_state_dict(shape, sd, dt, dev)
    for k in FP8_KEYS:
        assert model.state[k].dtype == FP8 and model.state[k + "_scale"].dtype == torch.float32, k
    assert model.state["lm_head"].dtype == dt and model.state["l1.moe.router"].dtype == dt
    assert model.moe[1].experts_fp8 and model.moe[1].shared_fp8 and not model._decode_fast_path(2, dt, None)
    want_all, toks = _cpu_logits(dname, F8.dequantised_sd(sd, dt))
    pool = MM._pool(dt, shape.num_hidden_layers).to(dev)
    tol = MM.LOGIT_TOL[dname]
    calls = {"kernel": 0, "dequant": 0}
    real_k, real_d = gemm.linear_decode_fp8, gemm.dequant_fp8_block
    gemm.linear_decode_fp8 = lambda *a, **k: (calls.__setitem__("kernel", calls["kernel"] + 1), real_k(*a, **k))[1]
    gemm.dequant_fp8_block = lambda *a, **k: (calls.__setitem__("dequant", calls["dequant"] + 1), real_d(*a, **k))[1]
    try:
        gen = _steps()
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
            if s == 0:
                # 73 rows: qkv and o of both layers and the dense MLP dequantise; the last layer's two selected rows do not
                assert len(m["ids"]) == 73 and calls == {"kernel": 2, "dequant": 6}, calls
                scratch = model.fp8_scratch
                assert scratch is not None and scratch.numel() == max(model.state[k].numel() for k in FP8_KEYS if model.state[k].dim() == 2)
            if s < C.TINY_DECODE_STEPS:
                m = gen.send(toks[s])                 # both sides follow the CPU's tokens
        assert calls == {"kernel": 2 + 8 * C.TINY_DECODE_STEPS, "dequant": 6} and model.fp8_scratch is scratch
    finally:
        gemm.linear_decode_fp8, gemm.dequant_fp8_block = real_k, real_d
    print(f"fp8 dense {dname}: worst logit error {worst:.4f} (tolerance {tol})")
    # quantize_dense() on the loaded model: nothing left to do, twice
    before = dict(model.state)
    model.quantize_dense().quantize_dense()
    assert sorted(before) == sorted(model.state) and all(before[k] is model.state[k] for k in before)


def test_quantize_dense_twice_is_the_identity_after_the_first_call():
    """... and the first call gives the tensors the published state dict holds (the same quantiser, block by block)."""
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    dt, dev = torch.bfloat16, "cpu"          # load-time work in plain torch: the comparison needs no device
    loaded = DeepseekMoeForCausalLM.from_reference_state_dict(MM.moe_shape(), _published_sd("bf16"), dt, dev)
    model = DeepseekMoeForCausalLM.from_reference_state_dict(MM.moe_shape(), MM.reference_sd("bf16"), dt, dev)
    assert model.quantize_experts().quantize_dense() is model
    first = dict(model.state)
    model.quantize_dense()
    assert sorted(first) == sorted(model.state) == sorted(loaded.state)
    for k, v in first.items():
        assert v is model.state[k], k
        assert v.dtype == loaded.state[k].dtype and torch.equal(v.view(torch.uint8) if v.dtype == FP8 else v,
                                                                loaded.state[k].view(torch.uint8) if v.dtype == FP8 else loaded.state[k]), k
    assert model.moe[1].shared_gate_up is model.state["l1.moe.sgu"] and model.moe[1].shared_down_scale is model.state["l1.moe.sdown_scale"]


def _published_cluster(dname, graph_decode):
    """MM's engine cluster with the model's linears quantised in place before the first step (nothing captured yet): the
    tensors of the published state dict (test above)."""
    cluster, n_img_tok = MM._engine_cluster(dname, graph_decode)
    lm = cluster.nodes[0].executor.fill_executor.language_model.language_model
    lm.quantize_experts().quantize_dense()
    # the engine takes an image-token id among the text rows for an image placeholder and refuses the batch; with these
    # weights a request of the trace samples it.  Its lm_head row is zeroed (in this model's own copy): a logit of exactly
    # 0 is never the largest of 512
    lm.state["lm_head"][C.TINY_IMAGE_TOKEN_ID].zero_()
    assert lm.moe[1].experts_fp8 and lm.moe[1].shared_fp8 and lm.state["l0.wqkv"].dtype == FP8
    return cluster, n_img_tok


def test_engine_eager_and_graphed_decode_give_the_same_tokens_fp8_dense():
    from hydrainfer_amd.engine import InstructionCreator
    from tests.engine_util import run_trace
    outs, decoder = [], None
    for graph_decode in (False, True):
        cluster, n_img_tok = _published_cluster("bf16", graph_decode)
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


def test_offline_engine_serves_the_published_model():
    from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
    from hydrainfer_amd.engine.offline import OfflineInferenceEngine, OfflineRequest
    from tests.engine_util import run_trace
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (7 + 9 * i,), generator=g).tolist() for i in range(3)]
    cluster, n_img_tok = _published_cluster("fp16", False)
    creator = InstructionCreator(image_token_id=C.TINY_IMAGE_TOKEN_ID, n_image_tokens_per_image=n_img_tok, block_size=MM.BS, ignore_eos=True)
    eager = run_trace(cluster, creator, [(0, TokenRequest(request_id=i, token_ids=p, pixel_values=None, image_size=(0, 0), image_hash=0,
                                                           sampling_params=SamplingParameters(max_tokens=6))) for i, p in enumerate(prompts)])
    node = cluster.nodes[0].executor
    eng = OfflineInferenceEngine(node.fill_executor.language_model, node.image_embed_executor.vision_model, torch.float16, DEV,
                                 max_running_requests=4, token_budgets=64, max_context=256, warm_up=False)
    got = eng.generate([OfflineRequest(p, None, max_tokens=6) for p in prompts])
    assert [r.output_token_ids for r in got] == [r.output_token_ids for r in eager]
    assert all(len(r.output_token_ids) == 6 for r in got)
