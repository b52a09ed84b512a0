"""GPU: prompt log-probabilities through the engine (SamplingParameters.prompt_logprobs -> Fill.score_targets -> the
builder's ScorePlan -> the eager step's hx_token_logprob_rows launch over the union logits -> rcb.prompt_logprobs ->
OfflineInferenceOutput / the chat stream's first chunk), on the tiny model of tests/engine_util.py.  Asking changes no
token; every prompt token but the first and the image placeholders gets exactly one entry, and every entry is held to
the float64 reference of the logits row that produced it."""
import asyncio
import json
import math
from collections import Counter
from types import SimpleNamespace as NS

import pytest
import torch

from hydrainfer_amd.engine import BatchSchedulerConfig, InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.engine.node import LocalCluster
from hydrainfer_amd.engine.rcb import PromptTokenLogprob
from tests.engine_util import make_node, run_trace
from tests.golden import cases as C
from tests.token_logprob_ref import ATOL, token_reference

pytestmark = pytest.mark.gpu

N_IMG_TOK = (C.TINY_CLIP["image_size"] // C.TINY_CLIP["patch_size"]) ** 2
BS = C.TINY_BLOCK_SIZE
DT = torch.float16
IMG = C.TINY_IMAGE_TOKEN_ID
LOGITS_TOL = 2e-2           # tests/test_tiny_llama.py: the fp16 tiny model's logits against the reference's CPU path


class ScoreTap:
    """A LlavaLanguageModel that counts, per executor step, which of its entry points ran, and keeps what a scoring step's
    forward saw and gave: the inputs, the union logits (on the host) and — caught by a wrapper round the executor's
    _execute_scoring — the step's ScorePlan."""

    def __init__(self, lm):
        self.lm, self.language_model, self.image_token_id = lm, lm.language_model, lm.image_token_id
        self.steps = []          # NS(plan, logits, inputs, calls, requests) per fill step
        self.calls, self.last, self.plan = [], None, None

    def embed(self, *a):
        return self.lm.embed(*a)

    def forward_logits(self, input_ids, image_features, position_ids, params):
        self.calls.append("forward_logits")
        logits = self.lm.forward_logits(input_ids, image_features, position_ids, params)
        self.last = (logits, input_ids, image_features, position_ids)
        return logits

    def forward(self, *a):
        self.calls.append("forward")
        return self.lm.forward(*a)

    def forward_logprobs(self, *a, **k):
        self.calls.append("forward_logprobs")
        return self.lm.forward_logprobs(*a, **k)

    def forward_penalized(self, *a, **k):
        self.calls.append("forward_penalized")
        return self.lm.forward_penalized(*a, **k)

    def forward_sampled(self, *a, **k):
        self.calls.append("forward_sampled")
        return self.lm.forward_sampled(*a, **k)


def _models():
    from hydrainfer_amd.model.clip import ClipShape, LlavaVisionModel, random_state_dict
    from hydrainfer_amd.model.llama import LlamaForCausalLM, LlamaShape
    from hydrainfer_amd.model.llava import LlavaLanguageModel
    dev = torch.device("cuda:0")
    lshape, cshape = LlamaShape(**C.TINY_LLAMA), ClipShape(**C.TINY_CLIP)
    lm = LlavaLanguageModel(LlamaForCausalLM.from_reference_state_dict(lshape, C.tiny_llama_state_dict(DT), DT, dev),
                            image_token_id=IMG)
    clip = {k: v.to(DT).to(dev) for k, v in random_state_dict(cshape, seed=3, std=0.05).items()}
    return lm, LlavaVisionModel(cshape, DT, dev, clip), lshape


def _cluster(chunked, graph_decode, budget=64, topology=("EPD",)):
    from hydrainfer_amd.memory.token_cache_manger import (TokenCacheBlockManager, TokenCacheBlockManagerConfig,
                                                          TokenCacheBlockManagerContext)
    lm, vision, lshape = _models()
    tap = ScoreTap(lm)
    nodes = []
    for k, t in enumerate(topology):
        ctx = TokenCacheBlockManagerContext(rank=0, rank2host={0: "localhost"})
        kv = TokenCacheBlockManager(TokenCacheBlockManagerConfig(
            n_layers=lshape.num_hidden_layers, n_tokens=2, n_blocks=48, block_size=BS, n_heads=lshape.num_key_value_heads,
            head_size=lshape.head_dim, dtype="fp16", device="cuda:0"), ctx)
        img = TokenCacheBlockManager(TokenCacheBlockManagerConfig(
            n_layers=1, n_tokens=1, n_blocks=6, block_size=N_IMG_TOK, n_heads=lshape.num_attention_heads,
            head_size=lshape.head_dim, dtype="fp16", device="cuda:0"), ctx)
        cfg = BatchSchedulerConfig(priority="prefill", max_running_requests=6, chunked_prefill=chunked,
                                   token_budgets=budget, image_budgets=2)
        node = make_node(f"{t}{k}", t, tap, vision, kv, img, lshape, DT, torch.device("cuda:0"), cfg,
                         graph_decode=graph_decode)
        fill = node.executor.fill_executor
        if fill is not None:
            def scoring(batch, inputs, real=fill._execute_scoring):
                tap.plan = inputs.score_plan                # the step's ScorePlan, as the executor got it
                real(batch, inputs)
            fill._execute_scoring = scoring

            def execute(batch, real=fill.execute):
                tap.calls, tap.last, tap.plan = [], None, None
                requests = [rcb.request_id for rcb, inst in batch]
                real(batch)
                plan = tap.plan
                kept = None if plan is None else tuple(None if t is None else t.detach().cpu() for t in tap.last)
                tap.steps.append(NS(plan=plan, kept=kept, calls=list(tap.calls), requests=requests))
            fill.execute = execute
        nodes.append(node)
    return LocalCluster(nodes), tap


def _creator():
    return InstructionCreator(image_token_id=IMG, n_image_tokens_per_image=N_IMG_TOK, block_size=BS, ignore_eos=True)


def _requests(ask, extra=None, text_len=(10, 45, 3, 28, 17, 33), max_tokens=(5, 3, 6, 4, 7, 2), arrive=None):
    """ask[i]: None, or the request's prompt_logprobs; extra: {i: more SamplingParameters fields}.  Requests 0, 1, 2, 4,
    5 carry an image (the prompts of tests/test_gpu_logprobs_engine.py), request 3 is text only; the prompts run up to 46
    tokens."""
    g = torch.Generator().manual_seed(4242)
    pixels = C.tiny_clip_pixels(2)
    out = []
    for i, (n, m) in enumerate(zip(text_len, max_tokens)):
        text = torch.randint(0, IMG, (n,), generator=g).tolist()
        has_image = i != 3
        if i >= len(ask):
            continue
        sp = SamplingParameters(max_tokens=m, prompt_logprobs=ask[i], **dict(extra or {}).get(i, {}))
        out.append(((0 if i < 3 else 2) if arrive is None else arrive[i], TokenRequest(
            request_id=i, token_ids=([IMG] if has_image else []) + text,
            pixel_values=pixels[i % 2:i % 2 + 1].clone() if has_image else None, image_size=(56, 56),
            image_hash=9000 + i % 2, sampling_params=sp)))
    return out


def _check_entries(rcbs, reqs, tap):
    """Every entry against the float64 reference of the row that produced it; every token that must be scored is, once."""
    seen, worst = Counter(), 0.0
    own = {r.request_id: r.token_ids for _, r in reqs}
    for st in tap.steps:
        if st.plan is None:
            continue
        plan, logits = st.plan, st.kept[0]
        assert logits.shape[0] == len(plan.rows) == len(plan.targets) == len(plan.dst)
        ref = token_reference(logits, plan.targets, plan.top_k)
        for u, dst in enumerate(plan.dst):
            if dst is None:
                assert plan.targets[u] == -1
                continue
            rcb, idx = dst
            e, k = rcb.prompt_logprobs[idx], rcb.sampling_params.prompt_logprobs
            assert isinstance(e, PromptTokenLogprob) and e.token_id == plan.targets[u] == own[rcb.request_id][idx]
            assert e.rank == int(ref[1][u]) and len(e.top) == k and [t for t, _ in e.top] == ref[2][u][:k].tolist()
            for got, want in [(e.logprob, float(ref[0][u]))] + [(lp, float(w)) for (_, lp), w in zip(e.top, ref[3][u])]:
                assert math.isfinite(got) and math.isfinite(want)
                worst = max(worst, abs(got - want))
            if k:
                assert (e.rank == 0) == (e.top[0][0] == e.token_id)
            seen[(rcb.request_id, idx)] += 1
    n = 0
    for rcb in rcbs:
        tokens = own[rcb.request_id]
        if rcb.sampling_params.prompt_logprobs is None:
            assert rcb.prompt_logprobs == []
            continue
        assert len(rcb.prompt_logprobs) == len(tokens) and rcb.prompt_logprobs[0] is None
        for i, t in enumerate(tokens):
            scored = i >= 1 and t != IMG
            assert (rcb.prompt_logprobs[i] is not None) == scored and seen[(rcb.request_id, i)] == int(scored)
            n += int(scored)
    assert sum(seen.values()) == n
    print(f"{n} prompt entries, max |error| vs float64 log-softmax of the step's own logits: {worst:.2e}")
    assert worst <= ATOL
    return n


@pytest.mark.parametrize("chunked", [True, False], ids=["budget16", "unchunked"])
@pytest.mark.parametrize("graph_decode", [False, True], ids=["eager", "graphs"])
def test_asking_changes_no_token_and_every_entry_is_right(graph_decode, chunked):
    budget = 16 if chunked else 64
    plain = run_trace(_cluster(chunked, graph_decode, budget)[0], _creator(), _requests([None] * 6))
    cluster, tap = _cluster(chunked, graph_decode, budget)
    ask = [0, 2, 5, 20, 0, 1]
    reqs = _requests(ask)
    asked = run_trace(cluster, _creator(), reqs)
    assert [r.output_token_ids for r in asked] == [r.output_token_ids for r in plain]
    assert all(len(r.output_token_ids) == r.sampling_params.max_tokens for r in asked)
    n = _check_entries(asked, reqs, tap)
    assert n == sum(sum(i >= 1 and t != IMG for i, t in enumerate(r.token_ids)) for _, r in reqs)
    if chunked:
        assert sum(st.plan is not None for st in tap.steps) > 6, "no prompt was scored in chunks"
    fill = cluster.nodes[0].executor.fill_executor
    assert fill.pending is None and fill.cohort is None
    # decode is untouched: no step behind the prefills scores, and with graphs the eager forward is not used for it
    last_scoring = max(i for i, st in enumerate(tap.steps) if st.plan is not None)
    assert all(st.calls in (["forward"], []) for st in tap.steps[last_scoring + 1:])


def test_mixed_batch(monkeypatch):
    """Scoring only; scoring + logprobs; scoring + penalties; scoring + temperature with a seed; plain — tokens of each as
    without prompt_logprobs, and steps that score nothing make today's calls."""
    from hydrainfer_amd.engine import executor as ex
    extra = {1: dict(logprobs=True, top_logprobs=3), 2: dict(frequency_penalty=0.8, repetition_penalty=1.3),
             3: dict(temperature=0.9, top_p=0.9, seed=1234)}
    ask = [2, 0, 1, 5, None]
    kernel_calls = []
    for name in ("token_logprob_rows", "argmax_rows", "logprob_rows", "penalized_argmax_rows", "sample_rows"):
        def counted(*a, _real=getattr(ex, name), _name=name, **k):
            kernel_calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(ex, name, counted)

    cluster_of = []

    def run(asks):
        cluster, tap = _cluster(True, False, 40)
        cluster_of[:] = [cluster]
        reqs = _requests(asks, extra, arrive=[0] * 6)
        marks = []
        fill = cluster.nodes[0].executor.fill_executor

        def execute(batch, real=fill.execute):
            at = len(kernel_calls)
            real(batch)
            marks.append(kernel_calls[at:])
        fill.execute = execute
        return run_trace(cluster, _creator(), reqs), reqs, tap, marks

    base, _, base_tap, base_marks = run([None] * 5)
    assert all(st.plan is None for st in base_tap.steps) and "token_logprob_rows" not in sum(base_marks, [])
    assert "argmax_rows" not in sum(base_marks, [])             # (the executor's own argmax_rows call is the scoring step's)
    again = run(ask)[0]
    asked, reqs, tap, marks = run(ask)
    assert [r.output_token_ids for r in asked] == [r.output_token_ids for r in base]
    assert asked[3].sampling_params.seed == 1234
    assert again[3].output_token_ids == asked[3].output_token_ids, "the sampled request does not replay by its seed"
    _check_entries(asked, reqs, tap)
    assert [e.token_id for e in asked[1].output_logprobs] == asked[1].output_token_ids
    for a, b in zip(asked[1].output_logprobs, base[1].output_logprobs):
        assert a.token_id == b.token_id and abs(a.logprob - b.logprob) <= 2 * ATOL
    # a step that scores: one forward_logits, one token_logprob_rows, then the sampling kernels
    scoring = [i for i, st in enumerate(tap.steps) if st.plan is not None]
    assert scoring and all(tap.steps[i].calls == ["forward_logits"] and marks[i][0] == "token_logprob_rows"
                           and marks[i].count("token_logprob_rows") == 1 for i in scoring)
    rest = [i for i in range(len(tap.steps)) if i not in scoring]
    assert rest and all("token_logprob_rows" not in marks[i] and "argmax_rows" not in marks[i] for i in rest)
    # (the two runs do not correspond step by step: the run without prompt_logprobs takes prefix-cache hits on the shared
    # image block, a scoring prompt takes none) — every call pattern of a step that scores nothing is one the run without
    # prompt_logprobs made too, and request 4, which never asked, is in such steps from its first chunk on
    today = {(tuple(st.calls), tuple(m)) for st, m in zip(base_tap.steps, base_marks)}
    assert all((tuple(tap.steps[i].calls), tuple(marks[i])) in today for i in rest)
    assert any(4 in tap.steps[i].requests for i in rest)
    # and alone on the same engine the plain request takes the plain forward, step after step
    n_before = len(tap.steps)
    plain = run_trace(cluster_of[0], _creator(), _requests([None] * 5, arrive=[0] * 6)[4:5])[0]
    assert len(plain.output_token_ids) == plain.sampling_params.max_tokens and plain.prompt_logprobs == []
    assert len(tap.steps) > n_before and all(st.calls == ["forward"] for st in tap.steps[n_before:])
    assert all(m == [] for m in marks[n_before:])


def _alone(cluster, reqs):
    """The requests one after the other, each alone in the engine: the prefill of a request is the same forward whatever
    the topology."""
    return [run_trace(cluster, _creator(), [(0, r)])[0] for _, r in reqs]


def test_scores_agree_with_the_cpu_oracle():
    """The engine's prompt scores against the fp32 log-softmax of OracleLlama over the whole prompt in one pass (the
    image's embeddings as the engine's vision tower gave them): within 2 x the logits tolerance of
    tests/test_tiny_llama.py for this model and dtype — a logprob's error is at most the target logit's plus the
    log-sum's.  Every scored position is compared."""
    from hydrainfer_amd.model.llama import LlamaShape
    from oracle.model import OracleAttnMeta, OracleLlama
    cluster, tap = _cluster(False, False, 64)
    reqs = _requests([0] * 6)
    rcbs = _alone(cluster, reqs)
    shape = LlamaShape(**C.TINY_LLAMA)
    sd = {k: v.float() for k, v in C.tiny_llama_state_dict(DT).items()}
    oracle = OracleLlama(shape, sd, torch.float32)
    steps = [st for st in tap.steps if st.plan is not None]
    assert len(steps) == len(reqs)
    worst, n = 0.0, 0
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    for st, rcb, (_, req) in zip(steps, rcbs, reqs):
        _, ids, feats, pos = st.kept
        m = ids.numel()
        assert pos.tolist() == list(range(m)) and st.requests == [rcb.request_id]
        emb = torch.nn.functional.embedding(ids.long(), sd["model.embed_tokens.weight"])
        if feats is not None:
            emb[ids == IMG] = feats.reshape(-1, emb.shape[-1]).float()
        nb = (m + BS - 1) // BS
        meta = OracleAttnMeta(i32([0, m]), i32([0, m]), i32(list(range(m))), i32(list(range(nb))), i32([0, nb]))
        caches = [(torch.zeros(nb, BS, shape.num_key_value_heads, shape.head_dim),
                   torch.zeros(nb, BS, shape.num_key_value_heads, shape.head_dim)) for _ in range(shape.num_hidden_layers)]
        lsm = torch.log_softmax(oracle.forward_logits(emb, pos, meta, caches).double(), dim=-1)
        at, row_of = 0, []                      # own index -> the row in front of that token
        for t in req.token_ids:
            row_of.append(at - 1)
            at += N_IMG_TOK if t == IMG else 1
        assert at == m
        for i, e in enumerate(rcb.prompt_logprobs):
            if e is not None:
                worst, n = max(worst, abs(e.logprob - float(lsm[row_of[i], e.token_id]))), n + 1
    print(f"{n} prompt logprobs against the fp32 oracle: max |difference| {worst:.2e} (bound {2 * LOGITS_TOL})")
    assert n == sum(sum(i >= 1 and t != IMG for i, t in enumerate(r.token_ids)) for _, r in reqs)
    assert worst <= 2 * LOGITS_TOL


def test_prefix_cache_is_not_taken():
    """A plain request publishes its prompt's blocks; the same prompt, scoring, must still compute every row."""
    reqs = _requests([None, None])[1:2]           # the 46-token image prompt: three full blocks to hit
    scoring = _requests([None, 3])[1:2]
    cluster, tap = _cluster(True, False, 64)
    first = run_trace(cluster, _creator(), [(0, reqs[0][1])])[0]
    hashes = next(i for i in _creator().process(reqs[0][1]).instructions if getattr(i, "hashes", None) and hasattr(i, "token_ids")).hashes
    shared = cluster.nodes[0].executor.fill_executor.kv_manager.shared_cache
    assert len(hashes) == 3 and all(b != -1 for b in shared.match(hashes)), "the plain run published nothing to hit"
    tap.steps.clear()
    warm = run_trace(cluster, _creator(), [(0, scoring[0][1])])[0]
    n = _check_entries([warm], scoring, tap)
    assert n == len(scoring[0][1].token_ids) - 1 and warm.output_token_ids == first.output_token_ids
    fresh_cluster, fresh_tap = _cluster(True, False, 64)
    fresh = run_trace(fresh_cluster, _creator(), [(0, scoring[0][1])])[0]
    _check_entries([fresh], scoring, fresh_tap)
    for a, b in zip(warm.prompt_logprobs, fresh.prompt_logprobs):
        assert (a is None) == (b is None)
        if a is not None:
            assert (a.token_id, a.rank, [t for t, _ in a.top]) == (b.token_id, b.rank, [t for t, _ in b.top])
            assert abs(a.logprob - b.logprob) <= 2 * ATOL


def test_offline_engine_returns_prompt_logprobs():
    from hydrainfer_amd.engine.offline import OfflineInferenceEngine, OfflineRequest
    lm, vision, _ = _models()
    eng = OfflineInferenceEngine(lm, vision, DT, "cuda:0", max_running_requests=4, token_budgets=64, max_context=256,
                                 warm_up=False)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, IMG, (6 + 5 * i,), generator=g).tolist() for i in range(4)]
    plain = eng.generate([OfflineRequest(p, None, max_tokens=4) for p in prompts])
    ask = (0, None, 2, 20)
    asked = eng.generate([OfflineRequest(p, None, max_tokens=4, prompt_logprobs=ask[i]) for i, p in enumerate(prompts)])
    assert [o.output_token_ids for o in asked] == [o.output_token_ids for o in plain]
    assert all(o.prompt_logprobs == [] for o in plain) and asked[1].prompt_logprobs == []
    for i in (0, 2, 3):
        recs = asked[i].prompt_logprobs
        assert len(recs) == len(prompts[i]) and recs[0] is None and all(r is not None for r in recs[1:])
        assert [r.token_id for r in recs[1:]] == prompts[i][1:]
        assert all(len(r.top) == ask[i] and -math.log(C.TINY_LLAMA["vocab_size"]) - 20 < r.logprob <= 0 for r in recs[1:])
        assert all(0 <= r.rank < C.TINY_LLAMA["vocab_size"] for r in recs[1:])
        assert all((r.rank == 0) == (r.top[0][0] == r.token_id) for r in recs[1:] if r.top)
        assert all(r.top[j][1] >= r.top[j + 1][1] for r in recs[1:] for j in range(len(r.top) - 1))
    for bad in (-1, 21, True, 1.5):
        with pytest.raises(ValueError):
            eng.generate([OfflineRequest(prompts[0], None, max_tokens=2, prompt_logprobs=bad)])


async def _raw_stream(base_url, payload):
    """The stream's `data:` objects as they come, [DONE] excluded."""
    import httpx
    out, done = [], False
    async with httpx.AsyncClient(timeout=None) as client:
        async with client.stream("POST", f"{base_url}/chat/completions", json=payload) as response:
            assert response.status_code == 200
            async for line in response.aiter_lines():
                if not line or not line.startswith("data: "):
                    continue
                if line.strip() == "data: [DONE]":
                    done = True
                    break
                out.append(json.loads(line[len("data: "):]))
    return out, done


def test_api_server_first_chunk_carries_the_array():
    from hydrainfer_amd.entrypoint import ApiServer, EngineFrontend, SyntheticTokenizer
    from hydrainfer_amd.entrypoint.api_protocol import parse_chat_completion_request as parse
    from hydrainfer_amd.model.processor import ClipImageProcessor
    from tests.test_api_server import _payload, _png
    tok = SyntheticTokenizer(image_token_id=IMG, lo=3, hi=IMG)
    cluster, tap = _cluster(True, True, 64)
    front = EngineFrontend(cluster, _creator(), device=torch.device("cuda:0"))
    server = ApiServer(front, tok, ClipImageProcessor(size=56), host="127.0.0.1", port=0, image_size=(56, 56))
    payloads = [_payload("What is shown in this image?", _png(1), 6), _payload("Describe the weather. Briefly.", None, 5),
                _payload("one two three four five six seven", _png(2), 4)]
    payloads[0]["prompt_logprobs"] = 2
    payloads[2]["prompt_logprobs"] = 0
    payloads[2]["logprobs"] = True

    async def go():
        await server.start()
        front.start()
        try:
            return await asyncio.gather(*[_raw_stream(f"http://127.0.0.1:{server.port}/v1", p) for p in payloads])
        finally:
            front.stop()
            await server.close()
    got = asyncio.run(go())
    assert front.error is None and front.n_admitted == 3
    for (chunks, done), p in zip(got, payloads):
        assert done and len(chunks) == p["max_tokens"] + 1
        assert chunks[0]["choices"][0]["delta"] == {"role": "assistant", "content": ""}
        assert all("prompt_logprobs" not in c for c in chunks[1:])
        keys = ["id", "object", "created", "model", "choices"]
        assert all(list(c) == keys for c in chunks[1:])
        if "prompt_logprobs" not in p:
            assert list(chunks[0]) == keys              # the other stream's chunks are what they were
            continue
        assert list(chunks[0]) == keys + ["prompt_logprobs"]
        arr, k = chunks[0]["prompt_logprobs"], p["prompt_logprobs"]
        token_ids = server._token_request(parse(p)).token_ids
        assert len(arr) == len(token_ids) and arr[0] is None
        for t, e in zip(token_ids, arr):
            if t == IMG or e is None:
                assert e is None and (t == IMG or t == token_ids[0])
                continue
            assert list(e) == ["token", "logprob", "rank", "bytes", "top_logprobs"] and e["token"] == tok.decode(t)
            assert e["logprob"] <= 0 and 0 <= e["rank"] < C.TINY_LLAMA["vocab_size"] and len(e["top_logprobs"]) == k
            assert e["bytes"] == list(e["token"].encode())
        assert sum(e is not None for e in arr) == len(token_ids) - 1 - token_ids.count(IMG)
    assert all("logprobs" in c["choices"][0] for c in got[2][0][1:]) and "logprobs" not in got[0][0][1]["choices"][0]


def test_separate_e_p_d_nodes_give_the_single_nodes_entries():
    """One process, three nodes: the request control block is one object, so the scores gathered on the prefill node are
    there when the decode node ends the request."""
    reqs = _requests([3, 0, 1, 2])
    single_cluster, single_tap = _cluster(True, False, 16)
    single = _alone(single_cluster, reqs)
    epd_cluster, epd_tap = _cluster(True, False, 16, topology=("E", "P", "D"))
    split = _alone(epd_cluster, reqs)
    assert _check_entries(single, reqs, single_tap) == _check_entries(split, reqs, epd_tap)
    assert [r.output_token_ids for r in split] == [r.output_token_ids for r in single]
    for a, b in zip(single, split):
        assert len(a.prompt_logprobs) == len(b.prompt_logprobs)
        for x, y in zip(a.prompt_logprobs, b.prompt_logprobs):
            assert (x is None) == (y is None)
            if x is not None:
                assert (x.token_id, x.rank, [t for t, _ in x.top]) == (y.token_id, y.rank, [t for t, _ in y.top])
                assert abs(x.logprob - y.logprob) <= 2 * ATOL
