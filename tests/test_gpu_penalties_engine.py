"""GPU: frequency / presence / repetition penalties through the engine (SamplingParameters -> the eager step's
forward_penalized -> hx_penalized_argmax_rows, the request's PenaltyHistory fed by _deliver), on the tiny model of
tests/engine_util.py.  Every delivered token of a penalised request is what tests/penalty_ref.py gives for the logits of
that very step (kept by a wrapper round forward_logits) and the tokens delivered before it; requests without penalties
keep their tokens, beside penalised ones and alone."""
import asyncio

import pytest
import torch

from hydrainfer_amd.engine import BatchSchedulerConfig, InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.engine.node import LocalCluster
from hydrainfer_amd.sampling import PenaltyHistory
from tests import penalty_ref as ref
from tests.engine_util import make_node, run_trace
from tests.golden import cases as C

pytestmark = pytest.mark.gpu

N_IMG_TOK = (C.TINY_CLIP["image_size"] // C.TINY_CLIP["patch_size"]) ** 2
BS = C.TINY_BLOCK_SIZE
DT = torch.float16
# (frequency, presence, repetition): a strong push away from what was generated, a pull towards it (a token that has
# appeared has its positive logit multiplied by 100: greedy decoding then repeats it), OpenAI-sized values
PENALTIES = {0: (1.0, 1.0, 100.0), 2: (0.0, 0.0, 0.01), 4: (1.5, -0.5, 1.0)}


class Tap:
    """Keeps the logits of every eager sampling step (on the host) with the requests of its rows: forward_logits of the
    model instance is wrapped, so forward / forward_logprobs / forward_penalized themselves run as they are."""

    def __init__(self, lm, fill=None):
        self.steps, self.current = [], None
        real = lm.forward_logits

        def forward_logits(*a):
            logits = real(*a)
            self.steps.append((logits.cpu(), self.current))
            return logits
        lm.forward_logits = forward_logits
        if fill is not None:
            self.watch(fill)

    def watch(self, fill):
        real = fill.execute

        def execute(batch):
            self.current = [rcb.request_id for rcb, inst in batch if inst.sample]
            real(batch)
        fill.execute = execute

    def rows_of(self, request_id, n):
        """the logits rows of a request's last n sampling steps (a chunk head's row is discarded like its sample)"""
        rows = []
        for logits, ids in self.steps:
            assert logits.shape[0] == len(ids)
            rows += [logits[j] for j, r in enumerate(ids) if r == request_id]
        return rows[-n:], len(rows)


def _models():
    from hydrainfer_amd.model.clip import ClipShape, LlavaVisionModel, random_state_dict
    from hydrainfer_amd.model.llama import LlamaForCausalLM, LlamaShape
    from hydrainfer_amd.model.llava import LlavaLanguageModel
    dev = torch.device("cuda:0")
    lshape, cshape = LlamaShape(**C.TINY_LLAMA), ClipShape(**C.TINY_CLIP)
    lm = LlavaLanguageModel(LlamaForCausalLM.from_reference_state_dict(lshape, C.tiny_llama_state_dict(DT), DT, dev),
                            image_token_id=C.TINY_IMAGE_TOKEN_ID)
    clip = {k: v.to(DT).to(dev) for k, v in random_state_dict(cshape, seed=3, std=0.05).items()}
    return lm, LlavaVisionModel(cshape, DT, dev, clip), lshape


def _cluster(chunked, graph_decode, budget=40):
    from hydrainfer_amd.memory.token_cache_manger import (TokenCacheBlockManager, TokenCacheBlockManagerConfig,
                                                          TokenCacheBlockManagerContext)
    lm, vision, lshape = _models()
    ctx = TokenCacheBlockManagerContext(rank=0, rank2host={0: "localhost"})
    kv = TokenCacheBlockManager(TokenCacheBlockManagerConfig(
        n_layers=lshape.num_hidden_layers, n_tokens=2, n_blocks=48, block_size=BS, n_heads=lshape.num_key_value_heads,
        head_size=lshape.head_dim, dtype="fp16", device="cuda:0"), ctx)
    img = TokenCacheBlockManager(TokenCacheBlockManagerConfig(
        n_layers=1, n_tokens=1, n_blocks=6, block_size=N_IMG_TOK, n_heads=lshape.num_attention_heads,
        head_size=lshape.head_dim, dtype="fp16", device="cuda:0"), ctx)
    cfg = BatchSchedulerConfig(priority="prefill", max_running_requests=6, chunked_prefill=chunked, token_budgets=budget,
                               image_budgets=2)
    node = make_node("EPD0", "EPD", lm, vision, kv, img, lshape, DT, torch.device("cuda:0"), cfg, graph_decode=graph_decode)
    return LocalCluster([node]), Tap(lm, node.executor.fill_executor)


def _creator():
    return InstructionCreator(image_token_id=C.TINY_IMAGE_TOKEN_ID, n_image_tokens_per_image=N_IMG_TOK, block_size=BS,
                              ignore_eos=True)


def _requests(penalties, text_len=(10, 45, 3, 28, 17, 33), max_tokens=(8, 3, 7, 4, 8, 2), eos=()):
    """penalties: {request: (frequency, presence, repetition)}.  Requests 0, 1, 2, 4, 5 carry an image, 3 is text only."""
    g = torch.Generator().manual_seed(4242)
    pixels = C.tiny_clip_pixels(2)
    out = []
    for i, (n, m) in enumerate(zip(text_len, max_tokens)):
        text = torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (n,), generator=g).tolist()
        has_image = i != 3
        sp = SamplingParameters(m, list(dict(eos).get(i, ())))
        if i in penalties:
            sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty = penalties[i]
        out.append((0 if i < 3 else 2, TokenRequest(
            request_id=i, token_ids=([C.TINY_IMAGE_TOKEN_ID] if has_image else []) + text,
            pixel_values=pixels[i % 2:i % 2 + 1].clone() if has_image else None, image_size=(56, 56),
            image_hash=9000 + i % 2, sampling_params=sp)))
    return out


def _check_tokens(request_id, tokens, penalties, tap):
    """every token = the restatement over the step's own logits and the tokens delivered before it"""
    rows, n_sampled = tap.rows_of(request_id, len(tokens))
    assert len(rows) == len(tokens), f"request {request_id}: {len(rows)} eager sampling steps for {len(tokens)} tokens"
    hist = PenaltyHistory()
    for s, (row, token) in enumerate(zip(rows, tokens)):
        want = ref.penalized_row(row, list(hist.ids), list(hist.counts), *penalties)[2]
        assert token == want, f"request {request_id} token {s}: {token}, the restatement gives {want} (history {list(hist.ids)})"
        if s == 0:
            assert token == int(torch.argmax(row.float())), "the first generated token sees an empty history"
        hist.append(token)
    return n_sampled


@pytest.mark.parametrize("graph_decode", [False, True], ids=["eager", "graphs"])
def test_mixed_batch(graph_decode):
    plain_cluster, plain_tap = _cluster(True, graph_decode)
    plain = run_trace(plain_cluster, _creator(), _requests({}))
    cluster, tap = _cluster(True, graph_decode)
    rcbs = run_trace(cluster, _creator(), _requests(PENALTIES))
    assert all(len(r.output_token_ids) == r.sampling_params.max_tokens for r in rcbs)
    for i, rcb in enumerate(rcbs):
        if i in PENALTIES:
            _check_tokens(i, rcb.output_token_ids, PENALTIES[i], tap)
            assert list(rcb.penalty_history.ids) == list(dict.fromkeys(rcb.output_token_ids))
            assert sum(rcb.penalty_history.counts) == len(rcb.output_token_ids)
        else:
            # beside penalised requests (an eager step with an empty history) as alone (graphs, cohort, argmax_rows)
            assert rcb.penalty_history is None and rcb.output_token_ids == plain[i].output_token_ids
    changed = [i for i in PENALTIES if rcbs[i].output_token_ids != plain[i].output_token_ids]
    print("tokens", {i: (plain[i].output_token_ids, rcbs[i].output_token_ids) for i in PENALTIES})
    assert changed, "no penalty changed a token: the run shows nothing"
    fill = cluster.nodes[0].executor.fill_executor
    assert fill.pending is None and fill.cohort is None
    if graph_decode:
        # no request penalised: the decode steps were launched from graphs, not through the eager step
        eager = run_trace(_cluster(True, False)[0], _creator(), _requests({}))
        assert [r.output_token_ids for r in eager] == [r.output_token_ids for r in plain]
        assert plain_cluster.nodes[0].executor.fill_executor.graph_decoder is not None
        assert len(plain_tap.steps) < len(tap.steps)


def test_logprobs_beside_penalties():
    """One request asks for log-probabilities, another is penalised (no request may do both): the batch's ids come from
    the penalised launch, the scores from hx_logprob_rows over the same logits."""
    from tests.logprob_ref import ATOL, reference
    plain = run_trace(_cluster(True, False)[0], _creator(), _requests({}))
    reqs = _requests({0: PENALTIES[0], 2: PENALTIES[2]})
    for i, k in ((1, 3), (4, 0)):
        reqs[i][1].sampling_params.logprobs, reqs[i][1].sampling_params.top_logprobs = True, k
    cluster, tap = _cluster(True, False)
    rcbs = run_trace(cluster, _creator(), reqs)
    for i in (0, 2):
        _check_tokens(i, rcbs[i].output_token_ids, PENALTIES[i], tap)
        assert rcbs[i].output_logprobs == []
    for i, k in ((1, 3), (4, 0)):
        assert rcbs[i].output_token_ids == plain[i].output_token_ids
        rows, _ = tap.rows_of(i, len(rcbs[i].output_token_ids))
        want = reference(torch.stack(rows), k)
        assert [rec.token_id for rec in rcbs[i].output_logprobs] == rcbs[i].output_token_ids == want[0].tolist()
        for s, rec in enumerate(rcbs[i].output_logprobs):
            assert abs(rec.logprob - float(want[1][s])) <= ATOL and [t for t, _ in rec.top] == want[2][s].tolist()
            assert all(abs(lp - float(w)) <= ATOL for (_, lp), w in zip(rec.top, want[3][s]))
    assert rcbs[3].output_token_ids == plain[3].output_token_ids and rcbs[5].output_token_ids == plain[5].output_token_ids


def test_chunked_prefill_and_eos():
    """token_budgets 16: the 45- and 33-token prompts are prefilled in chunks whose heads sample a token that is thrown
    away and never enters a history; the first token sees an empty history; an end-of-sequence id ends a penalised
    request as before."""
    pens = {1: (1.0, 0.5, 50.0), 2: (0.0, 0.0, 0.01), 5: (0.5, 0.5, 1.3)}
    cluster, tap = _cluster(True, False, budget=16)
    first = run_trace(cluster, _creator(), _requests(pens))
    plain = run_trace(_cluster(True, False, budget=16)[0], _creator(), _requests({}))
    sampled = {i: _check_tokens(i, first[i].output_token_ids, pens[i], tap) for i in pens}
    assert any(sampled[i] > len(first[i].output_token_ids) for i in (1, 5)), "no chunk head sampled"
    for i, rcb in enumerate(first):
        assert rcb.output_token_ids[0] == plain[i].output_token_ids[0]
        assert i in pens or rcb.output_token_ids == plain[i].output_token_ids
    # the same trace with request 2's third token as its end-of-sequence id
    eos = first[2].output_token_ids[2]
    cut = first[2].output_token_ids.index(eos) + 1
    again = run_trace(_cluster(True, False, budget=16)[0], _creator(), _requests(pens, eos={2: [eos]}))
    assert again[2].output_token_ids == first[2].output_token_ids[:cut] and cut <= 3
    assert sum(again[2].penalty_history.counts) == cut


def test_offline_engine_honours_the_fields():
    from hydrainfer_amd.engine.offline import OfflineInferenceEngine, OfflineRequest
    lm, vision, _ = _models()
    eng = OfflineInferenceEngine(lm, vision, DT, "cuda:0", max_running_requests=4, token_budgets=64, max_context=256,
                                 warm_up=False)
    tap = Tap(lm, eng.node.executor.fill_executor)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (6 + 5 * i,), generator=g).tolist() for i in range(4)]
    plain = eng.generate([OfflineRequest(p, None, max_tokens=6) for p in prompts])
    pens = {0: (2.0, 2.0, 1.0), 2: (0.0, 0.0, 0.01), 3: (0.0, 0.0, 100.0)}
    tap.steps.clear()
    got = eng.generate([OfflineRequest(p, None, max_tokens=6, frequency_penalty=pens.get(i, (0, 0, 1))[0],
                                       presence_penalty=pens.get(i, (0, 0, 1))[1],
                                       repetition_penalty=pens.get(i, (0, 0, 1))[2]) for i, p in enumerate(prompts)])
    assert got[1].output_token_ids == plain[1].output_token_ids
    for i in pens:
        _check_tokens(i, got[i].output_token_ids, pens[i], tap)
    assert any(got[i].output_token_ids != plain[i].output_token_ids for i in pens)
    for bad in (dict(repetition_penalty=0.0), dict(frequency_penalty=float("nan")), dict(presence_penalty=0.5, logprobs=True)):
        with pytest.raises(ValueError):
            eng.generate([OfflineRequest(prompts[0], None, max_tokens=2, **bad)])


def test_api_server_streams_a_penalised_request():
    import httpx
    from hydrainfer_amd.entrypoint import ApiServer, EngineFrontend, SyntheticTokenizer
    from hydrainfer_amd.entrypoint.api_protocol import parse_chat_completion_request as parse
    from hydrainfer_amd.model.processor import ClipImageProcessor
    from tests.test_api_server import _client_stream, _payload, _png
    creator = _creator

    def cluster():
        return _cluster(True, True)[0]
    tok = SyntheticTokenizer(image_token_id=C.TINY_IMAGE_TOKEN_ID, lo=3, hi=C.TINY_IMAGE_TOKEN_ID)
    front = EngineFrontend(cluster(), creator(), device=torch.device("cuda:0"))
    server = ApiServer(front, tok, ClipImageProcessor(size=56), host="127.0.0.1", port=0, image_size=(56, 56))
    extra = [dict(repetition_penalty=0.01), {}, dict(frequency_penalty=1.5, presence_penalty=-0.5, repetition_penalty=100.0)]
    jobs = [dict(_payload("What is shown in this image?", _png(1), 8), **extra[0]),
            dict(_payload("Describe the weather. Briefly.", None, 5), **extra[1]),
            dict(_payload("one two three four five six seven", _png(2), 8), **extra[2])]
    bad = [dict(_payload("hi", None, 2), frequency_penalty=2.5), dict(_payload("hi", None, 2), repetition_penalty=0),
           dict(_payload("hi", None, 2), presence_penalty="1"), dict(_payload("hi", None, 2), logprobs=True, presence_penalty=1)]

    async def go():
        await server.start()
        front.start()
        base = f"http://127.0.0.1:{server.port}/v1"
        try:
            streams = await asyncio.gather(*[_client_stream(base, p) for p in jobs])
            async with httpx.AsyncClient(timeout=None) as client:
                codes = [(await client.post(f"{base}/chat/completions", json=p)).status_code for p in bad]
            return streams, codes
        finally:
            front.stop()
            await server.close()
    streams, codes = asyncio.run(go())
    assert codes == [400] * len(bad)
    assert front.error is None and front.n_admitted == len(jobs)
    # each request run ALONE through a second identical engine, penalties in its SamplingParameters
    direct, n_same = cluster(), 0
    for payload, (text, n_events, done) in zip(jobs, streams):
        n = payload["max_tokens"]
        assert done and n_events == n + 1 and len(text.split()) == n
        req = server._token_request(parse(payload))
        sp = req.sampling_params
        assert (sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty) == (
            payload.get("frequency_penalty", 0.0), payload.get("presence_penalty", 0.0), payload.get("repetition_penalty", 1.0))
        rcb = run_trace(direct, creator(), [(0, req)])[0]
        n_same += int(text == "".join(tok.decode(t) for t in rcb.output_token_ids))
    # (a stream's tokens may depend on what shared its batches by a near-tie: the bar of test_gpu_api_server.py)
    assert n_same >= len(jobs) - 1, f"only {n_same} of {len(jobs)} streams equal the direct run's tokens"
    # the stream under repetition_penalty 0.01 differs from the same request without it
    plain = run_trace(direct, creator(), [(0, server._token_request(parse(_payload("What is shown in this image?", _png(1), 8))))])[0]
    assert streams[0][0] != "".join(tok.decode(t) for t in plain.output_token_ids)
