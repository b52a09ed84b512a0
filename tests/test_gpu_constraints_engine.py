"""GPU: token constraints through the engine (SamplingParameters -> rcb.token_constraints -> the eager step's
forward_constrained -> hx_sample_rows_constrained) on the tiny model of tests/engine_util.py.  Every delivered token of a
constrained request is held against the logits of that very step (the Tap of test_gpu_penalties_engine.py): the same row
through sample_rows_constrained alone, with the request's record, history and THIS step's bias table, gives the same
token.  Requests beside them keep the tokens of a run without constraints."""
import asyncio
import re

import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, PenaltyHistory, TokenConstraints, pack_constrained_step,
                                     sample_rows_constrained)
from tests.engine_util import run_trace
from tests.golden import cases as C
from tests.test_gpu_penalties_engine import _cluster, _creator, _models, _requests

pytestmark = pytest.mark.gpu

VOCAB = C.TINY_LLAMA["vocab_size"]
IMG = C.TINY_IMAGE_TOKEN_ID
# a constraint moves a request off the tokens of the plain run, and the next-best token of this random model may be the image
# placeholder, which the engine cannot take back as a text token: the constrained requests below ban it too
NO_IMG = {IMG: -100}


def _with(fields, **kw):
    """the six requests of test_gpu_penalties_engine.py with `fields[i]` set on request i's sampling parameters"""
    reqs = _requests({}, **kw)
    for i, f in fields.items():
        for k, v in f.items():
            setattr(reqs[i][1].sampling_params, k, v)
    return reqs


def _relaunch(rcb, tap):
    """every token of a constrained request: what sample_rows_constrained gives for the step's own logits, the request's
    record, the tokens delivered before and the bias table of that step"""
    sp, tokens, tc = rcb.sampling_params, rcb.output_token_ids, rcb.token_constraints
    assert isinstance(tc, TokenConstraints)
    rows, n_sampled = tap.rows_of(rcb.request_id, len(tokens))
    assert len(rows) == len(tokens), f"request {rcb.request_id}: {len(rows)} eager sampling steps for {len(tokens)} tokens"
    pen = (sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty)
    entries = []
    for s in range(len(tokens)):
        rec = (sp.temperature, sp.top_p, sp.top_k, sp.seed, s, sp.min_p) if sp.temperature > 0 else GREEDY_RECORD
        entries.append((PenaltyHistory(tokens[:s]) if rcb.penalty_history is not None else None,
                        pen if rcb.penalty_history is not None else NO_PENALTIES, rec, tc.step_entries(s)))
    ids = sample_rows_constrained(torch.stack(rows).to("cuda:0"), *pack_constrained_step(entries).to_device("cuda:0")).tolist()
    assert ids == tokens, f"request {rcb.request_id}: delivered {tokens}, the steps' logits give {ids}"
    return n_sampled


def _count_launches(monkeypatch):
    """counts every hx_sample_rows_constrained call, whichever Python path makes it"""
    calls = []
    real = _lib.lib().hx_sample_rows_constrained

    def counted(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(_lib.lib(), "hx_sample_rows_constrained", counted)
    return calls


def test_logit_bias_pushes_and_bans():
    plain = run_trace(_cluster(True, False)[0], _creator(), _requests({}))
    emitted = {t for r in plain for t in r.output_token_ids}
    t = next(v for v in range(3, VOCAB - 1) if v not in emitted)
    first = plain[3].output_token_ids[0]
    cluster, tap = _cluster(True, False)
    rcbs = run_trace(cluster, _creator(), _with({0: dict(logit_bias={t: 100}), 3: dict(logit_bias={first: -100, **NO_IMG})}))
    # +100 on a token the plain run never emits: every generated token is that one
    assert rcbs[0].output_token_ids == [t] * rcbs[0].sampling_params.max_tokens
    # -100 on the plain run's first token: another one, the one the constrained launch gives for that step's logits
    assert rcbs[3].output_token_ids[0] != first and len(rcbs[3].output_token_ids) == rcbs[3].sampling_params.max_tokens
    assert first not in rcbs[3].output_token_ids
    for i in (0, 3):
        _relaunch(rcbs[i], tap)
    for i in (1, 2, 4, 5):
        assert rcbs[i].token_constraints is None and rcbs[i].output_token_ids == plain[i].output_token_ids


def test_min_tokens_holds_the_end_back():
    plain = run_trace(_cluster(True, False)[0], _creator(), _requests({}))
    eos = {i: [plain[i].output_token_ids[0]] for i in (0, 4)}
    stopped = run_trace(_cluster(True, False)[0], _creator(), _requests({}, eos=eos))
    assert all(stopped[i].output_token_ids == eos[i] for i in (0, 4)), "the plain run ends on its first token"
    cluster, tap = _cluster(True, False)
    rcbs = run_trace(cluster, _creator(), _with({0: dict(min_tokens=3, logit_bias=NO_IMG), 4: dict(min_tokens=8, logit_bias=NO_IMG)}, eos=eos))
    for i, min_tokens in ((0, 3), (4, 8)):
        tokens, stop, most = rcbs[i].output_token_ids, eos[i][0], rcbs[i].sampling_params.max_tokens
        assert min_tokens <= len(tokens) <= most and stop not in tokens[:min_tokens]
        later = [s for s, t in enumerate(tokens) if t == stop]
        assert len(tokens) == (later[0] + 1 if later else most), (tokens, stop)
        _relaunch(rcbs[i], tap)
    for i in (1, 2, 3, 5):
        assert rcbs[i].output_token_ids == plain[i].output_token_ids


@pytest.mark.parametrize("graph_decode", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_mixed_batch(chunked, graph_decode, monkeypatch):
    """0: constrained and greedy; 1: asks for logprobs; 2: sampled, unconstrained; 3, 5: plain; 4: constrained, sampled
    with a seed, penalised"""
    from tests.logprob_ref import ATOL
    calls = _count_launches(monkeypatch)
    budget = 16 if chunked else 128
    plain = run_trace(_cluster(chunked, graph_decode, budget)[0], _creator(), _requests({}))
    emitted = {t for r in plain for t in r.output_token_ids}
    push = [v for v in range(3, VOCAB - 1) if v not in emitted][:2]
    common = {1: dict(logprobs=True, top_logprobs=3), 2: dict(temperature=0.9, top_p=0.9, top_k=40, seed=(1 << 41) + 5),
              4: dict(temperature=0.8, top_p=0.95, top_k=50, seed=77, frequency_penalty=1.0, presence_penalty=0.5,
                      repetition_penalty=1.3)}
    base = run_trace(_cluster(chunked, graph_decode, budget)[0], _creator(), _with(common))
    assert calls == [], "a batch with no constrained request made the constrained launch"
    # request 0: its first plain token is banned for good, and its second is an end-of-sequence id held back to the end
    ban, stop = plain[0].output_token_ids[0], plain[0].output_token_ids[1]
    constrained = dict(common)
    constrained[0] = dict(logit_bias={ban: -100, push[0]: 2.5, **NO_IMG}, min_tokens=8, eos_token_ids=[stop])
    constrained[4] = dict(common[4], logit_bias={push[1]: 4.0, base[4].output_token_ids[0]: -100, **NO_IMG}, min_p=0.05)
    cluster, tap = _cluster(chunked, graph_decode, budget)
    rcbs = run_trace(cluster, _creator(), _with(constrained))
    assert len(calls) > 0
    assert all(len(r.output_token_ids) == r.sampling_params.max_tokens for r in rcbs)
    n_sampled = {i: _relaunch(rcbs[i], tap) for i in (0, 4)}     # (every token came from an eager step: never a graph or the cohort)
    if chunked:
        assert any(n_sampled[i] > len(rcbs[i].output_token_ids) for i in (0, 4)), "no chunk head sampled"
    assert ban not in rcbs[0].output_token_ids and stop not in rcbs[0].output_token_ids
    assert base[4].output_token_ids[0] != rcbs[4].output_token_ids[0]
    assert sum(rcbs[4].penalty_history.counts) == len(rcbs[4].output_token_ids)
    # the others as in the run without constraints: tokens, and the records of the one that asked
    for i in (1, 2, 3, 5):
        assert rcbs[i].token_constraints is None and rcbs[i].output_token_ids == base[i].output_token_ids
    assert [rec.token_id for rec in rcbs[1].output_logprobs] == rcbs[1].output_token_ids
    for got, want in zip(rcbs[1].output_logprobs, base[1].output_logprobs):
        assert abs(got.logprob - want.logprob) <= ATOL and [t for t, _ in got.top] == [t for t, _ in want.top]
    assert rcbs[0].output_logprobs == [] and rcbs[4].output_logprobs == []
    fill = cluster.nodes[0].executor.fill_executor
    assert fill.pending is None and fill.cohort is None
    # the seeded run again: the same tokens
    second = run_trace(_cluster(chunked, graph_decode, budget)[0], _creator(), _with(constrained))
    assert [r.output_token_ids for r in second] == [r.output_token_ids for r in rcbs]


def test_prompt_logprobs_stay_combinable():
    """a constrained request that also scores its prompt (the scoring step picks the constrained launch too): the same
    tokens as without the scores, and the scores of the raw logits"""
    plain = run_trace(_cluster(True, False)[0], _creator(), _requests({}))
    fields = {3: dict(logit_bias={plain[3].output_token_ids[0]: -100, **NO_IMG}, temperature=0.7, seed=5, min_p=0.1),
              0: dict(logit_bias={plain[0].output_token_ids[0]: -100, **NO_IMG})}
    alone = run_trace(_cluster(True, False)[0], _creator(), _with(fields))
    scored = run_trace(_cluster(True, False)[0], _creator(),
                       _with({i: dict(f, prompt_logprobs=1) for i, f in fields.items()}))
    want = run_trace(_cluster(True, False)[0], _creator(), _with({3: dict(prompt_logprobs=1), 0: dict(prompt_logprobs=1)}))
    for i in range(6):
        assert scored[i].output_token_ids == alone[i].output_token_ids
    for i in (0, 3):
        assert scored[i].output_token_ids[0] != plain[i].output_token_ids[0]
        got, ref_scores = scored[i].prompt_logprobs, want[i].prompt_logprobs
        assert len(got) == len(ref_scores) and any(e is not None for e in got)
        assert [None if e is None else (e.token_id, e.rank) for e in got] == [None if e is None else (e.token_id, e.rank) for e in ref_scores]


def test_offline_engine_honours_the_fields():
    from hydrainfer_amd.engine.offline import OfflineInferenceEngine, OfflineRequest
    lm, vision, _ = _models()
    eng = OfflineInferenceEngine(lm, vision, torch.float16, "cuda:0", max_running_requests=4, token_budgets=64, max_context=256,
                                 warm_up=False)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (6 + 5 * i,), generator=g).tolist() for i in range(3)]
    plain = eng.generate([OfflineRequest(p, None, max_tokens=6) for p in prompts])
    emitted = {t for r in plain for t in r.output_token_ids}
    t = next(v for v in range(3, VOCAB - 1) if v not in emitted)
    stop = plain[2].output_token_ids[0]
    reqs = lambda: [OfflineRequest(prompts[0], None, max_tokens=6, logit_bias={t: 100}),
                    OfflineRequest(prompts[1], None, max_tokens=6),
                    OfflineRequest(prompts[2], None, max_tokens=6, eos_token_ids=[stop], min_tokens=4, temperature=0.9, seed=3,
                                   min_p=0.2, logit_bias=NO_IMG)]
    got, again = eng.generate(reqs()), eng.generate(reqs())
    assert got[0].output_token_ids == [t] * 6 and got[1].output_token_ids == plain[1].output_token_ids
    assert len(got[2].output_token_ids) >= 4 and stop not in got[2].output_token_ids[:4]
    assert [r.output_token_ids for r in got] == [r.output_token_ids for r in again]
    assert eng.generate([OfflineRequest(prompts[2], None, max_tokens=6, eos_token_ids=[stop])])[0].output_token_ids == [stop]
    for bad in (dict(logit_bias={-1: 1.0}), dict(logit_bias={VOCAB: 1.0}), dict(logit_bias={5: 101.0}), dict(min_tokens=-1),
                dict(min_tokens=3), dict(min_p=1.5), dict(logit_bias={5: 1.0}, logprobs=True), dict(min_p=0.5, logprobs=True)):
        with pytest.raises(ValueError):
            eng.generate([OfflineRequest(prompts[0], None, max_tokens=2, **bad)])


def test_api_server_streams_a_constrained_request():
    import httpx
    from hydrainfer_amd.entrypoint import ApiServer, EngineFrontend, SyntheticTokenizer
    from hydrainfer_amd.entrypoint.api_protocol import parse_chat_completion_request as parse
    from hydrainfer_amd.model.processor import ClipImageProcessor
    from tests.test_api_server import _client_stream, _payload
    tok = SyntheticTokenizer(image_token_id=C.TINY_IMAGE_TOKEN_ID, lo=3, hi=C.TINY_IMAGE_TOKEN_ID)
    assert tok.vocab_size == VOCAB
    front = EngineFrontend(_cluster(True, True)[0], _creator(), device=torch.device("cuda:0"))
    server = ApiServer(front, tok, ClipImageProcessor(size=56), host="127.0.0.1", port=0, image_size=(56, 56))
    assert front.vocab_size == VOCAB
    text = "Describe the weather. Briefly."
    direct = _cluster(True, True)[0]
    plain = run_trace(direct, _creator(), [(0, server._token_request(parse(_payload(text, None, 6))))])[0].output_token_ids
    stop, second = plain[0], plain[1]
    jobs = [dict(_payload(text, None, 6), stop_token_ids=[stop]),                                    # ends on its first token
            dict(_payload(text, None, 6), stop_token_ids=[stop], min_tokens=3, logit_bias={str(second): -100, str(IMG): -100})]
    bad = [dict(_payload("hi", None, 2), logit_bias={"abc": 1}), dict(_payload("hi", None, 2), logit_bias={"5": 101}),
           dict(_payload("hi", None, 2), logit_bias={str(VOCAB): 1}), dict(_payload("hi", None, 2), min_p=1.5),
           dict(_payload("hi", None, 2), stop_token_ids=[-1]), dict(_payload("hi", None, 2), logprobs=True, min_tokens=1)]

    async def go():
        await server.start()
        front.start()
        base = f"http://127.0.0.1:{server.port}/v1"
        try:
            streams = [await _client_stream(base, p) for p in jobs]          # one at a time: each stream's batches as the direct run's
            async with httpx.AsyncClient(timeout=None) as client:
                codes = [(await client.post(f"{base}/chat/completions", json=p)).status_code for p in bad]
            return streams, codes
        finally:
            front.stop()
            await server.close()
    streams, codes = asyncio.run(go())
    assert codes == [400] * len(bad)
    assert front.error is None and front.n_admitted == len(jobs)
    ids = [[int(v) for v in re.findall(r"<(\d+)>", body)] for body, _, done in streams]
    assert all(done for _, _, done in streams)
    assert ids[0] == [stop]
    req = server._token_request(parse(jobs[1]))
    sp = req.sampling_params
    assert (sp.eos_token_ids, sp.min_tokens, sp.logit_bias, sp.min_p) == ([stop], 3, {second: -100.0, IMG: -100.0}, 0.0)
    want = run_trace(direct, _creator(), [(0, req)])[0].output_token_ids
    assert ids[1] == want, f"the stream gave {ids[1]}, the direct run {want}"
    assert 3 <= len(want) <= 6 and stop not in want[:3] and second not in want
    later = [s for s, t in enumerate(want) if t == stop]
    assert len(want) == (later[0] + 1 if later else 6)
