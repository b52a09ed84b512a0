"""GPU: processed log-probabilities through the engine (SamplingParameters.logprobs_mode = "processed_logprobs" -> the eager
step's scored_rows -> forward_scored -> hx_sample_rows_logprobs -> rcb.output_logprobs) on the tiny model of
tests/engine_util.py.  Asking for them changes no token; every TokenLogprob is held to the float64 reference of
tests/sample_logprob_ref.py over the logits of that very step (the Tap of test_gpu_penalties_engine.py), the request's
record, the tokens delivered before and that step's bias table, with the kept set taken from hx_sample_rows_constrained's
cut; a raw-mode request beside them keeps its hx_logprob_rows scores bit for bit."""
import asyncio
import json
import math
import re

import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, PenaltyHistory, pack_constrained_step,
                                     sample_rows_constrained)
from tests import sample_logprob_ref as sref
from tests.engine_util import run_trace
from tests.golden import cases as C
from tests.logprob_ref import ATOL
from tests.test_gpu_constraints_engine import IMG, NO_IMG, VOCAB, _with
from tests.test_gpu_penalties_engine import _cluster, _creator, _models

pytestmark = pytest.mark.gpu

PROCESSED = "processed_logprobs"
# 0: greedy under penalties; 1: RAW-mode logprobs; 2: sampled with a seed; 3: plain; 4: all three families at once;
# 5: sampled, no logprobs.  (A request that leaves the plain run's tokens bans the image placeholder, which the engine
# cannot take back as a text token — test_gpu_constraints_engine.py.)
FIELDS = {0: dict(frequency_penalty=1.0, presence_penalty=1.0, repetition_penalty=100.0),
          1: dict(logprobs=True, top_logprobs=3),
          2: dict(temperature=0.9, top_p=0.9, top_k=40, seed=(1 << 41) + 5),
          4: dict(temperature=0.8, top_p=0.95, top_k=50, seed=77, frequency_penalty=1.0, presence_penalty=0.5,
                  repetition_penalty=1.3, logit_bias={11: 4.0, **NO_IMG}, min_p=0.05, min_tokens=3, eos_token_ids=[13]),
          5: dict(temperature=0.7, top_k=30, seed=9, logit_bias=NO_IMG)}
ASK = {0: 2, 2: 3, 4: 5}          # the processed requests and their top_logprobs


def _asking(fields=FIELDS, ask=ASK):
    return {i: dict(f, **(dict(logprobs=True, top_logprobs=ask[i], logprobs_mode=PROCESSED) if i in ask else {}))
            for i, f in fields.items()}


def _count(monkeypatch, name):
    calls = []
    real = getattr(_lib.lib(), name)

    def counted(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(_lib.lib(), name, counted)
    return calls


def _check_scores(rcb, tap):
    """every TokenLogprob of a processed request against the float64 reference for that step; returns the largest error"""
    sp, tokens, tc = rcb.sampling_params, rcb.output_token_ids, rcb.token_constraints
    rows, _ = tap.rows_of(rcb.request_id, len(tokens))
    assert len(rows) == len(tokens) == len(rcb.output_logprobs), f"request {rcb.request_id}"
    pen = (sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty) if rcb.penalty_history is not None else NO_PENALTIES
    entries = []
    for s in range(len(tokens)):
        rec = (sp.temperature, sp.top_p, sp.top_k, sp.seed, s, sp.min_p) if sp.temperature > 0 else GREEDY_RECORD
        entries.append((PenaltyHistory(tokens[:s]) if rcb.penalty_history is not None else None, pen, rec,
                        tc.step_entries(s) if tc is not None else None))
    cut = torch.empty(len(tokens), device="cuda:0")
    ids = sample_rows_constrained(torch.stack(rows).to("cuda:0"), *pack_constrained_step(entries).to_device("cuda:0"), cut_out=cut)
    assert ids.tolist() == tokens, f"request {rcb.request_id}: delivered {tokens}, the existing kernel gives {ids.tolist()}"
    worst = 0.0
    for s, (entry, (hist, p, rec, bias)) in enumerate(zip(rcb.output_logprobs, entries)):
        z = sref.row_z(rows[s], bias, hist, p, rec)
        lp, top_ids, top_lp = sref.reference_logprobs(z, float(cut[s]) if rec[0] > 0 else None, sp.top_logprobs)
        what = f"request {rcb.request_id} token {s}"
        assert entry.token_id == tokens[s] and len(entry.top) == sp.top_logprobs, what
        assert math.isfinite(entry.logprob) and abs(entry.logprob - lp[tokens[s]]) <= ATOL, (what, entry.logprob, lp[tokens[s]])
        assert [t for t, _ in entry.top] == top_ids.tolist(), what
        for (_, got), want in zip(entry.top, top_lp.tolist()):
            assert got == want if want == -math.inf else abs(got - want) <= ATOL, (what, entry.top, top_lp)
        worst = max([worst, abs(entry.logprob - lp[tokens[s]])] + [abs(g - w) for (_, g), w in zip(entry.top, top_lp.tolist()) if w != -math.inf])
    return worst


@pytest.mark.parametrize("graph_decode", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_mixed_batch_tokens_and_scores(chunked, graph_decode, monkeypatch):
    scored = _count(monkeypatch, "hx_sample_rows_logprobs")
    budget = 16 if chunked else 128
    base = run_trace(_cluster(chunked, graph_decode, budget)[0], _creator(), _with(FIELDS))
    assert scored == [], "a batch without a processed request made the scored launch"
    cluster, tap = _cluster(chunked, graph_decode, budget)
    rcbs = run_trace(cluster, _creator(), _with(_asking()))
    assert len(scored) > 0
    # the same tokens as without the scores, for the three that ask and for the three beside them
    assert [r.output_token_ids for r in rcbs] == [r.output_token_ids for r in base]
    assert all(len(r.output_token_ids) >= 2 for r in rcbs)
    worst = max(_check_scores(rcbs[i], tap) for i in ASK)
    print(f"largest |TokenLogprob - float64 reference| over the processed requests: {worst:.3e}")
    # the raw-mode request: hx_logprob_rows over the raw logits, bit for bit what it got without the processed ones beside
    assert [(e.token_id, e.logprob, e.top) for e in rcbs[1].output_logprobs] == \
        [(e.token_id, e.logprob, e.top) for e in base[1].output_logprobs] and len(base[1].output_logprobs) == len(base[1].output_token_ids)
    assert rcbs[3].output_logprobs == [] and rcbs[5].output_logprobs == []
    fill = cluster.nodes[0].executor.fill_executor
    assert fill.pending is None and fill.cohort is None
    # the seeded run again: the same tokens and the same scores
    second = run_trace(_cluster(chunked, graph_decode, budget)[0], _creator(), _with(_asking()))
    assert [(r.output_token_ids, r.output_logprobs) for r in second] == [(r.output_token_ids, r.output_logprobs) for r in rcbs]


@pytest.mark.parametrize("i", sorted(ASK), ids=["penalised", "sampled", "all"])
def test_each_family_alone_and_with_prompt_logprobs(i):
    """one processed request beside plain ones (a step with no raw-mode request is ONE launch: forward_scored);
    prompt_logprobs stays raw and combinable"""
    base = run_trace(_cluster(True, False)[0], _creator(), _with({i: FIELDS[i]}))
    cluster, tap = _cluster(True, False)
    alone = run_trace(cluster, _creator(), _with({i: _asking()[i]}))
    assert [r.output_token_ids for r in alone] == [r.output_token_ids for r in base]
    _check_scores(alone[i], tap)
    # with the prompt scored too (the step's logits are then the scoring forward's: no Tap): the same tokens, a score each
    rcbs = run_trace(_cluster(True, False)[0], _creator(), _with({i: dict(_asking()[i], prompt_logprobs=1)}))
    assert [r.output_token_ids for r in rcbs] == [r.output_token_ids for r in base]
    assert [e.token_id for e in rcbs[i].output_logprobs] == rcbs[i].output_token_ids
    for e in rcbs[i].output_logprobs:
        assert math.isfinite(e.logprob) and len(e.top) == ASK[i] and all(lp == e.logprob for t, lp in e.top if t == e.token_id)
    want = run_trace(_cluster(True, False)[0], _creator(), _with({i: dict(prompt_logprobs=1)}))[i].prompt_logprobs
    got = rcbs[i].prompt_logprobs
    assert len(got) == len(want) and any(e is not None for e in got)
    assert [None if e is None else (e.token_id, e.rank) for e in got] == [None if e is None else (e.token_id, e.rank) for e in want]


def test_offline_engine_and_the_refusals_without_the_field():
    from hydrainfer_amd.engine.offline import OfflineInferenceEngine, OfflineRequest
    lm, vision, _ = _models()
    eng = OfflineInferenceEngine(lm, vision, torch.float16, "cuda:0", max_running_requests=4, token_budgets=64, max_context=256,
                                 warm_up=False)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (6 + 5 * i,), generator=g).tolist() for i in range(3)]
    kw = [dict(temperature=0.9, top_k=20, seed=3, logit_bias=NO_IMG), dict(), dict(repetition_penalty=1.5, frequency_penalty=0.5)]
    reqs = lambda ask: [OfflineRequest(p, None, max_tokens=5, **k,
                                       **(dict(logprobs=True, top_logprobs=2 + i, logprobs_mode=PROCESSED) if ask else {}))
                        for i, (p, k) in enumerate(zip(prompts, kw))]
    plain, got = eng.generate(reqs(False)), eng.generate(reqs(True))
    assert [r.output_token_ids for r in got] == [r.output_token_ids for r in plain]
    for i, r in enumerate(got):
        assert [e.token_id for e in r.output_logprobs] == r.output_token_ids and all(len(e.top) == 2 + i for e in r.output_logprobs)
        assert all(math.isfinite(e.logprob) and e.logprob <= 0 for e in r.output_logprobs)
        # the chosen token is in the kept set: where it is among the alternatives, with the same score
        for e in r.output_logprobs:
            assert all(lp == e.logprob for t, lp in e.top if t == e.token_id)
    # greedy and unadjusted: the most likely alternative IS the token
    assert all(e.top[0] == (e.token_id, e.logprob) for e in got[1].output_logprobs)
    # the old refusals still fire without the field, and with "raw_logprobs"
    for mode in (None, "raw_logprobs"):
        for bad in (dict(temperature=0.5), dict(frequency_penalty=0.5), dict(logit_bias={5: 1.0}), dict(min_p=0.5, temperature=1.0)):
            with pytest.raises(ValueError, match="logprobs"):
                eng.generate([OfflineRequest(prompts[0], None, max_tokens=2, logprobs=True, logprobs_mode=mode, **bad)])
    for bad in (dict(logprobs_mode=PROCESSED), dict(logprobs=True, logprobs_mode="processed")):
        with pytest.raises(ValueError, match="logprobs_mode"):
            eng.generate([OfflineRequest(prompts[0], None, max_tokens=2, **bad)])


def test_api_server_streams_processed_logprobs():
    import httpx
    from hydrainfer_amd.entrypoint import ApiServer, EngineFrontend, SyntheticTokenizer
    from hydrainfer_amd.entrypoint.api_protocol import parse_chat_completion_request as parse
    from hydrainfer_amd.model.processor import ClipImageProcessor
    from tests.test_api_server import _payload
    tok = SyntheticTokenizer(image_token_id=C.TINY_IMAGE_TOKEN_ID, lo=3, hi=C.TINY_IMAGE_TOKEN_ID)
    front = EngineFrontend(_cluster(True, True)[0], _creator(), device=torch.device("cuda:0"))
    server = ApiServer(front, tok, ClipImageProcessor(size=56), host="127.0.0.1", port=0, image_size=(56, 56))
    text = "Describe the weather. Briefly."
    job = dict(_payload(text, None, 5), temperature=0.8, top_k=4, seed=11, logprobs=True, top_logprobs=6,
               logprobs_mode=PROCESSED, logit_bias={str(IMG): -100})
    bad = [dict(job, logprobs_mode="processed"), {k: v for k, v in job.items() if k != "logprobs_mode"},
           dict(job, logprobs_mode="raw_logprobs"), dict(job, logprobs=False, top_logprobs=0)]

    async def go():
        await server.start()
        front.start()
        base = f"http://127.0.0.1:{server.port}/v1"
        chunks = []
        try:
            async with httpx.AsyncClient(timeout=None) as client:
                async with client.stream("POST", f"{base}/chat/completions", json=job) as response:
                    assert response.status_code == 200
                    async for line in response.aiter_lines():
                        if line.startswith("data: ") and line.strip() != "data: [DONE]":
                            chunks.append(json.loads(line[len("data: "):]))
                codes = [(await client.post(f"{base}/chat/completions", json=p)).status_code for p in bad]
            return chunks, codes
        finally:
            front.stop()
            await server.close()
    chunks, codes = asyncio.run(go())
    assert codes == [400] * len(bad) and front.error is None
    scored = [c["choices"][0] for c in chunks if c["choices"][0].get("logprobs")]
    want = run_trace(_cluster(True, True)[0], _creator(), [(0, server._token_request(parse(job)))])[0]
    assert len(scored) == len(want.output_token_ids) == 5
    for choice, token, entry in zip(scored, want.output_token_ids, want.output_logprobs):
        (item,) = choice["logprobs"]["content"]
        assert [int(v) for v in re.findall(r"<(\d+)>", item["token"])] == [token] and item["logprob"] == entry.logprob
        tops = item["top_logprobs"]
        assert len(tops) == 6 and [int(re.findall(r"<(\d+)>", t["token"])[0]) for t in tops] == [t for t, _ in entry.top]
        # top_k = 4 keeps four tokens (more on a tie at the cut): the alternatives it dropped are listed with null
        assert [t["logprob"] for t in tops] == [lp if math.isfinite(lp) else None for _, lp in entry.top]
        assert all(t["logprob"] is not None for t in tops[:4])
    assert any(t["logprob"] is None for c in scored for t in c["logprobs"]["content"][0]["top_logprobs"])
