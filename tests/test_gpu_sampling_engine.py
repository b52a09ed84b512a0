"""GPU: sampled decoding through the engine (SamplingParameters -> the eager step's forward_sampled -> hx_sample_rows) on
the tiny model of tests/engine_util.py.  Every delivered token of a sampled request is held against the logits of that
very step (kept by the wrapper round forward_logits of test_gpu_penalties_engine.py), the request's seed and its offset:
the same row through sample_rows alone gives the same token, and that token passes checks 2 and 3 of
tests/sampling_ref.py.  Greedy requests beside them keep the tokens of an all-greedy run."""
import numpy as np
import pytest
import torch

from hydrainfer_amd.engine import SamplingParameters, TokenRequest
from hydrainfer_amd.sampling import NO_PENALTIES, PenaltyHistory, pack_sample_step, sample_rows
from tests import sampling_ref as ref
from tests.engine_util import run_trace
from tests.golden import cases as C
from tests.test_gpu_penalties_engine import Tap, _cluster, _creator, _models, _requests

pytestmark = pytest.mark.gpu

# requests 1, 3 and 5 stay greedy; 2 has no seed (the engine assigns one); 4 is sampled AND penalised
SAMPLED = {0: dict(temperature=0.8, top_p=0.9, top_k=20, seed=(1 << 40) + 1),
           2: dict(temperature=1.3),
           4: dict(temperature=0.7, top_p=0.95, top_k=50, seed=77)}
PENALTIES = {4: (1.0, 0.5, 1.3)}


def _sampled_requests(sampled=SAMPLED, penalties=PENALTIES, **kw):
    reqs = _requests(penalties, **kw)
    for i, fields in sampled.items():
        for k, v in fields.items():
            setattr(reqs[i][1].sampling_params, k, v)
    return reqs


def _check_tokens(rcb, tap):
    """every token of a sampled request: what sample_rows gives for the step's own logits, the request's record and the
    tokens delivered before — and that launch's cut, u and token pass sampling_ref's checks"""
    sp, tokens = rcb.sampling_params, rcb.output_token_ids
    rows, n_sampled = tap.rows_of(rcb.request_id, len(tokens))
    assert len(rows) == len(tokens), f"request {rcb.request_id}: {len(rows)} eager sampling steps for {len(tokens)} tokens"
    pen = (sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty)
    hist = PenaltyHistory() if rcb.penalty_history is not None else None
    entries = []
    for s, token in enumerate(tokens):
        entries.append((PenaltyHistory(tokens[:s]) if hist is not None else None, pen if hist is not None else NO_PENALTIES,
                        (sp.temperature, sp.top_p, sp.top_k, sp.seed, s)))
    logits = torch.stack(rows).to("cuda:0")
    tables = pack_sample_step(entries).to_device("cuda:0")
    cut, u = (torch.empty(len(tokens), device="cuda:0") for _ in range(2))
    ids = sample_rows(logits, *tables, cut_out=cut, u_out=u).tolist()
    assert ids == tokens, f"request {rcb.request_id}: delivered {tokens}, the steps' logits give {ids}"
    for s, (h, p, rec) in enumerate(entries):
        kind = ref.check_row(rows[s], list(h.ids) if h else [], list(h.counts) if h else [], p, rec, tokens[s], float(cut[s]),
                             np.float32(u[s].item()), f"request {rcb.request_id} token {s}")
        assert kind == "sampled"
    return n_sampled


@pytest.mark.parametrize("graph_decode", [False, True], ids=["eager", "graphs"])
@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_mixed_batch(chunked, graph_decode):
    budget = 16 if chunked else 128
    plain = run_trace(_cluster(chunked, graph_decode, budget)[0], _creator(), _requests({}))
    cluster, tap = _cluster(chunked, graph_decode, budget)
    rcbs = run_trace(cluster, _creator(), _sampled_requests())
    assert all(len(r.output_token_ids) == r.sampling_params.max_tokens for r in rcbs)
    n_sampled = {}
    for i, rcb in enumerate(rcbs):
        if i in SAMPLED:
            n_sampled[i] = _check_tokens(rcb, tap)          # (every token came from an eager step: never a graph or the cohort)
        else:
            assert rcb.sampling_params.seed is None and rcb.output_token_ids == plain[i].output_token_ids
    if chunked:
        assert any(n_sampled[i] > len(rcbs[i].output_token_ids) for i in SAMPLED), "no chunk head sampled"
    assert isinstance(rcbs[2].sampling_params.seed, int) and 0 <= rcbs[2].sampling_params.seed < 1 << 63
    assert rcbs[0].sampling_params.seed == (1 << 40) + 1 and rcbs[4].sampling_params.seed == 77
    assert sum(rcbs[4].penalty_history.counts) == len(rcbs[4].output_token_ids)
    assert any(rcbs[i].output_token_ids != plain[i].output_token_ids for i in SAMPLED), "no draw left the greedy path"
    fill = cluster.nodes[0].executor.fill_executor
    assert fill.pending is None and fill.cohort is None
    # a request given a seed, run again (request 2 with the seed it was assigned): the same tokens
    again = dict(SAMPLED)
    again[2] = dict(SAMPLED[2], seed=rcbs[2].sampling_params.seed)
    second = run_trace(_cluster(chunked, graph_decode, budget)[0], _creator(), _sampled_requests(again))
    assert [r.output_token_ids for r in second] == [r.output_token_ids for r in rcbs]


def test_sampled_with_logprobs_raises_and_logprobs_ride_beside():
    with pytest.raises(ValueError, match="logprobs"):
        _creator().process(TokenRequest(request_id=1, token_ids=[5, 6, 7],
                                        sampling_params=SamplingParameters(4, [], True, 2, temperature=0.5)))
    # a greedy request that asks for log-probabilities beside a sampled one: its tokens and records as alone
    plain_reqs = _requests({})
    plain_reqs[1][1].sampling_params.logprobs, plain_reqs[1][1].sampling_params.top_logprobs = True, 3
    plain = run_trace(_cluster(True, False)[0], _creator(), plain_reqs)
    reqs = _sampled_requests()
    reqs[1][1].sampling_params.logprobs, reqs[1][1].sampling_params.top_logprobs = True, 3
    cluster, tap = _cluster(True, False)
    rcbs = run_trace(cluster, _creator(), reqs)
    for i in SAMPLED:
        _check_tokens(rcbs[i], tap)
        assert rcbs[i].output_logprobs == []
    assert rcbs[1].output_token_ids == plain[1].output_token_ids
    assert [rec.token_id for rec in rcbs[1].output_logprobs] == rcbs[1].output_token_ids
    assert all(len(rec.top) == 3 and rec.top[0][0] == rec.token_id for rec in rcbs[1].output_logprobs)


def test_offline_engine_honours_the_fields():
    from hydrainfer_amd.engine.offline import OfflineInferenceEngine, OfflineRequest
    lm, vision, _ = _models()
    eng = OfflineInferenceEngine(lm, vision, torch.float16, "cuda:0", max_running_requests=4, token_budgets=64, max_context=256,
                                 warm_up=False)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (6 + 5 * i,), generator=g).tolist() for i in range(3)]
    plain = eng.generate([OfflineRequest(p, None, max_tokens=6) for p in prompts])
    reqs = lambda: [OfflineRequest(prompts[0], None, max_tokens=6, temperature=1.2, seed=9),
                    OfflineRequest(prompts[1], None, max_tokens=6),
                    OfflineRequest(prompts[2], None, max_tokens=6, temperature=0.9, top_p=0.8, top_k=30, seed=(1 << 50) + 3)]
    got, again = eng.generate(reqs()), eng.generate(reqs())
    assert got[1].output_token_ids == plain[1].output_token_ids
    assert [r.output_token_ids for r in got] == [r.output_token_ids for r in again]
    assert any(got[i].output_token_ids != plain[i].output_token_ids for i in (0, 2))
    for bad in (dict(temperature=-1.0), dict(top_p=0.0), dict(top_k=-1), dict(seed=-5), dict(temperature=0.5, logprobs=True)):
        with pytest.raises(ValueError):
            eng.generate([OfflineRequest(prompts[0], None, max_tokens=2, **bad)])


def test_api_request_reaches_sampling_parameters():
    from hydrainfer_amd.entrypoint import ApiServer, SyntheticTokenizer
    from hydrainfer_amd.entrypoint.api_protocol import parse_chat_completion_request as parse
    from hydrainfer_amd.model.processor import ClipImageProcessor
    from tests.test_api_server import _payload, _png
    tok = SyntheticTokenizer(image_token_id=C.TINY_IMAGE_TOKEN_ID, lo=3, hi=C.TINY_IMAGE_TOKEN_ID)
    server = ApiServer(None, tok, ClipImageProcessor(size=56), host="127.0.0.1", port=0, image_size=(56, 56))
    payload = dict(_payload("What is shown in this image?", _png(1), 6), temperature=0.9, top_p=0.85, top_k=12, seed=(1 << 45) + 9)
    req = server._token_request(parse(payload))
    sp = req.sampling_params
    assert (sp.temperature, sp.top_p, sp.top_k, sp.seed) == (0.9, 0.85, 12, (1 << 45) + 9)
    sp = server._token_request(parse(_payload("hi there", None, 3))).sampling_params
    assert (sp.temperature, sp.top_p, sp.top_k, sp.seed) == (0.0, 1.0, 0, None)
    # and through the engine: the request is sampled, from an eager step, with that seed
    cluster, tap = _cluster(True, True)
    rcb = run_trace(cluster, _creator(), [(0, req)])[0]
    assert rcb.sampling_params.seed == (1 << 45) + 9 and len(rcb.output_token_ids) == 6
    _check_tokens(rcb, tap)
