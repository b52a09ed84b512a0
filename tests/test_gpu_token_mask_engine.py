"""GPU: token masks through the engine (SamplingParameters.allowed_token_ids / guided_choice -> rcb.token_mask -> the eager
step's _sample_masked -> hx_sample_rows_masked) on the tiny model of tests/engine_util.py: a masked request emits only
what its mask allows, a guided_choice request exactly one of its choices and ends there, the requests beside them keep the
tokens of a run without masks, and a seeded masked request replays."""
import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd.sampling import TokenMask
from tests.golden import cases as C
from tests.test_gpu_penalties_engine import _cluster, _creator, _requests

pytestmark = pytest.mark.gpu

VOCAB = C.TINY_LLAMA["vocab_size"]
IMG = C.TINY_IMAGE_TOKEN_ID
PLAIN = {}


def _run(cluster, requests, max_steps=4000):
    """engine_util.run_trace with the vocabulary handed to the creator: a request's masks are as wide as the logits"""
    creator = _creator()
    rcbs = [None] * len(requests)
    last = max(a for a, _ in requests)
    step = 0
    while step <= last or not cluster.idle():
        for i, (a, r) in enumerate(requests):
            if a == step:
                rcbs[i] = creator.process(r, vocab_size=VOCAB)
                cluster.add_request(rcbs[i])
        cluster.step()
        step += 1
        assert step < max_steps, "engine did not drain"
    return rcbs


def _plain(graph_decode=False):
    """the six requests without masks, once per decode mode"""
    if graph_decode not in PLAIN:
        PLAIN[graph_decode] = [list(r.output_token_ids) for r in _run(_cluster(True, graph_decode)[0], _requests({}))]
    return PLAIN[graph_decode]


def _with(fields):
    reqs = _requests({})
    for i, f in fields.items():
        for k, v in f.items():
            setattr(reqs[i][1].sampling_params, k, v)
    return reqs


def _count_launches(monkeypatch):
    calls = []
    real = _lib.lib().hx_sample_rows_masked

    def counted(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(_lib.lib(), "hx_sample_rows_masked", counted)
    return calls


def test_allowed_token_ids_hold_every_step(monkeypatch):
    calls = _count_launches(monkeypatch)
    plain = _plain()
    assert not calls, "a run without masks never takes the masked launch"
    emitted = {t for tokens in plain for t in tokens}
    never = [t for t in range(3, IMG) if t not in emitted]
    allowed = {0: never[:5], 4: never[5:8] + [plain[4][0]]}
    rcbs = _run(_cluster(True, False)[0], _with({0: dict(allowed_token_ids=allowed[0]),
                                                4: dict(allowed_token_ids=allowed[4], temperature=1.0, seed=1234, top_k=3)}))
    for i in (0, 4):
        tokens = rcbs[i].output_token_ids
        assert isinstance(rcbs[i].token_mask, TokenMask) and not rcbs[i].token_mask.finished
        assert len(tokens) == rcbs[i].sampling_params.max_tokens and set(tokens) <= set(allowed[i]), (i, tokens, allowed[i])
    for i in (1, 2, 3, 5):      # greedy, unmasked, in the same batches: token for token what they get without the masks
        assert rcbs[i].token_mask is None and rcbs[i].output_token_ids == plain[i]
    assert calls


@pytest.mark.parametrize("graph_decode", [False, True], ids=["eager", "graphs"])
def test_guided_choice_emits_one_choice_and_ends(graph_decode):
    plain = _plain(graph_decode)
    emitted = {t for tokens in plain for t in tokens}
    a, b, c, d, e, f, g = [t for t in range(3, IMG) if t not in emitted][:7]
    choices = {0: [[a, b, c], [a, d], [e]], 4: [[f, g, a, b], [g, f], [b, c, d]]}
    fields = {0: dict(guided_choice=choices[0]), 4: dict(guided_choice=choices[4], temperature=1.0, seed=77)}
    runs = [_run(_cluster(True, graph_decode)[0], _with(fields)) for _ in range(2)]
    for rcbs in runs:
        for i in (0, 4):
            tokens, most = rcbs[i].output_token_ids, rcbs[i].sampling_params.max_tokens
            assert tokens in choices[i] and len(tokens) < most and rcbs[i].token_mask.finished, (i, tokens)
            assert len(rcbs[i].metric.token_times) == len(tokens)
        for i in (1, 2, 3, 5):
            assert rcbs[i].output_token_ids == plain[i]
    # the seeded, sampled request replays; so does everything else
    assert [r.output_token_ids for r in runs[0]] == [r.output_token_ids for r in runs[1]]


def test_max_tokens_truncates_a_choice():
    plain = _plain()
    a, b, c = [t for t in range(3, IMG) if t not in {t for tokens in plain for t in tokens}][:3]
    rcbs = _run(_cluster(True, False)[0], _with({3: dict(guided_choice=[[a, b, c, a, b, c]])}))      # request 3: max_tokens 4
    assert rcbs[3].output_token_ids == [a, b, c, a] and not rcbs[3].token_mask.finished
    for i in (0, 1, 2, 4, 5):
        assert rcbs[i].output_token_ids == plain[i]


def test_logprobs_beside_and_under_a_mask():
    """a processed-logprobs request under a mask is scored over its allowed set by the same launch; a raw-mode logprobs
    request in the same batches keeps its hx_logprob_rows scores (its batches are not row for row those of the run
    without masks, and the model's fp16 logits may differ in the last place with the batch's shape: the scores are held to
    1e-2, two units in the last place of an fp16 logit below 8, the ids exactly)"""
    import math
    plain = _plain()
    never = [t for t in range(3, IMG) if t not in {t for tokens in plain for t in tokens}]
    allowed = never[:3]
    raw = dict(logprobs=True, top_logprobs=2)
    alone = _run(_cluster(True, False)[0], _with({1: raw}))
    rcbs = _run(_cluster(True, False)[0], _with({0: dict(allowed_token_ids=allowed, logprobs=True, top_logprobs=3,
                                                         logprobs_mode="processed_logprobs"), 1: raw,
                                                 4: dict(guided_choice=[never[3:5], never[5:6]])}))
    entries = rcbs[0].output_logprobs
    assert len(entries) == len(rcbs[0].output_token_ids) == rcbs[0].sampling_params.max_tokens
    for e, token in zip(entries, rcbs[0].output_token_ids):
        assert e.token_id == token and token in allowed and math.isfinite(e.logprob) and e.logprob <= 0
        assert sorted(t for t, _ in e.top) == sorted(allowed), "the three most likely tokens of the masked row are the allowed ones"
        assert abs(sum(math.exp(lp) for _, lp in e.top) - 1.0) <= 1e-4 and e.top[0] == (token, e.logprob)      # (greedy)
    assert rcbs[4].output_token_ids in (never[3:5], never[5:6])
    assert rcbs[1].output_token_ids == alone[1].output_token_ids == plain[1]
    assert len(rcbs[1].output_logprobs) == len(alone[1].output_logprobs) == len(plain[1])
    for got, ref in zip(rcbs[1].output_logprobs, alone[1].output_logprobs):
        assert got.token_id == ref.token_id and [t for t, _ in got.top] == [t for t, _ in ref.top]
        assert got.logprob == pytest.approx(ref.logprob, abs=1e-2)
        assert [lp for _, lp in got.top] == pytest.approx([lp for _, lp in ref.top], abs=1e-2)
