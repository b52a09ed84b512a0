"""GPU: penalties from the captured step through the engine (the graph_penalties switch: GraphedDecoder(sampled=True,
penalized=True) behind BatchFillExecutor), on the cluster and the Watch of tests/test_gpu_graph_sampling_engine.py.  Six
requests of 12 tokens: 0 penalised and sampled with a seed, 1 penalised and greedy, 2 sampled without penalties, 3-5
greedy.  With the switch on, once the prefill steps are over no eager sampling step runs: the penalised requests decode
from the penalised variant of the graph and from the cohort, their tokens live in the resident token log, and the host's
table of them (rcb.penalty_history) keeps up.  A request that asks for logprobs sends the steps back to the eager path for
as long as it lives; afterwards the penalised requests are seeded again and go on from the graph."""
from collections import Counter

import pytest

from hydrainfer_amd.engine.graph_decode import GraphedDecoder
from tests.engine_util import run_trace
from tests.test_gpu_graph_sampling_engine import Watch, requests
from tests.test_gpu_graph_sampling_engine import run as run_sampled_only
from tests.test_gpu_penalties_engine import _cluster, _creator

pytestmark = pytest.mark.gpu

SAMPLED = {0: dict(temperature=0.8, seed=(1 << 40) + 1), 2: dict(temperature=1.3)}
PENALTIES = {0: (0.4, 0.3, 1.2), 1: (0.7, 0.5, 1.3)}
MAX_TOKENS = (12, 12, 12, 12, 12, 12)
LOG_CAP = 64


def run(reqs, monkeypatch, switch=True):
    """-> (rcbs, watch, fill, {launch id: (variant, the step it was made in)})"""
    cluster, _ = _cluster(False, True, 128)
    fill = cluster.nodes[0].executor.fill_executor
    old = fill.graph_decoder
    variants, made = {}, []
    if switch:
        dec = fill.graph_decoder = GraphedDecoder(old.lm, old.kv, max_batch=old.max_batch, max_blocks_per_seq=old.cap,
                                                  sampled=True, penalized=True, penalty_log_cap=LOG_CAP, keep_draws=True)
        assert dec.sampled and dec.penalized
        real_replay = dec._replay

        def replay(n, B, kv_max, variant):
            launch = real_replay(n, B, kv_max, variant)
            variants[launch] = (variant, made[0].step)
            return launch
        dec._replay = replay
    watch = Watch(old.lm, fill, monkeypatch)
    made.append(watch)
    rcbs = run_trace(cluster, _creator(), reqs)
    assert fill.pending is None and fill.cohort is None
    return rcbs, watch, fill, variants


def check_logs(rcbs, dec, max_tokens):
    """the host's table is the multiset of the delivered tokens; a live slot's log prefix is the request's tokens"""
    for i in PENALTIES:
        out, hist = rcbs[i].output_token_ids, rcbs[i].penalty_history
        assert len(out) == max_tokens[i] and all(isinstance(t, int) for t in out)
        assert Counter(out) == dict(zip(hist.ids, hist.counts)), f"request {i}: the host's history fell behind"
        slot = dec.log_table.slot_of[rcbs[i].sid][0]
        assert dec.token_log[slot, :len(out)].tolist() == out, f"request {i}: the token log"


def test_penalised_requests_decode_from_the_graph(monkeypatch):
    eager = run(requests(SAMPLED, PENALTIES, MAX_TOKENS), monkeypatch, switch=False)[0]
    rcbs, watch, fill, variants = run(requests(SAMPLED, PENALTIES, MAX_TOKENS), monkeypatch)
    dec = fill.graph_decoder
    assert all(len(r.output_token_ids) == m for r, m in zip(rcbs, MAX_TOKENS))
    assert all(r.penalty_history is not None for r in (rcbs[0], rcbs[1])) and rcbs[2].penalty_history is None
    # after the prefill steps: no eager sampling launch; the penalised variant ran, the cohort formed and ran it
    assert watch.last_prefill > 0 and watch.eager and max(watch.eager) <= watch.last_prefill, (watch.eager, watch.last_prefill)
    assert any(key[2] == "penalized" for key in dec.graphs), "the penalised variant was never replayed"
    assert fill.n_cohort_steps > 0
    cohort_launches = [launch for launch in watch.fetched if launch not in watch.by_launch_decode]
    assert cohort_launches and all(variants[launch][0] == "penalized" for launch in cohort_launches), \
        "the cohort did not run the penalised variant"
    # every draw is Philox(seed, s), every token of a launch is the request's token s
    seen = watch.check_draws(rcbs)
    for i in SAMPLED:
        assert seen[i] == sorted(set(seen[i])) and seen[i][0] >= 1 and seen[i][-1] == MAX_TOKENS[i] - 1, (i, seen[i])
    check_logs(rcbs, dec, MAX_TOKENS)
    # nobody was seeded but on arrival in the decode batch and after an eager step (a prefill step that took it along)
    assert dec.log_table.n_seeds <= len(PENALTIES) * (1 + len(set(watch.eager)))
    # the greedy requests' tokens are those of a run without the switch; so are the penalised greedy request's — the
    # eager step penalises with the same arithmetic over the same history
    for i in (3, 4, 5, 1):
        assert rcbs[i].output_token_ids == eager[i].output_token_ids, i
    # the same trace again, request 2 with the seed it was assigned: the same tokens
    again = dict(SAMPLED)
    again[2] = dict(SAMPLED[2], seed=rcbs[2].sampling_params.seed)
    second = run(requests(again, PENALTIES, MAX_TOKENS), monkeypatch)[0]
    assert [r.output_token_ids for r in second] == [r.output_token_ids for r in rcbs]


def test_a_return_from_eager_steps_seeds_the_log_again(monkeypatch):
    """request 5 asks for logprobs and lives for 4 tokens: while it decodes the steps are eager, afterwards the penalised
    requests are back in the graph — seeded with the tokens the eager steps delivered"""
    max_tokens = (12, 12, 12, 12, 12, 4)
    reqs = requests(SAMPLED, PENALTIES, max_tokens)
    reqs[5][1].sampling_params.logprobs = True
    rcbs, watch, fill, variants = run(reqs, monkeypatch)
    dec = fill.graph_decoder
    assert all(len(r.output_token_ids) == m for r, m in zip(rcbs, max_tokens))
    assert len(rcbs[5].output_logprobs) == 4
    assert max(watch.eager) > watch.last_prefill, "the logprobs request never sent a decode step to the eager path"
    # the eager steps are over when request 5 is: every later step with a penalised request in it is a penalised launch
    later = [v for launch, (v, step) in variants.items()
             if step > max(watch.eager) and any(i in PENALTIES for i, _ in watch.rows[launch])]
    assert later and all(v == "penalized" for v in later), later
    assert dec.log_table.n_seeds > len(PENALTIES), "nobody was seeded again after the eager steps"
    watch.check_draws(rcbs)
    check_logs(rcbs, dec, max_tokens)


def test_switch_off_a_penalised_request_still_sends_the_steps_to_eager(monkeypatch):
    rcbs, watch, fill, _ = run_sampled_only(requests(SAMPLED, PENALTIES, MAX_TOKENS), monkeypatch)
    dec = fill.graph_decoder
    assert dec.sampled and not dec.penalized and not hasattr(dec, "token_log")
    assert all(len(r.output_token_ids) == m for r, m in zip(rcbs, MAX_TOKENS))
    assert max(watch.eager) > watch.last_prefill
    assert not any(key[2] == "penalized" for key in dec.graphs)
    for i in PENALTIES:
        assert Counter(rcbs[i].output_token_ids) == dict(zip(rcbs[i].penalty_history.ids, rcbs[i].penalty_history.counts))
