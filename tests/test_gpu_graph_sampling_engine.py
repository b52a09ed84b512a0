"""GPU: sampled decoding from the captured step through the engine (the graph_sampling switch: GraphedDecoder(sampled=True)
behind BatchFillExecutor), on the cluster of tests/test_gpu_sampling_engine.py.  Six requests without penalties, three of
them sampled.  With the switch on, once the prefill steps are over no eager sampling step runs: the tokens come from the
sampled variant of the graph and from the cohort, and every draw the graph made for token s of a request is
Philox(seed, s) — the offset the eager step would have used, so a request may move between the two paths step by step
(a penalised request in the batch sends the steps back to the eager path, and the draws still line up)."""
import numpy as np
import pytest
import torch

from hydrainfer_amd.engine import executor as executor_module
from hydrainfer_amd.engine.graph_decode import GraphedDecoder
from tests import sampling_ref as ref
from tests.engine_util import run_trace
from tests.test_gpu_penalties_engine import _cluster, _creator, _requests
from tests.test_gpu_sampling_engine import _check_tokens

pytestmark = pytest.mark.gpu

# requests 1, 3 and 5 stay greedy; 2 has no seed (the engine assigns one)
SAMPLED = {0: dict(temperature=0.8, seed=(1 << 40) + 1),
           2: dict(temperature=1.3),
           4: dict(temperature=0.7, top_p=0.9, top_k=20, seed=77)}
MAX_TOKENS = (12, 12, 12, 12, 12, 12)


def requests(sampled=SAMPLED, penalties={}, max_tokens=MAX_TOKENS):
    reqs = _requests(penalties, max_tokens=max_tokens)
    for i, fields in sampled.items():
        for k, v in fields.items():
            setattr(reqs[i][1].sampling_params, k, v)
    return reqs


class Watch:
    """What ran: the step number of every eager sampling launch (forward_sampled and sample_rows are tapped) and of the
    last step with a prefill piece in it; per decode launch, the (request, index of the token being generated) of its rows
    — read off the requests when the launch is made — and, once fetched, its tokens and draws."""

    def __init__(self, lm, fill, monkeypatch):
        self.step, self.last_prefill, self.eager = 0, -1, []
        self.rows, self.fetched, self.by_launch_decode = {}, {}, set()
        dec = fill.graph_decoder
        real_execute, real_forward, real_kernel = fill.execute, lm.forward_sampled, executor_module.sample_rows
        real_launch, real_cohort, real_fetch = fill._launch_decode, dec.launch_cohort, dec.fetch

        def execute(batch):
            self.step += 1
            if any(len(inst.token_ids) != 1 for _, inst in batch):
                self.last_prefill = self.step
            real_execute(batch)

        def forward_sampled(*a, **kw):
            self.eager.append(self.step)
            return real_forward(*a, **kw)

        def kernel(*a, **kw):
            self.eager.append(self.step)
            return real_kernel(*a, **kw)

        def launch_decode(batch, rows):
            self.rows[dec.launches + 1] = [(rcb.request_id, len(rcb.output_token_ids)) for rcb, _ in batch]
            self.by_launch_decode.add(dec.launches + 1)
            real_launch(batch, rows)

        def launch_cohort(*a):
            self.step += 1
            self.rows[dec.launches + 1] = [(i, s + 1) for i, s in self.rows[dec.launches]]
            return real_cohort(*a)

        def fetch(launch):
            tokens = real_fetch(launch)
            self.fetched[launch] = (tokens, dec.fetch_draws(launch) if dec.keep_draws else None)
            return tokens
        fill.execute, fill._launch_decode, dec.launch_cohort, dec.fetch = execute, launch_decode, launch_cohort, fetch
        lm.forward_sampled = forward_sampled
        monkeypatch.setattr(executor_module, "sample_rows", kernel)

    def check_draws(self, rcbs):
        """every draw of a sampled launch: Philox(seed, s) bit for bit, and the token is the request's token s ->
        {request: [s, ...]} of the tokens that came from sampled launches"""
        seen = {}
        for launch, (tokens, u) in sorted(self.fetched.items()):
            if u is None:
                continue
            for row, (i, s) in enumerate(self.rows[launch]):
                sp, out = rcbs[i].sampling_params, rcbs[i].output_token_ids
                if sp.temperature > 0:
                    want = ref.uniform(sp.seed, s)
                    assert u[row].view(np.uint32) == want.view(np.uint32), f"launch {launch} request {i} token {s}: u {u[row]!r} != {want!r}"
                    seen.setdefault(i, []).append(s)
                if s < len(out):
                    assert tokens[row] == out[s], f"launch {launch} request {i} token {s}"
        return seen


def run(reqs, monkeypatch, graph_sampling=True):
    cluster, tap = _cluster(False, True, 128)
    fill = cluster.nodes[0].executor.fill_executor
    if graph_sampling:
        old = fill.graph_decoder
        fill.graph_decoder = GraphedDecoder(old.lm, old.kv, max_batch=old.max_batch, max_blocks_per_seq=old.cap, sampled=True,
                                            keep_draws=True)
        assert fill.graph_decoder.sampled
    watch = Watch(old.lm if graph_sampling else fill.language_model, fill, monkeypatch)
    rcbs = run_trace(cluster, _creator(), reqs)
    assert fill.pending is None and fill.cohort is None
    return rcbs, watch, fill, tap


def test_sampled_requests_decode_from_the_graph(monkeypatch):
    greedy = run(requests({}), monkeypatch, graph_sampling=False)[0]
    rcbs, watch, fill, _ = run(requests(), monkeypatch)
    dec = fill.graph_decoder
    assert all(len(r.output_token_ids) == m for r, m in zip(rcbs, MAX_TOKENS))
    assert any(key[2] == "sampled" for key in dec.graphs), "the sampled variant was never replayed"
    # after the prefill steps: no eager sampling launch, every token from a sampled launch, the cohort among them
    assert watch.last_prefill > 0 and watch.eager and max(watch.eager) <= watch.last_prefill, (watch.eager, watch.last_prefill)
    seen = watch.check_draws(rcbs)
    for i in SAMPLED:
        # token 0 comes from the prefill step; of the others at most one per eager step did not come from a graph
        assert seen[i] == sorted(set(seen[i])) and seen[i][0] >= 1 and seen[i][-1] == MAX_TOKENS[i] - 1, (i, seen[i])
        assert len(seen[i]) >= MAX_TOKENS[i] - 1 - (len(set(watch.eager)) - 1), (i, seen[i], watch.eager)
    assert fill.n_cohort_steps > 0
    cohort_launches = [launch for launch in watch.fetched if launch not in watch.by_launch_decode]
    assert cohort_launches and all(watch.fetched[launch][1] is not None for launch in cohort_launches), \
        "the cohort did not run the sampled variant"
    assert isinstance(rcbs[2].sampling_params.seed, int) and rcbs[0].sampling_params.seed == (1 << 40) + 1
    for i in (1, 3, 5):
        assert rcbs[i].sampling_params.seed is None and rcbs[i].output_token_ids == greedy[i].output_token_ids
    assert any(rcbs[i].output_token_ids != greedy[i].output_token_ids for i in SAMPLED), "no draw left the greedy path"
    # the same trace again, request 2 with the seed it was assigned: the same tokens
    again = dict(SAMPLED)
    again[2] = dict(SAMPLED[2], seed=rcbs[2].sampling_params.seed)
    second = run(requests(again), monkeypatch)[0]
    assert [r.output_token_ids for r in second] == [r.output_token_ids for r in rcbs]


def test_switch_off_every_sampled_token_is_eager(monkeypatch):
    rcbs, watch, fill, tap = run(requests(), monkeypatch, graph_sampling=False)
    assert not fill.graph_decoder.sampled and all(key[2] == "greedy" for key in fill.graph_decoder.graphs)
    for i in SAMPLED:
        _check_tokens(rcbs[i], tap)              # (one eager sampling step per token, none from a graph)
    assert max(watch.eager) > watch.last_prefill


def test_a_penalised_request_sends_the_steps_back_to_eager(monkeypatch):
    """request 5 adds a frequency penalty and lives for 4 tokens: while it decodes the batch is eager, before and after it
    the sampled requests are back in the graph — their offsets agree across the two paths"""
    max_tokens = (12, 12, 12, 12, 12, 4)
    rcbs, watch, fill, _ = run(requests(penalties={5: (0.7, 0.0, 1.0)}, max_tokens=max_tokens), monkeypatch)
    assert all(len(r.output_token_ids) == m for r, m in zip(rcbs, max_tokens))
    assert max(watch.eager) > watch.last_prefill, "the penalised request never sent a decode step to the eager path"
    seen = watch.check_draws(rcbs)
    for i in SAMPLED:
        assert seen.get(i) and seen[i][-1] == max_tokens[i] - 1, (i, seen.get(i))
    assert sum(rcbs[5].penalty_history.counts) == 4
