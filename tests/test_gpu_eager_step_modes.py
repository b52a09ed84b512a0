"""GPU: the seams of the eager sampling step (engine/executor.py), mode by mode.  A step of BatchFillExecutor.execute is
constrained, drawn, penalised, logprobs or plain; what it calls is a contract other code stands on (the test taps that
stand in for the language model, the tests that patch the executor module's kernel names, the bench tools): ONE entry
point of the language model, the kernel wrappers reached through the `executor` module in one order, one packed buffer
sent to the device.  Every step of ten small traces is held to a literal table of those three, written from the `if`
chain of the executor as it stood when the five modes were five functions; the tokens of every trace replay on a fresh
engine, and asking for log-probabilities changes no token."""
import functools

import pytest

from hydrainfer_amd import sampling
from hydrainfer_amd.engine import executor as ex
from hydrainfer_amd.engine.isa import Fill
from tests.engine_util import run_trace
from tests.golden import cases as C
from tests.test_gpu_penalties_engine import _cluster, _creator, _requests

pytestmark = pytest.mark.gpu

LM_ENTRIES = ("forward", "forward_logits", "forward_logprobs", "forward_penalized", "forward_sampled", "forward_constrained")
KERNELS = ("argmax_rows", "logprob_rows", "penalized_argmax_rows", "sample_rows", "sample_rows_constrained",
           "token_logprob_rows")
STEP_CLASSES = (sampling.PenaltyStep, sampling.SampleStep, sampling.ConstrainedStep)
# request 0 of a trace is of the trace's kind; the image placeholder is banned where a constraint moves the tokens
# (the engine cannot take it back as a text token)
KINDS = {"constrained": dict(logit_bias={C.TINY_IMAGE_TOKEN_ID: -100, 7: 5.0}),
         "drawn": dict(temperature=0.8, top_p=0.9, top_k=20, seed=(1 << 40) + 1),
         "penalised": dict(frequency_penalty=1.0, presence_penalty=1.0, repetition_penalty=100.0),
         "logprobs": dict(logprobs=True, top_logprobs=1),
         "plain": {}}
BESIDE = dict(logprobs=True, top_logprobs=2)        # request 1 in a trace's second run: the 46-token prompt, chunked
# (the step's mode, some request of the step asks for log-probabilities with an instruction that is not a chunk) ->
# (the language model's entry points, the kernel wrappers called through the executor module, packed buffers sent)
EXPECTED = {
    None: ([], [], 0),                              # nothing samples: forward_hidden, for the cache writes
    ("plain", False): (["forward"], [], 0),
    ("logprobs", True): (["forward_logprobs"], [], 0),
    ("penalised", False): (["forward_penalized"], [], 1),
    ("penalised", True): (["forward_logits"], ["logprob_rows", "penalized_argmax_rows"], 1),
    ("drawn", False): (["forward_sampled"], [], 1),
    ("drawn", True): (["forward_logits"], ["logprob_rows", "sample_rows"], 1),
    ("constrained", False): (["forward_constrained"], [], 1),
    ("constrained", True): (["forward_logits"], ["logprob_rows", "sample_rows_constrained"], 1),
}


def trace_requests(mode, beside, max_tokens=(4, 3, 4)):
    """three requests arriving together: 0 of the trace's kind, 1 (asking when `beside`) and 2 plain"""
    reqs = _requests({}, text_len=(10, 45, 3), max_tokens=max_tokens)
    for i, fields in ((0, KINDS[mode]), (1, BESIDE if beside else {})):
        for k, v in fields.items():
            setattr(reqs[i][1].sampling_params, k, v)
    return reqs


def _key(batch, mode):
    rows = [(rcb, inst) for rcb, inst in batch if isinstance(inst, Fill) and inst.sample]
    if not rows:
        return None
    asking = any(rcb.sampling_params.logprobs and not inst.is_chunked for rcb, inst in rows)
    special = mode not in ("plain", "logprobs") and any(rcb.request_id == 0 for rcb, _ in rows)
    return (mode if special else "logprobs" if asking else "plain", asking)


def _run(mode, beside):
    """-> (the requests' token ids, [(key, entry points, kernel wrappers, packed buffers) per executor step])"""
    cluster, _ = _cluster(True, False)
    fill = cluster.nodes[0].executor.fill_executor
    lm = fill.language_model
    calls = dict(lm=[], kernels=[], packs=0, depth=0)
    steps = []
    with pytest.MonkeyPatch.context() as mp:
        for name in LM_ENTRIES:                     # on the instance; an entry point called by another one is not counted
            def entry(*a, _real=getattr(lm, name), _name=name, **k):
                if calls["depth"] == 0:
                    calls["lm"].append(_name)
                calls["depth"] += 1
                try:
                    return _real(*a, **k)
                finally:
                    calls["depth"] -= 1
            mp.setattr(lm, name, entry, raising=False)
        for name in KERNELS:
            def kernel(*a, _real=getattr(ex, name), _name=name, **k):
                calls["kernels"].append(_name)
                return _real(*a, **k)
            mp.setattr(ex, name, kernel)
        for cls in STEP_CLASSES:
            def to_device(self, device, _real=cls.to_device):
                calls["packs"] += 1
                return _real(self, device)
            mp.setattr(cls, "to_device", to_device)

        def execute(batch, real=fill.execute):
            key = _key(batch, mode)
            calls.update(lm=[], kernels=[], packs=0)
            real(batch)
            steps.append((key, calls["lm"], calls["kernels"], calls["packs"]))
        fill.execute = execute
        rcbs = run_trace(cluster, _creator(), trace_requests(mode, beside))
    assert fill.pending is None and fill.cohort is None
    assert all(len(r.output_token_ids) == r.sampling_params.max_tokens for r in rcbs)
    return [r.output_token_ids for r in rcbs], steps


first_run = functools.lru_cache(maxsize=None)(_run)


@pytest.mark.parametrize("beside", [False, True], ids=["alone", "beside_logprobs"])
@pytest.mark.parametrize("mode", list(KINDS))
def test_every_step_makes_the_calls_of_its_mode(mode, beside):
    ids, steps = first_run(mode, beside)
    for n, (key, lm_calls, kernels, packs) in enumerate(steps):
        assert (lm_calls, kernels, packs) == EXPECTED[key], f"step {n} ({key})"
    print(mode, beside, [key for key, *_ in steps])
    # the trace shows what it is there for: a step of its own mode, with the asking request in it when there is one
    want = (mode, beside) if mode not in ("plain", "logprobs") else ("logprobs", True) if beside or mode == "logprobs" \
        else ("plain", False)
    assert want in {key for key, *_ in steps}, f"no {want} step in the trace"
    assert ids == _run(mode, beside)[0], "the trace does not replay on a fresh engine"


def test_asking_for_logprobs_changes_no_token():
    plain = first_run("plain", False)[0]
    assert plain == first_run("logprobs", False)[0] == first_run("plain", True)[0] == first_run("logprobs", True)[0]
    # and the greedy requests beside a request of another kind keep their tokens
    for mode in ("constrained", "drawn", "penalised"):
        for beside in (False, True):
            assert first_run(mode, beside)[0][1:] == plain[1:]
