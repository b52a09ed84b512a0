"""The one decision of the eager sampling step (engine/executor.py: step_mode) over every mix of requests, against a
table written out from the `if` chain that `execute` and `_execute_scoring` each carried before there was one decision;
and SAMPLING_MODES, whose names must exist where the step looks them up.  The requests are stand-ins with the fields the
decision reads."""
from types import SimpleNamespace as NS

import pytest

from hydrainfer_amd.engine import executor as ex
from hydrainfer_amd.engine.executor import SAMPLING_MODES, step_mode
from hydrainfer_amd.model.llama import LlamaForCausalLM
from hydrainfer_amd.model.llava import LlavaLanguageModel


def _row(constrained=False, drawn=False, penalised=False, top_logprobs=None, chunked=False):
    sp = NS(logprobs=top_logprobs is not None, top_logprobs=top_logprobs or 0, temperature=0.7 if drawn else 0.0)
    rcb = NS(sampling_params=sp, token_constraints=object() if constrained else None,
             penalty_history=object() if penalised else None)
    return rcb, NS(is_chunked=chunked)


# (a constrained, a drawn, a penalised, a request asking for top_logprobs = 2 is in the batch) -> (mode, top_k);
# a plain request is in every batch
TABLE = {
    (0, 0, 0, 0): ("plain", None),
    (0, 0, 0, 1): ("logprobs", 2),
    (0, 0, 1, 0): ("penalised", None),
    (0, 0, 1, 1): ("penalised", 2),
    (0, 1, 0, 0): ("drawn", None),
    (0, 1, 0, 1): ("drawn", 2),
    (0, 1, 1, 0): ("drawn", None),
    (0, 1, 1, 1): ("drawn", 2),
    (1, 0, 0, 0): ("constrained", None),
    (1, 0, 0, 1): ("constrained", 2),
    (1, 0, 1, 0): ("constrained", None),
    (1, 0, 1, 1): ("constrained", 2),
    (1, 1, 0, 0): ("constrained", None),
    (1, 1, 0, 1): ("constrained", 2),
    (1, 1, 1, 0): ("constrained", None),
    (1, 1, 1, 1): ("constrained", 2),
}


@pytest.mark.parametrize("present", list(TABLE), ids=["".join(map(str, k)) for k in TABLE])
def test_every_mix_of_requests(present):
    c, d, p, a = present
    rows = [_row()] + [_row(constrained=True)] * c + [_row(drawn=True)] * d + [_row(penalised=True)] * p \
        + [_row(top_logprobs=2)] * a
    assert step_mode(rows) == TABLE[present]
    assert step_mode(rows[::-1]) == TABLE[present]          # whatever the order of the rows


def test_one_request_of_several_kinds_and_no_request():
    # one request may be constrained, sampled and penalised at once
    assert step_mode([_row(constrained=True, drawn=True, penalised=True)]) == ("constrained", None)
    assert step_mode([_row(drawn=True, penalised=True), _row()]) == ("drawn", None)
    assert step_mode([]) == ("plain", None)


def test_a_chunk_head_that_asks_contributes_no_top_k():
    # its sample is thrown away, and so would its scores be: alone it leaves the step plain
    assert step_mode([_row(top_logprobs=5, chunked=True), _row()]) == ("plain", None)
    assert step_mode([_row(top_logprobs=5, chunked=True), _row(top_logprobs=1)]) == ("logprobs", 1)
    assert step_mode([_row(top_logprobs=5, chunked=True), _row(penalised=True)]) == ("penalised", None)
    assert step_mode([_row(top_logprobs=5, chunked=True), _row(drawn=True, chunked=True)]) == ("drawn", None)


def test_two_asking_requests_give_the_larger_top_logprobs():
    assert step_mode([_row(top_logprobs=3), _row(top_logprobs=7), _row()]) == ("logprobs", 7)
    assert step_mode([_row(top_logprobs=7), _row(constrained=True), _row(top_logprobs=3)]) == ("constrained", 7)
    assert step_mode([_row(top_logprobs=0), _row()]) == ("logprobs", 0)       # asking for no alternatives is still asking


def test_the_modes_name_what_exists():
    assert list(SAMPLING_MODES) == ["constrained", "drawn", "penalised"]        # the order of the decision
    for mode, (take, packer, forward, kernel) in SAMPLING_MODES.items():
        assert callable(getattr(ex, packer)) and callable(getattr(ex, kernel)), mode
        assert callable(getattr(LlavaLanguageModel, forward)) and callable(getattr(LlamaForCausalLM, forward)), mode
    assert [m[0] for m in SAMPLING_MODES.values()] == [4, 3, 2]
    # and the two modes that are not in the table
    for name in ("forward", "forward_logits", "forward_logprobs"):
        assert callable(getattr(LlavaLanguageModel, name)) and callable(getattr(LlamaForCausalLM, name))
    for name in ("argmax_rows", "logprob_rows", "token_logprob_rows"):
        assert callable(getattr(ex, name))
