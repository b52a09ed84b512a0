"""CPU: the token-choice host layer as one chain — penalty, sample, constrained, scored and masked step buffers nest word
for word, every view aliases the buffer it was cut from, the packers reproduce the buffers recorded before the layouts
were described once (tests/golden/token_choice_layout.npz), and the executor's one scored step makes the calls its two
predecessors made."""
import os

import numpy as np
import torch

from hydrainfer_amd.engine import InstructionCreator
from hydrainfer_amd.engine import executor as ex
from hydrainfer_amd._C.kernel.norm import logprob_rows_bytes, logprob_rows_views
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, SAMPLE_RECORD_WORDS, PenaltyHistory, TokenMask,
                                     pack_constrained_step, pack_masked_step, pack_penalty_step, pack_sample_step,
                                     pack_scored_step)
from tests.test_token_mask_cpu import _executor, _request, _step

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_choice_layout.npz")
PROCESSED = "processed_logprobs"


def mixed_entries():
    """One 5-row step as six-element entries (history, penalties, record, bias, want, mask): row 1 has no history, rows 1-3
    no bias, rows 1, 2 and 4 want = -1, rows 0 and 3 share one mask object, row 2 has a mask of its own."""
    n = 100
    a, b = TokenMask(n, guided_choice=[[5, 6], [7, 8]]), TokenMask(n, allowed_token_ids=[1, 99])
    bias = (np.asarray([3, 9], np.int32), np.asarray([0.5, -2.0], np.float32))
    ban = (np.asarray([2], np.int32), np.asarray([-np.inf], np.float32))
    return [(PenaltyHistory([4, 4, 5]), (0.5, 0.25, 1.5), (0.7, 0.9, 50, 77, 4, 0.25), bias, 0, a.current()),
            (None, NO_PENALTIES, GREEDY_RECORD, None, -1, None),
            (PenaltyHistory(), NO_PENALTIES, (1.0, 1.0, 0, (1 << 63) - 1, 1), None, -1, b.current()),
            (PenaltyHistory([8]), (0.0, 0.0, 2.0), GREEDY_RECORD, None, 3, a.current()),
            (PenaltyHistory([7, 1, 7, 7]), (-0.5, 0.0, 1.0), (0.3, 0.5, 0, 9, 6, 0.0), ban, -1, None)]


def chain(entries):
    """{name: step} of the five packers over the same rows."""
    return {"penalty": pack_penalty_step([e[:2] for e in entries]), "sample": pack_sample_step([e[:3] for e in entries]),
            "constrained": pack_constrained_step([e[:4] for e in entries]), "scored": pack_scored_step([e[:5] for e in entries]),
            "masked": pack_masked_step(entries)}


def test_the_layout_chain_word_for_word():
    entries = mixed_entries()
    steps = chain(entries)
    buf = {k: s.buffer for k, s in steps.items()}
    rows = len(entries)
    assert all(b.dtype == np.int32 and b.ndim == 1 for b in buf.values())
    assert np.array_equal(buf["sample"][SAMPLE_RECORD_WORDS * rows:], buf["penalty"])
    for inner, outer in (("sample", "constrained"), ("constrained", "scored"), ("scored", "masked")):
        assert buf[outer].size > buf[inner].size and np.array_equal(buf[outer][:buf[inner].size], buf[inner]), (inner, outer)
    want = [e[4] for e in entries]
    assert np.array_equal(buf["scored"], np.concatenate([buf["constrained"], np.asarray(want, dtype=np.int32)]))
    assert buf["masked"].size == buf["scored"].size + rows + 2 * 4, "mask_row and two distinct masks of four words"
    # what the classes say about themselves
    assert [(s.rows, s.total) for s in steps.values()] == [(5, 5)] * 5
    assert [s.bias_total for s in (steps["constrained"], steps["scored"], steps["masked"])] == [3, 3, 3]
    assert (steps["masked"].n_masks, steps["masked"].words) == (2, 4)
    # the tuple orders: the scored step is the constrained step's eight tables, then want
    *eight, w = steps["scored"].views()
    assert len(eight) == 8 and w.dtype == torch.int32 and w.tolist() == want
    for got, ref in zip(eight, steps["constrained"].views()):
        assert got.dtype == ref.dtype and got.shape == ref.shape and torch.equal(got, ref)
    assert steps["masked"].views()[-1].tolist() == want and steps["masked"].views()[5].tolist() == [0, -1, 1, 0, -1]
    assert [len(s.views()) for s in steps.values()] == [4, 5, 8, 9, 11]
    # every view is an alias of the buffer it was cut from: on the default host tensor and on a tensor handed in
    for name, step in steps.items():
        lo = step.buffer.ctypes.data
        hi = lo + step.buffer.nbytes
        for v in step.views():
            assert v.numel() == 0 or lo <= v.data_ptr() < hi, f"{name}: a view of the default tensor is a copy"
        t = torch.from_numpy(step.buffer.copy())
        store = t.untyped_storage().data_ptr()
        for v in step.views(t):
            assert v.untyped_storage().data_ptr() == store, f"{name}: a view of the given tensor is a copy"
        assert sum(v.numel() for v in step.views(t)) == t.numel(), f"{name}: the views cover the buffer once"


def test_the_packers_reproduce_the_recorded_buffers():
    golden = np.load(GOLDEN)
    steps = chain(mixed_entries())
    assert sorted(golden.files) == sorted(steps)
    for name, step in steps.items():
        assert golden[name].dtype == np.int32 and np.array_equal(step.buffer, golden[name]), name


# ---------------------------------------------------------------------------------------------------- the executor seam
def _packed_result(rows, k, token, lp):
    """a launch's four results over one packed buffer, as logprob_rows and sample_rows_logprobs return them"""
    views = logprob_rows_views(torch.zeros(logprob_rows_bytes(rows, k), dtype=torch.uint8), rows, k)
    views[0].fill_(token), views[1].fill_(lp), views[3].fill_(lp)
    views[2].copy_(torch.arange(100 * token, 100 * token + k, dtype=torch.int32).expand(rows, k))
    return views


def _seam(monkeypatch, log):
    """the executor on the stand-in language model, `forward_scored` added, every kernel it reaches by name recorded"""
    fill = _executor(log)

    def forward_scored(input_ids, image_features, position_ids, params, *tables, top_k, want):
        log.append(("forward_scored", len(tables), want.dtype, want.tolist(), top_k))
        return _packed_result(len(params.selected), top_k, 21, -0.5)
    fill.language_model.forward_scored = forward_scored

    def logprob_rows(logits, top_k):
        log.append(("logprob_rows", top_k))
        return _packed_result(logits.shape[0], top_k, 11, -0.25)

    def sample_rows_logprobs(logits, *tables, top_k, want):
        log.append(("sample_rows_logprobs", len(tables), want.tolist(), top_k))
        return _packed_result(logits.shape[0], top_k, 21, -0.5)

    def sample_rows_masked(logits, *tables, top_k=None, want=None):
        log.append(("sample_rows_masked", len(tables), tables[5].tolist(), None if want is None else want.tolist(), top_k))
        return torch.tensor([4 if j >= 0 else 11 for j in tables[5].tolist()])
    for f in (logprob_rows, sample_rows_logprobs, sample_rows_masked):
        monkeypatch.setattr(ex, f.__name__, f)
    for name in ("sample_rows_constrained", "sample_rows", "penalized_argmax_rows", "argmax_rows"):
        def other(*a, _name=name, **kw):
            raise AssertionError(f"{_name} launched in a scored step")
        monkeypatch.setattr(ex, name, other)
    return fill


def test_the_scored_step_makes_the_calls_it_made(monkeypatch):
    log = []
    fill = _seam(monkeypatch, log)
    c = InstructionCreator(image_token_id=63, n_image_tokens_per_image=4, block_size=16)
    new = lambda **sp: c.process(_request(**sp), vocab_size=64)
    processed = dict(logprobs=True, top_logprobs=2, logprobs_mode=PROCESSED, temperature=0.5, seed=3)
    # one processed-logprobs request beside plain ones: ONE entry point, eight tables, want as a tensor
    rcbs = [new(), new(**processed), new()]
    _step(fill, rcbs)
    assert log == [("forward_scored", 8, torch.int32, [-1, 0, -1], 2)]
    assert [r.output_token_ids for r in rcbs] == [[21]] * 3
    assert [len(r.output_logprobs) for r in rcbs] == [0, 1, 0]
    assert rcbs[1].output_logprobs[0] == ex.TokenLogprob(21, -0.5, [(2100, -0.5), (2101, -0.5)])
    # a raw-mode request beside them: the logits, the raw scores' side launch, then the scored launch
    del log[:]
    rcbs = [new(), new(**processed), new(logprobs=True, top_logprobs=3)]
    _step(fill, rcbs)
    assert log == ["forward_logits", ("logprob_rows", 3), ("sample_rows_logprobs", 8, [-1, 0, -1], 2)]
    assert [r.output_token_ids for r in rcbs] == [[21]] * 3
    assert rcbs[1].output_logprobs[0] == ex.TokenLogprob(21, -0.5, [(2100, -0.5), (2101, -0.5)])
    assert rcbs[2].output_logprobs[0] == ex.TokenLogprob(21, -0.25, [(1100, -0.25), (1101, -0.25), (1102, -0.25)]), \
        "the raw-mode request's scores are logprob_rows', not the launch's"
    # a masked step beside a raw-mode request: the same order, the unscored masked launch
    del log[:]
    rcbs = [new(allowed_token_ids=[3, 4]), new(logprobs=True, top_logprobs=1), new()]
    _step(fill, rcbs)
    assert log == ["forward_logits", ("logprob_rows", 1), ("sample_rows_masked", 10, [0, -1, -1], None, None)]
    assert [r.output_token_ids for r in rcbs] == [[4], [11], [11]]
    assert [len(r.output_logprobs) for r in rcbs] == [0, 1, 0]
    assert rcbs[1].output_logprobs[0] == ex.TokenLogprob(11, -0.25, [(1100, -0.25)])
    # and a masked, processed request beside a raw-mode one: the scored masked launch, want on its row alone
    del log[:]
    masked = new(allowed_token_ids=[3, 4], logprobs=True, top_logprobs=2, logprobs_mode=PROCESSED)
    monkeypatch.setattr(ex, "sample_rows_masked", lambda logits, *tables, top_k=None, want=None: (
        log.append(("sample_rows_masked", len(tables), want.tolist(), top_k)), _packed_result(logits.shape[0], top_k, 4, -0.5))[1])
    rcbs = [new(logprobs=True, top_logprobs=3), masked]
    _step(fill, rcbs)
    assert log == ["forward_logits", ("logprob_rows", 3), ("sample_rows_masked", 10, [-1, 0], 2)]
    assert rcbs[0].output_logprobs[0] == ex.TokenLogprob(4, -0.25, [(1100, -0.25), (1101, -0.25), (1102, -0.25)])
    assert rcbs[1].output_logprobs[0] == ex.TokenLogprob(4, -0.5, [(400, -0.5), (401, -0.5)])
