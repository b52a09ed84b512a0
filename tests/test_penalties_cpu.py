"""CPU: the host side of frequency / presence / repetition penalties — the fp32 restatement the GPU tests measure against
(tests/penalty_ref.py) held to what the reference's own process_logits gave (tests/golden/g14_penalties.npz), the
request's history table and the step packer, request parsing and validation, and the refusals."""
import json
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.entrypoint import api_protocol as proto
from hydrainfer_amd.sampling import NO_PENALTIES, PenaltyHistory, is_penalized, pack_penalty_step
from tests import penalty_ref as ref


def test_restatement_reproduces_the_reference_exactly():
    rows = ref.load_golden()
    assert len(rows) >= 24 and {r["n"] for r in rows} == {8, 1000, 32064}
    assert {len(r["ids"]) for r in rows} >= {0, 1, 63, 300}
    inside = [r for r in rows if r["raw_best"] in r["ids"]]
    assert 2 * len(inside) >= len(rows)
    moved = 0
    for r in rows:
        assert len(set(r["ids"])) == len(r["ids"])
        row, scores, best = ref.penalized_row(r["logits"], r["ids"], r["counts"], *r["penalties"])
        assert torch.equal(scores.view(torch.int32), r["scores"].view(torch.int32)), f"n={r['n']} h={len(r['ids'])}: scores differ"
        assert best == r["best"] and float(row[best]) == r["max"]
        assert int(torch.argmax(r["logits"].float())) == r["raw_best"]
        if not r["ids"]:
            assert best == r["raw_best"]
        moved += best != r["raw_best"]
    assert moved >= len(rows) // 3, "the fixture's penalties hardly ever change the token"


def test_restatement_on_hand_computed_rows():
    x = torch.tensor([2.0, -1.0, 1.5, 0.5, 1.5])
    # token 0 seen 3 times, f = 0.5: 2 - 1.5 = 0.5; p = 0.25: 0.25; r = 2: 0.125.  token 1 seen once: -1 - .5 - .25 = -1.75, * 2
    row, scores, best = ref.penalized_row(x, [0, 1], [3, 1], 0.5, 0.25, 2.0)
    assert scores.tolist() == [0.125, -3.5] and row.tolist() == [0.125, -3.5, 1.5, 0.5, 1.5] and best == 2
    # count 0: no frequency / presence term, repetition still applies
    assert ref.penalized_row(x, [0], [0], 0.5, 0.25, 2.0)[1].tolist() == [1.0]
    # ids outside the row are ignored
    row, scores, best = ref.penalized_row(x, [-1, 5, 0], [1, 1, 1], 0.0, 0.0, 4.0)
    assert math.isnan(scores[0]) and math.isnan(scores[1]) and scores[2] == 0.5 and best == 2
    assert ref.argmax_in_order(torch.tensor([1.0, math.nan, 5.0, math.nan])) == 1
    assert ref.argmax_in_order(torch.full((4,), -math.inf)) == 0
    ids, scores = ref.penalized_batch(torch.stack([x, x]), [0, 1], [3, 1], [0, 0, 2], [[9, 9, 9], [0.5, 0.25, 2.0]])
    assert ids.tolist() == [0, 2] and scores.tolist() == [0.125, -3.5]


def test_history_counts():
    h = PenaltyHistory()
    assert len(h) == 0 and list(h.ids) == [] and list(h.counts) == []
    for t in (7, 3, 7, 7, 9, 3):
        h.append(t)
    assert list(h.ids) == [7, 3, 9] and list(h.counts) == [3, 2, 1] and h.slot == {7: 0, 3: 1, 9: 2} and len(h) == 3
    assert list(PenaltyHistory([5, 5, 5]).ids) == [5] and list(PenaltyHistory([5, 5, 5]).counts) == [3]
    for t in range(2000):           # appending after the packer has looked at the arrays (no buffer left exported)
        pack_penalty_step([(h, NO_PENALTIES)])
        h.append(t)
    assert len(h) == 2000 and [h.counts[h.slot[t]] for t in (7, 3, 9, 0)] == [4, 3, 2, 1] and sum(h.counts) == 2006


def test_packer_builds_the_csr_of_a_mixed_step():
    a, only = PenaltyHistory([4, 8, 4, 15]), PenaltyHistory([6, 6, 6, 6])
    step = pack_penalty_step([(a, (0.5, -0.25, 1.5)), (None, NO_PENALTIES), (PenaltyHistory(), (1.0, 1.0, 2.0)),
                              (only, (0.0, 0.0, 1.25)), (None, NO_PENALTIES)])
    assert (step.rows, step.total) == (5, 4) and step.buffer.dtype == np.int32 and step.buffer.shape == (4 * 5 + 1 + 8,)
    hist_ids, hist_counts, cu_hist, penalties = step.views()
    assert cu_hist.tolist() == [0, 3, 3, 3, 4, 4] and cu_hist.dtype == torch.int32
    assert hist_ids.tolist() == [4, 8, 15, 6] and hist_counts.tolist() == [2, 1, 1, 4]
    assert penalties.dtype == torch.float32 and penalties.tolist() == [[0.5, -0.25, 1.5], [0, 0, 1], [1, 1, 2], [0, 0, 1.25], [0, 0, 1]]
    # one contiguous buffer: the four views alias it
    base = torch.from_numpy(step.buffer)
    assert all(v.untyped_storage().data_ptr() == base.untyped_storage().data_ptr() for v in step.views(base))
    empty = pack_penalty_step([(None, NO_PENALTIES)] * 2)
    ids, counts, cu, pen = empty.views()
    assert empty.total == 0 and ids.numel() == 0 and counts.numel() == 0 and cu.tolist() == [0, 0, 0] and pen.shape == (2, 3)


def _body(**kw):
    return dict({"model": "m", "messages": [{"role": "user", "content": "hi"}], "stream": True}, **kw)


def test_protocol_accepts_the_penalties():
    parse = proto.parse_chat_completion_request
    r = parse(_body())
    assert (r.frequency_penalty, r.presence_penalty, r.repetition_penalty) == (0.0, 0.0, 1.0)
    r = parse(_body(frequency_penalty=None, presence_penalty=None, repetition_penalty=None))
    assert (r.frequency_penalty, r.presence_penalty, r.repetition_penalty) == (0.0, 0.0, 1.0)
    r = parse(_body(frequency_penalty=2, presence_penalty=-2.0, repetition_penalty=1.3))
    assert (r.frequency_penalty, r.presence_penalty, r.repetition_penalty) == (2.0, -2.0, 1.3)
    assert all(isinstance(v, float) for v in (r.frequency_penalty, r.presence_penalty, r.repetition_penalty))
    assert parse(_body(repetition_penalty=0.01)).repetition_penalty == 0.01
    assert parse(_body(logprobs=True, frequency_penalty=0, repetition_penalty=1)).logprobs is True


@pytest.mark.parametrize("bad", [dict(frequency_penalty=2.5), dict(frequency_penalty=-2.01), dict(presence_penalty=3),
                                 dict(presence_penalty="1"), dict(frequency_penalty=True), dict(presence_penalty=[1]),
                                 dict(frequency_penalty=math.nan), dict(presence_penalty=math.inf),
                                 dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty="2"),
                                 dict(repetition_penalty=True), dict(repetition_penalty=math.inf),
                                 dict(repetition_penalty=math.nan), dict(logprobs=True, presence_penalty=0.5),
                                 dict(logprobs=True, repetition_penalty=1.2)], ids=lambda d: json.dumps(d))
def test_protocol_refuses_bad_penalties(bad):
    with pytest.raises(proto.ProtocolError):
        proto.parse_chat_completion_request(_body(**bad))


def _request(**sp):
    return TokenRequest(request_id=3, token_ids=[5, 6, 7], sampling_params=SamplingParameters(max_tokens=2, **sp))


def test_instruction_creator_validates_the_penalties():
    c = InstructionCreator(image_token_id=511, n_image_tokens_per_image=16, block_size=16)
    rcb = c.process(_request())
    sp = rcb.sampling_params
    assert (sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty) == (0.0, 0.0, 1.0)
    assert not is_penalized(sp) and rcb.penalty_history is None
    assert c.process(_request(frequency_penalty=0, presence_penalty=0.0, repetition_penalty=1)).penalty_history is None
    for kw in (dict(frequency_penalty=0.5), dict(presence_penalty=-1), dict(repetition_penalty=1.2),
               dict(frequency_penalty=7.0, presence_penalty=-3.5, repetition_penalty=0.5)):
        rcb = c.process(_request(**kw))
        assert is_penalized(rcb.sampling_params) and isinstance(rcb.penalty_history, PenaltyHistory) and len(rcb.penalty_history) == 0
        for k, v in kw.items():
            assert getattr(rcb.sampling_params, k) == v
    for bad in (dict(frequency_penalty=math.nan), dict(presence_penalty=math.inf), dict(repetition_penalty=-math.inf),
                dict(frequency_penalty="1"), dict(presence_penalty=None), dict(frequency_penalty=True),
                dict(repetition_penalty=False), dict(repetition_penalty=0), dict(repetition_penalty=-0.5)):
        with pytest.raises(ValueError):
            c.process(_request(**bad))
    with pytest.raises(ValueError, match="follow-up"):
        c.process(_request(logprobs=True, top_logprobs=2, repetition_penalty=1.2))
    with pytest.raises(ValueError, match="logprobs"):
        c.process(_request(logprobs=True, presence_penalty=0.1))
    assert c.process(_request(logprobs=True, top_logprobs=2)).sampling_params.logprobs is True


def test_positional_sampling_parameters_are_unchanged():
    """engine/offline.py and engine/distributed.py build SamplingParameters positionally: the new fields come last."""
    sp = SamplingParameters(7, [2], True, 5)
    assert (sp.max_tokens, sp.eos_token_ids, sp.logprobs, sp.top_logprobs) == (7, [2], True, 5)
    assert (sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty) == (0.0, 0.0, 1.0) and not is_penalized(sp)
    sp = SamplingParameters(9, [1, 2])
    assert (sp.max_tokens, sp.eos_token_ids, sp.logprobs, sp.top_logprobs) == (9, [1, 2], False, 0) and not is_penalized(sp)
    assert not is_penalized(SamplingParameters())
    import dataclasses
    assert [f.name for f in dataclasses.fields(SamplingParameters)][:4] == ["max_tokens", "eos_token_ids", "logprobs", "top_logprobs"]
    from hydrainfer_amd.engine.offline import OfflineRequest
    r = OfflineRequest([1, 2], None, 4, (2,), None, True, 3)
    assert (r.max_tokens, r.logprobs, r.top_logprobs, r.frequency_penalty, r.presence_penalty, r.repetition_penalty) == (4, True, 3, 0.0, 0.0, 1.0)


def test_rank_front_end_refuses_penalised_requests():
    from hydrainfer_amd.engine.distributed import RankEngine
    from hydrainfer_amd.entrypoint import RankEngineFrontend
    submitted = []
    engine = NS(submit=lambda *a: submitted.append(a), creator=None)
    front = RankEngineFrontend(engine, InstructionCreator(511, 16, 16))
    for kw in (dict(frequency_penalty=0.5), dict(presence_penalty=0.5), dict(repetition_penalty=1.1)):
        with pytest.raises(ValueError, match="sampling penalties are not available in multi-process serving"):
            front._start(_request(**kw), object())
    assert submitted == []
    front._start(_request(), "p")
    front._start(_request(frequency_penalty=0.0, repetition_penalty=1.0), "p")
    assert len(submitted) == 2
    handlers = {}
    with pytest.raises(ValueError, match="sampling penalties"):
        RankEngine.submit(NS(token_handlers=handlers), _request(repetition_penalty=2.0), "p", None)
    assert handlers == {}


def test_the_op_refuses_cpu_tensors():
    from hydrainfer_amd import _lib
    from hydrainfer_amd.sampling import penalized_argmax_rows
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    with pytest.raises(_lib.HydraHipError, match="CPU tensor"):
        penalized_argmax_rows(torch.zeros((1, 8), dtype=torch.float16), i32(3), i32(1), i32(0, 1),
                              torch.tensor([[0.5, 0.0, 1.0]]))


def test_library_exports_the_new_symbol():
    from hydrainfer_amd import _lib
    assert "hx_penalized_argmax_rows" in _lib.exported_symbols()
    assert _lib.lib().hx_abi_version() == 3
    # the refusals that need no device: checked before anything is launched
    f = _lib.lib().hx_penalized_argmax_rows
    p = 4096        # never dereferenced: every call below is refused before a launch
    assert f(p, None, p, 0, 8, 8, p, p, p, 1, p, _lib.HX_F16, None) == -2
    assert f(p, None, p, 1, 0, 8, p, p, p, 1, p, _lib.HX_F16, None) == -2
    assert f(p, None, p, 1, 8, 7, p, p, p, 1, p, _lib.HX_F16, None) == -2
    assert f(p, None, p, 1, (1 << 18) + 1, 1 << 19, p, p, p, 1, p, _lib.HX_F16, None) == -2
    assert f(p, None, p, 1, 8, 8, p, p, p, -1, p, _lib.HX_F16, None) == -2
    assert f(p, None, p, 1, 8, 8, p, p, p, 1, p, _lib.HX_F32, None) == -1
    for missing in (0, 2, 8, 10):
        args = [p, None, p, 1, 8, 8, p, p, p, 1, p, _lib.HX_F16, None]
        args[missing] = None
        assert f(*args) == -4
    assert f(p, None, p, 1, 8, 8, None, p, p, 1, p, _lib.HX_F16, None) == -4
    assert f(p, None, p, 1, 8, 8, p, None, p, 1, p, _lib.HX_F16, None) == -4
