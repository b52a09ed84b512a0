"""CPU: the host side of token constraints (logit_bias, min_tokens, min_p) — the checks of tests/constraint_ref.py against
its own float64 sampler, value validation, the step packer's layout, TokenConstraints' bans, the API parser, admission in
the engine, and the refusals."""
import json
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.entrypoint import api_protocol as proto
from hydrainfer_amd.sampling import (GREEDY_RECORD, MAX_LOGIT_BIAS, NO_PENALTIES, ConstrainedStep, PenaltyHistory,
                                     TokenConstraints, check_constraints, is_constrained, pack_constrained_step,
                                     pack_sample_records, pack_sample_step)
from tests import constraint_ref as cref
from tests import sampling_ref as ref


def test_checks_accept_the_float64_sampler_and_refuse_its_neighbours():
    g = torch.Generator().manual_seed(17)
    for n, k, p, mp in ((1, 0, 1.0, 0.5), (7, 3, 0.5, 0.1), (1025, 50, 0.9, 0.01), (1025, 0, 0.9, 0.1), (1025, 0, 1.0, 0.5),
                        (1025, 5, 1e-6, 0.5), (64, 65, 0.5, 1.0), (1025, 0, 1.0, 0.0), (1025, 3, 1.0, 0.001)):
        z = (torch.randn(n, generator=g) * 3).to(torch.bfloat16).float().numpy()
        for u in (0.0, 0.37, 0.999999):
            token, cut = cref.reference_sample_constrained(z, k, p, mp, u)
            if mp > 0:
                cref.check_cut_constrained(z, k, p, mp, cut)
            else:
                assert (token, cut) == ref.reference_sample(z, k, p, u)
            ref.check_draw(z, cut, u, token)
    z = np.array([0.0, 3.0, 2.0, 3.0, -1.0, 1.0], dtype=np.float32)      # e = 1 at the 3s, e^-1 = 0.37 at 2, 0.135 at 1, 0.05 at 0
    sample = cref.reference_sample_constrained
    assert sample(z, 0, 1.0, 0.3, 0.0)[1] == 2.0 and sample(z, 0, 1.0, 0.1, 0.0)[1] == 1.0 and sample(z, 0, 1.0, 1.0, 0.9) == (3, 3.0)
    assert sample(z, 1, 1.0, 0.1, 0.0)[1] == 3.0            # top-k cuts higher: v_K' = max(v_K, v_M)
    assert sample(z, 5, 1.0, 0.3, 0.0)[1] == 2.0            # min_p cuts higher
    cref.check_cut_constrained(z, 0, 1.0, 0.3, 2.0)
    with pytest.raises(AssertionError):
        cref.check_cut_constrained(z, 0, 1.0, 0.3, 1.0)     # keeps e = 0.135 < 0.3
    with pytest.raises(AssertionError):
        cref.check_cut_constrained(z, 0, 1.0, 0.3, 3.0)     # drops e = 0.37 >= 0.3 and neither top-k nor top-p explains it
    cref.check_cut_constrained(z, 2, 1.0, 0.3, 3.0)         # top-k explains it
    cref.check_cut_constrained(z, 0, 1e-6, 0.3, 3.0)        # top-p explains it
    # an element on the edge of the band may fall on either side
    edge = np.array([0.0, math.log(0.25)], dtype=np.float32)
    cref.check_cut_constrained(edge, 0, 1.0, 0.25, edge[1])
    cref.check_cut_constrained(edge, 0, 1.0, 0.25, 0.0)
    x = torch.tensor([1.0, 2.0, 3.0]).to(torch.bfloat16)
    assert cref.biased_row(x, [2, 0, 5, -1], [-1.5, 0.25, 9.0, 9.0]).tolist() == [1.25, 2.0, 1.5]
    assert cref.biased_row(x, [1], [-math.inf]).tolist() == [1.0, -math.inf, 3.0]
    # the full row check: bias moves the maximum, the greedy answer follows it
    assert cref.check_row_constrained(x, [0], [5.0], [], [], NO_PENALTIES, (0.0, 1.0, 0, 1, 0, 0.5), 0, math.nan,
                                      ref.uniform(1, 0)) == "greedy"
    assert cref.check_row_constrained(x, [0, 1, 2], [-math.inf] * 3, [], [], NO_PENALTIES, (1.0, 1.0, 0, 1, 0, 0.5), 0,
                                      math.nan, ref.uniform(1, 0)) == "degenerate"


def test_check_constraints():
    assert check_constraints(None, 0, 0) == (None, 0, 0.0)
    assert check_constraints({}, 0, 0.0) == (None, 0, 0.0)
    bias, mt, mp = check_constraints({5: 100, 0: -100.0, 7: 0.5}, 3, 1)
    assert bias == {5: 100.0, 0: -100.0, 7: 0.5} and all(isinstance(v, float) for v in bias.values())
    assert (mt, mp) == (3, 1.0) and isinstance(mp, float)
    assert len(check_constraints({t: 1.0 for t in range(MAX_LOGIT_BIAS)}, 0, 0)[0]) == MAX_LOGIT_BIAS == 300
    for bad in (({-1: 1.0}, 0, 0), ({"5": 1.0}, 0, 0), ({True: 1.0}, 0, 0), ({1.0: 1.0}, 0, 0), ({5: 100.5}, 0, 0),
                ({5: -101}, 0, 0), ({5: math.nan}, 0, 0), ({5: math.inf}, 0, 0), ({5: "1"}, 0, 0), ({5: True}, 0, 0),
                ({5: None}, 0, 0), ([(5, 1.0)], 0, 0), ({t: 1.0 for t in range(MAX_LOGIT_BIAS + 1)}, 0, 0),
                (None, -1, 0), (None, 1.0, 0), (None, True, 0), (None, "1", 0), (None, None, 0),
                (None, 0, -0.1), (None, 0, 1.5), (None, 0, math.nan), (None, 0, "0.5"), (None, 0, True), (None, 0, None)):
        with pytest.raises(ValueError):
            check_constraints(*bad)


def test_is_constrained():
    assert not is_constrained(SamplingParameters())
    assert is_constrained(SamplingParameters(logit_bias={3: 1.0}))
    assert not is_constrained(SamplingParameters(min_p=0.5)) and is_constrained(SamplingParameters(min_p=0.5, temperature=1.0))
    assert not is_constrained(SamplingParameters(min_tokens=2)) and is_constrained(SamplingParameters(min_tokens=2, eos_token_ids=[2]))


def test_record_layout_with_min_p():
    five = pack_sample_records([(0.7, 0.9, 50, 77, 4), GREEDY_RECORD])
    six = pack_sample_records([(0.7, 0.9, 50, 77, 4, 0.25), GREEDY_RECORD, (1.0, 1.0, 0, 1, 2, 0.0)])
    assert five[:, 3].tolist() == [0, 0]                                    # as before
    assert six[:, 3].view(np.float32).tolist() == [0.25, 0.0, 0.0] and six[2, 3] == 0
    assert np.array_equal(np.delete(six[:2], 3, axis=1), np.delete(five, 3, axis=1))


def test_token_constraints_bans_until_min_tokens():
    c = TokenConstraints({9: 1.5, 2: -3.0, 40: 100.0}, [7, 2, 7], 3)
    assert c.ids.dtype == np.int32 and c.values.dtype == np.float32
    assert c.ids.tolist() == [2, 9, 40] and c.values.tolist() == [-3.0, 1.5, 100.0] and c.eos_ids == [2, 7] and c.min_tokens == 3
    for n in (0, 1, 2):
        ids, values = c.step_entries(n)
        assert ids.tolist() == [2, 7, 9, 40] and values.tolist() == [-math.inf, -math.inf, 1.5, 100.0]   # the ban replaces -3.0 on 2
        assert ids.dtype == np.int32 and values.dtype == np.float32 and len(set(ids.tolist())) == len(ids)
    for n in (3, 4, 100):
        ids, values = c.step_entries(n)
        assert ids.tolist() == [2, 9, 40] and values.tolist() == [-3.0, 1.5, 100.0]
    # no end-of-sequence id: min_tokens has nothing to hold back; no bias: the bans alone
    assert TokenConstraints({4: 1.0}, [], 5).step_entries(0)[0].tolist() == [4]
    only = TokenConstraints(None, [11], 1)
    assert only.step_entries(0)[0].tolist() == [11] and only.step_entries(1)[0].size == 0


def test_constrained_step_packer_layout():
    h = PenaltyHistory([4, 8, 4, 15])
    held = TokenConstraints({8: 2.5, 3: -1.0}, [3], 2)
    entries = [(h, (0.5, -0.25, 1.5), (0.7, 0.9, 50, 77, 4, 0.125), held.step_entries(0)),       # ban merged over -1.0 on id 3
               (None, NO_PENALTIES, GREEDY_RECORD, None),                                         # a row with no entries
               (PenaltyHistory([6, 6]), (0.0, 0.0, 1.25), GREEDY_RECORD, held.step_entries(2)),
               (None, NO_PENALTIES, (1.0, 1.0, 0, 1 << 40, 0), (np.zeros(0, np.int32), np.zeros(0, np.float32)))]
    step = pack_constrained_step(entries)
    assert isinstance(step, ConstrainedStep) and (step.rows, step.total, step.bias_total) == (4, 4, 4)
    inner = pack_sample_step([e[:3] for e in entries])
    assert step.buffer.dtype == np.int32 and step.buffer.shape == (inner.buffer.size + 5 + 2 * 4,)
    # SampleStep's buffer, then [cu_bias | bias_ids | bias_values bits]
    assert np.array_equal(step.buffer[:inner.buffer.size], inner.buffer)
    tail = step.buffer[inner.buffer.size:]
    assert tail[:5].tolist() == [0, 2, 2, 4, 4] and tail[5:9].tolist() == [3, 8, 3, 8]
    assert tail[9:].view(np.float32).tolist() == [-math.inf, 2.5, -1.0, 2.5]
    sample_params, bias_ids, bias_values, cu_bias, hist_ids, hist_counts, cu_hist, penalties = step.views()
    assert np.array_equal(sample_params.numpy(), pack_sample_records([e[2] for e in entries]))
    assert sample_params[0, 3].view(torch.float32).item() == 0.125 and sample_params[1:, 3].tolist() == [0, 0, 0]
    assert bias_ids.tolist() == [3, 8, 3, 8] and bias_ids.dtype == torch.int32
    assert bias_values.tolist() == [-math.inf, 2.5, -1.0, 2.5] and bias_values.dtype == torch.float32
    assert cu_bias.tolist() == [0, 2, 2, 4, 4] and cu_bias.dtype == torch.int32
    for got, want in zip((hist_ids, hist_counts, cu_hist, penalties), inner.views()[1:]):
        assert torch.equal(got, want)
    base = torch.from_numpy(step.buffer)
    assert all(v.untyped_storage().data_ptr() == base.untyped_storage().data_ptr() for v in step.views(base))
    assert all(v.is_contiguous() for v in step.views())
    assert all(v.device.type == "cpu" for v in step.to_device("cpu"))
    empty = pack_constrained_step([(None, NO_PENALTIES, GREEDY_RECORD, None)] * 2)
    assert (empty.total, empty.bias_total) == (0, 0) and empty.views()[1].numel() == 0 and empty.views()[3].tolist() == [0, 0, 0]


def _body(**kw):
    return dict({"model": "m", "messages": [{"role": "user", "content": "hi"}], "stream": True}, **kw)


def test_protocol_accepts_the_constraint_fields():
    parse = proto.parse_chat_completion_request
    for r in (parse(_body()), parse(_body(logit_bias=None, min_tokens=None, min_p=None, stop_token_ids=None)),
              parse(_body(logit_bias={}, stop_token_ids=[]))):
        assert (r.logit_bias, r.min_tokens, r.min_p, r.stop_token_ids) == (None, 0, 0.0, None)
    r = parse(_body(logit_bias={"50256": -100, "7": 2.5, "0": 100}, min_tokens=3, min_p=1, stop_token_ids=[2, 9]))
    assert r.logit_bias == {50256: -100.0, 7: 2.5, 0: 100.0} and all(isinstance(v, float) for v in r.logit_bias.values())
    assert (r.min_tokens, r.min_p, r.stop_token_ids) == (3, 1.0, [2, 9]) and isinstance(r.min_p, float)
    assert len(parse(_body(logit_bias={str(t): 1 for t in range(300)})).logit_bias) == 300
    assert parse(_body(stop_token_ids=list(range(16)))).stop_token_ids == list(range(16))
    # logprobs beside fields that are off, prompt_logprobs beside fields that are on
    assert parse(_body(logprobs=True, min_tokens=0, min_p=0, logit_bias={})).logprobs is True
    assert parse(_body(prompt_logprobs=2, logit_bias={"5": 1}, min_tokens=1)).prompt_logprobs == 2
    # a body without the fields parses to today's request: every other field as before, the new ones at their defaults
    plain = parse(_body(max_tokens=5, temperature=0.5, top_k=3))
    assert plain == proto.ChatRequest(model="m", role="user", text="hi", image_png=None, max_tokens=5, stream=True,
                                      temperature=0.5, top_k=3)


@pytest.mark.parametrize("bad", [dict(logit_bias={"5": "1"}), dict(logit_bias={"5": True}), dict(logit_bias={"abc": 1}),
                                 dict(logit_bias={"-1": 1}), dict(logit_bias={"1.0": 1}), dict(logit_bias={" 5": 1}),
                                 dict(logit_bias={"+5": 1}), dict(logit_bias={"5": 100.5}), dict(logit_bias={"5": -101}),
                                 dict(logit_bias={"5": math.nan}), dict(logit_bias={"5": None}), dict(logit_bias=[["5", 1]]),
                                 dict(logit_bias="5"), dict(logit_bias={"5": 1, "05": 2}),
                                 dict(logit_bias={str(t): 1 for t in range(301)}),
                                 dict(min_tokens=-1), dict(min_tokens=1.0), dict(min_tokens="1"), dict(min_tokens=True),
                                 dict(min_p=1.5), dict(min_p=-0.1), dict(min_p="0.5"), dict(min_p=True), dict(min_p=math.nan),
                                 dict(stop_token_ids=[-1]), dict(stop_token_ids=[1.0]), dict(stop_token_ids=["2"]),
                                 dict(stop_token_ids=[True]), dict(stop_token_ids=2), dict(stop_token_ids=list(range(17))),
                                 dict(logprobs=True, logit_bias={"5": 1}), dict(logprobs=True, min_tokens=1),
                                 dict(logprobs=True, min_p=0.1)],
                         ids=lambda d: json.dumps(d)[:60])
def test_protocol_refuses_bad_constraint_fields(bad):
    with pytest.raises(proto.ProtocolError):
        proto.parse_chat_completion_request(_body(**bad))


def _request(max_tokens=4, **sp):
    return TokenRequest(request_id=3, token_ids=[5, 6, 7], sampling_params=SamplingParameters(max_tokens=max_tokens, **sp))


def test_admission():
    c = InstructionCreator(image_token_id=511, n_image_tokens_per_image=16, block_size=16)
    rcb = c.process(_request())
    sp = rcb.sampling_params
    assert (sp.logit_bias, sp.min_tokens, sp.min_p) == (None, 0, 0.0) and rcb.token_constraints is None
    rcb = c.process(_request(logit_bias={9: 1, 4: -100}, min_tokens=2, eos_token_ids=[6], min_p=0.25, temperature=1.0))
    sp, tc = rcb.sampling_params, rcb.token_constraints
    assert sp.logit_bias == {9: 1.0, 4: -100.0} and (sp.min_tokens, sp.min_p) == (2, 0.25)
    assert isinstance(tc, TokenConstraints) and tc.ids.tolist() == [4, 9] and tc.eos_ids == [6] and tc.min_tokens == 2
    # the fields that have no effect are accepted, and the request stays on its old paths
    assert c.process(_request(min_p=0.5)).token_constraints is None                   # greedy: min_p is ignored
    assert c.process(_request(min_tokens=3)).token_constraints is None                # ignore_eos and no id of its own
    assert c.process(_request(logit_bias={})).token_constraints is None
    assert c.process(_request(min_p=0.5, temperature=0.5)).token_constraints is not None
    assert c.process(_request(min_tokens=3, eos_token_ids=[2])).token_constraints is not None
    # the server's own end-of-sequence id is held back too
    with_eos = InstructionCreator(image_token_id=511, n_image_tokens_per_image=16, block_size=16, ignore_eos=False, eos_token_id=2)
    tc = with_eos.process(_request(min_tokens=1, eos_token_ids=[8])).token_constraints
    assert tc.eos_ids == [2, 8] and tc.step_entries(0)[0].tolist() == [2, 8]
    # vocab_size: unchecked by default, refused at or above it
    assert c.process(_request(logit_bias={100000: 1.0})).token_constraints is not None
    assert c.process(_request(logit_bias={511: 1.0}), vocab_size=512).token_constraints is not None
    with pytest.raises(ValueError, match="request 3: logit_bias names token 512"):
        c.process(_request(logit_bias={3: 1.0, 512: 1.0}), vocab_size=512)
    with pytest.raises(ValueError, match="request 3: min_tokens 5 exceeds max_tokens 4"):
        c.process(_request(min_tokens=5, eos_token_ids=[2]))
    assert c.process(_request(min_tokens=4, eos_token_ids=[2])).token_constraints is not None
    for bad in (dict(logit_bias={-1: 1.0}), dict(logit_bias={5: 101}), dict(logit_bias={5: True}), dict(min_tokens=-1),
                dict(min_tokens=1.5), dict(min_p=1.5), dict(min_p=-1), dict(min_p=math.nan)):
        with pytest.raises(ValueError, match="request 3: "):
            c.process(_request(**bad))
    for fields in (dict(logit_bias={5: 1.0}), dict(min_tokens=1), dict(min_p=0.5)):
        with pytest.raises(ValueError, match="request 3: .*logprobs.*raw"):
            c.process(_request(logprobs=True, **fields))
    assert c.process(_request(prompt_logprobs=1, logit_bias={5: 1.0})).token_constraints is not None
    # the caller's object is not touched
    req = _request(logit_bias={9: 1})
    c.process(req)
    assert req.sampling_params.logit_bias == {9: 1}


def test_positional_construction_is_unchanged():
    sp = SamplingParameters(7, [2], True, 5, 0.5, 0.25, 1.5, 0.7, 0.9, 50, 11, 3)
    assert (sp.max_tokens, sp.eos_token_ids, sp.logprobs, sp.top_logprobs, sp.frequency_penalty, sp.presence_penalty,
            sp.repetition_penalty, sp.temperature, sp.top_p, sp.top_k, sp.seed, sp.prompt_logprobs) \
        == (7, [2], True, 5, 0.5, 0.25, 1.5, 0.7, 0.9, 50, 11, 3)
    assert (sp.logit_bias, sp.min_tokens, sp.min_p) == (None, 0, 0.0)
    from hydrainfer_amd.engine.offline import OfflineRequest
    r = OfflineRequest([1, 2], None, 4, (2,), None, True, 3, 0.5, 0.25, 1.5, 0.7, 0.9, 50, 11, 2)
    assert (r.max_tokens, r.eos_token_ids, r.logprobs, r.top_logprobs, r.repetition_penalty, r.seed, r.prompt_logprobs) \
        == (4, (2,), True, 3, 1.5, 11, 2)
    assert (r.logit_bias, r.min_tokens, r.min_p) == (None, 0, 0.0)
    r = OfflineRequest([1, 2], logit_bias={5: 1.0}, min_tokens=2, min_p=0.1)
    assert (r.logit_bias, r.min_tokens, r.min_p) == ({5: 1.0}, 2, 0.1)
    # the new fields are keyword-only: one positional argument more than before is refused, not taken for logit_bias
    import dataclasses
    with pytest.raises(TypeError):
        SamplingParameters(7, [2], True, 5, 0.5, 0.25, 1.5, 0.7, 0.9, 50, 11, 3, {5: 1.0})
    with pytest.raises(TypeError):
        OfflineRequest([1, 2], None, 4, (2,), None, True, 3, 0.5, 0.25, 1.5, 0.7, 0.9, 50, 11, 2, {5: 1.0})
    for cls, new in ((SamplingParameters, 3), (OfflineRequest, 3), (proto.ChatRequest, 4)):
        assert sum(f.kw_only for f in dataclasses.fields(cls)) == new


def test_multi_process_serving_refuses_constraints():
    from hydrainfer_amd.engine.distributed import RankEngine, refuse_constraints
    from hydrainfer_amd.entrypoint import RankEngineFrontend
    refuse_constraints(_request())
    refuse_constraints(_request(temperature=0.5, top_k=3, eos_token_ids=[2]))
    refuse_constraints(NS(request_id=1))
    for fields in (dict(logit_bias={5: 1.0}), dict(min_tokens=1), dict(min_p=0.5)):
        with pytest.raises(ValueError, match="logit_bias / min_tokens / min_p are not available in multi-process serving"):
            refuse_constraints(_request(**fields))
    submitted = []
    front = RankEngineFrontend(NS(submit=lambda *a: submitted.append(a), creator=None), InstructionCreator(511, 16, 16))
    with pytest.raises(ValueError, match="multi-process serving"):
        front._start(_request(logit_bias={5: 1.0}), object())
    assert submitted == []
    front._start(_request(), "p")
    assert len(submitted) == 1
    handlers = {}
    with pytest.raises(ValueError, match="multi-process serving"):
        RankEngine.submit(NS(token_handlers=handlers), _request(min_tokens=1, eos_token_ids=[2]), "p", None)
    assert handlers == {}


def test_tokenizers_name_a_vocabulary_size():
    from hydrainfer_amd.entrypoint.tokenizer import SyntheticTokenizer
    assert SyntheticTokenizer().vocab_size == 32001 and SyntheticTokenizer(image_token_id=511, lo=3, hi=511).vocab_size == 512
    assert SyntheticTokenizer(vocab_size=32064).vocab_size == 32064


def test_the_op_refuses_cpu_tensors():
    from hydrainfer_amd import _lib
    from hydrainfer_amd.sampling import sample_rows_constrained
    step = pack_constrained_step([(None, NO_PENALTIES, GREEDY_RECORD, None)])
    with pytest.raises(_lib.HydraHipError, match="CPU tensor"):
        sample_rows_constrained(torch.zeros((1, 8), dtype=torch.float16), *step.views()[:4])


def test_library_exports_the_symbol_and_refuses_before_a_launch():
    from hydrainfer_amd import _lib
    from hydrainfer_amd.sampling import SAMPLE_MAX_N
    assert "hx_sample_rows_constrained" in _lib.exported_symbols()
    assert _lib.lib().hx_abi_version() == 3
    f = _lib.lib().hx_sample_rows_constrained
    p = 4096        # never dereferenced: every call below is refused before a launch
    #     ids cut   u     logits rows n ld hist...  total pen bias...  bias_total records dtype stream
    ok = [p, None, None, p, 1, 8, 8, p, p, p, 1, p, p, p, p, 1, p, _lib.HX_F16, None]
    for at, v in ((4, 0), (5, 0), (6, 7), (5, SAMPLE_MAX_N + 1), (10, -1), (15, -1), (15, 1 << 31), (10, 1 << 31)):
        args = list(ok)
        args[at] = v
        if at == 5:
            args[6] = max(v, 8)
        assert f(*args) == -2, (at, v)
    assert f(*(ok[:17] + [_lib.HX_F32, None])) == -1
    for missing in (0, 3, 16, 7, 8, 9, 11, 12, 13, 14):
        args = list(ok)
        args[missing] = None
        assert f(*args) == -4, missing
