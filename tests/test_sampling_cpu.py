"""CPU: the host side of sampled decoding — Philox4x32-10 of tests/sampling_ref.py against Random123's known answers,
the checks of sampling_ref against a float64 sampler, the record / step packer, parameter validation in the engine and in
the API parser, seed assignment at admission, and the refusals."""
import json
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.entrypoint import api_protocol as proto
from hydrainfer_amd.sampling import (GREEDY_RECORD, MAX_SEED, NO_PENALTIES, SAMPLE_MAX_N, PenaltyHistory, check_sampling,
                                     is_penalized, is_sampled, pack_penalty_step, pack_sample_records, pack_sample_step)
from tests import sampling_ref as ref


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{w:08x}" for w in ref.philox4x32_10(counter, key)) == want


def test_uniform_is_the_top_24_bits():
    assert ref.uniform(0, 0) == np.float32(0x6627e8 / 2 ** 24)
    us = [ref.uniform(s, o) for s in (1, (1 << 40) + 3, MAX_SEED) for o in (0, 1, (1 << 32) + 5)]
    assert all(0.0 <= u < 1.0 and u.dtype == np.float32 for u in us) and len(set(us)) == len(us)
    # the high words matter
    assert ref.uniform(1 << 32, 0) != ref.uniform(0, 0) != ref.uniform(0, 1 << 32)


def test_checks_accept_the_float64_sampler_and_refuse_its_neighbours():
    g = torch.Generator().manual_seed(11)
    for n, k, p in ((1, 0, 1.0), (7, 3, 0.5), (1025, 50, 0.9), (1025, 0, 0.9), (1025, 0, 1.0), (1025, 5, 1e-6), (64, 65, 0.5)):
        z = (torch.randn(n, generator=g) * 3).to(torch.bfloat16).float().numpy()
        for u in (0.0, 0.37, 0.999999):
            token, cut = ref.reference_sample(z, k, p, u)
            ref.check_cut(z, k, p, cut)
            ref.check_draw(z, cut, u, token)
    z = np.array([1.0, 3.0, 2.0, 3.0, -1.0, 0.0], dtype=np.float32)
    # ties stand together: k = 1 keeps both 3s; the draw goes by index order
    assert ref.reference_sample(z, 1, 1.0, 0.25) == (1, 3.0) and ref.reference_sample(z, 1, 1.0, 0.75) == (3, 3.0)
    assert ref.reference_sample(z, 3, 1.0, 0.0)[1] == 2.0 and ref.reference_sample(z, 0, 1.0, 0.0)[1] == -1.0
    assert ref.reference_sample(z, 0, 1e-6, 0.9) == (3, 3.0)
    with pytest.raises(AssertionError):
        ref.check_cut(z, 1, 1.0, 2.0)            # top_p >= 1: the cut is v_K exactly
    with pytest.raises(AssertionError):
        ref.check_cut(z, 0, 1.0, 2.5)            # no value of the row
    with pytest.raises(AssertionError):
        ref.check_cut(z, 0, 0.5, 0.0)            # far more than half the mass above it
    with pytest.raises(AssertionError):
        ref.check_cut(z, 0, 0.99, 3.0)           # 2.0 would still do
    with pytest.raises(AssertionError):
        ref.check_draw(z, 3.0, 0.25, 3)          # u = 0.25 is the first 3's
    with pytest.raises(AssertionError):
        ref.check_draw(z, 3.0, 0.25, 2)          # not in S


def test_record_layout():
    rec = pack_sample_records([(0.7, 0.9, 50, (1 << 63) - 1, (1 << 32) + 5), GREEDY_RECORD, (1.5, 1.0, 0, 0x123456789, 2)])
    assert rec.dtype == np.int32 and rec.shape == (3, 8)
    assert rec[:, :2].view(np.float32).tolist() == [[np.float32(0.7), np.float32(0.9)], [0.0, 1.0], [1.5, 1.0]]
    assert rec[:, 2].tolist() == [50, 0, 0] and rec[:, 3].tolist() == [0, 0, 0]
    assert rec[:, 4:].view(np.uint32).tolist() == [[0xffffffff, 0x7fffffff, 5, 1], [0, 0, 0, 0], [0x23456789, 1, 2, 0]]


def test_step_packer_one_buffer():
    a = PenaltyHistory([4, 8, 4, 15])
    entries = [(a, (0.5, -0.25, 1.5), (0.7, 0.9, 50, 77, 4)), (None, NO_PENALTIES, GREEDY_RECORD),
               (PenaltyHistory([6, 6]), (0.0, 0.0, 1.25), GREEDY_RECORD), (None, NO_PENALTIES, (1.0, 1.0, 0, 1 << 40, 0))]
    step = pack_sample_step(entries)
    assert (step.rows, step.total) == (4, 4) and step.buffer.dtype == np.int32 and step.buffer.shape == (8 * 4 + 4 * 4 + 1 + 8,)
    sample_params, hist_ids, hist_counts, cu_hist, penalties = step.views()
    assert np.array_equal(sample_params.numpy(), pack_sample_records([e[2] for e in entries]))
    # behind the records: pack_penalty_step's layout, unchanged
    assert np.array_equal(step.buffer[32:], pack_penalty_step([(h, p) for h, p, _ in entries]).buffer)
    assert cu_hist.tolist() == [0, 3, 3, 4, 4] and hist_ids.tolist() == [4, 8, 15, 6] and hist_counts.tolist() == [2, 1, 1, 2]
    assert penalties.tolist() == [[0.5, -0.25, 1.5], [0, 0, 1], [0, 0, 1.25], [0, 0, 1]]
    assert sample_params.is_contiguous() and sample_params.dtype == torch.int32 and penalties.dtype == torch.float32
    base = torch.from_numpy(step.buffer)
    assert all(v.untyped_storage().data_ptr() == base.untyped_storage().data_ptr() for v in step.views(base))
    empty = pack_sample_step([(None, NO_PENALTIES, GREEDY_RECORD)] * 2)
    assert empty.total == 0 and empty.views()[1].numel() == 0 and empty.views()[3].tolist() == [0, 0, 0]


def test_check_sampling():
    assert check_sampling(0, 1, 0, None) == (0.0, 1.0, 0, None)
    got = check_sampling(0.7, 0.9, 50, MAX_SEED)
    assert got == (0.7, 0.9, 50, MAX_SEED) and isinstance(got[0], float) and isinstance(got[1], float)
    assert check_sampling(100.0, 1e-9, 1 << 20, 0) == (100.0, 1e-9, 1 << 20, 0)
    for bad in ((-0.1, 1, 0, None), (math.nan, 1, 0, None), (math.inf, 1, 0, None), ("1", 1, 0, None), (True, 1, 0, None),
                (None, 1, 0, None), (1, 0, 0, None), (1, 1.01, 0, None), (1, math.nan, 0, None), (1, "0.5", 0, None),
                (1, True, 0, None), (1, 1, -1, None), (1, 1, 1.0, None), (1, 1, True, None), (1, 1, "3", None),
                (1, 1, 0, -1), (1, 1, 0, MAX_SEED + 1), (1, 1, 0, 1.0), (1, 1, 0, True), (1, 1, 0, "7")):
        with pytest.raises(ValueError):
            check_sampling(*bad)


def test_defaults_are_greedy():
    sp = SamplingParameters()
    assert (sp.temperature, sp.top_p, sp.top_k, sp.seed) == (0.0, 1.0, 0, None) and not is_sampled(sp) and not is_penalized(sp)
    assert is_sampled(SamplingParameters(temperature=0.01)) and not is_sampled(SamplingParameters(top_p=0.5, top_k=5, seed=3))
    # positional construction as before: the new fields come last
    sp = SamplingParameters(7, [2], True, 5, 0.5, 0.25, 1.5)
    assert (sp.max_tokens, sp.repetition_penalty, sp.temperature, sp.seed) == (7, 1.5, 0.0, None)
    from hydrainfer_amd.engine.offline import OfflineRequest
    r = OfflineRequest([1, 2], None, 4)
    assert (r.temperature, r.top_p, r.top_k, r.seed) == (0.0, 1.0, 0, None)
    r = OfflineRequest([1, 2], None, 4, temperature=0.7, top_p=0.9, top_k=50, seed=5)
    assert (r.temperature, r.top_p, r.top_k, r.seed) == (0.7, 0.9, 50, 5)
    assert SAMPLE_MAX_N >= 32064


def _body(**kw):
    return dict({"model": "m", "messages": [{"role": "user", "content": "hi"}], "stream": True}, **kw)


def test_protocol_accepts_the_sampling_fields():
    parse = proto.parse_chat_completion_request
    for r in (parse(_body()), parse(_body(temperature=None, top_p=None, top_k=None, seed=None))):
        assert (r.temperature, r.top_p, r.top_k, r.seed) == (0.0, 1.0, 0, None)
    r = parse(_body(temperature=2, top_p=1, top_k=0, seed=0))
    assert (r.temperature, r.top_p, r.top_k, r.seed) == (2.0, 1.0, 0, 0) and isinstance(r.temperature, float) and isinstance(r.top_p, float)
    r = parse(_body(temperature=0.7, top_p=0.9, top_k=50, seed=(1 << 63) - 1))
    assert (r.temperature, r.top_p, r.top_k, r.seed) == (0.7, 0.9, 50, (1 << 63) - 1)
    assert parse(_body(logprobs=True, temperature=0, top_p=0.5, seed=4)).logprobs is True
    assert parse(_body(temperature=1.0, frequency_penalty=0.5)).frequency_penalty == 0.5


@pytest.mark.parametrize("bad", [dict(temperature=-0.1), dict(temperature=2.01), dict(temperature="1"), dict(temperature=True),
                                 dict(temperature=math.nan), dict(temperature=[1]), dict(top_p=0), dict(top_p=1.01),
                                 dict(top_p=-0.5), dict(top_p="0.9"), dict(top_p=True), dict(top_p=math.nan),
                                 dict(top_k=-1), dict(top_k=1.0), dict(top_k="5"), dict(top_k=True), dict(seed=-1),
                                 dict(seed=1 << 63), dict(seed=1.0), dict(seed="7"), dict(seed=True),
                                 dict(logprobs=True, temperature=0.5)], ids=lambda d: json.dumps(d))
def test_protocol_refuses_bad_sampling_fields(bad):
    with pytest.raises(proto.ProtocolError):
        proto.parse_chat_completion_request(_body(**bad))


def _request(**sp):
    return TokenRequest(request_id=3, token_ids=[5, 6, 7], sampling_params=SamplingParameters(max_tokens=2, **sp))


def test_admission_validates_and_assigns_a_seed():
    c = InstructionCreator(image_token_id=511, n_image_tokens_per_image=16, block_size=16)
    sp = c.process(_request()).sampling_params
    assert not is_sampled(sp) and sp.seed is None
    # a greedy request keeps what it was given and gets no seed
    sp = c.process(_request(top_p=0.5, top_k=4)).sampling_params
    assert (sp.temperature, sp.top_p, sp.top_k, sp.seed) == (0.0, 0.5, 4, None)
    sp = c.process(_request(temperature=0.7, top_p=0.9, top_k=50, seed=12345)).sampling_params
    assert (sp.temperature, sp.top_p, sp.top_k, sp.seed) == (0.7, 0.9, 50, 12345) and is_sampled(sp)
    seeds = [c.process(_request(temperature=1.0)).sampling_params.seed for _ in range(8)]
    assert all(isinstance(s, int) and 0 <= s <= MAX_SEED for s in seeds) and len(set(seeds)) == 8
    assert max(seeds) >= 1 << 40, "63 random bits: eight seeds all below 2^40 do not happen"
    req = _request(temperature=1.0)
    assert c.process(req).sampling_params.seed is not None and req.sampling_params.seed is None   # the caller's object is not touched
    # sampled and penalised together
    rcb = c.process(_request(temperature=1.0, repetition_penalty=1.2))
    assert is_sampled(rcb.sampling_params) and isinstance(rcb.penalty_history, PenaltyHistory)
    for bad in (dict(temperature=-1.0), dict(temperature=math.nan), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-2),
                dict(top_k=2.0), dict(seed=-1), dict(seed=1 << 63), dict(temperature="1")):
        with pytest.raises(ValueError):
            c.process(_request(**bad))
    with pytest.raises(ValueError, match="logprobs"):
        c.process(_request(logprobs=True, temperature=0.5))
    assert c.process(_request(logprobs=True, top_logprobs=2, temperature=0.0, top_p=0.5)).sampling_params.logprobs is True


def test_rank_front_end_refuses_sampled_requests():
    from hydrainfer_amd.engine.distributed import RankEngine
    from hydrainfer_amd.entrypoint import RankEngineFrontend
    submitted = []
    engine = NS(submit=lambda *a: submitted.append(a), creator=None)
    front = RankEngineFrontend(engine, InstructionCreator(511, 16, 16))
    with pytest.raises(ValueError, match="sampled decoding .* is not available in multi-process serving"):
        front._start(_request(temperature=0.5), object())
    assert submitted == []
    front._start(_request(top_p=0.5, seed=3), "p")
    assert len(submitted) == 1
    handlers = {}
    with pytest.raises(ValueError, match="sampled decoding"):
        RankEngine.submit(NS(token_handlers=handlers), _request(temperature=1.0, seed=1), "p", None)
    assert handlers == {}


def test_the_op_refuses_cpu_tensors():
    from hydrainfer_amd import _lib
    from hydrainfer_amd.sampling import sample_rows
    with pytest.raises(_lib.HydraHipError, match="CPU tensor"):
        sample_rows(torch.zeros((1, 8), dtype=torch.float16), torch.from_numpy(pack_sample_records([GREEDY_RECORD])))


def test_library_exports_the_new_symbol():
    from hydrainfer_amd import _lib
    assert "hx_sample_rows" in _lib.exported_symbols()
    assert _lib.lib().hx_abi_version() == 3
    # the refusals that need no device: checked before anything is launched
    f = _lib.lib().hx_sample_rows
    p = 4096        # never dereferenced: every call below is refused before a launch
    ok = [p, None, None, p, 1, 8, 8, p, p, p, 1, p, p, _lib.HX_F16, None]
    for at, v in ((4, 0), (5, 0), (6, 7), (5, SAMPLE_MAX_N + 1), (10, -1)):
        args = list(ok)
        args[at] = v
        if at == 5:
            args[6] = max(v, 8)
        assert f(*args) == -2, (at, v)
    assert f(*(ok[:13] + [_lib.HX_F32, None])) == -1
    for missing in (0, 3, 12, 7, 8, 9, 11):
        args = list(ok)
        args[missing] = None
        assert f(*args) == -4, missing
