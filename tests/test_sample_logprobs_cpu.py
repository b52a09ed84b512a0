"""CPU: the host side of processed log-probabilities (logprobs_mode = "processed_logprobs") — the API parser and admission
(what the mode opens, and that without it every refusal stands), the executor's scored_rows decision against a literal
table, the C ABI binding, the new kernel's code-object rows (no scratch, no spills, wave64) and the float64 reference of
tests/sample_logprob_ref.py against hand-computed rows."""
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.engine.executor import SAMPLING_MODES, scored_rows, step_mode
from hydrainfer_amd.entrypoint import api_protocol as proto
from hydrainfer_amd.sampling import PenaltyHistory, TokenConstraints
from tests import sample_logprob_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROCESSED, RAW = "processed_logprobs", "raw_logprobs"
FAMILIES = {"sampling": dict(temperature=0.7, top_p=0.9, top_k=40, seed=5),
            "penalties": dict(frequency_penalty=0.5, presence_penalty=0.25, repetition_penalty=1.3),
            "constraints": dict(logit_bias={"5": 1.5}, min_tokens=1, min_p=0.1)}
ALL = {k: v for f in FAMILIES.values() for k, v in f.items()}


def _body(**extra):
    return dict({"model": "m", "messages": [{"role": "user", "content": "hi"}], "stream": True}, **extra)


def _request(max_tokens=4, **sp):
    return TokenRequest(request_id=3, token_ids=[5, 6, 7], sampling_params=SamplingParameters(max_tokens=max_tokens, **sp))


def _engine_fields(fields):
    out = dict(fields)
    if "logit_bias" in out:
        out["logit_bias"] = {int(t): b for t, b in out["logit_bias"].items()}
    if "min_tokens" in out:
        out["eos_token_ids"] = [2]
    return out


@pytest.mark.parametrize("fields", list(FAMILIES.values()) + [ALL], ids=list(FAMILIES) + ["all"])
def test_protocol_accepts_the_mode_with_every_family(fields):
    r = proto.parse_chat_completion_request(_body(logprobs=True, top_logprobs=3, logprobs_mode=PROCESSED, **fields))
    assert r.logprobs is True and r.top_logprobs == 3 and r.logprobs_mode == PROCESSED
    r = proto.parse_chat_completion_request(_body(logprobs=True, logprobs_mode=PROCESSED, prompt_logprobs=2, **fields))
    assert r.prompt_logprobs == 2


@pytest.mark.parametrize("fields", list(FAMILIES.values()) + [ALL], ids=list(FAMILIES) + ["all"])
@pytest.mark.parametrize("mode", [None, RAW])
def test_protocol_without_the_mode_refuses_what_it_refused(mode, fields):
    extra = {} if mode is None else {"logprobs_mode": mode}
    with pytest.raises(proto.ProtocolError, match="logprobs cannot be combined"):
        proto.parse_chat_completion_request(_body(logprobs=True, **extra, **fields))
    # and accepts what it accepted: the fields without logprobs, logprobs without the fields
    assert proto.parse_chat_completion_request(_body(**extra, **fields)).logprobs is False
    assert proto.parse_chat_completion_request(_body(logprobs=True, top_logprobs=2, **extra)).logprobs_mode == mode


@pytest.mark.parametrize("bad", [dict(logprobs_mode="processed"), dict(logprobs_mode="raw_logits"), dict(logprobs_mode=1),
                                 dict(logprobs_mode=True), dict(logprobs_mode=[PROCESSED]), dict(logprobs_mode=""),
                                 dict(logprobs_mode=PROCESSED), dict(logprobs_mode=PROCESSED, logprobs=False),
                                 dict(logprobs_mode=PROCESSED, temperature=0.5)], ids=str)
def test_protocol_refuses_a_bad_mode_and_the_mode_without_logprobs(bad):
    with pytest.raises(proto.ProtocolError, match="logprobs_mode"):
        proto.parse_chat_completion_request(_body(**bad))


def test_a_body_without_the_field_parses_to_the_same_request():
    plain = proto.parse_chat_completion_request(_body(max_tokens=5, logprobs=True, top_logprobs=2))
    assert plain.logprobs_mode is None
    assert plain == proto.ChatRequest(model="m", role="user", text="hi", image_png=None, max_tokens=5, stream=True,
                                      logprobs=True, top_logprobs=2)
    assert proto.parse_chat_completion_request(_body(logprobs_mode=RAW)).logprobs_mode == RAW     # (raw needs no logprobs)


@pytest.mark.parametrize("fields", list(FAMILIES.values()) + [ALL], ids=list(FAMILIES) + ["all"])
def test_admission_accepts_the_mode_with_every_family(fields):
    c = InstructionCreator(image_token_id=511, n_image_tokens_per_image=16, block_size=16)
    f = _engine_fields(fields)
    rcb = c.process(_request(logprobs=True, top_logprobs=4, logprobs_mode=PROCESSED, prompt_logprobs=1, **f))
    sp = rcb.sampling_params
    assert sp.logprobs and sp.logprobs_mode == PROCESSED and sp.top_logprobs == 4
    # set up as for any such request
    assert (rcb.penalty_history is not None) == ("frequency_penalty" in f) and (rcb.token_constraints is not None) == ("logit_bias" in f)
    if "frequency_penalty" in f:
        assert isinstance(rcb.penalty_history, PenaltyHistory)
    if "logit_bias" in f:
        assert isinstance(rcb.token_constraints, TokenConstraints) and rcb.token_constraints.ids.tolist() == [5]
    if "temperature" in f:
        assert sp.seed == 5
        unseeded = c.process(_request(logprobs=True, logprobs_mode=PROCESSED, temperature=0.5)).sampling_params
        assert isinstance(unseeded.seed, int)
    # a greedy, unadjusted request may ask for the mode too
    assert c.process(_request(logprobs=True, logprobs_mode=PROCESSED)).sampling_params.logprobs_mode == PROCESSED


@pytest.mark.parametrize("fields", list(FAMILIES.values()) + [ALL], ids=list(FAMILIES) + ["all"])
@pytest.mark.parametrize("mode", [None, RAW])
def test_admission_without_the_mode_refuses_what_it_refused(mode, fields):
    c = InstructionCreator(image_token_id=511, n_image_tokens_per_image=16, block_size=16)
    f = _engine_fields(fields)
    with pytest.raises(ValueError, match="request 3: .*cannot be.* combined with.*logprobs yet"):
        c.process(_request(logprobs=True, logprobs_mode=mode, **f))
    assert c.process(_request(logprobs_mode=mode, **f)).sampling_params.logprobs_mode == mode
    assert c.process(_request(logprobs=True, logprobs_mode=mode)).sampling_params.logprobs is True


def test_admission_refuses_a_bad_mode_and_the_mode_without_logprobs():
    c = InstructionCreator(image_token_id=511, n_image_tokens_per_image=16, block_size=16)
    for bad in ("processed", "raw", 1, True, ""):
        with pytest.raises(ValueError, match="request 3: logprobs_mode"):
            c.process(_request(logprobs=True, logprobs_mode=bad))
    with pytest.raises(ValueError, match="request 3: logprobs_mode = 'processed_logprobs' needs logprobs"):
        c.process(_request(logprobs_mode=PROCESSED, temperature=0.5))
    from hydrainfer_amd.engine.offline import OfflineRequest
    assert OfflineRequest([1, 2], logprobs=True, logprobs_mode=PROCESSED).logprobs_mode == PROCESSED
    assert OfflineRequest([1, 2]).logprobs_mode is None and SamplingParameters().logprobs_mode is None
    with pytest.raises(TypeError):                                       # keyword-only, prompt_logprobs stays the last positional
        SamplingParameters(7, [2], True, 5, 0.5, 0.25, 1.5, 0.7, 0.9, 50, 11, 3, PROCESSED)


def test_multi_process_serving_still_turns_them_away():
    from hydrainfer_amd.engine.distributed import refuse_logprobs
    refuse_logprobs(_request())
    with pytest.raises(ValueError, match="logprobs are not available in multi-process serving"):
        refuse_logprobs(_request(logprobs=True, logprobs_mode=PROCESSED, temperature=0.5))


def _row(logprobs=False, mode="absent", chunk=False, top=0, temperature=0.0, penalised=False, constrained=False):
    sp = NS(logprobs=logprobs, top_logprobs=top, temperature=temperature)
    if mode != "absent":
        sp.logprobs_mode = mode
    return (NS(sampling_params=sp, penalty_history=object() if penalised else None,
               token_constraints=object() if constrained else None), NS(is_chunked=chunk))


SCORED_TABLE = [
    ([], False),
    ([_row()], False),
    ([_row(logprobs=True)], False),                                      # a stand-in without the field: raw
    ([_row(logprobs=True, mode=None)], False),
    ([_row(logprobs=True, mode=RAW, top=3)], False),
    ([_row(logprobs=True, mode=PROCESSED)], True),
    ([_row(logprobs=False, mode=PROCESSED)], False),                     # (admission refuses it; the decision reads both)
    ([_row(logprobs=True, mode=PROCESSED, chunk=True)], False),          # a chunk head's sample is discarded
    ([_row(logprobs=True, mode=PROCESSED, chunk=True), _row(logprobs=True, mode=PROCESSED, temperature=0.5)], True),
    ([_row(), _row(temperature=0.7), _row(penalised=True), _row(constrained=True)], False),
    ([_row(), _row(temperature=0.7), _row(penalised=True), _row(constrained=True), _row(logprobs=True, mode=RAW)], False),
    ([_row(), _row(temperature=0.7), _row(logprobs=True, mode=RAW), _row(logprobs=True, mode=PROCESSED, penalised=True)], True),
    ([_row(logprobs=True, mode=PROCESSED, chunk=True), _row(logprobs=True, mode=RAW)], False),
]


@pytest.mark.parametrize("rows,want", SCORED_TABLE, ids=[str(i) for i in range(len(SCORED_TABLE))])
def test_scored_rows(rows, want):
    assert scored_rows(rows) is want


def test_step_mode_and_its_table_are_what_they_were():
    assert set(SAMPLING_MODES) == {"constrained", "drawn", "penalised"}
    rows = [_row(logprobs=True, mode=PROCESSED, top=4, temperature=0.5), _row(logprobs=True, top=2)]
    assert step_mode(rows) == ("drawn", 4)          # step_mode does not know the mode: scored_rows is consulted first


def test_c_abi_binding():
    assert "hx_sample_rows_logprobs" in _lib.exported_symbols()
    assert "hx_sample_rows_logprobs" in open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    f = _lib.lib().hx_sample_rows_logprobs
    assert len(f.argtypes) == 24
    # top_k outside 0..20, then the shared checks, then the score pointers: nothing needs a GPU to be refused
    SHAPE, NULL = -2, -4
    args = [1, None, None, 1, 1, 8, 8, None, None, None, 0, None, None, None, None, 0, 1, 1, 1, 1, 21, None, _lib.HX_F16, None]
    assert f(*args) == SHAPE
    args[20] = 3
    args[17] = None
    assert f(*args) == NULL
    args[17], args[18] = 1, None
    assert f(*args) == NULL
    args[18], args[4] = 1, 0
    assert f(*args) == SHAPE


def test_wrapper_refuses_cpu_tensors():
    from hydrainfer_amd.sampling import NO_PENALTIES, GREEDY_RECORD, pack_constrained_step, sample_rows_logprobs
    step = pack_constrained_step([(None, NO_PENALTIES, GREEDY_RECORD, None)])
    with pytest.raises(_lib.HydraHipError, match="CPU tensor"):
        sample_rows_logprobs(torch.zeros((1, 8), dtype=torch.float16), *step.views()[:4], top_k=0)


def test_the_new_kernel_uses_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = [r for r in kernel_table.kernels() if r["name"].startswith("sample_rows_logprobs_kernel<")]
    assert sorted(r["name"] for r in rows) == ["sample_rows_logprobs_kernel<BF16>", "sample_rows_logprobs_kernel<F16>"]
    for r in rows:
        # what tests/test_kernel_resources.py holds the decode path to: no scratch memory, no vector register spilled to it.
        # (Scalar registers parked in lanes of a vector register are no memory traffic; the body does that in all three
        # kernels — 12 and 14 in the two older ones, 27 here — and the vector budget below includes those lanes.)
        assert r.get("private_segment_fixed_size", 0) == 0 and r.get("vgpr_spill_count", 0) == 0, r
        assert r["wavefront_size"] == 64 and r["vgpr_count"] <= 128, r      # 1024 threads per row: 16 waves, 4 per SIMD
    # and its siblings, whose code this change must not touch, are still there with theirs
    names = {r["name"] for r in kernel_table.kernels()}
    assert {"sample_rows_kernel<BF16>", "sample_rows_kernel<F16>", "sample_rows_constrained_kernel<BF16>",
            "sample_rows_constrained_kernel<F16>"} <= names


def test_reference_against_hand_computed_rows():
    z = np.array([0.0, 3.0, 2.0, 3.0, -1.0, 1.0], dtype=np.float32)
    # greedy: the whole row
    lp, ids, top = sref.reference_logprobs(z, None, 3)
    total = 2 * math.exp(3) + math.exp(2) + math.exp(1) + 1 + math.exp(-1)
    assert np.allclose(lp, z.astype(np.float64) - math.log(total), atol=1e-12) and abs(np.exp(lp).sum() - 1) < 1e-12
    assert ids.tolist() == [1, 3, 2] and np.allclose(top, [3 - math.log(total)] * 2 + [2 - math.log(total)], atol=1e-12)
    # S = {z >= 2}: three tokens; the rest -inf but still named, in z order, then past the row's end
    lp, ids, top = sref.reference_logprobs(z, 2.0, 8)
    zs = 2 * math.exp(3) + math.exp(2)
    assert np.allclose(lp[[1, 3, 2]], [3 - math.log(zs)] * 2 + [2 - math.log(zs)], atol=1e-12) and np.isneginf(lp[[0, 4, 5]]).all()
    assert ids.tolist() == [1, 3, 2, 5, 0, 4, -1, -1] and np.isneginf(top[3:]).all() and np.isfinite(top[:3]).all()
    # S = the two tied maxima: log(1/2) each, lower index first; a single maximum: 0
    lp, ids, top = sref.reference_logprobs(z, 3.0, 2)
    assert ids.tolist() == [1, 3] and top.tolist() == [math.log(0.5)] * 2
    assert sref.reference_logprobs(np.array([1.0, 5.0], dtype=np.float32), 5.0, 1)[2].tolist() == [0.0]
    # K = 0, a banned token in an untruncated row, -0 and +0 tie by index
    assert sref.reference_logprobs(z, None, 0)[1].size == 0
    lp, ids, top = sref.reference_logprobs(np.array([-math.inf, 0.0, -0.0], dtype=np.float32), -math.inf, 3)
    assert ids.tolist() == [1, 2, 0] and top.tolist() == [math.log(0.5), math.log(0.5), -math.inf]
    # row_z: bias, then penalties, then one division by T (T' = 1 on a greedy row)
    x = torch.tensor([1.0, 2.0, 3.0]).to(torch.bfloat16)
    bias = (np.asarray([0], np.int32), np.asarray([4.0], np.float32))
    assert sref.row_z(x, bias, PenaltyHistory([0, 0]), (0.5, 1.0, 2.0), (0.5, 1.0, 0, 1, 0)).tolist() == [3.0, 4.0, 6.0]
    assert sref.row_z(x, bias, PenaltyHistory([0, 0]), (0.5, 1.0, 2.0), (0.0, 1.0, 0, 1, 0)).tolist() == [1.5, 2.0, 3.0]
    assert sref.row_z(x, None, None, (0.0, 0.0, 1.0), (2.0, 1.0, 0, 1, 0)).tolist() == [0.5, 1.0, 1.5]
