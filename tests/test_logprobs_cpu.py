"""CPU: the host side of per-token log-probabilities — request parsing, chunk rendering, request validation, the
refusal of multi-process serving, and the float64 reference the GPU tests measure against (tests/logprob_ref.py)."""
import json
import math
from types import SimpleNamespace as NS

import pytest
import torch

from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.engine.rcb import LogOutputTokenProcessor, TokenLogprob
from hydrainfer_amd.entrypoint import api_protocol as proto
from tests.logprob_ref import assert_logprobs_close, reference


def _body(**kw):
    return dict({"model": "m", "messages": [{"role": "user", "content": "hi"}], "stream": True}, **kw)


def test_protocol_accepts_the_valid_combinations():
    parse = proto.parse_chat_completion_request
    r = parse(_body())
    assert (r.logprobs, r.top_logprobs) == (False, 0)
    assert (parse(_body(logprobs=True)).logprobs, parse(_body(logprobs=True)).top_logprobs) == (True, 0)
    for k in (0, 1, 20):
        r = parse(_body(logprobs=True, top_logprobs=k))
        assert (r.logprobs, r.top_logprobs) == (True, k)
    r = parse(_body(logprobs=False, top_logprobs=0))
    assert (r.logprobs, r.top_logprobs) == (False, 0)
    r = parse(_body(logprobs=None, top_logprobs=None))          # JSON null: as if absent
    assert (r.logprobs, r.top_logprobs) == (False, 0)


@pytest.mark.parametrize("bad", [dict(logprobs=1), dict(logprobs="true"), dict(logprobs=True, top_logprobs=21),
                                 dict(logprobs=True, top_logprobs=-1), dict(logprobs=True, top_logprobs=2.0),
                                 dict(logprobs=True, top_logprobs=True), dict(logprobs=True, top_logprobs="3"),
                                 dict(top_logprobs=3), dict(logprobs=False, top_logprobs=1)],
                         ids=lambda d: json.dumps(d))
def test_protocol_refuses_the_invalid_ones(bad):
    with pytest.raises(proto.ProtocolError):
        proto.parse_chat_completion_request(_body(**bad))


def test_chunks_without_logprobs_are_what_they_were():
    """The renderer of the parent commit, restated: a request that does not ask gets the same bytes, no `logprobs` key."""
    def old(request_id, created, model, content, first=False):
        delta = {"role": "assistant", "content": ""} if first else {"content": content}
        return "data: " + json.dumps({"id": request_id, "object": "chat.completion.chunk", "created": created, "model": model,
                                      "choices": [{"index": 0, "delta": delta}]}, separators=(",", ":"),
                                     ensure_ascii=False) + "\n\n"
    for content, first in ((None, True), (" hello", False), ("é✓", False), ("", False)):
        new = proto.chat_stream_chunk("chatcmpl-1", 17, "llava", content, first=first)
        assert new == old("chatcmpl-1", 17, "llava", content, first) and "logprobs" not in new
        assert proto.chat_stream_chunk("chatcmpl-1", 17, "llava", content, first=first, logprobs=None) == new


def test_chunk_with_logprobs_has_the_openai_shape():
    lp = proto.chat_logprobs(" é", -0.25, [(" é", -0.25), ("x", -math.inf), ("", math.nan)])
    line = proto.chat_stream_chunk("id", 1, "m", " é", logprobs=lp)
    assert line.startswith("data: ") and line.endswith("\n\n")
    assert "Infinity" not in line and "NaN" not in line
    obj = json.loads(line[6:])                     # strict JSON: no -Infinity / NaN literals
    choice = obj["choices"][0]
    assert list(choice) == ["index", "delta", "logprobs"] and choice["delta"] == {"content": " é"}
    (entry,) = choice["logprobs"]["content"]
    assert list(entry) == ["token", "logprob", "bytes", "top_logprobs"]
    assert entry["token"] == " é" and entry["logprob"] == -0.25 and entry["bytes"] == list(" é".encode())
    assert entry["top_logprobs"] == [{"token": " é", "logprob": -0.25, "bytes": [32, 195, 169]},
                                     {"token": "x", "logprob": None, "bytes": [120]},
                                     {"token": "", "logprob": None, "bytes": []}]


def test_stream_processor_pairs_scores_with_their_token():
    """append_logprobs comes immediately before append_token_id of the same token; a processor that never hears
    append_logprobs queues plain text as before."""
    from hydrainfer_amd.entrypoint.api_server import StreamOutputTokenProcessor
    from hydrainfer_amd.entrypoint.tokenizer import SyntheticTokenizer
    loop = NS(call_soon_threadsafe=lambda fn, item: fn(item))
    p = StreamOutputTokenProcessor(loop, SyntheticTokenizer())
    got = []
    p.queue = NS(put_nowait=got.append)
    p.append_token_id(7)
    p.append_logprobs(TokenLogprob(9, -0.5, [(9, -0.5), (4, -1.25), (-1, -math.inf)]))
    p.append_token_id(9, True)
    assert got[0] == " <7>" and got[2] is None
    text, lp = got[1]
    assert text == " <9>" and lp == proto.chat_logprobs(" <9>", -0.5, [(" <9>", -0.5), (" <4>", -1.25), ("", -math.inf)])
    log = LogOutputTokenProcessor()                # the no-op default
    log.append_logprobs(TokenLogprob(1, -1.0))
    log.append_token_id(1)
    assert log.token_ids == [1]


def _request(**sp):
    return TokenRequest(request_id=3, token_ids=[5, 6, 7], sampling_params=SamplingParameters(max_tokens=2, **sp))


def test_instruction_creator_validates_the_new_fields():
    c = InstructionCreator(image_token_id=511, n_image_tokens_per_image=16, block_size=16)
    sp = c.process(_request()).sampling_params
    assert (sp.logprobs, sp.top_logprobs) == (False, 0)
    for k in (0, 5, 20):
        rcb = c.process(_request(logprobs=True, top_logprobs=k))
        assert (rcb.sampling_params.logprobs, rcb.sampling_params.top_logprobs) == (True, k) and rcb.output_logprobs == []
    for bad in (dict(logprobs=True, top_logprobs=21), dict(logprobs=True, top_logprobs=-1), dict(top_logprobs=1),
                dict(logprobs=True, top_logprobs=1.5), dict(logprobs=True, top_logprobs=True), dict(logprobs=1)):
        with pytest.raises(ValueError):
            c.process(_request(**bad))


def test_rank_front_end_refuses_logprobs():
    from hydrainfer_amd.engine.distributed import RankEngine
    from hydrainfer_amd.entrypoint import RankEngineFrontend
    submitted = []
    engine = NS(submit=lambda *a: submitted.append(a), creator=None)
    front = RankEngineFrontend(engine, InstructionCreator(511, 16, 16))
    with pytest.raises(ValueError, match="logprobs are not available in multi-process serving"):
        front._start(_request(logprobs=True, top_logprobs=2), object())
    assert submitted == []
    front._start(_request(), "p")
    assert len(submitted) == 1
    # and the engine's own entry, whoever calls it
    handlers = {}
    with pytest.raises(ValueError, match="logprobs"):
        RankEngine.submit(NS(token_handlers=handlers), _request(logprobs=True), "p", None)
    assert handlers == {}


def test_reference_on_a_hand_computed_row():
    """Probabilities 0.1, 0.2, 0.3, 0.4 (logits = their logs + a constant), and a row of ties with a masked entry."""
    x = torch.log(torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=torch.float64)) + 7.0
    ids, lp, top_ids, top_lp = reference(x, 6)
    assert ids.tolist() == [3] and abs(float(lp[0]) - math.log(0.4)) < 1e-12
    assert top_ids.tolist() == [[3, 2, 1, 0, -1, -1]]
    assert top_lp[0, 4:].tolist() == [-math.inf] * 2
    assert torch.allclose(top_lp[0, :4], torch.log(torch.tensor([0.4, 0.3, 0.2, 0.1], dtype=torch.float64)), atol=1e-12, rtol=0)
    y = torch.tensor([[1.0, -math.inf, 1.0, 0.0]], dtype=torch.float16)
    ids, lp, top_ids, top_lp = reference(y, 4)
    z = math.log(2 * math.e + 1)
    assert ids.tolist() == [0] and top_ids.tolist() == [[0, 2, 3, 1]]
    assert torch.allclose(top_lp[0, :3], torch.tensor([1 - z, 1 - z, -z], dtype=torch.float64), atol=1e-12, rtol=0)
    assert float(top_lp[0, 3]) == -math.inf
    nan = torch.tensor([[0.0, math.nan, 5.0]])
    ids, lp, top_ids, top_lp = reference(nan, 2)
    assert ids.tolist() == [1] and top_ids.tolist() == [[1, 2]] and bool(torch.isnan(top_lp).all()) and math.isnan(float(lp[0]))
    assert reference(x, 0)[2].shape == (1, 0)
    assert_logprobs_close(top_lp.float(), top_lp)
    with pytest.raises(AssertionError):
        assert_logprobs_close(torch.tensor([-1.0002]), torch.tensor([-1.0], dtype=torch.float64))


def test_the_op_refuses_cpu_tensors():
    from hydrainfer_amd import _lib
    from hydrainfer_amd._C.kernel.norm import logprob_rows
    with pytest.raises(_lib.HydraHipError):
        logprob_rows(torch.zeros((2, 8), dtype=torch.float16), 1)
