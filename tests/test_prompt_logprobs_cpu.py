"""CPU: prompt log-probabilities (`prompt_logprobs`) on the host side — the chat protocol, the InstructionCreator's score
lists and how chunk_prefill carries them, the parameters builder's score plan, the float64 reference the GPU tests use,
and the new kernels' resources as the built library records them."""
import json
import math
import os
import sys
from collections import Counter
from types import SimpleNamespace as NS

import pytest
import torch

from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.engine.isa import Fill
from hydrainfer_amd.engine.rcb import LogOutputTokenProcessor, TokenParameters
from hydrainfer_amd.entrypoint import api_protocol as proto

IMG, N_IMG_TOK, BS = 511, 16, 16


def _body(**kw):
    return dict({"model": "m", "messages": [{"role": "user", "content": "hi"}], "stream": True}, **kw)


# ------------------------------------------------------------------------------------------------------------ protocol
def test_protocol_accepts_and_refuses():
    parse = proto.parse_chat_completion_request
    assert parse(_body()).prompt_logprobs is None and parse(_body(prompt_logprobs=None)).prompt_logprobs is None
    for k in (0, 1, 20):
        assert parse(_body(prompt_logprobs=k)).prompt_logprobs == k
    # independent of logprobs, combinable with every sampling mode
    r = parse(_body(prompt_logprobs=3, temperature=0.7, seed=5, frequency_penalty=0.5))
    assert (r.prompt_logprobs, r.temperature, r.frequency_penalty, r.logprobs) == (3, 0.7, 0.5, False)
    r = parse(_body(prompt_logprobs=0, logprobs=True, top_logprobs=2))
    assert (r.prompt_logprobs, r.logprobs, r.top_logprobs) == (0, True, 2)
    for bad in (-1, 21, True, False, 2.0, "3", [1]):
        with pytest.raises(proto.ProtocolError, match="prompt_logprobs"):
            parse(_body(prompt_logprobs=bad))


def test_first_chunk_carries_the_array_and_other_chunks_are_what_they_were():
    entries = [None, (" a", -0.25, 0, [(" a", -0.25), ("x", -math.inf)]), None, ("é", math.nan, 7, []),
               ("z", -math.inf, 510, [("", math.nan)])]
    arr = proto.chat_prompt_logprobs(entries)
    line = proto.chat_stream_chunk("id", 1, "m", None, first=True, prompt_logprobs=arr)
    assert line.startswith("data: ") and line.endswith("\n\n") and "Infinity" not in line and "NaN" not in line
    obj = json.loads(line[6:])
    assert list(obj) == ["id", "object", "created", "model", "choices", "prompt_logprobs"]
    assert obj["choices"] == [{"index": 0, "delta": {"role": "assistant", "content": ""}}]
    got = obj["prompt_logprobs"]
    assert len(got) == 5 and got[0] is None and got[2] is None
    assert list(got[1]) == ["token", "logprob", "rank", "bytes", "top_logprobs"]
    assert got[1] == {"token": " a", "logprob": -0.25, "rank": 0, "bytes": [32, 97],
                      "top_logprobs": [{"token": " a", "logprob": -0.25, "bytes": [32, 97]},
                                       {"token": "x", "logprob": None, "bytes": [120]}]}
    assert got[3] == {"token": "é", "logprob": None, "rank": 7, "bytes": [195, 169], "top_logprobs": []}
    assert got[4]["logprob"] is None and got[4]["rank"] == 510 and got[4]["top_logprobs"][0]["logprob"] is None
    # a chunk without the field: byte for byte the call of today
    for content, first in ((None, True), (" hello", False), ("é✓", False), ("", False)):
        today = proto.chat_stream_chunk("chatcmpl-1", 17, "llava", content, first=first)
        assert proto.chat_stream_chunk("chatcmpl-1", 17, "llava", content, first=first, prompt_logprobs=None) == today
        assert "prompt_logprobs" not in today
    lp = proto.chat_logprobs(" é", -0.25, [])
    assert proto.chat_stream_chunk("i", 1, "m", " é", logprobs=lp, prompt_logprobs=None) == \
        proto.chat_stream_chunk("i", 1, "m", " é", logprobs=lp)


def test_stream_processor_queues_the_prompt_scores_in_front_of_the_first_token():
    from hydrainfer_amd.engine.rcb import PromptTokenLogprob
    from hydrainfer_amd.entrypoint.api_server import PromptScores, StreamOutputTokenProcessor
    from hydrainfer_amd.entrypoint.tokenizer import SyntheticTokenizer
    loop = NS(call_soon_threadsafe=lambda fn, item: fn(item))
    p = StreamOutputTokenProcessor(loop, SyntheticTokenizer())
    got = []
    p.queue = NS(put_nowait=got.append)
    p.set_prompt_logprobs([None, PromptTokenLogprob(9, -0.5, 3, [(4, -0.25), (-1, -math.inf)]), None])
    p.append_token_id(7, True)
    assert isinstance(got[0], PromptScores) and got[1] == " <7>" and got[2] is None
    assert got[0].array == proto.chat_prompt_logprobs([None, (" <9>", -0.5, 3, [(" <4>", -0.25), ("", -math.inf)]), None])
    log = LogOutputTokenProcessor()                # the no-op default
    log.set_prompt_logprobs([None])
    log.append_token_id(1)
    assert log.token_ids == [1]


def _request(token_ids=(5, 6, 7), **sp):
    return TokenRequest(request_id=3, token_ids=list(token_ids), sampling_params=SamplingParameters(max_tokens=2, **sp))


def test_multi_process_serving_refuses():
    from hydrainfer_amd.engine.distributed import RankEngine, refuse_prompt_logprobs
    from hydrainfer_amd.entrypoint import RankEngineFrontend
    with pytest.raises(ValueError, match="prompt_logprobs are not available in multi-process serving"):
        refuse_prompt_logprobs(_request(prompt_logprobs=0))
    refuse_prompt_logprobs(_request())
    submitted = []
    front = RankEngineFrontend(NS(submit=lambda *a: submitted.append(a), creator=None), InstructionCreator(IMG, N_IMG_TOK, BS))
    with pytest.raises(ValueError, match="prompt_logprobs"):
        front._start(_request(prompt_logprobs=2), object())
    assert submitted == []
    handlers = {}
    with pytest.raises(ValueError, match="prompt_logprobs"):
        RankEngine.submit(NS(token_handlers=handlers), _request(prompt_logprobs=0), "p", None)
    assert handlers == {}


# ------------------------------------------------------------------------------------- InstructionCreator and the Fill
def _creator():
    return InstructionCreator(image_token_id=IMG, n_image_tokens_per_image=N_IMG_TOK, block_size=BS, ignore_eos=True)


def _prompts():
    """(name, token_ids, pixel_values, token_params): text only, image in front, image in the middle, a focal-pruned image
    — random text like the prompts of tests/test_gpu_logprobs_engine.py."""
    g = torch.Generator().manual_seed(4242)
    text = lambda n: torch.randint(0, IMG, (n,), generator=g).tolist()
    px = torch.zeros(1, 3, 56, 56)
    return [("text", text(28), None, None),
            ("image in front", [IMG] + text(33), px, None),
            ("image in the middle", text(9) + [IMG] + text(21), px, None),
            ("focal-pruned image", [IMG] + text(45), px, TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=5))]


def _prompt_fill(rcb):
    return next(i for i in rcb.instructions if isinstance(i, Fill))


def _process(p, ask):
    name, token_ids, px, tp = p
    return _creator().process(TokenRequest(request_id=1, token_ids=list(token_ids), pixel_values=px, image_size=(56, 56),
                                           image_hash=77, token_params=tp,
                                           sampling_params=SamplingParameters(max_tokens=3, prompt_logprobs=ask)))


def _chunkings(n):
    """Every way to cut a fill of n tokens at most twice with pieces of 1, 15, 16, 17 or n - 1 tokens."""
    sizes = lambda m: sorted({s for s in (1, 15, 16, 17, m - 1) if 0 < s < m})
    out = [()]
    for a in sizes(n):
        out.append((a,))
        out += [(a, b) for b in sizes(n - a)]
    return out


@pytest.mark.parametrize("p", _prompts(), ids=lambda p: p[0])
def test_every_chunking_scores_every_token_once(p):
    own = p[1]
    n_img = 0 if p[2] is None else (p[3].n_embed_output_tokens if p[3] is not None else N_IMG_TOK)
    want = Counter((i, t) for i, t in enumerate(own) if i >= 1 and t != IMG)
    expanded_pos, at = [], 0                   # own index -> position of (the first copy of) that token in the expanded prompt
    for t in own:
        expanded_pos.append(at)
        at += n_img if t == IMG else 1
    n = _prompt_fill(_process(p, 2)).token_ids.__len__()
    assert n == at
    tried = 0
    for cuts in _chunkings(n):
        rcb = _process(p, 2)
        assert rcb.prompt_logprobs == [None] * len(own) and rcb.sampling_params.prompt_logprobs == 2
        fill = _prompt_fill(rcb)
        assert fill.hashes is None
        pieces = [fill]
        for c in cuts:
            pieces[-1].chunk_prefill(c)
            pieces.append(pieces[-1].next)
        assert sum(len(f.token_ids) for f in pieces) == n
        got = Counter()
        for f in pieces:
            assert f.hashes is None and len(f.score_targets) == len(f.score_index) == len(f.token_ids)
            for j, (t, i) in enumerate(zip(f.score_targets, f.score_index)):
                if t < 0:
                    assert i == -1
                    continue
                got[(i, t)] += 1
                assert f.position_ids[j] == expanded_pos[i] - 1, "the scoring row is not the one in front of the token"
        assert pieces[-1].score_targets[-1] == -1, "the last prompt position predicts the generated token"
        assert got == want, f"cuts {cuts}: scored {sorted(got.items())} instead of {sorted(want.items())}"
        tried += 1
    assert tried >= 10


@pytest.mark.parametrize("p", _prompts(), ids=lambda p: p[0])
def test_a_request_that_does_not_ask_is_untouched(p):
    plain = _process(p, None)
    fill = _prompt_fill(plain)
    assert fill.score_targets is None and fill.score_index is None and plain.prompt_logprobs == []
    assert plain.sampling_params.prompt_logprobs is None
    asked = _prompt_fill(_process(p, 0))
    assert fill.hashes is not None and len(fill.hashes) == len(fill.token_ids) // BS and asked.hashes is None
    assert asked.token_ids == fill.token_ids and asked.position_ids == fill.position_ids
    fill.chunk_prefill(3)
    assert fill.score_targets is None and fill.next.score_targets is None
    # decode Fills never carry a list
    assert all(i.score_targets is None for i in _process(p, 0).instructions if isinstance(i, Fill) and len(i.token_ids) == 1
               and i is not asked)


def test_instruction_creator_validates():
    c = _creator()
    for k in (0, 5, 20):
        rcb = c.process(_request(prompt_logprobs=k))
        assert rcb.sampling_params.prompt_logprobs == k and rcb.prompt_logprobs == [None, None, None]
    # combinable with every sampling mode
    rcb = c.process(_request(prompt_logprobs=1, temperature=0.5, seed=3, repetition_penalty=1.2))
    assert rcb.sampling_params.prompt_logprobs == 1 and rcb.penalty_history is not None
    rcb = c.process(_request(prompt_logprobs=1, logprobs=True, top_logprobs=4))
    assert rcb.sampling_params.logprobs and rcb.sampling_params.prompt_logprobs == 1
    for bad in (-1, 21, True, False, 1.5, "2"):
        with pytest.raises(ValueError, match="prompt_logprobs"):
            c.process(_request(prompt_logprobs=bad))
    # the new fields stand at the END of their dataclasses
    import dataclasses
    from hydrainfer_amd.engine.offline import OfflineInferenceOutput, OfflineRequest
    for cls in (SamplingParameters, OfflineRequest, proto.ChatRequest, OfflineInferenceOutput):
        assert dataclasses.fields(cls)[-1].name == "prompt_logprobs"
    assert OfflineInferenceOutput().prompt_logprobs == []


# ---------------------------------------------------------------------------------------------------- the builder's plan
def _builder():
    from hydrainfer_amd.engine.parameters_builder import LanguageModelParametersBuilder
    manager = NS(block_size=BS, v2p=lambda vc, ids: list(ids))
    return LanguageModelParametersBuilder(manager, manager, 1, 2, 2, 8, IMG, torch.float16, torch.device("cpu"))


def _batch(ask):
    """Two decodes, one prefill chunk of an image prompt (scoring if ask is not None) and one plain prefill."""
    vc = lambda: NS(block_table=list(range(8)))
    out = []
    for r in range(2):
        rcb = _creator().process(_request(token_ids=[7, 8, 9, 10]))
        rcb.virtual_kv_cache = vc()
        fill = _prompt_fill(rcb)
        out.append((rcb, fill.next.next.next))                         # its first decode Fill (behind PDMigrate, PullCache)
        assert len(out[-1][1].token_ids) == 1
    p = _prompts()[2]
    rcb = _process(p, ask)
    rcb.virtual_kv_cache, rcb.virtual_image_cache = vc(), vc()
    chunk = _prompt_fill(rcb)
    chunk.chunk_prefill(17)                                             # 9 text rows, 8 of the image's 16
    out.append((rcb, chunk))
    rcb = _process(_prompts()[0], None)
    rcb.virtual_kv_cache = vc()
    out.append((rcb, _prompt_fill(rcb)))
    return out


def test_builder_plan():
    scoring, plain = _builder(), _builder()
    batch = _batch(3)
    for rcb, inst in batch:
        scoring.add(rcb, inst)
    for rcb, inst in _batch(None):
        plain.add(rcb, inst)
    assert plain.build_score_plan() is None
    assert scoring.selected_token_ids == plain.selected_token_ids == [0, 1, 18, 46]     # what the parent builds
    plan = scoring.build_score_plan()
    # the chunk is batch rows 2 .. 18: rows 2 .. 9 score text tokens 1 .. 8, row 10 (text token 8) stands in front of the
    # image and rows 11 .. 18 in front of image placeholders: nothing to score; row 18 also samples (a chunk head's)
    own = _prompts()[2][1]
    assert plan.rows == [0, 1] + list(range(2, 10)) + [18, 46]
    assert plan.sample_pos == [0, 1, 10, 11] and [plan.rows[i] for i in plan.sample_pos] == scoring.selected_token_ids
    assert plan.targets == [-1, -1] + own[1:9] + [-1, -1]
    assert [d and d[1] for d in plan.dst] == [None, None] + list(range(1, 9)) + [None, None]
    assert all(d is None or d[0] is batch[2][0] for d in plan.dst) and plan.top_k == 3


def test_builder_plan_all_single_token_fills():
    """A one-token piece of a scored prompt among decodes: the model narrows nothing in an all-decode batch, so every row
    reaches the logits."""
    b = _builder()
    batch = _batch(0)[:2]
    rcb = _process(_prompts()[0], 0)
    rcb.virtual_kv_cache = NS(block_table=list(range(8)))
    head = _prompt_fill(rcb)
    head.chunk_prefill(1)
    for r, i in batch + [(rcb, head)]:
        b.add(r, i)
    plan = b.build_score_plan()
    assert plan.rows == [0, 1, 2] and plan.targets == [-1, -1, _prompts()[0][1][1]] and plan.sample_pos == [0, 1, 2]


# ------------------------------------------------------------------------------------------------------- the reference
def test_reference_self_test_and_a_hand_computed_row():
    from tests.token_logprob_ref import self_test, token_reference
    self_test()
    x = torch.tensor([[1.0, 3.0, 2.0, 3.0, -math.inf]], dtype=torch.float16)
    z = math.log(math.e + 2 * math.e ** 3 + math.e ** 2)
    for t, rank, lp in ((1, 0, 3 - z), (3, 1, 3 - z), (2, 2, 2 - z), (0, 3, 1 - z), (4, 4, -math.inf)):
        got = token_reference(x, [t], 2)
        assert int(got[1][0]) == rank and (got[0][0] == lp if lp == -math.inf else abs(float(got[0][0]) - lp) < 1e-12)
        assert got[2][0].tolist() == [1, 3]


def test_the_op_refuses_cpu_tensors():
    from hydrainfer_amd import _lib
    from hydrainfer_amd._C.kernel.norm import (token_logprob_rows, token_logprob_rows_bytes, token_logprob_rows_views)
    with pytest.raises(_lib.HydraHipError):
        token_logprob_rows(torch.zeros(2, 8, dtype=torch.float16), torch.zeros(2, dtype=torch.int32))
    assert token_logprob_rows_bytes(3, 4) == 3 * 8 + 2 * 3 * 4 * 4
    lp, ranks, top_ids, top_lp = token_logprob_rows_views(torch.zeros(token_logprob_rows_bytes(3, 4), dtype=torch.uint8), 3, 4)
    assert (lp.dtype, ranks.dtype, top_ids.dtype, top_lp.dtype) == (torch.float32, torch.int32, torch.int32, torch.float32)
    assert lp.shape == (3,) and ranks.shape == (3,) and top_ids.shape == (3, 4) and top_lp.shape == (3, 4)


# ------------------------------------------------------------------------------------------------------------ resources
def test_new_kernels_use_no_scratch_and_wave64():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from kernel_table import kernels
    rows = [r for r in kernels() if "token_logprob_rows_kernel" in r["name"]]
    assert len(rows) == 4, [r["name"] for r in rows]           # fp16 / bf16 x (from global memory, staged in LDS)
    for r in rows:
        assert r["private_segment_fixed_size"] == 0 and r["wavefront_size"] == 64, r
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, r
