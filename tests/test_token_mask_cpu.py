"""CPU: the host side of token masks (allowed_token_ids, guided_choice) — the bit layout of pack_mask_words against a
plain Python loop (tests/mask_ref.py), TokenMask's trie, every refusal of check_token_mask and of admission, the step
packer against pack_constrained_step, the executor's masked_rows / _choose / _sample_masked with the kernels patched by
name, the API parser, and the C ABI binding."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.engine import executor as ex
from hydrainfer_amd.engine.rcb import BatchRequest
from hydrainfer_amd.entrypoint import api_protocol as proto
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, PenaltyHistory, TokenMask, check_token_mask,
                                     pack_constrained_step, pack_mask_words, pack_masked_step)
from tests import mask_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = 500
CHOICES = [[5], [7, 8], [7, 9, 2]]


# ---------------------------------------------------------------------------------------------------- pack_mask_words
@pytest.mark.parametrize("n", [1, 31, 32, 33, 32064])
def test_pack_mask_words_against_a_plain_loop(n):
    g = np.random.default_rng(n)
    for ids in ([], [0], [n - 1], list(range(n)), sorted(set(g.integers(0, n, size=min(n, 200)).tolist()))):
        words = pack_mask_words(ids, n)
        assert words.dtype == np.uint32 and words.shape == ((n + 31) // 32,)
        assert words.tolist() == mask_ref.words_by_loop(ids, n)
        assert mask_ref.allowed_of(words, n) == sorted(ids)
        assert all(not (int(words[t // 32]) >> (t % 32)) & 1 for t in range(n, 32 * len(words))), "a bit at or above n is set"
    assert pack_mask_words(np.asarray([0, n - 1] if n > 1 else [0], dtype=np.int64), n).tolist() \
        == mask_ref.words_by_loop({0, n - 1}, n)


@pytest.mark.parametrize("bad", [[-1], [100], [3, 3], [True], [1.0], ["2"], [None]])
def test_pack_mask_words_refuses(bad):
    with pytest.raises(ValueError):
        pack_mask_words(bad, 100)


# ---------------------------------------------------------------------------------------------------- TokenMask
def test_trie_walk():
    allowed = lambda m: mask_ref.allowed_of(m.current(), VOCAB)
    for path in CHOICES:
        m = TokenMask(VOCAB, guided_choice=CHOICES)
        assert allowed(m) == [5, 7] and not m.finished
        root = m.current()
        assert m.current() is root, "the same node gives the same array object"
        for i, t in enumerate(path):
            assert not m.finished
            m.advance(t)
            assert m.finished == (i == len(path) - 1), "finished comes exactly at the leaves"
            if path[:i + 1] == [7]:
                assert allowed(m) == [8, 9] and m.current() is m.current() and m.current() is not root
            if path[:i + 1] == [7, 9]:
                assert allowed(m) == [2]
        with pytest.raises(ValueError):
            m.current()
        with pytest.raises(ValueError):
            m.advance(5)
    m = TokenMask(VOCAB, guided_choice=CHOICES)
    with pytest.raises(ValueError, match="not among"):
        m.advance(8)
    # two requests on the same choices do not share arrays; one request's node does, step after step
    assert TokenMask(VOCAB, guided_choice=CHOICES).current() is not TokenMask(VOCAB, guided_choice=CHOICES).current()


def test_allowed_token_ids_is_one_node_every_step():
    m = TokenMask(VOCAB, allowed_token_ids=[3, 400, 64])
    words = m.current()
    assert mask_ref.allowed_of(words, VOCAB) == [3, 64, 400]
    for t in (3, 400, 3, 64):
        m.advance(t)
        assert m.current() is words and not m.finished
    with pytest.raises(ValueError):
        TokenMask(VOCAB)
    with pytest.raises(ValueError):
        TokenMask(VOCAB, [1], [[1]])


BAD_MASKS = [
    (dict(allowed_token_ids=[1], guided_choice=[[1]]), "cannot be combined"),
    (dict(allowed_token_ids=[]), "allowed_token_ids"), (dict(allowed_token_ids=[1, 1]), "twice"),
    (dict(allowed_token_ids=[1.0]), "allowed_token_ids"), (dict(allowed_token_ids=[True]), "allowed_token_ids"),
    (dict(allowed_token_ids=[VOCAB]), "allowed_token_ids"), (dict(allowed_token_ids=[-1]), "allowed_token_ids"),
    (dict(allowed_token_ids=5), "allowed_token_ids"),
    (dict(guided_choice=[]), "guided_choice"), (dict(guided_choice=[[]]), "guided_choice"),
    (dict(guided_choice=[[1]] * 2), "twice"), (dict(guided_choice=[[i] for i in range(65)]), "guided_choice"),
    (dict(guided_choice=[list(range(65))]), "guided_choice"), (dict(guided_choice=[[1, VOCAB]]), "guided_choice"),
    (dict(guided_choice=[[1, True]]), "guided_choice"), (dict(guided_choice=[[1, 2.0]]), "guided_choice"),
    (dict(guided_choice=[7]), "guided_choice"), (dict(guided_choice="ab"), "guided_choice"),
    (dict(guided_choice=[[7], [7, 8]]), "prefix"), (dict(guided_choice=[[7, 8, 9], [5], [7, 8]]), "prefix"),
]


@pytest.mark.parametrize("fields,match", BAD_MASKS)
def test_check_token_mask_refuses(fields, match):
    with pytest.raises(ValueError, match=match):
        check_token_mask(fields.get("allowed_token_ids"), fields.get("guided_choice"), VOCAB)


def test_check_token_mask_accepts():
    assert check_token_mask(None, None, VOCAB) == (None, None) and check_token_mask(None, None, None) == (None, None)
    assert check_token_mask([VOCAB - 1, 0], None, VOCAB) == ([VOCAB - 1, 0], None)
    assert check_token_mask(None, CHOICES, VOCAB) == (None, CHOICES)
    assert check_token_mask(None, [[1, 1], [1, 2]], VOCAB) == (None, [[1, 1], [1, 2]])     # within a choice an id may repeat
    assert check_token_mask(None, [list(range(64))] + [[100 + i] for i in range(63)], VOCAB)[1] is not None
    with pytest.raises(ValueError, match="vocabulary"):
        check_token_mask([1], None, None)


# ---------------------------------------------------------------------------------------------------- the step packer
def test_pack_masked_step():
    n = 100
    a, b = TokenMask(n, guided_choice=[[5, 6], [7, 8]]), TokenMask(n, allowed_token_ids=[1, 99])
    bias = (np.asarray([3, 9], np.int32), np.asarray([0.5, -2.0], np.float32))
    four = [(PenaltyHistory([4, 4, 5]), (0.5, 0.25, 1.5), (0.7, 0.9, 50, 77, 4, 0.25), bias),
            (None, NO_PENALTIES, GREEDY_RECORD, None),
            (None, NO_PENALTIES, (1.0, 1.0, 0, 5, 1), None),
            (PenaltyHistory([8]), (0.0, 0.0, 2.0), GREEDY_RECORD, None),
            (None, NO_PENALTIES, GREEDY_RECORD, bias)]
    extra = [(0, a.current()), (-1, None), (-1, b.current()), (3, a.current()), (-1, None)]
    step = pack_masked_step([f + e for f, e in zip(four, extra)])
    assert step.buffer.dtype == np.int32 and (step.rows, step.n_masks, step.words) == (5, 2, 4)
    *tables, want = step.views()
    sp, bi, bv, cb, allow, mask_row, hi, hc, cu, pen = tables
    inner = pack_constrained_step(four)
    assert np.array_equal(step.buffer[:inner.buffer.size], inner.buffer)
    for got, ref in zip((sp, bi, bv, cb, hi, hc, cu, pen), inner.views()):
        assert got.dtype == ref.dtype and torch.equal(got, ref)
    assert want.tolist() == [0, -1, -1, 3, -1]
    assert mask_row.tolist() == [0, -1, 1, 0, -1], "rows on one node share a mask, a row without one carries -1"
    assert allow.shape == (2, 4) and allow.dtype == torch.int32
    assert mask_ref.allowed_of(allow[0].numpy().view(np.uint32), n) == [5, 7]
    assert mask_ref.allowed_of(allow[1].numpy().view(np.uint32), n) == [1, 99]
    assert step.buffer.size == inner.buffer.size + 2 * 5 + 2 * 4, "one buffer: the tables, want, mask_row, the masks"
    # the same content in another array is another mask: identity, not content
    twin = TokenMask(n, allowed_token_ids=[1, 99])
    two = pack_masked_step([four[1] + (-1, b.current()), four[1] + (-1, twin.current())])
    assert two.n_masks == 2 and two.views()[5].tolist() == [0, 1]
    # no mask at all
    none = pack_masked_step([f + (-1, None) for f in four])
    assert none.n_masks == 0 and none.views()[4].shape == (0, 0) and none.views()[5].tolist() == [-1] * 5
    with pytest.raises(ValueError, match="width"):
        pack_masked_step([four[1] + (-1, b.current()), four[1] + (-1, TokenMask(200, allowed_token_ids=[1]).current())])


# ---------------------------------------------------------------------------------------------------- admission
def _request(max_tokens=4, token_ids=(5, 6, 7), **sp):
    return TokenRequest(request_id=3, token_ids=list(token_ids), sampling_params=SamplingParameters(max_tokens=max_tokens, **sp))


def _creator(**kw):
    return InstructionCreator(image_token_id=VOCAB - 1, n_image_tokens_per_image=16, block_size=16, **kw)


def test_sampling_parameters_take_the_fields_by_keyword_only():
    sp = SamplingParameters(7, [2], True, 5, 0.5, 0.25, 1.5, 0.7, 0.9, 50, 11, 3)
    assert (sp.allowed_token_ids, sp.guided_choice, sp.prompt_logprobs) == (None, None, 3)
    sp = SamplingParameters(allowed_token_ids=[1, 2])
    assert sp.allowed_token_ids == [1, 2] and sp.guided_choice is None and sp == SamplingParameters(allowed_token_ids=[1, 2])
    assert sp != SamplingParameters()
    with pytest.raises(TypeError):
        SamplingParameters(7, [2], True, 5, 0.5, 0.25, 1.5, 0.7, 0.9, 50, 11, 3, [1, 2])
    from hydrainfer_amd.engine.offline import OfflineRequest
    r = OfflineRequest([1, 2], guided_choice=[[3], [4, 5]])
    assert r.guided_choice == [[3], [4, 5]] and r.allowed_token_ids is None
    assert OfflineRequest([1, 2], allowed_token_ids=[9]).allowed_token_ids == [9]


def test_admission_builds_the_mask():
    c = _creator()
    rcb = c.process(_request(allowed_token_ids=[3, 4]), vocab_size=VOCAB)
    assert isinstance(rcb.token_mask, TokenMask) and mask_ref.allowed_of(rcb.token_mask.current(), VOCAB) == [3, 4]
    assert rcb.sampling_params.allowed_token_ids == [3, 4] and rcb.token_constraints is None
    rcb = c.process(_request(guided_choice=CHOICES, temperature=0.5, logit_bias={7: 50.0}), vocab_size=VOCAB)
    assert mask_ref.allowed_of(rcb.token_mask.current(), VOCAB) == [5, 7] and rcb.token_constraints is not None
    # processed log-probabilities and prompt_logprobs combine with a mask
    rcb = c.process(_request(allowed_token_ids=[3], logprobs=True, top_logprobs=2, logprobs_mode="processed_logprobs",
                             prompt_logprobs=1), vocab_size=VOCAB)
    assert rcb.token_mask is not None
    rcb = c.process(_request(guided_choice=CHOICES, prompt_logprobs=0), vocab_size=VOCAB)
    assert rcb.token_mask is not None
    # min_tokens beside allowed_token_ids that hold something besides the end-of-sequence ids
    rcb = c.process(_request(allowed_token_ids=[2, 9], min_tokens=2, eos_token_ids=[2]), vocab_size=VOCAB)
    assert rcb.token_mask is not None and rcb.token_constraints is not None


@pytest.mark.parametrize("fields,match", BAD_MASKS + [
    (dict(allowed_token_ids=[3], logprobs=True), "processed_logprobs"),
    (dict(guided_choice=CHOICES, logprobs=True, logprobs_mode="raw_logprobs"), "processed_logprobs"),
    (dict(guided_choice=CHOICES, min_tokens=1), "min_tokens"),
    (dict(guided_choice=CHOICES, min_tokens=2, eos_token_ids=[2]), "min_tokens"),
    (dict(allowed_token_ids=[2, 3], min_tokens=1, eos_token_ids=[3, 2, 4]), "end-of-sequence"),
])
def test_admission_refuses(fields, match):
    with pytest.raises(ValueError, match=match):
        _creator().process(_request(**fields), vocab_size=VOCAB)


def test_admission_refuses_the_servers_own_end_of_sequence_id_alone():
    with pytest.raises(ValueError, match="end-of-sequence"):
        _creator(ignore_eos=False, eos_token_id=2).process(_request(allowed_token_ids=[2], min_tokens=1), vocab_size=VOCAB)
    with pytest.raises(ValueError, match="vocabulary"):
        _creator().process(_request(allowed_token_ids=[2]))


def test_a_request_with_neither_field_is_what_it_was():
    c = _creator()
    for fields in ({}, dict(temperature=0.7, seed=3, repetition_penalty=1.2, logit_bias={5: 1.0}, min_p=0.1)):
        for vocab in (None, VOCAB):
            rcb = c.process(_request(**fields), vocab_size=vocab)
            assert rcb.token_mask is None
            assert (rcb.token_constraints is not None) == bool(fields) and (rcb.penalty_history is not None) == bool(fields)
            sp = rcb.sampling_params
            assert sp.allowed_token_ids is None and sp.guided_choice is None
            kinds, inst = [], rcb.instructions.head
            while inst is not None:
                kinds.append((type(inst).__name__, getattr(inst, "token_ids", None)))
                inst = inst.next
            assert [k for k, _ in kinds if k == "TextFill"] == ["TextFill"] * 4
            assert kinds[:2] == [("EmptyInstruction", None), ("TextFill", [5, 6, 7])] and rcb.current_instruction().sample


def test_multi_process_serving_refuses_masks():
    from hydrainfer_amd.engine.distributed import refuse_token_mask
    from hydrainfer_amd.entrypoint import RankEngineFrontend
    refuse_token_mask(_request())
    refuse_token_mask(NS(request_id=1))
    for fields in (dict(allowed_token_ids=[1]), dict(guided_choice=[[1]])):
        with pytest.raises(ValueError, match="allowed_token_ids / guided_choice are not available in multi-process serving"):
            refuse_token_mask(_request(**fields))
    submitted = []
    front = RankEngineFrontend(NS(submit=lambda *a: submitted.append(a), creator=None), _creator())
    with pytest.raises(ValueError, match="multi-process serving"):
        front._start(_request(guided_choice=[[1]]), object())
    assert submitted == []
    front._start(_request(), "p")
    assert len(submitted) == 1


# ---------------------------------------------------------------------------------------------------- the executor
class _LM:
    """forward / forward_logits of the language model: logits whose argmax is 11 in every row"""

    def __init__(self, log):
        self.log = log

    def forward_logits(self, input_ids, image_features, position_ids, params):
        self.log.append("forward_logits")
        x = torch.zeros((len(params.selected), 64))
        x[:, 11] = 1.0
        return x

    def forward(self, input_ids, image_features, position_ids, params):
        self.log.append("forward")
        return torch.full((len(params.selected),), 11, dtype=torch.int64)


def _executor(log):
    fill = object.__new__(ex.BatchFillExecutor)
    fill.language_model, fill.device = _LM(log), torch.device("cpu")
    return fill


def _step(fill, rcbs):
    """one eager sampling step over the requests' current instructions, through _choose and _deliver"""
    from hydrainfer_amd.engine.isa import Fill
    for rcb in rcbs:                        # (the node runs the migrate / pull instructions between the fills)
        while not isinstance(rcb.current_instruction(), Fill):
            rcb.step()
    batch = BatchRequest(rcbs)
    sel = list(range(len(rcbs)))
    inputs = NS(selected_token_ids=sel, all_sequences_decode=False, input_ids=torch.zeros(len(rcbs)), image_features=None,
                position_ids=None)
    fill._deliver(batch, *fill._choose(batch, inputs, NS(selected=sel)))


def _patch_kernels(monkeypatch, log, pick):
    """every sampling kernel the executor reaches by name, recorded; sample_rows_masked answers pick(row's allowed ids)"""
    def masked(logits, sp, bi, bv, cb, allow, mask_row, hi, hc, cu, pen, *, top_k=None, want=None, **kw):
        log.append(("sample_rows_masked", mask_row.tolist(), None if want is None else want.tolist(), top_k,
                    tuple(allow.shape)))
        ids = []
        for r, j in enumerate(mask_row.tolist()):
            ids.append(pick(mask_ref.allowed_of(allow[j].numpy().view(np.uint32), logits.shape[1])) if j >= 0
                       else int(logits[r].argmax()))
        assert top_k is None
        return torch.tensor(ids)
    monkeypatch.setattr(ex, "sample_rows_masked", masked)
    for name in ("sample_rows_logprobs", "sample_rows_constrained", "sample_rows", "penalized_argmax_rows", "argmax_rows",
                 "logprob_rows"):
        def other(*a, _name=name, **kw):
            log.append(_name)
            raise AssertionError(f"{_name} launched beside sample_rows_masked")
        monkeypatch.setattr(ex, name, other)


def test_one_masked_row_makes_one_masked_launch_and_nothing_else(monkeypatch):
    log = []
    _patch_kernels(monkeypatch, log, pick=max)
    c = InstructionCreator(image_token_id=63, n_image_tokens_per_image=4, block_size=16)
    plain, sampled = c.process(_request(), vocab_size=64), c.process(_request(temperature=0.5, seed=1), vocab_size=64)
    guided = c.process(_request(guided_choice=[[5], [7, 8], [7, 9, 2]]), vocab_size=64)
    rows = lambda rcbs: [(r, r.current_instruction()) for r in rcbs]
    assert ex.masked_rows(rows([plain, guided])) and not ex.masked_rows(rows([plain, sampled]))
    assert not ex.masked_rows([(NS(sampling_params=None), NS(is_chunked=False))]), "a stand-in without the attribute"
    fill = _executor(log)
    _step(fill, [plain, guided, sampled])
    assert log == ["forward_logits", ("sample_rows_masked", [-1, 0, -1], None, None, (1, 2))]
    assert (plain.output_token_ids, guided.output_token_ids) == ([11], [7]) and not guided.is_finished()
    del log[:]
    _step(fill, [guided, plain])
    assert log == ["forward_logits", ("sample_rows_masked", [0, -1], None, None, (1, 2))]
    assert guided.output_token_ids == [7, 9] and not guided.is_finished()
    _step(fill, [guided])
    assert guided.output_token_ids == [7, 9, 2] and guided.token_mask.finished
    assert guided.is_finished() and len(guided.output_token_ids) < guided.sampling_params.max_tokens, \
        "a complete choice ends the request"


def test_rows_on_one_node_share_a_mask_and_a_chunk_head_does_not_advance(monkeypatch):
    log = []
    _patch_kernels(monkeypatch, log, pick=min)
    c = InstructionCreator(image_token_id=63, n_image_tokens_per_image=4, block_size=16)
    a = c.process(_request(allowed_token_ids=[20, 30]), vocab_size=64)
    head = c.process(_request(guided_choice=[[5, 6], [7]], token_ids=(1, 2, 3, 4, 5, 6)), vocab_size=64)
    head.current_instruction().chunk_prefill(2)
    assert head.current_instruction().is_chunked and head.current_instruction().sample
    assert ex.masked_rows([(head, head.current_instruction())]) is False, "a chunk head delivers nothing"
    fill = _executor(log)
    _step(fill, [a, head])
    assert log[-1] == ("sample_rows_masked", [0, -1], None, None, (1, 2)), "the chunk head rides along unmasked"
    assert a.output_token_ids == [20] and head.output_token_ids == [] and head.token_mask.node == 0
    root = head.token_mask.current()
    _step(fill, [a, head])              # the rest of the prompt: now it delivers, from the root
    assert log[-1] == ("sample_rows_masked", [0, 1], None, None, (2, 2))
    assert head.output_token_ids == [5] and head.token_mask.current() is not root and not head.token_mask.finished
    _step(fill, [head, a])
    assert head.output_token_ids == [5, 6] and head.is_finished() and a.output_token_ids == [20, 20, 20]


def test_a_batch_without_masks_makes_the_calls_it_made(monkeypatch):
    log = []
    monkeypatch.setattr(ex, "sample_rows_masked", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("masked launch")))
    c = InstructionCreator(image_token_id=63, n_image_tokens_per_image=4, block_size=16)
    fill = _executor(log)
    rcbs = [c.process(_request(), vocab_size=64), c.process(_request())]
    _step(fill, rcbs)
    assert log == ["forward"] and [r.output_token_ids for r in rcbs] == [[11], [11]]
    seen = []
    monkeypatch.setattr(ex, "sample_rows_constrained", lambda logits, *t: seen.append(len(t)) or torch.tensor([11, 11]))
    fill.language_model.forward_constrained = lambda i, f, p, params, *t: ex.sample_rows_constrained(None, *t)
    _step(fill, [c.process(_request(logit_bias={5: 1.0}), vocab_size=64), c.process(_request())])
    assert seen == [8], "the constrained mode's launch, with its eight tables"
    assert ex.SAMPLING_MODES == {"constrained": (4, "pack_constrained_step", "forward_constrained", "sample_rows_constrained"),
                                 "drawn": (3, "pack_sample_step", "forward_sampled", "sample_rows"),
                                 "penalised": (2, "pack_penalty_step", "forward_penalized", "penalized_argmax_rows")}


def test_decode_rows_sends_a_masked_request_to_the_eager_path():
    c = InstructionCreator(image_token_id=63, n_image_tokens_per_image=4, block_size=16)
    fill = object.__new__(ex.BatchFillExecutor)
    fill.kv_manager, fill.pending = NS(block_size=16), None
    fill.graph_decoder = NS(fits=lambda n, b: True)
    for fields, eager in (({}, False), (dict(allowed_token_ids=[3]), True), (dict(guided_choice=[[3, 4]]), True)):
        rcb = c.process(_request(**fields), vocab_size=64)
        rcb.virtual_kv_cache = NS(block_table=[0])
        while len(getattr(rcb.current_instruction(), "token_ids", None) or ()) != 1:
            rcb.step()
        rcb.current_instruction().token_ids = [9]
        assert (fill._decode_rows(BatchRequest([rcb])) is None) == eager, fields


# ---------------------------------------------------------------------------------------------------- the protocol
def _body(**extra):
    return dict({"model": "m", "messages": [{"role": "user", "content": "hi"}], "stream": True}, **extra)


def test_protocol_parses_the_fields():
    plain = proto.parse_chat_completion_request(_body())
    assert plain.allowed_token_ids is None and plain.guided_choice is None
    assert plain == proto.parse_chat_completion_request(_body(allowed_token_ids=None, guided_choice=None))
    r = proto.parse_chat_completion_request(_body(allowed_token_ids=[5, 9, 2]))
    assert r.allowed_token_ids == [5, 9, 2] and r.guided_choice is None and r != plain
    r = proto.parse_chat_completion_request(_body(guided_choice=["yes", "no", "not sure"], temperature=0.5, prompt_logprobs=1))
    assert r.guided_choice == ["yes", "no", "not sure"] and r.allowed_token_ids is None
    r = proto.parse_chat_completion_request(_body(guided_choice=["A"], logprobs=True, logprobs_mode="processed_logprobs"))
    assert r.guided_choice == ["A"] and r.logprobs
    import dataclasses
    assert dataclasses.fields(proto.ChatRequest)[-1].name == "prompt_logprobs"


@pytest.mark.parametrize("bad", [
    dict(allowed_token_ids=[1], guided_choice=["a"]), dict(allowed_token_ids=[]), dict(allowed_token_ids="1"),
    dict(allowed_token_ids=[1, 1]), dict(allowed_token_ids=[True]), dict(allowed_token_ids=[1.5]), dict(allowed_token_ids=[-1]),
    dict(guided_choice=[]), dict(guided_choice="yes"), dict(guided_choice=[""]), dict(guided_choice=[1]),
    dict(guided_choice=["a", "a"]), dict(guided_choice=[str(i) for i in range(65)]),
    dict(allowed_token_ids=[1], logprobs=True), dict(guided_choice=["a"], logprobs=True, logprobs_mode="raw_logprobs"),
    dict(guided_choice=["a"], min_tokens=1)])
def test_protocol_refuses(bad):
    with pytest.raises(proto.ProtocolError):
        proto.parse_chat_completion_request(_body(**bad))


def test_server_encodes_the_choices_and_checks_the_vocabulary():
    from hydrainfer_amd.entrypoint.api_server import ApiServer
    from hydrainfer_amd.entrypoint.tokenizer import SyntheticTokenizer
    tok = SyntheticTokenizer(image_token_id=32000)
    server = ApiServer(None, tok)
    parse = lambda **kw: server._token_request(proto.parse_chat_completion_request(_body(**kw)))
    plain = parse().sampling_params
    assert plain == SamplingParameters(max_tokens=16) and plain.allowed_token_ids is None and plain.guided_choice is None
    sp = parse(guided_choice=["yes", "not sure"]).sampling_params
    assert sp.guided_choice == [tok.encode("yes"), tok.encode("not sure")] and len(sp.guided_choice[1]) == 2
    assert parse(allowed_token_ids=[5, 31999]).sampling_params.allowed_token_ids == [5, 31999]
    with pytest.raises(proto.ProtocolError, match="vocabulary"):
        parse(allowed_token_ids=[5, tok.vocab_size])
    with pytest.raises(proto.ProtocolError, match="encodes to no token"):
        parse(guided_choice=["yes", "   "])
    with pytest.raises(proto.ProtocolError, match="prefix"):
        parse(guided_choice=["not", "not sure"])


# ---------------------------------------------------------------------------------------------------- the binding
def test_the_library_exports_the_entry():
    assert "hx_sample_rows_masked" in _lib.exported_symbols()
    assert "hx_sample_rows_masked" in open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    f = _lib.lib().hx_sample_rows_masked
    assert len(f.argtypes) == 27
    assert _lib.lib().hx_abi_version() == 3
    # the argument checks run before anything touches the device: HX_ERR_SHAPE for rows = 0, HX_ERR_NULL for no mask_row
    args = [1, None, None, 1, 0, 8, 8, None, None, None, 0, None, None, None, None, 0, 1, None, None, None, 0, None, None, 0,
            1, _lib.HX_F16, None]
    assert f(*args) == -2
    args[4] = 1
    args[24] = None
    assert f(*args) == -4
    args[24], args[23] = 1, -1
    assert f(*args) == -2


def test_the_new_kernel_uses_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = [r for r in kernel_table.kernels() if r["name"].startswith("sample_rows_masked_kernel<")]
    assert sorted(r["name"] for r in rows) == ["sample_rows_masked_kernel<BF16>", "sample_rows_masked_kernel<F16>"]
    for r in rows:      # as its siblings: no scratch memory, no vector register spilled to it, 16 waves of 64 per row
        assert r.get("private_segment_fixed_size", 0) == 0 and r.get("vgpr_spill_count", 0) == 0, r
        assert r["wavefront_size"] == 64 and r["vgpr_count"] <= 128, r
