"""GPU: per-token log-probabilities through the engine (SamplingParameters.logprobs / top_logprobs -> the eager step's
forward_logprobs -> rcb.output_logprobs -> OfflineInferenceOutput), on the tiny model of tests/engine_util.py.  Asking
never changes a token; a record per delivered token, none for a chunk head's discarded sample, none for requests that
did not ask; every recorded value within 1e-4 of float64 log-softmax."""
import math

import pytest
import torch

from hydrainfer_amd.engine import BatchSchedulerConfig, InstructionCreator, SamplingParameters, TokenRequest
from hydrainfer_amd.engine.node import LocalCluster
from tests.engine_util import make_node, run_trace
from tests.golden import cases as C
from tests.logprob_ref import ATOL, reference

pytestmark = pytest.mark.gpu

N_IMG_TOK = (C.TINY_CLIP["image_size"] // C.TINY_CLIP["patch_size"]) ** 2
BS = C.TINY_BLOCK_SIZE
DT = torch.float16


class LogprobTap:
    """A LlavaLanguageModel that keeps the logits of every sampling step (fp16, on the host), whichever of forward /
    forward_logprobs the executor calls — and counts the device-to-host copies it makes itself out of the picture by
    doing them after the step's launch."""

    def __init__(self, lm):
        self.lm, self.language_model, self.image_token_id = lm, lm.language_model, lm.image_token_id
        self.steps = []          # (kind, logits [rows, vocab] on the CPU, the request ids of those rows)
        self.current = None      # set by the fill executor's wrapper: the requests that sample in the batch being run

    def embed(self, *a):
        return self.lm.embed(*a)

    def forward_logits(self, *a):
        return self.lm.forward_logits(*a)

    def forward(self, input_ids, image_features, position_ids, params):
        logits = self.lm.forward_logits(input_ids, image_features, position_ids, params)
        self.steps.append(("plain", logits.cpu(), self.current))
        return logits.argmax(-1)

    def forward_logprobs(self, input_ids, image_features, position_ids, params, top_k=0, out=None):
        from hydrainfer_amd._C.kernel.norm import logprob_rows
        logits = self.lm.forward_logits(input_ids, image_features, position_ids, params)
        res = logprob_rows(logits, top_k, out)
        self.steps.append(("logprobs", logits.cpu(), self.current))
        return res


def _models():
    from hydrainfer_amd.model.clip import ClipShape, LlavaVisionModel, random_state_dict
    from hydrainfer_amd.model.llama import LlamaForCausalLM, LlamaShape
    from hydrainfer_amd.model.llava import LlavaLanguageModel
    dev = torch.device("cuda:0")
    lshape, cshape = LlamaShape(**C.TINY_LLAMA), ClipShape(**C.TINY_CLIP)
    lm = LlavaLanguageModel(LlamaForCausalLM.from_reference_state_dict(lshape, C.tiny_llama_state_dict(DT), DT, dev),
                            image_token_id=C.TINY_IMAGE_TOKEN_ID)
    clip = {k: v.to(DT).to(dev) for k, v in random_state_dict(cshape, seed=3, std=0.05).items()}
    return lm, LlavaVisionModel(cshape, DT, dev, clip), lshape


def _cluster(chunked, graph_decode, budget=40):
    from hydrainfer_amd.memory.token_cache_manger import (TokenCacheBlockManager, TokenCacheBlockManagerConfig,
                                                          TokenCacheBlockManagerContext)
    lm, vision, lshape = _models()
    tap = LogprobTap(lm)
    ctx = TokenCacheBlockManagerContext(rank=0, rank2host={0: "localhost"})
    kv = TokenCacheBlockManager(TokenCacheBlockManagerConfig(
        n_layers=lshape.num_hidden_layers, n_tokens=2, n_blocks=48, block_size=BS, n_heads=lshape.num_key_value_heads,
        head_size=lshape.head_dim, dtype="fp16", device="cuda:0"), ctx)
    img = TokenCacheBlockManager(TokenCacheBlockManagerConfig(
        n_layers=1, n_tokens=1, n_blocks=6, block_size=N_IMG_TOK, n_heads=lshape.num_attention_heads,
        head_size=lshape.head_dim, dtype="fp16", device="cuda:0"), ctx)
    cfg = BatchSchedulerConfig(priority="prefill", max_running_requests=6, chunked_prefill=chunked, token_budgets=budget,
                               image_budgets=2)
    node = make_node("EPD0", "EPD", tap, vision, kv, img, lshape, DT, torch.device("cuda:0"), cfg, graph_decode=graph_decode)
    fill = node.executor.fill_executor
    real = fill.execute

    def execute(batch):
        tap.current = [rcb.request_id for rcb, inst in batch if inst.sample]
        real(batch)
    fill.execute = execute
    return LocalCluster([node]), tap


def _creator():
    return InstructionCreator(image_token_id=C.TINY_IMAGE_TOKEN_ID, n_image_tokens_per_image=N_IMG_TOK, block_size=BS,
                              ignore_eos=True)


def _requests(ask, text_len=(10, 45, 3, 28, 17, 33), max_tokens=(5, 3, 6, 4, 7, 2), eos=()):      # eos: {request: its ids}
    """ask[i]: None, or the request's top_logprobs.  Requests 0, 1, 2, 4, 5 carry an image, request 3 is text only."""
    g = torch.Generator().manual_seed(4242)
    pixels = C.tiny_clip_pixels(2)
    out = []
    for i, (n, m) in enumerate(zip(text_len, max_tokens)):
        text = torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (n,), generator=g).tolist()
        has_image = i != 3
        sp = SamplingParameters(max_tokens=m, eos_token_ids=list(dict(eos).get(i, ())))
        if ask[i] is not None:
            sp.logprobs, sp.top_logprobs = True, ask[i]
        out.append((0 if i < 3 else 2, TokenRequest(
            request_id=i, token_ids=([C.TINY_IMAGE_TOKEN_ID] if has_image else []) + text,
            pixel_values=pixels[i % 2:i % 2 + 1].clone() if has_image else None, image_size=(56, 56),
            image_hash=9000 + i % 2, sampling_params=sp)))
    return out


def _kept_logits(rcbs, tap):
    """request -> the logits rows of its delivered tokens, for the requests whose every sampling step ran eagerly (those
    that asked).  A chunk head's row is discarded like its sample: the kept ones are a request's last len(output) rows."""
    seq = {rcb.request_id: [] for rcb in rcbs}
    for _, logits, ids in tap.steps:
        assert logits.shape[0] == len(ids)
        for j, r in enumerate(ids):
            seq[r].append(logits[j])
    return {rcb.request_id: seq[rcb.request_id][-len(rcb.output_token_ids):] for rcb in rcbs}, seq


def _check_records(rcbs, ask, kept):
    worst, n = 0.0, 0
    for rcb, k in zip(rcbs, ask):
        if k is None:
            assert rcb.output_logprobs == []
            continue
        assert len(rcb.output_logprobs) == len(rcb.output_token_ids) == len(kept[rcb.request_id])
        ref = reference(torch.stack(kept[rcb.request_id]), k)
        for s, rec in enumerate(rcb.output_logprobs):
            assert rec.token_id == rcb.output_token_ids[s] == int(ref[0][s])
            assert len(rec.top) == k and [t for t, _ in rec.top] == ref[2][s].tolist()
            for got, want in [(rec.logprob, float(ref[1][s]))] + [(lp, float(w)) for (_, lp), w in zip(rec.top, ref[3][s])]:
                assert math.isfinite(got)
                worst, n = max(worst, abs(got - want)), n + 1
    print(f"{n} recorded logprobs, max |error| vs float64 log-softmax of the step's own logits: {worst:.2e}")
    assert n > 0 and worst <= ATOL
    return n


@pytest.mark.parametrize("graph_decode", [False, True], ids=["eager", "graphs"])
def test_asking_for_logprobs_does_not_change_tokens(graph_decode):
    plain = run_trace(_cluster(True, graph_decode)[0], _creator(), _requests([None] * 6))
    cluster, tap = _cluster(True, graph_decode)
    asked = run_trace(cluster, _creator(), _requests([5] * 6))
    assert [r.output_token_ids for r in asked] == [r.output_token_ids for r in plain]
    assert all(len(r.output_token_ids) == r.sampling_params.max_tokens for r in asked)
    assert all(kind == "logprobs" for kind, _, _ in tap.steps[-3:])


@pytest.mark.parametrize("graph_decode", [False, True], ids=["eager", "graphs"])
def test_mixed_batch_records(graph_decode):
    ask = [0, None, 3, 20, None, None]
    cluster, tap = _cluster(False, graph_decode)
    rcbs = run_trace(cluster, _creator(), _requests(ask))
    assert _check_records(rcbs, ask, _kept_logits(rcbs, tap)[0]) >= 5 + 6 * 4 + 4 * 21
    fill = cluster.nodes[0].executor.fill_executor
    assert fill.pending is None and fill.cohort is None


def test_chunked_prefill_and_eos():
    """token_budgets 16: the 45- and 33-token prompts are prefilled in chunks whose heads sample a token that is thrown
    away — no record for those; and a request whose eos id comes up ends there, records included."""
    ask = [2, 4, None, 1, 0, 3]
    cluster, tap = _cluster(True, False, budget=16)
    rcbs = run_trace(cluster, _creator(), _requests(ask))
    kept, sampled = _kept_logits(rcbs, tap)
    assert any(len(sampled[r.request_id]) > len(r.output_token_ids) for r in rcbs if r.sampling_params.logprobs), "no chunk head sampled"
    _check_records(rcbs, ask, kept)
    # the same trace with request 2's third token as its end-of-sequence id
    first = run_trace(_cluster(True, False, budget=16)[0], _creator(), _requests([1] * 6))
    eos = first[2].output_token_ids[2]
    cut = first[2].output_token_ids.index(eos) + 1
    again = run_trace(_cluster(True, False, budget=16)[0], _creator(), _requests([1] * 6, eos={2: [eos]}))
    assert again[2].output_token_ids == first[2].output_token_ids[:cut] and cut <= 3
    for rcb in again:
        assert [rec.token_id for rec in rcb.output_logprobs] == rcb.output_token_ids


def test_offline_engine_returns_logprobs():
    from hydrainfer_amd.engine.offline import OfflineInferenceEngine, OfflineRequest
    lm, vision, _ = _models()
    eng = OfflineInferenceEngine(lm, vision, DT, "cuda:0", max_running_requests=4, token_budgets=64, max_context=256,
                                 warm_up=False)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, C.TINY_IMAGE_TOKEN_ID, (6 + 5 * i,), generator=g).tolist() for i in range(4)]
    plain = eng.generate([OfflineRequest(p, None, max_tokens=4) for p in prompts])
    asked = eng.generate([OfflineRequest(p, None, max_tokens=4, logprobs=i != 1, top_logprobs=(0, 0, 2, 20)[i])
                          for i, p in enumerate(prompts)])
    assert [o.output_token_ids for o in asked] == [o.output_token_ids for o in plain]
    assert all(o.output_logprobs == [] for o in plain) and asked[1].output_logprobs == []
    for i in (0, 2, 3):
        recs = asked[i].output_logprobs
        assert [r.token_id for r in recs] == asked[i].output_token_ids
        assert all(len(r.top) == (0, 0, 2, 20)[i] and -math.log(C.TINY_LLAMA["vocab_size"]) - 20 < r.logprob <= 0 for r in recs)
        assert all(r.top[0] == (r.token_id, r.logprob) for r in recs if r.top)
        assert all(r.top[j][1] >= r.top[j + 1][1] for r in recs for j in range(len(r.top) - 1))
    with pytest.raises(ValueError):
        eng.generate([OfflineRequest(prompts[0], None, max_tokens=2, top_logprobs=3)])
