"""CPU: focal image-token pruning — the restatement (tests/focal_ref.py) against hand-worked examples and the reference's
own score fixture, the request -> instruction wiring (counts, cache ids, positions, prefix-cache hashes, refusals) and
the three new C-ABI entries."""
import ctypes
import json
import math
import os
import re

import pytest
import torch

from tests import focal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = 32000


# ------------------------------------------------------------------ the restatement
def _qk_1head(qv, kv):
    """4 tokens, 1 head, head dim 1 (scale 1): S[i, j] = q_i * k_j."""
    q = torch.tensor(qv, dtype=torch.float32).reshape(1, -1, 1, 1)
    k = torch.tensor(kv, dtype=torch.float32).reshape(1, -1, 1, 1)
    return q, k


def test_hand_worked_query_side():
    """q = (4, 1, 2, 2), k = 1: S[i, j] = q_i, so s1 is constant (variance 0) and s2 = q wins.  'rank', n = 2: token 0, then
    the exact tie 2 == 2 goes to the lower index -> {0, 2}.  'row' on the 2 x 2 grid: row sums (5, 4) -> row 0 = {0, 1}."""
    q, k = _qk_1head([4, 1, 2, 2], [1, 1, 1, 1])
    s1, s2 = R.significance(q, k)
    assert torch.equal(s1[0], torch.full((4,), 2.25)) and torch.equal(s2[0], torch.tensor([4.0, 1.0, 2.0, 2.0]))
    tokens = torch.arange(8.0).reshape(1, 4, 2)
    rows, ids = R.focal_prunning(tokens, q, k, 2, "rank")
    assert ids[0].tolist() == [0, 2] and torch.equal(rows[0], tokens[0, [0, 2]])
    assert R.focal_prunning(tokens, q, k, 2, "row")[1][0].tolist() == [0, 1]
    assert R.focal_prunning(tokens, q, k, 4, "rank")[1][0].tolist() == [0, 1, 2, 3]
    assert R.focal_prunning(tokens, q, k, 1, "rank")[1][0].tolist() == [0]


def test_hand_worked_key_side_and_skip_leading():
    """q = 1, k = (9, 1, 5, 2, 7) with the leading token skipped: S[i, j] = k_j over tokens 1..4, s2 constant, s1 = (1, 5, 2, 7)
    wins; n = 2 keeps patch tokens {1, 3}; rows (6, 9) -> 'row' keeps {2, 3}.  The skipped token (the largest k) plays
    no part."""
    q, k = _qk_1head([1, 1, 1, 1, 1], [9, 1, 5, 2, 7])
    s1, s2 = R.significance(q, k, skip_leading=1)
    assert torch.equal(s1[0], torch.tensor([1.0, 5.0, 2.0, 7.0])) and torch.var(s2[0]).item() == 0
    tokens = torch.arange(8.0).reshape(1, 4, 2)
    assert R.focal_prunning(tokens, q, k, 2, "rank", skip_leading=1)[1][0].tolist() == [1, 3]
    assert R.focal_prunning(tokens, q, k, 2, "row", skip_leading=1)[1][0].tolist() == [2, 3]


def test_equal_variances_choose_s2():
    s = torch.tensor([3.0, -1.0, 0.5, 2.0])
    assert R.select_one(-s, s, 2, "rank").tolist() == [0, 3]        # s2 = s: tokens 0 and 3; s1 = -s would keep 1 and 2


def test_reference_score_fixture():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "focal_scores_fixture.json")))
    S = torch.tensor(fx["scores"], dtype=torch.float32)[None]          # [1, H, N, N]
    s1, s2 = R.significance_from_scores(S)
    assert R.select(s1, s2, fx["n_keep"], fx["strategy"])[0].tolist() == fx["kept"]


@pytest.mark.parametrize("shift", ["k", "q"])
def test_collapsed_form_is_the_rule(shift):
    """What the fused kernel computes — s2[i] = scale / (H N) sum_h q[i,h,:] . (sum_j k[j,h,:]) and s1 alike — IS the
    materialised rule: fp64 against fp64, 1e-12 of the range."""
    g = torch.Generator().manual_seed(5)
    B, T, H, D = 2, 50, 4, 16
    q = torch.randn((B, T, H, D), generator=g).half() + (0.3 if shift == "q" else 0.0)
    k = torch.randn((B, T, H, D), generator=g).half() + (0.3 if shift == "k" else 0.0)
    s1, s2 = R.significance(q, k, skip_leading=1, dtype=torch.float64)
    qd, kd = q[:, 1:].double(), k[:, 1:].double()
    f = 1.0 / math.sqrt(D) / (H * (T - 1))
    c2 = f * torch.einsum("bihd,bhd->bi", qd, kd.sum(dim=1))
    c1 = f * torch.einsum("bjhd,bhd->bj", kd, qd.sum(dim=1))
    rng = (s1.max() - s1.min()).item() + (s2.max() - s2.min()).item()
    assert (c1 - s1).abs().max().item() < 1e-12 * rng and (c2 - s2).abs().max().item() < 1e-12 * rng
    v1, v2 = torch.var(s1[0]).item(), torch.var(s2[0]).item()
    assert (v2 > v1) == (shift == "k")                                   # the shift decides which side wins


# ------------------------------------------------------------------ request -> instructions
def _creator(**kw):
    from hydrainfer_amd.engine import InstructionCreator
    return InstructionCreator(image_token_id=IMG, n_image_tokens_per_image=576, block_size=16, **kw)


def _request(token_params=None, text_before=0, text_after=40, image=True, rid=1):
    from hydrainfer_amd.engine import SamplingParameters, TokenRequest
    ids = list(range(100, 100 + text_before)) + ([IMG] if image else []) + list(range(300, 300 + text_after))
    return TokenRequest(request_id=rid, token_ids=ids, pixel_values=torch.zeros(1, 3, 4, 4) if image else None,
                        image_hash=0x1234_5678_9ABC, sampling_params=SamplingParameters(max_tokens=5),
                        token_params=token_params)


def _chain(rcb):
    return list(rcb.instructions)[1:-1]


def test_focal_request_expands_to_n_tokens():
    from hydrainfer_amd.engine import ImageEmbed, ImageEmbedFill, TokenParameters
    rcb = _creator().process(_request(TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=64)))
    md = rcb.request_metadata
    assert (md.n_prompt_tokens, md.n_image_tokens, md.n_text_tokens, md.n_images) == (64 + 40, 64, 40, 1)
    embed, fill = _chain(rcb)[0], _chain(rcb)[3]
    assert isinstance(embed, ImageEmbed) and isinstance(fill, ImageEmbedFill)
    assert embed.cache_ids == list(range(64)) and embed.n_keep == 64 and embed.strategy == "rank"
    assert fill.image_token_cache_ids == list(range(64))
    assert fill.token_ids == [IMG] * 64 + list(range(300, 340)) and sum(fill.image_token_mask) == 64
    assert fill.position_ids == list(range(104)) and fill.cache_ids == list(range(104))
    decodes = _chain(rcb)[6:]
    assert [d.position_ids[0] for d in decodes] == list(range(104, 108))
    assert len(fill.hashes) == 104 // 16


def test_unpruned_request_is_unchanged():
    """token_params = None, a default TokenParameters() and a text request with pruning asked for: today's chain and hashes."""
    from hydrainfer_amd.engine import TokenParameters
    from hydrainfer_amd.memory.shared_cache import compute_hash

    def summary(rcb):
        return [(type(i).__name__, getattr(i, "token_ids", None), getattr(i, "position_ids", None),
                 getattr(i, "cache_ids", None), getattr(i, "hashes", None), getattr(i, "image_token_cache_ids", None))
                for i in _chain(rcb)]
    base = _creator().process(_request(None))
    assert summary(_creator().process(_request(TokenParameters()))) == summary(base)
    embed = _chain(base)[0]
    assert embed.n_keep is None and embed.hashes == [0x1234_5678_9ABC] and embed.cache_ids == list(range(576))
    # the hash chain itself, as it was before the feature: the image hash stands in for 575 placeholders
    want = compute_hash([0x1234_5678_9ABC] * 575 + [IMG] + list(range(300, 340)), 16, -1)
    assert _chain(base)[3].hashes == want and base.request_metadata.n_image_tokens == 576
    text = _creator().process(_request(None, image=False))
    focal_text = _creator().process(_request(TokenParameters(token_pruning_policy="focal"), image=False))
    assert summary(focal_text) == summary(text)


@pytest.mark.parametrize("text_before", [0, 20])
def test_pruned_and_unpruned_prompts_share_no_image_block(text_before):
    from hydrainfer_amd.engine import TokenParameters
    from hydrainfer_amd.engine.request_processor import pruned_image_hash
    tp = TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=64)
    full = _chain(_creator().process(_request(None, text_before)))[3].hashes
    pruned = _chain(_creator().process(_request(tp, text_before)))[3].hashes
    n_text_blocks = text_before // 16                   # blocks of text in front of the image: the same prompt prefix
    assert pruned[:n_text_blocks] == full[:n_text_blocks]
    assert not set(pruned[n_text_blocks:]) & set(full), "a block with an image stand-in is shared"
    # other counts / strategies of the same image do not share either
    other = _chain(_creator().process(_request(TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=144),
                                               text_before)))[3].hashes
    row = _chain(_creator(pruning_strategy="row").process(_request(TokenParameters(token_pruning_policy="focal",
                                                                                   n_embed_output_tokens=72), text_before)))
    assert not set(pruned[n_text_blocks:]) & set(other) and row[0].strategy == "row"
    h = 0x1234_5678_9ABC
    stand_ins = {pruned_image_hash(h, 64, "rank"), pruned_image_hash(h, 144, "rank"), pruned_image_hash(h, 64, "row"), h}
    assert len(stand_ins) == 4 and all(0 <= s < 2 ** 63 for s in stand_ins)
    assert _chain(_creator().process(_request(tp)))[0].hashes == [pruned_image_hash(h, 64, "rank")]


def test_declared_but_unimplemented_is_refused():
    from hydrainfer_amd.engine import TokenParameters
    c = _creator()
    with pytest.raises(ValueError, match="kv_cache_eviction_policy"):
        c.process(_request(TokenParameters(kv_cache_eviction_policy="streamingllm")))
    with pytest.raises(ValueError, match="token_pruning_policy"):
        c.process(_request(TokenParameters(token_pruning_policy="fastv")))
    for n in (0, 577, -3):
        with pytest.raises(ValueError, match="n_embed_output_tokens"):
            c.process(_request(TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=n)))
    with pytest.raises(ValueError, match="multiple"):
        _creator(pruning_strategy="row").process(_request(TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=64)))
    assert c.process(_request(TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=576))).request_metadata.n_image_tokens == 576
    assert c.process(_request(TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=1))).request_metadata.n_prompt_tokens == 41


def test_token_parameters_fields():
    import dataclasses
    from hydrainfer_amd.engine import TokenParameters
    from hydrainfer_amd.engine.offline import OfflineRequest
    got = [(f.name, f.default) for f in dataclasses.fields(TokenParameters)]
    assert got == [("kv_cache_eviction_policy", None), ("window_size", 28), ("attention_sink_size", 4),
                   ("token_pruning_policy", None), ("n_embed_output_tokens", 64)]
    assert OfflineRequest(token_ids=[1]).token_params is None


def test_counts_are_checked_on_the_host():
    from hydrainfer_amd.layer.token_prunning import check_counts, keep_counts
    check_counts([1, 64, 576], 576, "rank")
    check_counts([24, 576], 576, "row")
    for bad in ([0], [577]):
        with pytest.raises(ValueError):
            check_counts(bad, 576, "rank")
    with pytest.raises(ValueError):
        check_counts([64], 576, "row")
    with pytest.raises(ValueError):
        check_counts([5], 575, "row")
    with pytest.raises(ValueError):
        check_counts([5], 576, "column")
    t, n_max = keep_counts([3, 9], 2, 16, "rank", "cpu")
    assert t.dtype == torch.int32 and t.tolist() == [3, 9] and n_max == 9


# ------------------------------------------------------------------ C ABI
def _declared_arity(name):
    src = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    args = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, re.S).group(1)
    return len([a for a in args.split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("hx_focal_significance", 16), ("hx_focal_select", 8), ("hx_focal_gather", 11),
                                        ("hx_focal_significance_workspace_bytes", 3)])
def test_focal_symbols_are_exported_with_the_declared_arity(name, arity):
    from hydrainfer_amd import _lib
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _declared_arity(name) == arity == len(_lib._SIGNATURES[name][1])
    l = _lib.lib()
    assert l.hx_focal_significance_workspace_bytes(8, 16, 64) > 0
    # limits are statuses, not assertions (no launch happens: the checks come first)
    assert l.hx_focal_significance(None, None, None, None, 1, 577, 1, 16, 60, 3072, 3072, 0.125, None, 0, _lib.HX_F16, None) == -2
    assert l.hx_focal_significance(None, None, None, None, 1, 5000, 1, 16, 64, 3072, 3072, 0.125, None, 0, _lib.HX_F16, None) == -2
    assert l.hx_focal_significance(None, None, None, None, 1, 577, 1, 16, 64, 3072, 3072, 0.125, None, 0, _lib.HX_F32, None) == -1
    assert l.hx_focal_select(None, None, None, None, 1, 575, _lib.HX_FOCAL_ROW, None) == -2
    assert l.hx_focal_select(None, None, None, None, 1, 4097, _lib.HX_FOCAL_RANK, None) == -2
    assert l.hx_focal_gather(None, None, None, None, 1, 576, 4100, 4100, 4100, _lib.HX_F16, None) == -2
    assert l.hx_focal_gather(None, None, None, None, 1, 576, 4096, 4096, 4096, 7, None) == -1
