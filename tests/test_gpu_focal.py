"""GPU: focal image-token pruning — hx_focal_significance / hx_focal_select / hx_focal_gather, the layer surface, the
vision model, graph and launch-plan capture, and the engine — against the restatement in tests/focal_ref.py.

Measured on an MI355X (test_significance_matches_fp64, randn inputs, k shifted by +0.3): the kernel's error against fp64
is 0.97 - 1.61 x e_ref over the ten cases (CLIP shape, 1 / 3 / 8 images: 1.11 - 1.61; H 8 / D 128: 0.97 - 1.13;
skip_leading = 0: 1.23 - 1.30), e_ref itself being 4 - 8e-8 of the range of sig; the bound is 4 x e_ref."""
import math

import pytest
import torch

from tests import focal_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]


def _qk(n_images, T, H, D, dt, seed, shift="k"):
    """q, k [n_images, T, H, D] as strided views of ONE [n_images * T, 3 H D] buffer (the tower's fused qkv product).  k (or
    q) shifted by +0.3: the column sum of the shifted side is large, so the OTHER side's dot products spread and win."""
    g = torch.Generator().manual_seed(seed)
    W = H * D
    buf = torch.randn((n_images * T, 3 * W), generator=g)
    if shift == "k":
        buf[:, W:2 * W] += 0.3
    elif shift == "q":
        buf[:, :W] += 0.3
    buf = buf.to(dt)
    return buf, buf[:, :W].view(n_images, T, H, D), buf[:, W:2 * W].view(n_images, T, H, D)


def _dev_views(buf, n_images, T, H, D):
    d = buf.to(DEV)
    W = H * D
    return d[:, :W].view(n_images, T, W), d[:, W:2 * W].view(n_images, T, W)


def _e_ref(q, k, skip, device="cpu"):
    """(fp64 s1, s2; fp32 materialised s1, s2; e_ref = max |fp32 materialised - fp64| over both vectors)."""
    q, k = q.to(device), k.to(device)
    d1, d2 = R.significance(q, k, skip, torch.float64)
    f1, f2 = R.significance(q, k, skip, torch.float32)
    e = max((f1.double() - d1).abs().max().item(), (f2.double() - d2).abs().max().item())
    return (d1, d2), (f1, f2), e


# ------------------------------------------------------------------ significance
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 577, 1, 16, 64), (3, 577, 1, 16, 64), (8, 577, 1, 16, 64), (2, 577, 1, 8, 128),
                                   (2, 576, 0, 16, 64)], ids=lambda s: "x".join(map(str, s)))
def test_significance_matches_fp64(dt, shape):
    """hx_focal_significance vs the fp64 restatement, within 4 * e_ref (e_ref: the fp32 MATERIALISED restatement's own
    error against fp64 on the same inputs — two legitimate fp32 summation orders, each allowed the reference's own error,
    doubled for margin).  The test prints kernel error / e_ref per case; measured: 0.97 - 1.61 (module docstring)."""
    from hydrainfer_amd.layer.token_prunning import focal_significance
    n_images, T, skip, H, D = shape
    buf, q, k = _qk(n_images, T, H, D, dt, seed=11 + n_images)
    (d1, d2), _, e_ref = _e_ref(q, k, skip)
    qd, kd = _dev_views(buf, n_images, T, H, D)
    assert qd.stride(1) == 3 * H * D
    s1, s2 = focal_significance(qd, kd, n_images, T, H, D, skip_leading=skip)
    torch.cuda.synchronize()
    assert s1.shape == (n_images, T - skip) and s1.dtype == torch.float32
    err = max((s1.cpu().double() - d1).abs().max().item(), (s2.cpu().double() - d2).abs().max().item())
    rng = max((d1.max() - d1.min()).item(), (d2.max() - d2.min()).item())
    print(f"focal significance {shape} {dt}: kernel err {err:.3e} = {err / e_ref:.2f} x e_ref ({e_ref:.3e}, {e_ref / rng:.2e} of range)")
    assert err <= 4 * e_ref, f"kernel error {err:.3e} > 4 x e_ref {e_ref:.3e}"


def test_significance_refuses_bad_shapes():
    from hydrainfer_amd import _lib
    from hydrainfer_amd.layer.token_prunning import focal_significance
    x = torch.zeros((10, 3 * 120), dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.HydraHipError, match="size"):
        focal_significance(x[:, :60], x[:, 60:120], 1, 10, 1, 60)          # head_dim % 8
    y = torch.zeros((10, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.HydraHipError, match="data type"):
        focal_significance(y, y, 1, 10, 1, 64)


# ------------------------------------------------------------------ selection on given s1 / s2
def _select_gpu(s1, s2, counts, strategy):
    from hydrainfer_amd.layer.token_prunning import focal_select
    ids = focal_select(s1.to(DEV), s2.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), strategy)
    torch.cuda.synchronize()
    return ids.cpu()


def _check_select(s1, s2, counts, strategy):
    want = R.padded_ids(R.select(s1, s2, counts, strategy), s1.shape[1])
    got = _select_gpu(s1, s2, counts, strategy)
    assert torch.equal(got, want), f"{strategy} {counts}: ids differ"
    for b, n in enumerate(counts):
        assert (got[b, n:] == -1).all() and (got[b, :n] >= 0).all()
    return got


COUNTS = [1, 64, 144, 575, 576]


@pytest.mark.parametrize("N", [576, 100, 4096, 1500])
def test_select_random_vectors_mixed_counts(N):
    g = torch.Generator().manual_seed(N)
    counts = [min(c, N) for c in COUNTS]
    s1, s2 = torch.randn((5, N), generator=g), 0.5 * torch.randn((5, N), generator=g)      # var(s1) > var(s2)
    _check_select(s1, s2, counts, "rank")
    _check_select(s2, s1, counts, "rank")                                                   # the opposite


def test_select_exact_ties_across_the_cut():
    """Eight levels over 576 tokens: ~72 tokens per level, every cut falls inside a run of equal values -> lower index wins."""
    g = torch.Generator().manual_seed(3)
    s2 = torch.randint(0, 8, (5, 576), generator=g).float()
    s1 = torch.zeros((5, 576))
    got = _check_select(s1, s2, COUNTS, "rank")
    lvl = s2[1]
    kept = got[1, :64].long()
    cut = lvl[kept].min()
    assert (lvl == cut).sum() > (lvl[kept] == cut).sum() > 0                    # the cut really splits a tie
    tied = torch.nonzero(lvl == cut).flatten()
    assert torch.equal(torch.sort(kept[lvl[kept] == cut]).values, tied[: (lvl[kept] == cut).sum()])
    _check_select(torch.zeros((2, 576)), torch.zeros((2, 576)), [64, 576], "rank")          # all equal: ids 0..n-1


def test_select_variance_choice():
    g = torch.Generator().manual_seed(9)
    s = torch.randn((5, 576), generator=g)
    a = _check_select(-s, s, COUNTS, "rank")         # equal variances, bit for bit -> s2 (s1 = -s2 would keep the opposite end)
    b = _check_select(s, -s, COUNTS, "rank")
    assert not torch.equal(a[1], b[1])
    assert torch.equal(a, _select_gpu(torch.zeros_like(s), s, COUNTS, "rank"))
    assert torch.equal(b, _select_gpu(-s * 1.5, s, COUNTS, "rank"))                         # var(s1) > var(s2) -> s1


def test_select_rows():
    """'row': values are multiples of 1/64 below 8 in magnitude, so every row sum is exact in fp32 whatever the order."""
    g = torch.Generator().manual_seed(21)
    s2 = torch.randint(-512, 513, (5, 576), generator=g).float() / 64
    s1 = torch.zeros((5, 576))
    got = _check_select(s1, s2, [24, 72, 144, 552, 576], "row")
    assert (got[0, :24] // 24 == got[0, 0] // 24).all()                        # one whole grid row
    s2[3].view(24, 24)[5] = s2[3].view(24, 24)[17]                              # two rows with the same sum: the lower one first
    _check_select(s1, s2, [24, 72, 144, 24 * int((s2[3].view(24, 24).sum(1) > s2[3].view(24, 24)[5].sum()).sum()) + 24, 576], "row")
    _check_select(torch.randint(-64, 65, (3, 4096), generator=g).float() / 8, torch.zeros((3, 4096)), [64, 640, 4096], "row")
    from hydrainfer_amd import _lib
    with pytest.raises(_lib.HydraHipError, match="size"):
        _select_gpu(torch.zeros((1, 575)), torch.zeros((1, 575)), [5], "row")


# ------------------------------------------------------------------ end to end ids
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shift", ["k", "q"])
def test_fused_ids_equal_the_materialised_rule(dt, shift):
    """focal_prunning_qk vs the materialised restatement run on the GPU: seeds 0-5 (one image each) x n in {64, 144, 288}.
    Precondition, asserted (not skipped): the restatement's own gap at the cut is at least 8 x e_ref — then the id sets are
    equal.  Also 'row'."""
    from hydrainfer_amd.layer.token_prunning import focal_prunning_qk
    T, H, D = 577, 16, 64
    bufs = [_qk(1, T, H, D, dt, seed, shift) for seed in range(6)]
    buf = torch.cat([b[0] for b in bufs]).to(DEV)
    W = H * D
    q, k = buf[:, :W].view(6, T, H, D), buf[:, W:2 * W].view(6, T, H, D)
    (d1, d2), (f1, f2), e_ref = _e_ref(q, k, 1, DEV)
    assert (torch.var(f2[0]) > torch.var(f1[0])).item() == (shift == "k")
    tokens = torch.randn((6, T - 1, 256), device=DEV).to(dt)
    for n in (64, 144, 288):
        gaps = [R.cut_gap(f1[b], f2[b], n) for b in range(6)]
        assert min(gaps) >= 8 * e_ref, f"near-tie at the cut: gap {min(gaps):.3e} < 8 x e_ref {e_ref:.3e}"
        want_rows, want_ids = R.focal_prunning(tokens, q, k, n, "rank", 1)
        out, ids = focal_prunning_qk(tokens, q, k, n, "rank", skip_leading=1)
        torch.cuda.synchronize()
        assert out.shape == (6, n, 256)
        assert torch.equal(ids.cpu(), R.padded_ids(want_ids, T - 1)), f"n = {n}"
        assert torch.equal(out, torch.stack(want_rows))
    g_rows = [torch.sort(R.choose(f1[b], f2[b]).view(24, 24).sum(1), descending=True).values for b in range(6)]
    assert min((r[5] - r[6]).item() for r in g_rows) >= 8 * 24 * e_ref
    out, ids = focal_prunning_qk(tokens, q, k, 144, "row", skip_leading=1)
    assert torch.equal(ids.cpu(), R.padded_ids(R.focal_prunning(tokens, q, k, 144, "row", 1)[1], T - 1))


# ------------------------------------------------------------------ layer surface
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_return_scores_and_the_reference_signature(dt):
    """MultiHeadAttention(return_scores=True): the same `o` bit for bit, fp32 pre-softmax scaled logits within the
    worst-case bound of an fp32 dot product of D terms in any order, the rounding of q * scale included —
    (D + 2) * 2^-24 * sum |terms| <= (D + 2) * 2^-24 * D * max|q| * max|k| * scale; focal_prunning(tokens, scores, ...)
    over those scores (CLS row and column dropped) keeps the rows focal_prunning_qk keeps."""
    from hydrainfer_amd.layer.multihead_attention import (MultiHeadAttention, MultiHeadAttentionConfig,
                                                          MultiHeadAttentionParameters)
    from hydrainfer_amd.layer.token_prunning import focal_prunning, focal_prunning_qk
    B, T, H, D = 2, 577, 16, 64
    buf, q4, k4 = _qk(B, T, H, D, dt, seed=2)
    d = buf.to(DEV)
    W = H * D
    q, k, v = (d[:, i * W:(i + 1) * W].view(B, T, W) for i in range(3))
    attn = MultiHeadAttention(MultiHeadAttentionConfig(H, D))
    plain = attn(q, k, v, MultiHeadAttentionParameters())
    with_scores = attn(q, k, v, MultiHeadAttentionParameters(return_scores=True))
    assert plain.attention_scores is None and torch.equal(plain.o, with_scores.o)
    S = with_scores.attention_scores
    assert S.shape == (B, H, T, T) and S.dtype == torch.float32
    ref = R.scores(q4.to(DEV), k4.to(DEV), 0, torch.float64)
    bound = (D + 2) * 2.0 ** -24 * D * q4.float().abs().max().item() * k4.float().abs().max().item() / math.sqrt(D)
    err = (S.double() - ref).abs().max().item()
    print(f"return_scores {dt}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    tokens = torch.randn((B, T - 1, 128), device=DEV).to(dt)
    for n, strategy in ((64, "rank"), (144, "rank"), (144, "row")):
        a = focal_prunning(tokens, S[:, :, 1:, 1:], n, strategy)
        b, _ = focal_prunning_qk(tokens, q.view(B, T, H, D), k.view(B, T, H, D), n, strategy, skip_leading=1)
        assert a.shape == (B, n, 128) and torch.equal(a, b)


# ------------------------------------------------------------------ vision model
def _mid_clip(dt, image_size=336, patch_size=14):
    """3 layers, 2 heads of 64, 577 tokens (the CLIP-L/14-336 token grid at a fraction of the width)."""
    from hydrainfer_amd.model.clip import ClipShape, LlavaVisionModel, random_state_dict
    shape = ClipShape(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2,
                      image_size=image_size, patch_size=patch_size, projector_hidden_size=256)
    sd = {k: v.to(dt).to(DEV) for k, v in random_state_dict(shape, seed=3, std=0.05).items()}
    return LlavaVisionModel(shape, dt, DEV, sd)


def _pixels(n, size=336, seed=0):
    return torch.randn((n, 3, size, size), generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_vision_forward_pruned_equals_gathered_full(dt):
    model = _mid_clip(dt)
    px = _pixels(4)
    full = model(px)
    counts = [64, 576, 1, 144]
    out = model(px, counts)
    ids = model.last_kept_ids
    torch.cuda.synchronize()
    assert out.shape == (4, 576, 256) and ids.shape == (4, 576)
    for b, n in enumerate(counts):
        kept = ids[b, :n].long()
        assert (ids[b, n:] == -1).all() and (kept[1:] > kept[:-1]).all()
        assert torch.equal(out[b, :n], full[b, kept]), f"image {b}"
    assert torch.equal(model(px, 576), full)
    assert torch.equal(model(px), full)                                         # the unpruned path is deterministic too
    row = model(px, [24, 576, 48, 144], "row")
    assert torch.equal(row[0, :24], full[0, model.last_kept_ids[0, :24].long()])
    with pytest.raises(ValueError):
        model(px, [64, 0, 1, 1])
    with pytest.raises(ValueError):
        model(px, 100, "row")


def test_pruned_forward_in_a_graph_and_in_a_launch_plan():
    """One captured graph serves every mix of counts (n_keep is a device tensor); the three launches record into a launch
    plan; two eager runs are bit-identical."""
    from hydrainfer_amd.launch_plan import LaunchPlan
    from hydrainfer_amd.layer.token_prunning import focal_prunning_qk
    dt = torch.bfloat16
    model = _mid_clip(dt)
    px = _pixels(2, seed=4)
    n_a = torch.tensor([64, 144], dtype=torch.int32, device=DEV)
    n_b = torch.tensor([300, 7], dtype=torch.int32, device=DEV)
    eager = {}
    for name, t in (("a", n_a), ("b", n_b)):
        eager[name] = (model(px, t).clone(), model.last_kept_ids.clone())
        again = model(px, t)
        for b, n in enumerate(t.tolist()):
            assert torch.equal(again[b, :n], eager[name][0][b, :n])
        assert torch.equal(model.last_kept_ids, eager[name][1])
    static_px, static_n = px.clone(), n_a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model(static_px, static_n)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = model(static_px, static_n)
        static_ids = model.last_kept_ids
    for name, t in (("b", n_b), ("a", n_a)):
        static_n.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_ids, eager[name][1]), name
        for b, n in enumerate(t.tolist()):
            assert torch.equal(static_out[b, :n], eager[name][0][b, :n]), (name, b)
    # launch plan: significance (two kernels), select, gather
    buf, _, _ = _qk(2, 577, 16, 64, dt, seed=8)
    d = buf.to(DEV)
    q, k = d[:, :1024].view(2, 577, 16, 64), d[:, 1024:2048].view(2, 577, 16, 64)
    tokens = torch.randn((2, 576, 512), device=DEV).to(dt)
    want_out, want_ids = focal_prunning_qk(tokens, q, k, n_a, "rank", skip_leading=1)
    torch.cuda.synchronize()
    plan = LaunchPlan(DEV)
    out, ids = plan.capture(lambda: focal_prunning_qk(tokens, q, k, n_a, "rank", skip_leading=1))
    assert plan.n_launches == 4
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(ids, want_ids)
    for b, n in enumerate(n_a.tolist()):
        assert torch.equal(out[b, :n], want_out[b, :n])


# ------------------------------------------------------------------ engine
class _AttnTap:
    """Stands where LlavaVisionModel.attn stands and keeps the q, k of its last call (the last executed layer)."""

    def __init__(self, attn):
        self.attn, self.qk = attn, None

    def __call__(self, q, k, v, params):
        self.qk = (q, k)
        return self.attn(q, k, v, params)


class _HostPrunedVision:
    """The oracle for the engine test: the UNPRUNED forward, then — for the images listed in `prune` (matched by pixel
    content) — the restatement's selection computed on the host from the last layer's q and k, and the kept rows picked by
    plain indexing.  Returns the rows of all images back to back, which is all the unpruned executor path looks at."""

    def __init__(self, model, prune):
        self.model, self.prune, self.shape = model, prune, model.shape
        self.tap = model.attn = _AttnTap(model.attn)

    def forward(self, pixels):
        full = self.model.forward(pixels)
        q, k = self.tap.qk
        H = self.shape.num_attention_heads
        B, T, W = q.shape
        q4, k4 = q.reshape(B, T, H, W // H).cpu(), k.reshape(B, T, H, W // H).cpu()
        rows = []
        for b in range(B):
            n = next((n for px, n in self.prune if torch.equal(px.to(pixels), pixels[b])), None)
            if n is None:
                rows.append(full[b])
            else:
                s1, s2 = R.significance(q4[b:b + 1], k4[b:b + 1], 1)
                rows.append(full[b, R.select_one(s1[0], s2[0], n, "rank").to(full.device)])
        return torch.cat(rows)


def _engine(dname, prune=None, graphs=False):
    from hydrainfer_amd.engine import BatchSchedulerConfig
    from hydrainfer_amd.engine.node import LocalCluster
    from hydrainfer_amd.memory.token_cache_manger import (TokenCacheBlockManager, TokenCacheBlockManagerConfig,
                                                          TokenCacheBlockManagerContext)
    from hydrainfer_amd.model.llama import LlamaForCausalLM, LlamaShape
    from hydrainfer_amd.model.llava import LlavaLanguageModel
    from tests.engine_util import make_node
    from tests.golden import cases as C
    dt = C.DTYPES[dname]
    dev = torch.device(DEV)
    lshape = LlamaShape(**C.TINY_LLAMA)
    lm = LlavaLanguageModel(LlamaForCausalLM.from_reference_state_dict(lshape, C.tiny_llama_state_dict(dt), dt, dev),
                            image_token_id=C.TINY_IMAGE_TOKEN_ID)
    vision = _mid_clip(dt, image_size=48, patch_size=2)                    # 576 patch tokens + CLS, projector out = lm hidden
    if prune is not None:
        vision = _HostPrunedVision(vision, prune)
    ctx = TokenCacheBlockManagerContext(rank=0, rank2host={0: "localhost"})
    kv = TokenCacheBlockManager(TokenCacheBlockManagerConfig(
        n_layers=lshape.num_hidden_layers, n_tokens=2, n_blocks=160, block_size=16, n_heads=lshape.num_key_value_heads,
        head_size=lshape.head_dim, dtype=dname, device=DEV), ctx)
    img = TokenCacheBlockManager(TokenCacheBlockManagerConfig(
        n_layers=1, n_tokens=1, n_blocks=6, block_size=576, n_heads=lshape.num_attention_heads, head_size=lshape.head_dim,
        dtype=dname, device=DEV), ctx)
    sched = BatchSchedulerConfig(priority="prefill", max_running_requests=6, chunked_prefill=True, token_budgets=256,
                                 image_budgets=2)
    node = make_node("EPD0", "EPD", lm, vision, kv, img, lshape, dt, dev, sched, graph_decode=graphs)
    return LocalCluster([node]), kv


def _drive(cluster, rcbs, watch=None):
    """Feed the requests, step until idle; returns the largest KV block table `watch` held."""
    most = 0
    for r in rcbs:
        cluster.add_request(r)
    for _ in range(2000):
        if cluster.idle():
            break
        cluster.step()
        if watch is not None and watch.virtual_kv_cache is not None:
            most = max(most, len(watch.virtual_kv_cache.block_table))
    assert cluster.idle(), "engine did not drain"
    torch.cuda.synchronize()
    return most


@pytest.mark.parametrize("dname,graphs", [("fp16", False), ("bf16", True)], ids=["fp16-eager", "bf16-graphs"])
def test_engine_focal_request(dname, graphs):
    from hydrainfer_amd.engine import InstructionCreator, SamplingParameters, TokenParameters, TokenRequest
    from tests.golden import cases as C
    IMG = C.TINY_IMAGE_TOKEN_ID
    g = torch.Generator().manual_seed(77)
    px = torch.randn((2, 3, 48, 48), generator=g)
    text = [torch.randint(0, IMG, (n,), generator=g).tolist() for n in (10, 7, 12)]
    focal = TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=64)
    GEN = 4

    def request(rid, ids, image=None, tp=None):
        return TokenRequest(request_id=rid, token_ids=ids, pixel_values=px[image:image + 1].clone() if image is not None else None,
                            image_size=(48, 48), image_hash=7000 + (image or 0), sampling_params=SamplingParameters(max_tokens=GEN),
                            token_params=tp)

    def creator(n=576):
        return InstructionCreator(image_token_id=IMG, n_image_tokens_per_image=n, block_size=16, ignore_eos=True)

    # the engine under test: a focal request, an unpruned image request and a text request in one batch
    cluster, kv = _engine(dname, graphs=graphs)
    hits = []
    allocate = kv.allocate_virtual_cache
    kv.allocate_virtual_cache = lambda hashes=None: (lambda vc: (hits.append(vc.n_cache_tokens), vc)[1])(allocate(hashes))
    rcbs = [creator().process(r) for r in (request(0, [IMG] + text[0], 0, focal), request(1, [IMG] + text[1], 1),
                                           request(2, text[2]))]
    assert rcbs[0].request_metadata.n_prompt_tokens == 64 + 10 and rcbs[1].request_metadata.n_prompt_tokens == 576 + 7
    blocks = _drive(cluster, rcbs, watch=rcbs[0])
    assert all(len(r.output_token_ids) == GEN for r in rcbs)
    assert blocks == math.ceil((64 + 10 + GEN) / 16) == 5
    assert hits == [0, 0, 0]

    # the oracle: the same engine, image 0's features pruned ON THE HOST with the restatement, fed through the unpruned path
    o_cluster, _ = _engine(dname, prune=[(px[0], 64)], graphs=False)
    o_rcbs = [creator(64).process(request(0, [IMG] + text[0], 0)), creator().process(request(1, [IMG] + text[1], 1)),
              creator().process(request(2, text[2]))]
    _drive(o_cluster, o_rcbs)
    for got, want in zip(rcbs, o_rcbs):
        assert got.output_token_ids == want.output_token_ids, f"request {got.request_id}"

    # afterwards, on the SAME engine: the same focal request again hits its own prefix blocks (64 + 10 tokens: four whole
    # blocks) and repeats its tokens ...
    del hits[:]
    again_focal = creator().process(request(4, [IMG] + text[0], 0, focal))
    _drive(cluster, [again_focal])
    assert hits == [64] and again_focal.output_token_ids == rcbs[0].output_token_ids
    # ... while the same image and text UNPRUNED must not hit blocks computed from pruned image tokens, and gives the tokens
    # of a cold run
    del hits[:]
    again_full = creator().process(request(3, [IMG] + text[0], 0))
    _drive(cluster, [again_full])
    assert hits == [0], "the unpruned prompt hit blocks computed from pruned image tokens"
    cold_cluster, _ = _engine(dname, graphs=graphs)
    cold = creator().process(request(3, [IMG] + text[0], 0))
    _drive(cold_cluster, [cold])
    assert again_full.output_token_ids == cold.output_token_ids
