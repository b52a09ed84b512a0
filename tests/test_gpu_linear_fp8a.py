"""GPU: hx_quant_fp8_group and hx_linear_fp8a (csrc/gemm_fp8a.hip) on the inputs of tests/linear_fp8a_ref.py.
Quantiser bit for bit; exact rows and one-hot k probes for both tile heights (operands inside NaN buffers, outputs between
sentinel gaps); random inputs; non-finite x; the model's routing under the switch; LAST: the shims' refusals."""
import pytest
import torch

from tests import gemm_exact as G
from tests import linear_fp8_ref as L8
from tests import linear_fp8a_ref as A8
from tests import moe_fp8_ref as F8
from tests import test_gpu_linear_fp8 as W8

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = {"F16": torch.float16, "BF16": torch.bfloat16}
GAP_BYTE = 0x55


def _acts(xq, xs):
    """The device operands: xq as the middle of a buffer of NaN bytes with row gaps, xs k-major between NaN floats."""
    M, K = xq.shape
    big = torch.full((M + 6, K + 32), F8.NAN_BYTE, dtype=torch.uint8)
    big[3:3 + M, :K] = xq
    flat = torch.full((K // A8.BLK, M + 10), float("nan"))
    flat[:, 5:5 + M] = xs.t()
    return big.to(DEV)[3:3 + M, :K], flat.to(DEV)[:, 5:5 + M].t()


def _gemm(xq, xs, wq, ws, dt, tile=0):
    from hydrainfer_amd._C.kernel import gemm
    out = G.strided(torch.zeros((xq.shape[0], wq.shape[0]), dtype=dt, device=DEV), 4, G.SENTINEL)
    W8._set(b"fp8a_tile_rows", tile)
    try:
        got = gemm.linear_fp8a(xq, xs, wq, ws, dt, out=out)
    finally:
        W8._set(b"fp8a_tile_rows", 0)
    assert got.data_ptr() == out.data_ptr() and G.gaps_hold(out, 4, G.SENTINEL), "the gap columns of the output were written"
    return got.cpu()


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("M,K", [(m, k) for m in (1, 127, 130) for k in (128, 384)])
def test_quantiser_is_bit_identical(dname, M, K):
    from hydrainfer_amd._C.kernel import gemm
    dt = DTYPES[dname]
    x = (torch.randn((M, K), generator=torch.Generator().manual_seed(M + K)) * 3).to(dt)
    x[0, :128] = 0                                            # an all-zero group
    x[M // 2, K - 128:] = x[M // 2, K - 128:].clamp(-1, 1)
    x[M // 2, K - 3] = -7                                     # a group whose maximum is negative
    want_q, want_s = A8.quant_group(x)
    xq = torch.full((M, K + 16), GAP_BYTE, dtype=torch.uint8, device=DEV)
    xs = torch.full((K // 128, M + 3), G.SENTINEL, device=DEV)
    gq, gs = gemm.quant_fp8_group(G.strided(x.to(DEV), 8), out=(xq[:, :K], xs[:, :M].t()))
    assert torch.equal(gq.cpu(), want_q) and torch.equal(gs.cpu(), want_s)
    assert bool((xq[:, K:] == GAP_BYTE).all()) and bool((xs[:, M:] == G.SENTINEL).all())
    dq, ds = gemm.quant_fp8_group(x.to(DEV))                  # the shim's own buffers: shape [M, K / 128], k-major
    assert ds.shape == (M, K // 128) and torch.equal(dq.view(torch.uint8).cpu(), want_q) and torch.equal(ds.cpu(), want_s)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("N,K", [(128, 128), (384, 384), (256, 2816)])
def test_exact_rows(dname, N, K):
    dt = DTYPES[dname]
    c = L8.exact_case(N, K)
    wq, ws = W8._weight(c.q, c.scale)
    for M in (1, 64, 65, 128, 129, 200):
        xq, xs, ref = A8.exact_rows(c, M)
        dq, ds = _acts(xq, xs)
        for tile in (64, 128):
            got, want = _gemm(dq, ds, wq, ws, dt, tile), ref.to(dt)
            assert torch.equal(got, want), f"{dname} M={M} [{N}, {K}] tile {tile}: {W8._describe(got.double(), want.double())}"


@pytest.mark.parametrize("dname", list(DTYPES))
def test_one_hot_k_probe(dname):
    dt, N, K = DTYPES[dname], 128, 256
    wq = A8.probe_weight(N, K)
    xq = torch.zeros((K, K), dtype=torch.uint8)
    xq[torch.arange(K), torch.arange(K)] = F8.to_bytes(torch.tensor([A8.PROBE_X]))
    want = (A8.PROBE_X * wq.view(F8.FP8).double().t()).to(dt)
    for tile in (64, 128):
        got = _gemm(xq.to(DEV), torch.ones((K, 2), device=DEV), wq.to(DEV), torch.ones((1, 2), device=DEV), dt, tile)
        assert torch.equal(got, want), f"tile {tile}: {W8._describe(got.double(), want.double())}"


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("N,K", [(256, 2816), (128, 11008)])
def test_random_inputs_within_the_16_bit_gemm_tolerance(dname, N, K):
    """Against the float64 product of the dequantised operands, within linear_fp8_ref.tolerance.  Measured on the MI355X, worst
    error in units of the tolerance: BF16 (FP8 MFMA) 0.51 .. 0.56, F16 (16-bit MFMA over widened bytes) 0.49 .. 0.50; F16 on
    the FP8 MFMA was 1.40 .. 2.25 (profiles/linear_fp8a.md, Finding), which is why F16 does not run on it."""
    from hydrainfer_amd._C.kernel.moe.experts import quantize_fp8_block
    dt = DTYPES[dname]
    g = torch.Generator().manual_seed(N + K)
    xq, xs = A8.quant_group(torch.randn((200, K), generator=g).to(dt))
    q, s = quantize_fp8_block(torch.randn((N, K), generator=g) * 0.02)
    ref = A8.dequant_rows(xq, xs) @ F8.dequant(q.view(torch.uint8), s).double().t()
    worst = {}
    for M in (65, 200):
        got = _gemm(xq[:M].to(DEV), xs[:M].to(DEV), q.to(DEV), s.to(DEV), dt).double()
        worst[M] = float(((got - ref[:M]).abs() / L8.tolerance(ref[:M], dt)).max())
        print(f"{dname} [{N}, {K}] M={M}: worst error {worst[M]:.2f} of the tolerance")
    assert max(worst.values()) <= 1.0, f"worst error in units of the tolerance, by M: {worst}"


def test_a_non_finite_activation_poisons_exactly_its_row():
    from hydrainfer_amd._C.kernel import gemm
    from hydrainfer_amd._C.kernel.moe.experts import quantize_fp8_block
    g = torch.Generator().manual_seed(9)
    x = torch.randn((130, 384), generator=g).to(torch.bfloat16).to(DEV)
    q, s = (t.to(DEV) for t in quantize_fp8_block(torch.randn((256, 384), generator=g) * 0.02))
    clean = gemm.linear_fp8a(*gemm.quant_fp8_group(x), q, s, torch.bfloat16).cpu()
    x[77, 200], x[3, 383] = float("nan"), float("inf")
    got = gemm.linear_fp8a(*gemm.quant_fp8_group(x), q, s, torch.bfloat16).cpu()
    bad = torch.zeros(130, dtype=torch.bool)
    bad[77] = bad[3] = True
    assert bool(torch.isnan(got[bad]).all()) and torch.equal(got[~bad], clean[~bad]) and not bool(torch.isnan(clean).any())


def test_model_routes_prefill_through_the_switch():
    from hydrainfer_amd._C.kernel import gemm
    from hydrainfer_amd.layer.causal_attention import AttentionParametersBuilder
    from hydrainfer_amd.memory.kv_cache import KVCache
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    from hydrainfer_amd.model.llama import LanguageModelParameters, LlamaForCausalLM, LlamaShape
    from tests import test_gpu_moe_model as MM
    from tests.golden import cases as C
    dt, shape = torch.bfloat16, MM.moe_shape()
    model = DeepseekMoeForCausalLM.random_init(shape, dt, DEV, dense_dtype="fp8", dense_activations="fp8")
    w, sc = model.state["l0.wqkv"], model.state["l0.wqkv_scale"]
    x = torch.randn((130, w.shape[1]), device=DEV).to(dt)
    assert model.fp8_activations and torch.equal(model.linear(x, w, sc), gemm.linear_fp8a(*gemm.quant_fp8_group(x), w, sc, dt))
    assert torch.equal(model.linear(x[:64], w, sc), gemm.linear_decode_fp8(x[:64], w, sc))
    model.enable_fp8_activations(False)
    assert torch.equal(model.linear(x, w, sc), torch.matmul(x, gemm.dequant_fp8_block(w, sc, dt).t()))
    with pytest.raises(ValueError):
        LlamaForCausalLM.random_init(LlamaShape(**C.TINY_LLAMA), dt, DEV).enable_fp8_activations()
    # a 130-token prefill and two decode steps under the switch
    model.enable_fp8_activations()
    pool = torch.zeros((shape.num_hidden_layers, 2, C.TINY_BLOCKS, MM.BS, shape.num_key_value_heads, shape.head_dim), dtype=dt, device=DEV)
    table, ids, done = list(range(C.TINY_BLOCKS)), torch.randint(0, 256, (130,), generator=torch.Generator().manual_seed(1)).tolist(), 0
    for step in range(3):
        b = AttentionParametersBuilder(shape.num_attention_heads, shape.num_key_value_heads, shape.head_dim, MM.BS, torch.device(DEV))
        b.add_request(len(ids), done + len(ids), [table[p // MM.BS] * MM.BS + p % MM.BS for p in range(done, done + len(ids))],
                      table[: (done + len(ids) + MM.BS - 1) // MM.BS])
        for l in range(shape.num_hidden_layers):
            b.add_kv_cache(KVCache(pool[l, 0], pool[l, 1]))
        params = LanguageModelParameters(attention_params=b.build_attention_parameters(), all_sequences_decode=step > 0,
                                         selected_token_ids=torch.tensor([len(ids) - 1], device=DEV) if step == 0 else None)
        logits = model.forward_logits(torch.tensor(ids, dtype=torch.int64, device=DEV),
                                      torch.arange(done, done + len(ids), dtype=torch.int32, device=DEV), params)
        assert logits.shape[0] == 1 and bool(torch.isfinite(logits.float()).all()), f"step {step}"
        done, ids = done + len(ids), [int(logits[0].argmax())]


def test_shims_refuse_what_does_not_fit():
    from hydrainfer_amd import _lib
    from hydrainfer_amd._C.kernel import gemm
    x = torch.zeros((70, 256), dtype=torch.bfloat16, device=DEV)
    q = torch.zeros((128, 256), dtype=torch.uint8, device=DEV)
    s = torch.ones((1, 2), device=DEV)
    xq, xs = gemm.quant_fp8_group(x)
    assert gemm.fp8a_supported(x, q, s) and gemm.fp8a_supported(xq, q, s) and not gemm.fp8a_supported(x.t().contiguous().t()[:, :256], q, s)
    assert torch.equal(gemm.linear_fp8a(xq, xs, q, s, torch.bfloat16).cpu(), torch.zeros((70, 128), dtype=torch.bfloat16))
    for bad in (lambda: gemm.quant_fp8_group(x.float()), lambda: gemm.quant_fp8_group(x.cpu()), lambda: gemm.quant_fp8_group(x[:, :192]),
                lambda: gemm.quant_fp8_group(x, out=(xq, xs[:, :1])), lambda: gemm.quant_fp8_group(x, out=(xq.view(torch.uint8)[:, :128], xs)),
                lambda: gemm.linear_fp8a(x, xs, q, s, torch.bfloat16),                              # 16-bit activations
                lambda: gemm.linear_fp8a(xq, xs.double(), q, s, torch.bfloat16), lambda: gemm.linear_fp8a(xq, xs[:, :1], q, s, torch.bfloat16),
                lambda: gemm.linear_fp8a(xq, xs, q.to(torch.bfloat16), s, torch.bfloat16), lambda: gemm.linear_fp8a(xq, xs, q, s.cpu(), torch.bfloat16),
                lambda: gemm.linear_fp8a(xq, xs, q, torch.ones((2, 1), device=DEV), torch.bfloat16),  # scale shape
                lambda: gemm.linear_fp8a(xq, xs, q, s, torch.float32),
                lambda: gemm.linear_fp8a(xq[:, :128], xs[:, :1], q, s, torch.bfloat16),              # K of x and of the weight
                lambda: gemm.linear_fp8a(xq, xs, q, s, torch.bfloat16, out=torch.zeros((70, 128), dtype=torch.float16, device=DEV)),
                lambda: gemm.linear_fp8a(xq, xs, q, s, torch.bfloat16, out=torch.zeros((70, 130), dtype=torch.bfloat16, device=DEV)[:, :128])):
        with pytest.raises(_lib.HydraHipError):
            bad()
