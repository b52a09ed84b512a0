"""CPU: FP8 block-scaled dense linears without a GPU — the properties of the inputs tests/test_gpu_linear_fp8.py feeds
csrc/gemm_skinny_fp8.hip (restated in tests/linear_fp8_ref.py), the published state-dict names through layer and model
(round trip bit for bit, the missing-scale KeyError, the plain-Llama refusal), the byte models, the C entries' refusals and
the shims' (nothing is launched: no device is needed for a refusal)."""
import ctypes

import pytest
import torch

from tests import gemm_exact as G
from tests import linear_fp8_ref as L8
from tests import moe_fp8_ref as F8
from tests.golden import cases as C

FP8 = F8.FP8


# ---------------------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(128, 256), (384, 2816), (128, 11008)])
def test_exact_case_is_exact_and_a_neighbour_scale_shows(N, K):
    c = L8.exact_case(N, K)
    assert c.block_bound < 2 ** 24 and c.sum_bound < 2 ** 24
    # the reference is the product over the dequantised weights, which are grid values again
    w = F8.dequant(c.q, c.scale)
    assert torch.equal((w / G.STEP).round() * G.STEP, w) and float(w.abs().max()) <= G.LEVELS * G.STEP
    assert torch.equal(c.ref, c.x.double() @ w.double().t())
    # every block differs from its neighbour in both directions
    assert bool((c.scale[:, 1:] != c.scale[:, :-1]).all()) and (N == 128 or bool((c.scale[1:] != c.scale[:-1]).all()))
    # exact in fp16 and bf16 alike as far as the inputs go; the answer of a neighbour-scale mutant differs
    for T in (torch.float16, torch.bfloat16):
        assert torch.equal(c.x.to(T).float(), c.x)
    mutant = L8.neighbour_mutant(c)
    for M in (1, 16, 64):
        assert not torch.equal(mutant[:M], c.ref[:M])
    # the fp32 restatement of the contract gives the float64 answer, bit for bit, where that is representable
    for T in (torch.float16, torch.bfloat16):
        assert torch.equal(L8.contract_fp32(c.x[:17], c.q, c.scale, T), c.ref[:17].to(T))


def test_fine_case_separates_the_rounded_weight_mutant():
    c = L8.fine_case()
    K = c.q.shape[1]
    assert set((0, 127, 128, 255, 256, 1023, 1024, 2048, K - 1)) <= set(c.ks) and K == 2816 and K % L8.SPLIT_K == 768
    assert torch.equal(c.x.sum(dim=1), torch.full((len(c.ks),), L8.FINE_VALUE)) and int((c.x != 0).sum()) == len(c.ks)
    # 3 q s in fp32 is exact: at most 19 significant bits
    w = c.q.view(FP8).float() * F8.expand(c.scale)
    assert torch.equal((L8.FINE_VALUE * w).double(), L8.FINE_VALUE * c.q.view(FP8).float().double() * F8.expand(c.scale).double())
    for T in (torch.float16, torch.bfloat16):
        true, mutant = L8.fine_out(c, T), L8.fine_out(c, T, round_weight=True)
        assert not torch.isnan(true.float()).any() and true.shape == mutant.shape == (len(c.ks), c.q.shape[0])
        assert int((true != mutant).sum()) > 0, T
        assert torch.equal(L8.contract_fp32(c.x, c.q, c.scale, T), true)


@pytest.mark.parametrize("T", [torch.float16, torch.bfloat16])
def test_random_inputs_contract_is_inside_the_tolerance(T):
    from hydrainfer_amd._C.kernel.moe.experts import quantize_fp8_block
    N, K, M = 256, 2816, 32
    g = torch.Generator().manual_seed(N + K + M)
    x = torch.randn((M, K), generator=g).to(T)
    q, s = quantize_fp8_block(torch.randn((N, K), generator=g) * 0.02)
    ref = x.double() @ F8.dequant(q.view(torch.uint8), s).double().t()
    tol = L8.tolerance(ref, T)
    err = (L8.contract_fp32(x, q.view(torch.uint8), s, T).double() - ref).abs()
    print(f"{T}: contract in fp32 at {float((err / tol).max()):.2f} of the tolerance; rounded-weight product at "
          f"{float(((L8.rounded_weight_product(x, q.view(torch.uint8), s, T) - ref).abs() / tol).max()):.2f}")
    assert bool((err <= tol).all())


# ---------------------------------------------------------------------------------------------------------------------
# layer and model: published names, bytes
# ---------------------------------------------------------------------------------------------------------------------
def _shape():
    from hydrainfer_amd.model.deepseek_moe import MoeShape
    return MoeShape(**dict(C.TINY_LLAMA), n_routed_experts=8, num_experts_per_tok=3, moe_intermediate_size=128,
                    n_shared_experts=2, first_k_dense_replace=1, norm_topk_prob=True, routed_scaling_factor=1.0)


def _published_sd(dt=torch.bfloat16):
    from hydrainfer_amd._C.kernel.moe.experts import quantize_fp8_block
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    m = DeepseekMoeForCausalLM.random_init(_shape(), dt, "cpu", seed=20, std=0.02, router_std=0.2, expert_std=0.1)
    return L8.published_full(m.to_reference_state_dict(), quantize_fp8_block)


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_published_state_dict_round_trips_bit_for_bit():
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    sd = _published_sd()
    fp8_names = [k for k, v in sd.items() if v.dtype == FP8]
    assert any("self_attn.q_proj" in k for k in fp8_names) and any("shared_experts.down_proj" in k for k in fp8_names)
    assert any("layers.0.mlp.gate_proj" in k for k in fp8_names) and any(".experts.3.up_proj" in k for k in fp8_names)
    assert all(k[:-len("weight")] + "weight_scale_inv" in sd for k in fp8_names)
    model = DeepseekMoeForCausalLM.from_reference_state_dict(_shape(), sd, torch.bfloat16, "cpu")
    st = model.state
    for key in ("l0.wqkv", "l0.wo", "l0.wgu", "l0.wdown", "l1.wqkv", "l1.wo", "l1.moe.sgu", "l1.moe.sdown"):
        assert st[key].dtype == FP8 and st[key + "_scale"].dtype == torch.float32, key
        assert tuple(st[key + "_scale"].shape) == (st[key].shape[0] // 128, st[key].shape[1] // 128), key
    # the raw e4m3 values were not cast: the bytes of q_proj are the first rows of wqkv
    assert _same(st["l0.wqkv"][:256], sd["model.layers.0.self_attn.q_proj.weight"])
    for k in ("embed", "lm_head", "norm", "l1.moe.router", "l0.norm1"):
        assert st[k].dtype == torch.bfloat16, k
    back = model.to_reference_state_dict()
    assert sorted(back) == sorted(sd)
    for k in sd:
        assert _same(back[k], sd[k]), k


def test_fp8_weight_without_its_scale_is_a_key_error_naming_it():
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    full = _published_sd()
    for name in ("model.layers.0.self_attn.k_proj.weight_scale_inv", "model.layers.1.self_attn.o_proj.weight_scale_inv",
                 "model.layers.0.mlp.up_proj.weight_scale_inv", "model.layers.0.mlp.down_proj.weight_scale_inv",
                 "model.layers.1.mlp.shared_experts.gate_proj.weight_scale_inv",
                 "model.layers.1.mlp.shared_experts.down_proj.weight_scale_inv"):
        sd = {k: v for k, v in full.items() if k != name}
        with pytest.raises(KeyError, match=name.replace(".", r"\.")):
            DeepseekMoeForCausalLM.from_reference_state_dict(_shape(), sd, torch.bfloat16, "cpu")


def test_projections_fused_here_must_agree_in_dtype():
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    full = _published_sd()
    for name in ("model.layers.0.self_attn.v_proj.weight", "model.layers.0.mlp.gate_proj.weight",
                 "model.layers.1.mlp.shared_experts.up_proj.weight"):
        sd = dict(full)
        sd[name] = F8.dequant(full[name].view(torch.uint8), full[name[:-len("weight")] + "weight_scale_inv"]).to(torch.bfloat16)
        del sd[name[:-len("weight")] + "weight_scale_inv"]
        with pytest.raises(ValueError):
            DeepseekMoeForCausalLM.from_reference_state_dict(_shape(), sd, torch.bfloat16, "cpu")


def test_plain_llama_refuses_fp8_scales_and_odd_head_sizes_are_refused():
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM, MoeShape
    from hydrainfer_amd.model.llama import LlamaForCausalLM, LlamaShape
    model = DeepseekMoeForCausalLM.from_reference_state_dict(_shape(), _published_sd(), torch.bfloat16, "cpu")
    dense = {k: v for k, v in model.state.items() if ".moe." not in k}
    with pytest.raises(ValueError, match="FP8"):
        LlamaForCausalLM(LlamaShape(**dict(C.TINY_LLAMA)), torch.bfloat16, "cpu", dense)
    # q_size / kv_size that are no multiples of 128: the concatenated scales would not line up
    t = dict(C.TINY_LLAMA, num_attention_heads=4, num_key_value_heads=4, head_dim=32, hidden_size=128)
    shape = MoeShape(**t, n_routed_experts=8, num_experts_per_tok=3, moe_intermediate_size=128, n_shared_experts=2,
                     first_k_dense_replace=1)
    m = DeepseekMoeForCausalLM.random_init(shape, torch.bfloat16, "cpu", seed=1)
    m.q_size = m.kv_size = 96
    with pytest.raises(ValueError, match="multiples of 128"):
        m.quantize_dense()


def test_weight_bytes_unquantised_unchanged_and_quantised_by_the_formula():
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    sh = _shape()
    m = DeepseekMoeForCausalLM.random_init(sh, torch.bfloat16, "cpu", seed=3)
    h, I, V, L = sh.hidden_size, sh.intermediate_size, sh.vocab_size, sh.num_hidden_layers
    E, Im, Is, topk = sh.n_routed_experts, sh.moe_intermediate_size, sh.moe_intermediate_size * sh.n_shared_experts, sh.num_experts_per_tok
    attn = L * (3 * h * h + h * h)                  # q_size == kv_size == h
    dense_mlp = 3 * h * I
    shared = 3 * h * Is
    for n in (1, 64):
        hit = min(E, n * topk)
        assert m.weight_bytes(n) == 2 * (V * h + attn + dense_mlp + shared + E * h + hit * 3 * h * Im)
    assert m.weight_bytes_resident() == sum(v.numel() * 2 for v in m.state.values())
    resident16 = m.weight_bytes_resident()
    assert m.quantize_dense() is m
    blocks = lambda elems: elems // (128 * 128)
    fp8_elems = attn + dense_mlp + shared
    for n in (1, 64):
        hit = min(E, n * topk)
        assert m.weight_bytes(n) == fp8_elems + 4 * blocks(fp8_elems) + 2 * (V * h + E * h + hit * 3 * h * Im)
    assert m.weight_bytes_resident() == resident16 - fp8_elems + 4 * blocks(fp8_elems)
    # idempotent: the second call changes no tensor
    before = {k: v for k, v in m.state.items()}
    m.quantize_dense()
    assert sorted(before) == sorted(m.state) and all(before[k] is m.state[k] for k in before)
    # the routed experts are quantize_experts()'s
    assert m.state["l1.moe.wgu"].dtype == torch.bfloat16 and m.moe[1].shared_fp8 and not m.moe[1].experts_fp8
    both = DeepseekMoeForCausalLM.random_init(sh, torch.bfloat16, "cpu", seed=3, expert_dtype="fp8", dense_dtype="fp8")
    assert both.moe[1].experts_fp8 and both.state["l0.wqkv"].dtype == FP8 and _same(both.state["l0.wqkv"], m.state["l0.wqkv"])
    with pytest.raises(ValueError):
        DeepseekMoeForCausalLM.random_init(sh, torch.bfloat16, "cpu", dense_dtype="fp4")


# ---------------------------------------------------------------------------------------------------------------------
# the C entries and the shims: refusals (no launch)
# ---------------------------------------------------------------------------------------------------------------------
def test_c_entries_refuse_what_does_not_fit():
    from hydrainfer_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 15) & ~15
    ws = l.hx_linear_decode_workspace_bytes(1, 128, 256)

    def call(out=a, x=a, wq=a, sc=a, M=1, N=128, K=256, ldx=256, ldw=256, ldo=128, work=a, wb=ws, dtype=_lib.HX_BF16):
        return l.hx_linear_decode_fp8w(out, x, wq, sc, M, N, K, ldx, ldw, ldo, work, wb, dtype, None)
    SHAPE, NULL, DTYPE, WORK, STRIDE = -1, -2, -3, -6, -4
    codes = {l.hx_strerror(c).decode(): c for c in range(-8, 0)}
    assert len(codes) == 8
    for kw in (dict(M=0), dict(M=65), dict(N=64), dict(N=192), dict(K=128), dict(K=384), dict(ldw=264), dict(ldw=128),
               dict(ldx=260), dict(ldo=130), dict(ldo=64)):
        assert call(**kw) == call(M=0), kw                       # HX_ERR_SHAPE
    for kw in (dict(out=None), dict(x=None), dict(wq=None), dict(sc=None), dict(work=None)):
        assert call(**kw) == call(out=None) != call(M=0), kw     # HX_ERR_NULL
    assert call(dtype=_lib.HX_F32) not in (0, call(M=0), call(out=None))
    assert call(wb=ws - 1) not in (0, call(M=0), call(out=None), call(dtype=_lib.HX_F32))
    assert call(wq=a + 8) == call(x=a + 2) == call(sc=a + 2) not in (0, call(M=0), call(out=None))
    deq = lambda **kw: l.hx_dequant_fp8_block(kw.get("out", a), kw.get("wq", a), kw.get("sc", a), kw.get("N", 128), kw.get("K", 128),
                                               kw.get("ldo", 128), kw.get("dtype", _lib.HX_F16), None)
    assert deq(N=64) == deq(K=64) == deq(ldo=132) == deq(ldo=120) == deq(N=0) == call(M=0)
    assert deq(out=None) == deq(sc=None) == call(out=None)
    assert deq(dtype=_lib.HX_F32) == call(dtype=_lib.HX_F32)
    # the options and the plan query
    out = (ctypes.c_int32 * 2)()
    assert l.hx_debug_linear_fp8_plan(1, 128, 256, out) == 0 and tuple(out) == (4, 1)
    try:
        assert l.hx_debug_set_option(b"gemm_fp8_waves", 8) == 0 and l.hx_debug_set_option(b"gemm_fp8_rows_per_wave", 2) == 0
        assert l.hx_debug_linear_fp8_plan(64, 128, 256, out) == 0 and tuple(out) == (8, 2)
        assert l.hx_debug_set_option(b"gemm_fp8_rows_per_wave", 3) == 0
        assert l.hx_debug_linear_fp8_plan(1, 128, 256, out) != 0          # not built
    finally:
        l.hx_debug_set_option(b"gemm_fp8_waves", 0); l.hx_debug_set_option(b"gemm_fp8_rows_per_wave", 0)
    assert l.hx_debug_linear_fp8_plan(1, 128, 256, out) == 0 and tuple(out) == (4, 1)


def test_shims_refuse_cpu_tensors_and_what_does_not_fit():
    from hydrainfer_amd import _lib
    from hydrainfer_amd._C.kernel import gemm
    x = torch.zeros((2, 256), dtype=torch.bfloat16)
    q, s = torch.zeros((128, 256), dtype=torch.uint8), torch.ones((1, 2))
    assert gemm.fp8_supported(x, q, s) and gemm.fp8_supported(x, q.view(FP8), s)
    assert not gemm.fp8_supported(torch.zeros((65, 256), dtype=torch.bfloat16), q, s)
    assert not gemm.fp8_supported(torch.zeros((2, 384), dtype=torch.float16), torch.zeros((128, 384), dtype=torch.uint8), torch.ones((1, 3)))
    for bad in (lambda: gemm.fp8_supported(x, q.to(torch.bfloat16), s), lambda: gemm.fp8_supported(x, q, s.double()),
                lambda: gemm.fp8_supported(x, q, torch.ones((2, 1))), lambda: gemm.fp8_supported(x, q, None),
                lambda: gemm.fp8_supported(x.float(), q, s), lambda: gemm.fp8_supported(x[:, :128], q, s),
                lambda: gemm.fp8_supported(x, torch.zeros((64, 256), dtype=torch.uint8), torch.ones((0, 2))),
                lambda: gemm.fp8_supported(x, torch.zeros((128, 192), dtype=torch.uint8), torch.ones((1, 1))),
                lambda: gemm.linear_decode_fp8(x, q, s), lambda: gemm.dequant_fp8_block(q, s, torch.bfloat16)):
        with pytest.raises(_lib.HydraHipError):
            bad()
