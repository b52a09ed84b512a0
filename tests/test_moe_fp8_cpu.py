"""CPU: FP8 block-scaled expert weights (csrc/moe_experts_fp8.hip, layer/moe.py, model/deepseek_moe.py) without a GPU —
the quantiser's derived error bound, the exactness of the inputs tests/test_gpu_moe_fp8.py feeds the kernels (restated in
tests/moe_fp8_ref.py), the published state-dict names through layer and model, the byte models, the C entries' refusals
and the compiled kernels' resources."""
import os
import sys

import pytest
import torch

from tests import gemm_exact as G
from tests import moe_block_ref as R
from tests import moe_fp8_ref as F8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = torch.float8_e4m3fn


def _experts():
    from hydrainfer_amd._C.kernel.moe import experts as K
    return K


# ---------------------------------------------------------------------------------------------------------------------
# the quantiser
# ---------------------------------------------------------------------------------------------------------------------
def test_quantiser_error_is_within_the_derived_bound():
    """|w - dq(q(w))| <= 2^-4 |w| + scale 2^-10: half an ulp of a 3-bit mantissa (relative 2^-4 at worst), plus half the
    subnormal step 2^-9, in units of the block's scale.  Derived from the format, not tuned."""
    K = _experts()
    w = torch.randn((3, 256, 384), generator=torch.Generator().manual_seed(1)) * 0.1
    q, s = K.quantize_fp8_block(w)
    assert q.dtype == FP8 and q.shape == w.shape and s.dtype == torch.float32 and s.shape == (3, 2, 3)
    amax = w.reshape(3, 2, 128, 3, 128).abs().amax(dim=(2, 4))
    assert torch.equal(s, amax / 448.0)
    back = K.dequantize_fp8_block(q, s)
    assert back.dtype == torch.float32
    bound = 2.0 ** -4 * w.abs() + F8.expand(s) * 2.0 ** -10
    assert bool(((w - back).abs() <= bound).all()), float(((w - back).abs() - bound).max())
    assert bool((w - back).abs().max() > 0)                       # (it is a lossy format: the bound is not met trivially)
    # 16-bit inputs quantise from their fp32 value
    q16, s16 = K.quantize_fp8_block(w.to(torch.bfloat16))
    qf, sf = K.quantize_fp8_block(w.to(torch.bfloat16).float())
    assert torch.equal(q16.view(torch.uint8), qf.view(torch.uint8)) and torch.equal(s16, sf)


def test_quantiser_with_given_scales_is_bit_exact_on_grid_values():
    K = _experts()
    g = torch.Generator().manual_seed(2)
    q0 = torch.randint(0, 256, (2, 128, 256), generator=g, dtype=torch.int32).to(torch.uint8)
    q0[(q0 & 0x7F) == 0x7F] = 0x3A                                # no NaN bytes
    s0 = F8._fine_scales((2, 1, 2), g)
    w = K.dequantize_fp8_block(q0.view(FP8), s0)
    assert torch.equal(w, F8.dequant(q0, s0))
    q, s = K.quantize_fp8_block(w, s0)
    assert torch.equal(s, s0)
    same = q.view(torch.uint8) == q0
    zero = ((q.view(torch.uint8) & 0x7F) == 0) & ((q0 & 0x7F) == 0)             # +0 and -0
    assert bool((same | zero).all())
    assert torch.equal(K.dequantize_fp8_block(q, s), w)
    assert torch.equal(K.dequantize_fp8_block(q.view(torch.uint8), s), w)       # uint8 holders are e4m3 bytes too


def test_all_zero_block_gets_scale_one_and_zero_bytes():
    K = _experts()
    w = torch.randn((128, 256), generator=torch.Generator().manual_seed(3))
    w[:, 128:] = 0
    q, s = K.quantize_fp8_block(w)
    assert float(s[0, 1]) == 1.0 and torch.equal(s[0, 0], w[:, :128].abs().max() / 448.0)
    assert bool((q.view(torch.uint8)[:, 128:] == 0).all())
    with pytest.raises(Exception):
        K.quantize_fp8_block(torch.zeros((128, 100)))


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the exact cases
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_weights_are_e4m3_numbers():
    vals = torch.tensor([j * G.STEP for j in range(-G.LEVELS, G.LEVELS + 1)] + [R.GATE_VALUE]
                        + [R.GATE_VALUE / s for s in F8.PAIRING_SCALES])
    assert torch.equal(vals.to(FP8).float(), vals)
    # ... and every finite e4m3 value is a bf16 and an fp16 number (the kernels widen bytes to T before the MFMA)
    every = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(FP8).float()
    finite = ~torch.isnan(every)
    assert int(finite.sum()) == 254
    for T in R.DTYPES.values():
        assert torch.equal(every[finite].to(T).float(), every[finite])


@pytest.mark.parametrize("case", R.PAIRING_CASES, ids=[c.name for c in R.PAIRING_CASES])
def test_pairing_cases_stay_exact_under_power_of_two_scales(case):
    f = F8.fp8_pairing(case)
    p, inter, routed = f.p, case.I, f.p.routed
    # the dequantised weights are the 16-bit case's, so its expected tensors and its exactness bounds (asserted by
    # build_pairing) are this case's too
    assert torch.equal(f.wgu[routed], p.wgu[routed]) and torch.equal(f.wdown[routed], p.wdown[routed])
    assert bool((f.wgu[routed][:, :inter] == R.GATE_VALUE).all()) and R.silu_of_gate_is_exact()
    assert bool((f.qgu[~routed] == F8.NAN_BYTE).all()) and bool((f.qdown[~routed] == F8.NAN_BYTE).all())
    assert bool(torch.isnan(f.sgu[~routed]).all()) and bool(torch.isnan(f.sdown[~routed]).all())
    assert bool(torch.isnan(f.wgu[~routed]).all()) and bool(torch.isnan(f.wdown[~routed]).all())
    for s in (f.sgu[routed], f.sdown[routed]):
        assert set(s.reshape(-1).tolist()) <= set(F8.PAIRING_SCALES)
    assert len(set(f.sgu[routed].reshape(-1).tolist())) >= 2                    # (the scales do vary)
    # ... and the bytes are not the weights: a kernel that ignored the scales would be seen
    assert not torch.equal(f.qgu[routed].view(FP8).float(), p.wgu[routed])
    for T in R.DTYPES.values():
        assert torch.equal(F8.pairing_act(f, T).double(), F8.pairing_act(f, torch.float64))      # act is exact in T
        out = F8.pairing_out(f, T)
        assert torch.equal(out, R.pairing_expected(p, T)) and bool(torch.isfinite(out.float()).all())
        assert bool(torch.isfinite(F8.pairing_y(f, T).float()).all())
    # new: the sum over one 128-k block before its scale runs over the bytes
    assert F8.pairing_block_bound() < 2 ** 24
    byte_vals = f.qdown[routed].view(FP8).float().abs()
    assert float(byte_vals.max()) <= G.LEVELS * G.STEP / min(F8.PAIRING_SCALES)
    quantum = G.STEP / max(F8.PAIRING_SCALES)
    assert torch.equal((byte_vals / quantum).round() * quantum, byte_vals)


def test_fine_scale_inputs_tell_the_mutant_apart():
    """3 q s has at most 19 significant bits (an fp32 number), and rounding q s to T before the product changes at least
    one expected element in both types — otherwise the GPU test could not tell the two apart."""
    c = F8.fine_case()
    assert sorted(k // 128 for k in F8.FINE_KS) == [0, 1, 2, 3, 4] and F8.FINE_H == 640 and F8.FINE_I == 256
    for q, s in ((c.qgu[:, F8.FINE_I:], c.sgu[:, F8.FINE_I // 128:]), (c.qdown, c.sdown)):
        prod = F8.FINE_VALUE * q.view(FP8).double() * F8.expand(s).double()
        assert torch.equal(prod.float().double(), prod)
    assert bool((c.sgu[:, :F8.FINE_I // 128] == 1).all()) and bool((c.qgu[:, :F8.FINE_I].view(FP8).float() == R.GATE_VALUE).all())
    v = torch.tensor([F8.FINE_VALUE * R.GATE_VALUE])
    assert bool(torch.nn.functional.silu(v) == v)
    assert all(len(set(row.tolist())) == F8.FINE_TOPK for row in c.ids)
    for T in R.DTYPES.values():
        for fn in (F8.fine_act, F8.fine_y):
            true, mutant = fn(c, T), fn(c, T, round_weight=True)
            assert not torch.isnan(true.float()).any() and true.shape == mutant.shape
            assert int((true != mutant).sum()) > 0, (fn.__name__, T)


# ---------------------------------------------------------------------------------------------------------------------
# published names through the layer and the model
# ---------------------------------------------------------------------------------------------------------------------
def test_layer_state_dict_round_trip_of_the_published_format():
    from hydrainfer_amd.layer.moe import SparseMoE
    K = _experts()
    sd = F8.published(R.block_weights("bf16"), K.quantize_fp8_block)
    assert sd["experts.3.up_proj.weight"].dtype == FP8 and sd["experts.3.up_proj.weight_scale_inv"].shape == (R.I // 128, R.H // 128)
    moe = SparseMoE.from_reference_state_dict("", sd, R.TOPK, dtype=torch.bfloat16)
    assert moe.experts_fp8 and moe.w_gate_up.dtype == FP8 and moe.w_down.dtype == FP8
    assert moe.w_gate_up.shape == (R.E, 2 * R.I, R.H) and moe.w_gate_up_scale.shape == (R.E, 2 * R.I // 128, R.H // 128)
    assert moe.w_down_scale.shape == (R.E, R.H // 128, R.I // 128) and moe.w_gate_up_scale.dtype == torch.float32
    assert moe.router_weight.dtype == torch.bfloat16 and moe.shared_gate_up.dtype == torch.bfloat16
    for e in (0, R.E - 1):          # gate rows before up rows, for the scales too
        assert torch.equal(moe.w_gate_up[e, R.I:].view(torch.uint8), sd[f"experts.{e}.up_proj.weight"].view(torch.uint8))
        assert torch.equal(moe.w_gate_up_scale[e, R.I // 128:], sd[f"experts.{e}.up_proj.weight_scale_inv"])
        assert torch.equal(moe.w_gate_up_scale[e, :R.I // 128], sd[f"experts.{e}.gate_proj.weight_scale_inv"])
    back = moe.to_reference_state_dict("")
    assert sorted(back) == sorted(sd)
    for k, v in sd.items():
        assert back[k].dtype == v.dtype and back[k].shape == v.shape, k
        assert torch.equal(back[k].view(torch.uint8) if v.dtype == FP8 else back[k], v.view(torch.uint8) if v.dtype == FP8 else v), k
    # quantize_experts() of the 16-bit layer gives the same bytes and scales, and is idempotent
    plain = SparseMoE.from_reference_state_dict("", R.block_weights("bf16"), R.TOPK)
    assert not plain.experts_fp8 and plain.w_gate_up_scale is None
    router, shared = plain.router_weight, plain.shared_gate_up
    plain.quantize_experts()
    assert torch.equal(plain.w_gate_up.view(torch.uint8), moe.w_gate_up.view(torch.uint8))
    assert torch.equal(plain.w_down_scale, moe.w_down_scale) and plain.router_weight is router and plain.shared_gate_up is shared
    held = plain.w_gate_up
    assert plain.quantize_experts() is plain and plain.w_gate_up is held


def test_layer_refuses_mixed_formats():
    from hydrainfer_amd.layer.moe import SparseMoE
    K = _experts()
    sd = dict(F8.published(R.block_weights("fp16"), K.quantize_fp8_block))
    sd["experts.2.down_proj.weight"] = R.block_weights("fp16")["experts.2.down_proj.weight"]
    with pytest.raises(ValueError, match="one layer"):
        SparseMoE.from_reference_state_dict("", sd, R.TOPK)
    with pytest.raises(ValueError):                      # one scale without the other
        SparseMoE(torch.zeros(2, 128), torch.zeros((2, 256, 128), dtype=FP8), torch.zeros((2, 128, 128), dtype=FP8), None, None, 1,
                  w_gate_up_scale=torch.ones(2, 2, 1))


def _tiny(dt=torch.bfloat16, **kw):
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    from tests.test_gpu_moe_model import moe_shape
    return DeepseekMoeForCausalLM.random_init(moe_shape(), dt, "cpu", seed=20, std=0.02, router_std=0.2, expert_std=0.1, **kw)


def test_model_state_dict_round_trip_of_the_published_format():
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    from tests.test_gpu_moe_model import moe_shape
    a = _tiny().quantize_experts()
    assert a.state["l1.moe.wgu"].dtype == FP8 and a.state["l1.moe.wdown"].dtype == FP8
    assert a.state["l1.moe.wgu_scale"].shape == (8, 2, 2) and a.state["l1.moe.wdown_scale"].shape == (8, 2, 1)
    assert a.state["l1.moe.wgu"] is a.moe[1].w_gate_up and a.state["l1.moe.wgu_scale"] is a.moe[1].w_gate_up_scale
    assert a.state["l1.moe.sgu"].dtype == torch.bfloat16 and a.state["l1.moe.router"].dtype == torch.bfloat16
    sd = a.to_reference_state_dict()
    p = "model.layers.1.mlp.experts.5."
    assert sd[p + "gate_proj.weight"].dtype == FP8 and sd[p + "down_proj.weight_scale_inv"].dtype == torch.float32
    assert sd[p + "down_proj.weight_scale_inv"].shape == (2, 1)
    # fp16 is the dtype asked for: neither bytes nor scales may be cast to it
    b = DeepseekMoeForCausalLM.from_reference_state_dict(moe_shape(), sd, torch.float16, "cpu")
    assert b.state["l1.moe.wgu"].dtype == FP8 and b.state["l1.moe.wgu_scale"].dtype == torch.float32
    assert b.state["l1.wqkv"].dtype == torch.float16
    assert torch.equal(b.state["l1.moe.wgu"].view(torch.uint8), a.state["l1.moe.wgu"].view(torch.uint8))
    assert torch.equal(b.state["l1.moe.wdown_scale"], a.state["l1.moe.wdown_scale"])
    sd2 = DeepseekMoeForCausalLM.from_reference_state_dict(moe_shape(), sd, torch.bfloat16, "cpu").to_reference_state_dict()
    assert sorted(sd2) == sorted(sd)
    for k, v in sd.items():
        assert sd2[k].dtype == v.dtype, k
        assert torch.equal(sd2[k].view(torch.uint8) if v.dtype == FP8 else sd2[k], v.view(torch.uint8) if v.dtype == FP8 else v), k
    # random_init(expert_dtype="fp8") is the same draw, quantised
    c = _tiny(expert_dtype="fp8")
    assert sorted(c.state) == sorted(a.state)
    assert all(torch.equal(c.state[k].view(torch.uint8) if v.dtype == FP8 else c.state[k], v.view(torch.uint8) if v.dtype == FP8 else v)
               for k, v in a.state.items())


def test_byte_models_before_and_after_quantisation():
    """The tiny model by hand: h 256, dense MLP 512, 2 layers (one dense, one sparse), q = k = v = 256 wide, vocab 512;
    E 8, topk 3, I 128, 2 shared experts."""
    two_d = 512 * 256 + 2 * (768 * 256 + 256 * 256) + (1024 * 256 + 256 * 512) + 8 * 256 + (512 * 256 + 256 * 256)
    assert two_d == 1247232
    per_expert = 3 * 256 * 128
    blocks = per_expert // (128 * 128)
    assert (per_expert, blocks) == (98304, 6)
    rest = 512 * 256 + 256 + 2 * 2 * 256          # embeddings and norms
    m = _tiny()
    assert m.weight_bytes(1) == 2 * two_d + 3 * per_expert * 2 == 3084288
    assert m.weight_bytes(64) == 2 * two_d + 8 * per_expert * 2 == 4067328
    assert m.weight_bytes_resident() == 2 * (two_d + rest + 8 * per_expert) == 4332032
    m.quantize_experts()
    assert m.weight_bytes(1) == 2 * two_d + 3 * (per_expert + 4 * blocks) == 2789448
    assert m.weight_bytes(2) == 2 * two_d + 6 * (per_expert + 4 * blocks)
    assert m.weight_bytes(64) == 2 * two_d + 8 * (per_expert + 4 * blocks) == 3281088
    assert m.weight_bytes_resident() == 2 * (two_d + rest) + 8 * (per_expert + 4 * blocks) == 3545792
    held = m.state["l1.moe.wgu"]
    assert m.quantize_experts() is m and m.state["l1.moe.wgu"] is held


# ---------------------------------------------------------------------------------------------------------------------
# the C entries' refusals (before any launch: readable without a GPU) and the kernels' resources
# ---------------------------------------------------------------------------------------------------------------------
_PTR = 0x10000          # non-NULL, 16-byte aligned, never dereferenced: every case below is refused on the host
_OK = dict(out=_PTR, x=_PTR, wq=_PTR, scale=_PTR, seg=_PTR, n=4, topk=2, E=8, h=256, I=128, dtype=2, stream=None)


@pytest.mark.parametrize("entry", ["hx_moe_gate_up_silu_fp8w", "hx_moe_down_fp8w"])
def test_fp8_entries_refuse_bad_arguments_before_any_launch(entry):
    from hydrainfer_amd import _lib
    fn = getattr(_lib.lib(), entry)

    def call(**changes):
        return fn(*{**_OK, **changes}.values())
    assert call(scale=None) == -4
    for name in ("out", "x", "wq", "seg"):
        assert call(**{name: None}) == -4, name
    assert call(h=192) == -2 and call(I=64) == -2 and call(h=0) == -2
    assert call(E=257) == -2 and call(topk=9) == -2 and call(n=0) == -2
    assert call(dtype=0) == -1                                   # fp32
    assert call(dtype=0, h=192) == -2 and call(dtype=0, scale=None) == -4


def test_fp8_kernels_use_no_scratch_and_spill_nothing():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    rows = [r for r in kernel_table.kernels() if r["name"].startswith("moe_gemm_fp8w_kernel<")]
    assert sorted(r["name"] for r in rows) == sorted(f"moe_gemm_fp8w_kernel<{t}, {mb}, {gu}>" for t in ("BF16", "F16")
                                                     for mb in (1, 2, 4) for gu in (0, 1))
    for r in rows:
        assert r.get("private_segment_fixed_size", 0) == 0 and r.get("vgpr_spill_count", 0) == 0, r
        assert r.get("sgpr_spill_count", 0) == 0 and r.get("wavefront_size") == 64, r
    # the 16-bit kernels are all still there beside them
    assert len([r for r in kernel_table.kernels() if r["name"].startswith("moe_gemm_kernel<")]) == 12
