"""CPU: MXFP4 expert weights (csrc/moe_experts_mxfp4.hip, layer/moe.py, model/deepseek_moe.py) without a GPU — the
format's two conversions, the state-dict round trips, the byte model and the built kernels' resources."""
import os
import sys

import pytest
import torch

from tests import moe_block_ref as R
from tests import moe_mxfp4_ref as MX

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_table  # noqa: E402

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _K():
    from hydrainfer_amd._C.kernel.moe import experts
    return experts


@pytest.mark.parametrize("byte", [0, 1, 127, 254, 255])
def test_every_code_dequantises_exactly(byte):
    K = _K()
    codes = torch.arange(16).repeat(2)                           # one 32-k group: every code at an even and an odd k
    got = K.dequantize_mxfp4(MX.pack(codes)[None], torch.tensor([[byte]], dtype=torch.uint8), torch.float64)[0]
    if byte == 255:
        assert bool(torch.isnan(got).all())
        return
    want = torch.tensor([(-1.0 if c & 8 else 1.0) * E2M1[c & 7] * 2.0 ** (byte - 127) for c in codes.tolist()], dtype=torch.float64)
    assert torch.equal(got, want) and torch.equal(torch.signbit(got), torch.signbit(want))
    if byte < 254:                                               # fp32 holds them too (6 * 2^127 is not an fp32 number)
        assert torch.equal(K.dequantize_mxfp4(MX.pack(codes)[None], torch.tensor([[byte]], dtype=torch.uint8))[0].double(), want)


def test_quantise_inverts_dequantise_and_rounds_to_nearest_even():
    K = _K()
    g = torch.Generator().manual_seed(5)
    codes = torch.randint(0, 16, (3, 64, 256), generator=g)
    codes[..., ::32] = 6 + torch.randint(0, 2, (3, 64, 8), generator=g)      # every group holds a 4 or a 6
    q, s = MX.pack(codes), torch.randint(1, 255, (3, 64, 8), generator=g).to(torch.uint8)
    q2, s2 = K.quantize_mxfp4(K.dequantize_mxfp4(q, s, torch.float64))
    assert torch.equal(q2, q) and torch.equal(s2, s)
    # ties go to the even mantissa, magnitudes past 6 saturate, an all-zero group has byte 127
    w = torch.zeros((2, 32))
    w[0, :9] = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -7.9])
    q, s = K.quantize_mxfp4(w)
    assert s.tolist() == [[127], [127]] and not bool(q[1].any())
    assert K.dequantize_mxfp4(q, s)[0, :9].tolist() == [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -6.0]


def test_layer_and_model_state_dicts_round_trip_bit_for_bit():
    from hydrainfer_amd.layer.moe import SparseMoE
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM
    from tests.test_gpu_moe_model import moe_shape
    moe = SparseMoE.from_reference_state_dict("", R.block_weights("bf16"), R.TOPK).quantize_experts("mxfp4")
    assert moe.experts_mxfp4 and not moe.experts_fp8 and moe.shared_gate_up.dtype == torch.bfloat16
    assert moe.w_gate_up.shape == (R.E, 2 * R.I, R.H // 2) and moe.w_down_scale.shape == (R.E, R.H, R.I // 32)
    held = moe.w_gate_up
    assert moe.quantize_experts("mxfp4") is moe and moe.w_gate_up is held
    with pytest.raises(ValueError):
        moe.quantize_experts()                                   # the FP8 default on MXFP4 experts
    sd = moe.to_reference_state_dict("")
    assert sd["experts.3.up_proj.weight"].shape == (R.I, R.H // 2) and sd["experts.3.up_proj.weight_scale"].shape == (R.I, R.H // 32)
    back = SparseMoE.from_reference_state_dict("", sd, R.TOPK, dtype=torch.float16)
    assert back.experts_mxfp4 and back.router_weight.dtype == torch.float16
    sd2 = back.to_reference_state_dict("")
    assert sorted(sd2) == sorted(sd)
    assert all(torch.equal(sd2[k], v) for k, v in sd.items() if v.dtype == torch.uint8)
    missing = {k: v for k, v in sd.items() if k != "experts.2.down_proj.weight_scale"}
    with pytest.raises(KeyError, match="experts.2.down_proj.weight_scale"):
        SparseMoE.from_reference_state_dict("", missing, R.TOPK)

    kw = dict(seed=20, std=0.02, router_std=0.2, expert_std=0.1)
    a = DeepseekMoeForCausalLM.random_init(moe_shape(), torch.bfloat16, "cpu", expert_dtype="mxfp4", **kw)
    assert a.state["l1.moe.wgu"] is a.moe[1].w_gate_up and a.state["l1.moe.wgu_scale"].shape == (8, 256, 8)
    msd = a.to_reference_state_dict()
    b = DeepseekMoeForCausalLM.from_reference_state_dict(moe_shape(), msd, torch.bfloat16, "cpu")
    assert b.moe[1].experts_mxfp4 and sorted(b.state) == sorted(a.state)
    assert all(torch.equal(b.state[k], v) for k, v in a.state.items())
    msd2 = b.to_reference_state_dict()
    assert sorted(msd2) == sorted(msd) and all(torch.equal(msd2[k], v) for k, v in msd.items())
    with pytest.raises(ValueError):
        DeepseekMoeForCausalLM.random_init(moe_shape(), torch.bfloat16, "cpu", dense_dtype="fp4", **kw)
    # the byte model of the tiny model (tests/test_moe_fp8_cpu.py does the sum by hand): 1/2 + 1/32 byte per element
    two_d, per_expert = 1247232, 3 * 256 * 128
    assert a.weight_bytes(1) == 2 * two_d + 3 * (per_expert // 2 + per_expert // 32)
    assert a.weight_bytes(64) == 2 * two_d + 8 * (per_expert // 2 + per_expert // 32)


def test_the_built_library_holds_the_twelve_kernels_without_scratch():
    rows = [r for r in kernel_table.kernels() if r["name"].startswith("moe_gemm_mxfp4w_kernel<")]
    assert sorted(r["name"] for r in rows) == sorted(f"moe_gemm_mxfp4w_kernel<{t}, {mb}, {gu}>" for t in ("BF16", "F16")
                                                     for mb in (1, 2, 4) for gu in (0, 1))
    for r in rows:
        assert r.get("private_segment_fixed_size", 0) == 0 and r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, r
        assert r["vgpr_count"] <= 256 and r.get("group_segment_fixed_size", 0) == 0, r      # two workgroups of 4 waves per CU
