"""Generates tests/golden/g15_moe_block.npz: the reference's DeepseekV3MoE (hydrainfer/model/deepseek_v3.py:95-155) run on
the CPU in bf16 and fp16 on the seeded weights and inputs of tests/moe_block_ref.py.

    HYDRA_REFERENCE=<checkout of the reference> python tests/golden/generate_moe_block_golden.py

Reference OUTPUTS only (data): per case the output bits, the reference's expert ids, the indices of the kept token rows
and the reference's own error ratio; weights and inputs are regenerated from seeds by the tests.  Also the parameter names
of the reference's DeepseekForCausalLM for the tiny model of tests/test_gpu_moe_model.py.

Two conditions are enforced here, not assumed:
  ROUTING GAP.  A token is kept only if its k-th and (k+1)-th router scores differ by >= 1e-3 in the reference (spare rows
      are drawn and the first n that qualify are kept), so that an fp32 logit summed in another order picks the same
      experts.
  REFERENCE ERROR RATIO.  max |out - y64| / (tol (1 + |y64|)) <= 1 at tol = 1e-2 (bf16) / 1e-3 (fp16), y64 the float64
      evaluation of the same module with the same routing; stored, and the basis of the GPU tests' factor 2."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # repo root

from tests import moe_block_ref as R  # noqa: E402
from tests.golden.generate_goldens import import_reference  # noqa: E402


def reference_config(norm: bool, **over):
    cfg = dict(hidden_size=R.H, intermediate_size=4 * R.I, moe_intermediate_size=R.I, n_routed_experts=R.E,
               n_shared_experts=R.N_SHARED, num_experts_per_tok=R.TOPK, routed_scaling_factor=R.SCALE,
               scoring_func="softmax", aux_loss_alpha=0.001, seq_aux=True, topk_method="greedy", n_group=1, topk_group=1,
               norm_topk_prob=norm, hidden_act="silu")
    cfg.update(over)
    return SimpleNamespace(**cfg)


def reference_moe(dt: str, norm: bool):
    from hydrainfer.model.deepseek_v3 import DeepseekV3MoE
    moe = DeepseekV3MoE(reference_config(norm)).to(R.DTYPES[dt]).eval()
    moe.load_state_dict(R.block_weights(dt))
    return moe


def model_param_names():
    """Parameter names of the reference's decoder for the tiny MoE model (layer 0 dense, layer 1 sparse)."""
    from hydrainfer.model.deepseek_v3 import DeepseekV3Model
    cfg = reference_config(True, hidden_size=128, intermediate_size=256, moe_intermediate_size=128, num_hidden_layers=2,
                           first_k_dense_replace=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=512,
                           rms_norm_eps=1e-5, max_position_embeddings=64, rope_theta=10000.0)
    names = ["model." + k for k in DeepseekV3Model(cfg).state_dict().keys()] + ["lm_head.weight"]
    return sorted(n for n in names if "inv_freq" not in n and "cos_sin" not in n)


def main():
    import_reference()
    out = {}
    with torch.no_grad():
        for dt in R.DTYPES:
            wr, wgu, wdown, sgu, sdown = R.stacked(R.block_weights(dt))
            for norm in (False, True):
                moe = reference_moe(dt, norm)
                for n in R.N_VALUES:
                    cand = R.candidate_tokens(dt, n)
                    scores = torch.nn.functional.linear(cand.float(), moe.gate.weight.float()).softmax(dim=-1, dtype=torch.float32)
                    top = scores.sort(dim=-1, descending=True).values
                    keep = ((top[:, R.TOPK - 1] - top[:, R.TOPK]) >= R.MIN_GAP).nonzero()[:, 0][:n]
                    assert keep.numel() == n, f"{dt} n={n}: only {keep.numel()} rows hold the routing gap"
                    x = cand[keep]
                    y = moe(x)
                    ids, _ = moe.gate(x)
                    y64, _, _ = R.block(x, wr, wgu, wdown, sgu, sdown, R.TOPK, norm, R.SCALE, "f64", ids=ids.to(torch.int32))
                    ref64 = moe.double()(x.double())
                    moe.to(R.DTYPES[dt])
                    # (the module keeps its router and its combine in fp32 even when run in double: deepseek_v3.py:66, :150)
                    assert torch.allclose(ref64, y64, rtol=1e-5, atol=1e-6), "the float64 restatement is not the module's"
                    ratio = R.error_ratio(y, y64, R.TOL[dt])
                    assert ratio <= 1.0, f"{dt} norm={norm} n={n}: the reference's own error ratio is {ratio}"
                    key = R.fixture_key(dt, norm, n)
                    out[key + "_out"] = R.to_bits(y)
                    out[key + "_ids"] = ids.to(torch.int32).numpy()
                    out[key + "_keep"] = keep.to(torch.int32).numpy()
                    out[key + "_ratio"] = np.float64(ratio)
                    print(f"{key}: ratio {ratio:.3f}")
    out["model_param_names"] = np.array(model_param_names())
    np.savez_compressed(R.GOLDEN, **out)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
