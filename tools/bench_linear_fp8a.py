#!/usr/bin/env python3
"""The W8A8 prefill path (hx_quant_fp8_group + hx_linear_fp8a, csrc/gemm_fp8a.hip) against today's prefill path over the
same FP8 block-scaled weight (hx_dequant_fp8_block + torch.matmul) and against torch.matmul on a bf16 weight.

    python tools/bench_linear_fp8a.py [--out profiles/linear_fp8a.md] [--rounds 5] [--skip-model]

Kernel: M = 128 / 704 / 2048 / 4096 over the dense shapes of a DeepSeek-VL2-small sparse layer and one 7B-sized pair, bf16
activations.  An arm is REPS back-to-back calls captured into a hipGraph (no host launch cost in the figure) and timed with
device events; every arm is warmed up on every shape first, then `rounds` rounds interleave the arms.  The operands of a
shape (4 .. 45 MB of weight) stay warm in the caches, as they do between the chunks of a prefill.  Reported: the median of the rounds (min .. max) in us, the GEMM's achieved
TFLOP/s (2 M N K over its own time), the same for quantise + GEMM and for the two torch arms, and whether quantise + GEMM
beats dequantise + matmul by more than that arm's spread (max - min).  "fp8a_tile_rows" is forced to 64 and 128 in turn and
left automatic: the rule in the library is read off this table.

Model: the 4-layer model of tools/bench_linear_fp8.py with FP8 dense linears; its 704-token prefill chunk, eager, with the
switch off and on; and, on the tiny model of tests/test_gpu_moe_model_fp8_dense.py, the largest logit difference and the
share of identical greedy tokens over 32 steps, switch on against switch off."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_linear_fp8 import capture, cell, eager_us, replay_us, step_inputs  # noqa: E402
from hydrainfer_amd import _lib  # noqa: E402
from hydrainfer_amd._C.kernel import gemm  # noqa: E402
from hydrainfer_amd._C.kernel.moe.experts import quantize_fp8_block  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = {"qkv (6144, 2048)": (6144, 2048), "o (2048, 2048)": (2048, 2048), "gate|up (5632, 2048)": (5632, 2048),
          "down (2048, 2816)": (2048, 2816), "7B (4096, 4096)": (4096, 4096), "7B (11008, 4096)": (11008, 4096)}
M_VALUES = (128, 704, 2048, 4096)
REPS = 10


def tile_option(rows: int) -> None:
    _lib.check(_lib.lib().hx_debug_set_option(b"fp8a_tile_rows", rows), "fp8a_tile_rows")


def kernel_part(rounds, lines):
    dt = torch.bfloat16
    lost = []
    lines += ["## Kernels", "",
              "| shape | M | quantise us | GEMM us (tile 64) | GEMM us (tile 128) | GEMM us (automatic) | GEMM TFLOP/s | quantise + GEMM us | "
              "dequantise + matmul us | bf16 matmul us | TFLOP/s: new / today / bf16 | beats today by more than its spread |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, (N, K) in SHAPES.items():
        g = torch.Generator(device=DEV).manual_seed(N + K)
        w16 = (torch.randn((N, K), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dt)
        q, s = quantize_fp8_block(w16)
        scratch = torch.empty((N, K), dtype=dt, device=DEV)
        for M in M_VALUES:
            x = torch.randn((M, K), device=DEV, generator=g, dtype=torch.float32).to(dt)
            out = torch.empty((M, N), dtype=dt, device=DEV)
            xq, xs = gemm.quant_fp8_group(x)
            arms = {"quant": lambda: gemm.quant_fp8_group(x, out=(xq, xs)),
                    "g64": lambda: gemm.linear_fp8a(xq, xs, q, s, dt, out=out),
                    "g128": lambda: gemm.linear_fp8a(xq, xs, q, s, dt, out=out),
                    "gemm": lambda: gemm.linear_fp8a(xq, xs, q, s, dt, out=out),
                    "today": lambda: torch.matmul(x, gemm.dequant_fp8_block(q, s, dt, out=scratch).t(), out=out),
                    "bf16": lambda: torch.matmul(x, w16.t(), out=out)}
            graphs = {}
            for k, fn in arms.items():                       # the tile height is decided when the launch is recorded
                tile_option({"g64": 64, "g128": 128}.get(k, 0))
                graphs[k] = capture(lambda fn=fn: [fn() for _ in range(REPS)])
            tile_option(0)
            ts = {k: [] for k in arms}
            for r in range(rounds + 1):                      # round 0 warms every arm up
                for k, graph in graphs.items():
                    t = replay_us(graph, REPS)
                    if r:
                        ts[k].append(t)
            del graphs
            med = {k: statistics.median(v) for k, v in ts.items()}
            new = med["quant"] + med["gemm"]
            clear = med["today"] - new > max(ts["today"]) - min(ts["today"])
            fl = 2.0 * M * N * K / 1e6
            lines.append(f"| {name} | {M} | {cell(ts['quant'])} | {cell(ts['g64'])} | {cell(ts['g128'])} | {cell(ts['gemm'])} | "
                         f"{fl / med['gemm']:.0f} | {new:.2f} | {cell(ts['today'])} | {cell(ts['bf16'])} | "
                         f"{fl / new:.0f} / {fl / med['today']:.0f} / {fl / med['bf16']:.0f} | {'yes' if clear else 'NO'} |")
            print(lines[-1], flush=True)
            if not clear and M >= 704:
                lost.append(f"{name}, M = {M}: {new:.1f} us against {med['today']:.1f} us")
    lines += ["", "Quantise + GEMM faster than dequantise + matmul at every M >= 704 by more than that arm's spread? " +
              ("Yes." if not lost else "NO — " + "; ".join(lost)), ""]


def model_part(rounds, lines):
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM, MoeShape
    dt = torch.bfloat16
    shape = MoeShape(hidden_size=2048, intermediate_size=11008, num_hidden_layers=4, num_attention_heads=16, num_key_value_heads=16,
                     head_dim=128, vocab_size=4096, rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=4096,
                     n_routed_experts=64, num_experts_per_tok=6, moe_intermediate_size=1408, n_shared_experts=2,
                     first_k_dense_replace=0)
    model = DeepseekMoeForCausalLM.random_init(shape, dt, DEV, seed=1, expert_dtype="fp8", dense_dtype="fp8")
    pool = torch.zeros((shape.num_hidden_layers, 2, 512, 16, shape.num_key_value_heads, shape.head_dim), dtype=dt, device=DEV)
    ids, pos, params = step_inputs(shape, 1, 704, 0, pool)
    ts = {False: [], True: []}
    for r in range(rounds + 1):
        for on in (True, False):
            model.enable_fp8_activations(on)
            model.forward_logits(ids, pos, params)
            t = eager_us(lambda: model.forward_logits(ids, pos, params))
            if r:
                ts[on].append(t)
    off, on = statistics.median(ts[False]), statistics.median(ts[True])
    lines += ["## Model: 704-token prefill chunk, 4 sparse VL2-small-shaped layers, FP8 experts and FP8 dense linears, eager", "",
              "| switch off us | switch on us | off / on | faster by more than the off side's spread |", "|---|---|---|---|",
              f"| {cell(ts[False])} | {cell(ts[True])} | {off / on:.3f}x | {'yes' if off - on > max(ts[False]) - min(ts[False]) else 'NO'} |", ""]
    print(lines[-2], flush=True)
    model.release()
    # accuracy on the tiny model: recorded, not asserted
    from tests import test_gpu_moe_model as MM
    from tests.golden import cases as C
    tiny = DeepseekMoeForCausalLM.random_init(MM.moe_shape(), dt, DEV, seed=0, std=0.08, dense_dtype="fp8")
    tshape = tiny.shape
    worst, same, steps = 0.0, 0, 32
    pools = {on: torch.zeros((tshape.num_hidden_layers, 2, 16, 16, tshape.num_key_value_heads, tshape.head_dim), dtype=dt, device=DEV)
             for on in (False, True)}
    prompt = torch.randint(0, tshape.vocab_size, (130,), generator=torch.Generator().manual_seed(5)).to(DEV)
    ctx, new = 0, {False: prompt, True: prompt}
    for _ in range(steps):                                    # every step re-prefills > 64 rows so that the switch acts
        logits = {}
        for on in (False, True):
            tiny.enable_fp8_activations(on)
            i, p, prm = step_inputs(tshape, 1, int(new[on].numel()), ctx, pools[on])
            logits[on] = tiny.forward_logits(new[on], p, prm).float()
        worst = max(worst, float((logits[True] - logits[False]).abs().max()))
        tok = {on: logits[on][-1].argmax() for on in logits}
        same += int(tok[True] == tok[False])
        # both sides follow the switch-off tokens; the context is rebuilt from scratch with one more token
        prompt = torch.cat([prompt, tok[False].view(1)])[-200:]
        new = {False: prompt, True: prompt}
    lines += ["## Accuracy on the tiny model (tests/test_gpu_moe_model_fp8_dense.py's shape, bf16), recorded, not asserted", "",
              f"Prefill of a growing 130 .. 161-token prompt, 32 greedy steps, each step a fresh prefill so that the switch acts: largest "
              f"logit difference switch on against off {worst:.4f} (the project's bf16 logit tolerance is {MM.LOGIT_TOL['bf16']}); "
              f"identical greedy tokens {same} of {steps}.", ""]
    print(lines[-2], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "linear_fp8a.md"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    args = ap.parse_args()
    lines = ["# W8A8 prefill: per-token-group FP8 activations x FP8 block-scaled weights on the FP8 MFMAs", "",
             f"`python tools/bench_linear_fp8a.py --rounds {args.rounds}` on {torch.cuda.get_device_name(0)}, bf16 activations; method in "
             "the tool's header.  us: median of the rounds (min .. max).", ""]
    if not args.skip_kernels:
        kernel_part(args.rounds, lines)
    if not args.skip_model:
        model_part(args.rounds, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
