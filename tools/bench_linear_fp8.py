#!/usr/bin/env python3
"""The decode GEMM on FP8 block-scaled dense weights (hx_linear_decode_fp8w, csrc/gemm_skinny_fp8.hip) against
hx_linear_decode on bf16 weights of the same shape, and a DeepSeek-VL2-small-shaped model with FP8 experts whose dense
linears (attention projections, shared experts) are bf16 or FP8.

    python tools/bench_linear_fp8.py [--out profiles/linear_fp8.md] [--rounds 5] [--skip-model]

Kernel: the four dense shapes of a sparse layer of that model — qkv (6144, 2048), o (2048, 2048), shared gate|up
(5632, 2048), shared down (2048, 2816) — at M = 1 / 8 / 32 / 64, bf16 activations.  COLD weights: every format has enough
copies of the weight (>= 400 MB of them, more than L2 and the 256 MB MALL hold) and one timed pass calls the entry once
per copy, so no call finds its weight in a cache; x, the workspace and the output are shared and stay warm.  A pass is
captured into a hipGraph (no host launch cost in the figure) and timed with device events; both formats in one process,
one warm-up pass each, then `rounds` rounds that alternate fp8 / bf16.  Reported: the median over the rounds and their
min .. max per side, the weight bytes over the median, bf16 / fp8, and whether fp8 is faster by more than the bf16 side's
spread (max - min).

Model: 4 sparse layers (first_k_dense_replace = 0: the dense layer of the published model has an intermediate size that
is no multiple of 128), h 2048, 16 heads of 128, 64 experts of I 1408, top 6, 2 shared experts, vocab 4096 (the lm_head is
bf16 in both and would only dilute the comparison); FP8 routed experts in both models, bf16 against FP8 dense linears.
One decode step of n = 1 / 8 / 32 sequences (128 tokens of context each), eager (host included) and replayed from a
hipGraph capture of the same step, and the 704-token prefill chunk, eager (it dequantises above 64 rows)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hydrainfer_amd._C.kernel import gemm  # noqa: E402
from hydrainfer_amd._C.kernel.moe.experts import quantize_fp8_block  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = {"qkv (6144, 2048)": (6144, 2048), "o (2048, 2048)": (2048, 2048), "shared gate|up (5632, 2048)": (5632, 2048),
          "shared down (2048, 2816)": (2048, 2816)}
M_VALUES = (1, 8, 32, 64)
COLD_BYTES = 400 << 20
BS = 16


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def replay_us(g, per: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / per * 1e3


def cell(ts):
    return f"{statistics.median(ts):.2f} ({min(ts):.2f} .. {max(ts):.2f})"


def kernel_part(rounds, lines):
    dt = torch.bfloat16
    not_faster = []
    lines += ["## Kernel: hx_linear_decode_fp8w against hx_linear_decode (bf16 weights), cold weights", "",
              "| shape | M | (waves, row groups) | fp8 us | bf16 us | fp8 TB/s | bf16 TB/s | bf16 / fp8 | faster by more than the bf16 spread |",
              "|---|---|---|---|---|---|---|---|---|"]
    for name, (N, K) in SHAPES.items():
        g = torch.Generator(device=DEV).manual_seed(N + K)
        nc = -(-COLD_BYTES // (N * K))
        w16 = [(torch.randn((N, K), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dt) for _ in range(nc)]
        w8 = [quantize_fp8_block(w) for w in w16]
        for M in M_VALUES:
            x = torch.randn((M, K), device=DEV, generator=g, dtype=torch.float32).to(dt)
            out = torch.empty((M, N), dtype=dt, device=DEV)
            g8 = capture(lambda: [gemm.linear_decode_fp8(x, q, s, out=out) for q, s in w8])
            g16 = capture(lambda: [gemm.linear_decode(x, w, out=out) for w in w16])
            replay_us(g8, nc); replay_us(g16, nc)
            t8, t16 = [], []
            for _ in range(rounds):
                t8.append(replay_us(g8, nc))
                t16.append(replay_us(g16, nc))
            m8, m16 = statistics.median(t8), statistics.median(t16)
            clear = m16 - m8 > max(t16) - min(t16)
            b8, b16 = N * K + 4 * (N // 128) * (K // 128), 2 * N * K
            lines.append(f"| {name} | {M} | {gemm.fp8_plan(M, N, K)} | {cell(t8)} | {cell(t16)} | {b8 / m8 / 1e6:.2f} | {b16 / m16 / 1e6:.2f} | "
                         f"{m16 / m8:.2f}x | {'yes' if clear else 'NO'} |")
            print(lines[-1], flush=True)
            if not clear:
                not_faster.append(f"{name}, M = {M}: fp8 {m8:.2f} us against bf16 {m16:.2f} us (bf16 spread {max(t16) - min(t16):.2f} us)")
            del g8, g16
        del w16, w8
        torch.cuda.empty_cache()
    lines += ["", "Faster than bf16 at every measured M on every shape, by more than the bf16 side's spread? " +
              ("Yes." if not not_faster else "NO — " + "; ".join(not_faster)), ""]


def step_inputs(shape, n_seq, q_len, ctx, pool):
    """(ids, positions, LanguageModelParameters) of n_seq sequences that each add q_len tokens behind ctx cached ones."""
    from hydrainfer_amd.layer.causal_attention import AttentionParametersBuilder
    from hydrainfer_amd.memory.kv_cache import KVCache
    from hydrainfer_amd.model.llama import LanguageModelParameters
    b = AttentionParametersBuilder(shape.num_attention_heads, shape.num_key_value_heads, shape.head_dim, BS, DEV)
    per = (ctx + q_len + BS - 1) // BS
    pos = []
    for r in range(n_seq):
        table = list(range(r * per, (r + 1) * per))
        b.add_request(q_len, ctx + q_len, [table[p // BS] * BS + p % BS for p in range(ctx, ctx + q_len)], table)
        pos += list(range(ctx, ctx + q_len))
    for l in range(shape.num_hidden_layers):
        b.add_kv_cache(KVCache(pool[l, 0], pool[l, 1]))
    decode = q_len == 1
    params = LanguageModelParameters(attention_params=b.build_attention_parameters(), all_sequences_decode=decode,
                                     selected_token_ids=None if decode else torch.tensor([n_seq * q_len - 1], device=DEV))
    g = torch.Generator().manual_seed(n_seq + q_len)
    ids = torch.randint(0, shape.vocab_size, (n_seq * q_len,), generator=g).to(DEV)
    return ids, torch.tensor(pos, dtype=torch.int32, device=DEV), params


def eager_us(fn, min_seconds=0.2):
    reps = 4
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_seconds * 1e3:
            return ms / reps * 1e3
        reps = max(reps * 2, int(reps * min_seconds * 1e3 / max(ms, 1e-3) * 1.2))


def model_part(rounds, lines):
    from hydrainfer_amd.model.deepseek_moe import DeepseekMoeForCausalLM, MoeShape
    dt = torch.bfloat16
    shape = MoeShape(hidden_size=2048, intermediate_size=11008, num_hidden_layers=4, num_attention_heads=16, num_key_value_heads=16,
                     head_dim=128, vocab_size=4096, rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=4096,
                     n_routed_experts=64, num_experts_per_tok=6, moe_intermediate_size=1408, n_shared_experts=2,
                     first_k_dense_replace=0)
    models = {"bf16 dense": DeepseekMoeForCausalLM.random_init(shape, dt, DEV, seed=1, expert_dtype="fp8"),
              "fp8 dense": DeepseekMoeForCausalLM.random_init(shape, dt, DEV, seed=1, expert_dtype="fp8", dense_dtype="fp8")}
    pool = torch.zeros((shape.num_hidden_layers, 2, 512, BS, shape.num_key_value_heads, shape.head_dim), dtype=dt, device=DEV)
    lines += ["## Model: 4 sparse VL2-small-shaped layers, FP8 routed experts, bf16 against FP8 dense linears", "",
              f"Bytes a one-token step streams (`weight_bytes(1)`): {models['bf16 dense'].weight_bytes(1) / 1e6:.1f} MB with bf16 dense "
              f"linears, {models['fp8 dense'].weight_bytes(1) / 1e6:.1f} MB with FP8 ones.", "",
              "| step | bf16 dense us | fp8 dense us | bf16 / fp8 | faster by more than the bf16 spread |", "|---|---|---|---|---|"]
    points = [(f"decode n = {n}, eager", n, 1, 128, False) for n in (1, 8, 32)]
    points += [(f"decode n = {n}, hipGraph replay", n, 1, 128, True) for n in (1, 8, 32)]
    points.append(("prefill chunk of 704 tokens, eager", 1, 704, 0, False))
    for label, n_seq, q_len, ctx, graphed in points:
        ids, pos, params = step_inputs(shape, n_seq, q_len, ctx, pool)
        fns = {k: (lambda m=m: m.forward_logits(ids, pos, params)) for k, m in models.items()}
        ts = {k: [] for k in fns}
        if graphed:
            graphs = {k: capture(f) for k, f in fns.items()}
            for g in graphs.values():
                replay_us(g, 1)
            for _ in range(rounds):
                for k in ("fp8 dense", "bf16 dense"):
                    ts[k].append(statistics.median(replay_us(graphs[k], 1) for _ in range(20)))
        else:
            for f in fns.values():
                f(); f()
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k in ("fp8 dense", "bf16 dense"):
                    ts[k].append(eager_us(fns[k]))
        m8, m16 = statistics.median(ts["fp8 dense"]), statistics.median(ts["bf16 dense"])
        clear = m16 - m8 > max(ts["bf16 dense"]) - min(ts["bf16 dense"])
        lines.append(f"| {label} | {cell(ts['bf16 dense'])} | {cell(ts['fp8 dense'])} | {m16 / m8:.2f}x | {'yes' if clear else 'NO'} |")
        print(lines[-1], flush=True)
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "linear_fp8.md"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    lines = ["# FP8 block-scaled dense linears: decode GEMM and model against bf16 weights", "",
             f"`python tools/bench_linear_fp8.py --rounds {args.rounds}` on {torch.cuda.get_device_name(0)}, bf16 activations; method in "
             "the tool's header.  us: median of the rounds (min .. max).", ""]
    kernel_part(args.rounds, lines)
    if not args.skip_model:
        model_part(args.rounds, lines)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
