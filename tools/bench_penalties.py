#!/usr/bin/env python3
"""What frequency / presence / repetition penalties cost a decode step.

    python tools/bench_penalties.py [--reps 30] [--burst 20] [--out profiles/penalized_argmax.md]

1. Microseconds per launch of hx_penalized_argmax_rows for rows in {32, 64}, n = 32064 (LLaVA-1.5's vocabulary) and
   histories of 0, 64 and 1024 distinct tokens per row, fp16 and bf16 — beside argmax_rows on the same logits, the
   launch it replaces in a step without penalties.  The variants ALTERNATE inside every repetition; a repetition times
   a burst of launches of one variant between two device events and divides by the burst length; medians and quartiles
   over the repetitions.
2. Milliseconds per EAGER decode step (the step a batch with a penalised request takes) of a 2-layer model of
   LLaVA-1.5-7B's widths and vocabulary, 32 and 64 rows: the unpenalised step (forward: logits, argmax_rows, ids to the
   host) against the penalised one (the rows' histories packed into one pinned buffer, one host-to-device copy,
   forward_penalized, ids to the host), wall clock around a synchronised step, alternating.  The difference is what the
   penalties add to a step of any depth: packing, the copy and the wider launch.

No number here is a threshold."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 32064
HIST = (0, 64, 1024)


def measure(variants, reps, burst):
    for _ in range(3):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(burst):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / burst)
    return times


def histories(rows, length, seed):
    """`rows` PenaltyHistory tables of `length` distinct tokens each, counts 1..8"""
    from hydrainfer_amd.sampling import PenaltyHistory
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(rows):
        ids = torch.randperm(N, generator=g)[:length].tolist()
        counts = torch.randint(1, 9, (length,), generator=g).tolist()
        out.append(PenaltyHistory([t for t, c in zip(ids, counts) for _ in range(c)]))
    return out


def row(lines, cells):
    lines.append("| " + " | ".join(cells) + " |")
    print(lines[-1], flush=True)


def launches(lines, reps, burst):
    from hydrainfer_amd._C.kernel.norm import argmax_rows
    from hydrainfer_amd.sampling import pack_penalty_step, penalized_argmax_rows
    lines += ["## The launch: microseconds, n = 32064", "",
              "| dtype | rows | variant | median | q1 | q3 | x argmax_rows |", "|---|---|---|---|---|---|---|"]
    for dname, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        for rows in (32, 64):
            logits = (4.0 * torch.randn((rows, N), generator=torch.Generator().manual_seed(rows))).to(dt).cuda()
            ids_out = torch.empty(rows, dtype=torch.int64, device="cuda")
            variants = [("argmax_rows", lambda: argmax_rows(logits, ids_out))]
            for length in HIST:
                tables = pack_penalty_step([(h, (0.5, 0.5, 1.2)) for h in histories(rows, length, rows + length)]).to_device("cuda")
                variants.append((f"penalized_argmax_rows, {length} history entries per row",
                                 lambda tables=tables: penalized_argmax_rows(logits, *tables, out=ids_out)))
            times = measure(variants, reps, burst)
            base = statistics.median(times["argmax_rows"])
            for name, _ in variants:
                q, med = statistics.quantiles(times[name], n=4), statistics.median(times[name])
                row(lines, [dname, str(rows), name, f"{med:.1f}", f"{q[0]:.1f}", f"{q[2]:.1f}", f"{med / base:.2f}"])
    lines.append("")


def eager_steps(lines, reps):
    from hydrainfer_amd.model.llama import LlamaForCausalLM, LlamaShape
    from hydrainfer_amd.model.runner import DecodeRunner, RunnerConfig
    from hydrainfer_amd.sampling import pack_penalty_step
    lines += ["## The eager decode step: milliseconds (2 layers of LLaVA-1.5-7B's widths, vocabulary 32064, fp16, 512 cached tokens per row)",
              "", "| rows | step | median | q1 | q3 | minus the unpenalised step (us) |", "|---|---|---|---|---|---|"]
    dev = torch.device("cuda:0")
    model = LlamaForCausalLM.random_init(LlamaShape(4096, 11008, 2, 32, 32, 128, N), torch.float16, dev, seed=3)
    for rows in (32, 64):
        runner = DecodeRunner(model, RunnerConfig(batch=rows, prompt_len=512, n_generate=8, use_graph=False), seed=4)
        ids = torch.randint(0, 32000, (rows,), generator=torch.Generator().manual_seed(1)).to(dev)

        def plain():
            runner.set_state(512, ids)
            runner._advance()
            return model.forward(runner.input_ids, runner.positions, runner.decode_params).tolist()

        def penalised(hists):
            runner.set_state(512, ids)
            runner._advance()
            tables = pack_penalty_step([(h, (0.5, 0.5, 1.2)) for h in hists]).to_device(dev)
            return model.forward_penalized(runner.input_ids, runner.positions, runner.decode_params, *tables).tolist()
        variants = [("unpenalised (forward)", plain)]
        for length in HIST:
            hists = histories(rows, length, 7 * rows + length)
            variants.append((f"penalised (forward_penalized), {length} history entries per row", lambda hists=hists: penalised(hists)))
        for _ in range(3):
            for _, fn in variants:
                fn()
        times = {name: [] for name, _ in variants}
        for _ in range(reps):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
        base = statistics.median(times[variants[0][0]])
        for name, _ in variants:
            q, med = statistics.quantiles(times[name], n=4), statistics.median(times[name])
            row(lines, [str(rows), name, f"{med:.3f}", f"{q[0]:.3f}", f"{q[2]:.3f}", f"{(med - base) * 1e3:+.0f}"])
        del runner
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    lines = ["# hx_penalized_argmax_rows: what sampling penalties cost", "",
             "`python " + " ".join(["tools/bench_penalties.py"] + sys.argv[1:]) + "`", ""]
    launches(lines, args.reps, args.burst)
    eager_steps(lines, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
