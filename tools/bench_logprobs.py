#!/usr/bin/env python3
"""What per-token log-probabilities cost a decode step.

    python tools/bench_logprobs.py [--reps 30] [--burst 20] [--out profiles/logprob_rows.md]

Microseconds per launch of hx_logprob_rows (the greedy id, its log-softmax value and the K most likely alternatives of
every row) for rows in {1, 8, 32, 64}, n = 32064 (LLaVA-1.5's vocabulary), K in {0, 5, 20}, fp16 and bf16 — beside
 * argmax_rows on the same logits: the launch it stands beside in a step without log-probabilities (the kernel of the
   parent commit: this change does not touch norm_rope_act.hip), and
 * the torch sequence it replaces: log_softmax(logits.float(), -1), then topk(K) (K = 0: argmax) and a gather.

The variants ALTERNATE inside every repetition; a repetition times a burst of launches of one variant between two device
events and divides by the burst length; medians and quartiles over the repetitions.  The logits were just written
(as by the lm_head GEMM in a step), so they are read through the caches the way a step reads them.

No number here is a threshold."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 32064


def torch_sequence(logits, k):
    lsm = torch.log_softmax(logits.float(), dim=-1)
    if k == 0:
        ids = lsm.argmax(-1)
        return ids, lsm.gather(1, ids[:, None])
    return torch.topk(lsm, k, dim=-1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    from hydrainfer_amd._C.kernel.norm import argmax_rows, logprob_rows, logprob_rows_bytes
    lines = ["# hx_logprob_rows: microseconds per launch, n = 32064", "",
             "`python " + " ".join(["tools/bench_logprobs.py"] + sys.argv[1:]) + "`", "",
             "| dtype | rows | variant | median | q1 | q3 | x argmax_rows |", "|---|---|---|---|---|---|---|"]
    for dname, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        for rows in (1, 8, 32, 64):
            logits = (4.0 * torch.randn((rows, N), generator=torch.Generator().manual_seed(rows))).to(dt).cuda()
            ids_out = torch.empty(rows, dtype=torch.int64, device="cuda")
            variants = [("argmax_rows", lambda: argmax_rows(logits, ids_out))]
            for k in (0, 5, 20):
                out = torch.empty(logprob_rows_bytes(rows, k), dtype=torch.uint8, device="cuda")
                variants.append((f"logprob_rows K={k}", lambda k=k, out=out: logprob_rows(logits, k, out)))
            for k in (0, 5, 20):
                variants.append((f"torch log_softmax(float)+topk K={k}", lambda k=k: torch_sequence(logits, k)))
            times = measure(variants, args.reps, args.burst)
            base = statistics.median(times["argmax_rows"])
            for name, _ in variants:
                q, med = statistics.quantiles(times[name], n=4), statistics.median(times[name])
                lines.append(f"| {dname} | {rows} | {name} | {med:.1f} | {q[0]:.1f} | {q[2]:.1f} | {med / base:.2f} |")
                print(lines[-1], flush=True)
    lines.append("")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
