#!/usr/bin/env python3
"""What token constraints (logit_bias, min_tokens, min_p) cost the sampling launch.

    python tools/bench_constraints.py [--reps 30] [--burst 20] [--commit REV] [--out profiles/sample_rows_constrained.md]

Microseconds per launch for rows in {32, 64}, n = 32064 (LLaVA-1.5's vocabulary), bf16, no history, timed as
tools/bench_sampling.py times hx_sample_rows (the variants ALTERNATE inside every repetition; a repetition times a burst
of launches of one variant between two device events and divides by the burst length; medians and quartiles over the
repetitions):
- hx_sample_rows at (T=1, k=0, p=1) and (T=0.7, k=50, p=0.9): the baseline;
- hx_sample_rows_constrained on the same records with no bias entries, with 16 and with 300 entries per row;
- the same with min_p = 0.05 and no entries, without and with top-k / top-p;
- an all-greedy constrained batch (T = 0, 16 entries per row) beside hx_penalized_argmax_rows and hx_argmax_rows: what a
  constrained greedy step pays for riding through the sampling launch.
Below the table: the ratio of the no-entry constrained launch to hx_sample_rows and the run-to-run spread of the baseline
leg ((q3 - q1) / median) from the same run.  No number here is a threshold."""
import argparse
import datetime
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_penalties import measure, row      # noqa: E402

N = 32064
SETTINGS = ((1.0, 0, 1.0), (0.7, 50, 0.9))      # (temperature, top_k, top_p)
ENTRIES = (0, 16, 300)
MIN_P = 0.05


def tables_of(rows, count, seed):
    """`rows` bias tables of `count` distinct tokens each, biases in -5 .. 5"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randperm(N, generator=g)[:count].to(torch.int32).numpy(),
             (torch.rand(count, generator=g) * 10 - 5).numpy().astype(np.float32)) for _ in range(rows)]


def launches(lines, reps, burst):
    from hydrainfer_amd._C.kernel.norm import argmax_rows
    from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, pack_constrained_step, pack_penalty_step,
                                         pack_sample_step, penalized_argmax_rows, sample_rows, sample_rows_constrained)
    lines += ["## The launch: microseconds, n = 32064, bf16, no history", "",
              "| rows | variant | median | q1 | q3 | x hx_sample_rows, same record |", "|---|---|---|---|---|---|"]
    notes = []
    for rows in (32, 64):
        logits = (3.0 * torch.randn((rows, N), generator=torch.Generator().manual_seed(rows))).to(torch.bfloat16).cuda()
        ids_out = torch.empty(rows, dtype=torch.int64, device="cuda")
        variants, base_of = [], {}
        for t, k, p in SETTINGS:
            tag = f"T={t}, k={k}, p={p}"
            recs = [(t, p, k, (1 << 40) + r, 3) for r in range(rows)]
            plain = pack_sample_step([(None, NO_PENALTIES, rec) for rec in recs]).to_device("cuda")
            base = f"sample_rows ({tag})"
            variants.append((base, lambda plain=plain: sample_rows(logits, *plain, out=ids_out)))
            for count in ENTRIES:
                bias = tables_of(rows, count, rows + count)
                step = pack_constrained_step([(None, NO_PENALTIES, rec, b) for rec, b in zip(recs, bias)]).to_device("cuda")
                variants.append((f"sample_rows_constrained ({tag}), {count} bias entries per row",
                                 lambda step=step: sample_rows_constrained(logits, *step, out=ids_out)))
                base_of[variants[-1][0]] = base
            step = pack_constrained_step([(None, NO_PENALTIES, rec + (MIN_P,), None) for rec in recs]).to_device("cuda")
            variants.append((f"sample_rows_constrained ({tag}), min_p={MIN_P}, no bias entries",
                             lambda step=step: sample_rows_constrained(logits, *step, out=ids_out)))
            base_of[variants[-1][0]] = base
        empty = pack_penalty_step([(None, NO_PENALTIES)] * rows).to_device("cuda")
        greedy = pack_constrained_step([(None, NO_PENALTIES, GREEDY_RECORD, b) for b in tables_of(rows, 16, 7 * rows)]).to_device("cuda")
        variants += [("argmax_rows", lambda: argmax_rows(logits, ids_out)),
                     ("penalized_argmax_rows, no history", lambda: penalized_argmax_rows(logits, *empty, out=ids_out)),
                     ("sample_rows_constrained, all rows greedy (T=0), 16 bias entries per row",
                      lambda: sample_rows_constrained(logits, *greedy, out=ids_out))]
        times = measure(variants, reps, burst)
        med = {name: statistics.median(times[name]) for name, _ in variants}
        for name, _ in variants:
            q = statistics.quantiles(times[name], n=4)
            row(lines, [str(rows), name, f"{med[name]:.1f}", f"{q[0]:.1f}", f"{q[2]:.1f}",
                        f"{med[name] / med[base_of[name]]:.3f}" if name in base_of else ""])
        for t, k, p in SETTINGS:
            tag = f"T={t}, k={k}, p={p}"
            base = f"sample_rows ({tag})"
            q = statistics.quantiles(times[base], n=4)
            none = f"sample_rows_constrained ({tag}), 0 bias entries per row"
            notes.append(f"- {rows} rows, {tag}: no-entry constrained launch / hx_sample_rows = {med[none] / med[base]:.3f} "
                         f"({med[none]:.1f} / {med[base]:.1f} us); spread of the baseline leg (q3 - q1) / median = "
                         f"{(q[2] - q[0]) / med[base]:.3f}")
        g = "sample_rows_constrained, all rows greedy (T=0), 16 bias entries per row"
        notes.append(f"- {rows} rows, greedy: constrained launch {med[g]:.1f} us, hx_penalized_argmax_rows "
                     f"{med['penalized_argmax_rows, no history']:.1f} us, hx_argmax_rows {med['argmax_rows']:.1f} us: a "
                     f"constrained greedy step pays {med[g] - med['argmax_rows']:+.1f} us over the argmax launch")
    lines += ["", "## Ratios, from the run above", ""] + notes + [""]
    for n in notes:
        print(n, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--commit", default=None, help="the revision measured (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                    check=True).stdout.strip()
        except Exception:
            commit = "unknown"
    lines = ["# hx_sample_rows_constrained: what token constraints cost the sampling launch", "",
             f"{datetime.date.today().isoformat()}, commit {commit}, {torch.cuda.get_device_name(0)}", "",
             "`python " + " ".join(["tools/bench_constraints.py"] + sys.argv[1:]) + "`", ""]
    launches(lines, args.reps, args.burst)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
