#!/usr/bin/env python3
"""What scoring the chosen token costs the sampling launch (hx_sample_rows_logprobs).

    python tools/bench_sample_logprobs.py [--reps 30] [--burst 20] [--commit REV] [--out profiles/sample_rows_logprobs.md]

Microseconds per launch for rows in {32, 64}, n = 32064 (LLaVA-1.5's vocabulary), bf16, no history, no bias entries,
records (T=0.7, k=50, p=0.9), timed as tools/bench_constraints.py times its launches (the variants ALTERNATE inside every
repetition; a repetition times a burst of launches of one variant between two device events and divides by the burst
length; medians and quartiles over the repetitions):
(a) hx_sample_rows_logprobs with every want = -1 beside hx_sample_rows_constrained on the same inputs — the one
    expectation this tool checks: (a) lies inside the spread (q1 .. q3) of the baseline measured in the same run;
(b) every row scored, K = 0, 5, 20;
(c) hx_sample_rows_constrained followed by hx_token_logprob_rows (targets: the sampled ids) with the same K: the
    two-launch route to RAW scores of the sampled tokens, for scale;
(d) the host's wall time for the sampling part of an eager 64-row step over ready logits — pack the step's tables, one
    pinned upload, the launch, one copy back, lists — without scored rows (hx_sample_rows_constrained) and with half of
    the rows scored at K = 5.
No number here is a threshold."""
import argparse
import datetime
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_penalties import measure, row      # noqa: E402

N = 32064
RECORD = (0.7, 0.9, 50)                         # (temperature, top_p, top_k)
KS = (0, 5, 20)


def launches(lines, reps, burst):
    from hydrainfer_amd._C.kernel.norm import logprob_rows_bytes, token_logprob_rows
    from hydrainfer_amd.sampling import NO_PENALTIES, pack_constrained_step, sample_rows_constrained, sample_rows_logprobs
    lines += ["## The launch: microseconds, n = 32064, bf16, T=0.7, k=50, p=0.9, no history, no bias entries", "",
              "| rows | variant | median | q1 | q3 | x hx_sample_rows_constrained |", "|---|---|---|---|---|---|"]
    notes = []
    for rows in (32, 64):
        logits = (3.0 * torch.randn((rows, N), generator=torch.Generator().manual_seed(rows))).to(torch.bfloat16).cuda()
        ids_out = torch.empty(rows, dtype=torch.int64, device="cuda")
        recs = [RECORD + ((1 << 40) + r, 3) for r in range(rows)]
        step = pack_constrained_step([(None, NO_PENALTIES, rec, None) for rec in recs]).to_device("cuda")
        none = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        outs = {k: torch.empty(logprob_rows_bytes(rows, k), dtype=torch.uint8, device="cuda") for k in KS}
        base = "sample_rows_constrained"
        variants = [(base, lambda: sample_rows_constrained(logits, *step, out=ids_out)),
                    ("(a) sample_rows_logprobs, every want = -1, K=5",
                     lambda: sample_rows_logprobs(logits, *step, top_k=5, want=none, out=outs[5]))]
        for k in KS:
            variants.append((f"(b) sample_rows_logprobs, every row scored, K={k}",
                             lambda k=k: sample_rows_logprobs(logits, *step, top_k=k, out=outs[k])))
        for k in KS:
            def two(k=k):
                ids = sample_rows_constrained(logits, *step, out=ids_out)
                token_logprob_rows(logits, ids.to(torch.int32), k)
            variants.append((f"(c) sample_rows_constrained + token_logprob_rows, K={k}", two))
        times = measure(variants, reps, burst)
        med = {name: statistics.median(times[name]) for name, _ in variants}
        for name, _ in variants:
            q = statistics.quantiles(times[name], n=4)
            row(lines, [str(rows), name, f"{med[name]:.1f}", f"{q[0]:.1f}", f"{q[2]:.1f}", f"{med[name] / med[base]:.3f}"])
        q = statistics.quantiles(times[base], n=4)
        a = med["(a) sample_rows_logprobs, every want = -1, K=5"]
        inside = q[0] <= a <= q[2]
        notes.append(f"- {rows} rows: (a) {a:.1f} us against the baseline's median {med[base]:.1f} us, q1 .. q3 = {q[0]:.1f} .. "
                     f"{q[2]:.1f} us: {'INSIDE' if inside else 'OUTSIDE'} the baseline's spread "
                     f"((q3 - q1) / median = {(q[2] - q[0]) / med[base]:.3f})")
        notes.append(f"- {rows} rows: scoring every row adds " + ", ".join(
            f"{med[f'(b) sample_rows_logprobs, every row scored, K={k}'] - med[base]:+.1f} us at K={k}" for k in KS)
            + "; the two-launch route to raw scores adds " + ", ".join(
            f"{med[f'(c) sample_rows_constrained + token_logprob_rows, K={k}'] - med[base]:+.1f} us at K={k}" for k in KS))
    lines += ["", "## Against the expectation, from the run above", ""] + notes + [""]
    for n in notes:
        print(n, flush=True)


def host_steps(lines, reps):
    from hydrainfer_amd._C.kernel.norm import logprob_rows_packed, logprob_rows_views
    from hydrainfer_amd.sampling import NO_PENALTIES, pack_constrained_step, sample_rows_constrained, sample_rows_logprobs
    rows, k = 64, 5
    lines += ["## (d) The sampling part of an eager 64-row step on the host: milliseconds of wall time over ready logits", "",
              "| step | median | q1 | q3 | minus the step without scored rows (us) |", "|---|---|---|---|---|"]
    logits = (3.0 * torch.randn((rows, N), generator=torch.Generator().manual_seed(5))).to(torch.bfloat16).cuda()
    entries = [(None, NO_PENALTIES, RECORD + ((1 << 40) + r, 3, 0.0), None) for r in range(rows)]

    def without():
        tables = pack_constrained_step(entries).to_device("cuda")
        return sample_rows_constrained(logits, *tables).tolist()

    def scored():
        step = pack_constrained_step(entries)
        size = step.buffer.size
        host = np.empty(size + rows, dtype=np.int32)
        host[:size] = step.buffer
        host[size:] = -1
        host[size::2] = 0                                    # every other row asks
        dev = torch.from_numpy(host).pin_memory().to("cuda", non_blocking=True)
        ids = sample_rows_logprobs(logits, *step.views(dev[:size]), top_k=k, want=dev[size:])[0]
        ids, lp, top_ids, top_lp = logprob_rows_views(logprob_rows_packed(ids, k).cpu(), rows, k)
        return ids.tolist(), lp.tolist(), top_ids.tolist(), top_lp.tolist()
    variants = [("no scored rows (pack, upload, hx_sample_rows_constrained, ids back)", without),
                (f"32 of 64 rows scored, K={k} (pack, upload with want, hx_sample_rows_logprobs, packed buffer back)", scored)]
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
        row(lines, [name, f"{med:.3f}", f"{q[0]:.3f}", f"{q[2]:.3f}", f"{(med - base) * 1e3:+.0f}"])
    lines.append("")


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
    lines = ["# hx_sample_rows_logprobs: what scoring the chosen token costs the sampling launch", "",
             f"{datetime.date.today().isoformat()}, commit {commit}, {torch.cuda.get_device_name(0)}", "",
             "`python " + " ".join(["tools/bench_sample_logprobs.py"] + sys.argv[1:]) + "`", ""]
    launches(lines, args.reps, args.burst)
    host_steps(lines, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
