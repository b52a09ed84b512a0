#!/usr/bin/env python3
"""What a token mask costs the sampling launch (hx_sample_rows_masked).

    python tools/bench_token_mask.py [--reps 30] [--burst 20] [--commit REV] [--out profiles/sample_rows_masked.md]

Microseconds per launch for rows in {32, 64}, n = 32064 (LLaVA-1.5's vocabulary), bf16, no history, no bias entries,
records (T=0.7, k=50, p=0.9), timed as tools/bench_sample_logprobs.py times its launches (the variants ALTERNATE inside
every repetition; a repetition times a burst of launches of one variant between two device events and divides by the
burst length; medians and quartiles over the repetitions):
(a) hx_sample_rows_masked with no row masked (every mask_row = -1, every want = -1) beside hx_sample_rows_logprobs with
    every row unscored on the same inputs — the one expectation this tool checks: (a) lies inside the spread (q1 .. q3) of
    that baseline measured in the same run; the unscored launch (logprobs NULL) and hx_sample_rows_constrained for scale;
(b) every row masked, 4 allowed tokens, one distinct mask per row;
(c) every row masked, half of the vocabulary allowed, one distinct mask per row;
    each of the two beside hx_sample_rows_logprobs over logits that carry -inf at the masked positions — the launch the
    contract names, which the masked one equals bit for bit: the difference is the mask's own cost, the rest is what the
    body does with a row of that many -inf;
(d) the host's wall time for the sampling part of an eager 64-row step over ready logits — pack the step's tables, one
    pinned upload, the launch, the ids back, a list — as the constrained step (pack_constrained_step,
    hx_sample_rows_constrained) and with all 64 rows masked by distinct masks (pack_masked_step, hx_sample_rows_masked).
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
K = 5


def distinct_masks(rows, count, seed):
    """one mask per row, `count` allowed tokens each, as arrays of their own (pack_masked_step tells masks apart by identity)"""
    from hydrainfer_amd.sampling import pack_mask_words
    g = torch.Generator().manual_seed(seed)
    return [pack_mask_words(torch.randperm(N, generator=g)[:count].tolist(), N) for _ in range(rows)]


def launches(lines, reps, burst):
    from hydrainfer_amd._C.kernel.norm import logprob_rows_bytes
    from hydrainfer_amd.sampling import (NO_PENALTIES, pack_masked_step, sample_rows_constrained, sample_rows_logprobs,
                                         sample_rows_masked)
    lines += ["## The launch: microseconds, n = 32064, bf16, T=0.7, k=50, p=0.9, no history, no bias entries", "",
              "| rows | variant | median | q1 | q3 | x sample_rows_logprobs, every row unscored |", "|---|---|---|---|---|---|"]
    notes = []
    for rows in (32, 64):
        logits = (3.0 * torch.randn((rows, N), generator=torch.Generator().manual_seed(rows))).to(torch.bfloat16).cuda()
        ids_out = torch.empty(rows, dtype=torch.int64, device="cuda")
        out = torch.empty(logprob_rows_bytes(rows, K), dtype=torch.uint8, device="cuda")
        four = [(None, NO_PENALTIES, RECORD + ((1 << 40) + r, 3), None) for r in range(rows)]
        few, half = distinct_masks(rows, 4, rows), distinct_masks(rows, N // 2, rows + 1)
        dev = lambda masks: pack_masked_step([e + (-1, m) for e, m in zip(four, masks)]).to_device("cuda")
        *none, want = dev([None] * rows)
        *t_few, _ = dev(few)
        *t_half, _ = dev(half)
        plain = none[:4] + none[6:]                 # sample_rows_logprobs' tables: the same without allow_words, mask_row

        def banned(masks):
            keep = torch.from_numpy(np.unpackbits(np.stack(masks).view(np.uint8), axis=1, bitorder="little")[:, :N].astype(bool))
            return logits.masked_fill(~keep.cuda(), float("-inf"))
        x_few, x_half = banned(few), banned(half)
        base = "sample_rows_logprobs, every want = -1"
        variants = [(base, lambda: sample_rows_logprobs(logits, *plain, top_k=K, want=want, out=out)),
                    ("sample_rows_constrained", lambda: sample_rows_constrained(logits, *plain, out=ids_out)),
                    ("(a) sample_rows_masked, no row masked, every want = -1",
                     lambda: sample_rows_masked(logits, *none, top_k=K, want=want, out=out)),
                    ("(a') sample_rows_masked, no row masked, unscored launch",
                     lambda: sample_rows_masked(logits, *none, out=ids_out)),
                    ("(b) sample_rows_masked, every row masked, 4 allowed, every want = -1",
                     lambda: sample_rows_masked(logits, *t_few, top_k=K, want=want, out=out)),
                    ("(b ref) sample_rows_logprobs, -inf in the logits at those positions, every want = -1",
                     lambda: sample_rows_logprobs(x_few, *plain, top_k=K, want=want, out=out)),
                    ("(c) sample_rows_masked, every row masked, half the vocabulary allowed, every want = -1",
                     lambda: sample_rows_masked(logits, *t_half, top_k=K, want=want, out=out)),
                    ("(c ref) sample_rows_logprobs, -inf in the logits at those positions, every want = -1",
                     lambda: sample_rows_logprobs(x_half, *plain, top_k=K, want=want, out=out)),
                    ("(c') the same, every row scored, K=5",
                     lambda: sample_rows_masked(logits, *t_half, top_k=K, out=out))]
        times = measure(variants, reps, burst)
        med = {name: statistics.median(times[name]) for name, _ in variants}
        for name, _ in variants:
            q = statistics.quantiles(times[name], n=4)
            row(lines, [str(rows), name, f"{med[name]:.1f}", f"{q[0]:.1f}", f"{q[2]:.1f}", f"{med[name] / med[base]:.3f}"])
        q = statistics.quantiles(times[base], n=4)
        a = med[variants[2][0]]
        inside = q[0] <= a <= q[2]
        notes.append(f"- {rows} rows: (a) {a:.1f} us against the baseline's median {med[base]:.1f} us, q1 .. q3 = {q[0]:.1f} .. "
                     f"{q[2]:.1f} us: {'INSIDE' if inside else 'OUTSIDE'} the baseline's spread "
                     f"((q3 - q1) / median = {(q[2] - q[0]) / med[base]:.3f})")
        b, c, b_ref, c_ref = (med[variants[i][0]] for i in (4, 6, 5, 7))
        notes.append(f"- {rows} rows: against (a), 4 allowed tokens per row {b - a:+.1f} us, half the vocabulary {c - a:+.1f} "
                     f"us; against hx_sample_rows_logprobs over logits with -inf at the same positions {b - b_ref:+.1f} us "
                     f"and {c - c_ref:+.1f} us")
    lines += ["", "## Against the expectation, from the run above", ""] + notes + [""]
    for n in notes:
        print(n, flush=True)


def host_steps(lines, reps):
    from hydrainfer_amd.sampling import (NO_PENALTIES, pack_constrained_step, pack_masked_step, sample_rows_constrained,
                                         sample_rows_masked)
    rows = 64
    lines += ["## (d) The sampling part of an eager 64-row step on the host: milliseconds of wall time over ready logits", "",
              "| step | median | q1 | q3 | minus the constrained step (us) |", "|---|---|---|---|---|"]
    logits = (3.0 * torch.randn((rows, N), generator=torch.Generator().manual_seed(5))).to(torch.bfloat16).cuda()
    four = [(None, NO_PENALTIES, RECORD + ((1 << 40) + r, 3, 0.0), None) for r in range(rows)]
    masks = distinct_masks(rows, 4, 9)          # built at admission, not per step: outside the timed part
    six = [e + (-1, m) for e, m in zip(four, masks)]

    def constrained():
        tables = pack_constrained_step(four).to_device("cuda")
        return sample_rows_constrained(logits, *tables).tolist()

    def masked():
        *tables, _ = pack_masked_step(six).to_device("cuda")
        return sample_rows_masked(logits, *tables).tolist()
    variants = [("the constrained step (pack, upload, hx_sample_rows_constrained, ids back)", constrained),
                ("64 of 64 rows masked, distinct masks (pack with 64 masks of 4 KB, upload, hx_sample_rows_masked, ids back)",
                 masked)]
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
    lines = ["# hx_sample_rows_masked: what a token mask costs the sampling launch", "",
             f"{datetime.date.today().isoformat()}, commit {commit}, {torch.cuda.get_device_name(0)}", "",
             "`python " + " ".join(["tools/bench_token_mask.py"] + sys.argv[1:]) + "`", ""]
    launches(lines, args.reps, args.burst)
    host_steps(lines, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
