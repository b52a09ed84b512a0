#!/usr/bin/env python3
"""What sampled decoding costs a decode step.

    python tools/bench_sampling.py [--reps 30] [--burst 20] [--out profiles/sample_rows.md]

1. Microseconds per launch of hx_sample_rows for rows in {32, 64}, n = 32064 (LLaVA-1.5's vocabulary), bf16, for three
   settings — (T=1, k=0, p=1): no selection; (T=0.7, k=50, p=0.9): both searches; (T=1, k=0, p=0.9): top-p over the
   whole row — each with 0 and 64 history entries per row.  Beside them, on the same logits: argmax_rows,
   penalized_argmax_rows, and `torch process_logits + multinomial`: the reference's process_logits
   (hydrainfer/sampling/logits_processor.py:49-93) restated in torch on the same GPU — gather / scatter of the history,
   the division, one descending sort, the two masks, softmax, cumsum, the gather back — followed by softmax and
   torch.multinomial, which is the path the launch replaces.  The variants ALTERNATE inside every repetition; a
   repetition times a burst of launches of one variant between two device events and divides by the burst length;
   medians and quartiles over the repetitions.
2. Milliseconds per EAGER decode step of a 2-layer model of LLaVA-1.5-7B's widths and vocabulary, 64 rows: the greedy
   step (forward) against the sampled one (records and histories packed into one pinned buffer, one host-to-device
   copy, forward_sampled, ids to the host), wall clock around a synchronised step, alternating.  The difference is what
   sampling adds to a step of any depth.

No number here is a threshold; the one requirement is that the launch beats the torch restatement in every row of
table 1 (the last column says so)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_penalties import histories, measure, row      # noqa: E402

N = 32064
SETTINGS = ((1.0, 0, 1.0), (0.7, 50, 0.9), (1.0, 0, 0.9))       # (temperature, top_k, top_p)
HIST = (0, 64)


def torch_process_and_draw(logits, ids, counts, f, p, r, temperature, top_k, top_p, generator):
    """the reference's process_logits, in torch on the device, then the draw; ids / counts: [rows, h] padded tables
    (h may be 0), the parameters [rows] tensors"""
    x = logits.float()
    if ids.shape[1]:
        score = x.gather(1, ids)
        score = score - counts * f[:, None]
        score = score - (counts > 0) * p[:, None]
        score = torch.where(score < 0, score * r[:, None], score / r[:, None])
        x.scatter_(1, ids, score)
    x.div_(temperature[:, None])
    k = torch.where(top_k <= 0, 2147483647, top_k)
    srt, order = x.sort(dim=-1, descending=True)
    srt.masked_fill_(torch.arange(x.shape[1], device=x.device)[None, :] >= k[:, None], float("-inf"))
    probs = srt.softmax(dim=-1)
    srt.masked_fill_((probs.cumsum(dim=-1) - probs) > top_p[:, None], float("-inf"))
    x = srt.gather(-1, order.argsort())
    return torch.multinomial(x.softmax(dim=-1), 1, generator=generator)


def launches(lines, reps, burst):
    from hydrainfer_amd._C.kernel.norm import argmax_rows
    from hydrainfer_amd.sampling import NO_PENALTIES, pack_penalty_step, pack_sample_step, penalized_argmax_rows, sample_rows
    lines += ["## The launch: microseconds, n = 32064, bf16", "",
              "| rows | history entries per row | variant | median | q1 | q3 | torch restatement / this |", "|---|---|---|---|---|---|---|"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    lost = []
    for rows in (32, 64):
        logits = (3.0 * torch.randn((rows, N), generator=torch.Generator().manual_seed(rows))).to(torch.bfloat16).cuda()
        ids_out = torch.empty(rows, dtype=torch.int64, device="cuda")
        for length in HIST:
            hists = histories(rows, length, rows + length)
            pens = (0.5, 0.5, 1.2) if length else NO_PENALTIES
            ptab = pack_penalty_step([(h, pens) for h in hists]).to_device("cuda")
            variants = [("argmax_rows", lambda: argmax_rows(logits, ids_out)),
                        ("penalized_argmax_rows", lambda ptab=ptab: penalized_argmax_rows(logits, *ptab, out=ids_out))]
            h_ids = torch.tensor([list(h.ids) for h in hists], dtype=torch.int64).reshape(rows, length).cuda()
            h_counts = torch.tensor([list(h.counts) for h in hists], dtype=torch.float32).reshape(rows, length).cuda()
            pen_t = [torch.full((rows,), v, device="cuda") for v in pens]
            pairs = []
            for t, k, p in SETTINGS:
                tag = f"T={t}, k={k}, p={p}"
                tables = pack_sample_step([(h, pens, (t, p, k, (1 << 40) + r, 3)) for r, h in enumerate(hists)]).to_device("cuda")
                tt, kk, pp = (torch.full((rows,), t, device="cuda"), torch.full((rows,), k, dtype=torch.int64, device="cuda"),
                              torch.full((rows,), p, device="cuda"))
                variants.append((f"sample_rows ({tag})", lambda tables=tables: sample_rows(logits, *tables, out=ids_out)))
                variants.append((f"torch process_logits + multinomial ({tag})",
                                 lambda tt=tt, kk=kk, pp=pp: torch_process_and_draw(logits, h_ids, h_counts, *pen_t, tt, kk, pp, gen)))
                pairs.append((variants[-2][0], variants[-1][0]))
            times = measure(variants, reps, burst)
            med = {name: statistics.median(times[name]) for name, _ in variants}
            ratio = {a: med[b] / med[a] for a, b in pairs}
            for name, _ in variants:
                q = statistics.quantiles(times[name], n=4)
                row(lines, [str(rows), str(length), name, f"{med[name]:.1f}", f"{q[0]:.1f}", f"{q[2]:.1f}",
                            f"{ratio[name]:.1f}" if name in ratio else ""])
            lost += [f"{a} at {rows} rows, {length} history entries" for a, b in pairs if med[a] >= med[b]]
    lines += ["", "Configurations in which the launch LOSES to the torch restatement: " + ("; ".join(lost) if lost else "none") + ".", ""]


def eager_steps(lines, reps):
    from hydrainfer_amd.model.llama import LlamaForCausalLM, LlamaShape
    from hydrainfer_amd.model.runner import DecodeRunner, RunnerConfig
    from hydrainfer_amd.sampling import NO_PENALTIES, pack_sample_step
    lines += ["## The eager decode step: milliseconds (2 layers of LLaVA-1.5-7B's widths, vocabulary 32064, fp16, 512 cached tokens per row)",
              "", "| rows | step | median | q1 | q3 | minus the greedy step (us) |", "|---|---|---|---|---|---|"]
    dev = torch.device("cuda:0")
    model = LlamaForCausalLM.random_init(LlamaShape(4096, 11008, 2, 32, 32, 128, N), torch.float16, dev, seed=3)
    rows = 64
    runner = DecodeRunner(model, RunnerConfig(batch=rows, prompt_len=512, n_generate=8, use_graph=False), seed=4)
    ids = torch.randint(0, 32000, (rows,), generator=torch.Generator().manual_seed(1)).to(dev)

    def greedy():
        runner.set_state(512, ids)
        runner._advance()
        return model.forward(runner.input_ids, runner.positions, runner.decode_params).tolist()

    def sampled(hists, pens, setting):
        runner.set_state(512, ids)
        runner._advance()
        t, k, p = setting
        tables = pack_sample_step([(h, pens, (t, p, k, (1 << 40) + r, 3)) for r, h in enumerate(hists)]).to_device(dev)
        return model.forward_sampled(runner.input_ids, runner.positions, runner.decode_params, *tables).tolist()
    variants = [("greedy (forward)", greedy)]
    for length in HIST:
        hists = histories(rows, length, 7 * rows + length)
        pens = (0.5, 0.5, 1.2) if length else NO_PENALTIES
        for setting in SETTINGS:
            variants.append((f"sampled (forward_sampled), T={setting[0]}, k={setting[1]}, p={setting[2]}, {length} history entries per row",
                             lambda hists=hists, pens=pens, setting=setting: sampled(hists, pens, setting)))
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
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    lines = ["# hx_sample_rows: what sampled decoding costs", "",
             "`python " + " ".join(["tools/bench_sampling.py"] + sys.argv[1:]) + "`", ""]
    launches(lines, args.reps, args.burst)
    eager_steps(lines, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
