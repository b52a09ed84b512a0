#!/usr/bin/env python3
"""The routed-expert feed-forward of a sparse MoE layer at decode sizes: the four launches of csrc/moe_experts.hip
(segments, gate|up + silu*mul, down, combine) against the reference's moe_infer restated in torch on the GPU
(hydrainfer/model/deepseek_v3.py:124-155: scatter_ / argsort / index, the tokens_per_expert.cpu() host synchronisation, a
Python loop of three library GEMMs per expert that has rows, the fp32 combine).  Both sides get the same topk ids and
weights; the router and the shared experts are outside both.

    python tools/bench_moe_experts.py [--out profiles/moe_experts.md] [--rounds 5]

Shapes (h, I, E, topk): DeepSeek-VL2-small's (2048, 1408, 64, 6) and a Mixtral-shaped (4096, 14336, 8, 2); n in
{1, 8, 32, 64}; bf16.  Method: both paths in one process, warmed up, then `rounds` rounds that alternate new / baseline;
in a round a path is timed with device events over enough repetitions to fill 0.2 s.  Successive repetitions use
DIFFERENT pre-drawn routings (16 of them, cycled), so a small step's few experts are not served from the 256 MB
last-level cache by the repetition before.  Reported: the median over the rounds and their min .. max (the spread), the
bytes the step needs — distinct experts hit x 3 h I 2 B, averaged over the routings, plus the activations both GEMMs read
and write — the rate that gives, and baseline / new."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hydrainfer_amd._C.kernel.moe import experts as K  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = {"DeepSeek-VL2-small (2048, 1408, 64, top 6)": (2048, 1408, 64, 6),
          "Mixtral-shaped (4096, 14336, 8, top 2)": (4096, 14336, 8, 2)}
N_VALUES = (1, 8, 32, 64)
N_ROUTINGS = 16


def baseline(x, ids64, w, wgu, wdown):
    """moe_infer, op for op."""
    n, topk = ids64.shape
    inter = wgu.shape[1] // 2
    cnts = ids64.new_zeros((n, wgu.shape[0]))
    cnts.scatter_(1, ids64, 1)
    tokens_per_expert = cnts.sum(dim=0)
    idxs = ids64.view(-1).argsort()
    sorted_tokens = x[idxs // topk]
    tokens_per_expert = tokens_per_expert.cpu().numpy()          # the host synchronisation
    outputs, start = [], 0
    for e, num in enumerate(tokens_per_expert):
        if num == 0:
            continue
        t = sorted_tokens[start:start + num]
        g = torch.nn.functional.linear(t, wgu[e, :inter])
        u = torch.nn.functional.linear(t, wgu[e, inter:])
        outputs.append(torch.nn.functional.linear(torch.nn.functional.silu(g) * u, wdown[e]))
        start += num
    outs = torch.cat(outputs, dim=0)
    new_x = torch.empty_like(outs)
    new_x[idxs] = outs
    return new_x.view(n, topk, -1).type(w.dtype).mul_(w.unsqueeze(dim=-1)).sum(dim=1).type(new_x.dtype)


def timed(fn, routings, min_seconds=0.2):
    """us per call: device events around enough calls (cycling the routings) to fill min_seconds."""
    reps = len(routings)
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(*routings[i % len(routings)])
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_seconds * 1e3:
            return ms / reps * 1e3
        reps = max(reps * 2, int(reps * min_seconds * 1e3 / max(ms, 1e-3) * 1.2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "moe_experts.md"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dt = torch.bfloat16
    lines = ["# Routed-expert feed-forward: grouped HIP launches vs the reference's moe_infer restated on the GPU", "",
             f"`python tools/bench_moe_experts.py --rounds {args.rounds}` on {torch.cuda.get_device_name(0)}, bf16; method in the "
             "tool's header.  new = segments + gate|up+silu*mul + down + combine (4 launches); baseline = scatter / argsort / "
             "index, `.cpu()`, three library GEMMs per expert that has rows, fp32 combine.  us: median of the rounds "
             "(min .. max).", ""]
    misses = []
    for name, (h, inter, n_e, topk) in SHAPES.items():
        g = torch.Generator(device=DEV).manual_seed(1)
        wgu = (torch.randn((n_e, 2 * inter, h), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dt)
        wdown = (torch.randn((n_e, h, inter), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dt)
        lines += [f"## {name}", "", "| n | new us | baseline us | bytes needed | new TB/s | baseline / new |", "|---|---|---|---|---|---|"]
        for n in N_VALUES:
            x = torch.randn((n, h), device=DEV, generator=g, dtype=torch.float32).to(dt)
            routings, hit = [], []
            for _ in range(N_ROUTINGS):
                scores = torch.rand((n, n_e), device=DEV, generator=g)
                w, ids = scores.softmax(dim=-1).topk(topk, dim=-1)
                routings.append((ids.to(torch.int32).contiguous(), ids.contiguous(), w.contiguous()))
                hit.append(int(ids.unique().numel()))
            new = lambda ids32, ids64, w: K.experts_forward(x, wgu, wdown, w, ids32)
            base = lambda ids32, ids64, w: baseline(x, ids64, w, wgu, wdown)
            diff = float((new(*routings[0]).float() - base(*routings[0]).float()).abs().max())
            for r in routings[:4]:                      # warm-up: library GEMM heuristics, allocator
                new(*r); base(*r)
            torch.cuda.synchronize()
            t_new, t_base = [], []
            for _ in range(args.rounds):
                t_new.append(timed(new, routings))
                t_base.append(timed(base, routings))
            need = statistics.mean(hit) * 3 * h * inter * 2 + 2 * (n * h + 2 * n * topk * inter + 2 * n * topk * h + n * h)
            mn, mb = statistics.median(t_new), statistics.median(t_base)
            lines.append(f"| {n} | {mn:.1f} ({min(t_new):.1f} .. {max(t_new):.1f}) | {mb:.1f} ({min(t_base):.1f} .. {max(t_base):.1f}) | "
                         f"{need / 1e6:.1f} MB ({statistics.mean(hit):.1f} experts) | {need / mn / 1e6:.2f} | {mb / mn:.1f}x |")
            print(lines[-1], f" max |new - baseline| = {diff:.4f}", flush=True)
            if mn > min(t_base):
                misses.append(f"{name}, n = {n}: new {mn:.1f} us is not below the baseline's fastest round {min(t_base):.1f} us")
        lines.append("")
        del wgu, wdown
        torch.cuda.empty_cache()
    lines += ["## Not slower than the baseline at any n <= 64?", "",
              "Yes at every point: the new path's median is below the baseline's fastest round." if not misses else
              "NO — " + "; ".join(misses), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
