#!/usr/bin/env python3
"""The routed-expert feed-forward on FP8 block-scaled expert weights (csrc/moe_experts_fp8.hip) against the same four
launches on bf16 weights (csrc/moe_experts.hip): segments, gate|up + silu*mul, down, combine — K.experts_forward with and
without the scales.  Routed experts only; the router and the shared experts are outside both.

    python tools/bench_moe_experts_fp8.py [--out profiles/moe_experts_fp8.md] [--rounds 5]

Shapes (h, I, E, topk) and method are tools/bench_moe_experts.py's: DeepSeek-VL2-small's (2048, 1408, 64, 6) and a
Mixtral-shaped (4096, 14336, 8, 2); n in {1, 8, 32, 64} and one prefill point, n = 704; bf16 activations.  Both paths run
in one process on the same x and the same 16 pre-drawn routings (cycled, so that a small step's few experts are not
served from the last-level cache by the repetition before), warmed up, then `rounds` rounds that alternate fp8 / bf16;
in a round a path is timed with device events over enough repetitions to fill 0.2 s.  The fp8 weights are
quantize_fp8_block of the bf16 ones.  Reported per path: the median over the rounds and their min .. max, the bytes the
step needs — distinct experts hit x 3 h I x (2 B, resp. 1 B + 4 B per 128 x 128 block), averaged over the routings, plus
the activations both GEMMs read and write — and the rate that gives; then bf16 / fp8.  Also, per point, the largest
|fp8 path - bf16 path on the dequantised weights| of one routing: the two differ in where the scale is applied only."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hydrainfer_amd._C.kernel.moe import experts as K  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_moe_experts import N_ROUTINGS, SHAPES, timed  # noqa: E402

DEV = torch.device("cuda:0")
N_VALUES = (1, 8, 32, 64, 704)


def needed_bytes(hit: float, n: int, h: int, inter: int, topk: int, fp8: bool) -> float:
    per_expert = 3 * h * inter
    weights = hit * (per_expert + 4 * per_expert // (128 * 128) if fp8 else per_expert * 2)
    return weights + 2 * (n * h + 2 * n * topk * inter + 2 * n * topk * h + n * h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "moe_experts_fp8.md"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dt = torch.bfloat16
    lines = ["# Routed-expert feed-forward: FP8 block-scaled expert weights vs bf16 weights, the same four launches", "",
             f"`python tools/bench_moe_experts_fp8.py --rounds {args.rounds}` on {torch.cuda.get_device_name(0)}, bf16 activations; "
             "method in the tool's header.  Both paths: segments + gate|up+silu*mul + down + combine; fp8 = e4m3 bytes + one fp32 "
             "scale per 128 x 128 block (`hx_moe_*_fp8w`).  us: median of the rounds (min .. max); TB/s: the needed bytes of "
             "that path over its median.", ""]
    slower = []
    for name, (h, inter, n_e, topk) in SHAPES.items():
        g = torch.Generator(device=DEV).manual_seed(1)
        wgu = (torch.randn((n_e, 2 * inter, h), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dt)
        wdown = (torch.randn((n_e, h, inter), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dt)
        qgu, sgu = K.quantize_fp8_block(wgu)
        qdown, sdown = K.quantize_fp8_block(wdown)
        torch.cuda.empty_cache()
        lines += [f"## {name}", "", "| n | fp8 us | bf16 us | fp8 bytes needed | fp8 TB/s | bf16 bytes needed | bf16 TB/s | bf16 / fp8 |",
                  "|---|---|---|---|---|---|---|---|"]
        for n in N_VALUES:
            x = torch.randn((n, h), device=DEV, generator=g, dtype=torch.float32).to(dt)
            routings, hit = [], []
            for _ in range(N_ROUTINGS):
                scores = torch.rand((n, n_e), device=DEV, generator=g)
                w, ids = scores.softmax(dim=-1).topk(topk, dim=-1)
                routings.append((ids.to(torch.int32).contiguous(), w.contiguous()))
                hit.append(int(ids.unique().numel()))
            fp8 = lambda ids32, w: K.experts_forward(x, qgu, qdown, w, ids32, w_gate_up_scale=sgu, w_down_scale=sdown)
            b16 = lambda ids32, w: K.experts_forward(x, wgu, wdown, w, ids32)
            # what the fp8 path computes, on the bf16 kernels: the experts the first routing hits, dequantised (exact in
            # fp32, then rounded to bf16 — the one difference besides the summation order)
            ids0 = routings[0][0]
            es = ids0.unique().long()
            dq_gu, dq_down = wgu.clone(), wdown.clone()
            dq_gu[es] = K.dequantize_fp8_block(qgu[es], sgu[es]).to(dt)
            dq_down[es] = K.dequantize_fp8_block(qdown[es], sdown[es]).to(dt)
            ref = K.experts_forward(x, dq_gu, dq_down, routings[0][1], ids0).float()
            got = fp8(*routings[0]).float()
            diff, scale = float((got - ref).abs().max()), float(ref.abs().max())
            del dq_gu, dq_down, ref, got
            for r in routings[:4]:
                fp8(*r); b16(*r)
            torch.cuda.synchronize()
            t8, t16 = [], []
            for _ in range(args.rounds):
                t8.append(timed(fp8, routings))
                t16.append(timed(b16, routings))
            mhit = statistics.mean(hit)
            need8, need16 = needed_bytes(mhit, n, h, inter, topk, True), needed_bytes(mhit, n, h, inter, topk, False)
            m8, m16 = statistics.median(t8), statistics.median(t16)
            lines.append(f"| {n} | {m8:.1f} ({min(t8):.1f} .. {max(t8):.1f}) | {m16:.1f} ({min(t16):.1f} .. {max(t16):.1f}) | "
                         f"{need8 / 1e6:.1f} MB ({mhit:.1f} experts) | {need8 / m8 / 1e6:.2f} | {need16 / 1e6:.1f} MB | "
                         f"{need16 / m16 / 1e6:.2f} | {m16 / m8:.2f}x |")
            print(lines[-1], f" max |fp8 - bf16 on dequantised weights| = {diff:.5f} (max |out| {scale:.3f})", flush=True)
            if m8 > m16:
                slower.append(f"{name}, n = {n}: fp8 {m8:.1f} us against bf16 {m16:.1f} us")
        lines.append("")
        del wgu, wdown, qgu, qdown
        torch.cuda.empty_cache()
    lines += ["## fp8 not slower than bf16 at any measured point?", "",
              "Yes: the fp8 median is at or below the bf16 median of the same run at every point." if not slower else
              "NO — " + "; ".join(slower), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
