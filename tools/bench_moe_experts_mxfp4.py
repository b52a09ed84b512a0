#!/usr/bin/env python3
"""The routed-expert feed-forward on MXFP4 expert weights (csrc/moe_experts_mxfp4.hip) against the same four launches on
FP8 block-scaled weights (csrc/moe_experts_fp8.hip) and on bf16 weights (csrc/moe_experts.hip): segments, gate|up +
silu*mul, down, combine — K.experts_forward with uint8 scales, fp32 scales and none.  Routed experts only.

    python tools/bench_moe_experts_mxfp4.py [--out profiles/moe_experts_mxfp4.md] [--rounds 5]

Shapes and method are tools/bench_moe_experts_fp8.py's: DeepSeek-VL2-small's (2048, 1408, 64, 6) and a Mixtral-shaped
(4096, 14336, 8, 2); n in {1, 8, 32, 64} and the prefill chunk n = 704; bf16 activations.  The three paths run in one
process on the same x and the same 16 pre-drawn routings (cycled), warmed up, then `rounds` rounds that alternate
mxfp4 / fp8 / bf16; in a round a path is timed with device events over enough repetitions to fill 0.2 s.  The quantised
weights are quantize_mxfp4 / quantize_fp8_block of the bf16 ones.  Reported per path: the median over the rounds and
their min .. max, and the rate of the bytes the step needs — distinct experts hit x 3 h I x (1/2 + 1/32 B, 1 B + 4 B per
128 x 128 block, 2 B), averaged over the routings, plus the activations both GEMMs read and write.  Also, per point, the
largest |mxfp4 path - bf16 path on the dequantised weights| of one routing (bf16 holds every dequantised MXFP4 weight
exactly: the two differ in the summation order only)."""
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
BYTES_PER_ELEMENT = {"mxfp4": 0.5 + 1 / 32, "fp8": 1 + 4 / (128 * 128), "bf16": 2.0}


def needed_bytes(hit: float, n: int, h: int, inter: int, topk: int, fmt: str) -> float:
    return hit * 3 * h * inter * BYTES_PER_ELEMENT[fmt] + 2 * (n * h + 2 * n * topk * inter + 2 * n * topk * h + n * h)


def per_expert(quantize, w):
    """quantize(w[e]) stacked: the float64 temporaries of quantize_mxfp4 stay one expert large."""
    parts = [quantize(w[e]) for e in range(w.shape[0])]
    return torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "moe_experts_mxfp4.md"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dt = torch.bfloat16
    lines = ["# Routed-expert feed-forward: MXFP4 vs FP8 block-scaled vs bf16 expert weights, the same four launches", "",
             f"`python tools/bench_moe_experts_mxfp4.py --rounds {args.rounds}` on {torch.cuda.get_device_name(0)}, bf16 activations; "
             "method in the tool's header.  All paths: segments + gate|up+silu*mul + down + combine; mxfp4 = E2M1 nibbles + one "
             "E8M0 byte per 32 k (`hx_moe_*_mxfp4w`), fp8 = e4m3 bytes + one fp32 scale per 128 x 128 block (`hx_moe_*_fp8w`).  "
             "us: median of the rounds (min .. max); TB/s: the needed bytes of that path over its median.", ""]
    slower = []
    for name, (h, inter, n_e, topk) in SHAPES.items():
        g = torch.Generator(device=DEV).manual_seed(1)
        wgu = (torch.randn((n_e, 2 * inter, h), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dt)
        wdown = (torch.randn((n_e, h, inter), device=DEV, generator=g, dtype=torch.float32) * 0.02).to(dt)
        f8 = K.quantize_fp8_block(wgu) + K.quantize_fp8_block(wdown)
        mgu, msgu = per_expert(K.quantize_mxfp4, wgu)
        mdown, msdown = per_expert(K.quantize_mxfp4, wdown)
        torch.cuda.empty_cache()
        lines += [f"## {name}", "", "| n | mxfp4 us | fp8 us | bf16 us | experts hit | mxfp4 TB/s | fp8 TB/s | bf16 TB/s | fp8 / mxfp4 | bf16 / mxfp4 |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for n in N_VALUES:
            x = torch.randn((n, h), device=DEV, generator=g, dtype=torch.float32).to(dt)
            routings, hit = [], []
            for _ in range(N_ROUTINGS):
                scores = torch.rand((n, n_e), device=DEV, generator=g)
                w, ids = scores.softmax(dim=-1).topk(topk, dim=-1)
                routings.append((ids.to(torch.int32).contiguous(), w.contiguous()))
                hit.append(int(ids.unique().numel()))
            paths = {"mxfp4": lambda ids32, w: K.experts_forward(x, mgu, mdown, w, ids32, w_gate_up_scale=msgu, w_down_scale=msdown),
                     "fp8": lambda ids32, w: K.experts_forward(x, f8[0], f8[2], w, ids32, w_gate_up_scale=f8[1], w_down_scale=f8[3]),
                     "bf16": lambda ids32, w: K.experts_forward(x, wgu, wdown, w, ids32)}
            # what the mxfp4 path computes, on the bf16 kernels: the experts the first routing hits, dequantised
            ids0 = routings[0][0]
            es = ids0.unique().long()
            dq_gu, dq_down = wgu.clone(), wdown.clone()
            for e in es.tolist():
                dq_gu[e] = K.dequantize_mxfp4(mgu[e], msgu[e]).to(dt)
                dq_down[e] = K.dequantize_mxfp4(mdown[e], msdown[e]).to(dt)
            ref = K.experts_forward(x, dq_gu, dq_down, routings[0][1], ids0).float()
            got = paths["mxfp4"](*routings[0]).float()
            diff, scale = float((got - ref).abs().max()), float(ref.abs().max())
            del dq_gu, dq_down, ref, got
            for r in routings[:4]:
                for fn in paths.values():
                    fn(*r)
            torch.cuda.synchronize()
            t = {k: [] for k in paths}
            for _ in range(args.rounds):
                for k, fn in paths.items():
                    t[k].append(timed(fn, routings))
            mhit = statistics.mean(hit)
            med = {k: statistics.median(v) for k, v in t.items()}
            cell = lambda k: f"{med[k]:.1f} ({min(t[k]):.1f} .. {max(t[k]):.1f})"
            rate = lambda k: f"{needed_bytes(mhit, n, h, inter, topk, k) / med[k] / 1e6:.2f}"
            lines.append(f"| {n} | {cell('mxfp4')} | {cell('fp8')} | {cell('bf16')} | {mhit:.1f} | {rate('mxfp4')} | {rate('fp8')} | "
                         f"{rate('bf16')} | {med['fp8'] / med['mxfp4']:.2f}x | {med['bf16'] / med['mxfp4']:.2f}x |")
            print(lines[-1], f" max |mxfp4 - bf16 on dequantised weights| = {diff:.5f} (max |out| {scale:.3f})", flush=True)
            if med["mxfp4"] > med["fp8"]:
                slower.append(f"{name}, n = {n}: mxfp4 {med['mxfp4']:.1f} us against fp8 {med['fp8']:.1f} us "
                              f"(fp8's own spread {min(t['fp8']):.1f} .. {max(t['fp8']):.1f})")
        lines.append("")
        del wgu, wdown, f8, mgu, msgu, mdown, msdown
        torch.cuda.empty_cache()
    lines += ["## mxfp4 not slower than fp8 at any measured point?", "",
              "Yes: the mxfp4 median is at or below the fp8 median of the same run at every point." if not slower else
              "NO — " + "; ".join(slower), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
