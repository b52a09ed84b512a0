#!/usr/bin/env python3
"""What focal image-token pruning costs and what it saves.

    python tools/bench_focal.py [--reps 30] [--skip-engine] [--out profiles/focal_prune.md]

1. The captured vision encode (CLIP ViT-L/14-336 + projector, bf16, random weights) for 1 and 8 images with n_keep =
   None / 64 / 144: one hipGraph per variant, the variants ALTERNATE inside every repetition, a repetition times one
   replay between two device events, medians and quartiles over the repetitions.  pruned - None = the cost of the four
   added launches (column sums, dot products, select, gather).
2. The 7B-shaped engine (random weights) with 576 against 64 image tokens per request, 128 text tokens: time to the first
   token of a LONE request (encode + prefill; requests 0.5 s apart, median over them) and the time per output token of 32
   requests decoding together (the 32-row decode step), from the engine's own per-token stamps.

No number here is a threshold."""
import argparse
import dataclasses
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def vision_part(reps, lines):
    from hydrainfer_amd.model.clip import CLIP_VIT_L_14_336, LlavaVisionModel
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    model = LlavaVisionModel.random_init(CLIP_VIT_L_14_336, dt, dev, seed=1)
    lines += ["## Captured vision encode (CLIP ViT-L/14-336 + projector, bf16), one replay, microseconds", "",
              "| images | n_keep | median | q1 | q3 | minus unpruned |", "|---|---|---|---|---|---|"]
    for n_img in (1, 8):
        px = torch.randn((n_img, 3, 336, 336), generator=torch.Generator().manual_seed(n_img)).to(dev).to(dt)
        graphs = []
        for keep in (None, 64, 144):
            extra = () if keep is None else (torch.full((n_img,), keep, dtype=torch.int32, device=dev),)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                model(px, *extra)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = model(px, *extra)
            graphs.append((keep, g, out))
        for _ in range(5):
            for _, g, _ in graphs:
                g.replay()
        torch.cuda.synchronize()
        times = {keep: [] for keep, _, _ in graphs}
        for _ in range(reps):
            for keep, g, _ in graphs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                times[keep].append(e0.elapsed_time(e1) * 1e3)
        base = statistics.median(times[None])
        for keep, ts in times.items():
            q = statistics.quantiles(ts, n=4)
            med = statistics.median(ts)
            lines.append(f"| {n_img} | {keep} | {med:.1f} | {q[0]:.1f} | {q[2]:.1f} | {med - base:+.1f} |")
            print(lines[-1])
    lines.append("")


def engine_part(lines):
    from hydrainfer_amd.engine.node import LocalCluster
    from hydrainfer_amd.engine.rcb import TokenParameters
    from hydrainfer_amd.engine.request_processor import InstructionCreator
    from hydrainfer_amd.engine.scheduler import BatchSchedulerConfig
    from hydrainfer_amd.engine.serve import build_node, replay, synthetic_requests, warm_library_gemms
    from hydrainfer_amd.model.clip import CLIP_VIT_L_14_336, LlavaVisionModel
    from hydrainfer_amd.model.llama import LLAVA_1_5_7B, LlamaForCausalLM
    from hydrainfer_amd.model.llava import LlavaLanguageModel
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    shape = LLAVA_1_5_7B
    lm = LlavaLanguageModel(LlamaForCausalLM.random_init(shape, dt, dev, seed=0), image_token_id=32000)
    vision = LlavaVisionModel.random_init(dataclasses.replace(CLIP_VIT_L_14_336, projector_hidden_size=shape.hidden_size),
                                          dt, dev, seed=1)
    rng = np.random.RandomState(0)
    pixels = torch.from_numpy(rng.rand(336, 336, 3).astype(np.float32) * 4 - 2).permute(2, 0, 1)[None]
    n_text, gen, rows = 128, 48, 32
    per_req = (576 + n_text + gen + 15) // 16 + 1
    sched = BatchSchedulerConfig(priority="prefill", max_running_requests=rows, chunked_prefill=True, token_budgets=2048,
                                 image_budgets=8)
    node = build_node("EPD0", "EPD", lm, vision, shape, dt, dev, per_req * (2 * rows + 2), 2 * rows + 2, 576, sched,
                      graph_decode=True, max_blocks_per_seq=per_req)
    node.executor.fill_executor.graph_decoder.warmup([rows], kv_max=1024)
    cluster = LocalCluster([node])
    creator = InstructionCreator(image_token_id=32000, n_image_tokens_per_image=576, block_size=16)
    warm_library_gemms(lm, 2048, rows, vision, pixels, 8)
    focal = TokenParameters(token_pruning_policy="focal", n_embed_output_tokens=64)

    def requests(n, tp, seed):
        reqs = synthetic_requests(n, n_text, gen, 32000, pixels, seed=seed)
        for r in reqs:
            r.token_params = tp
        return reqs

    lines += ["## 7B-shaped engine (random weights, bf16), 128 text tokens per request, milliseconds", "",
              "| image tokens | prompt | lone request: time to first token (encode + prefill), p50 | 32 requests together: time per output token, p50 |",
              "|---|---|---|---|"]
    for name, tp, seed in (("576", None, 3), ("64 (focal)", focal, 5)):
        replay(cluster, creator, requests(rows, tp, seed), [0.0] * rows, dev)                 # warm-up: graphs, allocator
        replay(cluster, creator, requests(2, tp, seed + 1), [0.0, 0.5], dev)
        lone = replay(cluster, creator, requests(8, tp, seed + 2), [0.5 * i for i in range(8)], dev)
        together = replay(cluster, creator, requests(rows, tp, seed + 3), [0.0] * rows, dev)
        n_img = 576 if tp is None else tp.n_embed_output_tokens
        lines.append(f"| {name} | {n_img + n_text} | {lone['ttft_p50_ms']:.2f} | {together['tpot_p50_ms']:.3f} |")
        print(lines[-1])
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    lines = ["# Focal image-token pruning: cost of the launches, effect on a request", "",
             "`python " + " ".join(["tools/bench_focal.py"] + sys.argv[1:]) + "`", ""]
    vision_part(args.reps, lines)
    if not args.skip_engine:
        engine_part(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
