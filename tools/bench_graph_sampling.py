"""What sampled decoding costs per decode step of the engine, from the captured step and from the eager path.
    python tools/bench_graph_sampling.py [--json OUT.json] [--baseline PARENT.json] [--out profiles/graph_sampling.md]

One MI355X, LLaVA-1.5-7B-shaped random weights, bf16, text-only requests that all decode together; 32 and 64 rows;
sampled rows use T = 0.7, top_k = 50, top_p = 0.9.  Legs:
  (a) an all-greedy batch (captured step, look-ahead, cohort);
  (b) an all-sampled batch, and one sampled row among greedy ones, with the graph_sampling switch off (eager steps);
  (c) the same two batches with the switch on.
A checkout that has no switch (the parent of the change that added it) runs (a) and (b) only: give its --json file as
--baseline and its leg (b) stands beside this checkout's in the report.

Per leg: the requests are admitted at once and stepped through their prefill and WARM decode steps, then WINDOWS windows of
STEPS engine steps are timed, the device synchronised at both ends of a window.  `ms/step` is a window's wall time over
its steps.  `host ms/step` is the time spent inside `cluster.step()` minus the time spent waiting inside
`GraphedDecoder.fetch` for an earlier launch's tokens: what the host needs to issue a step.  An eager step ends in a
blocking read of its own tokens, which cannot be told from host work here: its host time is the step itself.  The whole
sequence of legs runs PASSES times, so the windows of two legs that are compared alternate in time; the report gives the
median and the range over a leg's windows."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, STEPS, WINDOWS, PASSES = 24, 40, 3, 2
N_TEXT = 64
IMAGE_TOKEN_ID = 32064         # outside the vocabulary: random weights may GENERATE any id, and the eager step's builder
                               # takes an input row that holds the image token for an image row
SAMPLED = dict(temperature=0.7, top_k=50, top_p=0.9)


def build(graph_sampling, max_running):
    from hydrainfer_amd.engine.node import LocalCluster
    from hydrainfer_amd.engine.request_processor import InstructionCreator
    from hydrainfer_amd.engine.scheduler import BatchSchedulerConfig
    from hydrainfer_amd.engine.serve import build_node
    lm, vision, shape, dtype, dev = build.models
    per_req = (N_TEXT + WARM + STEPS * WINDOWS + 16 + 15) // 16 + 1
    sched = BatchSchedulerConfig(priority="prefill", max_running_requests=max_running, chunked_prefill=True,
                                 token_budgets=2048, image_budgets=8)
    extra = dict(graph_sampling=True) if graph_sampling else {}
    node = build_node("EPD0", "EPD", lm, vision, shape, dtype, dev, per_req * (max_running + 2), 2, 576, sched,
                      max_blocks_per_seq=per_req, **extra)
    node.executor.fill_executor.graph_decoder.warmup([32, 64], kv_max=256)
    creator = InstructionCreator(image_token_id=IMAGE_TOKEN_ID, n_image_tokens_per_image=576, block_size=16, ignore_eos=True)
    return LocalCluster([node]), creator


def leg(cluster, creator, n, sampled_rows, seed):
    """-> [(ms per step, host ms per step, cohort steps)] per window"""
    from hydrainfer_amd.engine.serve import quiet_gc, synthetic_requests
    dev = build.models[4]
    fill = cluster.nodes[0].executor.fill_executor
    dec = fill.graph_decoder
    reqs = synthetic_requests(n, N_TEXT, WARM + STEPS * WINDOWS + 8, IMAGE_TOKEN_ID, None, seed=seed)
    for i in sampled_rows:
        for k, v in SAMPLED.items():
            setattr(reqs[i].sampling_params, k, v)
        reqs[i].sampling_params.seed = 1000 + i
    waited = [0.0]
    real_fetch = dec.fetch

    def fetch(launch):
        t = time.perf_counter()
        try:
            return real_fetch(launch)
        finally:
            waited[0] += time.perf_counter() - t
    dec.fetch = fetch
    out = []
    try:
        with quiet_gc():
            rcbs = [creator.process(r) for r in reqs]
            for r in rcbs:
                cluster.add_request(r)
            while any(not r.output_token_ids for r in rcbs):            # the prefill steps
                cluster.step()
            for _ in range(WARM):                # (a step is a token per request; the cohort keeps its tokens to itself
                cluster.step()                   # until it ends, so the requests' lists cannot be asked)
            for _ in range(WINDOWS):
                torch.cuda.synchronize(dev)
                waited[0], in_step, cohort0 = 0.0, 0.0, fill.n_cohort_steps
                t0 = time.perf_counter()
                for _ in range(STEPS):
                    t = time.perf_counter()
                    cluster.step()
                    in_step += time.perf_counter() - t
                torch.cuda.synchronize(dev)
                wall = time.perf_counter() - t0
                out.append((wall / STEPS * 1e3, (in_step - waited[0]) / STEPS * 1e3, fill.n_cohort_steps - cohort0))
            while not cluster.idle():
                cluster.step()
        torch.cuda.synchronize(dev)
    finally:
        dec.fetch = real_fetch
    assert all(len(r.output_token_ids) == r.sampling_params.max_tokens for r in rcbs)
    return out


def measure():
    import dataclasses
    from hydrainfer_amd.engine.serve import build_node
    from hydrainfer_amd.model.clip import CLIP_VIT_L_14_336, LlavaVisionModel
    from hydrainfer_amd.model.llama import LLAVA_1_5_7B, LlamaForCausalLM
    from hydrainfer_amd.model.llava import LlavaLanguageModel
    dev, dtype, shape = torch.device("cuda:0"), torch.bfloat16, LLAVA_1_5_7B
    torch.cuda.set_device(dev)
    lm = LlavaLanguageModel(LlamaForCausalLM.random_init(shape, dtype, dev, seed=0), image_token_id=IMAGE_TOKEN_ID)
    vision = LlavaVisionModel.random_init(dataclasses.replace(CLIP_VIT_L_14_336, projector_hidden_size=shape.hidden_size),
                                          dtype, dev, seed=1)
    build.models = (lm, vision, shape, dtype, dev)
    has_switch = "graph_sampling" in inspect.signature(build_node).parameters
    engines = {"off": build(False, 64)}
    if has_switch:
        engines["on"] = build(True, 64)
    plan = []                                   # (leg name, engine, rows, sampled rows)
    for n in (32, 64):
        plan.append((f"(a) all greedy, graph, {n} rows", "off", n, []))
        for what, rows in (("all sampled", list(range(n))), (f"1 sampled + {n - 1} greedy", [n // 2])):
            plan.append((f"(b) {what}, switch off, {n} rows", "off", n, rows))
            if has_switch:
                plan.append((f"(c) {what}, switch on, {n} rows", "on", n, rows))
    for name, engine, n, rows in plan:          # one short pass that is not kept: code objects, allocator, workspaces
        leg(*engines[engine], n, rows, seed=7)
    results = {name: [] for name, *_ in plan}
    for p in range(PASSES):
        for j, (name, engine, n, rows) in enumerate(plan):
            results[name] += leg(*engines[engine], n, rows, seed=100 + 10 * p + j)
    return {"has_switch": has_switch, "device": torch.cuda.get_device_name(dev), "legs": results,
            "settings": dict(warm=WARM, steps=STEPS, windows=WINDOWS, passes=PASSES, n_text=N_TEXT, **SAMPLED)}


def spread(values):
    return f"{statistics.median(values):.3f} ({min(values):.3f}-{max(values):.3f})"


def report(mine, baseline):
    s = mine["settings"]
    lines = ["# Sampled decoding from the captured decode step: engine step times",
             "",
             f"`tools/bench_graph_sampling.py` on one {mine['device']}: LLaVA-1.5-7B-shaped random weights, bf16, text-only "
             f"requests ({s['n_text']} prompt tokens) decoding together; sampled rows T = {s['temperature']}, top_k = "
             f"{s['top_k']}, top_p = {s['top_p']}.  Per leg {s['passes']} x {s['windows']} windows of {s['steps']} engine steps, "
             f"taken after {s['warm']} decode steps; the legs alternate pass by pass.  Median (min-max) over "
             "the windows.  `ms/step`: wall time of a window over its steps, the device synchronised at both ends.  `host "
             "ms/step`: time inside `cluster.step()` minus the wait for an earlier launch's tokens inside "
             "`GraphedDecoder.fetch`; an eager step ends in a blocking read of its own tokens, so its host time is the step "
             "itself.  `cohort`: the share of the windows' steps that were cohort steps.",
             "",
             "| leg | ms/step | host ms/step | cohort |",
             "|---|---|---|---|"]

    def rows(data, tag):
        for name, windows in data["legs"].items():
            share = sum(w[2] for w in windows) / (len(windows) * data["settings"]["steps"])
            lines.append(f"| {name}{tag} | {spread([w[0] for w in windows])} | {spread([w[1] for w in windows])} | {share:.2f} |")
    rows(mine, "")
    if baseline is not None:
        lines += ["", "The same script on a checkout of the parent commit (no switch: legs (a) and (b) only), run back to back with it on "
                  "the same GPU — the baseline for leg (b):", "",
                  "| leg | ms/step | host ms/step | cohort |", "|---|---|---|---|"]
        at = len(lines)
        rows(baseline, ", parent")
        assert len(lines) > at
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="write the raw windows here")
    ap.add_argument("--baseline", default=None, help="the --json file of a run on the parent checkout")
    ap.add_argument("--out", default=None, help="write the report here (default: print it)")
    args = ap.parse_args()
    mine = measure()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(mine, f)
    baseline = None
    if args.baseline:
        with open(args.baseline) as f:
            baseline = json.load(f)
    text = report(mine, baseline)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
