"""What penalised decoding costs per decode step of the engine, from the captured step and from the eager path.
    python tools/bench_graph_penalties.py [--json OUT.json] [--baseline PARENT.json] [--isa-diff FILE] [--out profiles/graph_penalties.md]

One MI355X, LLaVA-1.5-7B-shaped random weights, bf16, text-only requests that all decode together; 32 and 64 rows;
penalised rows are greedy with (frequency, presence, repetition) = (0.5, 0.3, 1.1), sampled rows T = 0.7, top_k = 50,
top_p = 0.9.  Legs:
  (a) an all-greedy batch (captured step, look-ahead, cohort);
  (b) an all-penalised batch, and one penalised row among greedy ones, with the graph_penalties switch off (eager steps);
  (c) the same two batches with the switch on;
  (d) an all-sampled batch without penalties from the graph (the graph_sampling switch; here: graph_penalties, which
      implies it) — the sampled variant is to stand where it stood.
A checkout that has no graph_penalties switch (the parent of the change that added it) runs (a), (b) and (d): give its
--json file as --baseline and its legs stand beside this checkout's in the report.  The windows, the host time and the
cohort share are tools/bench_graph_sampling.py's (read its docstring), whose `spread` this report uses.

Then the launch alone, 64 rows x 32064, bf16, in the manner of tools/bench_sampling.py (bursts between device events,
the variants alternating): hx_sample_rows_resident against hx_sample_rows_resident_penalized with no row holding a slot
and with every row at L = 16, 256 and 1024 log entries (a pool of 64 distinct tokens: repeats and distinct ones).
--isa-diff: the output of `python tools/isa_diff.py <parent sampling.o> <this sampling.o>`, quoted in the report."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_graph_sampling import IMAGE_TOKEN_ID, N_TEXT, PASSES, SAMPLED, STEPS, WARM, WINDOWS, spread      # noqa: E402
from bench_penalties import measure as measure_launches                                                    # noqa: E402

PENALISED = dict(frequency_penalty=0.5, presence_penalty=0.3, repetition_penalty=1.1)
N, KERNEL_ROWS, LOG_LENGTHS = 32064, 64, (16, 256, 1024)


def build(models, max_running, **switches):
    from hydrainfer_amd.engine.node import LocalCluster
    from hydrainfer_amd.engine.request_processor import InstructionCreator
    from hydrainfer_amd.engine.scheduler import BatchSchedulerConfig
    from hydrainfer_amd.engine.serve import build_node
    lm, vision, shape, dtype, dev = models
    per_req = (N_TEXT + WARM + STEPS * WINDOWS + 16 + 15) // 16 + 1
    sched = BatchSchedulerConfig(priority="prefill", max_running_requests=max_running, chunked_prefill=True,
                                 token_budgets=2048, image_budgets=8)
    node = build_node("EPD0", "EPD", lm, vision, shape, dtype, dev, per_req * (max_running + 2), 2, 576, sched,
                      max_blocks_per_seq=per_req, **switches)
    node.executor.fill_executor.graph_decoder.warmup([32, 64], kv_max=256)
    creator = InstructionCreator(image_token_id=IMAGE_TOKEN_ID, n_image_tokens_per_image=576, block_size=16, ignore_eos=True)
    return LocalCluster([node]), creator


def leg(dev, cluster, creator, n, fields, rows, seed):
    """`rows` of the n requests get `fields` set on their sampling parameters -> [(ms per step, host ms per step, cohort
    steps)] per window (tools/bench_graph_sampling.py::leg, with the fields as an argument)"""
    from hydrainfer_amd.engine.serve import quiet_gc, synthetic_requests
    fill = cluster.nodes[0].executor.fill_executor
    dec = fill.graph_decoder
    reqs = synthetic_requests(n, N_TEXT, WARM + STEPS * WINDOWS + 8, IMAGE_TOKEN_ID, None, seed=seed)
    for i in rows:
        for k, v in fields.items():
            setattr(reqs[i].sampling_params, k, v)
        if "temperature" in fields:
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
            while any(not r.output_token_ids for r in rcbs):
                cluster.step()
            for _ in range(WARM):
                cluster.step()
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


def launch_times(reps=30, burst=20):
    """-> {variant: [us per launch]} or None on a checkout without the new entry"""
    from hydrainfer_amd import sampling
    if not hasattr(sampling, "sample_rows_resident_penalized"):
        return None
    rows = KERNEL_ROWS
    g = torch.Generator().manual_seed(1)
    logits = (3.0 * torch.randn((rows, N), generator=g)).to(torch.bfloat16).cuda()
    out = torch.empty(rows, dtype=torch.int64, device="cuda")
    pos = torch.full((rows,), 5, dtype=torch.int32, device="cuda")
    log = torch.zeros(2 * rows, 1024 + 8, dtype=torch.int32)
    pool = torch.randint(0, N, (rows, 64), generator=g)
    log[:rows] = pool.gather(1, torch.randint(0, 64, (rows, 1024 + 8), generator=g)).int()
    log = log.cuda()
    variants = []

    def records(L):
        return torch.from_numpy(sampling.pack_resident_records([(0.7, 0.9, 50, 1000 + r, L - 5) for r in range(rows)])).cuda()
    rec0 = records(3)
    variants.append(("hx_sample_rows_resident", lambda: sampling.sample_rows_resident(logits, rec0, pos, out=out)))
    none = torch.from_numpy(sampling.pack_penalty_records([None] * rows)).cuda()
    variants.append(("hx_sample_rows_resident_penalized, no row with a slot",
                     lambda: sampling.sample_rows_resident_penalized(logits, rec0, pos, none, log, out=out)))
    slots = torch.from_numpy(sampling.pack_penalty_records([(0.5, 0.3, 1.1, r) for r in range(rows)])).cuda()
    for L in LOG_LENGTHS:
        variants.append((f"hx_sample_rows_resident_penalized, every row at L = {L}",
                         lambda rec=records(L): sampling.sample_rows_resident_penalized(logits, rec, pos, slots, log, out=out)))
    return measure_launches(variants, reps, burst)


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
    models = (lm, vision, shape, dtype, dev)
    has_switch = "graph_penalties" in inspect.signature(build_node).parameters
    engines = {"off": build(models, 64)}
    engines["on"] = build(models, 64, graph_penalties=True) if has_switch else build(models, 64, graph_sampling=True)
    plan = []                                   # (leg name, engine, rows, fields, the rows that get them)
    for n in (32, 64):
        plan.append((f"(a) all greedy, graph, {n} rows", "off", n, {}, []))
        for what, rows in (("all penalised", list(range(n))), (f"1 penalised + {n - 1} greedy", [n // 2])):
            plan.append((f"(b) {what}, switch off, {n} rows", "off", n, PENALISED, rows))
            if has_switch:
                plan.append((f"(c) {what}, switch on, {n} rows", "on", n, PENALISED, rows))
        plan.append((f"(d) all sampled, from the graph, {n} rows", "on", n, SAMPLED, list(range(n))))
    for name, engine, n, fields, rows in plan:  # one short pass that is not kept: code objects, allocator, workspaces
        leg(dev, *engines[engine], n, fields, rows, seed=7)
    results = {name: [] for name, *_ in plan}
    for p in range(PASSES):
        for j, (name, engine, n, fields, rows) in enumerate(plan):
            results[name] += leg(dev, *engines[engine], n, fields, rows, seed=100 + 10 * p + j)
    seeds = engines["on"][0].nodes[0].executor.fill_executor.graph_decoder
    return {"has_switch": has_switch, "device": torch.cuda.get_device_name(dev), "legs": results, "launches": launch_times(),
            "n_seeds": seeds.log_table.n_seeds if has_switch else None,
            "settings": dict(warm=WARM, steps=STEPS, windows=WINDOWS, passes=PASSES, n_text=N_TEXT, **SAMPLED, **PENALISED)}


def report(mine, baseline, isa_diff):
    s = mine["settings"]
    lines = ["# Penalties from the captured decode step: engine step times",
             "",
             f"`tools/bench_graph_penalties.py` on one {mine['device']}: LLaVA-1.5-7B-shaped random weights, bf16, text-only "
             f"requests ({s['n_text']} prompt tokens) decoding together; penalised rows greedy with (frequency, presence, "
             f"repetition) = ({s['frequency_penalty']}, {s['presence_penalty']}, {s['repetition_penalty']}); sampled rows T = "
             f"{s['temperature']}, top_k = {s['top_k']}, top_p = {s['top_p']}.  Per leg {s['passes']} x {s['windows']} windows of "
             f"{s['steps']} engine steps, taken after {s['warm']} decode steps; the legs alternate pass by pass.  Median "
             "(min-max) over the windows; the columns are those of `profiles/graph_sampling.md`.",
             "",
             "| leg | ms/step | host ms/step | cohort |",
             "|---|---|---|---|"]

    def rows(data, tag):
        for name, windows in data["legs"].items():
            share = sum(w[2] for w in windows) / (len(windows) * data["settings"]["steps"])
            lines.append(f"| {name}{tag} | {spread([w[0] for w in windows])} | {spread([w[1] for w in windows])} | {share:.2f} |")
    rows(mine, "")
    med = lambda data, name: statistics.median(w[0] for w in data["legs"][name])      # noqa: E731
    if mine["has_switch"]:
        lines += ["", "(c) - (a), medians: " + "; ".join(
            f"{n} rows: all penalised {med(mine, f'(c) all penalised, switch on, {n} rows') - med(mine, f'(a) all greedy, graph, {n} rows'):+.3f} ms, "
            f"1 penalised {med(mine, f'(c) 1 penalised + {n - 1} greedy, switch on, {n} rows') - med(mine, f'(a) all greedy, graph, {n} rows'):+.3f} ms"
            for n in (32, 64)) + f".  Log seeds over the whole run: {mine['n_seeds']} (one per penalised request on its first decode "
            "step; a continuing request uploads nothing)."]
    if baseline is not None:
        lines += ["", "The same script on a checkout of the parent commit (no graph_penalties switch: legs (a), (b) and (d), the "
                  "last under graph_sampling), run back to back with it on the same GPU:", "",
                  "| leg | ms/step | host ms/step | cohort |", "|---|---|---|---|"]
        rows(baseline, ", parent")
        lines += ["", "Window by window, (c) on this tree against (b) on the parent (the windows in the order they were taken):", ""]
        for name in mine["legs"]:
            if name.startswith("(c)"):
                b = baseline["legs"][name.replace("(c)", "(b)").replace("switch on", "switch off")]
                pairs = [(c[0], p[0]) for c, p in zip(mine["legs"][name], b)]
                lines.append(f"- {name}: " + ", ".join(f"{c:.3f} < {p:.3f}" if c < p else f"**{c:.3f} >= {p:.3f}**" for c, p in pairs))
    if mine.get("launches"):
        lines += ["", f"## The launch alone: microseconds, {KERNEL_ROWS} rows x {N}, bf16, T = 0.7, top_k = 50, top_p = 0.9", "",
                  "| variant | median | q1 | q3 |", "|---|---|---|---|"]
        for name, times in mine["launches"].items():
            q = statistics.quantiles(times, n=4)
            lines.append(f"| {name} | {statistics.median(times):.1f} | {q[0]:.1f} | {q[2]:.1f} |")
    if isa_diff:
        lines += ["", "## The older sampling kernels' device code", "",
                  "`python tools/isa_diff.py <parent sampling.o> <this sampling.o>`:", "", "```", isa_diff.strip(), "```"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="write the raw windows here")
    ap.add_argument("--baseline", default=None, help="the --json file of a run on the parent checkout")
    ap.add_argument("--isa-diff", default=None, help="a file holding tools/isa_diff.py's output for sampling.o")
    ap.add_argument("--out", default=None, help="write the report here (default: print it)")
    args = ap.parse_args()
    mine = measure()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(mine, f)
    baseline = isa = None
    if args.baseline:
        with open(args.baseline) as f:
            baseline = json.load(f)
    if args.isa_diff:
        with open(args.isa_diff) as f:
            isa = f.read()
    text = report(mine, baseline, isa)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
