#!/usr/bin/env python3
"""bench.py — headline benchmark of the hot path (BASELINE.json:metric).

A "step" = one batched decode step of a LLaVA-1.5-7B-shaped language model (random weights,
SURVEY.md §8d) for 32 concurrent requests (576 image + 128 text prompt tokens each) on ONE
MI355X: embed -> 32 x [qkv GEMM, (RoPE + set_kv_cache + paged decode attention), o GEMM,
(residual add + rms_norm), gate|up GEMM, silu*mul, down GEMM, (residual add + rms_norm)]
-> lm_head -> argmax.  Every per-layer launch is libhydra_hip (decode GEMMs: the
weight-streaming HIP kernel; --lib-gemm switches them to hipBLASLt); prefill GEMMs and lm_head
are library GEMMs.  The KV
context starts at the prompt (704 cached tokens) and ends at 959 as in a real 256-token
generation: K=255 steps walk contexts 705..959 one by one; a shorter run (K < 255) takes K
contexts evenly spaced over the same 705..959 (`timed_contexts`), so that `value` is the rate of
the workload the metric names whatever --steps is.  Inputs (weights, KV cache, metadata) are
resident in HBM before the timed region.

python bench.py [--gpus N --steps K --warmup W]
N>1 without WORLD_SIZE in the environment: this process starts N ranks itself (fresh child
processes through torch.distributed.run, before anything here touches a GPU) and exits with their
code; under torch.distributed.run (WORLD_SIZE set) --gpus must equal WORLD_SIZE.
Prints ONE JSON line on rank 0."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=255)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", default="7b", choices=["7b", "13b", "tiny"])
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--executor", default=os.environ.get("HX_DECODE_EXECUTOR", "plan"), choices=["graph", "plan"],
                   help="replay of the decode step: one captured hipGraph, or a launch plan (the same launches in stream "
                        "order, issued by a native loop: hydrainfer_amd/launch_plan.py)")
    p.add_argument("--skip-prefill", action="store_true",
                   help="decode against the randn-filled cache instead of a real prefill")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-ttft", action="store_true")
    p.add_argument("--no-serving", action="store_true", help="skip the continuous-batching engine leg")
    p.add_argument("--no-serving-64", action="store_true",
                   help="skip the second engine leg with 2 x --batch requests (decode batches past the 32-row fast path)")
    p.add_argument("--no-disaggregated", action="store_true", help="N>1: skip the E/P/D engine leg")
    p.add_argument("--rate", type=float, default=6.0,
                   help="N>1, E/P/D leg: offered load in requests/s PER D RANK of the Poisson trace (BASELINE configs[4]: "
                        "benchmark/synthetic_dataset.py requests with benchmark/timestamp.py arrivals); 0 = only the burst at t=0")
    p.add_argument("--no-migration", action="store_true")
    p.add_argument("--lib-gemm", action="store_true",
                   help="library GEMMs (hipBLASLt) for decode too, instead of the weight-streaming HIP kernel")
    p.add_argument("--no-fused-attention", action="store_true")
    p.add_argument("--cpu-layers", type=int, default=2)
    p.add_argument("--cpu-full", action="store_true",
                   help="also run BASELINE configs[0] IN FULL on the host cores (all decoder + CLIP layers of the oracle, ~1 min "
                        "incl. building 13 GB of weights): cpu_baseline.config0_full and full_over_extrapolated")
    p.add_argument("--no-13b", action="store_true", help="skip the short LLaVA-1.5-13B leg (BASELINE configs[2])")
    p.add_argument("--no-tune", action="store_true",
                   help="skip the start-up autotuning of the library's prefill GEMMs in front of the TTFT / serving legs (serve.tune_library_gemms)")
    p.add_argument("--steps-13b", type=int, default=20)
    p.add_argument("--leg-13b-in-process", action="store_true",
                   help="run the 13B leg inside this process behind the 7B legs instead of in a fresh child process")
    p.add_argument("--as-13b-leg", action="store_true", help=argparse.SUPPRESS)      # set by leg_13b_child only
    p.add_argument("--no-ranked", action="store_true",
                   help="decode attention on the static (head, sequence) grid instead of the length-ranked one (A/B; attn_decode.hip)")
    p.add_argument("--no-ragged", action="store_true", help="skip whole_step_ragged (the decode step on ragged batches)")
    p.add_argument("--no-null-step", action="store_true",
                   help="skip whole_step.null_step (the launch structure's ceiling: the step with math-free stand-in launches)")
    p.add_argument("--dry-run", action="store_true",
                   help="launch plumbing only (ranks, rendezvous, barrier, max-over-ranks timing of empty steps): "
                        "no GPU is touched; the JSON line says dry_run")
    p.add_argument("--full", action="store_true",
                   help="everything beyond the headline: stream ceilings, prefill batch time, TTFT, serving legs, roofline / "
                        "null-step / ragged / 64-row objects, prefill attention, CPU baseline + parity probe, the 13B leg, "
                        "multi-GPU migration and E/P/D legs, and the headline as the median of several timed regions.  "
                        "Without it a run sets up, warms up, times --steps steps once and prints the line")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")
    if not args.full:      # a plain run: nothing but the headline
        for flag in ("no_cpu_baseline", "no_ttft", "no_serving", "no_serving_64", "no_disaggregated", "no_migration",
                     "no_13b", "no_tune", "no_ragged", "no_null_step"):
            setattr(args, flag, True)
    return args


def launch_ranks_if_needed(args):
    """`python bench.py --gpus N` must run N ranks (hydrainfer/cluster/cluster.py:63-79 starts one node
    per GPU).  Without WORLD_SIZE this process is the launcher: N fresh children via
    torch.distributed.run, started before this process makes any GPU call (a process that has
    initialised the GPU must never exec another program; children are spawned, not exec'd), and the
    launcher exits with their return code.  With WORLD_SIZE set the two must agree."""
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is not None:
        if int(env_world) != args.gpus:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={env_world}: refusing to report a line for a "
                  f"different rank count", file=sys.stderr, flush=True)
            sys.exit(2)
        return
    if args.gpus <= 1:
        return
    with socket.socket() as so:      # a free rendezvous port on the loopback
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


def timed_contexts(prompt_len, n_generate, steps):
    """KV lengths of the timed steps.  The generation's decode steps see contexts prompt_len+1 ..
    prompt_len+n_generate-1 (705..959); fewer steps than that sample the same range at a FIXED spacing, centred,
    so that their mean is the generation's mean context (832) and the step's own device-side advance
    (hx_decode_advance with that stride) walks them — no extra launch in the timed region."""
    lo, hi = prompt_len + 1, prompt_len + n_generate - 1
    if steps >= hi - lo + 1:
        return list(range(lo, hi + 1))
    if steps == 1:
        return [(lo + hi) // 2]
    stride = (hi - lo) // (steps - 1)
    first = lo + ((hi - lo) - stride * (steps - 1)) // 2
    return [first + k * stride for k in range(steps)]


def timed_passes(prompt_len, n_generate, steps):
    """The contexts of exactly `steps` timed decode steps, as passes over the generation (the decode state is rewound to
    the pass's first context in front of each).  Up to the generation's 255 decode steps: one pass, `timed_contexts`.
    More: whole passes over 705..959 and a last pass of the remaining steps at consecutive contexts, centred in the same
    range — every pass has stride 1, so one captured step serves them all."""
    lo, hi = prompt_len + 1, prompt_len + n_generate - 1
    n = hi - lo + 1
    if steps <= n:
        return [timed_contexts(prompt_len, n_generate, steps)]
    passes = [list(range(lo, hi + 1))] * (steps // n)
    if steps % n:
        first = lo + (n - steps % n) // 2
        passes.append(list(range(first, first + steps % n)))
    return passes


def dry_run(args):
    """Everything of the N-rank contract except the GPU work: rendezvous (gloo), barrier, K empty
    steps, MAX over ranks, one JSON line on rank 0."""
    from hydrainfer_amd import parallel
    ctx = parallel.init_from_env(backend="gloo")
    ctx.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    elapsed = ctx.max_over_ranks(time.perf_counter() - t0)
    ctx.barrier()
    if ctx.rank == 0:
        print(json.dumps({"metric": "dry run (no GPU work)", "dry_run": True, "value": 0.0, "unit": "tokens/s",
                          "n_gpus": ctx.world_size, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": elapsed / max(args.steps, 1) * 1e3,
                          "roles": parallel.epd_roles(ctx.world_size)}), flush=True)
    ctx.shutdown()


def model_shape(name):
    from hydrainfer_amd.model.llama import LLAVA_1_5_13B, LLAVA_1_5_7B, LlamaShape
    if name == "7b":
        return LLAVA_1_5_7B, "LLaVA-1.5-7B"
    if name == "13b":
        return LLAVA_1_5_13B, "LLaVA-1.5-13B"
    return LlamaShape(512, 1024, 2, 4, 4, 128, 2048), "tiny"


def synth_prompts(batch, prompt_len, vocab, device):
    """576 x image_token_id followed by random text ids, distinct seed per request (§8d)."""
    rows = []
    for r in range(batch):
        g = torch.Generator().manual_seed(r)
        text = torch.randint(1000, min(31999, vocab - 1), (prompt_len - 576,), generator=g)
        rows.append(torch.cat([torch.full((576,), image_token_id(vocab)), text]))
    return torch.stack(rows).to(device)


def image_token_id(vocab):
    return 32000 if vocab > 32000 else vocab - 1


def copy_ceiling_gbs(dev, nbytes=1 << 30, reps=5):
    """Measured streaming-copy rate of this GPU in this run (read + write bytes / time): the
    practical HBM ceiling SURVEY.md §8(d) asks to be reported beside the 8 TB/s vendor peak."""
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(reps):
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize(dev)
        best = min(best, e0.elapsed_time(e1))
    del src, dst
    return 2 * nbytes / (best * 1e-3) / 1e9


def read_stream_ceiling_gbs(dev, nbytes=1 << 30, reps=7):
    """Measured READ-streaming rate of this GPU in this run: 1 GiB read once per launch by the library's own probe
    (hx_measure_read_stream: the access shape of the weight-streaming kernels, no arithmetic), median of `reps`
    launches under HIP events on the launch stream.  The decode step is >99 % reads, so this — not a copy — is the
    practical ceiling its kernels can be held against."""
    import statistics
    from hydrainfer_amd import _lib
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    buf.random_(0, 255)
    sink = torch.zeros(4, dtype=torch.float32, device=dev)
    lib = _lib.lib()
    ts = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.hx_measure_read_stream(buf.data_ptr(), nbytes, sink.data_ptr(), _lib.current_stream()), "read_stream")
        e1.record()
        torch.cuda.synchronize(dev)
        ts.append(e0.elapsed_time(e1))
    del buf
    return nbytes / (statistics.median(ts[1:]) * 1e-3) / 1e9


def time_attention_kernel(runner, ctxs):
    """Average duration of the decode-attention launch (the variant the decode graph runs:
    fused RoPE + cache append + attention) over the same context sequence `ctxs` (KV lengths) as
    the timed region, HIP events on the launch stream (torch's current stream).  MEAN over
    launches and replays, not the best one."""
    import math
    from hydrainfer_amd._C.kernel.flash_attn import decode_attention_fused, decode_rank, mha_varlen_fwd
    sh = runner.model.shape
    B = runner.cfg.batch
    H, HK, D = sh.num_attention_heads, sh.num_key_value_heads, sh.head_dim
    g = torch.Generator(device=runner.dev).manual_seed(5)
    rnd = lambda *s: torch.randn(s, device=runner.dev, generator=g).to(runner.model.dtype)
    q, k_new, v_new = rnd(B, H, D), rnd(B, HK, D), rnd(B, HK, D)
    out = torch.empty_like(q)
    ap = runner.decode_params.attention_params[0]
    kc, vc = ap.kv_cache.get_kv_cache()
    # launch i reads the cache of layer i mod L, like the decode step: a replay over ONE layer's
    # cache (375-437 MB) could be flattered by the 256 MiB Infinity Cache
    layer_caches = [p_.kv_cache.get_kv_cache() for p_ in runner.decode_params.attention_params]
    saved = (runner.positions.clone(), runner.kv_lens.clone())
    evs = []
    scale = 1.0 / math.sqrt(D)
    fused = runner.model.fuse_decode_attention
    # with the HIP decode GEMMs the graph runs the variant that also reduces the qkv split-K slabs
    slabs, n_slabs = None, 0
    if fused and runner.model.use_hip_gemm and B <= 64:
        from hydrainfer_amd._C.kernel import gemm as hip_gemm
        x = rnd(B, sh.hidden_size)
        slabs = torch.empty(hip_gemm.workspace_floats(B, (H + 2 * HK) * D, sh.hidden_size),
                            dtype=torch.float32, device=runner.dev)
        n_slabs = hip_gemm.linear_decode_partial(x, runner.model.state["l0.wqkv"], slabs)
    def launch():
        if fused:
            decode_attention_fused(out, q, k_new, v_new, kc, vc, runner.positions, runner.model.cos_sin,
                                   ap.new_cache_slots, ap.q_cu_seq_lens, ap.kv_cu_seq_lens,
                                   ap.block_tables, ap.cu_blocks_lens, runner.max_len, scale, 0, slabs, n_slabs, ap.decode_rank)
        else:
            mha_varlen_fwd(out, q, kc, vc, ap.q_cu_seq_lens, ap.kv_cu_seq_lens, ap.block_tables,
                           ap.cu_blocks_lens, None, 1, runner.max_len, scale, 0.0, -1, 0, 0)

    steps = len(ctxs)
    if runner.cfg.use_graph:
        # Issued from Python one by one, a launch that is shorter than the host's ~40 us per call
        # would be timed with the host's gaps in it.  So the launches of the whole context sequence
        # are captured back to back into one graph — each with its own precomputed metadata
        # (positions, slots, cumulative lengths of that step), no other kernel in between — and the
        # replay is timed with HIP events: kernel + dispatch gap, as inside the decode step.
        bs = runner.cfg.block_size
        i32 = dict(dtype=torch.int32, device=runner.dev)
        metas = []
        for ctx_len in ctxs:       # an int (every sequence at that length) or one length per sequence (a ragged batch)
            lens = [ctx_len] * B if isinstance(ctx_len, int) else list(ctx_len)
            cu = [0]
            for l_ in lens:
                cu.append(cu[-1] + l_)
            cu_t = torch.tensor(cu, **i32)
            metas.append((torch.tensor([l_ - 1 for l_ in lens], **i32),
                          torch.tensor([runner.tables[b][(lens[b] - 1) // bs] * bs + (lens[b] - 1) % bs for b in range(B)], **i32),
                          cu_t, decode_rank(cu_t)))      # (the step's rank descriptor, as its step head would leave it)

        def launch_step(m, i=0):
            kc, vc = layer_caches[i % len(layer_caches)]
            if fused:
                decode_attention_fused(out, q, k_new, v_new, kc, vc, m[0], runner.model.cos_sin, m[1],
                                       ap.q_cu_seq_lens, m[2], ap.block_tables, ap.cu_blocks_lens,
                                       runner.max_len, scale, 0, slabs, n_slabs, m[3])
            else:
                mha_varlen_fwd(out, q, kc, vc, ap.q_cu_seq_lens, m[2], ap.block_tables, ap.cu_blocks_lens, None, 1,
                               runner.max_len, scale, 0.0, -1, 0, 0)
        launch_step(metas[0]); torch.cuda.synchronize()      # warm outside capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i, m in enumerate(metas):
                launch_step(m, i)
        graph.replay(); torch.cuda.synchronize()             # one untimed replay
        total, reps = 0.0, 3
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            e1.synchronize()
            total += e0.elapsed_time(e1)
        ms = total / reps / steps
    else:
        for s in range(steps + 2):
            c_ = ctxs[max(s - 2, 0)]
            if isinstance(c_, int):
                runner.set_state(c_ - runner.cfg.advance_stride)
            else:
                runner.set_state_lens([l_ - runner.cfg.advance_stride for l_ in c_])
            runner._advance()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            if s >= 2:
                evs.append((e0, e1))
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in evs) / len(evs)
    runner.positions.copy_(saved[0]); runner.kv_lens.copy_(saved[1])
    return ms


def make_vision(shape, dtype, dev):
    """CLIP ViT-L/14-336 + projector with random weights, and the reference's synthetic image
    (hydrainfer/utils/image_utils.py:4-7) after CLIP preprocessing."""
    from hydrainfer_amd.model.clip import CLIP_VIT_L_14_336, ClipShape, LlavaVisionModel
    import dataclasses
    import numpy as np
    if shape.hidden_size < 1024:     # tiny smoke configuration
        cshape = ClipShape(hidden_size=128, intermediate_size=256, num_hidden_layers=3,
                           num_attention_heads=2, image_size=336, patch_size=14,
                           projector_hidden_size=shape.hidden_size)
    else:
        cshape = dataclasses.replace(CLIP_VIT_L_14_336, projector_hidden_size=shape.hidden_size)
    vision = LlavaVisionModel.random_init(cshape, dtype, dev, seed=1)
    from PIL import Image
    from hydrainfer_amd.model.processor import ClipImageProcessor
    rng = np.random.RandomState(0)
    image = Image.fromarray(rng.randint(0, 256, (336, 336, 3), dtype=np.uint8))
    pixels = ClipImageProcessor().process(image)
    return vision, pixels


def measure_serving(model, vision, pixels, shape, dtype, dev, batch, n_text, max_tokens):
    """The whole serving path on this GPU (BASELINE configs[1]/[2]): `batch` image+text requests
    admitted together to the continuous-batching engine (hydrainfer_amd/engine: scheduler with
    chunked prefill, CLIP encode -> image cache -> prefill -> decode steps replayed from hipGraphs
    with one step of look-ahead), until every request has its max_tokens."""
    from hydrainfer_amd.engine.node import LocalCluster
    from hydrainfer_amd.engine.request_processor import InstructionCreator
    from hydrainfer_amd.engine.scheduler import BatchSchedulerConfig
    from hydrainfer_amd.engine.serve import build_node, replay, synthetic_requests, warm_library_gemms
    from hydrainfer_amd.model.llava import LlavaLanguageModel
    itid = image_token_id(shape.vocab_size)
    lm = LlavaLanguageModel(model, image_token_id=itid)
    per_req = (576 + n_text + max_tokens + 15) // 16 + 1
    sched = BatchSchedulerConfig(priority="prefill", max_running_requests=batch, chunked_prefill=True,
                                 token_budgets=2048, image_budgets=8)
    node = build_node("EPD0", "EPD", lm, vision, shape, dtype, dev, per_req * (batch + 2), batch + 2, 576, sched,
                      max_blocks_per_seq=per_req)
    node.executor.fill_executor.graph_decoder.warmup(list(range(4, batch + 1, 4)), kv_max=1024)
    node.executor.image_embed_executor.warmup(pixels, sched.image_budgets)
    warm_library_gemms(lm, sched.token_budgets, batch, vision, pixels, sched.image_budgets)
    cluster = LocalCluster([node])
    creator = InstructionCreator(image_token_id=itid, n_image_tokens_per_image=576, block_size=16,
                                 max_position_embeddings=shape.max_position_embeddings)
    text_hi = min(31999, itid - 1)
    # warm-up: the same burst once with 4 generated tokens — every shape the timed burst meets (8-image encodes through
    # the pinned staging buffer, 2048-token chunks that continue a prompt, several requests completing in one chunk) has
    # then been through the allocator and the libraries' lazy loading once, as on a server that has taken traffic before
    # (a 2-request warm-up left sporadic 50-200 ms stalls in the timed burst's first chunks: tools/burst_timeline.py)
    replay(cluster, creator, synthetic_requests(batch, n_text, 4, itid, pixels, (min(1000, text_hi - 1), text_hi), 99),
           [0.0] * batch, dev)
    reqs = synthetic_requests(batch, n_text, max_tokens, itid, pixels, (min(1000, text_hi - 1), text_hi), 1)
    res = replay(cluster, creator, reqs, [0.0] * batch, dev)
    gd = node.executor.fill_executor.graph_decoder
    res["engine_executor"] = gd.executor        # what replays the engine's decode steps: "graph" (hipGraph) or "plan"
    # how many of the engine's decode launches ran as steady-state cohort steps (engine/executor.py::DecodeCohort: no scheduler,
    # no per-request object work — 23 us of host time at 64 rows against 0.39 ms for a general step, tools/prof_engine_host_cpu.py)
    res["decode_launches"], res["decode_cohort_steps"] = gd.launches, node.executor.fill_executor.n_cohort_steps
    # HBM held by all weight layouts once this leg has announced its largest decode batch: batches of 33 .. 64 rows add
    # the LDS-slice copies of the projections the <= 32-row layer runs on the activations-in-registers layout
    res["weight_bytes_resident"] = model.weight_bytes_resident()
    res["what"] = (f"{batch} requests (1 image + {n_text} text tokens, {max_tokens} generated) admitted at t=0 to one "
                   f"collocated EPD engine: continuous batching, chunked prefill (2048-token budget), decode steps "
                   f"replayed by the engine's '{gd.executor}' executor (the headline decode loop replays a launch plan: "
                   "0.5-1 % faster in a GPU-bound loop, 0.65 ms of host time per step that the engine's one thread does "
                   "not have — engine/graph_decode.py)")
    return res


def build_rank_engine(ctx, model, vision, shape, dtype, dev, batch, n_text, max_tokens):
    """This rank's E / P / D node (parallel.epd_roles) with its own cache pools, for the
    disaggregated leg.  Pools are created (and, by the caller, IPC-mapped by their peers) before
    any hipGraph exists."""
    import torch.distributed as dist
    from hydrainfer_amd import parallel
    from hydrainfer_amd.engine.distributed import RankEngine
    from hydrainfer_amd.engine.scheduler import BatchSchedulerConfig
    from hydrainfer_amd.engine.serve import build_node
    from hydrainfer_amd.model.llava import LlavaLanguageModel
    roles = parallel.epd_roles(ctx.world_size)
    role = roles[ctx.rank]
    n_d = sum("D" in r for r in roles)
    n_p = sum("P" in r for r in roles)
    per_req = (576 + n_text + max_tokens + 15) // 16 + 1
    # a P node keeps a prefilled request's blocks until a D node has pulled them
    live = batch + 2 if "D" in role else (batch * n_d + n_p - 1) // n_p + 2
    sched = BatchSchedulerConfig(priority="prefill", max_running_requests=batch, chunked_prefill=True,
                                 token_budgets=2048, image_budgets=8)
    lm = LlavaLanguageModel(model, image_token_id=image_token_id(shape.vocab_size))
    node = build_node(f"{role}{ctx.rank}", role, lm, vision, shape, dtype, dev, per_req * live, 2 * batch + 2, 576,
                      sched, rank=ctx.rank, max_blocks_per_seq=per_req, world_size=ctx.world_size,
                      release_prefill_weights=False)   # the replica leg of the same process prefills on every rank
    group = None if ctx.backend == "gloo" else dist.new_group(backend="gloo")
    engine = RankEngine(ctx.rank, roles, node, group)
    engine.connect_transfer_peers(timeout_s=60)      # send/recv hops only (none with the intra-node IPC pull): bounded
    return engine


def measure_disaggregated(ctx, engine, shape, dev, pixels, batch, n_text, max_tokens, rate_per_d=6.0):
    """BASELINE configs[3]/[4]: one E / P / D node per GPU, requests enter at the E ranks, image
    blocks are pulled E->P and KV blocks P->D over the IPC-mapped peer pools (hx_migrate_blocks),
    control messages over gloo.  Two traces of 32 requests per D rank: a POISSON trace (configs[4]: exponential
    inter-arrival gaps, numpy RandomState seeded like benchmark/benchmark.py:136-137, benchmark/timestamp.py:9-16)
    at rate_per_d x (number of D ranks) requests/s — the headline object — and the burst admitted at t=0
    (`burst_at_t0`: the worst case for TTFT, the best for tokens/s)."""
    import torch.distributed as dist
    from hydrainfer_amd.engine.distributed import replay_distributed, summarize
    from hydrainfer_amd.engine.request_processor import InstructionCreator
    from hydrainfer_amd.engine.serve import poisson_arrivals, synthetic_requests
    torch.cuda.set_device(dev)
    itid = image_token_id(shape.vocab_size)
    roles = engine.roles
    n_d = sum("D" in r for r in roles)
    fe = engine.node.executor.fill_executor
    if fe is not None and fe.graph_decoder is not None:
        fe.graph_decoder.warmup(list(range(4, batch + 1, 4)), kv_max=1024)
    from hydrainfer_amd.engine.serve import warm_library_gemms
    nt = engine.node.node_type
    if fe is not None and nt.enable_prefill:
        warm_library_gemms(fe.language_model, engine.node.batch_scheduler.token_budgets, batch)
    ie = engine.node.executor.image_embed_executor
    if ie is not None:      # the vision tower's graphs for 1 .. image budget images
        ie.warmup(pixels, engine.node.batch_scheduler.image_budgets)
    creator = InstructionCreator(image_token_id=itid, n_image_tokens_per_image=576, block_size=16,
                                 max_position_embeddings=shape.max_position_embeddings)
    hi = min(31999, itid - 1)
    vocab_text = (min(1000, hi - 1), hi)
    kv_bytes = (576 + n_text) * 2 * shape.num_hidden_layers * shape.num_key_value_heads * shape.head_dim * 2

    def run(n, gen, seed, arrivals):
        reqs = synthetic_requests(n, n_text, gen, itid, pixels, vocab_text, seed)
        engine.open_mailbox(f"disagg{seed}")
        box = [time.perf_counter() + 0.2]
        dist.broadcast_object_list(box, src=0, group=engine.group)
        mine = replay_distributed(engine, creator, reqs, arrivals, box[0], dev, deadline_s=150)
        allr = [None] * ctx.world_size
        dist.all_gather_object(allr, mine, group=engine.group)
        merged = {}
        for m in allr:
            merged.update(m)
        res = summarize(merged, box[0])
        if res["pd_pull_p50_ms"]:
            res["pd_pull_GBps"] = round(kv_bytes / res["pd_pull_p50_ms"] / 1e6, 1)
        return res

    n = batch * n_d
    run(2 * len(roles), 4, 99, [0.0] * (2 * len(roles)))                     # warm-up through every hop
    burst = run(n, max_tokens, 1, [0.0] * n)
    burst["what"] = f"{n} requests admitted at t=0"
    if rate_per_d > 0:
        rate = rate_per_d * n_d
        res = run(n, max_tokens, 2, poisson_arrivals(n, rate, seed=0))
        res["arrivals"] = (f"Poisson, {rate:g} requests/s offered ({rate_per_d:g} per D rank), numpy RandomState(0) exponential "
                           "gaps (benchmark/timestamp.py:9-16, seeded as benchmark/benchmark.py:136-137)")
        res["rate_req_s"] = rate
        res["burst_at_t0"] = burst
    else:
        res = burst
        res["arrivals"] = "all at t=0"
    res["kv_bytes_per_request"] = kv_bytes
    res["roles"] = roles
    res["n_ranks"] = len(roles)
    res["what"] = (f"{n} requests (1 image + {n_text} text tokens, {max_tokens} generated); "
                   "one E/P/D engine node per GPU, pulls over IPC-mapped peer pools, control over gloo")
    return res


def measure_ttft(runner, prompts, shape, dtype, dev, rank, vision, pixels, reps=7):
    """p50 time-to-first-token of ONE image+text request on an idle replica: CLIP ViT-L/14-336
    encode (23 layers, dense HIP attention) + projector + 704-token prefill + greedy sample."""
    pixels = pixels.to(dev)
    times, enc_times = [], []
    use_graph = runner.cfg.use_graph and shape.vocab_size > 32000
    if use_graph:
        # both phases replayed from hipGraphs: an idle replica's TTFT is otherwise dominated by
        # the host cost of ~600 eager launches (23 CLIP layers + 32 decoder layers)
        pg, p_ids, p_feats, p_first = runner.capture_prefill(0, image_token_id(shape.vocab_size))
        p_ids.copy_(prompts[0])
        static_pixels = pixels.clone()
        s = torch.cuda.Stream(device=dev); s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            vision(static_pixels)
        torch.cuda.current_stream(dev).wait_stream(s)
        vg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(vg):
            v_out = vision(static_pixels)
    B = runner.cfg.batch
    for i in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if use_graph:
            static_pixels.copy_(pixels)
            vg.replay()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            p_feats.copy_(v_out[0])
            pg.replay()
            p_first[0].item()
        else:
            feats = vision(pixels)                                   # [1, 576, hidden]
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            full = feats.expand(B, -1, -1)
            first = runner.prefill(prompts, full, image_token_id(shape.vocab_size), requests=[0])
            first[0].item()                                          # token reaches the host
        t2 = time.perf_counter()
        if i >= 2:
            times.append((t2 - t0) * 1e3)
            enc_times.append((t1 - t0) * 1e3)
    times.sort(); enc_times.sort()
    return {"p50_ms": round(times[len(times) // 2], 3), "encode_p50_ms": round(enc_times[len(enc_times) // 2], 3),
            "what": "1 request on an idle replica: CLIP ViT-L/14-336 encode + projector + 704-token prefill + "
                    "greedy sample" + (", each phase replayed from a hipGraph" if use_graph else " (eager launches)"),
            "reps": reps}


def measure_migration(ctx, runner, dev, peer, reps=5):
    """P->D KV migration of one 704-token request between neighbouring ranks (rank r pulls from
    r-1) through the IPC-mapped peer pool over xGMI: one gather-copy kernel per transfer."""
    try:
        torch.cuda.set_device(dev)            # runs in a helper thread: the current device is per thread
        from hydrainfer_amd._C.data_transfer import block_migration as bm
        from hydrainfer_amd import parallel
        bs, P = runner.cfg.block_size, runner.cfg.prompt_len
        n_blk = (P + bs - 1) // bs
        # destination: the blocks of local request 1 (rewritten by nothing afterwards)
        dst_table = runner.tables[1][:n_blk]
        nbytes = runner.pool[:, :, :n_blk].numel() * runner.pool.element_size()
        ts = []
        for i in range(reps + 1):
            ctx.barrier(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            bm.migrate_blocks(peer["table"], dst_table, peer["handle"], runner.pool, peer["n_blocks"])
            e1.record(); torch.cuda.synchronize()
            if i >= 1:
                ts.append(e0.elapsed_time(e1))
        ts.sort()
        ms = ctx.max_over_ranks(ts[len(ts) // 2], dev)
        return {"bytes_per_request": int(nbytes), "p50_ms": round(ms, 3),
                "GBps_per_link": round(nbytes / ms / 1e6, 1),
                "what": "all ranks pull one 704-token request's KV (44 blocks x 32 layers x k/v) "
                        "from their ring neighbour concurrently, IPC-mapped peer pool, 1 launch"}
    except Exception as e:   # never let the optional leg break the benchmark line
        return {"error": repr(e)[:300]}


def measured_traffic(args, model_name, algorithmic_bytes):
    """HBM bytes per attention launch.  PMC counters cannot be read from inside the benchmark, so the
    committed PMC pass (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, collected at ctx 832) gives
    the RATIO measured / algorithmic bytes of this kernel, and the figure reported is that ratio
    times the algorithmic bytes of the contexts timed here — reported only for the workload that
    was profiled.  Returns (bytes, description) or (None, None)."""
    for name in ("r5_attn_decode_pmc.json", "r4_attn_decode_pmc.json", "r2_attn_decode_pmc.json", "r1_attn_decode_pmc.json"):
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            break
    else:
        return None, None
    if not (args.model == "7b" and args.batch == 32 and args.dtype == "bf16"):
        return None, None
    try:
        d = json.load(open(path))
        ratio = float(d["traffic_bytes_per_launch"]) / float(d["algorithmic_bytes_per_launch"])
        return int(algorithmic_bytes * ratio), (f"profiles/{name}: PMC traffic / algorithmic bytes = {ratio:.4f} at ctx 832 "
                                                "(incl. the qkv slabs the fused variant reads), applied to the "
                                                "algorithmic bytes of the contexts timed in this run")
    except Exception:
        return None, None


def measured_gemm_traffic(args, model_name, weight_bytes_per_layer):
    """HBM bytes of one layer's four decode GEMM launches from the committed PMC passes (FETCH_SIZE x2 gfx950 correction
    + WRITE_SIZE, separate rocprofv3 --pmc runs): the norm-fused qkv and gate|up+silu launches and the down launch
    from the latest profiles/r*_gemm_xreg_pmc.json, the o launch from profiles/r2_gemm_packed_pmc.json.  Only for the workload
    that was profiled (7B, 32 rows, bf16).  Returns (bytes, source) or (None, None)."""
    if not (args.model == "7b" and args.batch == 32 and args.dtype == "bf16"):
        return None, None
    try:
        import glob
        xr_path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_gemm_xreg_pmc.json")))[-1]      # the latest round's passes
        xr_name = os.path.basename(xr_path)
        xr = {s_["name"]: s_ for s_ in json.load(open(xr_path))["shapes"]}
        pk = {s_["name"]: s_ for s_ in json.load(open(os.path.join(ROOT, "profiles", "r2_gemm_packed_pmc.json")))["shapes"]}
        parts = [xr["norm+qkv"], xr["norm+gate_up+silu"], xr["down"], pk["o"]]
        traffic = sum(p_["fetch_bytes_corrected"] + p_["write_bytes"] for p_ in parts)
        alg = sum(p_["algorithmic_weight_bytes"] for p_ in parts)
        if alg != weight_bytes_per_layer:
            return None, None
        return int(traffic), (f"profiles/{xr_name} (norm+qkv, norm+gate|up+silu, down) + profiles/r2_gemm_packed_pmc.json (o): "
                              f"fetch (x2) + write bytes of the four launches = {traffic / alg:.4f} x the weight bytes "
                              "(the rest: the activations, the slabs in and out, the residual)")
    except Exception:
        return None, None


def in_step_attention(args, model_name):
    """The attention launch's duration INSIDE the decode step, from the last committed rocprofv3 kernel trace of this
    command (profiles/*_in_step.json, written by tools/layer_timeline.py through tools/prof_step.sh): the standalone figure of `roofline`
    is the conservative one, this is the one the step's time is made of.  Returns a dict or None."""
    if not (args.model == "7b" and args.batch == 32 and args.dtype == "bf16"):
        return None
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench7b_in_step.json")), reverse=True):
        try:
            d = json.load(open(path))
            return {"in_step_us": d["attention_us"], "in_step_frac": d.get("attention_frac"),
                    "in_step_source": f"profiles/{os.path.basename(path)} ({d.get('source', 'rocprofv3 --kernel-trace of this command')})"}
        except Exception:
            continue
    return None


def time_decode_gemms(runner, reps=3):
    """Summed duration of the four decode GEMM launches of a layer (qkv, o, gate|up, down: the
    weight-streaming HIP kernel exactly as the decode step calls it), HIP events over one graph
    that walks all layers' weights once (cold weights, like the step).  Returns per-projection
    microseconds and weight bytes."""
    from hydrainfer_amd._C.kernel import gemm as hip_gemm
    m, sh = runner.model, runner.model.shape
    B, dev, dt = runner.cfg.batch, runner.dev, runner.model.dtype
    if not (m.use_hip_gemm and B <= 64):
        return None
    m.pack_decode_weights()
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s_: torch.randn(s_, device=dev, generator=g).to(dt)
    x_h, x_q, x_i = rnd(B, sh.hidden_size), rnd(B, m.q_size), rnd(B, sh.intermediate_size)
    shapes = {"qkv": ("wqkv", x_h), "o": ("wo", x_q), "gate_up": ("wgu", x_h), "down": ("wdown", x_i)}
    ws = torch.empty(max(hip_gemm.workspace_floats(B, m.state[f"l0.{k}"].shape[0], m.state[f"l0.{k}"].shape[1])
                         for k, _ in shapes.values()), dtype=torch.float32, device=dev)
    L = sh.num_hidden_layers
    res = {}
    hid, inter = sh.hidden_size, sh.intermediate_size
    xreg = m.use_xreg and m._xreg_mlp_ok(B) and f"l{L - 1}.wdown" in m.packed_x
    fused = xreg and hip_gemm.gate_up_silu_supported(B, inter, hid, dt)
    if xreg:   # the activations as the decode step hands them over: fragment-major
        xf_h, xf_i = hip_gemm.to_fragment_major(x_h), hip_gemm.to_fragment_major(x_i)
        actf = torch.empty(hip_gemm.fragment_major_elems(B, inter), dtype=dt, device=dev)

    nf = xreg and fused and m.fuse_norm and hip_gemm.norm_xreg_supported(B, 2 * inter, hid, dt, gate_up=True)
    if nf:   # add+norm folded into the launch: give it slabs, a residual and a hand-over area per launch
        slabs_in = torch.randn((4, B, hid), device=dev, generator=g)
        resid = rnd(B, hid)
        nw = rnd(hid)
        xf_s = torch.empty_like(xf_h)
        ws_q = torch.empty_like(ws)
        sync = torch.zeros((L, hip_gemm.XREG_SYNC_WORDS), dtype=torch.int32, device=dev)

    def call(name, key, x, l):
        """One projection exactly as LlamaForCausalLM._decode_hidden_hip_gemm launches it."""
        full = f"l{l}.{key}"
        if xreg and name == "gate_up":
            if nf:
                return hip_gemm.norm_gate_up_silu_xreg(resid, slabs_in, 4, nw, 1e-5, xf_s, m.packed_x[full], inter, actf, sync[l])
            if fused:
                return hip_gemm.gate_up_silu_xreg(xf_h, m.packed_x[full], inter, actf, frag_shape=(B, hid))
            return hip_gemm.linear_decode_partial_xreg(xf_h, m.packed_x[full], 2 * inter, ws, frag_shape=(B, hid))
        if xreg and name == "down":
            return hip_gemm.linear_decode_partial_xreg(xf_i, m.packed_x[full], hid, ws, frag_shape=(B, inter))
        if xreg and name == "qkv" and full in m.packed_x:
            if nf:
                return hip_gemm.norm_linear_decode_xreg(resid, slabs_in, 4, nw, 1e-5, xf_s, m.packed_x[full],
                                                        m.state[full].shape[0], ws_q, sync[l])
            return hip_gemm.linear_decode_partial_xreg(xf_h, m.packed_x[full], m.state[full].shape[0], ws, frag_shape=(B, hid))
        return m._partial(x, full, ws)

    for name, (key, x) in shapes.items():
        def body():
            if nf:
                sync.zero_()
            for l in range(L):
                call(name, key, x, l)
        body(); torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            body()
        gr.replay(); torch.cuda.synchronize()
        total = 0.0
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); gr.replay(); e1.record(); e1.synchronize()
            total += e0.elapsed_time(e1)
        w = m.state[f"l0.{key}"]
        res[name] = {"us": round(total / reps / L * 1e3, 2), "weight_bytes": w.numel() * w.element_size()}
    res["_kernels"] = ("gemm_xreg_kernel (activations in registers; gate|up with the silu*mul epilogue, down, qkv of "
                       "layers >= 1" + ("; the gate|up and qkv launches INCLUDE the add+RMSNorm that produces their "
                                        "input (4 slabs in)" if nf else "") +
                       ") + gemm_packed_kernel (o, qkv of layer 0)") if xreg else "gemm_packed_kernel"
    return res


def cpu_clip_encode_s(dtype, n_layers=2):
    """The oracle's CLIP ViT-L/14-336 tower + LLaVA projector (oracle/vision.py, the reference's
    torch path restated) on this host's cores for ONE image: n_layers of the 23 executed encoder
    layers timed, extrapolated per layer."""
    try:
        import dataclasses
        from hydrainfer_amd.model.clip import CLIP_VIT_L_14_336
        from oracle.vision import vision_forward
        g = torch.Generator().manual_seed(3)
        full = CLIP_VIT_L_14_336
        h, i_, p_ = full.hidden_size, full.intermediate_size, full.patch_size
        n_pos = (full.image_size // p_) ** 2 + 1

        def w(*s_):
            return (torch.randn(s_, generator=g) * 0.02).to(dtype)

        def state(nl):
            vt = "vision_tower.vision_model."
            sd = {vt + "embeddings.class_embedding": w(h),
                  vt + "embeddings.patch_embedding.weight": w(h, 3, p_, p_),
                  vt + "embeddings.position_embedding.weight": w(n_pos, h),
                  vt + "pre_layrnorm.weight": torch.ones(h, dtype=dtype),
                  vt + "pre_layrnorm.bias": torch.zeros(h, dtype=dtype),
                  "multi_modal_projector.linear_1.weight": w(full.projector_hidden_size, h),
                  "multi_modal_projector.linear_1.bias": w(full.projector_hidden_size),
                  "multi_modal_projector.linear_2.weight": w(full.projector_hidden_size, full.projector_hidden_size),
                  "multi_modal_projector.linear_2.bias": w(full.projector_hidden_size)}
            for l in range(nl):
                pre = vt + f"encoder.layers.{l}."
                for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
                    sd[pre + f"self_attn.{nm}.weight"] = w(h, h)
                    sd[pre + f"self_attn.{nm}.bias"] = w(h)
                sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"] = w(i_, h), w(i_)
                sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"] = w(h, i_), w(h)
                for nm in ("layer_norm1", "layer_norm2"):
                    sd[pre + nm + ".weight"], sd[pre + nm + ".bias"] = torch.ones(h, dtype=dtype), torch.zeros(h, dtype=dtype)
            return sd
        pixels = torch.randn((1, 3, full.image_size, full.image_size), generator=g).to(dtype)

        def run(nl):
            # vision_feature_layer = nl - 1 makes the oracle run exactly nl encoder layers
            shp = dataclasses.replace(full, num_hidden_layers=nl, vision_feature_layer=nl - 1)
            sd = state(nl)
            with torch.inference_mode():
                vision_forward(shp, sd, pixels)
                t0 = time.perf_counter()
                vision_forward(shp, sd, pixels)
            return time.perf_counter() - t0
        t_n, t_1 = run(n_layers + 1), run(1)     # the oracle always runs at least one layer
        return round(t_1 + (t_n - t_1) / n_layers * (full.num_hidden_layers - 2), 3)
    except Exception as e:     # the CLIP timing is a side figure: never lose the baseline for it
        return f"not timed: {e!r}"[:120]


def cpu_baseline(shape, dtype, batch, ctx, n_layers):
    """The oracle (reference's eager-PyTorch CPU path restated) timed on this host's cores:
    one decode step of `n_layers` of the decoder layers + final norm + lm_head at the mid-run
    context, extrapolated linearly to all layers."""
    from oracle.model import OracleAttnMeta, OracleLlama
    g = torch.Generator().manual_seed(0)
    # torch's default (all hardware threads) can be far from the fastest setting for M=32
    # GEMMs on a many-core host: calibrate the thread count on one projection-sized GEMM and
    # report the count actually used.
    xa = torch.randn((batch, shape.hidden_size), generator=g).to(dtype)
    wa = torch.randn((shape.intermediate_size, shape.hidden_size), generator=g).to(dtype)
    best_t, best = None, float("inf")
    for t in sorted({min(os.cpu_count(), n) for n in (8, 16, 32, 64, 128, os.cpu_count())}):
        torch.set_num_threads(t)
        torch.nn.functional.linear(xa, wa)
        t0 = time.perf_counter()
        torch.nn.functional.linear(xa, wa)
        dt_ = time.perf_counter() - t0
        if dt_ < best:
            best_t, best = t, dt_
        if dt_ > 2.0:
            break
    torch.set_num_threads(best_t)
    n_threads = best_t
    h, i = shape.hidden_size, shape.intermediate_size
    q = shape.num_attention_heads * shape.head_dim
    kv = shape.num_key_value_heads * shape.head_dim

    def w(*s):
        return (torch.randn(s, generator=g) * 0.02).to(dtype)
    sd = {"model.embed_tokens.weight": w(shape.vocab_size, h), "lm_head.weight": w(shape.vocab_size, h),
          "model.norm.weight": torch.ones(h, dtype=dtype)}
    for l in range(n_layers):
        p = f"model.layers.{l}."
        sd.update({p + "self_attn.q_proj.weight": w(q, h), p + "self_attn.k_proj.weight": w(kv, h),
                   p + "self_attn.v_proj.weight": w(kv, h), p + "self_attn.o_proj.weight": w(h, q),
                   p + "mlp.gate_proj.weight": w(i, h), p + "mlp.up_proj.weight": w(i, h),
                   p + "mlp.down_proj.weight": w(h, i),
                   p + "input_layernorm.weight": torch.ones(h, dtype=dtype),
                   p + "post_attention_layernorm.weight": torch.ones(h, dtype=dtype)})
    model = OracleLlama(shape, sd, dtype, n_layers=n_layers)
    bs = 16
    nb_seq = (ctx + bs - 1) // bs
    n_blocks = max(batch * nb_seq, (608 + 16 + bs - 1) // bs)
    caches = [(torch.randn((n_blocks, bs, shape.num_key_value_heads, shape.head_dim), generator=g).to(dtype),
               torch.randn((n_blocks, bs, shape.num_key_value_heads, shape.head_dim), generator=g).to(dtype))
              for _ in range(n_layers)]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    bt = list(range(n_blocks))
    slots = [bt[b * nb_seq + (ctx - 1) // bs] * bs + (ctx - 1) % bs for b in range(batch)]
    meta = OracleAttnMeta(i32(list(range(batch + 1))), i32([ctx * b for b in range(batch + 1)]),
                          i32(slots), i32(bt), i32([nb_seq * b for b in range(batch + 1)]))
    ids = torch.randint(0, shape.vocab_size, (batch,), generator=g, dtype=torch.int64)
    pos = i32([ctx - 1] * batch)

    def run(nl):
        model.n_layers = nl
        t0 = time.perf_counter()
        with torch.inference_mode():
            model.forward(ids, pos, meta, caches)
        return time.perf_counter() - t0
    run(n_layers)                                # warm
    t_full = min(run(n_layers) for _ in range(2))
    t_head = min(run(0) for _ in range(2))       # embed + final norm + lm_head only
    per_layer = (t_full - t_head) / n_layers
    step_s = t_head + per_layer * shape.num_hidden_layers

    # BASELINE configs[0] on the same cores: ONE request, 576 image + 32 text tokens prefilled
    # (608 tokens, 38 blocks), then single-sequence decode steps — the reference's eager CPU path
    n_p = 608
    nb_p = (n_p + 16 + bs - 1) // bs
    meta_p = OracleAttnMeta(i32([0, n_p]), i32([0, n_p]), i32(list(range(n_p))), i32(list(range(nb_p))),
                            i32([0, nb_p]))
    ids_p = torch.randint(0, 32000, (n_p,), generator=g, dtype=torch.int64)
    pos_p = torch.arange(n_p, dtype=torch.int32)
    meta_d = OracleAttnMeta(i32([0, 1]), i32([0, n_p + 1]), i32([n_p]), i32(list(range(nb_p))), i32([0, nb_p]))

    def run1(nl, prefill):
        model.n_layers = nl
        t0 = time.perf_counter()
        with torch.inference_mode():
            if prefill:
                model.forward(ids_p, pos_p, meta_p, caches)
            else:
                model.forward(ids_p[:1], i32([n_p]), meta_d, caches)
        return time.perf_counter() - t0
    run1(n_layers, True)
    # layers over all 608 rows; embedding + final norm + lm_head only for the one sampled row
    pf = min(run1(n_layers, True) for _ in range(2)) - min(run1(0, True) for _ in range(2))
    prefill_s = min(run1(0, False) for _ in range(2)) + pf / n_layers * shape.num_hidden_layers
    run1(n_layers, False)
    dc = min(run1(n_layers, False) for _ in range(2)) - (h1 := min(run1(0, False) for _ in range(2)))
    decode1_s = h1 + dc / n_layers * shape.num_hidden_layers
    clip_s = cpu_clip_encode_s(dtype)
    # ---- the SAME decode step through ALL layers (round 5): the two timed layers above are re-run over the same 0.8 GB
    # of weights, which a big host's last-level caches hold; the full step streams every layer's own weights and KV from
    # DRAM (profiles/r5_cpu_config0_full.json: batch-1 decode 0.62 tok/s in full against 5.9 extrapolated).  Layer l's
    # tensors are clones of layer l mod n_layers (distinct memory), the caches of the other layers a constant fill.
    full_step_s = full_err = None
    try:
        L = shape.num_hidden_layers
        for l in range(n_layers, L):
            for k_ in [k for k in sd if k.startswith(f"model.layers.{l % n_layers}.")]:
                sd[k_.replace(f"model.layers.{l % n_layers}.", f"model.layers.{l}.", 1)] = sd[k_].clone()
        caches_full = list(caches) + [(torch.empty_like(caches[0][0]).fill_(0.01), torch.empty_like(caches[0][1]).fill_(0.01))
                                      for _ in range(L - n_layers)]
        model.n_layers = L
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            with torch.inference_mode():
                model.forward(ids, pos, meta, caches_full)
            ts.append(time.perf_counter() - t0)
        full_step_s = min(ts)
        del caches_full
    except Exception as e:      # e.g. a host without the ~30 GB this needs: the extrapolated figure stays
        full_err = repr(e)[:200]
    measured = full_step_s is not None
    return {"value": round(batch / (full_step_s if measured else step_s), 3), "unit": "tokens/s", "cores": n_threads,
            "kind": "port" if measured else "port-extrapolated",
            "extrapolated_value": round(batch / step_s, 3),
            "full_step_s": None if not measured else round(full_step_s, 3), "full_step_error": full_err,
            "config0": {"what": "BASELINE configs[0]: 1 request = CLIP ViT-L/14-336 encode of 1 image (2 of 23 "
                                "tower layers timed, extrapolated) + 608-token prefill + batch-1 decode, same "
                                "per-layer extrapolation for the language model",
                        "clip_encode_s": clip_s, "prefill_s": round(prefill_s, 2),
                        "decode_tokens_per_s": round(1.0 / decode1_s, 3)},
            "sample": (f"one decode step, batch {batch}, ctx {ctx}, through ALL {shape.num_hidden_layers} decoder layers + lm_head "
                       f"with torch CPU ({str(dtype).split('.')[-1]} weights, fp32 attention as the reference's torch handler): "
                       f"{full_step_s:.1f} s of CPU work, best of 2; `extrapolated_value` is the former figure ({n_layers} layers "
                       f"timed and scaled x{shape.num_hidden_layers}: cache-resident weights, optimistic)" if measured else
                       f"one decode step, batch {batch}, ctx {ctx}: {n_layers} of {shape.num_hidden_layers} decoder layers + "
                       f"lm_head timed with torch CPU, per-layer time extrapolated x{shape.num_hidden_layers}; "
                       f"{t_full + t_head:.1f}s of CPU work per repetition")}


def cpu_config0_full(shape, dtype, n_threads, n_generate=16):
    """BASELINE configs[0] run FOR REAL on the host cores (round-4 review, item 5): ONE request — CLIP ViT-L/14-336 encode
    of one image (all 23 executed tower layers + projector, oracle/vision.py), 576 + 32 = 608-token prefill through ALL
    decoder layers (oracle/model.py = the reference's eager torch CPU path, hydrainfer/layer/causal_attention.py:297-374),
    then n_generate - 1 single-sequence decode steps — nothing extrapolated.  Weights: one random decoder layer cloned
    per layer (distinct memory, identical values: random-filling 6.7 G parameters on the CPU would take longer than the
    measurement); same for the tower."""
    import numpy as np
    from hydrainfer_amd.model.clip import CLIP_VIT_L_14_336
    from oracle.model import OracleAttnMeta, OracleLlama
    from oracle.vision import vision_forward
    torch.set_num_threads(n_threads)
    g = torch.Generator().manual_seed(0)
    h, i = shape.hidden_size, shape.intermediate_size
    q, kv = shape.num_attention_heads * shape.head_dim, shape.num_key_value_heads * shape.head_dim

    def w(*s_):
        return (torch.randn(s_, generator=g) * 0.02).to(dtype)
    t_build = time.perf_counter()
    base = {"self_attn.q_proj.weight": w(q, h), "self_attn.k_proj.weight": w(kv, h), "self_attn.v_proj.weight": w(kv, h),
            "self_attn.o_proj.weight": w(h, q), "mlp.gate_proj.weight": w(i, h), "mlp.up_proj.weight": w(i, h),
            "mlp.down_proj.weight": w(h, i), "input_layernorm.weight": torch.ones(h, dtype=dtype),
            "post_attention_layernorm.weight": torch.ones(h, dtype=dtype)}
    sd = {"model.embed_tokens.weight": w(shape.vocab_size, h), "lm_head.weight": w(shape.vocab_size, h),
          "model.norm.weight": torch.ones(h, dtype=dtype)}
    for l in range(shape.num_hidden_layers):
        for k_, v_ in base.items():
            sd[f"model.layers.{l}.{k_}"] = v_.clone()
    full = CLIP_VIT_L_14_336
    ch, ci, cp = full.hidden_size, full.intermediate_size, full.patch_size
    vt = "vision_tower.vision_model."
    vsd = {vt + "embeddings.class_embedding": w(ch), vt + "embeddings.patch_embedding.weight": w(ch, 3, cp, cp),
           vt + "embeddings.position_embedding.weight": w((full.image_size // cp) ** 2 + 1, ch),
           vt + "pre_layrnorm.weight": torch.ones(ch, dtype=dtype), vt + "pre_layrnorm.bias": torch.zeros(ch, dtype=dtype),
           "multi_modal_projector.linear_1.weight": w(full.projector_hidden_size, ch),
           "multi_modal_projector.linear_1.bias": w(full.projector_hidden_size),
           "multi_modal_projector.linear_2.weight": w(full.projector_hidden_size, full.projector_hidden_size),
           "multi_modal_projector.linear_2.bias": w(full.projector_hidden_size)}
    cbase = {}
    for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
        cbase[f"self_attn.{nm}.weight"], cbase[f"self_attn.{nm}.bias"] = w(ch, ch), w(ch)
    cbase["mlp.fc1.weight"], cbase["mlp.fc1.bias"] = w(ci, ch), w(ci)
    cbase["mlp.fc2.weight"], cbase["mlp.fc2.bias"] = w(ch, ci), w(ch)
    for nm in ("layer_norm1", "layer_norm2"):
        cbase[nm + ".weight"], cbase[nm + ".bias"] = torch.ones(ch, dtype=dtype), torch.zeros(ch, dtype=dtype)
    n_run = (full.vision_feature_layer + full.num_hidden_layers) % full.num_hidden_layers + 1      # 23 of 24
    for l in range(n_run):
        for k_, v_ in cbase.items():
            vsd[vt + f"encoder.layers.{l}.{k_}"] = v_.clone()
    t_build = time.perf_counter() - t_build
    model = OracleLlama(shape, sd, dtype)
    bs, n_p = 16, 608
    nb = (n_p + n_generate + bs - 1) // bs
    caches = [(torch.zeros((nb, bs, shape.num_key_value_heads, shape.head_dim), dtype=dtype),
               torch.zeros((nb, bs, shape.num_key_value_heads, shape.head_dim), dtype=dtype)) for _ in range(shape.num_hidden_layers)]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    np.random.seed(0)
    pixels = torch.from_numpy(np.random.randint(0, 256, (1, 3, 336, 336)).astype(np.float32) / 255.0).to(dtype)
    ids = torch.randint(1000, 31999, (n_p,), generator=g, dtype=torch.int64)
    with torch.inference_mode():
        t0 = time.perf_counter()
        feats = vision_forward(full, vsd, pixels)                       # [1, 576, hidden]
        t_enc = time.perf_counter() - t0
        embeds = torch.nn.functional.embedding(ids, sd["model.embed_tokens.weight"])
        embeds[:576] = feats[0].to(dtype)                               # llava.py:132-135: image-token rows
        meta = OracleAttnMeta(i32([0, n_p]), i32([0, n_p]), i32(list(range(n_p))), i32(list(range(nb))), i32([0, nb]))
        t0 = time.perf_counter()
        tok = model.forward(embeds, torch.arange(n_p, dtype=torch.int32), meta, caches, torch.tensor([n_p - 1]))
        t_pre = time.perf_counter() - t0
        t0 = time.perf_counter()
        for s_ in range(n_generate - 1):
            ctx_ = n_p + s_ + 1
            meta = OracleAttnMeta(i32([0, 1]), i32([0, ctx_]), i32([ctx_ - 1]), i32(list(range(nb))), i32([0, nb]))
            tok = model.forward(tok.reshape(1), i32([ctx_ - 1]), meta, caches)
        t_dec = time.perf_counter() - t0
    total = t_enc + t_pre + t_dec
    return {"what": "BASELINE configs[0] in full on the host cores: 1 image (23 CLIP layers + projector) + 608-token prefill "
                    f"through all {shape.num_hidden_layers} decoder layers + {n_generate - 1} batch-1 decode steps, oracle/ (the "
                    "reference's eager torch CPU path restated); nothing extrapolated",
            "cores": os.cpu_count(), "threads": n_threads, "dtype": str(dtype).split(".")[-1],
            "clip_encode_s": round(t_enc, 3), "prefill_s": round(t_pre, 3), "ttft_s": round(t_enc + t_pre, 3),
            "decode_s": round(t_dec, 3), "decode_tokens_per_s": round((n_generate - 1) / t_dec, 3),
            "request_s": round(total, 3), "output_tokens_per_s": round(n_generate / total, 3),
            "weight_build_s": round(t_build, 1)}


def parity_probe(dtype, dev, executor, steps=4):
    """`parity_probe` (round-5 review, item 5): the tokens/s above travels with evidence FROM THE SAME PROCESS that the path
    it timed computes what the reference computes.  A 2-layer model of the headline's width (hidden 4096, 32 heads x 128,
    inter 11008, vocab 32064; random weights, seed 3) is run through the benchmarked configuration — 32 rows, the decode
    step replayed by the same executor, default flags — for `steps` decode steps behind a 40-token prefill, and the CPU
    oracle (oracle/model.py: the reference's eager torch path restated; a CHECKER here, like the cpu_baseline leg — never
    part of the measured path) is teacher-forced with the device's tokens on the same weights and block tables.
    tests/test_gpu_bench_config.py is the full form of this check (8 steps, both widths, both executors, both dtypes)."""
    from hydrainfer_amd.model.llama import LlamaForCausalLM, LlamaShape
    from hydrainfer_amd.model.runner import DecodeRunner, RunnerConfig
    from oracle.model import OracleAttnMeta, OracleLlama
    B, P, bs = 32, 40, 16
    tol = {torch.bfloat16: 1.5e-1, torch.float16: 3e-2}[dtype]
    tol32 = {torch.bfloat16: 1e-1, torch.float16: 2e-2}[dtype]
    ulp = {torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}[dtype]
    shape = LlamaShape(4096, 11008, 2, 32, 32, 128, 32064)
    model = LlamaForCausalLM.random_init(shape, dtype, dev, seed=3)
    runner = DecodeRunner(model, RunnerConfig(batch=B, prompt_len=P, n_generate=steps + 4, use_graph=True, executor=executor), seed=4)
    oracle = OracleLlama(shape, model.to_reference_state_dict(), dtype)
    pool0 = runner.pool.cpu().clone()
    prompts = torch.randint(5, 32000, (B, P), generator=torch.Generator().manual_seed(11))
    stash = {}
    orig, orig_hidden = model.forward_logits, model.forward_hidden
    model.forward_logits = lambda *a, **k: stash.__setitem__("logits", orig(*a, **k)) or stash["logits"]
    model.forward_hidden = lambda *a, **k: stash.__setitem__("x", orig_hidden(*a, **k)) or stash["x"]
    toks = [runner.prefill(prompts.to(dev)).cpu()]
    logits, xs = [], []
    for _ in range(steps):
        runner.step()
        torch.cuda.synchronize(dev)
        logits.append(stash["logits"].float().cpu().clone())
        xs.append(stash["x"].float().cpu().clone())
        toks.append(runner.input_ids.cpu().clone())
    if model.handover_failed():
        return {"error": "a norm-fused launch gave up waiting for its producer workgroups"}
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    caches = [(pool0[l, 0], pool0[l, 1]) for l in range(shape.num_hidden_layers)]
    tables, n_pb = runner.tables, (P + bs - 1) // bs
    meta = OracleAttnMeta(i32([P * r for r in range(B + 1)]), i32([P * r for r in range(B + 1)]),
                          i32([tables[r][p_ // bs] * bs + p_ % bs for r in range(B) for p_ in range(P)]),
                          i32([b for r in range(B) for b in tables[r][:n_pb]]), i32([n_pb * r for r in range(B + 1)]))
    w32 = oracle.sd["lm_head.weight"].float()
    n_rows = n_cmp = n_cmp32 = n_same = n_bad = n_far = 0
    worst = worst32 = 0.0
    with torch.inference_mode():
        oracle.forward_logits(prompts.reshape(-1), i32(list(range(P)) * B), meta, caches, torch.arange(P - 1, B * P, P))   # fills the oracle's cache
        for s_ in range(steps):
            ctx_, pos = P + s_ + 1, P + s_
            nb = (ctx_ + bs - 1) // bs
            meta = OracleAttnMeta(i32(list(range(B + 1))), i32([ctx_ * r for r in range(B + 1)]),
                                  i32([tables[r][pos // bs] * bs + pos % bs for r in range(B)]),
                                  i32([b for r in range(B) for b in tables[r][:nb]]), i32([nb * r for r in range(B + 1)]))
            ref_x = oracle.forward_hidden(toks[s_], i32([pos] * B), meta, caches)
            ref = torch.nn.functional.linear(ref_x, oracle.sd["lm_head.weight"]).float()
            ref32, hip32 = ref_x.float() @ w32.t(), xs[s_] @ w32.t()
            worst = max(worst, (logits[s_] - ref).abs().max().item())
            worst32 = max(worst32, (hip32 - ref32).abs().max().item())
            top = ref.sort(dim=-1).values
            clear = (top[:, -1] - top[:, -2]) > 2 * tol
            top32 = ref32.sort(dim=-1).values
            clear32 = (top32[:, -1] - top32[:, -2]) > 2 * tol32 + 2 * ulp
            same, same32 = toks[s_ + 1] == ref.argmax(-1), toks[s_ + 1] == ref32.argmax(-1)
            gap = ref.max(-1).values - ref.gather(1, toks[s_ + 1][:, None])[:, 0]      # every row: how far below the oracle's top-1
            n_far += int((gap > 2 * tol).sum())
            n_bad += int((clear & ~same).sum()) + int((clear32 & ~same32).sum())
            n_rows += B
            n_cmp += int(clear.sum())
            n_cmp32 += int(clear32.sum())
            n_same += int(same.sum())
    model.forward_logits, model.forward_hidden = orig, orig_hidden
    model.release()
    return {"what": f"2-layer model of the headline's width, {B} rows, {steps} decode steps replayed by the '{runner.executor_used}' executor behind a "
                    f"{P}-token prefill, teacher-forced against oracle/model.py on the host (checker only)",
            "dtype": str(dtype).split(".")[-1], "max_abs_dlogit": round(worst, 4), "logit_tolerance": tol,
            "max_abs_dlogit_fp32_head": round(worst32, 4), "fp32_head_tolerance": tol32,
            "rows": n_rows, "tokens_compared_by_margin": n_cmp, "tokens_compared_by_fp32_head_margin": n_cmp32,
            "tokens_identical_regardless_of_margin": n_same, "compared_tokens_that_differ": n_bad,
            "tokens_further_than_2_tol_below_the_oracles_top1": n_far,
            "ok": bool(n_bad == 0 and n_far == 0 and worst <= tol and worst32 <= tol32)}


TIMED_REGIONS = 3


def decode_leg(ctx, model, runner, passes, warmup, prompt_len, regions=TIMED_REGIONS):
    """Warm-up, then the timed region of the contract: barrier + synchronize on both sides, exactly
    sum(len(p) for p in passes) decode steps, MAX over ranks.  Within a pass the contexts are equally spaced: the step's
    own device-side advance moves the decode state from one to the next (stride 1 = the generation itself), so the timed
    region is nothing but the K steps; between passes (more steps than the generation has: `timed_passes`) the clock
    stops while the state is rewound.
    The region is run `regions` times behind the one warm-up (state rewound in between, outside the clocks), each bracketed
    as the contract says; the line reports the MEDIAN region (round-5 review: one 0.1-s region at a threshold with +-1 %
    box-to-box spread is a coin flip) and carries the fastest and slowest beside it.  Returns (median elapsed s, all)."""
    ctxs = passes[0]
    stride = ctxs[1] - ctxs[0] if len(ctxs) > 1 else 1
    assert all(b - a == stride for p in passes for a, b in zip(p, p[1:])), "timed contexts must be equally spaced"
    assert len(passes) == 1 or stride == 1, "several passes walk consecutive contexts"
    runner.cfg.advance_stride = stride
    ids = runner.input_ids.clone()
    if runner.cfg.use_graph:
        runner.set_state(ctxs[0] - stride, ids)
        runner.capture()
    for _ in range(warmup):
        runner.set_state(ctxs[0] - stride, ids)
        runner.step(record=False)
    all_elapsed = []
    for _ in range(max(1, regions)):
        elapsed = 0.0
        for i, p in enumerate(passes):
            runner.set_state(p[0] - stride, ids)      # the first step's advance makes it p[0]
            if i == 0:
                ctx.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in p:
                runner.step(record=False)
            torch.cuda.synchronize()
            elapsed += time.perf_counter() - t0
            assert int(runner.kv_lens[0]) == p[-1], "the timed steps did not walk the announced contexts"
        all_elapsed.append(ctx.max_over_ranks(elapsed, runner.dev))
        ctx.barrier(); torch.cuda.synchronize()
    # an in-kernel hand-over that gave up waiting leaves an error word: not a measurement
    if model.handover_failed():
        print("bench.py: a norm-fused launch gave up waiting for its producer workgroups",
              file=sys.stderr, flush=True)
        sys.exit(4)
    return sorted(all_elapsed)[len(all_elapsed) // 2], all_elapsed


DUMP_BYTES_PER_ARRAY = 48 << 20


def dump_outputs(runner, out_dir, max_bytes=DUMP_BYTES_PER_ARRAY):
    """--dump-outputs: what the last timed step handed its caller, as DIR/<name>.npy — the token each sequence sampled
    (float64, exact) and the K / V rows the step appended to every layer's cache ([layers, k|v, sequence, kv head,
    head_dim], float32).  An array larger than `max_bytes` is written as a fixed sample of its flattened elements: the
    first max_bytes / 4 of torch.randperm(size, generator=torch.Generator().manual_seed(0)), in ascending order."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    torch.cuda.synchronize(runner.dev)
    bs = runner.cfg.block_size
    slots = runner.slots.long()          # the cache slots the last step wrote
    arrays = {"next_token_ids": runner.input_ids.to(torch.float64),
              "kv_appended": runner.pool[:, :, slots // bs, slots % bs].float()}
    for name, t in arrays.items():
        a = t.cpu().numpy()
        if a.nbytes > max_bytes:
            g = torch.Generator().manual_seed(0)
            idx = torch.randperm(a.size, generator=g)[: max_bytes // a.itemsize].sort().values.numpy()
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def region_spread(all_elapsed, n_steps):
    """ms_per_step of every timed region, for the line."""
    ms = [e / n_steps * 1e3 for e in all_elapsed]
    return {"timed_regions": len(ms), "ms_per_step_min": round(min(ms), 4), "ms_per_step_max": round(max(ms), 4),
            "ms_per_step_all": [round(m, 4) for m in ms]}


def leg_64_rows(ctx, model, args, dev, prompt_len, n_generate, steps=20):
    """`whole_step_64`: the decode step at TWICE the batch (64 rows; the reference's layers have no batch limit,
    hydrainfer/model/model_forward.py:29-37) on the same model: 33 .. 64 rows run the wide form of the
    activations-in-registers GEMMs (6 launches per layer).  KV cache: its random fill (no prefill: only the
    step is timed), contexts spaced over the generation's 705..959 like the headline."""
    from hydrainfer_amd.model.runner import DecodeRunner, RunnerConfig
    B = 2 * args.batch
    if B > 64:
        return None
    cfg = RunnerConfig(batch=B, prompt_len=prompt_len, n_generate=n_generate, use_graph=not args.no_graph, executor=args.executor)
    runner = DecodeRunner(model, cfg, seed=7)
    runner.input_ids.copy_(torch.randint(1000, 30000, (B,), device=dev))
    ctxs = timed_contexts(prompt_len, n_generate, steps)
    elapsed, all_elapsed = decode_leg(ctx, model, runner, [ctxs], 3, prompt_len)
    ms = elapsed / len(ctxs) * 1e3
    step_bytes = sum(runner.step_bytes(c * B) for c in ctxs) / len(ctxs)
    gbs = step_bytes / (ms * 1e-3) / 1e9
    dp = model._decode_plan(B, model.dtype)
    return {"rows": B, "ms_per_step": round(ms, 4), **region_spread(all_elapsed, len(ctxs)),
            "value": round(B * len(ctxs) / elapsed, 2), "unit": "tokens/s",
            "algorithmic_bytes": int(step_bytes), "achieved_GBps": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
            "launches_per_layer": (5 if dp.get("wide_silu") else 6) if dp["wide"] and dp["nf_gu"] and dp["nf_qkv"] else 8,
            "layer": (("attention | o | norm + gate|up + silu*mul (both K halves in one workgroup, no slabs) | down | norm + qkv "
                       "(2 slabs): wide activations-in-registers kernel over the <= 32-row packing" if dp.get("wide_silu") else
                       "attention | o | norm + gate|up (2 slabs) | silu*mul | down | norm + qkv (2 slabs): wide activations-in-registers "
                       "kernel over the <= 32-row packing") if dp["wide"] else "LDS-slice GEMMs with separate norm / silu launches"),
            "weight_bytes_resident": model.weight_bytes_resident(), "contexts": ctx_label(ctxs)}


def leg_ragged(model, runner, args, steps=20, regions=TIMED_REGIONS):
    """`whole_step_ragged` (round-5 review, item 2): the decode step on RAGGED batches — the reference's scheduler makes
    one every step (hydrainfer/engine/scheduler.py:99-194; BASELINE configs[2] "mixed image+text") while the headline's 32
    sequences all share one context.  Two length sets (hydrainfer_amd/model/runner.py::ragged_contexts): uniform over
    64..959, and bimodal 16 x ~130 (text-only) + 16 x ~830 (image).  Each is timed as `steps` consecutive decode steps of a
    generation starting there (every sequence grows by one key per step; median of `regions` timed regions), next to a
    batch with the SAME sum of contexts spread evenly over the sequences; algorithmic bytes from the true sum of contexts
    of every step; the attention launch alone on the same lengths beside it.  ragged_over_even = even ms / ragged ms."""
    import statistics
    from hydrainfer_amd.model.runner import ragged_contexts
    B, dev = runner.cfg.batch, runner.dev
    runner.cfg.advance_stride = 1
    ids = torch.randint(1000, 30000, (B,), device=dev)
    captured = [False]

    def timed(lens0):
        start = [l - 1 for l in lens0]          # the first step's own advance makes it lens0
        if runner.cfg.use_graph and not captured[0]:
            runner.graph = None
            runner.set_state_lens(start, ids)
            runner.capture()                        # stride 1 is an argument recorded with the step
            captured[0] = True
        for _ in range(2):
            runner.set_state_lens(start, ids)
            runner.step(record=False)
        ts = []
        for _ in range(regions):
            runner.set_state_lens(start, ids)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                runner.step(record=False)
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) / steps * 1e3)
        assert runner.kv_lens.tolist() == [l + steps - 1 for l in lens0], "the timed steps did not walk the announced contexts"
        return statistics.median(ts), ts

    def one(lens0):
        per_step = [[l + k for l in lens0] for k in range(steps)]
        ms, ts = timed(lens0)
        step_bytes = sum(runner.step_bytes(sum(c)) for c in per_step) / steps
        attn_bytes = sum(runner.attention_bytes(c) for c in per_step) / steps
        attn_ms = time_attention_kernel(runner, per_step)
        return {"ms_per_step": round(ms, 4), "ms_per_step_min": round(min(ts), 4), "ms_per_step_max": round(max(ts), 4),
                "value": round(B / ms * 1e3, 1), "unit": "tokens/s", "algorithmic_bytes": int(step_bytes),
                "frac_of_hbm_peak": round(step_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "attention": {"avg_launch_us": round(attn_ms * 1e3, 2), "algorithmic_bytes_per_launch": int(attn_bytes),
                              "achieved_GBps": round(attn_bytes / (attn_ms * 1e-3) / 1e9, 1),
                              "frac": round(attn_bytes / (attn_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}}

    out = {"what": f"batch {B}, {steps} consecutive decode steps from ragged contexts, median of {regions} timed regions "
                   "(host clock around synchronize, the step replayed as in the headline); `even` = the same sum of contexts "
                   "spread evenly; attention = that launch alone on the same lengths (hipGraph of the steps' launches, HIP events)",
           "attention_grid": "one workgroup per (head, sequence) [the reference: one CTA per (m_block, seq, head), "
                             "flash_fwd_launch_template.h:77], 4 waves interleaving the sequence's 16-key tiles"
                             + ("" if args.no_ranked else "; ragged batches: the pairs are taken in length-ranked snake order over "
                                "the CUs (attn_decode.hip, RANKED)")}
    for kind in ("uniform", "bimodal"):
        cap = runner.max_len - 1 - steps
        lens0 = [min(l, cap) for l in ragged_contexts(kind, B)]
        total = sum(lens0)
        even = [total // B + (1 if i < total % B else 0) for i in range(B)]
        r, e = one(lens0), one(even)
        out[kind] = {"contexts_at_step_0": lens0, "sum_contexts": total, "min": min(lens0), "max": max(lens0),
                     "ragged": r, "even": e,
                     "ragged_over_even_step": round(e["ms_per_step"] / r["ms_per_step"], 4),
                     "ragged_over_even_attention": round(e["attention"]["avg_launch_us"] / r["attention"]["avg_launch_us"], 4)}
    runner.graph = None          # (captured with stride 1 and this leg's state: nothing after this leg replays it)
    return out


MFMA_PEAK_TFLOPS = 2500.0      # dense bf16 / fp16, MI355X_MICROARCH.md


def time_prefill_attention(shape, dtype, dev, n_seqs=4, n_tokens=704, reps=3, launches=10, kv_tokens=None, brief=False):
    """`roofline_prefill_attention`: the MFMA-bound kernel of the path — paged causal prefill attention of n_seqs x
    n_tokens new tokens (the prefill of 4 of the benchmark's requests) through the C ABI (hx_attn, the 32x32x16
    kernel), HIP events over a hipGraph of `launches` launches on random pages, mean of `reps` replays."""
    import math
    from hydrainfer_amd._C.kernel.flash_attn import mha_varlen_fwd
    H, HK, D, bs = shape.num_attention_heads, shape.num_key_value_heads, shape.head_dim, 16
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *s_: torch.randn(s_, device=dev, generator=g).to(dtype)
    kv = kv_tokens or n_tokens          # kv > n_tokens: a chunk of a longer prompt (cached prefix of kv - n_tokens keys)
    nb = (kv + bs - 1) // bs
    kc, vc, q = rnd(n_seqs * nb, bs, HK, D), rnd(n_seqs * nb, bs, HK, D), rnd(n_seqs * n_tokens, H, D)
    out = torch.empty_like(q)
    perm = torch.randperm(n_seqs * nb, generator=g, device=dev).to(torch.int32)
    cu_b = torch.arange(0, (n_seqs + 1) * nb, nb, dtype=torch.int32, device=dev)
    cu = torch.arange(0, (n_seqs + 1) * n_tokens, n_tokens, dtype=torch.int32, device=dev)
    cu_k = torch.arange(0, (n_seqs + 1) * kv, kv, dtype=torch.int32, device=dev)
    fn = lambda: mha_varlen_fwd(out, q, kc, vc, cu, cu_k, perm, cu_b, None, n_tokens, kv, 1 / math.sqrt(D), 0, -1, 0, 0)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            fn()
    graph.replay()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); graph.replay(); e1.record()
        torch.cuda.synchronize(dev)
        ts.append(e0.elapsed_time(e1) / launches * 1e3)
    us = sum(ts) / len(ts)
    flops = 4 * H * D * n_seqs * sum(kv - n_tokens + i + 1 for i in range(n_tokens))       # Q.K and P.V over the causal triangle
    tf = flops / us / 1e6
    if brief:
        return {"workload": f"{n_seqs} x {n_tokens} new tokens" + (f" of {kv}" if kv != n_tokens else ""), "avg_launch_us": round(us, 2),
                "achieved": round(tf, 1), "frac": round(tf / MFMA_PEAK_TFLOPS, 4)}
    return {"bound": "mfma", "kernel": "attn_fwd32_kernel / attn_fwd32p_kernel (paged causal prefill attention, v_mfma_f32_32x32x16; one workgroup per item at 4 x 704, persistent workgroups for the two launches under other_workloads)",
            "achieved": round(tf, 1), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / MFMA_PEAK_TFLOPS, 4),
            "traffic": None, "avg_launch_us": round(us, 2), "algorithmic_flops_per_launch": flops,
            "workload": f"{n_seqs} sequences x {n_tokens} new tokens, H = {H}, D = {D}, block_size {bs}",
            "timing": f"hipGraph of {launches} launches, mean of {reps} replays, HIP events",
            "pmc": "profiles/r4_attn_prefill_pmc.json (SQ_VALU_MFMA_BUSY_CYCLES, LDS bank conflicts)"}


def prefill_attention_object(shape, dtype, dev):
    """The 4 x 704 launch (the prefill of 4 of the benchmark's requests) as the object's headline, and the two launches the
    serving legs actually make beside it: all 32 prompts admitted at once, and a 2048-token chunk of a 4096-token prompt."""
    obj = time_prefill_attention(shape, dtype, dev)
    obj["other_workloads"] = [time_prefill_attention(shape, dtype, dev, n_seqs=32, launches=4, brief=True),
                              time_prefill_attention(shape, dtype, dev, n_seqs=1, n_tokens=2048, kv_tokens=4096, launches=6, brief=True)]
    obj["in_kernel_shader_clock_GHz"] = "1.85-1.96 (profiles/r4_attn_prefill_pmc.json): the MFMA peak at that clock is 1.9-2.0 PFLOP/s"
    return obj


def roofline_objects(model, runner, ctxs, ms_per_step, args, model_name, with_gemm=True):
    """`roofline` (decode attention kernel), `roofline_gemm`, `whole_step` for one timed leg."""
    B = runner.cfg.batch
    ctxs_per_step = [[c] * B for c in ctxs]
    attn_bytes = sum(runner.attention_bytes(c) for c in ctxs_per_step) / len(ctxs)
    attn_ms = time_attention_kernel(runner, ctxs)
    attn_gbs = attn_bytes / (attn_ms * 1e-3) / 1e9
    step_bytes = sum(runner.step_bytes(sum(c)) for c in ctxs_per_step) / len(ctxs)
    step_gbs = step_bytes / (ms_per_step * 1e-3) / 1e9
    traffic, traffic_src = measured_traffic(args, model_name, attn_bytes)
    roofline = {"bound": "hbm",
                "kernel": "attn_decode_kernel<BF16,128,4,nt,fused> (qkv split-K reduce + RoPE + cache append "
                          "+ paged decode attention)" if model.fuse_decode_attention else
                          "attn_decode_kernel (paged decode attention)",
                "achieved": round(attn_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(attn_gbs / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
                "avg_launch_us": round(attn_ms * 1e3, 2), "timing": "STANDALONE launches: the timed contexts' attention launches back to back in their own hipGraph, mean "
                          "over launches and 3 replays, HIP events on the launch stream.  Inside the real decode step "
                          "(behind the qkv GEMM) the same launch is shorter — see profiles/ (rocprofv3 kernel trace of "
                          "this command: r3 70.6 us in-step vs 78.2 us standalone); this line is the conservative one",
                "algorithmic_bytes_per_launch": int(attn_bytes)}
    roofline_gemm = None
    gemm_t = time_decode_gemms(runner) if with_gemm else None
    if gemm_t:
        gemm_kernels = gemm_t.pop("_kernels")
        wb = sum(v["weight_bytes"] for v in gemm_t.values())
        us = sum(v["us"] for v in gemm_t.values())
        roofline_gemm = {"bound": "hbm", "kernel": gemm_kernels + ": qkv + o + gate|up + down of one layer, as the "
                                                   "decode step launches them",
                         "achieved": round(wb / us / 1e3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(wb / us / 1e3 / HBM_PEAK_GBS, 4), "traffic": None, "traffic_source": None,
                         "weight_bytes_per_layer": wb, "us_per_layer": round(us, 2),
                         "per_projection": {k: {"us": v["us"], "GBps": round(v["weight_bytes"] / v["us"] / 1e3, 1)}
                                            for k, v in gemm_t.items()},
                         "what": "algorithmic bytes = the weights; HIP events (mean of 3 replays) over one graph "
                                 "walking all layers' weights (cold), one launch per layer and projection"}
        roofline_gemm["traffic"], roofline_gemm["traffic_source"] = measured_gemm_traffic(args, model_name, wb)
    ins = in_step_attention(args, model_name)
    if ins:
        roofline.update(ins)
    whole = {"algorithmic_bytes": int(step_bytes), "achieved_GBps": round(step_gbs, 1),
             "frac_of_hbm_peak": round(step_gbs / HBM_PEAK_GBS, 4), "weight_bytes": model.weight_bytes(),
             "weight_bytes_resident": model.weight_bytes_resident()}
    return roofline, roofline_gemm, whole


def null_step_object(model, runner, ctxs, ms_per_step, reps=5, grid_wgs=256):
    """`whole_step.null_step` — the ceiling of the step's LAUNCH STRUCTURE on this GPU in this run (round-4 review, item 1a).
    The decode step replayed as a launch plan in which every launch of a layer is replaced by a math-free stand-in over
    the SAME bytes with the SAME grid: the paged-read probe over the layer's real KV pages with the real block table
    (hx_measure_paged_read: (head, sequence) workgroups, the attention kernel's loads, nothing else) and the read-stream
    probe over the real packed weights of o / gate|up / down / qkv (hx_measure_read_grid, one workgroup per CU like the
    real launches) — no activations, no arithmetic, no hand-over, no stores; the step's edges (step head, final norm,
    library lm_head GEMM, argmax) are the REAL kernels on scratch buffers.  One plan per timed context (its tile count),
    replayed in the timed order, HIP events around each pass, median of `reps` passes.  built / null says how much of what
    a 5-launch layer can reach the built step reaches; `null_step_best_grid` is the same with 512 workgroups per weight
    launch (the probe's best shape)."""
    import statistics
    from hydrainfer_amd import _lib, launch_plan
    from hydrainfer_amd._C.kernel.norm import add_rms_norm_slabs, argmax_rows, decode_step_head
    lib = _lib.lib()
    sh, dev, dt = model.shape, runner.dev, model.dtype
    B, bs = runner.cfg.batch, runner.cfg.block_size
    L, H, HK, D, hid = sh.num_hidden_layers, sh.num_attention_heads, sh.num_key_value_heads, sh.head_dim, sh.hidden_size
    if HK != H or D * runner.pool.element_size() != 256:
        return None
    e = runner.pool.element_size()
    page_bytes, row_bytes = bs * HK * D * e, HK * D * e
    sink = torch.zeros(4, dtype=torch.float32, device=dev)

    def weight(l, n):
        t = model.packed_x.get(f"l{l}.{n}")
        return t if t is not None else model.packed[f"l{l}.{n}"]

    def read(t, wgs):
        nbytes = t.numel() * t.element_size()
        _lib.check(lib.hx_measure_read_grid(t.data_ptr(), nbytes - nbytes % 8192, wgs, sink.data_ptr(), _lib.current_stream()), "read_grid")

    ids = torch.randint(1000, 30000, (B,), device=dev)
    slabs = torch.zeros((1, B, hid), dtype=torch.float32, device=dev)
    w_lm = model.state["lm_head"]

    def record(tiles, wgs):
        plan = launch_plan.LaunchPlan(dev)

        def body():
            sync = model._new_sync(dev)
            h, x0 = decode_step_head(ids, model.state["embed"], model.state["l0.norm1"], sh.rms_norm_eps, zero=sync, head=None)
            read(weight(0, "wqkv"), wgs)
            for l in range(L):
                _lib.check(lib.hx_measure_paged_read(runner.pool[l, 0].data_ptr(), runner.pool[l, 1].data_ptr(),
                                                     runner.block_table.data_ptr(), runner.blocks_per_seq, B, H, tiles,
                                                     page_bytes, row_bytes, 256, sink.data_ptr(), _lib.current_stream()), "paged_read")
                read(weight(l, "wo"), wgs)
                read(weight(l, "wgu"), wgs)
                read(weight(l, "wdown"), wgs)
                if l + 1 < L:
                    read(weight(l + 1, "wqkv"), wgs)
            x = torch.empty_like(h)
            add_rms_norm_slabs(x, h, slabs, 1, model.state["norm"], sh.rms_norm_eps)
            logits = torch.empty((B, w_lm.shape[0]), dtype=dt, device=dev)
            launch_plan.host_op(lambda: torch.matmul(x, w_lm.t(), out=logits))
            argmax_rows(logits, None)
        plan.capture(body)
        return plan

    def timed(wgs):
        plans = {}
        for c in ctxs:
            t = (c + bs - 1) // bs
            if t not in plans:
                plans[t] = record(t, wgs)
        order = [plans[(c + bs - 1) // bs] for c in ctxs]
        for p_ in order[:2]:
            p_.replay()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for p_ in order:
                p_.replay()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / len(ctxs))
        n = order[0].n_launches
        del plans, order
        return statistics.median(ts), n

    null_ms, n_launches = timed(grid_wgs)
    best_ms, _ = timed(512)
    step_bytes = sum(runner.step_bytes(c * B) for c in ctxs) / len(ctxs)
    return {"ms_per_step": round(null_ms, 4), "launches": n_launches + 1,
            "frac_of_hbm_peak": round(step_bytes / (null_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "built_over_null": round(null_ms / ms_per_step, 4),
            "null_step_best_grid_ms": round(best_ms, 4),
            "built_over_null_best_grid": round(best_ms / ms_per_step, 4),
            "what": "the same plan with every layer launch replaced by a math-free read of the same bytes on the same grid "
                    "(paged-read probe over the real KV pages + read-stream probe over the real packed weights, "
                    f"{grid_wgs} workgroups per weight launch), real step edges; built_over_null = null ms / built ms: the share of "
                    "the 5-launch structure's ceiling the built step reaches on this GPU in this run"}


def ctx_label(ctxs, passes=None):
    if passes is not None and len(passes) > 1:
        return (f"{len(ctxs)} steps in {len(passes)} passes of consecutive contexts (the generation's 705..959, the last pass "
                f"ctx {passes[-1][0]}..{passes[-1][-1]}), the state rewound between passes outside the clock")
    if len(ctxs) > 1 and ctxs[1] - ctxs[0] == 1:
        return f"ctx {ctxs[0]}..{ctxs[-1]} (consecutive steps of the generation)"
    return (f"ctx {ctxs[0]}..{ctxs[-1]} in {len(ctxs)} steps {ctxs[1] - ctxs[0] if len(ctxs) > 1 else 0} apart (mean "
            f"{sum(ctxs) / len(ctxs):.0f}; the generation's 255 decode steps see 705..959, mean 832)")


def leg_13b(ctx, args, dtype, dev, rank):
    """BASELINE configs[2] (LLaVA-1.5-13B, batch 32, decode HBM-roofline run) as a short second leg of the
    default command: same prompts / prefill / strided contexts, no CPU baseline, no serving."""
    from hydrainfer_amd.model.llama import LlamaForCausalLM
    from hydrainfer_amd.model.runner import DecodeRunner, RunnerConfig
    shape, name = model_shape("13b")
    prompt_len, n_generate = 704, 256
    cfg = RunnerConfig(batch=args.batch, prompt_len=prompt_len, n_generate=n_generate, use_graph=not args.no_graph,
                       executor=args.executor)
    model = LlamaForCausalLM.random_init(shape, dtype, dev, seed=0)
    model.use_hip_gemm = not args.lib_gemm
    model.prepare_decode(max_rows=args.batch, keep_row_major=True)
    runner = DecodeRunner(model, cfg, seed=rank)
    prompts = synth_prompts(args.batch, prompt_len, shape.vocab_size, dev)
    g = torch.Generator(device=dev).manual_seed(100 + rank)
    img = (torch.randn((args.batch, 576, shape.hidden_size), generator=g, device=dev) * 0.02).to(dtype)
    runner.prefill(prompts, img, image_token_id(shape.vocab_size))
    ctxs = timed_contexts(prompt_len, n_generate, min(args.steps_13b, n_generate - 1))
    elapsed, all_elapsed = decode_leg(ctx, model, runner, [ctxs], args.warmup, prompt_len)
    ms = elapsed / len(ctxs) * 1e3
    roofline, roofline_gemm, whole = roofline_objects(model, runner, ctxs, ms, args, name)
    if not args.no_null_step:
        try:
            whole["null_step"] = null_step_object(model, runner, ctxs, ms)
        except Exception as e:
            whole["null_step"] = {"error": repr(e)[:300]}
    whole_64 = None
    if not args.no_serving_64:
        # configs[4]'s D nodes hold 13B batches of 33 .. 64 rows: round 5 runs them on the wide activations-in-registers
        # kernel over the SAME packing (k-steps per wave 40 -> 20, 27 -> 14 + 13): 6 launches per layer, no third copy
        try:
            whole_64 = leg_64_rows(ctx, model, args, dev, prompt_len, n_generate)
        except SystemExit:
            raise
        except Exception as e:
            whole_64 = {"error": repr(e)[:300]}
    return {"workload": f"{name}-shaped random weights, batch {args.batch} decode, paged KV block_size=16, "
                        f"{ctx_label(ctxs)} (BASELINE configs[2]: 13B batch-32 decode HBM-roofline run)",
            "value": round(args.batch * len(ctxs) / elapsed, 2), "unit": "tokens/s", "steps": len(ctxs),
            "ms_per_step": round(ms, 4), **region_spread(all_elapsed, len(ctxs)), "roofline": roofline, "roofline_gemm": roofline_gemm, "whole_step": whole,
            "whole_step_64": whole_64}


def leg_13b_child(args):
    """The 13B leg in a FRESH process (started only after this one has released the 7B model): `python bench.py --model 13b`
    with this run's flags, its one JSON line reshaped to leg_13b's object.  Why a child: weights allocated behind the 7B
    legs' allocations and frees stream 1.5-3 % slower through the same GEMM kernels than in a process that allocated them
    first (profiles/r6_13b_alone_vs_after7b.md: gate|up 51.7 against 50.1 us, attention unchanged) — an engine holds ONE
    model from start-up, so the fresh process is the case to quote.  The child is spawned, never exec'd."""
    cmd = [sys.executable, os.path.abspath(__file__), "--model", "13b", "--as-13b-leg", "--gpus", "1",
           "--steps", str(args.steps_13b), "--warmup", str(args.warmup), "--batch", str(args.batch), "--dtype", args.dtype,
           "--executor", args.executor, "--full", "--no-cpu-baseline", "--no-serving", "--no-ttft", "--no-ragged"]
    for flag in ("no_graph", "lib_gemm", "no_fused_attention", "no_ranked", "no_null_step", "no_serving_64"):
        if getattr(args, flag):
            cmd.append("--" + flag.replace("_", "-"))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
    lines = [l for l in r.stdout.decode(errors="replace").splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"13B child exited {r.returncode}: {r.stderr.decode(errors='replace')[-300:]}")
    d = json.loads(lines[-1])
    leg = {"workload": d["config"]["workload"], "process": "child: python bench.py --model 13b (fresh process, after this one "
                                                           "released the 7B model)"}
    for k in ("value", "unit", "steps", "ms_per_step", "timed_regions", "ms_per_step_min", "ms_per_step_max", "ms_per_step_all",
              "roofline", "roofline_gemm", "whole_step", "whole_step_64"):
        if k in d:
            leg[k] = d[k]
    return leg


def main():
    args = parse()
    launch_ranks_if_needed(args)             # N > 1 without WORLD_SIZE: this process only starts the ranks
    if args.dry_run:
        return dry_run(args)
    if os.environ.get("HX_BENCH_WATCHDOG"):      # diagnose hangs: periodic stack dumps
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["HX_BENCH_WATCHDOG"]), repeat=True)
    from hydrainfer_amd import parallel
    ctx = parallel.init_from_env()
    world, rank, local_rank = ctx.world_size, ctx.rank, ctx.local_rank
    n_gpus = world
    if os.environ.get("HX_SINGLE_DEVICE") == "1":   # test mode: all ranks share cuda:0
        local_rank = 0
    dev = torch.device(f"cuda:{local_rank}")
    torch.cuda.set_device(dev)

    from hydrainfer_amd import _lib
    from hydrainfer_amd.model.llama import LlamaForCausalLM
    from hydrainfer_amd.model.runner import DecodeRunner, RunnerConfig
    _lib.lib()   # no library, no benchmark
    if args.no_ranked:
        _lib.check(_lib.lib().hx_debug_set_option(b"decode_ranked", 0), "decode_ranked")

    shape, model_name = model_shape(args.model)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    prompt_len, n_generate = 704, 256
    steps = args.steps
    passes = timed_passes(prompt_len, n_generate, steps)
    ctxs = [c for p in passes for c in p]
    cfg = RunnerConfig(batch=args.batch, prompt_len=prompt_len, n_generate=n_generate,
                       use_graph=not args.no_graph, executor=args.executor)
    # the GPU's streaming rates, measured FIRST: at the end of a run the heap is fragmented and a fresh 1 GiB buffer reads
    # 20 % slower than the decode step itself streams (5.3 against 6.6-6.7 TB/s at the start: profiles/r5_kv_pool_placement.md)
    stream_rates = (round(read_stream_ceiling_gbs(dev), 1), round(copy_ceiling_gbs(dev), 1)) if args.full else None
    model = LlamaForCausalLM.random_init(shape, dtype, dev, seed=0)
    model.use_hip_gemm = not args.lib_gemm
    if args.no_fused_attention:
        model.fuse_decode_attention = False
    # every decode-side weight layout this run can need is built NOW (never in the middle of serving); the
    # serving / TTFT legs prefill on this GPU, so the row-major tensors stay for the library prefill GEMMs
    model.prepare_decode(max_rows=args.batch, keep_row_major=True)
    runner = DecodeRunner(model, cfg, seed=rank)
    resident_headline = model.weight_bytes_resident()      # before the 64-request serving leg adds its layouts

    # multi-GPU: exchange IPC handles and map the neighbour's pool NOW — before any hipGraph is
    # captured (mapping a peer allocation after graphs were instantiated wedged in a 2-process
    # test) — bounded by a watchdog so a driver problem cannot cost the benchmark line
    peer_info, ipc_stuck = None, False
    vision = pixels = engine = None
    if not (args.skip_prefill or (args.no_ttft and args.no_serving and (world == 1 or args.no_disaggregated))):
        vision, pixels = make_vision(shape, dtype, dev)
    engine_error = None
    if world > 1 and not args.no_disaggregated and vision is not None and not args.no_migration:
        try:      # an optional leg must never cost the benchmark line
            engine = build_rank_engine(ctx, model, vision, shape, dtype, dev, args.batch, prompt_len - 576, n_generate)
        except Exception as e:
            engine, engine_error = None, repr(e)[:300]
        # every rank must agree on whether the leg runs (its collectives involve all of them)
        if ctx.sum_over_ranks(0.0 if engine is not None else 1.0, dev) > 0:
            engine = None
    if world > 1 and not args.no_migration:
        import threading
        box = {}

        def _exchange():
            torch.cuda.set_device(dev)        # the current device is per thread; new threads start on 0
            from hydrainfer_amd._C.data_transfer import block_migration as bm
            n_blk = (prompt_len + cfg.block_size - 1) // cfg.block_size
            infos = ctx.all_gather_object({"handle": bm.get_ipc_mem_handle(runner.pool),
                                           "table": runner.tables[0][:n_blk], "n_blocks": runner.pool.shape[2]})
            peer = infos[parallel.migration_peer(ctx.rank, ctx.world_size)]
            bm._open(peer["handle"])          # cached mapping; later calls are lookups
            box["peer"] = peer
            if engine is not None:            # pools this rank will pull from: E image pools for P, P kv pools for D
                node = engine.node
                mine = {"kv": node.kv_cache_block_manager.memory_handle if node.kv_cache_block_manager else None,
                        "image": node.image_cache_block_manager.memory_handle if node.image_cache_block_manager else None}
                pools = ctx.all_gather_object(mine)
                for r, role in enumerate(engine.roles):
                    if r == ctx.rank:
                        continue
                    if node.node_type.enable_prefill and "E" in role and pools[r]["image"]:
                        bm._open(pools[r]["image"])
                    if node.node_type.enable_decode and "P" in role and pools[r]["kv"]:
                        bm._open(pools[r]["kv"])
        th = threading.Thread(target=_exchange, daemon=True)
        th.start()
        th.join(timeout=60)
        ipc_stuck = th.is_alive()
        peer_info = box.get("peer")

    prompts = synth_prompts(args.batch, prompt_len, shape.vocab_size, dev)
    ttft_ms = None
    if args.skip_prefill:
        runner.set_state(prompt_len, prompts[:, -1])
    else:
        g = torch.Generator(device=dev).manual_seed(100 + rank)
        img = (torch.randn((args.batch, 576, shape.hidden_size), generator=g, device=dev) * 0.02).to(dtype)
        runner.prefill(prompts, img, image_token_id(shape.vocab_size))   # also warms every kernel / GEMM heuristic
        if args.full:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner.prefill(prompts, img, image_token_id(shape.vocab_size))
            torch.cuda.synchronize()
            ttft_ms = (time.perf_counter() - t0) * 1e3   # prefill of the whole 32-request batch

    # ---- warmup (untimed: graph capture + W steps, state rewound) and the timed region
    elapsed, all_elapsed = decode_leg(ctx, model, runner, passes, args.warmup, prompt_len,
                                      regions=TIMED_REGIONS if args.full else 1)
    ms_per_step = elapsed / steps * 1e3
    tokens = args.batch * steps * n_gpus
    value = tokens / elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(runner, args.dump_outputs)
    configs_i = {"7b": "configs[1]: LLaVA-1.5-7B bf16, collocated prefill+decode on 1 MI355X",
                 "13b": "configs[2]: LLaVA-1.5-13B, batch 32, decode HBM-roofline run"}.get(args.model, "smoke shape")
    headline = {
        "metric": "decode output tokens/s, LLaVA-1.5-7B image+text requests (576 image + 128 text "
                  "prompt, 256 generated), batch 32 per GPU" if args.model == "7b" else
                  f"decode output tokens/s, {model_name}, batch {args.batch} per GPU",
        "value": round(value, 2), "unit": "tokens/s", "n_gpus": n_gpus, "steps": steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), **region_spread(all_elapsed, steps),
        "timing": (f"{len(all_elapsed)} timed regions of exactly {steps} steps each behind one warm-up, every one bracketed by "
                   "barrier + synchronize and reduced with MAX over ranks; value and ms_per_step are the MEDIAN region's"
                   if len(all_elapsed) > 1 else
                   f"one timed region of exactly {steps} steps behind the warm-up, bracketed by barrier + synchronize and "
                   "reduced with MAX over ranks"),
        "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"{model_name}-shaped random weights, batch {args.batch} "
                               f"decode, paged KV block_size=16, {ctx_label(ctxs, passes)} (BASELINE {configs_i})",
                   "global_batch": args.batch * n_gpus, "prompt_tokens": prompt_len,
                   "generated_tokens": n_generate,
                   "hip_graph": cfg.use_graph and runner.executor_used == "graph",
                   # the executor that REALLY replayed the step (a plan falls back to the hipGraph when the step
                   # holds torch ops, e.g. --lib-gemm: launch_plan.PlanNotRecordable)
                   "step_executor": runner.executor_used if cfg.use_graph else "eager",
                   "parallelism": f"replicas x{n_gpus} (independent requests, no data-path collective)"},
    }
    if not args.full:      # a plain run ends with its headline
        if rank == 0:
            print(json.dumps(headline), flush=True)
        ctx.shutdown()
        return

    # The prefill side of the TTFT and serving legs is library GEMM (82 % of a single request's TTFT, 24 of the 29 ms of a
    # 2048-token chunk): an engine tunes the four projections for its configured prompt length and chunk budget ONCE at
    # start-up (torch's TunableOp over the library's own kernels, switched off again behind the pass — engine/serve.py).
    # Only the decoder's projections: the same pass over the vision tower for 8 images ends in a GPU memory fault inside a
    # candidate kernel of the library (tools/probes/tune_probe.py, profiles/rejected.md).  N = 1 only; TunableOp is
    # disabled again behind the two legs (the decode loop timed above and the legs below run the library's defaults).
    tuned = None
    if (world == 1 and vision is not None and not args.no_tune and not args.skip_prefill and args.model == "7b"
            and not (args.no_ttft and args.no_serving)):
        try:
            from hydrainfer_amd.engine.serve import tune_library_gemms
            tuned = tune_library_gemms(model, rows=(prompt_len,) if args.no_serving else (prompt_len, 2048))
        except Exception as e:      # a convenience of the library, never the benchmark's problem
            tuned = {"error": repr(e)[:200]}
    ttft = None if args.skip_prefill or args.no_ttft else measure_ttft(runner, prompts, shape, dtype, dev, rank,
                                                                         vision, pixels)
    if ttft is not None:
        ttft["library_gemms_tuned"] = tuned
    serving = None
    if rank == 0 and world == 1 and vision is not None and not args.no_serving:
        serving = measure_serving(model, vision, pixels, shape, dtype, dev, args.batch, prompt_len - 576, n_generate)
        if not args.no_serving_64:
            # twice as many requests at once: decode batches of 33 .. 64 rows leave the 5-launch layer (x for 64 rows does
            # not fit the registers of the activations-in-registers GEMM) for the LDS-slice GEMMs with separate norm /
            # silu launches (13B) resp. the 6-launch wide layer (7B) — DESIGN.md section 4
            serving["twice_the_batch"] = measure_serving(model, vision, pixels, shape, dtype, dev, 2 * args.batch,
                                                         prompt_len - 576, n_generate)
    if tuned is not None:
        if serving is not None:
            serving["library_gemms_tuned"] = tuned
        try:
            torch.cuda.tunable.enable(False)
        except Exception:
            pass
    whole_64 = None
    if rank == 0 and world == 1 and (args.model == "7b" or args.as_13b_leg) and not args.no_serving_64:
        try:
            whole_64 = leg_64_rows(ctx, model, args, dev, prompt_len, n_generate)
        except SystemExit:
            raise
        except Exception as e:      # an extra leg must never cost the headline
            whole_64 = {"error": repr(e)[:300]}
    # ---- roofline of the dominant hand-written kernel + whole-step fraction (rank 0)
    out = whole_ragged = None
    if rank == 0:
        mid_ctx = int(round(sum(ctxs) / len(ctxs)))
        roofline, roofline_gemm, whole = roofline_objects(model, runner, ctxs, ms_per_step, args, model_name)
        whole["weight_bytes_resident"] = resident_headline
        if not args.no_null_step:
            try:
                whole["null_step"] = null_step_object(model, runner, ctxs, ms_per_step)
            except Exception as e:      # a measurement aid must never cost the headline
                whole["null_step"] = {"error": repr(e)[:300]}
        whole["weight_layouts"] = ("row-major (the library prefill GEMMs of this EPD replica) + one decode layout per projection "
                                   "(activations-in-registers; LDS-slice for o and layer 0's qkv); a D-role node keeps only the "
                                   "decode layout; serving 33..64 rows adds LDS-slice copies: serving.twice_the_batch.weight_bytes_resident")
        if world == 1 and not args.no_ragged:
            try:
                whole_ragged = leg_ragged(model, runner, args)
            except SystemExit:
                raise
            except Exception as e:      # an extra leg must never cost the headline
                whole_ragged = {"error": repr(e)[:300]}
        roofline["measured_read_stream_ceiling_GBps"] = stream_rates[0]      # (measured before the model was built)
        roofline["measured_copy_GBps"] = stream_rates[1]     # torch copy_ (read + write): NOT a ceiling
        out = {
            **headline,
            "roofline": roofline,
            "roofline_gemm": roofline_gemm,
            "roofline_prefill_attention": None if args.skip_prefill else prefill_attention_object(shape, dtype, dev),
            "whole_step": whole,
            "whole_step_64": whole_64,
            "whole_step_ragged": whole_ragged,
            "prefill_batch_ms": None if ttft_ms is None else round(ttft_ms, 2),
            "ttft": ttft, "serving": serving, "migration": None,
        }
        if not args.no_cpu_baseline and world == 1:   # CPU baseline: rank 0 at N=1 only
            try:
                out["parity_probe"] = parity_probe(dtype, dev, args.executor) if args.model == "7b" else None
            except Exception as e:      # evidence, not the headline
                out["parity_probe"] = {"error": repr(e)[:300]}
            out["cpu_baseline"] = cpu_baseline(shape, dtype, args.batch, mid_ctx, args.cpu_layers)
            cb = out["cpu_baseline"]
            if args.cpu_full:
                full = cpu_config0_full(shape, dtype, cb["cores"])
                ex = cb["config0"]
                cb["config0_full"] = full
                if isinstance(ex.get("clip_encode_s"), (int, float)):
                    cb["full_over_extrapolated"] = {
                        "clip_encode": round(full["clip_encode_s"] / ex["clip_encode_s"], 3),
                        "prefill": round(full["prefill_s"] / ex["prefill_s"], 3),
                        "decode_tokens_per_s": round(full["decode_tokens_per_s"] / ex["decode_tokens_per_s"], 3)}
            else:
                # the measured relation of the two on an MI355X box's host (profiles/, `--cpu-full`), for the reader of a default line
                try:
                    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r5_cpu_config0_full.json")))
                    cb["full_over_extrapolated"] = dict(ref["full_over_extrapolated"], source="profiles/r5_cpu_config0_full.json "
                                                        "(python bench.py --cpu-full on an MI355X box; not re-measured in this run)")
                except Exception:
                    pass
    # ---- optional last leg on every rank (nothing touches the GPU after it)
    migration, stuck = None, ipc_stuck
    if world > 1 and not args.no_migration:
        if ipc_stuck or peer_info is None:
            migration = {"error": "mapping the neighbour's pool (hipIpcOpenMemHandle) did not return within 60 s"}
        else:
            import threading
            box = {}
            th = threading.Thread(target=lambda: box.update(r=measure_migration(ctx, runner, dev, peer_info)),
                                  daemon=True)
            th.start()
            th.join(timeout=90)
            stuck = th.is_alive()
            migration = {"error": "timed out after 90 s"} if stuck else box.get("r")

    disagg = None
    if engine is not None and not stuck:
        import threading
        box = {}

        def _leg():
            try:
                box["r"] = measure_disaggregated(ctx, engine, shape, dev, pixels, args.batch, prompt_len - 576,
                                                 n_generate, args.rate)
            except Exception as e:      # never let the optional leg break the benchmark line
                box["r"] = {"error": repr(e)[:300]}
        th = threading.Thread(target=_leg, daemon=True)
        th.start()
        # three replays (warm-up, burst, Poisson) with deadline_s = 150 each + the warm-ups in front of them: a slow but
        # healthy leg must not be declared wedged (round-4 ADVICE)
        th.join(timeout=3 * 150 + 120)
        stuck = th.is_alive()
        disagg = {"error": "timed out after 570 s"} if stuck else box.get("r")

    # ---- LLaVA-1.5-13B leg (BASELINE configs[2]) in the same line: N = 1, 7B model, default flags only
    llava_13b = None
    if world == 1 and args.model == "7b" and not args.no_13b and not stuck:
        try:
            del runner, serving
            engine = vision = None
            model.release()
            del model
            import gc
            gc.collect(); torch.cuda.empty_cache()
            print(f"[bench] before the 13B leg: {torch.cuda.memory_allocated() / 2**30:.2f} GiB allocated, "
                  f"{torch.cuda.memory_reserved() / 2**30:.2f} GiB reserved", file=sys.stderr)
            if args.leg_13b_in_process:
                llava_13b = dict(leg_13b(ctx, args, dtype, dev, rank), process="this one, behind the 7B legs")
            else:
                try:
                    llava_13b = leg_13b_child(args)
                except Exception as e:      # e.g. a sandbox without child processes: the in-process leg, and say so
                    llava_13b = dict(leg_13b(ctx, args, dtype, dev, rank),
                                     process=f"this one, behind the 7B legs (the child process failed: {repr(e)[:200]})")
        except SystemExit:
            raise
        except Exception as e:      # an extra leg must never cost the headline
            llava_13b = {"error": repr(e)[:300]}

    # ---- every rank's view of the optional legs, folded into the ONE line before rank 0 prints it (round-4 ADVICE: a wedge
    # on rank k != 0 used to leave a clean line).  Exchanged through the TCPStore — no collective, so it works while a HIP
    # call is wedged in a helper thread of some rank; a rank that does not report within 120 s counts as wedged.
    mine = {"stuck": bool(stuck), "failed": []}
    if ipc_stuck:
        mine["failed"].append({"leg": "peer mapping", "error": "hipIpcOpenMemHandle did not return within 60 s"})
    if isinstance(migration, dict) and "error" in migration:
        mine["failed"].append({"leg": "migration", "error": str(migration["error"])[:200]})
    if engine_error is not None:
        mine["failed"].append({"leg": "disaggregated", "error": engine_error[:200]})
    elif isinstance(disagg, dict) and "error" in disagg:
        mine["failed"].append({"leg": "disaggregated", "error": str(disagg["error"])[:200]})
    if isinstance(llava_13b, dict) and "error" in llava_13b:
        mine["failed"].append({"leg": "llava_13b", "error": str(llava_13b["error"])[:200]})
    views = ctx.gather_via_store("bench_legs", json.dumps(mine))
    wedged_ranks = [r for r, v in enumerate(views) if v is None or json.loads(v)["stuck"]]
    if rank == 0:
        out["migration"] = migration
        out["disaggregated"] = disagg if engine_error is None else {"error": engine_error}
        out["llava_13b"] = llava_13b
        # a reader of this line must treat a non-empty legs_failed / wedged_ranks as RED for those legs: the headline
        # (value, roofline, whole_step) was measured before any of them ran and stands
        out["legs_failed"] = [dict(f, rank=r) for r, v in enumerate(views) if v is not None for f in json.loads(v)["failed"]]
        for extra in ("whole_step_64", "whole_step_ragged", "serving", "parity_probe"):
            if isinstance(out.get(extra), dict) and "error" in out[extra]:
                out["legs_failed"].append({"leg": extra, "error": str(out[extra]["error"])[:200], "rank": 0})
        out["wedged_ranks"] = wedged_ranks
        print(json.dumps(out), flush=True)
    # A HIP call wedged in the helper thread of an OPTIONAL leg (peer mapping / migration / E-P-D replay) on ANY rank: the
    # headline line above is complete and names the wedged ranks and legs; collective teardown would hang behind the
    # wedged thread, so EVERY rank leaves without it (agreed through the TCPStore above: a rank that exited alone would
    # leave the others in the final barrier) — with status 3: a hung HIP call is a failure of the run.
    # HX_BENCH_WEDGE_OK=1 opts in to status 0 (keep a scaling point whose optional leg hung).
    if wedged_ranks:
        if stuck:
            print(f"bench.py: rank {rank}: an optional multi-GPU leg is wedged (see the line's legs_failed / wedged_ranks)",
                  file=sys.stderr, flush=True)
        sys.stdout.flush()
        os._exit(0 if os.environ.get("HX_BENCH_WEDGE_OK") == "1" else 3)
    ctx.shutdown()


if __name__ == "__main__":
    main()
