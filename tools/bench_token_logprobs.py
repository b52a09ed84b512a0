#!/usr/bin/env python3
"""What prompt log-probabilities cost a prefill chunk.

    python tools/bench_token_logprobs.py [--reps 30] [--burst 5] [--out profiles/token_logprob_rows.md]

Microseconds per launch of hx_token_logprob_rows (the log-softmax value of a GIVEN id per row, its rank and the K most
likely entries of the row) for rows in {64, 512, 2048}, n = 32064 (LLaVA-1.5's vocabulary), K in {0, 5}, fp16 and bf16:
 * the new launch in both forms (hx_token_logprob_rows_ex): the pass straight from global memory and the row staged in
   LDS first — for K > 0 both stage nothing different: form 1 runs the selection rounds from global memory (L2);
 * hx_logprob_rows on the same rows (the kernel of the parent commit: this change does not touch it): the same traffic,
   a different answer (the argmax's score);
 * the torch sequence it replaces: log_softmax(logits.float(), -1), a gather, [topk(K)] and the rank as a comparison
   count (values greater, or equal with a lower index).

The variants ALTERNATE inside every repetition; a repetition times a burst of launches of one variant between two device
events and divides by the burst length; medians and quartiles over the repetitions.  The 2048-row cases also state
bytes / time — the logits read once — beside the 8 TB/s of the memory's specification.

Then a 2048-token text prefill of a model with LLaVA-1.5-7B's widths and vocabulary and 2 layers, with and without
scoring every position (K = 0): what scoring adds to a chunk — the last layer's MLP and the lm_head over all rows instead
of one, and the launch.  The difference is the figure; it does not depend on the number of layers in front.

No number here is a threshold."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 32064
PEAK_TBS = 8.0


def torch_sequence(logits, targets, k):
    x = logits.float()
    lsm = torch.log_softmax(x, dim=-1)
    t = targets.long()[:, None]
    lp = lsm.gather(1, t)
    zt = x.gather(1, t)
    idx = torch.arange(x.shape[1], device=x.device)[None, :]
    rank = ((x > zt) | ((x == zt) & (idx < t))).sum(-1)
    return (lp, rank) if k == 0 else (lp, rank, torch.topk(lsm, k, dim=-1))


def measure(variants, reps, burst):
    for _ in range(2):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(burst):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / burst)
    return times


def prefill_steps(lines, reps, tokens=2048):
    from hydrainfer_amd._C.kernel.norm import argmax_rows, token_logprob_rows, token_logprob_rows_packed
    from hydrainfer_amd.layer.causal_attention import AttentionParametersBuilder
    from hydrainfer_amd.memory.kv_cache import KVCache
    from hydrainfer_amd.model.llama import LanguageModelParameters, LlamaForCausalLM, LlamaShape
    lines += ["", f"## A {tokens}-token text prefill: milliseconds (2 layers of LLaVA-1.5-7B's widths, vocabulary 32064, fp16)",
              "", "| step | median | q1 | q3 | minus the plain step (us) |", "|---|---|---|---|---|"]
    dev, bs = torch.device("cuda:0"), 16
    shape = LlamaShape(4096, 11008, 2, 32, 32, 128, N)
    model = LlamaForCausalLM.random_init(shape, torch.float16, dev, seed=3)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 32000, (tokens,), generator=g, dtype=torch.int32).to(dev)
    pos = torch.arange(tokens, dtype=torch.int32, device=dev)
    targets = torch.cat([ids[1:], torch.full((1,), -1, dtype=torch.int32, device=dev)]).contiguous()
    n_blocks = tokens // bs
    pools = [(torch.zeros((n_blocks, bs, 32, 128), dtype=torch.float16, device=dev),
              torch.zeros((n_blocks, bs, 32, 128), dtype=torch.float16, device=dev)) for _ in range(2)]

    def params(selected):
        b = AttentionParametersBuilder(32, 32, 128, bs, dev)
        b.add_request(tokens, tokens, list(range(tokens)), list(range(n_blocks)))
        for k, v in pools:
            b.add_kv_cache(KVCache(k, v))
        return LanguageModelParameters(attention_params=b.build_attention_parameters(), all_sequences_decode=False,
                                       selected_token_ids=selected)
    last, every = torch.tensor([tokens - 1], device=dev), torch.arange(tokens, device=dev)

    def plain():
        return model.forward(ids, pos, params(last)).tolist()

    def scoring():
        logits = model.forward_logits(ids, pos, params(every))
        packed = token_logprob_rows_packed(token_logprob_rows(logits, targets, 0)[0], 0)
        token = argmax_rows(logits.index_select(0, last)).tolist()
        return token, packed.cpu()
    variants = [("plain (the last row through the last MLP and the lm_head)", plain),
                ("scoring every position, K = 0 (all rows through them + hx_token_logprob_rows + one more copy)", scoring)]
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
        lines.append(f"| {name} | {med:.3f} | {q[0]:.3f} | {q[2]:.3f} | {(med - base) * 1e3:+.0f} |")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    from hydrainfer_amd._C.kernel.norm import (logprob_rows, logprob_rows_bytes, token_logprob_rows,
                                               token_logprob_rows_bytes)
    lines = ["# hx_token_logprob_rows: microseconds per launch, n = 32064", "",
             "`python " + " ".join(["tools/bench_token_logprobs.py"] + sys.argv[1:]) + "`", "",
             "| dtype | rows | K | variant | median | q1 | q3 | TB/s (share of 8) |", "|---|---|---|---|---|---|---|---|"]
    for dname, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        for rows in (64, 512, 2048):
            g = torch.Generator().manual_seed(rows)
            logits = (4.0 * torch.randn((rows, N), generator=g)).to(dt).cuda()
            targets = torch.randint(0, N, (rows,), generator=g, dtype=torch.int32).cuda()
            for k in (0, 5):
                out = torch.empty(token_logprob_rows_bytes(rows, k), dtype=torch.uint8, device="cuda")
                out_lp = torch.empty(logprob_rows_bytes(rows, k), dtype=torch.uint8, device="cuda")
                variants = [("token_logprob_rows, from global memory", lambda: token_logprob_rows(logits, targets, k, out, form=1)),
                            ("token_logprob_rows, staged in LDS", lambda: token_logprob_rows(logits, targets, k, out, form=2)),
                            ("logprob_rows (the argmax's score)", lambda: logprob_rows(logits, k, out_lp)),
                            ("torch log_softmax(float)+gather+rank" + ("+topk" if k else ""),
                             lambda: torch_sequence(logits, targets, k))]
                times = measure(variants, args.reps, args.burst)
                for name, _ in variants:
                    q, med = statistics.quantiles(times[name], n=4), statistics.median(times[name])
                    rate = ""
                    if rows == 2048:
                        tbs = rows * N * 2 / (med * 1e-6) / 1e12
                        rate = f"{tbs:.2f} ({100 * tbs / PEAK_TBS:.0f} %)"
                    lines.append(f"| {dname} | {rows} | {k} | {name} | {med:.1f} | {q[0]:.1f} | {q[2]:.1f} | {rate} |")
                    print(lines[-1], flush=True)
    prefill_steps(lines, args.reps)
    lines.append("")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines))


if __name__ == "__main__":
    main()
