"""Writes tests/golden/g14_penalties.npz: what the reference's own process_logits
(hydrainfer/sampling/logits_processor.py) gives for a few dozen rows.  Runs on the CPU:

    HYDRA_REFERENCE=<checkout of the reference> python tests/golden/generate_penalty_golden.py

The function is called ONE ROW AT A TIME with exactly that row's history: it ignores unique_token_lens, so the padding of
a batched call would be penalised like real entries.  temperatures = 0 (the function turns that into 1), top_k = 0 (all)
and top_p = 2.0 (no cumulative probability exceeds it) make its steps 3-5 the identity — checked below: every entry
outside the history comes back bit for bit.  The function prints; the prints are captured and dropped.

Stored per row (rows concatenated): n, the logits as bf16 bits (the function gets them as fp32), the history (ids,
counts), (frequency, presence, repetition), the reference's penalised values of the history entries (fp32), and the
argmax of its output row — first NaN, else largest value, lowest index — with that maximum."""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def load_process_logits():
    root = os.environ.get("HYDRA_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not root:
        raise SystemExit("set HYDRA_REFERENCE (or pass the path) to a checkout of the reference")
    spec = importlib.util.spec_from_file_location(
        "reference_logits_processor", os.path.join(root, "hydrainfer", "sampling", "logits_processor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.process_logits


def main():
    process_logits = load_process_logits()
    g = torch.Generator().manual_seed(1414)
    out = {k: [] for k in ("n", "hist_len", "logits_bits", "hist_ids", "hist_counts", "penalties", "scores", "argmax",
                           "max", "raw_argmax")}
    penalties = [(0.5, 0.25, 1.0), (0.0, 0.0, 1.3), (1.1, -0.4, 2.0), (-0.7, 1.9, 0.6), (2.0, 2.0, 1.0), (0.0, 0.6, 1.15)]
    case = 0
    for n, variants in ((8, 3), (1000, 3), (32064, 2)):
        for h in sorted({min(h, n) for h in (0, 1, 63, 300)}):
            for v in range(variants):
                x = (3.0 * torch.randn(n, generator=g)).to(torch.bfloat16)
                raw = int(torch.argmax(x.float()))
                ids = torch.randperm(n, generator=g)[:h]
                # the raw winner inside the history in most rows (all but one variant of n = 1000): the penalties then
                # move the token
                if h > 0 and not (n == 1000 and v == 1) and raw not in ids.tolist():
                    ids[int(torch.randint(0, h, (1,), generator=g))] = raw
                counts = torch.randint(1, 9, (h,), generator=g, dtype=torch.int32)
                f, p, r = penalties[case % len(penalties)]
                case += 1
                row = x.float().clone()[None]
                with contextlib.redirect_stdout(io.StringIO()):
                    res = process_logits(row, ids[None].to(torch.int64), counts[None], torch.tensor([h]),
                                         torch.tensor([f]), torch.tensor([p]), torch.tensor([r]),
                                         torch.tensor([0.0]), torch.tensor([0]), torch.tensor([2.0]))[0]
                assert res.dtype == torch.float32 and res.shape == (n,)
                rest = torch.ones(n, dtype=torch.bool)
                rest[ids] = False
                assert torch.equal(res[rest].view(torch.int32), x.float()[rest].view(torch.int32)), "steps 3-5 were not the identity"
                assert not bool(torch.isnan(res).any())
                best = int(torch.nonzero(res == res.max())[0])
                out["n"].append(n)
                out["hist_len"].append(h)
                out["logits_bits"].append((x.float().view(torch.int32) >> 16).to(torch.int32).numpy().astype(np.uint16))
                out["hist_ids"].append(ids.numpy().astype(np.int32))
                out["hist_counts"].append(counts.numpy().astype(np.int32))
                out["penalties"].append((f, p, r))
                out["scores"].append(res[ids].numpy().astype(np.float32))
                out["argmax"].append(best)
                out["max"].append(float(res.max()))
                out["raw_argmax"].append(raw)
    moved = sum(a != b for a, b in zip(out["argmax"], out["raw_argmax"]))
    inside = sum(int(r in ids.tolist()) for r, ids in zip(out["raw_argmax"], out["hist_ids"]))
    print(f"{len(out['n'])} rows, raw argmax inside the history in {inside}, token moved in {moved}")
    np.savez_compressed(
        os.path.join(HERE, "g14_penalties.npz"),
        n=np.asarray(out["n"], dtype=np.int32), hist_len=np.asarray(out["hist_len"], dtype=np.int32),
        logits_bits=np.concatenate(out["logits_bits"]), hist_ids=np.concatenate(out["hist_ids"]),
        hist_counts=np.concatenate(out["hist_counts"]), penalties=np.asarray(out["penalties"], dtype=np.float32),
        scores=np.concatenate(out["scores"]), argmax=np.asarray(out["argmax"], dtype=np.int64),
        max=np.asarray(out["max"], dtype=np.float32), raw_argmax=np.asarray(out["raw_argmax"], dtype=np.int64))


if __name__ == "__main__":
    main()
