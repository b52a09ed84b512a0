#!/usr/bin/env python3
"""What an ALiBi decode launch costs: the unfused mha_varlen_fwd decode launch at the headline shape (B = 32, H = HK = 32,
D = 128, contexts 705..959, bf16, pages of 16) with and without slopes, and — with --baseline-lib — the same launch of a
library built from another revision (the parent commit), loaded into the SAME process beside the in-tree one.

    python tools/bench_alibi_decode.py [--baseline-lib /path/to/libhydra_hip.so] [--reps 30] [--inner 200] [--json OUT]

Method: every variant is warmed up; a repetition times `inner` back-to-back launches between two device events; the
variants ALTERNATE inside every repetition; medians over the repetitions.  The baseline is measured twice per
repetition (first and last): the distance between its two medians, and its own quartiles, are the run-to-run spread any
difference has to be read against.  The 436 MB of K / V do not fit the 256 MB last-level cache: every launch streams
from HBM.  Outputs of the variants without slopes are compared bit for bit."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hydrainfer_amd import _lib  # noqa: E402
from hydrainfer_amd.layer.alibi import alibi_slopes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: there is no CPU path to time"
    dev = torch.device("cuda:0")
    B, H, D, bs, dt = 32, 32, 128, 16, torch.bfloat16
    kv_lens = [705 + 8 * i + (6 if i % 2 else 0) for i in range(B)]      # 705 .. 959
    g = torch.Generator().manual_seed(0)
    n_blocks = sum((l + bs - 1) // bs for l in kv_lens)
    kc = torch.randn((n_blocks, bs, H, D), generator=g).to(dt).to(dev)
    vc = torch.randn((n_blocks, bs, H, D), generator=g).to(dt).to(dev)
    q = torch.randn((B, H, D), generator=g).to(dt).to(dev)
    perm = torch.randperm(n_blocks, generator=g).tolist()
    cu_b, cu_k = [0], [0]
    for l in kv_lens:
        cu_b.append(cu_b[-1] + (l + bs - 1) // bs)
        cu_k.append(cu_k[-1] + l)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    cu_q, cu_k, bt, cu_b = i32(list(range(B + 1))), i32(cu_k), i32(perm), i32(cu_b)
    slopes = alibi_slopes(H).to(dev)

    def make_args(out, with_slopes):
        a = _lib.hx_attn_args()
        a.out, a.q, a.k, a.v = out.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr()
        a.cu_seqlens_q, a.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
        a.block_table, a.cu_block_lens = bt.data_ptr(), cu_b.data_ptr()
        a.batch, a.n_heads, a.n_kv_heads, a.head_dim = B, H, H, D
        a.block_size, a.max_seqlen_q, a.max_seqlen_k, a.total_q = bs, 1, max(kv_lens), B
        a.q_row_stride, a.o_row_stride = q.stride(0), out.stride(0)
        a.k_block_stride, a.k_row_stride, a.k_head_stride = kc.stride(0), kc.stride(1), kc.stride(2)
        a.v_block_stride, a.v_row_stride, a.v_head_stride = vc.stride(0), vc.stride(1), vc.stride(2)
        a.softmax_scale, a.causal, a.dtype, a.num_splits = 1.0 / math.sqrt(D), 1, _lib.dtype_code(q), 0
        a.softcap, a.window_left, a.window_right, a.flags = 0.0, -1, -1, 0
        if with_slopes:
            a.alibi_slopes, a.alibi_batch_stride, a.flags = slopes.data_ptr(), 0, _lib.HX_ATTN_ALIBI
        return a

    new = _lib.lib()
    variants = []      # (name, library handle, args, output)

    def add(name, handle, with_slopes):
        out = torch.zeros_like(q)
        a = make_args(out, with_slopes)
        assert handle.hx_mha_varlen_fwd_workspace_bytes(ctypes.byref(a)) == 0      # 1024 pairs: one split, no scratch
        variants.append((name, handle, a, out))

    if args.baseline_lib:
        base = ctypes.CDLL(args.baseline_lib)
        base.hx_mha_varlen_fwd.restype, base.hx_mha_varlen_fwd.argtypes = ctypes.c_int, [ctypes.POINTER(_lib.hx_attn_args), ctypes.c_void_p]
        base.hx_mha_varlen_fwd_workspace_bytes.restype = ctypes.c_int64
        base.hx_mha_varlen_fwd_workspace_bytes.argtypes = [ctypes.POINTER(_lib.hx_attn_args)]
        add("baseline", base, False)       # reads the struct up to `flags`: the layout in front of the new tail is unchanged
    else:
        add("baseline", new, False)
    add("this tree, no slopes", new, False)
    add("this tree, ALiBi", new, True)
    variants.append(("baseline (again)",) + variants[0][1:])

    stream = _lib.current_stream()

    def launch(v, n):
        _, handle, a, _ = v
        for _ in range(n):
            rc = handle.hx_mha_varlen_fwd(ctypes.byref(a), stream)
            assert rc == 0, rc

    for v in variants:      # warm-up: code objects loaded, clocks up
        launch(v, 50)
    torch.cuda.synchronize()
    assert torch.equal(variants[0][3], variants[1][3]), "baseline and this tree differ without slopes"
    assert not torch.equal(variants[0][3], variants[2][3])
    times = {v[0]: [] for v in variants}
    for _ in range(args.reps):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(v, args.inner)
            e1.record()
            e1.synchronize()
            times[v[0]].append(e0.elapsed_time(e1) * 1e3 / args.inner)      # us per launch
    kv_bytes = 2 * sum(kv_lens) * H * D * 2
    res = {"shape": {"B": B, "H": H, "D": D, "ctx": [min(kv_lens), max(kv_lens)], "dtype": "bf16", "block": bs},
           "reps": args.reps, "inner": args.inner, "kv_bytes": kv_bytes, "variants": {}}
    for name, ts in times.items():
        qs = statistics.quantiles(ts, n=4)
        med = statistics.median(ts)
        res["variants"][name] = {"median_us": round(med, 3), "q1_us": round(qs[0], 3), "q3_us": round(qs[2], 3),
                                 "min_us": round(min(ts), 3), "max_us": round(max(ts), 3), "tb_per_s": round(kv_bytes / med / 1e6, 3)}
        print(f"{name:24s} median {med:8.3f} us  quartiles {qs[0]:.3f} .. {qs[2]:.3f}  min {min(ts):.3f} max {max(ts):.3f}  "
              f"{kv_bytes / med / 1e6:.2f} TB/s of K/V")
    b0, b1 = res["variants"]["baseline"]["median_us"], res["variants"]["baseline (again)"]["median_us"]
    al = res["variants"]["this tree, ALiBi"]["median_us"]
    res["baseline_spread_us"] = round(abs(b0 - b1), 3)
    res["alibi_minus_baseline_us"] = round(al - (b0 + b1) / 2, 3)
    print(f"baseline against itself: {abs(b0 - b1):.3f} us between its two medians; ALiBi - baseline: {al - (b0 + b1) / 2:+.3f} us")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
