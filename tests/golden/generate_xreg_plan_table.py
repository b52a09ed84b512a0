"""Every host-side answer of the activations-in-registers decode GEMMs (csrc/gemm_xreg.hip) over a grid of shapes,
and the status each launch entry gives for one deliberate argument defect -> tests/golden/xreg_plan_table.json.

Run ONCE against the library of the commit whose answers are to be pinned, on a machine WITHOUT a GPU (the planning
entries assume 256 CUs, an MI355X's count, when there is no device; every call of `arg_check_statuses` carries a
defect and must be refused before anything is launched):

    python tests/golden/generate_xreg_plan_table.py

tests/test_xreg_plan_table.py replays `sweep` and `arg_check_statuses` against the current library and compares
point by point.

File format: "codes" / "plan_codes" are the distinct answers, "table"[N] one short string per K of `k_values()`:
one character per M (an index into "codes": the ten answers of `point`), one for hx_linear_decode_xreg_splits, and
one per (max_rows, flags) of hx_decode_weight_plan (an index into "plan_codes").
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from hydrainfer_amd import _lib  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xreg_plan_table.json")

M_VALUES = (1, 16, 17, 32, 33, 48, 64, 65)
N_VALUES = (16, 32, 48, 64, 1024, 2816, 4096, 5120, 11008, 12288, 13824, 15360, 22016, 27648)
PLAN_ROWS = (8, 32, 64)
PLAN_FLAGS = (0, _lib.HX_DW_GATE_UP, _lib.HX_DW_FORCE_LDS_SLICE, _lib.HX_DW_GATE_UP | _lib.HX_DW_FORCE_LDS_SLICE)
ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
POINT_FIELDS = ("linear_supported", "linear_slabs", "norm_supported", "norm_supported_gate_up", "gate_up_silu_supported",
                "gate_up_supported", "gate_up_supported_norm", "gate_up_slabs", "gate_up_silu_wide_supported")


def k_values():
    ks = set(range(32, 2048 + 1, 32)) | set(range(128, 16384 + 1, 128)) | {3584, 11008, 13824}
    return sorted(ks) + [8, 4100]          # the last two are invalid (no multiple of 32)


def slabs(nbytes, rows, cols):
    q, r = divmod(nbytes, rows * cols * 4)
    assert r == 0, (nbytes, rows, cols)
    return q


def point(l, M, N, K):
    """The answers for one (M, N, K), in POINT_FIELDS order; gate|up entries take inter = N / 2."""
    inter = N // 2
    return (l.hx_linear_decode_xreg_supported(M, N, K),
            slabs(l.hx_linear_decode_xreg_workspace_bytes(M, N, K), M, N),
            l.hx_norm_xreg_supported(M, N, K, 0),
            l.hx_norm_xreg_supported(M, N, K, 1),
            l.hx_gate_up_silu_xreg_supported(M, inter, K),
            l.hx_gate_up_xreg_supported(M, inter, K, 0),
            l.hx_gate_up_xreg_supported(M, inter, K, 1),
            slabs(l.hx_gate_up_xreg_workspace_bytes(M, inter, K), M, 2 * inter),
            l.hx_gate_up_silu_wide_xreg_supported(M, inter, K))


def weight_plan(l, N, K, max_rows, flags):
    """(status, layout, flags) of hx_decode_weight_plan; layout and flags only where the plan succeeded."""
    w = _lib.hx_decode_weight()
    rc = l.hx_decode_weight_plan(ctypes.byref(w), N, K, _lib.HX_F16, max_rows, flags)
    return (rc, w.layout, w.flags) if rc == 0 else (rc, -1, -1)


def sweep(l):
    """{(N, K): (per-M answers of `point`, hx_linear_decode_xreg_splits, hx_decode_weight_plan answers)}"""
    out = {}
    for N in N_VALUES:
        for K in k_values():
            out[(N, K)] = (tuple(point(l, M, N, K) for M in M_VALUES), l.hx_linear_decode_xreg_splits(N, K),
                           tuple(weight_plan(l, N, K, r, f) for r in PLAN_ROWS for f in PLAN_FLAGS))
    return out


# ---- one defect per call ---------------------------------------------------------------------------------------
A = 0x7F0000001000                # fake pointers: 16-byte aligned addresses that are never dereferenced on the host
ODD = A + 1
F16 = _lib.HX_F16
BAD_DTYPE = 7
M0, N0, K0, I0 = 32, 4096, 4096, 2048           # a product every narrow entry supports; I0 = its gate|up's inter
MW = 64                                          # rows of the wide entries
BIG = 1 << 40                                    # partial_bytes that always suffices


def _norm(residual=A, slabs_in=A, n_splits=1, weight=A, x_frag=A):
    return [residual, slabs_in, n_splits, weight, 1e-5, x_frag]


def _dw(l, packed=A, dtype=F16, max_rows=32):
    w = _lib.hx_decode_weight()
    assert l.hx_decode_weight_plan(ctypes.byref(w), N0, K0, F16, max_rows, 0) == 0 and w.layout == _lib.HX_DW_XREG
    w.packed, w.dtype = packed, dtype
    return ctypes.byref(w)


def arg_check_calls(l):
    """{"entry:defect": (function, arguments)} — every call has EXACTLY ONE defect; none is valid."""
    c = {}

    def entry(fn, defects):
        for what, args in defects.items():
            c[f"{fn}:{what}"] = (getattr(l, fn), args)

    entry("hx_pack_decode_weight_xreg", {
        "null": [None, A, N0, K0, K0, 0, F16, None],
        "shape": [A, A, N0 + 8, K0, K0, 0, F16, None],
        "dtype": [A, A, N0, K0, K0, 0, BAD_DTYPE, None],
        "misaligned": [A, ODD, N0, K0, K0, 0, F16, None],
    })
    entry("hx_linear_decode_partial_xreg", {
        "null": [A, None, A, M0, N0, K0, K0, 0, BIG, F16, None],
        "shape": [A, A, A, 65, N0, K0, K0, 0, BIG, F16, None],
        "shape_ldx": [A, A, A, M0, N0, K0, K0 + 4, 0, BIG, F16, None],
        "dtype": [A, A, A, M0, N0, K0, K0, 0, BIG, BAD_DTYPE, None],
        "misaligned": [A, ODD, A, M0, N0, K0, K0, 0, BIG, F16, None],
        "workspace": [A, A, A, M0, N0, K0, K0, 0, M0 * N0 * 4 - 1, F16, None],
        "workspace_wide": [A, A, A, MW, N0, K0, K0, 0, 2 * MW * N0 * 4 - 1, F16, None],
    })
    entry("hx_gate_up_silu_xreg", {
        "null": [A, A, None, M0, I0, K0, K0, 0, F16, None],
        "shape": [A, A, A, 33, I0, K0, K0, 0, F16, None],
        "dtype": [A, A, A, M0, I0, K0, K0, 0, BAD_DTYPE, None],
        "misaligned": [ODD, A, A, M0, I0, K0, K0, 0, F16, None],
    })
    entry("hx_norm_linear_decode_xreg", {
        "null": [A] + _norm(weight=None) + [A, M0, N0, K0, A, BIG, F16, None],
        "null_sync": [A] + _norm() + [A, M0, N0, K0, None, BIG, F16, None],
        "shape": [A] + _norm() + [A, M0, N0, 11008, A, BIG, F16, None],
        "shape_splits": [A] + _norm(n_splits=0) + [A, M0, N0, K0, A, BIG, F16, None],
        "dtype": [A] + _norm() + [A, M0, N0, K0, A, BIG, BAD_DTYPE, None],
        "misaligned": [A] + _norm(residual=ODD) + [A, M0, N0, K0, A, BIG, F16, None],
        "misaligned_weight": [A] + _norm() + [ODD, M0, N0, K0, A, BIG, F16, None],
        "workspace": [A] + _norm() + [A, M0, N0, K0, A, M0 * N0 * 4 - 1, F16, None],
        "workspace_wide": [A] + _norm() + [A, MW, N0, K0, A, 2 * MW * N0 * 4 - 1, F16, None],
    })
    entry("hx_norm_gate_up_silu_xreg", {
        "null": [None] + _norm() + [A, M0, I0, K0, A, F16, None],
        "shape": [A] + _norm() + [A, M0, I0 + 16, K0, A, F16, None],
        "dtype": [A] + _norm() + [A, M0, I0, K0, A, BAD_DTYPE, None],
        "misaligned": [A] + _norm(x_frag=ODD) + [A, M0, I0, K0, A, F16, None],
    })
    entry("hx_gate_up_xreg", {
        "null": [None, A, A, MW, I0, K0, K0, 0, BIG, F16, None],
        "shape": [A, A, A, MW, I0 + 16, K0, K0, 0, BIG, F16, None],
        "dtype": [A, A, A, MW, I0, K0, K0, 0, BIG, BAD_DTYPE, None],
        "misaligned": [A, A, ODD, MW, I0, K0, K0, 0, BIG, F16, None],
        "workspace": [A, A, A, MW, I0, K0, K0, 0, 2 * MW * 2 * I0 * 4 - 1, F16, None],
    })
    entry("hx_norm_gate_up_silu_wide_xreg", {
        "null": [A] + _norm(slabs_in=None) + [A, MW, I0, K0, A, F16, None],
        "shape": [A] + _norm() + [A, 32, I0, K0, A, F16, None],
        "shape_k": [A] + _norm() + [A, MW, I0, 5120, A, F16, None],
        "dtype": [A] + _norm() + [A, MW, I0, K0, A, BAD_DTYPE, None],
        "misaligned": [A] + _norm() + [A, MW, I0, K0, ODD, F16, None],
    })
    entry("hx_norm_gate_up_xreg", {
        "null": [A] + _norm() + [None, MW, I0, K0, A, BIG, F16, None],
        "shape": [A] + _norm() + [A, MW, I0, 11008, A, BIG, F16, None],
        "dtype": [A] + _norm() + [A, MW, I0, K0, A, BIG, BAD_DTYPE, None],
        "misaligned": [ODD] + _norm() + [A, MW, I0, K0, A, BIG, F16, None],
        "workspace": [A] + _norm() + [A, MW, I0, K0, A, 2 * MW * 2 * I0 * 4 - 1, F16, None],
    })
    entry("hx_linear_decode_ex", {
        "null": [A, BIG, A, K0, 0, _dw(l, packed=None), M0, None],
        "shape": [A, BIG, A, K0, 0, _dw(l), M0 + 1, None],
        "dtype": [A, BIG, A, K0, 0, _dw(l, dtype=BAD_DTYPE), M0, None],
        "misaligned": [A, BIG, ODD, K0, 0, _dw(l), M0, None],
        "workspace": [A, M0 * N0 * 4 - 1, A, K0, 0, _dw(l), M0, None],
    })
    return c


def arg_check_statuses(l):
    return {name: fn(*args) for name, (fn, args) in arg_check_calls(l).items()}


def encode(l):
    import torch
    assert not torch.cuda.is_available(), "generate the table on a machine without a GPU (see the module docstring)"
    table = sweep(l)
    codes = sorted({a for per_m, _, _ in table.values() for a in per_m})
    plan_codes = sorted({a for _, _, plans in table.values() for a in plans})
    splits = sorted({s for _, s, _ in table.values()})
    assert max(len(codes), len(plan_codes), len(splits)) <= len(ALPHABET)
    rows = {}
    for N in N_VALUES:
        rows[str(N)] = ["".join(ALPHABET[codes.index(a)] for a in table[(N, K)][0]) +
                        ALPHABET[splits.index(table[(N, K)][1])] +
                        "".join(ALPHABET[plan_codes.index(a)] for a in table[(N, K)][2]) for K in k_values()]
    return {"point_fields": list(POINT_FIELDS), "codes": codes, "splits": splits, "plan_codes": plan_codes, "table": rows,
            "arg_checks": arg_check_statuses(l)}


def decode(doc):
    """The inverse of `encode`'s table: the dictionary `sweep` returns."""
    codes = [tuple(c) for c in doc["codes"]]
    plan_codes = [tuple(c) for c in doc["plan_codes"]]
    n_m = len(M_VALUES)
    out = {}
    for N in N_VALUES:
        for K, s in zip(k_values(), doc["table"][str(N)]):
            out[(N, K)] = (tuple(codes[ALPHABET.index(ch)] for ch in s[:n_m]), doc["splits"][ALPHABET.index(s[n_m])],
                           tuple(plan_codes[ALPHABET.index(ch)] for ch in s[n_m + 1:]))
    return out


if __name__ == "__main__":
    doc = encode(_lib.lib())
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(doc['codes'])} point codes, {len(doc['plan_codes'])} plan codes, "
          f"{len(doc['arg_checks'])} defect calls")
