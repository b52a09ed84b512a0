"""CPU: the C-ABI shared library loads and exports every symbol include/hydra_hip.h
declares (no compute calls — there is no GPU here)."""
import ctypes
import os
import re

from hydrainfer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(experimental=False):
    """hx_* functions declared by include/hydra_hip.h (the product ABI) or, experimental=True, by
    include/hydra_hip_experimental.h (exported only by `make EXPERIMENTS=1` builds)."""
    names = []
    for hdr in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if not hdr.endswith(".h") or hdr.endswith("_experimental.h") != experimental:
            continue
        src = open(os.path.join(ROOT, "include", hdr)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names += re.findall(r"\b(hx_[a-z0-9_]+)\s*\(", src)
    return sorted(set(names))


def test_library_exports_every_declared_symbol():
    declared = _declared()
    assert len(declared) >= 19
    handle = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in declared if not hasattr(handle, n)]
    assert not missing, f"declared in include/ but not exported: {missing}"


def test_experiments_are_not_in_the_default_library():
    """Rejected experiments and microbenchmarks (four-heads decode attention, stream probes) ship
    only in `make EXPERIMENTS=1` builds: either all of hydra_hip_experimental.h is exported or none of it, and the
    ctypes binding types exactly those names."""
    exp = _declared(experimental=True)
    assert exp == sorted(_lib._EXPERIMENTAL_SIGNATURES) and len(exp) >= 2
    handle = ctypes.CDLL(_lib.LIB_PATH)
    present = [n for n in exp if hasattr(handle, n)]
    assert present in ([], exp), present
    assert _lib.has_experiments() == bool(present)
    assert not set(exp) & set(_declared())


def test_python_binding_covers_the_header():
    assert sorted(_lib.exported_symbols()) == _declared()
    lib = _lib.lib()
    assert lib.hx_abi_version() == _lib.HX_ABI_VERSION == 3
    assert lib.hx_strerror(0) == b"ok"
    assert b"data type" in lib.hx_strerror(-1)


def test_attn_args_struct_layout_matches_header():
    # field order/size of hx_attn_args as declared in the header
    src = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    body = re.search(r"typedef struct hx_attn_args \{(.*?)\} hx_attn_args;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split()[-1] if "," not in decl else None
        if names is None:
            first, *rest = decl.split(",")
            fields.append(first.split()[-1].lstrip("*"))
            fields += [r.strip().lstrip("*") for r in rest]
        else:
            fields.append(names.lstrip("*"))
    assert fields == [f[0] for f in _lib.hx_attn_args._fields_]


def test_cpu_tensors_are_refused_not_emulated():
    import pytest
    import torch
    from hydrainfer_amd._C.kernel.norm import rms_norm
    x = torch.randn(2, 8)
    with pytest.raises(_lib.HydraHipError):
        rms_norm(torch.empty_like(x), x, torch.ones(8), 1e-5)


def test_op_modules_match_the_reference_stubs():
    """Module paths, function names and positional parameter lists of hydrainfer._C.* as the
    reference's own .pyi stubs declare them (tests/golden/op_signatures.json, extracted by
    tests/golden/generate_stub_signatures.py).  flash_infer is the one package deliberately absent
    (north_star: the flashinfer path is removed)."""
    import importlib
    import inspect
    import json
    want = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "op_signatures.json")))
    missing = []
    for module, fns in want.items():
        if module.endswith("flash_infer"):
            continue
        mod = importlib.import_module(f"hydrainfer_amd.{module}")
        for name, params in fns.items():
            fn = getattr(mod, name, None)
            if fn is None:
                missing.append(f"{module}.{name}")
                continue
            got = [p.name for p in inspect.signature(fn).parameters.values()
                   if p.default is inspect.Parameter.empty and p.kind == p.POSITIONAL_OR_KEYWORD]
            assert len(got) == len(params), f"{module}.{name}: {got} vs reference {params}"
    assert not missing, missing


def test_xreg_split_plan_is_stable():
    """The packed layout of hx_pack_decode_weight_xreg depends on the split plan for (N, K): weights packed by one
    build must be readable by the next.  Pins the plan for the LLaVA-1.5 7B / 13B projections and two small shapes
    (256 CUs assumed when no device is present; an MI355X has 256)."""
    l = _lib.lib()
    want = {(12288, 4096): 1, (22016, 4096): 1, (4096, 11008): 4, (4096, 4096): 1,
            (15360, 5120): 1, (27648, 5120): 1, (5120, 13824): 4, (48, 64): 1, (64, 2816): 1}
    for (n, k), s in want.items():
        assert l.hx_linear_decode_xreg_splits(n, k) == s, (n, k)
        assert l.hx_linear_decode_xreg_supported(32, n, k) == 1
        assert l.hx_linear_decode_xreg_workspace_bytes(32, n, k) == s * 32 * n * 4
    # 33 .. 64 rows: the wide kernel reads the SAME packing with half the k-steps per wave (twice the slabs) where the
    # packing's k-steps per wave halve to a built count: all 7B projections and, since round 5, the 13B ones
    # (40 -> 20 with one row group per unit; 27 -> 14 + 13)
    for (n, k), s in {(12288, 4096): 2, (4096, 11008): 8, (4096, 4096): 2, (64, 2816): 2,
                      (15360, 5120): 2, (5120, 13824): 8}.items():
        assert l.hx_linear_decode_xreg_supported(64, n, k) == 1 and l.hx_linear_decode_xreg_supported(33, n, k) == 1
        assert l.hx_linear_decode_xreg_workspace_bytes(64, n, k) == s * 64 * n * 4, (n, k)
    assert l.hx_gate_up_xreg_supported(64, 11008, 4096, 1) == 1 and l.hx_gate_up_xreg_workspace_bytes(64, 11008, 4096) == 2 * 64 * 22016 * 4
    assert l.hx_gate_up_xreg_supported(64, 13824, 5120, 1) == 1 and l.hx_gate_up_xreg_workspace_bytes(64, 13824, 5120) == 2 * 64 * 27648 * 4
    assert l.hx_norm_xreg_supported(64, 15360, 5120, 0) == 1 and l.hx_norm_xreg_supported(64, 5120, 13824, 0) == 0
    assert l.hx_linear_decode_xreg_supported(64, 1024, 3584) == 0       # 29 k-steps per wave: no built half
    assert l.hx_linear_decode_xreg_supported(65, 4096, 4096) == 0
    assert l.hx_gate_up_silu_xreg_supported(33, 11008, 4096) == 0      # the fused silu*mul epilogue: <= 32 rows
    assert l.hx_norm_xreg_supported(64, 12288, 4096, 0) == 1 and l.hx_norm_xreg_supported(64, 4096, 11008, 0) == 0
    assert l.hx_gate_up_silu_xreg_supported(32, 11008, 4096) == 1 and l.hx_gate_up_silu_xreg_supported(32, 13824, 5120) == 1
    assert l.hx_norm_xreg_supported(32, 12288, 4096, 0) == 1 and l.hx_norm_xreg_supported(32, 4096, 11008, 0) == 0
    assert l.hx_fragment_major_elems(5, 4096) == 16 * 4096 and l.hx_fragment_major_elems(32, 64) == 32 * 64


# The token-choice entries refuse bad arguments before any launch, so their status codes can be read without a GPU.
# Per entry: a good argument list (the pointer 4096 is never dereferenced: no call below is good), the positions of
# rows, n, ld, top_k and dtype in it, further (position, value) pairs that are a shape error, and the pointers that
# must not be null.  HX_ERR_DTYPE -1, HX_ERR_SHAPE -2, HX_ERR_NULL -4.
_P = 4096
_SMP_MAX_N = 35840
_BIG = 0x7ffffff1            # n of a logprob row past 0x7ffffff0
_TOKEN_CHOICE_ENTRIES = {
    #                 ids cut   u     logits rows n ld hist_ids counts cu total pen records dtype stream
    "hx_sample_rows": ([_P, None, None, _P, 1, 8, 8, _P, _P, _P, 1, _P, _P, 1, None],
                       dict(rows=4, n=5, ld=6, top_k=None, dtype=13),
                       [(5, _SMP_MAX_N + 1), (10, -1), (10, 1 << 31)], [0, 3, 12, 7, 8, 9, 11]),
    #                             ... pen bias_ids values cu bias_total records dtype stream
    "hx_sample_rows_constrained": ([_P, None, None, _P, 1, 8, 8, _P, _P, _P, 1, _P, _P, _P, _P, 1, _P, 1, None],
                                   dict(rows=4, n=5, ld=6, top_k=None, dtype=17),
                                   [(5, _SMP_MAX_N + 1), (10, -1), (10, 1 << 31), (15, -1), (15, 1 << 31)],
                                   [0, 3, 16, 7, 8, 9, 11, 12, 13, 14]),
    #                          ... records logprobs top_ids top_logprobs top_k want dtype stream
    "hx_sample_rows_logprobs": ([_P, None, None, _P, 1, 8, 8, _P, _P, _P, 1, _P, _P, _P, _P, 1, _P, _P, _P, _P, 2, None, 1, None],
                                dict(rows=4, n=5, ld=6, top_k=20, dtype=22),
                                [(5, _SMP_MAX_N + 1), (10, -1), (10, 1 << 31), (15, -1), (15, 1 << 31)],
                                [0, 3, 16, 7, 8, 9, 11, 12, 13, 14, 17, 18, 19]),
    #                  ids logprobs top_ids top_logprobs logits rows n ld top_k dtype stream
    "hx_logprob_rows": ([_P, _P, _P, _P, _P, 2, 16, 16, 1, 1, None],
                        dict(rows=5, n=6, ld=7, top_k=8, dtype=9), [(6, _BIG), (5, 1 << 31)], [0, 1, 2, 3, 4]),
    #                           logprobs ranks top_ids top_logprobs logits targets rows n ld top_k dtype form stream
    "hx_token_logprob_rows_ex": ([_P, _P, _P, _P, _P, _P, 2, 16, 16, 1, 1, 0, None],
                                 dict(rows=6, n=7, ld=8, top_k=9, dtype=10),
                                 [(7, _BIG), (6, 1 << 31), (11, -1), (11, 3)], [0, 1, 2, 3, 4, 5]),
}


def _token_choice_cases(name):
    """[(what, arguments, status)] for one entry.  The statuses are what the library gave before the three sampling
    entries shared one argument record and every entry one launch helper; they are written out here, not derived."""
    ok, at, shape, pointers = _TOKEN_CHOICE_ENTRIES[name]

    def call(*changes):
        args = list(ok)
        for pos, v in changes:
            args[pos] = v
            if pos == at["n"] and v > args[at["ld"]]:
                args[at["ld"]] = v                  # a wide row, not a row stride below the width
        return args
    f32, rows0, null0 = (at["dtype"], 0), (at["rows"], 0), (pointers[0], None)
    cases = [("rows 0", call(rows0), -2), ("n 0", call((at["n"], 0)), -2), ("ld < n", call((at["ld"], ok[at["n"]] - 1)), -2)]
    cases += [(f"shape {pos} {v}", call((pos, v)), -2) for pos, v in shape]
    if at["top_k"] is not None:
        cases += [("top_k 21", call((at["top_k"], 21)), -2), ("top_k -1", call((at["top_k"], -1)), -2),
                  ("top_k before dtype and null", call((at["top_k"], 21), f32, null0), -2)]
    cases += [("fp32", call(f32), -1), ("shape before dtype and null", call(rows0, f32, null0), -2),
              ("dtype before null", call(f32, null0), -1)]
    cases += [(f"null {pos}", call((pos, None)), -4) for pos in pointers]
    return cases


def test_token_choice_entries_refuse_bad_arguments_with_the_same_status():
    from hydrainfer_amd.sampling import SAMPLE_MAX_N
    assert SAMPLE_MAX_N == _SMP_MAX_N
    lib = _lib.lib()
    for name in _TOKEN_CHOICE_ENTRIES:
        cases = _token_choice_cases(name)
        assert len(cases) >= 14
        for what, args, status in cases:
            assert getattr(lib, name)(*args) == status, (name, what)


# The four grouped expert GEMM entries share one argument check (csrc/moe_gemm.h).  Each keeps the order in which it has
# always reported: the 16-bit entries a misaligned pointer (HX_ERR_STRIDE -3) before a dtype they do not do
# (HX_ERR_DTYPE -1), the FP8 entries the dtype first.  Every call below is refused on the host, before any launch.
#                 out  in   weight [scale] seg n topk E  h    I   dtype stream
_MOE_16 = [_P, _P, _P, _P, 4, 2, 8, 256, 128, 2, None]
_MOE_FP8 = [_P, _P, _P, _P, _P, 4, 2, 8, 256, 128, 2, None]
_MOE_ENTRIES = {"hx_moe_gate_up_silu": (_MOE_16, -3), "hx_moe_down": (_MOE_16, -3),
                "hx_moe_gate_up_silu_fp8w": (_MOE_FP8, -1), "hx_moe_down_fp8w": (_MOE_FP8, -1)}


def test_moe_gemm_entries_keep_their_order_of_refusals():
    lib = _lib.lib()
    for name, (ok, both) in _MOE_ENTRIES.items():
        fn, dtype = getattr(lib, name), len(ok) - 2

        def call(*changes):
            args = list(ok)
            for pos, v in changes:
                args[pos] = v
            return fn(*args)
        f32 = (dtype, 0)
        for pos in (0, 1, 2):
            assert call((pos, _P + 8)) == -3, (name, pos)                  # misaligned alone
            assert call((pos, _P + 8), f32) == both, (name, pos)           # ... and a dtype the entry does not do
        assert call(f32) == -1, name
        if len(ok) == len(_MOE_FP8):
            assert call((3, _P + 2)) == -3 and call((3, _P + 2), f32) == -1 and call((3, None)) == -4, name
        # NULL and shape come first in both families
        assert call((0, None), f32, (1, _P + 8)) == -4 and call((dtype - 2, 192), f32, (1, _P + 8)) == -2, name
