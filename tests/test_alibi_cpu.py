"""CPU: the ALiBi surface that can be checked without a GPU — the C ABI's new tail, the slope schedule, the torch
restatement against a closed form, and what the compiler made of the new kernels (tests/test_gpu_alibi.py runs them)."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

from hydrainfer_amd import _lib
from tests import alibi_ref as R
from tests.util import ATTN_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_table  # noqa: E402


def _header():
    return open(os.path.join(ROOT, "include", "hydra_hip.h")).read()


def test_header_and_ctypes_struct_agree_on_the_alibi_tail():
    src = _header()
    body = re.search(r"typedef struct hx_attn_args \{(.*?)\} hx_attn_args;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls[-3:] == ["int32_t flags", "const float* alibi_slopes", "int64_t alibi_batch_stride"]
    fields = _lib.hx_attn_args._fields_
    assert [f[0] for f in fields[-3:]] == ["flags", "alibi_slopes", "alibi_batch_stride"]
    assert fields[-2][1] is ctypes.c_void_p and fields[-1][1] is ctypes.c_int64
    # the tail is appended: nothing in front of it moved (flags sits where ABI version 3 had it, at the struct's old end)
    assert _lib.hx_attn_args.flags.offset + 4 == _lib.hx_attn_args.alibi_slopes.offset == 208
    assert ctypes.sizeof(_lib.hx_attn_args) == 224
    assert int(re.search(r"#define HX_ATTN_ALIBI (\d+)", src).group(1)) == _lib.HX_ATTN_ALIBI == 2
    assert int(re.search(r"#define HX_ATTN_LOCAL_WINDOW (\d+)", src).group(1)) == _lib.HX_ATTN_LOCAL_WINDOW == 1
    # a zero-filled struct means "off"
    a = _lib.hx_attn_args()
    assert a.flags == 0 and a.alibi_slopes is None and a.alibi_batch_stride == 0


def test_abi_version_and_exported_symbols_are_unchanged():
    """The feature is detected by the flag (an older library answers the unknown bit with HX_ERR_UNSUPPORTED), not by a
    new version or a new symbol."""
    assert _lib.lib().hx_abi_version() == 3
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("hx_"))
    if not _lib.has_experiments():
        assert exported == sorted(_lib.exported_symbols())
    assert not [n for n in exported if "alibi" in n]


def test_alibi_slopes_hand_written_values():
    from hydrainfer_amd.layer.alibi import alibi_slopes
    s8 = alibi_slopes(8)
    assert s8.dtype == torch.float32 and s8.shape == (8,)
    assert s8.tolist() == [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.00390625]
    # 12 heads: the 8-head schedule, then the 1st, 3rd, 5th, 7th slope of the 16-head schedule 2^(-k/2)
    want12 = [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.00390625,
              1 / math.sqrt(2), 1 / (2 * math.sqrt(2)), 1 / (4 * math.sqrt(2)), 1 / (8 * math.sqrt(2))]
    torch.testing.assert_close(alibi_slopes(12), torch.tensor(want12, dtype=torch.float32), rtol=1e-6, atol=0)
    assert alibi_slopes(1).tolist() == [2.0 ** -8]
    assert alibi_slopes(32)[0].item() == 2.0 ** -0.25 or abs(alibi_slopes(32)[0].item() - 2.0 ** -0.25) < 1e-7
    with pytest.raises(ValueError):
        alibi_slopes(0)


def test_restatement_matches_the_closed_form_at_q_zero():
    from hydrainfer_amd.layer.alibi import alibi_slopes
    H, D, lk = 8, 64, 832
    g = torch.Generator().manual_seed(5)
    k = torch.randn((lk, H, D), generator=g)
    v = torch.randn((lk, H, D), generator=g)
    slopes = alibi_slopes(H)
    q = torch.zeros((1, H, D))
    for causal in (True, False):
        got = R.attend_alibi(q, k, v, 1.0 / math.sqrt(D), causal, slopes)[0].double()
        want = R.closed_form_q0(v, slopes)
        assert (got - want).abs().max().item() < 2e-6
    # and it is not the plain mean of the values (what ignoring the slopes would give)
    assert (R.closed_form_q0(v, slopes) - v.double().mean(dim=0)).abs().max().item() > 0.1


def test_restatement_bias_is_relative_uncapped_and_two_sided():
    H, D = 2, 32
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn((n, H, D), generator=g) for n in (5, 9, 9))
    slopes = torch.tensor([0.3, 0.05])
    sc = 1.0 / math.sqrt(D)
    # causal: the relative form equals the reference's `+ slope * j` form (a constant per row apart)
    s = torch.einsum("qhd,khd->hqk", q, k) * sc + slopes[:, None, None] * torch.arange(9)[None, None, :]
    x, y = torch.arange(9)[None, None, :], torch.arange(5)[None, :, None]
    s = s.masked_fill((x - y) > 4, float("-inf"))
    want = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v)
    torch.testing.assert_close(R.attend_alibi(q, k, v, sc, True, slopes), want, rtol=1e-5, atol=1e-5)
    # non-causal: keys to the right of the diagonal are penalised too (|.|), so it differs from the one-sided form
    two = R.attend_alibi(q, k, v, sc, False, slopes)
    s1 = torch.einsum("qhd,khd->hqk", q, k) * sc - slopes[:, None, None] * (y + 4 - x).float()
    one = torch.einsum("hqk,khd->qhd", torch.softmax(s1, -1), v)
    assert (two - one).abs().max().item() > 1e-2
    # softcap: the bias is added after the cap — it can push a score below -softcap
    capped = R.attend_alibi(q, k, v, sc, False, slopes * 50, softcap=1.0)
    inside = torch.einsum("qhd,khd->hqk", q, k) * sc - (slopes * 50)[:, None, None] * (y + 4 - x).abs().float()
    wrong = torch.einsum("hqk,khd->qhd", torch.softmax(torch.tanh(inside), -1), v)
    assert (capped - wrong).abs().max().item() > 1e-2


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_first_gpu_case_cannot_pass_by_ignoring_the_slopes(dt):
    """The inputs of test_gpu_alibi.py's first case: on the restatement alone, the output with slopes lies more than 10 x
    the tolerance from the output without them."""
    from hydrainfer_amd.layer.alibi import alibi_slopes
    c = R.FIRST_CASE
    kv = R.ragged_lens(c["batch"], c["lo"], c["hi"], c["seed"])
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(c["batch"], c["H"], c["HK"], c["D"], kv, [1] * c["batch"], dt, seed=c["seed"])
    with_s = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, alibi_slopes(c["H"]))
    without = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, None)
    atol, rtol = ATTN_TOL[dt]
    gap = (with_s - without).abs() - 10 * (atol + rtol * with_s.abs())
    assert gap.max().item() > 0, gap.max().item()
    assert max(kv) > 600 and min(kv) < 200, kv       # ragged indeed


@pytest.fixture(scope="module")
def table():
    rows = kernel_table.kernels()
    assert len(rows) > 300
    return rows


def test_alibi_kernels_use_no_scratch_and_fit_the_decode_budget(table):
    dec = [r for r in table if r["name"].startswith("attn_decode_alibi_kernel<")]
    gqa = [r for r in table if r["name"].startswith("attn_decode_gqa_alibi_kernel<")]
    fwd = [r for r in table if r["name"].startswith("attn_fwd_alibi_kernel<")]
    assert len(dec) == 24 and len(gqa) == 6 and len(fwd) == 20, (len(dec), len(gqa), len(fwd))
    for r in dec + gqa + fwd:
        assert r.get("private_segment_fixed_size", 0) == 0 and r.get("vgpr_spill_count", 0) == 0, r
        assert r.get("sgpr_spill_count", 0) == 0, r
        assert r.get("wavefront_size") == 64, r
    by = {r["name"]: r for r in table}
    for dt in ("BF16", "F16"):
        for nt in ("true", "false"):
            r = by[f"attn_decode_alibi_kernel<{dt}, 128, 4, {nt}>"]
            assert r["vgpr_count"] <= 128, r                      # 4 workgroups of 4 waves per CU, like attn_decode_kernel
            assert r["group_segment_fixed_size"] <= 40 * 1024, r
            assert r["kernarg_segment_size"] >= 64, r
    # the existing entries kept their names
    for name in ("attn_decode_kernel<BF16, 128, 4, true, true, false>", "attn_decode_kernel<BF16, 128, 4, true, true, true>",
                 "attn_decode_gqa_kernel<BF16, 128>", "attn_fwd_kernel<BF16, 128, true, 1, 1>"):
        assert name in by, name
