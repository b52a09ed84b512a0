"""CPU: what the compiler made of the FP8 decode GEMM (csrc/gemm_skinny_fp8.hip), read from the BUILT library's code-object
metadata (tools/kernel_table.py; no GPU, no compiler run): no scratch, no spilled registers, registers inside what a
workgroup of its size may hold, and an LDS image — dynamic: x slice + one 2 KiB transpose image per wave — that fits the CU
for the 33 .. 64-row form."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_table  # noqa: E402

X_ROW_STRIDE = 1024 * 2 + 32        # bytes of one row of the x image (kRS): 1024 k of T and a 32-byte bank offset
LDS_PER_CU = 160 * 1024


def _rows():
    rows = [r for r in kernel_table.kernels() if r["name"].startswith("gemm_skinny_fp8w_kernel<")]
    assert len(rows) == 18, sorted(r["name"] for r in rows)
    return rows


def test_fp8_gemm_kernels_use_no_scratch_and_spill_nothing():
    for r in _rows():
        assert r.get("private_segment_fixed_size", 0) == 0 and r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, r
        assert r.get("wavefront_size") == 64, r["name"]
        mb, rpw, nw = (int(v) for v in re.match(r".*<\w+, (\d), (\d), (\d)>", r["name"]).groups())
        # 512 registers per SIMD lane: a workgroup of 8 waves puts two waves on a SIMD
        assert r["vgpr_count"] <= (512 if nw == 4 else 256), r
        assert r.get("group_segment_fixed_size", 0) == 0          # the image is dynamic LDS


def test_fp8_gemm_lds_fits_the_cu_at_64_rows():
    names = sorted(r["name"] for r in _rows())
    assert names == sorted(f"gemm_skinny_fp8w_kernel<{t}, {mb}, {rpw}, {nw}>" for t in ("BF16", "F16")
                           for mb, cfgs in ((1, ((1, 4), (2, 4), (2, 8))), (2, ((1, 4), (2, 4), (2, 8))), (4, ((1, 4), (1, 8), (2, 8))))
                           for rpw, nw in cfgs)
    for mb, nw in ((4, 4), (4, 8)):
        lds = mb * 16 * X_ROW_STRIDE + nw * 2048
        assert lds <= LDS_PER_CU, (mb, nw, lds)
    # two 4-wave workgroups per CU at 17 .. 32 rows, three at <= 16
    assert 2 * (2 * 16 * X_ROW_STRIDE + 4 * 2048) <= LDS_PER_CU and 3 * (16 * X_ROW_STRIDE + 4 * 2048) <= LDS_PER_CU
    rows = [r for r in kernel_table.kernels() if r["name"].startswith("dequant_fp8_block_kernel<")]
    assert len(rows) == 2 and all(r.get("private_segment_fixed_size", 0) == 0 for r in rows)
