"""CPU: tools/isa_diff.py, the comparison a refactor uses to show that the device code did not change, on a two-kernel
source compiled for gfx950 (no GPU): identical objects, objects that differ only in the compilation-unit id, and
objects that differ in one kernel; and on a source whose first kernel reaches a global through the .got: the same kernel
with a function that grew between it and the .got is MOVED, a changed constant in it is DIFF whether it moved or not."""
import io
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_diff  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

SRC = """#include <hip/hip_runtime.h>
// %s
__global__ void scale_kernel(float* x) { x[threadIdx.x] *= %s; }
__global__ void shift_kernel(float* x) { x[threadIdx.x] += 1.0f; }
"""
# table_kernel forms the address of g_table's .got slot pc-relatively.  The .got lies behind .text and a function keeps
# its distance to it unless something between the two changes size: the long form of resized_kernel (one store per line;
# kernels are aligned to 256 bytes) moves table_kernel against the .got.  3.0f and 5.0f are 32-bit literals of the same
# instruction.
SRC_GOT = """#include <hip/hip_runtime.h>
__device__ __attribute__((visibility("default"))) float g_table[64];
__global__ void table_kernel(float* x) { x[threadIdx.x] += g_table[threadIdx.x & 63] * %s; }
__global__ void resized_kernel(float* x) {
%s}
"""
SHORT = "  x[threadIdx.x] = 1.5f;\n"
LONG = "".join("  x[%d * blockDim.x + threadIdx.x] = %d.5f;\n" % (i, i) for i in range(64))


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_diff")
    out = {}
    texts = [(name, SRC % (comment, factor)) for name, comment, factor in
             (("base", "one", "2.0f"), ("comment", "another comment", "2.0f"), ("constant", "one", "3.0f"))]
    texts += [(name, SRC_GOT % (factor, body)) for name, body, factor in
              (("got", SHORT, "3.0f"), ("got_moved", LONG, "3.0f"), ("got_constant", SHORT, "5.0f"), ("got_moved_constant", LONG, "5.0f"))]
    for name, text in texts:
        src = d / (name + ".hip")
        src.write_text(text)
        out[name] = str(d / (name + ".o"))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-fno-gpu-rdc", "-c", str(src), "-o", out[name]], check=True)
    return out


def run(a, b):
    buf = io.StringIO()
    return isa_diff.compare(a, b, out=buf), buf.getvalue().splitlines()


def test_an_object_against_itself(objs):
    assert set(isa_diff.kernels(objs["base"])) == {"_Z12scale_kernelPf", "_Z12shift_kernelPf"}
    rc, lines = run(objs["base"], objs["base"])
    assert rc == 0 and len(lines) == 1 and "identical" in lines[0] and "2 in both (2 with a kernel descriptor)" in lines[0]


def test_a_comment_changes_the_cuid_only(objs):
    cuid = [{n for n in isa_diff.symbols(isa_diff.code_objects(objs[k])[0]) if n.startswith("__hip_cuid_")} for k in ("base", "comment")]
    assert cuid[0] and cuid[1] and cuid[0] != cuid[1]
    rc, lines = run(objs["base"], objs["comment"])
    assert rc == 0 and len(lines) == 1 and "identical" in lines[0]


def test_one_constant_in_one_kernel(objs):
    rc, lines = run(objs["base"], objs["constant"])
    assert rc == 1
    assert len(lines) == 2 and lines[0].startswith("DIFF scale_kernel(float*): code") and "1 differ" in lines[1]
    # and as a command: the exit status
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_diff.py"), objs["base"], objs["constant"]],
                       capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout.splitlines() == lines


def test_the_same_kernel_is_moved_when_a_function_next_to_it_grew(objs, monkeypatch):
    a, b = isa_diff.kernels(objs["got"]), isa_diff.kernels(objs["got_moved"])
    (ca, _, _, (addr_a, got_a)), (cb, _, _, (addr_b, got_b)) = a["_Z12table_kernelPf"], b["_Z12table_kernelPf"]
    assert got_a[1] == got_b[1] and [s[2] for s in got_a[1]] == ["g_table"]
    assert len(ca) == len(cb) and ca != cb and addr_a - got_a[0] != addr_b - got_b[0]      # only this rule can pass it
    assert len(a["_Z14resized_kernelPf"][0]) != len(b["_Z14resized_kernelPf"][0])
    rc, lines = run(objs["got"], objs["got_moved"])
    assert rc == 1 and len(lines) == 3      # resized_kernel itself changed
    assert lines[0].startswith("MOVED table_kernel(float*): same .got target") and lines[1].startswith("DIFF resized_kernel(float*): code")
    assert "0 identical, 1 moved (same .got target), 1 differ" in lines[2]
    # with nothing but the moved kernel in view: exit status 0
    only, real = {"_Z12table_kernelPf", "_Z12table_kernelPf.kd"}, isa_diff.symbols
    monkeypatch.setattr(isa_diff, "symbols", lambda elf: {n: v for n, v in real(elf).items() if n in only})
    rc, lines = run(objs["got"], objs["got_moved"])
    assert rc == 0 and len(lines) == 2 and lines[0].startswith("MOVED table_kernel(float*)")
    assert "0 identical, 1 moved (same .got target), 0 differ" in lines[1]


@pytest.mark.parametrize("other", ["got_constant", "got_moved_constant"])
def test_a_changed_word_that_is_no_got_displacement_is_diff(objs, other):
    a, b = isa_diff.kernels(objs["got"])["_Z12table_kernelPf"], isa_diff.kernels(objs[other])["_Z12table_kernelPf"]
    words = [o for o in range(0, len(a[0]), 4) if a[0][o:o + 4] != b[0][o:o + 4]]
    assert len(a[0]) == len(b[0]) and len(words) == (2 if other == "got_moved_constant" else 1)      # the constant (and the displacement)
    rc, lines = run(objs["got"], objs[other])
    assert rc == 1
    assert any(ln.startswith("DIFF table_kernel(float*): code") for ln in lines) and not any(ln.startswith("MOVED") for ln in lines)
