"""CPU: tools/isa_diff.py, the comparison a refactor uses to show that the device code did not change, on a two-kernel
source compiled for gfx950 (no GPU): identical objects, objects that differ only in the compilation-unit id, and
objects that differ in one kernel."""
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


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_diff")
    out = {}
    for name, comment, factor in (("base", "one", "2.0f"), ("comment", "another comment", "2.0f"), ("constant", "one", "3.0f")):
        src = d / (name + ".hip")
        src.write_text(SRC % (comment, factor))
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
