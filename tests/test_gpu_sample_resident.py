"""GPU: hx_sample_rows_resident (csrc/sampling.hip) against hx_sample_rows.  The resident launch reads a record whose
words [6] and [7] are a 64-bit offset_base and draws with offset_base + positions[row]; for the same logits and a record
that carries that sum as its explicit offset (no history), hx_sample_rows gives the ids, the cut and u that the resident
launch must give BIT FOR BIT — compared as int32 views, NaN cuts included.  One launch holds a greedy row, a row with a
temperature only, a top-k row, a top-p row and a row with both; positions are not monotone across the rows; the bases
include 0, a negative one, one whose sum is negative (wraps modulo 2^64) and 2^32 - 3 at position 5, whose sum carries
into the high word."""
import numpy as np
import pytest
import torch

from hydrainfer_amd import _lib
from hydrainfer_amd.sampling import (SAMPLE_MAX_N, pack_resident_records, pack_sample_records, sample_rows,
                                     sample_rows_resident)
from tests import sampling_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
HX_ERR_SHAPE, HX_ERR_NULL = -2, -4
CARRY_ROW, CARRY_BASE, CARRY_POS = 2, (1 << 32) - 3, 5
# (temperature, top_p, top_k, seed, offset_base) per row, None = greedy; and the rows' positions
RECORDS = [None,
           (0.9, 1.0, 0, (1 << 40) + 3, 0),
           (0.7, 1.0, 20, 5, CARRY_BASE),
           (1.1, 0.8, 0, (1 << 63) - 1, -3),
           (0.8, 0.9, 50, (1 << 32) + 7, -20)]
POSITIONS = [7, 10, CARRY_POS, 100, 2]


def explicit(records, positions):
    """the records hx_sample_rows takes for the same draws: offset = (offset_base + position) mod 2^64"""
    return [(0.0, 1.0, 0, 0, p) if r is None else r[:4] + ((r[4] + p) % (1 << 64),) for r, p in zip(records, positions)]


def padded(host, pad):
    """[rows, n] values as a device tensor with row stride n + pad"""
    rows, n = host.shape
    wide = torch.zeros(rows, n + pad, dtype=host.dtype)
    wide[:, :n] = host
    return wide.to(DEV)[:, :n]


def both(logits, records, positions, diagnostics=True):
    """(ids, cut, u) of the resident launch and of hx_sample_rows, as int32 views on the host"""
    rows = logits.shape[0]
    pos = torch.tensor(positions, dtype=torch.int32, device=DEV)
    resident = torch.from_numpy(pack_resident_records(records)).to(DEV)
    plain = torch.from_numpy(pack_sample_records(explicit(records, positions))).to(DEV)
    got, want = [], []
    for out, fn, args in ((got, sample_rows_resident, (resident, pos)), (want, sample_rows, (plain,))):
        cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2)) if diagnostics else (None, None)
        ids = fn(logits, *args, cut_out=cut, u_out=u)
        out += [ids.cpu().view(torch.int32)] + ([cut.cpu().view(torch.int32), u.cpu().view(torch.int32)] if diagnostics else [])
    return got, want


@pytest.mark.parametrize("n", [33, 1025, 32064])          # most threads own nothing; chunk 2 made odd (3); the product's vocabulary
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bit_for_bit_with_sample_rows(dtype, n):
    g = torch.Generator().manual_seed(n)
    logits = padded((torch.randn(len(RECORDS), n, generator=g) * 3).to(dtype), 8 if n == 32064 else 3)
    assert logits.stride(0) > n
    got, want = both(logits, RECORDS, POSITIONS)
    for name, a, b in zip(("ids", "cut", "u"), got, want):
        assert torch.equal(a, b), f"{name}: resident {a.tolist()} != sample_rows {b.tolist()}"
    ids, cut, u = got[0].view(torch.int64), got[1].view(torch.float32), got[2].view(torch.float32)
    # the carry into the high word, against the numpy Philox itself
    seed = RECORDS[CARRY_ROW][3]
    assert CARRY_BASE + CARRY_POS == (1 << 32) + 2
    assert np.float32(u[CARRY_ROW].item()).view(np.uint32) == ref.uniform(seed, (1 << 32) + 2).view(np.uint32)
    assert np.float32(u[CARRY_ROW].item()).view(np.uint32) != ref.uniform(seed, 2).view(np.uint32)       # (a lost carry)
    # every row against the CPU reference, the greedy row as the argmax
    host = logits.cpu()
    kinds = [ref.check_row(host[r], [], [], (0.0, 0.0, 1.0), rec, int(ids[r]), float(cut[r]), np.float32(u[r].item()), f"row {r}")
             for r, rec in enumerate(explicit(RECORDS, POSITIONS))]
    assert kinds == ["greedy"] + ["sampled"] * 4
    # cut_out and u_out NULL: the same ids
    got, want = both(logits, RECORDS, POSITIONS, diagnostics=False)
    assert torch.equal(got[0], want[0]) and torch.equal(got[0].view(torch.int64), ids)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_degenerate_rows(dtype):
    n = 1025
    g = torch.Generator().manual_seed(3)
    host = (torch.randn(3, n, generator=g) * 3).to(dtype)
    host[0, 700] = float("nan")
    host[1, :] = float("-inf")
    logits = padded(host, 3)
    records = [(0.8, 0.9, 20, 11, 4), (1.2, 1.0, 0, 12, -1), (0.8, 0.9, 20, 11, 4)]
    positions = [9, 3, 9]
    got, want = both(logits, records, positions)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    ids, cut, u = got[0].view(torch.int64), got[1].view(torch.float32), got[2].view(torch.float32)
    assert ids[:2].tolist() == [700, 0] and torch.isnan(cut[:2]).all() and not torch.isnan(cut[2])
    for r in range(3):
        assert np.float32(u[r].item()).view(np.uint32) == ref.uniform(records[r][3], records[r][4] + positions[r]).view(np.uint32)


def test_errors_launch_nothing():
    rows, n = 2, 64
    logits = torch.zeros(rows, n, dtype=torch.bfloat16, device=DEV)
    sp = torch.from_numpy(pack_resident_records([(1.0, 1.0, 0, 1, 0)] * rows)).to(DEV)
    pos = torch.zeros(rows, dtype=torch.int32, device=DEV)
    ids = torch.full((rows,), -77, dtype=torch.int64, device=DEV)
    cut, u = (torch.full((rows,), 7.0, device=DEV) for _ in range(2))
    fn, stream = _lib.lib().hx_sample_rows_resident, _lib.current_stream()

    def call(rows_=rows, n_=n, ld=n, positions=pos.data_ptr()):
        return fn(ids.data_ptr(), cut.data_ptr(), u.data_ptr(), logits.data_ptr(), rows_, n_, ld, sp.data_ptr(), positions,
                  _lib.HX_BF16, stream)
    assert call(positions=None) == HX_ERR_NULL
    assert call(n_=SAMPLE_MAX_N + 1, ld=SAMPLE_MAX_N + 1) == HX_ERR_SHAPE
    assert call(rows_=0) == HX_ERR_SHAPE
    torch.cuda.synchronize()
    assert ids.tolist() == [-77] * rows and cut.tolist() == [7.0] * rows and u.tolist() == [7.0] * rows
    assert call() == 0
    torch.cuda.synchronize()
    assert all(0 <= t < n for t in ids.tolist()) and u.tolist() != [7.0] * rows
    # the shim refuses what the entry would
    with pytest.raises(_lib.HydraHipError):
        sample_rows_resident(logits, sp, pos.long())
    with pytest.raises(_lib.HydraHipError):
        sample_rows_resident(logits, sp, pos[:1])


def test_captured_at_the_product_vocabulary():
    """n = 32064 needs 125 KiB of dynamic LDS: the limit is raised by a launch outside the capture, the captured launch
    replays with whatever the position array holds by then"""
    n = 32064
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(len(RECORDS), n, generator=g) * 3).to(torch.bfloat16).to(DEV)
    resident = torch.from_numpy(pack_resident_records(RECORDS)).to(DEV)
    pos = torch.tensor(POSITIONS, dtype=torch.int32, device=DEV)
    ids = torch.zeros(len(RECORDS), dtype=torch.int64, device=DEV)
    cut, u = (torch.zeros(len(RECORDS), device=DEV) for _ in range(2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sample_rows_resident(logits, resident, pos, out=ids, cut_out=cut, u_out=u)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sample_rows_resident(logits, resident, pos, out=ids, cut_out=cut, u_out=u)
    for shift in (0, 1):
        positions = [p + shift for p in POSITIONS]
        pos.copy_(torch.tensor(positions, dtype=torch.int32))
        ids.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want = both(logits, RECORDS, positions)[1]
        for a, b in zip((ids, cut, u), want):
            assert torch.equal(a.cpu().view(torch.int32), b)
