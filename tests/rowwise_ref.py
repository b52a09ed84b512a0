"""Helpers for the row-wise kernel tests (rms_norm, rope, silu, quick_gelu, cache scatter): buffers that notice a stray
write, misaligned copies, the exhaustive 16-bit input grid, and the references that oracle/ops.py does not already hold.

Every reference here is plain torch and runs on whatever device its inputs live on.  tests/test_rowwise_ref_cpu.py holds
each of them to an fp64 evaluation of the same chain of operations (same rounding points, fp64 in between)."""
from typing import Callable, Optional, Sequence, Tuple

import torch
from torch import Tensor

from oracle import ops

GUARD_BYTE = 0xA5          # fp16 / bf16 0xA5A5 and fp32 0xA5A5A5A5 are small negative numbers: finite, non-zero
GUARD_BYTES = 256          # on each side of the body


def misaligned(t: Tensor) -> Tensor:
    """A contiguous copy of t whose first element sits one element (2 bytes; 4 for fp32) past a 16-byte boundary: the
    vector forms of the kernels refuse it, the element forms take over."""
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    lead = (-buf.data_ptr() % 16) // t.element_size() + 1
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def guarded(shape: Sequence[int], dtype: torch.dtype, device="cpu", row_stride: Optional[int] = None,
            misalign: bool = False) -> Tuple[Tensor, Callable[[], None]]:
    """A tensor of `shape` that lives inside a larger byte buffer pre-filled with GUARD_BYTE, and a check() that asserts
    that every byte of the buffer outside the tensor still holds GUARD_BYTE.  The tensor itself starts out as the same
    pattern.  row_stride (elements, >= the elements of one row): the first dimension is strided and the gaps between
    the rows are guard too.  misalign: the tensor starts one element past a 16-byte boundary instead of on one."""
    es = torch.empty((), dtype=dtype).element_size()
    shape = tuple(int(s) for s in shape)
    rows = shape[0]
    inner = 1
    for s in shape[1:]:
        inner *= s
    stride = inner if row_stride is None else int(row_stride)
    assert stride >= inner and rows >= 1
    body = ((rows - 1) * stride + inner) * es
    buf = torch.full((GUARD_BYTES + 16 + body + GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=device)
    start = GUARD_BYTES + (-(buf.data_ptr() + GUARD_BYTES) % 16) + (es if misalign else 0)
    flat = buf[start:start + body].view(dtype)
    view = flat.as_strided((rows, inner), (stride, 1)).view(shape)
    assert view.data_ptr() % 16 == (es if misalign else 0)
    inside = torch.zeros(buf.numel(), dtype=torch.bool)
    if stride == inner:
        inside[start:start + body] = True
    else:
        for r in range(rows):
            inside[start + r * stride * es: start + (r * stride + inner) * es] = True
    outside = ~inside

    def check() -> None:
        stray = (buf.cpu() != GUARD_BYTE) & outside
        assert not stray.any(), (f"{int(stray.sum())} bytes outside the tensor were written, the first at byte "
                                 f"{int(stray.nonzero()[0]) - start} relative to its start")

    return view, check


def same_bits(a: Tensor, b: Tensor) -> bool:
    """Bit-for-bit equality (torch.equal calls -0 and +0 equal and NaN unequal to itself)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.detach().cpu().contiguous().view(it), b.detach().cpu().contiguous().view(it))


def all_finite_16bit(dtype: torch.dtype) -> Tensor:
    """Every 16-bit pattern of fp16 / bf16 once, as an [8, 8192] tensor; the non-finite patterns are replaced by 0."""
    assert dtype in (torch.float16, torch.bfloat16)
    x = (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16).view(dtype)
    x = torch.where(torch.isfinite(x), x, torch.zeros((), dtype=dtype))
    return x.view(8, 8192).clone()


def up_cycle(dtype: torch.dtype, shape: Sequence[int]) -> Tensor:
    """`up` operand of the exhaustive silu_and_mul run: cycles through 1, -1, 0.5, 3 and the largest finite value."""
    vals = torch.tensor([1.0, -1.0, 0.5, 3.0, torch.finfo(dtype).max], dtype=torch.float32).to(dtype)
    n = 1
    for s in shape:
        n *= s
    return vals[torch.arange(n) % 5].view(tuple(shape)).clone()


# ---------------------------------------------------------------------------
# references that oracle/ops.py does not have
# ---------------------------------------------------------------------------
def sum_slabs(partial: Tensor) -> Tensor:
    """fp32 slabs [n_splits, ...] added strictly in split order: ((s0 + s1) + s2) + ..."""
    acc = partial[0].clone()
    for s in range(1, partial.shape[0]):
        acc = acc + partial[s]
    return acc


def add_rms_norm_slabs(partial: Tensor, residual: Tensor, weight: Tensor, eps: float) -> Tuple[Tensor, Tensor]:
    """hx_add_rms_norm_slabs: a = (T) sum of the slabs in split order [1 rounding]; h = (T)(a + residual) [1 rounding];
    out = oracle.ops.rms_norm_kernel(h) [2 roundings: (T)(h * s), then * w].  Returns (h, out)."""
    dt = residual.dtype
    a = sum_slabs(partial).to(dt)
    h = (a.to(torch.float32) + residual.to(torch.float32)).to(dt)
    return h, ops.rms_norm_kernel(h, weight, eps)


def silu_and_mul_slabs(partial: Tensor, inter: int, dtype: torch.dtype) -> Tensor:
    """hx_silu_and_mul_slabs on slabs [n_splits, rows, 2 * inter]: gate | up = (T) sum of the slabs in split order
    [1 rounding each]; s = oracle.ops.silu_kernel(gate) [1 rounding]; out = (T)(s * up) [1 rounding]."""
    gu = sum_slabs(partial).to(dtype)
    s = ops.silu_kernel(gu[..., :inter])
    return (s.to(torch.float32) * gu[..., inter:2 * inter].to(torch.float32)).to(dtype)


def rope_set_kv_cache(query: Tensor, key: Tensor, value: Tensor, positions: Tensor, cos_sin: Tensor, rotary_dim: int,
                      slot_ids: Tensor, key_cache: Tensor, value_cache: Tensor) -> Tuple[Tensor, Tensor]:
    """hx_rope_set_kv_cache: oracle.ops.apply_rotary_pos_emb (NeoX form) on every token, then oracle.ops.set_kv_cache of
    the rotated keys and the values of the tokens whose slot is not negative.  Returns the rotated (query, key); writes
    key_cache / value_cache in place."""
    q, k = ops.apply_rotary_pos_emb(query, key, positions, cos_sin, rotary_dim, False)
    keep = slot_ids >= 0
    ops.set_kv_cache(slot_ids[keep], k[keep], value[keep], key_cache, value_cache)
    return q, k


def quick_gelu(x: Tensor) -> Tensor:
    """x * sigmoid(1.702 x) as the three torch ops of the reference's QuickGELU round it: t = (T)(1.702 x),
    s = (T)sigmoid(t), out = (T)(x * s) — three T roundings, each product rounded to fp32 first."""
    dt = x.dtype
    xf = x.to(torch.float32)
    t = (xf * 1.702).to(dt)
    s = torch.sigmoid(t)
    return (xf * s.to(torch.float32)).to(dt)


# ---------------------------------------------------------------------------
# elements left out of the 1-ulp comparison with the reference, by name
# ---------------------------------------------------------------------------
# Outputs of the form out = (T)(first * second), first itself rounded to T (rms_norm: first = (T)(x * s), second = the
# weight; silu * up: first = (T)silu(gate), second = up).  Where the kernel's `first` sits its allowed 1 ulp from the
# reference's (another fp32 summation order of the row statistic; the fast exp of silu) and the product lands in the
# upper half of its binade, the reference's second rounding turns that one ulp into two.  Neither side is wrong; the
# seven fp16 elements below are the ones where it happens in tests/test_gpu_rowwise_branches.py (seeded inputs), with
# what the MI355X gave.  case -> [(index, out, ref, first, first_ref, second)]
DOUBLED_ULP = {
    "add_rms_norm torch.float16 hidden 2048 misaligned False scale 1024.0 zero row False": [
        ((0, 897), 1.8759765625, 1.8779296875, 2.38671875, 2.388671875, 0.7861328125)],
    "silu_and_mul_slabs torch.float16 M 17 hidden 4096 inter 2816 splits 6": [
        ((3, 434), -0.12451171875, -0.1243896484375, -0.167724609375, -0.1676025390625, 0.7421875),
        ((7, 1305), 0.3427734375, 0.34228515625, -0.167724609375, -0.1676025390625, -2.04296875),
        ((16, 1680), 0.495361328125, 0.494873046875, -0.167724609375, -0.1676025390625, -2.953125)],
    "silu_and_mul_slabs torch.float16 M 17 hidden 4096 inter 2816 splits 12": [
        ((6, 1286), -0.19921875, -0.198974609375, -0.167724609375, -0.1676025390625, 1.1875),
        ((7, 2689), -0.432861328125, -0.432373046875, -0.167724609375, -0.1676025390625, 2.580078125),
        ((16, 191), 0.48095703125, 0.48046875, -0.167724609375, -0.1676025390625, -2.8671875)],
}
