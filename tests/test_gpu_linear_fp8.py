"""GPU: hx_linear_decode_fp8w and hx_dequant_fp8_block (csrc/gemm_skinny_fp8.hip) on the inputs of tests/linear_fp8_ref.py.

1. exact case: torch.equal against the float64 product, fp16 and bf16, M in {1, 16, 17, 33, 64}, on the cheapest shapes
   that reach every (waves, row groups per wave) the dispatch picks by itself (SHAPES) and, on (384, 2816), every pair that
   can be forced.  The workspace is NaN-poisoned with a guard tail, the output a strided view whose gaps must hold, the
   bytes the middle [N, K] of a larger buffer of 0x7F (NaN) bytes — above, below and in the row gaps (ldw > K) — and the
   scales sit between NaN floats: a stray read shows up as a NaN.
2. fine scales: torch.equal against the float64 value rounded once (the rounded-weight mutant differs, CPU test).
3. a NaN byte is a NaN weight.  4. random inputs within the 16-bit entry's tolerance.  5. hx_dequant_fp8_block bit for bit.
6. LAST BUT ONE: every gemm_skinny_fp8w_kernel instantiation of the built library was launched by this file.
7. LAST: the shims' refusals."""
import os
import sys

import pytest
import torch

from tests import gemm_exact as G
from tests import linear_fp8_ref as L8
from tests import moe_fp8_ref as F8

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = {"F16": torch.float16, "BF16": torch.bfloat16}
ROWS = (1, 16, 17, 33, 64)
# units = N / 16 * splits.  <= 32 rows: (4, 1) up to 1024 units, (4, 2) up to 4096, (8, 2) above; 33 .. 64 rows: (4, 1) up to
# 1024, (8, 1) up to 2048, (8, 2) above
SHAPES = (
    (128, 256),         # 8 units, one short split: 4 x 1 / 4 x 1
    (384, 2816),        # 72 units, a short last split of 768 k: 4 x 1 / 4 x 1
    (128, 11008),       # 88 units, 11 splits: 4 x 1 / 4 x 1
    (16512, 256),       # 1032 units: 4 x 2 / 8 x 1
    (65664, 256),       # 4104 units = 256.5 workgroups of 16 row groups, a ragged last workgroup: 8 x 2 / 8 x 2
)
FORCIBLE = {1: ((4, 1), (4, 2), (8, 2)), 2: ((4, 1), (4, 2), (8, 2)), 4: ((4, 1), (8, 1), (8, 2))}
LAUNCHED = {}       # (dtype name, MB, R, NW) -> (N, K)
PAD_ROWS, PAD_COLS, PAD_SCALE = 3, 32, 5


def _set(name, value):
    from hydrainfer_amd import _lib
    assert _lib.lib().hx_debug_set_option(name, value) == 0


def _weight(q, scale):
    """The device operands: q as the middle [N, K] of a (N + 2 PAD_ROWS, K + PAD_COLS) buffer of NaN bytes, scale
    between NaN floats."""
    N, K = q.shape
    big = torch.full((N + 2 * PAD_ROWS, K + PAD_COLS), F8.NAN_BYTE, dtype=torch.uint8)
    big[PAD_ROWS:PAD_ROWS + N, :K] = q
    big = big.to(DEV)
    flat = torch.full((scale.numel() + 2 * PAD_SCALE,), float("nan"))
    flat[PAD_SCALE:PAD_SCALE + scale.numel()] = scale.reshape(-1)
    flat = flat.to(DEV)
    wq = big[PAD_ROWS:PAD_ROWS + N, :K]
    assert wq.stride(0) == K + PAD_COLS and wq.data_ptr() % 16 == 0
    return wq, flat[PAD_SCALE:PAD_SCALE + scale.numel()].view(scale.shape)


def _run(x, wq, sc, what, dname, nan_columns=0):
    """hx_linear_decode_fp8w on x [M, K] (device) with a poisoned workspace and a strided, sentinel-gapped output.
    nan_columns: the output columns whose slabs legitimately hold NaN (a NaN weight)."""
    from hydrainfer_amd import _lib
    from hydrainfer_amd._C.kernel import gemm
    M, K = x.shape
    N = wq.shape[0]
    floats = gemm.workspace_floats(M, N, K)
    ws = G.poisoned(floats, DEV)
    out = G.strided(torch.zeros((M, N), dtype=x.dtype, device=DEV), 4, G.SENTINEL)
    _lib.check(_lib.lib().hx_linear_decode_fp8w(out.data_ptr(), x.data_ptr(), wq.data_ptr(), sc.data_ptr(), M, N, K, x.stride(0),
                                                wq.stride(0), out.stride(0), ws.data_ptr(), floats * 4, _lib.dtype_code(x),
                                                _lib.current_stream()), what)
    if nan_columns:         # the NaN of a NaN weight lands in its split's slab: M x columns floats, nothing else; guard intact
        assert int(torch.isnan(ws[:floats]).sum()) == M * nan_columns and bool((ws[floats:] == G.SENTINEL).all()), what
    else:
        G.checked(ws, floats, what)
    assert G.gaps_hold(out, 4, G.SENTINEL), f"{what}: the gap columns of the output were written"
    nw, r = gemm.fp8_plan(M, N, K)
    mb = (M + 15) // 16
    LAUNCHED.setdefault((dname, 4 if mb == 3 else mb, r, nw), (N, K))
    return out.cpu()


def _describe(got, ref):
    bad = (got != ref) | torch.isnan(got)
    first = bad.nonzero()[0].tolist() if bad.any() else None
    return f"{int(bad.sum())} of {bad.numel()} differ, first at {first}: got {got[tuple(first)]}, want {ref[tuple(first)]}" if first else "equal"


@pytest.mark.parametrize("N,K", SHAPES)
def test_exact_case_every_dispatch_choice(N, K):
    from hydrainfer_amd._C.kernel import gemm
    c = L8.exact_case(N, K)
    wq, sc = _weight(c.q, c.scale)
    seen = set()
    for dname, dt in DTYPES.items():
        xd = G.strided(c.x.to(dt).to(DEV), 8)
        for M in ROWS:
            got = _run(xd[:M], wq, sc, f"{dname} M={M} [{N}, {K}]", dname)
            want = c.ref[:M].to(dt)
            assert torch.equal(got, want), f"{dname} M={M} [{N}, {K}] {gemm.fp8_plan(M, N, K)}: {_describe(got.double(), want.double())}"
            seen.add((M > 32, gemm.fp8_plan(M, N, K)))
    print(f"[{N}, {K}]: (33 .. 64 rows, (waves, row groups)) {sorted(seen)}")


def test_exact_case_every_forcible_configuration():
    """(384, 2816): 24 row groups — 8 x 2 leaves a ragged second workgroup — and a short last split, under every pair."""
    N, K = 384, 2816
    c = L8.exact_case(N, K)
    wq, sc = _weight(c.q, c.scale)
    try:
        for dname, dt in DTYPES.items():
            xd = c.x.to(dt).to(DEV)
            for M in ROWS:
                mb = (M + 15) // 16
                for nw, r in FORCIBLE[4 if mb == 3 else mb]:
                    _set(b"gemm_fp8_waves", nw); _set(b"gemm_fp8_rows_per_wave", r)
                    got = _run(xd[:M], wq, sc, f"{dname} M={M} forced {nw} x {r}", dname)
                    want = c.ref[:M].to(dt)
                    assert torch.equal(got, want), f"{dname} M={M} forced {nw} x {r}: {_describe(got.double(), want.double())}"
    finally:
        _set(b"gemm_fp8_waves", 0); _set(b"gemm_fp8_rows_per_wave", 0)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_fine_scales_one_rounding(dname):
    dt = DTYPES[dname]
    c = L8.fine_case()
    wq, sc = _weight(c.q, c.scale)
    got = _run(c.x.to(dt).to(DEV), wq, sc, f"{dname} fine scales", dname)
    want = L8.fine_out(c, dt)
    assert torch.equal(got, want), _describe(got.double(), want.double())


@pytest.mark.parametrize("dname", list(DTYPES))
def test_a_nan_byte_is_a_nan_weight(dname):
    """0x7F at (n0, k0) and 0xFF at (n1, k1): exactly those output columns are NaN — in every row: x[m][k] * NaN is NaN
    whatever x[m][k] is, zero included (IEEE 754; the float64 reference says the same) — and every other output is the
    exact case's."""
    dt = DTYPES[dname]
    N, K = 384, 2816
    c = L8.exact_case(N, K)
    q = c.q.clone()
    (n0, k0), (n1, k1) = (130, 2815), (17, 1024)
    q[n0, k0], q[n1, k1] = 0x7F, 0xFF
    x = c.x.clone()
    x[::2, k0] = 0.0                                      # rows whose x is zero at the NaN weight
    x[1::2, k0] = 0.25
    wq, sc = _weight(q, c.scale)
    for M in (5, 64):
        got = _run(x[:M].to(dt).to(DEV), wq, sc, f"{dname} NaN byte M={M}", dname, nan_columns=2)
        want = (x[:M].double() @ F8.dequant(q, c.scale).double().t()).to(dt)
        nan = torch.zeros((M, N), dtype=torch.bool)
        nan[:, n0] = nan[:, n1] = True
        assert torch.equal(torch.isnan(want), nan)
        assert torch.equal(torch.isnan(got), nan), f"M={M}: NaN at {torch.isnan(got).nonzero().tolist()[:8]}"
        assert torch.equal(got[~nan], want[~nan])


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("N,K", [(256, 2816), (128, 11008)])
def test_random_inputs_within_the_16_bit_entrys_tolerance(dname, N, K):
    from hydrainfer_amd._C.kernel.gemm import linear_decode_fp8
    from hydrainfer_amd._C.kernel.moe.experts import quantize_fp8_block
    dt = DTYPES[dname]
    g = torch.Generator().manual_seed(N + K)
    x = torch.randn((64, K), generator=g).to(dt)
    q, s = quantize_fp8_block(torch.randn((N, K), generator=g) * 0.02)
    ref = x.double() @ F8.dequant(q.view(torch.uint8), s).double().t()
    qd, sd = q.to(DEV), s.to(DEV)
    for M in (1, 32, 64):
        got = linear_decode_fp8(x[:M].to(DEV), qd, sd).cpu().double()
        tol = L8.tolerance(ref[:M], dt)
        err = (got - ref[:M]).abs()
        print(f"{dname} [{N}, {K}] M={M}: worst error {float((err / tol).max()):.2f} of the tolerance")
        assert bool((err <= tol).all()), f"M={M}: max err {float(err.max())}"


@pytest.mark.parametrize("dname", list(DTYPES))
def test_dequant_fp8_block_is_bit_identical(dname):
    from hydrainfer_amd._C.kernel.gemm import dequant_fp8_block
    from hydrainfer_amd._C.kernel.moe.experts import dequantize_fp8_block, quantize_fp8_block
    dt = DTYPES[dname]
    g = torch.Generator().manual_seed(5)
    q, s = quantize_fp8_block(torch.randn((256, 384), generator=g) * 0.05)
    s = s * (1 + torch.rand(s.shape, generator=g))        # scales with full mantissas
    q8 = q.view(torch.uint8).clone()
    q8[3, 7], q8[200, 383] = 0x7F, 0xFF
    want = dequantize_fp8_block(q8, s).to(dt)
    out = G.strided(torch.zeros((256, 384), dtype=dt, device=DEV), 8, G.SENTINEL)
    got = dequant_fp8_block(q8.to(DEV).view(F8.FP8), s.to(DEV), dt, out=out)
    assert got.data_ptr() == out.data_ptr() and G.gaps_hold(out, 8, G.SENTINEL)
    got = got.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(want).sum()) == 2
    assert torch.equal(got.view(torch.int16)[~torch.isnan(want)], want.view(torch.int16)[~torch.isnan(want)])


# ---- the coverage gate: it judges what the tests above launched ------------------------------------------------------
def test_every_built_instantiation_was_launched():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_table
    prefix = "gemm_skinny_fp8w_kernel<"
    built = sorted(r["name"] for r in kernel_table.kernels() if r["name"].startswith(prefix))
    launched = sorted(f"{prefix}{d}, {mb}, {r}, {nw}>" for d, mb, r, nw in LAUNCHED)
    assert len(built) == 18, built
    missing = [b for b in built if b not in launched]
    assert not missing, f"{len(missing)} of {len(built)} built instantiations were never launched: {missing}"
    assert not [n for n in launched if n not in built], "launched but not built"
    # ... and the dispatch reaches each of them by itself (no option set)
    own = {(mb, cfg) for mb in (1, 2, 4) for cfg in _own_choices(mb)}
    assert own == {(mb, cfg) for mb in FORCIBLE for cfg in FORCIBLE[mb]}


def _own_choices(mb):
    from hydrainfer_amd._C.kernel import gemm
    return {gemm.fp8_plan(16 * mb, N, K) for N, K in SHAPES}


# ---- the shims' refusals, last -----------------------------------------------------------------------------------------
def test_shims_refuse_what_does_not_fit():
    from hydrainfer_amd import _lib
    from hydrainfer_amd._C.kernel import gemm
    x = torch.zeros((2, 256), dtype=torch.bfloat16, device=DEV)
    q = torch.zeros((128, 256), dtype=torch.uint8, device=DEV)
    s = torch.ones((1, 2), device=DEV)
    assert gemm.fp8_supported(x, q, s) and torch.equal(gemm.linear_decode_fp8(x, q, s).cpu(), torch.zeros((2, 128), dtype=torch.bfloat16))
    x65 = torch.zeros((65, 256), dtype=torch.bfloat16, device=DEV)
    assert not gemm.fp8_supported(x65, q, s)
    q384, s384 = torch.zeros((128, 384), dtype=torch.uint8, device=DEV), torch.ones((1, 3), device=DEV)
    for bad in (lambda: gemm.linear_decode_fp8(x65, q, s),                                               # M above 64
                lambda: gemm.linear_decode_fp8(x.float(), q, s), lambda: gemm.linear_decode_fp8(x, q.to(torch.bfloat16), s),
                lambda: gemm.linear_decode_fp8(x, q, s.double()), lambda: gemm.linear_decode_fp8(x, q, s.cpu()),
                lambda: gemm.linear_decode_fp8(x, q, torch.ones((2, 1), device=DEV)),                    # scale shape
                lambda: gemm.linear_decode_fp8(x, q[:64], torch.ones((0, 2), device=DEV)),               # N % 128
                lambda: gemm.linear_decode_fp8(torch.zeros((2, 384), dtype=torch.bfloat16, device=DEV), q384, s384),   # K % 256
                lambda: gemm.linear_decode_fp8(x, q, s, out=torch.zeros((2, 128), dtype=torch.float16, device=DEV)),
                lambda: gemm.dequant_fp8_block(q, s, torch.float32), lambda: gemm.dequant_fp8_block(q, s.double(), torch.float16),
                lambda: gemm.dequant_fp8_block(q.to(torch.float16), s, torch.float16),
                lambda: gemm.dequant_fp8_block(q, torch.ones((2, 1), device=DEV), torch.float16),
                lambda: gemm.dequant_fp8_block(q, s, torch.float16, out=torch.zeros((128, 256), dtype=torch.bfloat16, device=DEV))):
        with pytest.raises(_lib.HydraHipError):
            bad()
    assert gemm.dequant_fp8_block(q384, s384, torch.float16).shape == (128, 384)      # K % 128 is enough to dequantise
