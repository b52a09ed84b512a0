"""GPU: every built instantiation of the decode GEMMs is launched, on inputs whose product is exact in any summation
order (tests/gemm_exact.py; proven on the CPU by tests/test_gemm_exact_cpu.py).

csrc/gemm_xreg.hip builds one kernel per k-steps-per-wave count (KW) of its two tables, times {plain, NORM, EPI,
NORM+EPI}, times one / two 16-row blocks of x for the 32-row kernel.  The shapes here are not written down: for each
wanted (kernel, KW) the cheapest candidate (N, K) whose hx_debug_xreg_plan answer IS that instantiation is taken, and
the last test of this file compares what was launched with the tables read through hx_debug_xreg_built — a new KW
row without a shape that reaches it fails there.

Every product is compared with torch.equal against x.double() @ w.double().t() (or, for the fused NORM / EPI forms,
against the two-launch form they replace); every workspace is NaN before the launch and guarded behind its end."""
import collections

import pytest
import torch

from tests import gemm_exact as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTS = [torch.float16, torch.bfloat16]
# the (kernel, KW) this file has cases for; the coverage gate at the end compares them with what is BUILT
NARROW_KW = (4, 8, 16, 20, 22, 27, 29, 32, 40)
WIDE_KW = (2, 4, 8, 10, 11, 14, 16, 20)
PLAIN = [("narrow", kw) for kw in NARROW_KW] + [("wide", kw) for kw in WIDE_KW]
NARROW_NORM_KW = (4, 8, 16, 32, 40)
WIDE_NORM_KW = (2, 4, 8, 16, 20)
NARROW_SILU_KW = (4, 8, 16, 32, 40)
WIDE_SILU_KW = (16,)
NARROW_ROWS = (1, 13, 16, 17, 29, 32)        # one 16-row block of x, then two
WIDE_ROWS = (33, 47, 64)
WIDE_FEW_ROWS = (8, 20)                      # the wide kernel with one and two row blocks (hx_gate_up_xreg, hx_linear_decode_ex)

# (kernel, KW, row blocks (32-row kernel; 0 for the wide one), EPI, NORM) -> the (N, K) it was launched on
REACHED = collections.defaultdict(set)


def _gemm():
    from hydrainfer_amd._C.kernel import gemm
    return gemm


def _option(name, value):
    from hydrainfer_amd import _lib
    assert _lib.lib().hx_debug_set_option(name, value) == 0


def _mark(pl, N, K, epi=0, norm=0):
    """A launch that the library accepted: remember which instantiation the query says it was."""
    assert pl.ok
    REACHED[(pl.kernel, pl.kw, pl.row_blocks if pl.kernel == "narrow" else 0, epi, norm)].add((N, K))


def _matches(kernel, kw, gate_up=False, epi=False, rows=None, want=lambda N, K, pl: True):
    """Candidate (N, K, plan) whose launch the query answers with this (kernel, KW), cheapest weight first."""
    gemm = _gemm()
    wide = kernel == "wide"
    rows = rows or (64 if wide else 32)
    out = []
    for K in E.K_VALUES:
        for N in (E.GU_N_VALUES if gate_up else E.N_VALUES):
            pl = gemm.xreg_plan(rows, N, K, gate_up, wide, epi)
            if pl.ok and pl.kernel == kernel and pl.kw == kw and want(N, K, pl):
                out.append((N, K, pl))
    assert out, f"no candidate shape reaches the {kernel} kernel with {kw} k-steps per wave (gate_up={gate_up}, epi={epi})"
    return sorted(out, key=lambda c: c[0] * c[1])


def _plain_shapes(kernel, kw):
    """The cheapest shape; the cheapest with N = 4128 (258 row groups over 256 workgroups: two of them own two);
    the cheapest with the most and with the fewest K splits, where those are others (a partial last split, uneven
    halves; the whole K in one workgroup)."""
    cands = _matches(kernel, kw)
    pick = [cands[0]]
    pick += [c for c in cands if c[0] == 4128 and c is not cands[0]][:1]
    for n_splits in (max(c[2].splits for c in cands), min(c[2].splits for c in cands)):
        if all(c[2].splits != n_splits for c in pick):
            pick += [c for c in cands if c[2].splits == n_splits][:1]
    return [(N, K) for N, K, _ in pick]


def _describe(got, ref):
    bad = (got != ref).nonzero()
    m, n = bad[0].tolist()
    return f"{len(bad)} of {ref.numel()} elements differ, the first at [{m}, {n}]: {got[m, n].item()} for {ref[m, n].item()}"


def _product(entry, floats, M, N, pl, ref, what):
    """One plain product into a poisoned workspace: slab count as planned, every float written, none behind the end,
    the float64 sum of the slabs == the float64 product."""
    buf = E.poisoned(floats, DEV)
    s = entry(buf)
    assert s == pl.splits and floats == s * M * N, f"{what}: {s} slabs, planned {pl.splits}, workspace of {floats / (M * N)}"
    got = E.checked(buf, floats, what).view(s, M, N).double().sum(0).cpu()
    assert torch.equal(got, ref), f"{what}: {_describe(got, ref)}"


def _x_forms(x, M, K):
    """name -> (x argument, frag_shape): row-major, fragment-major, and a [:, :K] view of an (M, K + 8) buffer of NaN."""
    gemm = _gemm()
    return {"row-major x": (x, None), "fragment-major x": (gemm.to_fragment_major(x), (M, K)),
            "strided x": (E.strided(x, 8), None)}


# ---- 1. every plain instantiation, exact ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel,kw", PLAIN)
def test_plain_instantiation_is_exact(kernel, kw, dt):
    """hx_linear_decode_partial_xreg on the shapes the query picks for this (kernel, KW): 1 .. 16 and 17 .. 32 rows (the
    32-row kernel's two forms) or 33 .. 64 rows (wide), x row-major / fragment-major / strided, the weight packed from a
    contiguous tensor and from a strided view (same bytes), k rotation off and on."""
    gemm = _gemm()
    wide = kernel == "wide"
    try:
        for (N, K) in _plain_shapes(kernel, kw):
            p = E.problem(64 if wide else 32, N, K)
            w = p.w.to(dt).to(DEV)
            pk = gemm.pack_weight_xreg(w)
            pk_s = gemm.pack_weight_xreg(E.strided(w, 8))
            assert torch.equal(pk, pk_s), f"N={N} K={K}: the packing of a strided weight differs"
            for M in (WIDE_ROWS if wide else NARROW_ROWS):
                pl = gemm.xreg_plan(M, N, K, False, wide)
                assert (pl.kernel, pl.kw, pl.row_blocks) == (kernel, kw, (M + 15) // 16)
                floats = gemm.xreg_workspace_floats(M, N, K)
                for name, (x, fs) in _x_forms(p.x[:M].to(dt).to(DEV), M, K).items():
                    for stagger in (0, 1):
                        _option(b"xreg_stagger", stagger)
                        _product(lambda buf: gemm.linear_decode_partial_xreg(x, pk_s if name == "strided x" else pk, N, buf, frag_shape=fs),
                                 floats, M, N, pl, p.ref[:M], f"{kernel} KW={kw} N={N} K={K} M={M} {dt} {name} stagger={stagger}")
                _mark(pl, N, K)
    finally:
        _option(b"xreg_stagger", 1)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kw", WIDE_KW)
def test_wide_kernel_over_the_interleaved_packing_is_exact(kw, dt):
    """hx_gate_up_xreg (the wide kernel at EVERY row count over the gate|up packing): slab columns in [gate | up]
    order, exact, at 8 and 20 rows (one and two 16-row blocks of x) and at 33 .. 64; where the packing is the one the
    fused epilogue reads, also through DecodeWeight(max_rows=64, gate_up=True) and hx_linear_decode_ex."""
    gemm = _gemm()
    N, K, _ = _matches("wide", kw, gate_up=True)[0]
    inter = N // 2
    p = E.problem(64, N, K, seed=1)
    w = p.w.to(dt).to(DEV)
    pg = gemm.pack_weight_xreg(w, interleave_halves=True)
    assert torch.equal(gemm.pack_weight_xreg(E.strided(w, 8), interleave_halves=True), pg)
    dw = gemm.DecodeWeight(E.strided(w, 8), max_rows=64, gate_up=True)
    assert dw.layout == "xreg"
    if dw.interleaved:
        assert torch.equal(dw.packed, pg)
    else:       # no fused epilogue for this K: the single entry keeps the halves in order and runs the 32-row kernel below 33 rows
        assert kw not in (2, 4, 8, 16, 20), kw
    try:
        for M in WIDE_FEW_ROWS + WIDE_ROWS:
            pl = gemm.xreg_plan(M, N, K, True, True)
            assert (pl.kernel, pl.kw, pl.row_blocks) == ("wide", kw, (M + 15) // 16)
            floats = gemm.gate_up_xreg_workspace_floats(M, inter, K)
            for name, (x, fs) in _x_forms(p.x[:M].to(dt).to(DEV), M, K).items():
                for stagger in (0, 1):
                    _option(b"xreg_stagger", stagger)
                    what = f"wide KW={kw} gate|up N={N} K={K} M={M} {dt} {name} stagger={stagger}"
                    _product(lambda buf: gemm.gate_up_xreg(x, pg, inter, buf, frag_shape=fs), floats, M, N, pl, p.ref[:M], what)
                    if dw.interleaved and M in WIDE_FEW_ROWS:
                        assert dw.workspace_floats(M) == floats
                        _product(lambda buf: gemm.linear_decode_ex(x, dw, buf, frag_shape=fs), floats, M, N, pl, p.ref[:M],
                                 what + " linear_decode_ex")
            _mark(pl, N, K)
    finally:
        _option(b"xreg_stagger", 1)


# ---- 2. one-hot probes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel,kw", PLAIN)
def test_one_hot_probes_return_the_weight_column(kernel, kw, dt):
    """Row m of x is the unit vector at k_m: row m of the product is column k_m of w.  The k_m sit on every boundary
    of the launch's k decomposition (gemm_exact.probe_ks), so a wave that drops its first or last k-step, a split that
    starts one off or a padding slot that is not zero names its k here."""
    gemm = _gemm()
    wide = kernel == "wide"
    rows = 64 if wide else 32
    N, K, pl = _matches(kernel, kw)[0]
    pk_P = 4 * gemm.xreg_plan(32, N, K, False, False).kw        # the packing is the 32-row kernel's
    ks = E.probe_ks(K, kw, wide, pk_P)
    assert len(E.split_ranges(K, kw, wide, pk_P)) == pl.splits
    p = E.problem(rows, N, K)
    w = p.w.to(dt).to(DEV)
    pk = gemm.pack_weight_xreg(w)
    floats = gemm.xreg_workspace_floats(rows, N, K)
    for at in range(0, len(ks), rows):       # (one launch: the list is shorter than the rows for every candidate shape)
        chunk = ks[at:at + rows]
        chunk = chunk + [K - 1] * (rows - len(chunk))
        x1 = E.one_hot_rows(chunk, K)
        E.assert_exact(K, 1.0, E.LEVELS * E.STEP, E.STEP)
        x = gemm.to_fragment_major(x1.to(dt).to(DEV))
        buf = E.poisoned(floats, DEV)
        s = gemm.linear_decode_partial_xreg(x, pk, N, buf, frag_shape=(rows, K))
        assert s == pl.splits
        got = E.checked(buf, floats).view(s, rows, N).double().sum(0).cpu()
        want = p.w[:, chunk].t().double()
        wrong = [k for m, k in enumerate(chunk) if not torch.equal(got[m], want[m])]
        assert not wrong, f"{kernel} kernel, KW={kw}, N={N} K={K} {dt}: the probes at k = {sorted(set(wrong))} do not return w[:, k]"
    _mark(pl, N, K)


# ---- 3. NORM: add + RMSNorm inside the launch --------------------------------------------------------------------------
def _norm_inputs(M, K, S_in, dt, seed):
    g = torch.Generator().manual_seed(seed)
    nw = torch.randn(K, generator=g).to(dt).to(DEV)
    slabs = torch.randn((S_in, M, K), generator=g).to(DEV)
    h = torch.randn((M, K), generator=g).to(dt).to(DEV)
    return nw, slabs, h


def _nan_frag(M, K, dt):
    return torch.full((_gemm().fragment_major_elems(M, K),), float("nan"), dtype=dt, device=DEV)


def _sync():
    return torch.zeros(_gemm().XREG_SYNC_WORDS, dtype=torch.int32, device=DEV)


def _sync_is_clean(sync, M, what):
    assert int(sync[1]) == 0, f"{what}: a workgroup gave up waiting"
    assert int(sync[0]) == M, f"{what}: {int(sync[0])} rows counted in, not {M}"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kernel,kw", [("narrow", kw) for kw in NARROW_NORM_KW] + [("wide", kw) for kw in WIDE_NORM_KW])
def test_norm_fused_instantiation_equals_the_two_launch_form(kernel, kw, dt):
    """hx_norm_linear_decode_xreg == hx_add_rms_norm_slabs_ex (fragment-major) + hx_linear_decode_partial_xreg on the
    same instantiation: residual, x and slabs bit for bit, outputs NaN beforehand, the hand-over area clean."""
    gemm = _gemm()
    from hydrainfer_amd._C.kernel.norm import add_rms_norm_slabs
    wide = kernel == "wide"
    for M in ((47,) if wide else (13, 29)):
        N, K, _ = _matches(kernel, kw, rows=M, want=lambda N, K, pl: pl.packing_splits == 1 and gemm.norm_xreg_supported(M, N, K, dt))[0]
        pl = gemm.xreg_plan(M, N, K, False, wide)
        nw, slabs, h = _norm_inputs(M, K, 3, dt, 17 * kw + M)
        g = torch.Generator().manual_seed(kw)
        pk = gemm.pack_weight_xreg((torch.randn((N, K), generator=g) * 0.03).to(dt).to(DEV))
        floats = gemm.xreg_workspace_floats(M, N, K)
        h1, h2 = h.clone(), h.clone()
        xf, xf2 = _nan_frag(M, K, dt), _nan_frag(M, K, dt)
        a, b, sync = E.poisoned(floats, DEV), E.poisoned(floats, DEV), _sync()
        add_rms_norm_slabs(xf, h1, slabs, 3, nw, 1e-5, fragment_major=True)
        s = gemm.linear_decode_partial_xreg(xf, pk, N, a, frag_shape=(M, K))
        s2 = gemm.norm_linear_decode_xreg(h2, slabs, 3, nw, 1e-5, xf2, pk, N, b, sync)
        what = f"{kernel} KW={kw} NORM N={N} K={K} M={M} {dt}"
        assert s == s2 == pl.splits, what
        _sync_is_clean(sync, M, what)
        assert torch.equal(h1, h2), f"{what}: residual"
        assert torch.equal(gemm.from_fragment_major(xf, M, K), gemm.from_fragment_major(xf2, M, K)), f"{what}: x"
        assert not torch.isnan(gemm.from_fragment_major(xf2, M, K)).any()
        assert torch.equal(E.checked(a, floats, what), E.checked(b, floats, what)), f"{what}: slabs"
        _mark(pl, N, K, norm=1)


# ---- 4. EPI: silu(gate) * up inside the launch ------------------------------------------------------------------------
def _rows_past_m_hold(act, M, inter, fill):
    """Fragment-major act [inter / 32][row block][(k % 32) / 8][row % 16][k % 8]: rows M .. of the last block."""
    pad = (M + 15) // 16 * 16
    if pad == M:
        return True
    return bool((act[:pad * inter].view(inter // 32, pad // 16, 4, 16, 8)[:, -1, :, M % 16:, :] == fill).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kw", NARROW_SILU_KW)
def test_silu_epilogue_instantiation_equals_the_two_launch_form(kw, dt):
    """hx_gate_up_silu_xreg == the product + hx_silu_and_mul_slabs, and hx_norm_gate_up_silu_xreg ==
    hx_add_rms_norm_slabs_ex + hx_gate_up_silu_xreg, bit for bit with the k rotation off, at one and two row blocks, on
    a small weight and on one whose 258 (gate, up) pairs give two workgroups two pairs.  The first comparison runs on
    exact inputs (w drawn 64 times finer, so that gate stays where silu bends): both forms then round the same exact
    sums, whatever their split counts.  act holds a sentinel beforehand; rows past M of the last block keep it."""
    gemm = _gemm()
    from hydrainfer_amd._C.kernel.activation import silu_and_mul_slabs
    from hydrainfer_amd._C.kernel.norm import add_rms_norm_slabs
    w_step = 2.0 ** -8
    cands = _matches("narrow", kw, gate_up=True, epi=True)
    shapes = [cands[0][:2]] + [c[:2] for c in cands if c[0] == 8256][:1]
    try:
        _option(b"xreg_stagger", 0)
        for (N, K) in shapes:
            inter = N // 2
            x_all = E.grid_values((32, K), 3 * K + N)
            w = E.grid_values((N, K), 5 * K + N, w_step)
            E.assert_exact(K, x_all.abs().max().item(), w.abs().max().item(), E.STEP * w_step)
            w = w.to(dt).to(DEV)
            pk, pg = gemm.pack_weight_xreg(w), gemm.pack_weight_xreg(w, interleave_halves=True)
            for M in (13, 16, 29, 32):
                assert gemm.gate_up_silu_supported(M, inter, K, dt)
                pl = gemm.xreg_plan(M, N, K, True, False, True)
                assert (pl.kernel, pl.kw, pl.row_blocks, pl.splits) == ("narrow", kw, (M + 15) // 16, 1)
                x = x_all[:M].to(dt).to(DEV)
                floats = gemm.xreg_workspace_floats(M, N, K)
                ws = E.poisoned(floats, DEV)
                s = gemm.linear_decode_partial_xreg(x, pk, N, ws)
                want = silu_and_mul_slabs(E.checked(ws, floats), s, M, inter, dt)
                assert not torch.isnan(want).any() and not torch.isinf(want).any()
                for name, (xx, fs) in _x_forms(x, M, K).items():
                    what = f"narrow KW={kw} EPI N={N} K={K} M={M} {dt} {name}"
                    act = torch.full((gemm.fragment_major_elems(M, inter),), E.SENTINEL, dtype=dt, device=DEV)
                    gemm.gate_up_silu_xreg(xx, pg, inter, act, frag_shape=fs)
                    assert torch.equal(gemm.from_fragment_major(act, M, inter), want), what
                    assert _rows_past_m_hold(act, M, inter, E.SENTINEL), f"{what}: rows past M of the last block were written"
                _mark(pl, N, K, epi=1)
                # the norm in front of it: against its own two launches (x is whatever the norm gives: same kernel, same order)
                assert gemm.norm_xreg_supported(M, N, K, dt, gate_up=True)
                nw, slabs, h = _norm_inputs(M, K, 2, dt, 19 * kw + M)
                h1, h2 = h.clone(), h.clone()
                xf, xf2, sync = _nan_frag(M, K, dt), _nan_frag(M, K, dt), _sync()
                act1, act2 = (torch.full((gemm.fragment_major_elems(M, inter),), E.SENTINEL, dtype=dt, device=DEV) for _ in range(2))
                add_rms_norm_slabs(xf, h1, slabs, 2, nw, 1e-5, fragment_major=True)
                gemm.gate_up_silu_xreg(xf, pg, inter, act1, frag_shape=(M, K))
                gemm.norm_gate_up_silu_xreg(h2, slabs, 2, nw, 1e-5, xf2, pg, inter, act2, sync)
                what = f"narrow KW={kw} NORM+EPI N={N} K={K} M={M} {dt}"
                _sync_is_clean(sync, M, what)
                assert torch.equal(h1, h2), f"{what}: residual"
                assert torch.equal(gemm.from_fragment_major(xf, M, K), gemm.from_fragment_major(xf2, M, K)), f"{what}: x"
                a1, a2 = gemm.from_fragment_major(act1, M, inter), gemm.from_fragment_major(act2, M, inter)
                assert not torch.isnan(a2).any() and torch.equal(a1, a2), f"{what}: act"
                assert _rows_past_m_hold(act2, M, inter, E.SENTINEL), f"{what}: rows past M of the last block were written"
                _mark(pl, N, K, epi=1, norm=1)
    finally:
        _option(b"xreg_stagger", 1)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kw", WIDE_SILU_KW)
def test_wide_silu_epilogue_equals_the_two_launch_form(kw, dt):
    """hx_norm_gate_up_silu_wide_xreg == hx_norm_gate_up_xreg + hx_silu_and_mul_slabs_ex (fragment-major): residual, x
    and act bit for bit; rows past M of the last block keep the sentinel."""
    gemm = _gemm()
    from hydrainfer_amd._C.kernel.activation import silu_and_mul_slabs
    for M in (36, 47, 64):
        N, K, pl = _matches("wide", kw, gate_up=True, epi=True, rows=M,
                            want=lambda N, K, pl: gemm.gate_up_silu_wide_supported(M, N // 2, K, dt))[0]
        inter = N // 2
        nw, slabs, h = _norm_inputs(M, K, 4, dt, 23 * kw + M)
        g = torch.Generator().manual_seed(kw + 1)
        pg = gemm.pack_weight_xreg((torch.randn((N, K), generator=g) * 0.03).to(dt).to(DEV), interleave_halves=True)
        floats = gemm.gate_up_xreg_workspace_floats(M, inter, K)
        h1, h2 = h.clone(), h.clone()
        xf, xf2, ga = _nan_frag(M, K, dt), _nan_frag(M, K, dt), E.poisoned(floats, DEV)
        sync1, sync2 = _sync(), _sync()
        act = torch.full((gemm.fragment_major_elems(M, inter),), E.SENTINEL, dtype=dt, device=DEV)
        s = gemm.norm_gate_up_xreg(h1, slabs, 4, nw, 1e-5, xf, pg, inter, ga, sync1)
        plain = gemm.xreg_plan(M, N, K, True, True)
        assert s == plain.splits == 2
        want = silu_and_mul_slabs(E.checked(ga, floats), s, M, inter, dt, fragment_major=True)
        gemm.norm_gate_up_silu_wide_xreg(h2, slabs, 4, nw, 1e-5, xf2, pg, inter, act, sync2)
        what = f"wide KW={kw} NORM+EPI N={N} K={K} M={M} {dt}"
        _sync_is_clean(sync1, M, what)
        _sync_is_clean(sync2, M, what)
        assert torch.equal(h1, h2), f"{what}: residual"
        assert torch.equal(gemm.from_fragment_major(xf, M, K), gemm.from_fragment_major(xf2, M, K)), f"{what}: x"
        a2 = gemm.from_fragment_major(act, M, inter)
        assert not torch.isnan(a2).any() and torch.equal(a2, gemm.from_fragment_major(want, M, inter)), f"{what}: act"
        assert _rows_past_m_hold(act, M, inter, E.SENTINEL), f"{what}: rows past M of the last block were written"
        _mark(plain, N, K, norm=1)
        _mark(pl, N, K, epi=1, norm=1)


# ---- 6. the LDS-slice family (csrc/gemm_skinny.hip) -------------------------------------------------------------------
LDS_ROWS = (1, 16, 17, 32, 33, 64)


def _lds_case(p, w, ws_, packed, M, dt, what, entries=("skinny", "skinny strided", "packed", "linear_decode")):
    """x[:M] through the row-major kernel (contiguous and strided operands), the packed kernel, and hx_linear_decode with
    strided x, weight and output: poisoned workspaces, exact slabs, the T output == ref rounded to T."""
    from hydrainfer_amd import _lib
    gemm = _gemm()
    N, K = p.w.shape
    x = p.x[:M].to(dt).to(DEV)
    xs = E.strided(x, 8)
    ref = p.ref[:M]
    floats = gemm.workspace_floats(M, N, K)
    n_splits = (K + 1023) // 1024
    assert floats == n_splits * M * N

    def slabs(entry, name):
        buf = E.poisoned(floats, DEV)
        s = entry(buf)
        assert s == n_splits
        got = E.checked(buf, floats, f"{what} {name}").view(s, M, N).double().sum(0).cpu()
        assert torch.equal(got, ref), f"{what} {name}: {_describe(got, ref)}"

    if "skinny" in entries:
        slabs(lambda buf: gemm.linear_decode_partial(x, w, buf), "row-major weight")
    if "skinny strided" in entries:
        slabs(lambda buf: gemm.linear_decode_partial(xs, ws_, buf), "strided x and weight")
    if "packed" in entries:
        slabs(lambda buf: gemm.linear_decode_partial_packed(xs, packed, N, buf), "packed weight, strided x")
    if "linear_decode" in entries:
        out = E.strided(torch.zeros((M, N), dtype=dt, device=DEV), 4, E.SENTINEL)
        buf = E.poisoned(floats, DEV)
        _lib.check(_lib.lib().hx_linear_decode(out.data_ptr(), xs.data_ptr(), ws_.data_ptr(), M, N, K, xs.stride(0), ws_.stride(0),
                                               out.stride(0), buf.data_ptr(), floats * 4, _lib.dtype_code(x), _lib.current_stream()),
                   "linear_decode")
        E.checked(buf, floats, f"{what} linear_decode")
        assert torch.equal(out.cpu(), ref.to(dt)), f"{what} linear_decode: {_describe(out.cpu().double(), ref.to(dt).double())}"
        assert E.gaps_hold(out, 4, E.SENTINEL), f"{what} linear_decode: the gap columns of the output were written"


def _lds_weights(p, dt):
    gemm = _gemm()
    w = p.w.to(dt).to(DEV)
    ws_ = E.strided(w, 8)
    packed = gemm.pack_weight(w)
    assert torch.equal(gemm.pack_weight(ws_), packed), "pack_weight of a strided weight differs"
    return w, ws_, packed


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N,K", E.LDS_SHAPES)
def test_lds_slice_kernels_are_exact(N, K, dt):
    """gemm_skinny_kernel, gemm_packed_kernel and slab_reduce_kernel on shapes that reach each (waves, row groups per
    wave) the dispatch chooses by itself (tests/gemm_exact.py LDS_SHAPES), at one, two and four 16-row blocks."""
    p = E.problem(64, N, K, seed=2)
    w, ws_, packed = _lds_weights(p, dt)
    for M in LDS_ROWS:
        _lds_case(p, w, ws_, packed, M, dt, f"LDS-slice N={N} K={K} M={M} {dt}")


@pytest.mark.parametrize("dt", DTS)
def test_lds_slice_kernels_are_exact_for_every_forced_configuration(dt):
    """Every (row groups per wave, waves) in {1 .. 4} x {4, 8} on (1056, 2816) — 66 row groups that no configuration
    but 1 x 4 divides, a short last split."""
    N, K = E.LDS_SHAPES[0]
    p = E.problem(64, N, K, seed=2)
    w, ws_, packed = _lds_weights(p, dt)
    try:
        for R in (1, 2, 3, 4):
            for NW in (4, 8):
                _option(b"gemm_rows_per_wave", R)
                _option(b"gemm_waves", NW)
                for M in LDS_ROWS:
                    _lds_case(p, w, ws_, packed, M, dt, f"LDS-slice {NW} waves x {R} row groups, N={N} K={K} M={M} {dt}",
                              entries=("skinny strided", "packed"))
    finally:
        _option(b"gemm_rows_per_wave", 0)
        _option(b"gemm_waves", 0)


# ---- 5. the coverage gate: LAST, it judges what the tests above launched ---------------------------------------------
def test_every_built_instantiation_was_launched():
    """Everything csrc/gemm_xreg.hip builds (its two tables through hx_debug_xreg_built, is_built's rule, one and two row
    blocks for the 32-row kernel) against what the tests of this file launched, as the query named it.  Run with the
    whole file: it fails, listing them, if any built (kernel, KW, row blocks, EPI, NORM) was not reached — none is exempt."""
    gemm = _gemm()

    def is_built(norm_built, silu_built, wide, epi, norm):      # csrc/gemm_xreg.hip is_built
        return (not norm or norm_built) and (not epi or (silu_built and (norm or not wide)))

    built = set()
    for wide in (False, True):
        for kw, norm_built, silu_built in gemm.xreg_built(wide):
            for epi in (0, 1):
                for norm in (0, 1):
                    if is_built(norm_built, silu_built, wide, epi, norm):
                        built |= {("wide", kw, 0, epi, norm)} if wide else {("narrow", kw, mb, epi, norm) for mb in (1, 2)}
    assert len(built) >= 2 * (9 + 5 + 5 + 5) + 8 + 5 + 1
    print("\n(kernel, KW, row blocks, EPI, NORM) -> (N, K) launched")
    for key in sorted(REACHED):
        print(f"  {key} -> {sorted(REACHED[key])}")
    missing = sorted(built - set(REACHED))
    assert not missing, f"{len(missing)} of {len(built)} built instantiations were never launched: {missing}"
    stray = sorted(set(REACHED) - built)
    assert not stray, f"launched but not in the tables: {stray}"
