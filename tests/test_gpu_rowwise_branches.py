"""Every dispatch branch of the row-wise kernels (csrc/norm_rope_act.hip) and of the cache scatter (csrc/cache_ops.hip):
element fallbacks, chunk loops, negative slots, the scalar NeoX rope, the fused rope + cache write off its one production
shape, RMSNorm through every launcher arm, the slab consumers past one batch of splits, the activations over every finite
16-bit input, the id clamp of the embedding gather.  Outputs (and in-place operands) sit in buffers that notice a write
outside them (tests/rowwise_ref.py: guarded).

The bars are the ones the older tests of the same kernels use (tests/test_gpu_ops.py): the references are oracle/ops.py
and the few additions of tests/rowwise_ref.py, which tests/test_rowwise_ref_cpu.py checks on the CPU."""
import pytest
import torch

from oracle import ops
from tests import rowwise_ref as R
from tests.util import assert_ulp_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES16 = [F16, BF16]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, g, dt, scale=1.0):
    return (scale * torch.randn(shape, generator=g)).to(dt)


def _assert_bits(got, want, what):
    assert R.same_bits(got, want), f"{what}: {int((got.cpu() != want.cpu()).sum())} of {want.numel()} elements differ"


def _assert_product_chain(out, ref, first, first_ref, second, what, max_ulp, min_exact_frac=0.0):
    """For outputs of the form out = (T)(first * second) with first itself a value rounded to T (rms_norm: first = the
    normalised (T)(x * s), second = the weight; silu * up: first = (T)silu(gate), second = up).  `first` is what the
    KERNEL rounded to, read back through a second launch whose second operand is 1.

    The bar (max_ulp of T from the reference, min_exact_frac bit-exact) holds for `first`, all elements, and for `out`,
    all elements but the ones that tests/rowwise_ref.py names in DOUBLED_ULP for this case (seven fp16 elements in the
    whole file, listed there with their values: the reference's second rounding doubles a 1-ulp difference that the bar
    allows at the first).  Those are held to the values recorded for them.  And out == (T)(first * second) bit for bit,
    for every element."""
    out, ref, first, first_ref, second = (t.detach().cpu() for t in (out, ref, first, first_ref, second))
    dt = out.dtype
    assert_ulp_close(first, first_ref, max_ulp=max_ulp, min_exact_frac=min_exact_frac, what=what + " (first rounding)")
    _assert_bits(out, (first.float() * second.float()).to(dt), what + " (product of the kernel's own first rounding)")
    keep = torch.ones(out.shape, dtype=torch.bool)
    for idx, o, r, f, fr, _ in R.DOUBLED_ULP.get(what, []):
        assert (float(out[idx]), float(ref[idx]), float(first[idx]), float(first_ref[idx])) == (o, r, f, fr), (what, idx)
        keep[idx] = False
    assert_ulp_close(out[keep], ref[keep], max_ulp=max_ulp, min_exact_frac=min_exact_frac, what=what)


# ---------------------------------------------------------------------------
# 1 - 3: cache scatter
# ---------------------------------------------------------------------------
def _scatter(dt, heads, dim, bs, n_tokens, n_blocks, mis_src=False, mis_cache=False, negative=False, seed=0):
    """set_kv_cache and set_image_cache of n_tokens rows into a guarded pool against the oracle op on a CPU clone: the
    whole pool bit for bit.  Tokens with slot -1 are left out of the oracle's input."""
    from hydrainfer_amd._C.kernel import cache_kernels, kv_cache_kernels
    g = _gen(seed)
    k, v = _randn((n_tokens, heads, dim), g, dt), _randn((n_tokens, heads, dim), g, dt)
    slots = torch.randperm(n_blocks * bs, generator=g)[:n_tokens].to(torch.int32)
    if negative:
        slots[::3] = -1
    shape = (n_blocks, bs, heads, dim)
    init = [_randn(shape, g, dt) for _ in range(3)]
    pools, checks = zip(*(R.guarded(shape, dt, DEV, misalign=mis_cache) for _ in range(3)))
    for p, i in zip(pools, init):
        p.copy_(i)
    kc, vc, ic = pools
    kd = R.misaligned(k.to(DEV)) if mis_src else k.to(DEV)
    vd = R.misaligned(v.to(DEV)) if mis_src else v.to(DEV)
    kv_cache_kernels.set_kv_cache(slots.to(DEV), kd, vd, kc, vc)
    cache_kernels.set_image_cache(slots.to(DEV), kd, ic)
    keep = slots >= 0
    kc_ref, vc_ref, ic_ref = (i.clone() for i in init)
    ops.set_kv_cache(slots[keep], k[keep], v[keep], kc_ref, vc_ref)
    ops.set_image_cache(slots[keep], k[keep], ic_ref)
    what = f"{dt} rows {heads}x{dim} bs {bs} mis_src {mis_src} mis_cache {mis_cache}"
    _assert_bits(kc, kc_ref, what + " key cache")
    _assert_bits(vc, vc_ref, what + " value cache")
    _assert_bits(ic, ic_ref, what + " image cache")
    for c in checks:
        c()
    assert not R.same_bits(kc, init[0])            # something landed


@pytest.mark.parametrize("dt", DTYPES16 + [F32])
def test_scatter_rows_elem_fallback(dt):
    """scatter_rows_elem<uint16_t / uint32_t, 1 / 2>: rows that are no multiple of 16 bytes, 16-byte rows from a
    misaligned source, 16-byte rows into a misaligned cache."""
    vec = 16 // torch.empty((), dtype=dt).element_size()
    odd_rows = [(1, 3)] if dt == F32 else [(1, 4), (3, 12)]
    for bs in (4, 16):
        for heads, dim in odd_rows:
            _scatter(dt, heads, dim, bs, 37, 20, seed=bs + dim)
        _scatter(dt, 1, vec, bs, 37, 20, mis_src=True, seed=bs + 1)
        _scatter(dt, 1, vec, bs, 37, 20, mis_cache=True, seed=bs + 2)


@pytest.mark.parametrize("dt,heads,dim", [pytest.param(F16, 2, 64, id="vec-fp16"), pytest.param(BF16, 3, 12, id="elem-bf16"),
                                           pytest.param(F32, 1, 3, id="elem-fp32")])
def test_scatter_negative_slots_write_nothing(dt, heads, dim):
    """slot < 0 in scatter_rows_vec16 and scatter_rows_elem: a third of the tokens are skipped, the rest land."""
    for bs in (4, 16):
        _scatter(dt, heads, dim, bs, 37, 20, negative=True, seed=bs)


@pytest.mark.parametrize("dim", [pytest.param(8, id="vec"), pytest.param(4, id="elem")])
def test_scatter_more_than_65535_tokens(dim):
    """launch_scatter's loop over chunks of 65535 tokens: 65535 + 2 tokens with distinct slots — the last two tokens
    are the second launch, whose source and slot pointers are offset by the first chunk."""
    _scatter(F16, 1, dim, 16, 65535 + 2, 4097, seed=dim)


# ---------------------------------------------------------------------------
# 4: rope, scalar NeoX form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES16 + [F32])
def test_rope_kernel_scalar_neox_form(dt):
    """rope_kernel with interleaved == 0, chosen because half % N != 0, because a base is misaligned, or because a
    token stride is no multiple of 16 bytes: bit-exact against the oracle (the bar of test_rope_bit_exact), bit-identical
    to the vector kernel on the same data, nothing outside q / k written."""
    from hydrainfer_amd._C.kernel import position_embedding as pe
    H, HK, n = 4, 2, 5
    g = _gen(11)
    pos = torch.tensor([0, 3, 63, 17, 40], dtype=torch.int32)

    # rotary 20 of 32: half = 10
    D, rot = 32, 20
    q, k = _randn((n, H, D), g, dt), _randn((n, HK, D), g, dt)
    cs = ops.build_cos_sin_cache(rot, 64, 1e4, dt)
    (qd, qc), (kd, kc) = R.guarded(q.shape, dt, DEV), R.guarded(k.shape, dt, DEV)
    qd.copy_(q), kd.copy_(k)
    pe.apply_rotary_pos_emb(qd, kd, pos.to(DEV), cs.to(DEV), rot, False)
    q_ref, k_ref = ops.apply_rotary_pos_emb(q, k, pos, cs, rot, False)
    _assert_bits(qd, q_ref, f"{dt} rotary 20/32 q")
    _assert_bits(kd, k_ref, f"{dt} rotary 20/32 k")
    _assert_bits(qd[..., rot:], q[..., rot:], "pass-through dims of q")
    _assert_bits(kd[..., rot:], k[..., rot:], "pass-through dims of k")
    qc(), kc()

    # full rotary 64 on a misaligned q, next to its aligned twin (vector kernel)
    D = rot = 64
    q, k = _randn((n, H, D), g, dt), _randn((n, HK, D), g, dt)
    cs = ops.build_cos_sin_cache(rot, 64, 1e4, dt)
    q_ref, k_ref = ops.apply_rotary_pos_emb(q, k, pos, cs, rot, False)
    (qm, qmc), (km, kmc) = R.guarded(q.shape, dt, DEV, misalign=True), R.guarded(k.shape, dt, DEV)
    (qa, qac), (ka, kac) = R.guarded(q.shape, dt, DEV), R.guarded(k.shape, dt, DEV)
    for t, s in ((qm, q), (km, k), (qa, q), (ka, k)):
        t.copy_(s)
    pe.apply_rotary_pos_emb(qm, km, pos.to(DEV), cs.to(DEV), rot, False)
    pe.apply_rotary_pos_emb(qa, ka, pos.to(DEV), cs.to(DEV), rot, False)
    _assert_bits(qm, q_ref, f"{dt} misaligned q")
    _assert_bits(km, k_ref, f"{dt} misaligned k")
    _assert_bits(qm, qa, "scalar against vector kernel, q")
    _assert_bits(km, ka, "scalar against vector kernel, k")
    for c in (qmc, kmc, qac, kac):
        c()
    # the same through a misaligned copy made by the shared helper
    qm2, km2 = R.misaligned(q.to(DEV)), k.to(DEV)
    pe.apply_rotary_pos_emb(qm2, km2, pos.to(DEV), cs.to(DEV), rot, False)
    _assert_bits(qm2, q_ref, f"{dt} misaligned() q")

    # q / k whose token stride is 2 elements past a multiple of 8: the gaps between the rows are guard
    q, k = _randn((n, H, D), g, dt), _randn((n, HK, D), g, dt)
    (qs, qsc), (ks, ksc) = R.guarded(q.shape, dt, DEV, row_stride=H * D + 2), R.guarded(k.shape, dt, DEV, row_stride=HK * D + 2)
    qs.copy_(q), ks.copy_(k)
    pe.apply_rotary_pos_emb(qs, ks, pos.to(DEV), cs.to(DEV), rot, False)
    q_ref, k_ref = ops.apply_rotary_pos_emb(q, k, pos, cs, rot, False)
    _assert_bits(qs, q_ref, f"{dt} odd token stride q")
    _assert_bits(ks, k_ref, f"{dt} odd token stride k")
    qsc(), ksc()


# ---------------------------------------------------------------------------
# 5: fused rope + cache write
# ---------------------------------------------------------------------------
ROPE_CACHE_GRID = [(8, 2, 64, 64), (8, 8, 128, 64), (4, 1, 256, 128), (8, 2, 64, 32)]


@pytest.mark.parametrize("H,HK,D,rot,dt", [s + (dt,) for s in ROPE_CACHE_GRID for dt in DTYPES16] + [(8, 2, 64, 32, F32)])
def test_rope_cache_neox_vec_kernel_grid(H, HK, D, rot, dt):
    """hx_rope_set_kv_cache off its production shape: GQA, partial rotary (k's tail is copied into the cache), head dims
    64 / 256, fp32, block sizes 16 / 32, caches that are one layer of a 6-D pool, slots at -1.  q, k and both caches bit
    for bit against rope-then-scatter of the oracle; v, the other layer and everything around the buffers unchanged."""
    from hydrainfer_amd._C.kernel import position_embedding as pe
    n, nb = 7, 6
    g = _gen(H + HK + D + rot)
    W = (H + 2 * HK) * D
    cs = ops.build_cos_sin_cache(rot, 512, 1e4, dt)
    for bs in (16, 32):
        qkv = _randn((n, W), g, dt)
        pos = torch.randint(0, 512, (n,), generator=g).to(torch.int32)
        slots = torch.randperm(nb * bs, generator=g)[:n].to(torch.int32)
        slots[2] = slots[5] = -1
        pool = _randn((2, 2, nb, bs, HK, D), g, dt)
        view = lambda t: (t[:, :H * D].view(n, H, D), t[:, H * D:(H + HK) * D].view(n, HK, D), t[:, (H + HK) * D:].view(n, HK, D))
        qd, qc = R.guarded(qkv.shape, dt, DEV)
        pd, pc = R.guarded(pool.shape, dt, DEV)
        qd.copy_(qkv), pd.copy_(pool)
        q, k, v = view(qd)
        pe.rope_set_kv_cache(q, k, v, pos.to(DEV), cs.to(DEV), rot, slots.to(DEV), pd[1, 0], pd[1, 1])
        want, want_pool = qkv.clone(), pool.clone()
        qr, kr, vr = view(qkv)
        q_ref, k_ref = R.rope_set_kv_cache(qr, kr, vr, pos, cs, rot, slots, want_pool[1, 0], want_pool[1, 1])
        want[:, :H * D] = q_ref.reshape(n, -1)
        want[:, H * D:(H + HK) * D] = k_ref.reshape(n, -1)
        _assert_bits(qd, want, f"bs {bs}: q | k | v")
        _assert_bits(pd, want_pool, f"bs {bs}: pool")
        _assert_bits(pd[0], pool[0], f"bs {bs}: the other layer")
        assert not R.same_bits(pd[1], pool[1])
        qc(), pc()


def test_rope_set_kv_cache_refusals_touch_nothing():
    """Each refusal of hx_rope_set_kv_cache returns its status (HX_ERR_SHAPE -2, HX_ERR_STRIDE -3) and leaves every
    buffer as it was.  Straight through the C ABI: the shim cannot express a stride below the row, and its own checks
    would come first for some of the others.  ((head_dim - rotary_dim) % N != 0 cannot be the only failing clause: with
    half % N == 0 and head_dim % N == 0 the difference is a multiple of N; it is reached here together with head_dim % N.)"""
    from hydrainfer_amd import _lib
    lib = _lib.lib()
    dt, H, HK, D, rot, n, bs, nb = F16, 8, 2, 64, 32, 3, 16, 4
    g = _gen(5)
    W = (H + 2 * HK) * D
    qkv = _randn((n, W + 8), g, dt).to(DEV)
    pool = _randn((2, nb, bs, HK, 72), g, dt).to(DEV)                 # room for head_dim up to 72
    mis = R.misaligned(pool[0])
    pos = torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV)
    slots = torch.tensor([5, 9, 33], dtype=torch.int32, device=DEV)
    cs = ops.build_cos_sin_cache(rot, 64, 1e4, dt).to(DEV)
    before = [t.clone() for t in (qkv, pool, mis)]

    def call(head_dim=D, rotary=rot, kc=pool[0], k_stride=W + 8):
        rc = lib.hx_rope_set_kv_cache(qkv.data_ptr(), qkv.data_ptr() + 2 * H * D, qkv.data_ptr() + 2 * (H + HK) * D,
                                      pos.data_ptr(), cs.data_ptr(), slots.data_ptr(), kc.data_ptr(), pool[1].data_ptr(),
                                      n, H, HK, head_dim, rotary, W + 8, k_stride, W + 8, bs, bs * HK * 72, bs * HK * 72,
                                      _lib.HX_F16, _lib.current_stream())
        torch.cuda.synchronize()
        for t, b in zip((qkv, pool, mis), before):
            assert R.same_bits(t, b), "a refused call wrote to a buffer"
        return rc

    assert call(rotary=31) == -2                       # rotary_dim odd
    assert call(rotary=66) == -2                       # rotary_dim > head_dim
    assert call(head_dim=68, rotary=64) == -2          # (head_dim - rotary_dim) % 8 != 0
    assert call(kc=mis) == -3                          # misaligned cache
    assert call(k_stride=HK * D - 8) == -3             # k_stride < HK * D


# ---------------------------------------------------------------------------
# 6: RMSNorm
# ---------------------------------------------------------------------------
def _rms_case(dt, hidden, mis, scale, zero_row, g):
    from hydrainfer_amd._C.kernel import norm
    eps, rows = 1e-5, 3
    bar = dict(max_ulp=4, min_exact_frac=0.0) if dt == F32 else dict(max_ulp=1, min_exact_frac=0.98)
    x, r = _randn((rows, hidden), g, dt, scale), _randn((rows, hidden), g, dt, scale)
    if zero_row:
        x[1] = 0
        r[1] = 0
    w = (1 + 0.1 * torch.randn(hidden, generator=g)).to(dt)
    what = f"{dt} hidden {hidden} misaligned {mis} scale {scale} zero row {zero_row}"
    place = (lambda t: R.misaligned(t.to(DEV))) if mis else (lambda t: t.to(DEV))
    one = torch.ones_like(w)
    # rms_norm
    out, oc = R.guarded(x.shape, dt, DEV)
    norm.rms_norm(out, place(x), w.to(DEV), eps)
    n_gpu = torch.empty_like(out)
    norm.rms_norm(n_gpu, place(x), one.to(DEV), eps)
    _assert_product_chain(out, ops.rms_norm_kernel(x, w, eps), n_gpu, ops.rms_norm_kernel(x, one, eps), w,
                          "rms_norm " + what, **bar)
    oc()
    # add_rms_norm: the residual is r + x in T, bit for bit; the output is the norm of that
    out, oc = R.guarded(x.shape, dt, DEV)
    res, rc = R.guarded(x.shape, dt, DEV, misalign=mis)
    res.copy_(r)
    norm.add_rms_norm(out, res, place(x), w.to(DEV), eps)
    h = r + x
    _assert_bits(res, h, "add_rms_norm residual " + what)
    n_gpu, res1 = torch.empty_like(out), place(r)
    norm.add_rms_norm(n_gpu, res1, place(x), one.to(DEV), eps)
    _assert_bits(res1, h, "add_rms_norm residual (unit weight) " + what)
    _assert_product_chain(out, ops.rms_norm_kernel(h, w, eps), n_gpu, ops.rms_norm_kernel(h, one, eps), w,
                          "add_rms_norm " + what, **bar)
    oc(), rc()


@pytest.mark.parametrize("dt", DTYPES16 + [F32])
def test_rms_norm_every_launcher_arm(dt):
    """launch_rms: the generic kernel through a misaligned base (hidden % N == 0) and through 16-bit hidden > 8192,
    MAXV = 4 at 8192, MAXV = 1 with ADD at 2048, fp32 at 4096 (vector) and 4100 (generic); rows scaled by 2^k and an
    all-zero row.  Bars of test_rms_norm."""
    g = _gen(21)
    cases = [(1024, True), (4096, True)]
    cases += [(4096, False), (4100, False)] if dt == F32 else [(8200, False), (8192, False), (2048, False)]
    scales = {F16: (2.0 ** -10, 1.0, 2.0 ** 10), BF16: (2.0 ** -30, 1.0, 2.0 ** 30), F32: (1.0,)}[dt]
    for hidden, mis in cases:
        for scale in scales:
            _rms_case(dt, hidden, mis, scale, False, g)
        _rms_case(dt, hidden, mis, 1.0, True, g)


# ---------------------------------------------------------------------------
# 7: slab consumers past one batch of splits
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES16)
@pytest.mark.parametrize("M", [1, 17])
def test_slab_sum8_second_batch_of_splits(dt, M):
    """slab_sum8 with n_splits on both sides of its batches of 6 (1, 6, 7, 12, 13), stand-alone: add_rms_norm_slabs'
    residual bit for bit against the split-order reference and its output at the RMSNorm bar; silu_and_mul_slabs within
    1 ulp of T of the reference; the fragment-major forms equal to the row-major ones."""
    from hydrainfer_amd._C.kernel import gemm
    from hydrainfer_amd._C.kernel.activation import silu_and_mul_slabs
    from hydrainfer_amd._C.kernel.norm import add_rms_norm_slabs
    eps = 1e-5
    for hid, inter in ((256, 96), (4096, 2816)):
        for S in (1, 6, 7, 12, 13):
            g = _gen(hid + S + M)
            what = f"{dt} M {M} hidden {hid} inter {inter} splits {S}"
            ps = torch.randn((S, M, hid), generator=g)
            pg = torch.randn((S, M, 2 * inter), generator=g)
            r = _randn((M, hid), g, dt)
            w = (1 + 0.1 * torch.randn(hid, generator=g)).to(dt)
            h_ref, o_ref = R.add_rms_norm_slabs(ps, r, w, eps)
            one = torch.ones_like(w)
            psd, pgd, wd = ps.to(DEV), pg.to(DEV), w.to(DEV)
            out, oc = R.guarded((M, hid), dt, DEV)
            res, rc = R.guarded((M, hid), dt, DEV)
            res.copy_(r)
            add_rms_norm_slabs(out, res, psd, S, wd, eps)
            _assert_bits(res, h_ref, "residual " + what)
            n_gpu, res1 = torch.empty_like(out), r.to(DEV)
            add_rms_norm_slabs(n_gpu, res1, psd, S, one.to(DEV), eps)
            _assert_product_chain(out, o_ref, n_gpu, ops.rms_norm_kernel(h_ref, one, eps), w, "add_rms_norm_slabs " + what,
                                  max_ulp=1, min_exact_frac=0.98)
            oc(), rc()
            res2 = r.to(DEV)
            of = torch.zeros(gemm.fragment_major_elems(M, hid), dtype=dt, device=DEV)
            add_rms_norm_slabs(of, res2, psd, S, wd, eps, fragment_major=True)
            _assert_bits(res2, res, "fragment-major residual " + what)
            _assert_bits(gemm.from_fragment_major(of, M, hid), out, "fragment-major norm " + what)
            a = silu_and_mul_slabs(pgd, S, M, inter, dt)
            p1 = pg.clone()                      # the same gate slabs next to an `up` of exactly 1: the kernel's (T)silu(gate)
            p1[:, :, inter:] = 0
            p1[0, :, inter:] = 1
            s_gpu = silu_and_mul_slabs(p1.to(DEV), S, M, inter, dt)
            gu = R.sum_slabs(pg).to(dt)
            _assert_product_chain(a, R.silu_and_mul_slabs(pg, inter, dt), s_gpu, ops.silu_kernel(gu[:, :inter]), gu[:, inter:],
                                  "silu_and_mul_slabs " + what, max_ulp=1)
            af = silu_and_mul_slabs(pgd, S, M, inter, dt, fragment_major=True)
            _assert_bits(gemm.from_fragment_major(af, M, inter), a, "fragment-major silu * up " + what)


# ---------------------------------------------------------------------------
# 8: activations over every finite 16-bit input, and the untested forms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES16)
def test_activations_every_finite_16_bit_input(dt):
    """silu, silu_and_mul and quick_gelu over all finite patterns of T at the bars of test_silu,
    test_silu_and_mul_equals_unfused and test_quick_gelu_equals_the_three_torch_ops; no NaN for finite inputs."""
    from hydrainfer_amd._C.kernel import activation as act
    x = R.all_finite_16bit(dt)
    u = R.up_cycle(dt, x.shape)
    xd, ud = x.to(DEV), u.to(DEV)
    s = act.silu(xd)
    assert_ulp_close(s.cpu(), ops.silu_kernel(x), max_ulp=1, what=f"silu {dt}")
    m = act.silu_and_mul(xd, ud)
    assert not torch.isnan(m.float()).any()
    _assert_bits(m, s * ud, f"silu_and_mul {dt}")
    q = act.quick_gelu(xd)
    assert not torch.isnan(q.float()).any()
    _assert_bits(q, R.quick_gelu(xd), f"quick_gelu {dt}")


@pytest.mark.parametrize("dt", DTYPES16 + [F32])
def test_silu_elem_kernel_with_mul_and_fp32(dt):
    """silu_elem_kernel<T, MUL = true> through n = 333 and through misaligned gate / up; silu_and_mul in fp32."""
    from hydrainfer_amd._C.kernel import activation as act
    g = _gen(31)
    for rows, n, mis in ((5, 333, False), (5, 512, True), (5, 512, False)):
        gt, up = _randn((rows, n), g, dt, 2.0), _randn((rows, n), g, dt, 2.0)
        place = (lambda t: R.misaligned(t.to(DEV))) if mis else (lambda t: t.to(DEV))
        gd, ud = place(gt), place(up)
        got = act.silu_and_mul(gd, ud)
        what = f"{dt} n {n} misaligned {mis}"
        if dt == F32:       # the fast exp of the CUDA original: test_silu's fp32 bar, then one correctly rounded product
            assert_ulp_close(got.cpu(), ops.silu_kernel(gt) * up, max_ulp=16, what=what)
        else:
            _assert_bits(got, act.silu(gt.to(DEV)) * up.to(DEV), what)
            assert_ulp_close(act.silu(gd).cpu(), ops.silu_kernel(gt), max_ulp=1, what="silu " + what)


# ---------------------------------------------------------------------------
# 9: row chunks and the grid-stride loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES16)
@pytest.mark.parametrize("rows,n", [(65535 + 2, 8), (2, 8 * 16384 + 8 * 256 + 8)])
def test_activation_row_chunks_and_grid_stride(dt, rows, n):
    """launch_silu / launch_quick_gelu: more rows than one grid's y extent (the second launch starts 65535 rows in) and
    more vectors per row than 64 workgroups x 256 threads with a ragged last pass.  The shims allocate their outputs, so
    each op runs once more through the C entry into a guarded output: the same bits, nothing written around it."""
    from hydrainfer_amd import _lib
    from hydrainfer_amd._C.kernel import activation as act
    lib, code, st = _lib.lib(), _lib.dtype_code(torch.empty((), dtype=dt)), _lib.current_stream()
    g = _gen(rows)
    x, u = _randn((rows, n), g, dt, 3.0), _randn((rows, n), g, dt, 2.0)
    x[-1, -1], x[-1, 0] = 2.5, -2.5                 # the very last row is not a row of zeros by chance
    xd, ud = x.to(DEV), u.to(DEV)
    s = act.silu(xd)
    assert_ulp_close(s.cpu(), ops.silu_kernel(x), max_ulp=1, what="silu")
    m = act.silu_and_mul(xd, ud)
    _assert_bits(m, s * ud, "silu_and_mul")
    q = act.quick_gelu(xd)
    _assert_bits(q, R.quick_gelu(xd), "quick_gelu")
    for want, call in ((s, lambda o: lib.hx_silu(o, xd.data_ptr(), rows, n, n, code, st)),
                       (m, lambda o: lib.hx_silu_and_mul(o, xd.data_ptr(), ud.data_ptr(), rows, n, n, n, code, st)),
                       (q, lambda o: lib.hx_quick_gelu(o, xd.data_ptr(), rows, n, n, code, st))):
        out, oc = R.guarded((rows, n), dt, DEV)
        assert call(out.data_ptr()) == 0
        _assert_bits(out, want, "guarded output")
        oc()


# ---------------------------------------------------------------------------
# 10: id clamp of the embedding gather
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES16)
@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_embed_rms_norm_row_clamps_ids(dt, idt):
    """embed_rms_norm_row: ids outside [0, vocab) give the rows of ids 0 / vocab - 1, through hx_embed_rms_norm and
    through hx_decode_step_head."""
    from hydrainfer_amd._C.kernel.norm import decode_step_head, embed_rms_norm, rms_norm
    vocab, hidden = 11, 256
    g = _gen(41)
    table, w = _randn((vocab, hidden), g, dt).to(DEV), _randn((hidden,), g, dt).to(DEV)
    ids = torch.tensor([-1, 0, vocab - 1, vocab, vocab + 5], dtype=idt, device=DEV)
    clamped = torch.tensor([0, 0, vocab - 1, vocab - 1, vocab - 1], device=DEV)
    h_ref = table[clamped]
    x_ref = torch.empty_like(h_ref)
    rms_norm(x_ref, h_ref, w, 1e-5)
    assert not R.same_bits(h_ref[0], h_ref[2])
    for fn in (embed_rms_norm, decode_step_head):
        h, x = fn(ids, table, w, 1e-5)
        _assert_bits(h, h_ref, f"{fn.__name__} h")
        _assert_bits(x, x_ref, f"{fn.__name__} x")
        # and against the oracle, at the bar of test_rms_norm: independent of the project's own rms_norm
        assert_ulp_close(x.cpu(), ops.rms_norm_kernel(h_ref.cpu(), w.cpu(), 1e-5), max_ulp=1, min_exact_frac=0.98,
                         what=f"{fn.__name__} x against the oracle")
