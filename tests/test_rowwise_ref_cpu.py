"""The references of tests/rowwise_ref.py against fp64 evaluations of the same chains of operations, and the helpers
themselves.  No GPU.

The fp64 evaluation of a reference rounds to T at the same points as the reference and does everything between two
rounding points in fp64 where the reference works in fp32.  The two can then differ only where an fp32 intermediate and
its fp64 twin fall on different sides of a rounding boundary of T — one ulp of T at that rounding point, carried through
the (multiplicative) rest of the chain — so the bound is one ulp of T per rounding point on the way to an output element.
Inputs that would amplify such a flip are avoided by construction and said so where it is done."""
import pytest
import torch

from oracle import ops
from tests import rowwise_ref as R
from tests.util import assert_ulp_close

DTYPES16 = [torch.float16, torch.bfloat16]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES16 + [torch.float32])
def test_misaligned_is_one_element_past_a_16_byte_boundary(dt):
    t = torch.randn((3, 5, 8), generator=_gen(0)).to(dt)
    m = R.misaligned(t)
    assert m.data_ptr() % 16 == t.element_size() and m.is_contiguous() and R.same_bits(m, t)


@pytest.mark.parametrize("dt", DTYPES16 + [torch.float32])
def test_guarded_notices_every_stray_byte(dt):
    es = torch.empty((), dtype=dt).element_size()
    for kw in ({}, {"misalign": True}, {"row_stride": 13}, {"row_stride": 13, "misalign": True}):
        v, check = R.guarded((4, 2, 5), dt, **kw)
        assert v.shape == (4, 2, 5) and v.data_ptr() % 16 == (es if kw.get("misalign") else 0)
        assert v.stride() == (kw.get("row_stride", 10), 5, 1)
        v.copy_(torch.randn((4, 2, 5), generator=_gen(1)).to(dt))        # writing the tensor itself is fine
        check()
        flat = v.view(4, 10)
        for where in ("before", "after") + (("gap",) if "row_stride" in kw else ()):
            # one element next to the tensor: in front of row 0, behind the last row, in the gap behind row 1
            e = {"before": torch.as_strided(flat, (1,), (1,), flat.storage_offset() - 1),
                 "after": torch.as_strided(flat, (1,), (1,), flat.storage_offset() + 3 * flat.stride(0) + 10),
                 "gap": torch.as_strided(flat, (1,), (1,), flat.storage_offset() + flat.stride(0) + 10)}[where]
            old = e.clone()
            e.fill_(1.0)
            with pytest.raises(AssertionError):
                check()
            e.copy_(old)
            check()


@pytest.mark.parametrize("dt", DTYPES16)
def test_exhaustive_grid_holds_every_finite_pattern_once(dt):
    x = R.all_finite_16bit(dt)
    assert x.shape == (8, 8192) and bool(torch.isfinite(x).all())
    n_nonfinite = 2 * (1024 if dt == torch.float16 else 128)            # exponent all ones, either sign
    bits = x.view(torch.int16).flatten().to(torch.int32) & 0xFFFF
    assert torch.unique(bits).numel() == 65536 - n_nonfinite            # (+0 stands in for the non-finite ones)
    assert int((bits == 0).sum()) == 1 + n_nonfinite
    u = R.up_cycle(dt, (8, 8192))
    assert set(u.flatten()[:5].float().tolist()) == {1.0, -1.0, 0.5, 3.0, float(torch.finfo(dt).max)}
    assert R.same_bits(u.flatten()[5:10], u.flatten()[:5])


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def _dyadic_slabs(shape, seed):
    """Multiples of 2^-8 below 8 in size: up to 16 of them add up exactly in fp32 (15 bits), in any order, so fp32 and
    fp64 sums agree BEFORE the rounding to T.  (With arbitrary slabs the two sums round to different T neighbours once
    in ~2^12 elements, and where the residual then cancels most of the sum, or silu sits on its steep negative side,
    that one ulp of the sum is many ulps of the output: an artefact of the comparison, not of the reference.)"""
    return (torch.randn(shape, generator=_gen(seed)) * 256).round().clamp(-2047, 2047) / 256


def test_slab_sum_is_in_split_order():
    # (2^24 + 1) - 2^24: 0 in split order, 1 in any order that adds the two large slabs first
    p = torch.tensor([[2.0 ** 24], [1.0], [-2.0 ** 24]])
    assert R.sum_slabs(p).item() == 0.0
    assert R.sum_slabs(p[[0, 2, 1]]).item() == 1.0
    for dt in DTYPES16:
        h, _ = R.add_rms_norm_slabs(p.view(3, 1, 1), torch.zeros((1, 1), dtype=dt), torch.ones(1, dtype=dt), 1e-5)
        assert h.item() == 0.0
        big = torch.cat([p, p], dim=1).view(3, 1, 2)                     # gate | up
        assert R.silu_and_mul_slabs(big, 1, dt).item() == 0.0
        assert R.silu_and_mul_slabs(big[[0, 2, 1]], 1, dt).item() != 0.0


@pytest.mark.parametrize("dt", DTYPES16)
@pytest.mark.parametrize("n_splits", [1, 6, 7, 13])
def test_add_rms_norm_slabs_reference_against_fp64(dt, n_splits):
    rows, hidden, eps = 5, 1024, 1e-5
    p = _dyadic_slabs((n_splits, rows, hidden), n_splits)
    r = torch.randn((rows, hidden), generator=_gen(7)).to(dt)
    w = (1 + 0.1 * torch.randn(hidden, generator=_gen(8))).to(dt)
    h, out = R.add_rms_norm_slabs(p, r, w, eps)
    a64 = p.double().sum(0).to(dt)
    h64 = (a64.double() + r.double()).to(dt)
    # rounding points on the way to h: the sum -> T, the add -> T = 2
    assert_ulp_close(h, h64, max_ulp=2, what="residual")
    x = h64.double()
    s = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps)
    out64 = ((x * s).to(dt).double() * w.double()).to(dt)
    # rounding points on the way to out: those 2, (T)(h * s), (T)(n * w) = 4
    assert_ulp_close(out, out64, max_ulp=4, what="normalised")
    assert not torch.isnan(out.float()).any()


@pytest.mark.parametrize("dt", DTYPES16)
@pytest.mark.parametrize("n_splits", [1, 6, 7, 13])
def test_silu_and_mul_slabs_reference_against_fp64(dt, n_splits):
    rows, inter = 5, 96 * 8
    p = _dyadic_slabs((n_splits, rows, 2 * inter), 20 + n_splits)
    out = R.silu_and_mul_slabs(p, inter, dt)
    gu = p.double().sum(0).to(dt)
    g, u = gu[:, :inter].double(), gu[:, inter:].double()
    s64 = (g / (1.0 + torch.exp(-g))).to(dt)
    out64 = (s64.double() * u).to(dt)
    # rounding points on the way to out: gate sum -> T, up sum -> T, silu -> T, product -> T = 4
    assert_ulp_close(out, out64, max_ulp=4, what="silu_and_mul_slabs")


@pytest.mark.parametrize("dt", DTYPES16 + [torch.float32])
def test_rope_set_kv_cache_reference_against_fp64(dt):
    H, HK, D, rot, n, bs, nb = 4, 2, 32, 16, 9, 4, 5
    g = _gen(3)
    q = torch.randn((n, H, D), generator=g).to(dt)
    k = torch.randn((n, HK, D), generator=g).to(dt)
    v = torch.randn((n, HK, D), generator=g).to(dt)
    pos = torch.randint(0, 64, (n,), generator=g).to(torch.int32)
    cs = ops.build_cos_sin_cache(rot, 64, 1e4, dt)
    slots = torch.randperm(nb * bs, generator=g)[:n].to(torch.int32)
    slots[1] = slots[6] = -1
    kc0 = torch.randn((nb, bs, HK, D), generator=g).to(dt)
    vc0 = torch.randn((nb, bs, HK, D), generator=g).to(dt)
    kc, vc = kc0.clone(), vc0.clone()
    q_in, k_in, v_in = q.clone(), k.clone(), v.clone()
    q_ref, k_ref = R.rope_set_kv_cache(q, k, v, pos, cs, rot, slots, kc, vc)
    assert R.same_bits(q, q_in) and R.same_bits(k, k_in) and R.same_bits(v, v_in)      # inputs are not modified

    half = rot // 2
    c = cs.view(-1, 2, half)[pos.long()][:, 0, None, :].double()
    s = cs.view(-1, 2, half)[pos.long()][:, 1, None, :].double()

    def rot64(t):
        x, y = t[..., :half].double(), t[..., half:rot].double()
        r = lambda z: z.to(dt).double()
        out = t.clone()
        out[..., :half] = (r(x * c) - r(y * s)).to(dt)
        out[..., half:rot] = (r(x * s) + r(y * c)).to(dt)
        return out

    # rounding points on the way to an element: two products -> T, their sum or difference -> T = 3
    assert_ulp_close(q_ref, rot64(q), max_ulp=3, what="q")
    assert_ulp_close(k_ref, rot64(k), max_ulp=3, what="k")
    assert R.same_bits(q_ref[..., rot:], q[..., rot:]) and R.same_bits(k_ref[..., rot:], k[..., rot:])
    # the scatter has no rounding point: bit for bit, tokens with a negative slot write nothing
    kc_want, vc_want = kc0.clone(), vc0.clone()
    for i in range(n):
        sl = int(slots[i])
        if sl >= 0:
            kc_want[sl // bs, sl % bs] = k_ref[i]
            vc_want[sl // bs, sl % bs] = v[i]
    assert R.same_bits(kc, kc_want) and R.same_bits(vc, vc_want)
    assert not R.same_bits(kc, kc0)


@pytest.mark.parametrize("dt", DTYPES16)
def test_quick_gelu_reference_against_fp64(dt):
    x = (3 * torch.randn((64, 512), generator=_gen(4))).to(dt)
    out = R.quick_gelu(x)
    k = torch.tensor(1.702, dtype=torch.float32).double()
    t = (x.double() * k).float().to(dt)                      # the product is rounded to fp32 first, as the formula says
    s = (1.0 / (1.0 + torch.exp(-t.double()))).to(dt)
    out64 = (x.double() * s.double()).float().to(dt)
    # rounding points: (T)(1.702 x), (T)sigmoid, (T)(x * s) = 3
    assert_ulp_close(out, out64, max_ulp=3, what="quick_gelu")


@pytest.mark.parametrize("dt", DTYPES16)
def test_references_give_no_nan_on_the_exhaustive_grid(dt):
    x = R.all_finite_16bit(dt)
    u = R.up_cycle(dt, x.shape)
    for name, y in (("silu_kernel", ops.silu_kernel(x)), ("quick_gelu", R.quick_gelu(x)),
                    ("silu_kernel * up", (ops.silu_kernel(x).float() * u.float()).to(dt)),
                    ("silu_and_mul", ops.silu_and_mul(x, u))):
        assert not torch.isnan(y.float()).any(), name
    # a [1, rows, 2n] slab set of the same values goes through the slab reference NaN-free too
    p = torch.cat([x.float(), u.float()], dim=1).unsqueeze(0)
    assert not torch.isnan(R.silu_and_mul_slabs(p, 8192, dt).float()).any()


def test_elements_left_out_on_the_gpu_are_the_doubled_ulp_and_nothing_else():
    """R.DOUBLED_ULP: every recorded element is a `first` one ulp of fp16 from the reference's, whose exact product with
    `second`, rounded once, is the recorded output on either side, two ulp apart — arithmetic that needs no GPU.  The
    count stays at seven: at most 3 of the 47872 elements of a case (0.006 %)."""
    from tests.util import _ordered_bits
    dt = torch.float16
    t = lambda v: torch.tensor([v], dtype=torch.float64).to(dt)
    dist = lambda a, b: int((_ordered_bits(t(a)) - _ordered_bits(t(b))).abs())
    assert sum(len(v) for v in R.DOUBLED_ULP.values()) == 7 and max(len(v) for v in R.DOUBLED_ULP.values()) == 3
    for case, items in R.DOUBLED_ULP.items():
        for idx, out, ref, first, first_ref, second in items:
            for v in (out, ref, first, first_ref, second):
                assert float(t(v)) == v, (case, idx)                      # all are fp16 values
            assert dist(first, first_ref) == 1 and dist(out, ref) == 2, (case, idx)
            assert float(t(first * second)) == out and float(t(first_ref * second)) == ref, (case, idx)
    # the silu side of it: the gate is -2.724609375, whose silu (-0.167663569 in fp64) lies 5e-9, a third of an fp32 ulp,
    # short of the midpoint of the two fp16 neighbours; the reference's fp32 value rounds to the nearer one, as the exact
    # value does (compared in fp64: a conversion fp64 -> fp32 -> fp16 would round twice, onto the midpoint and then away)
    g = torch.tensor([-2.724609375], dtype=dt)
    assert float(ops.silu_kernel(g)) == -0.1676025390625
    exact = float(g.double() / (1.0 + torch.exp(-g.double())))
    assert 0.1676025390625 < -exact < (0.1676025390625 + 0.167724609375) / 2
