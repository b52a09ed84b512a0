"""CPU: the inputs of tests/gemm_exact.py are what they claim BEFORE a GPU sees them — the exactness bound holds for
every shape tests/test_gpu_gemm_instantiations.py can pick, fp32 sums of the products are the float64 product bit for
bit in any order, and the one-hot probe list reaches every boundary of the kernels' k decomposition for every built
k-steps-per-wave count."""
import os

import pytest
import torch

from hydrainfer_amd import _lib
from tests import gemm_exact as E


def test_exactness_bound_holds_for_every_shape_the_gpu_tests_use():
    worst = 0.0
    for K in sorted(set(E.K_VALUES) | {k for _, k in E.LDS_SHAPES}):
        for step_x, step_w in ((E.STEP, E.STEP), (E.STEP, 2.0 ** -8)):      # (the silu epilogue tests draw w finer)
            b = E.assert_exact(K, E.LEVELS * step_x, E.LEVELS * step_w, step_x * step_w)
            assert b == K * E.LEVELS ** 2
            worst = max(worst, b)
    assert worst == 13824 * 225 == 3110400 < 2 ** 24
    with pytest.raises(AssertionError):      # the check is a condition: it refuses what would round
        E.assert_exact(13824, 31 * 0.25, 63 * 0.25, 1 / 16)
    with pytest.raises(AssertionError):
        E.assert_exact(2 ** 24, 0.25, 0.25, 1 / 16)
    # the values are exact in both 16-bit formats, and problem() carries the bound of what it drew
    for step in (E.STEP, 2.0 ** -8):
        v = torch.arange(-E.LEVELS, E.LEVELS + 1, dtype=torch.float32) * step
        assert torch.equal(v.to(torch.float16).float(), v) and torch.equal(v.to(torch.bfloat16).float(), v)
    p = E.problem(5, 48, 13824)
    assert p.bound <= 13824 * 225 and p.quantum == 1 / 16
    assert set((p.w / E.STEP).flatten().tolist()) == set(range(-E.LEVELS, E.LEVELS + 1))


@pytest.mark.parametrize("K", [256, 4128, 13824])
def test_fp32_sums_in_any_order_equal_the_float64_reference(K):
    """The same products summed in fp32 — forwards, shuffled, in blocks of a k-step whose partial sums are then added
    (the kernels' shape: waves, splits, a rotated start), as one fp32 matmul — give ref.float() exactly, and ref is
    exact in fp32."""
    p = E.problem(7, 48, K, seed=3)
    assert torch.equal(p.ref.float().double(), p.ref)
    prod = p.x[:, None, :] * p.w[None, :, :]                       # fp32 [M, N, K]: every product exact
    assert torch.equal(prod.double(), p.x.double()[:, None, :] * p.w.double()[None, :, :])
    want = p.ref.float()
    g = torch.Generator().manual_seed(K)

    def chain(t):      # strictly sequential fp32 adds along the last axis
        acc = torch.zeros(t.shape[:-1], dtype=torch.float32)
        for i in range(t.shape[-1]):
            acc = acc + t[..., i]
        return acc

    assert torch.equal(prod.sum(-1), want)
    assert torch.equal(p.x @ p.w.t(), want)
    assert torch.equal(chain(prod[..., :: max(1, K // 512)]).double(),
                       prod[..., :: max(1, K // 512)].double().sum(-1))      # a sequential chain over a sample of k
    for _ in range(3):
        perm = torch.randperm(K, generator=g)
        assert torch.equal(prod[..., perm].sum(-1), want)
    for block in (32, 32 * 29, 1024):
        parts = [prod[..., a:a + block].sum(-1) for a in range(0, K, block)]
        order = torch.randperm(len(parts), generator=g).tolist()
        assert torch.equal(chain(torch.stack([parts[i] for i in order], -1)), want)
        r = len(parts) // 3                                         # a rotated start, as xreg_stagger makes it
        assert torch.equal(chain(torch.stack(parts[r:] + parts[:r], -1)), want)


def _built_tables():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhydra_hip.so is not built: the tables of built instantiations cannot be read")
    from hydrainfer_amd._C.kernel import gemm
    return gemm.xreg_built(False), gemm.xreg_built(True)


def test_built_tables_are_readable_and_end():
    narrow, wide = _built_tables()
    assert len(narrow) >= 9 and len(wide) >= 8
    for table in (narrow, wide):
        kws = [kw for kw, _, _ in table]
        assert kws == sorted(set(kws)) and kws[0] >= 1           # round_kw walks the table upwards
        assert all(norm or not silu for _, norm, silu in table)   # (a silu row of the table is a norm row)
    out = (_lib.ctypes.c_int32 * 3)()
    assert _lib.lib().hx_debug_xreg_built(0, len(narrow), out) == -2 and _lib.lib().hx_debug_xreg_built(1, -1, out) == -2
    assert _lib.lib().hx_debug_xreg_built(0, 0, None) == -4


def test_probe_list_covers_every_boundary_for_every_built_kw():
    """Brute force, stated per k instead of per range: k belongs to (packing split, half, wave) by plain division; wherever
    that owner changes between k - 1 and k both sides must be probes, and so must 0, 31, 32, K - 32 and K - 1."""
    narrow, wide = _built_tables()
    n_cases = 0
    for is_wide, table in ((False, narrow), (True, wide)):
        for kw, _, _ in table:
            # the packing's k-steps per split: the narrow kernel's own 4 * kw; the wide kernel reads a packing of twice
            # its k-steps per wave, or one less where that count is built for the narrow kernel (27 -> 14 + 13)
            pk_Ps = [4 * kw] if not is_wide else [4 * p for p in (2 * kw, 2 * kw - 1) if p in [r[0] for r in narrow]]
            assert pk_Ps, (is_wide, kw)
            for pk_P in pk_Ps:
                # one full split; a partial one; three splits with a partial last one; a last wave with one k-step
                for total in (pk_P, pk_P - 3, 2 * pk_P + pk_P // 2 + 1, pk_P + 3 * kw + 1 if not is_wide else pk_P + kw + 1):
                    if total < 2:
                        continue
                    K = 32 * total
                    ks = set(E.probe_ks(K, kw, is_wide, pk_P))

                    def owner(k):
                        q, r = divmod(k // 32, pk_P)
                        half, r = divmod(r, 4 * kw)
                        return (q, half, r // kw)

                    want = {0, 31, 32, K - 32, K - 1}
                    for k in range(1, K):
                        if owner(k) != owner(k - 1):
                            want |= {k - 1, k}
                    want = {k for k in want if 0 <= k < K}
                    assert want <= ks, (is_wide, kw, pk_P, K, sorted(want - ks))
                    assert len(ks) <= len(want) + 2
                    # the ranges tile 0 .. K / 32 without gap or overlap, and no wave holds more than kw k-steps
                    covered = sorted((a, n) for _, _, a, n in E.wave_ranges(K, kw, is_wide, pk_P))
                    assert covered[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(covered, covered[1:]))
                    assert sum(n for _, n in covered) == total and max(n for _, n in covered) <= kw
                    n_cases += 1
    assert n_cases >= 4 * 17
    x = E.one_hot_rows([0, 31, 95], 96)
    assert x.sum().item() == 3 and x[1, 31] == 1 and x[2, 95] == 1


def test_poison_guard_and_strided_helpers():
    buf = E.poisoned(10, "cpu")
    with pytest.raises(AssertionError):
        E.checked(buf, 10)                      # nothing written yet
    buf[:10] = 1.0
    assert E.checked(buf, 10).numel() == 10
    buf[10] = 0.0
    with pytest.raises(AssertionError):
        E.checked(buf, 10)                      # guard hit
    t = torch.arange(12.0).view(3, 4)
    v = E.strided(t, 8, -1.0)
    assert torch.equal(v, t) and v.stride() == (12, 1) and E.gaps_hold(v, 8, -1.0)
    torch.as_strided(v, (3, 12), (12, 1))[1, 5] = 0.0
    assert not E.gaps_hold(v, 8, -1.0)
    assert not torch.isnan(E.strided(t, 8)).any() and torch.isnan(torch.as_strided(E.strided(t, 8), (3, 12), (12, 1))[:, 4:]).all()
