"""GPU: ALiBi slopes in mha_varlen_fwd — the per-head decode kernel in its three launch forms, the grouped-query decode
kernel, the general kernel, the layer — against the fp32 restatement in tests/alibi_ref.py and a closed form."""
import ctypes
import math

import pytest
import torch

from tests import alibi_ref as R
from tests.util import ATTN_TOL, assert_close_t

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _slopes(H):
    from hydrainfer_amd.layer.alibi import alibi_slopes
    return alibi_slopes(H)


def _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, max_q, max_k, causal=True, num_splits=0, softcap=0.0, window=None):
    from hydrainfer_amd._C.kernel.flash_attn import mha_varlen_fwd
    qd = q.to(DEV)
    out = torch.empty_like(qd)
    wl, wr = window if window is not None else (-1, 0 if causal else -1)
    mha_varlen_fwd(out, qd, kc.to(DEV), vc.to(DEV), cu_q.to(DEV), cu_k.to(DEV), bt.to(DEV) if bt is not None else None,
                   cu_b.to(DEV) if cu_b is not None else None, slopes.to(DEV) if slopes is not None else None, max_q, max_k,
                   1.0 / math.sqrt(q.shape[-1]), softcap, wl, wr, num_splits)
    torch.cuda.synchronize()
    return out


def _first_case(dt):
    c = R.FIRST_CASE
    kv = R.ragged_lens(c["batch"], c["lo"], c["hi"], c["seed"])
    return kv, R.random_paged(c["batch"], c["H"], c["HK"], c["D"], kv, [1] * c["batch"], dt, seed=c["seed"])


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_paged_decode_with_standard_slopes(dt):
    """B = 8, H = HK = 32, D = 128, kv_lens ragged in 1..1000 (256 pairs: the 8-wave launch).  Without the feature the call
    raises.  It also cannot pass by ignoring the slopes: the output lies more than 10 x the tolerance from the
    alibi_slopes=None output (tests/test_alibi_cpu.py shows that gap on the restatement alone)."""
    kv, (q, kc, vc, cu_q, cu_k, bt, cu_b) = _first_case(dt)
    slopes = _slopes(32)
    ref = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes)
    out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, 1, max(kv))
    atol, rtol = ATTN_TOL[dt]
    print(f"alibi decode {dt}: max abs err {(out.cpu().float() - ref).abs().max().item():.3e}")
    assert_close_t(out, ref, atol, rtol, what=f"alibi decode {dt}")
    plain = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, None, 1, max(kv))
    gap = (out.float() - plain.float()).abs().cpu() - 10 * (atol + rtol * ref.abs())
    assert gap.max().item() > 0, "the slopes changed nothing"


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("num_splits", [1, 4, 0])
def test_decode_split_forms(dt, num_splits):
    kv, (q, kc, vc, cu_q, cu_k, bt, cu_b) = _first_case(dt)
    slopes = _slopes(32)
    ref = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes)
    out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, 1, max(kv), num_splits=num_splits)
    assert_close_t(out, ref, *ATTN_TOL[dt], what=f"alibi decode splits={num_splits} {dt}")


# (batch, H, hi): 2 x 32 = 64 pairs, one split -> the 4-wave launch; 24 x 32 = 768 pairs -> the 4-wave launch of big
# batches; 8 x 32 = 256 -> the 8-wave launch; 2 x 8 = 16 pairs at up to 1000 keys -> the automatic key split (3 splits)
@pytest.mark.parametrize("form", [(2, 32, 1000, 1), (24, 32, 300, 0), (8, 32, 600, 0), (2, 8, 1000, 0)])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_decode_launch_forms(dt, form):
    batch, H, hi, splits = form
    kv = R.ragged_lens(batch, 1, hi, seed=batch + H)
    kv[0] = hi                                              # the longest sequence decides the split count
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(batch, H, H, 128, kv, [1] * batch, dt, seed=batch)
    slopes = _slopes(H)
    ref = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes)
    out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, 1, max(kv), num_splits=splits)
    assert_close_t(out, ref, *ATTN_TOL[dt], what=f"alibi decode form {form} {dt}")


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("heads", [(8, 8), (32, 8), (32, 4)])          # per-head kernel; grouped-query groups 4 and 8
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_decode_head_dims_and_gqa_groups(dt, heads, D):
    H, HK = heads
    batch = 5
    kv = [1, 17, 333, 1000, 64]
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(batch, H, HK, D, kv, [1] * batch, dt, seed=D + H + HK)
    slopes = _slopes(H)
    ref = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes)
    for splits in (0, 1, 4):
        out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, 1, max(kv), num_splits=splits)
        assert_close_t(out, ref, *ATTN_TOL[dt], what=f"alibi decode D={D} {heads} splits={splits} {dt}")


@pytest.mark.parametrize("heads", [(16, 16), (16, 4)])
@pytest.mark.parametrize("block_size", [16, 48])
def test_per_sequence_slopes_and_page_sizes(heads, block_size):
    """slopes [batch, n_heads] with distinct rows; page size 48 is not a power of two."""
    H, HK = heads
    dt = torch.float16
    batch = 6
    kv = R.ragged_lens(batch, 1, 700, seed=block_size)
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(batch, H, HK, 128, kv, [1] * batch, dt, block_size=block_size,
                                                     seed=block_size + H)
    slopes = _slopes(H)[None, :] * (1.0 + 0.5 * torch.arange(batch, dtype=torch.float32))[:, None]
    assert slopes.shape == (batch, H)
    ref = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes)
    # a wrong row (every sequence taking sequence 0's slopes) would be visible
    wrong = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes[0])
    assert ((ref - wrong).abs() - 10 * (1e-3 + 1e-3 * ref.abs())).max().item() > 0
    for splits in (0, 1, 3):
        out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, 1, max(kv), num_splits=splits)
        assert_close_t(out, ref, *ATTN_TOL[dt], what=f"per-sequence slopes bs={block_size} {heads} splits={splits}")
    # a strided [batch, H] view (row stride 2 H) goes through alibi_batch_stride
    wide = torch.zeros((batch, 2 * H), dtype=torch.float32)
    wide[:, :H] = slopes
    out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, wide.to(DEV)[:, :H], 1, max(kv))
    assert_close_t(out, ref, *ATTN_TOL[dt], what="strided per-sequence slopes")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_general_kernel_paged_mixed_prefill_and_decode(dt):
    q_lens, kv_lens = [1, 50, 128, 3, 1, 200], [300, 50, 200, 67, 1, 200]
    for H, HK, D in ((8, 2, 128), (4, 4, 64)):
        q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(6, H, HK, D, kv_lens, q_lens, dt, seed=D)
        slopes = _slopes(H)
        ref = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes)
        out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, max(q_lens), max(kv_lens))
        assert_close_t(out, ref, *ATTN_TOL[dt], what=f"alibi mixed paged H={H} D={D} {dt}")


def _dense(batch, H, HK, D, q_lens, kv_lens, dt, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn((sum(q_lens), H, D), generator=g).to(dt)
    k = torch.randn((sum(kv_lens), HK, D), generator=g).to(dt)
    v = torch.randn((sum(kv_lens), HK, D), generator=g).to(dt)
    cu = lambda ls: torch.tensor([0] + torch.tensor(ls).cumsum(0).tolist(), dtype=torch.int32)
    return q, k, v, cu(q_lens), cu(kv_lens)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_general_kernel_dense_noncausal_is_two_sided(dt):
    q_lens, kv_lens = [70, 33, 130], [70, 90, 130]
    q, k, v, cu_q, cu_k = _dense(3, 8, 8, 64, q_lens, kv_lens, dt, seed=2)
    slopes = _slopes(8)
    ref = R.dense_attention_alibi(q, k, v, cu_q, cu_k, slopes, causal=False)
    out = _run(q, k, v, cu_q, cu_k, None, None, slopes, max(q_lens), max(kv_lens), causal=False)
    assert_close_t(out, ref, *ATTN_TOL[dt], what=f"alibi dense non-causal {dt}")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_general_kernel_with_window_and_with_softcap(dt):
    q_lens, kv_lens = [1, 100, 128, 1], [300, 100, 200, 65]
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(4, 8, 4, 128, kv_lens, q_lens, dt, seed=4)
    slopes = _slopes(8)
    ref = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, causal=False, window=(64, 0))
    out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, max(q_lens), max(kv_lens), causal=False, window=(64, 0))
    assert_close_t(out, ref, *ATTN_TOL[dt], what=f"alibi + window (64, 0) {dt}")
    # softcap 30 on scores scaled up to reach the cap (q x 8): the bias is added after the cap, not inside the tanh
    q8 = (q.float() * 8).to(dt)
    ref = R.paged_attention_alibi(q8, kc, vc, cu_q, cu_k, bt, cu_b, slopes, causal=True, softcap=30.0)
    out = _run(q8, kc, vc, cu_q, cu_k, bt, cu_b, slopes, max(q_lens), max(kv_lens), causal=True, softcap=30.0)
    assert_close_t(out, ref, *ATTN_TOL[dt], what=f"alibi + softcap 30 {dt}")
    # all-decode with a softcap also goes to the general kernel
    kv = [500, 31, 64]
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(3, 8, 8, 128, kv, [1, 1, 1], dt, seed=6)
    ref = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, softcap=30.0)
    out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, 1, max(kv), softcap=30.0)
    assert_close_t(out, ref, *ATTN_TOL[dt], what=f"alibi decode + softcap {dt}")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_closed_form_q_zero_through_the_decode_kernel(dt):
    """q = 0: every dot product vanishes and head h's output is sum_j w_j v_j, w_j ~ exp(-slope_h (lk - 1 - j)) — worked
    out in float64 from the cache's values, independent of the restatement.  lk = 832."""
    H, D, lk = 8, 128, 832
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(2, H, H, D, [lk, lk], [1, 1], dt, seed=8)
    q = torch.zeros_like(q)
    slopes = _slopes(H)
    atol, rtol = ATTN_TOL[dt]
    for splits in (1, 0, 4):
        out = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes, 1, lk, num_splits=splits).cpu()
        for b in range(2):
            pages = bt[int(cu_b[b]): int(cu_b[b + 1])].long()
            v = vc[pages].reshape(-1, H, D)[:lk]
            want = R.closed_form_q0(v, slopes)
            assert_close_t(out[b], want.float(), atol, rtol, what=f"closed form b={b} splits={splits} {dt}")
            assert (want - v.double().mean(dim=0)).abs().max().item() > 0.1


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_zero_slopes_equal_the_call_without_slopes(dt):
    """Adding 0 * distance is exact, so the per-head decode kernel gives the same bits as the kernel without ALiBi, in each
    launch form; the grouped-query and the general kernel likewise."""
    kv, (q, kc, vc, cu_q, cu_k, bt, cu_b) = _first_case(dt)
    zero = torch.zeros(32, dtype=torch.float32)
    for splits in (0, 1, 4):
        a = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, zero, 1, max(kv), num_splits=splits)
        b = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, None, 1, max(kv), num_splits=splits)
        assert torch.equal(a, b), f"per-head decode, splits={splits}: max diff {(a.float() - b.float()).abs().max().item()}"
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(4, 32, 8, 128, [700, 3, 90, 256], [1] * 4, dt, seed=1)
    a = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, zero, 1, 700)
    b = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, None, 1, 700)
    assert torch.equal(a, b), "grouped-query decode"
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(2, 32, 32, 128, [100, 60], [40, 60], dt, seed=2)
    a = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, zero, 60, 100)
    b = _run(q, kc, vc, cu_q, cu_k, bt, cu_b, None, 60, 100)
    assert_close_t(a, b.cpu().float(), *ATTN_TOL[dt], what="general kernel, zero slopes")


def test_error_paths():
    from hydrainfer_amd import _lib
    dt = torch.float16
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(2, 8, 8, 128, [40, 17], [1, 1], dt, seed=0)
    good = _slopes(8)
    _run(q, kc, vc, cu_q, cu_k, bt, cu_b, good, 1, 40)
    for bad in (good.half().to(DEV), torch.ones(9, device=DEV), torch.ones((3, 8), device=DEV), torch.ones((2, 8, 1), device=DEV),
                torch.ones((8, 2), device=DEV)[:, 0], good):                  # dtype, shapes, stride, CPU tensor
        with pytest.raises(_lib.HydraHipError):
            from hydrainfer_amd._C.kernel.flash_attn import mha_varlen_fwd
            qd = q.to(DEV)
            mha_varlen_fwd(torch.empty_like(qd), qd, kc.to(DEV), vc.to(DEV), cu_q.to(DEV), cu_k.to(DEV), bt.to(DEV), cu_b.to(DEV),
                           bad, 1, 40, 1.0 / math.sqrt(128), 0.0, -1, 0, 0)


def test_c_abi_flag_checks_and_fused_entry():
    """At the C ABI: the flag with a null / misaligned pointer or a negative stride is refused, and
    hx_decode_attention_fused answers the flag with HX_ERR_UNSUPPORTED (it fuses RoPE; ALiBi models have none)."""
    from hydrainfer_amd import _lib
    dt = torch.float16
    B, H, D = 2, 8, 128
    q, kc, vc, cu_q, cu_k, bt, cu_b = R.random_paged(B, H, H, D, [40, 17], [1, 1], dt, seed=0)
    t = [x.to(DEV) for x in (q, kc, vc, cu_q, cu_k, bt, cu_b)]
    qd, kcd, vcd, cu_qd, cu_kd, btd, cu_bd = t
    out = torch.empty_like(qd)
    slopes = _slopes(H).to(DEV)
    a = _lib.hx_attn_args()
    a.out, a.q, a.k, a.v = out.data_ptr(), qd.data_ptr(), kcd.data_ptr(), vcd.data_ptr()
    a.cu_seqlens_q, a.cu_seqlens_k = cu_qd.data_ptr(), cu_kd.data_ptr()
    a.block_table, a.cu_block_lens = btd.data_ptr(), cu_bd.data_ptr()
    a.batch, a.n_heads, a.n_kv_heads, a.head_dim = B, H, H, D
    a.block_size, a.max_seqlen_q, a.max_seqlen_k, a.total_q = 16, 1, 40, B
    a.q_row_stride, a.o_row_stride = qd.stride(0), out.stride(0)
    a.k_block_stride, a.k_row_stride, a.k_head_stride = kcd.stride(0), kcd.stride(1), kcd.stride(2)
    a.v_block_stride, a.v_row_stride, a.v_head_stride = vcd.stride(0), vcd.stride(1), vcd.stride(2)
    a.softmax_scale, a.causal, a.dtype, a.num_splits = 1.0 / math.sqrt(D), 1, _lib.dtype_code(qd), 1
    a.softcap, a.window_left, a.window_right = 0.0, -1, -1
    l = _lib.lib()
    stream = _lib.current_stream()
    HX_ERR_SHAPE, HX_ERR_STRIDE, HX_ERR_NULL, HX_ERR_UNSUPPORTED = -2, -3, -4, -5
    a.flags = _lib.HX_ATTN_ALIBI
    assert l.hx_mha_varlen_fwd(ctypes.byref(a), stream) == HX_ERR_NULL
    a.alibi_slopes = slopes.data_ptr() + 2
    assert l.hx_mha_varlen_fwd(ctypes.byref(a), stream) == HX_ERR_STRIDE
    a.alibi_slopes, a.alibi_batch_stride = slopes.data_ptr(), -1
    assert l.hx_mha_varlen_fwd(ctypes.byref(a), stream) == HX_ERR_SHAPE
    a.alibi_batch_stride = 0
    assert l.hx_mha_varlen_fwd(ctypes.byref(a), stream) == 0
    a.flags = _lib.HX_ATTN_ALIBI | 4
    assert l.hx_mha_varlen_fwd(ctypes.byref(a), stream) == HX_ERR_UNSUPPORTED      # unknown bits are still refused
    torch.cuda.synchronize()
    ref = R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, slopes.cpu())
    assert_close_t(out, ref, *ATTN_TOL[dt], what="C ABI call")
    # without the flag the tail is ignored, whatever it holds
    a.flags, a.alibi_slopes, a.alibi_batch_stride = 0, 12345, -7
    assert l.hx_mha_varlen_fwd(ctypes.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert_close_t(out, R.paged_attention_alibi(q, kc, vc, cu_q, cu_k, bt, cu_b, None), *ATTN_TOL[dt], what="flag off")

    # the fused entry: valid arguments, flag off -> ok; flag on -> HX_ERR_UNSUPPORTED
    from oracle import ops
    cs = ops.build_cos_sin_cache(D, 64, 10000.0, dt).to(DEV)
    k_new, v_new = torch.randn((B, H, D), device=DEV, dtype=dt), torch.randn((B, H, D), device=DEV, dtype=dt)
    pos = torch.tensor([39, 16], dtype=torch.int32, device=DEV)
    slots = torch.tensor([int(bt[int(cu_b[b])  + (l_ - 1) // 16]) * 16 + (l_ - 1) % 16 for b, l_ in enumerate([40, 17])],
                         dtype=torch.int32, device=DEV)
    f = _lib.hx_fused_decode_args()
    f.k_new, f.v_new = k_new.data_ptr(), v_new.data_ptr()
    f.k_new_row_stride, f.v_new_row_stride = k_new.stride(0), v_new.stride(0)
    f.positions, f.cos_sin, f.new_cache_slots = pos.data_ptr(), cs.data_ptr(), slots.data_ptr()
    f.rotary_dim, f.interleaved, f.qkv_partial, f.qkv_splits, f.rank_desc = D, 0, None, 0, None
    a.flags, a.alibi_slopes, a.alibi_batch_stride = 0, None, 0
    assert l.hx_decode_attention_fused(ctypes.byref(a), ctypes.byref(f), stream) == 0
    a.flags, a.alibi_slopes = _lib.HX_ATTN_ALIBI, slopes.data_ptr()
    assert l.hx_decode_attention_fused(ctypes.byref(a), ctypes.byref(f), stream) == HX_ERR_UNSUPPORTED
    torch.cuda.synchronize()


@pytest.mark.parametrize("heads", [(8, 8), (8, 2)])
def test_layer_prefill_chunk_then_three_decode_steps(heads):
    """CausalGroupedQueryPageAttention with alibi_slopes in its config, through a real KVCache: a prefill chunk for two
    sequences, then three decode steps; outputs against the restatement over the cache the layer itself filled."""
    from hydrainfer_amd.layer.causal_attention import (AttentionParametersBuilder, CausalGroupedQueryPageAttention,
                                                       CausalGroupedQueryPageAttentionConfig)
    from hydrainfer_amd.memory.kv_cache import KVCache
    H, HK = heads
    D, bs, n_blocks, dt = 128, 16, 32, torch.float16
    g = torch.Generator().manual_seed(H + HK)
    slopes = _slopes(H)
    kcd = torch.zeros((n_blocks, bs, HK, D), dtype=dt, device=DEV)
    vcd = torch.zeros_like(kcd)
    cache = KVCache(kcd, vcd)
    attn = CausalGroupedQueryPageAttention(CausalGroupedQueryPageAttentionConfig(H, HK, D, alibi_slopes=slopes.to(DEV)))
    perm = torch.randperm(n_blocks, generator=g).tolist()
    tables = [perm[:8], perm[8:16]]
    lens = [0, 0]
    ks = [torch.zeros((0, HK, D)), torch.zeros((0, HK, D))]
    vs = [torch.zeros((0, HK, D)), torch.zeros((0, HK, D))]
    atol, rtol = ATTN_TOL[dt]
    for step, q_lens in enumerate([[37, 70], [1, 1], [1, 1], [1, 1]]):
        builder = AttentionParametersBuilder(H, HK, D, bs, torch.device(DEV))
        n = sum(q_lens)
        q = torch.randn((n, H * D), generator=g).to(dt)
        k = torch.randn((n, HK * D), generator=g).to(dt)
        v = torch.randn((n, HK * D), generator=g).to(dt)
        off = 0
        for b, ql in enumerate(q_lens):
            slots = [tables[b][t // bs] * bs + t % bs for t in range(lens[b], lens[b] + ql)]
            lens[b] += ql
            builder.add_request(ql, lens[b], slots, tables[b][: (lens[b] + bs - 1) // bs])
            ks[b] = torch.cat([ks[b], k[off: off + ql].view(ql, HK, D).float()])
            vs[b] = torch.cat([vs[b], v[off: off + ql].view(ql, HK, D).float()])
            off += ql
        builder.add_kv_cache(cache)
        params = builder.build_attention_parameters()[0]
        o = attn(q.to(DEV), k.to(DEV), v.to(DEV), params).o
        torch.cuda.synchronize()
        off = 0
        for b, ql in enumerate(q_lens):
            ref = R.attend_alibi(q[off: off + ql].view(ql, H, D), ks[b], vs[b], 1.0 / math.sqrt(D), True, slopes)
            assert_close_t(o[off: off + ql].view(ql, H, D), ref, atol, rtol, what=f"layer step {step} seq {b} {heads}")
            off += ql
