"""GPU: every kernel instantiation and host branch of hydrainfer_amd/csrc/moe.hip on inputs that pair each expert row
with its own weight (tests/moe_cases.py; each case is proven sound and sensitive on the oracle by
tests/test_moe_cases_cpu.py).

1. unpermute on distinct rows, index and mask maps: two-byte types bit for bit against oracle.moe.unpermute_rows on the
   16-byte streaming form and, through a misaligned copy, on the scalar form; fp32 inside the float64 bound.
2. row maps at every rocPRIM sort algorithm and at the edges of the mask map's 256-token step.
3. permute: every element width, aligned and misaligned, rows wider than one pass of the workgroup.
4. sum_out at the topk values that mix the 4-row main loop with the tail, with and without row splits.
5. topk_softmax at every kPerLane on both sides of each edge, with ties, with -inf experts, topk == n_experts.
6. grouped_topk_sigmoid at the accepted shapes nothing launched so far.

Every test prints how many launches it checked.

What launches what (kernel instantiation or host branch of moe.hip -> test here):
  topk_softmax_kernel<1> / <2> / <4> / <8> / <16>   test_topk_softmax_every_lane_width[5, 60, 64] / [65, 128] / [129, 256] /
                                                    [257, 512] / [513, 1000, 1024]
  grouped_topk_sigmoid_kernel                       test_grouped_topk_sigmoid_accepted_shapes
  iota_kernel, row_id_map_from_sorted_kernel        test_index_row_map_at_every_sort_algorithm
  radix_sort_pairs: one block / merge / onesweep    ...[128-8] / [205-5], [4096-8], [131072-8] / [131073-8]
  mask_count_kernel, mask_assign_kernel             test_mask_row_map_on_uneven_masks
  permute_kernel<uint4>                             test_permute_every_element_width (fp32 4100, 4104; two-byte 4104; aligned)
  permute_kernel<uint16_t>                          ...[fp16], [bf16]: dim 7 and 4100, and every misaligned run
  permute_kernel<uint32_t>                          ...[fp32]: dim 7, and every misaligned run
  unpermute_vec_kernel<F16> / <BF16>                test_unpermute_pairs_every_row_with_its_own_weight[*-fp16] / [*-bf16], aligned,
                                                    dim 8 / 64 / 2056, n_rows <= 256; row splits and two chunks per thread:
                                                    test_unpermute_with_the_row_cut_over_several_workgroups, ..._two_chunks_per_thread
  unpermute_kernel<F16> / <BF16>                    the same cases misaligned, dim 36, and n_rows 257 / 320 (mask form)
  unpermute_kernel<F32>                             test_unpermute_pairs_every_row_with_its_own_weight[*-fp32]
  probs == NULL in the three unpermute kernels      test_unpermute_without_probabilities
  sum_out_vec_kernel<F16> / <BF16>                  test_sum_out_main_loop_and_tail[*-fp16] / [*-bf16] aligned, ..._two_chunks_per_thread
  sum_out_kernel<F32> / <F16> / <BF16>              test_sum_out_main_loop_and_tail[*-fp32] / the misaligned two-byte runs
  t_accum = 1 (topk 2, 3, 4, 8)                     tests/test_gpu_moe.py::test_sum_out (unchanged)
  error returns, n_tokens == 0                      test_host_refusals_and_empty_batches"""
import numpy as np
import pytest
import torch

from oracle import moe
from tests import moe_cases as M
from tests.rowwise_ref import misaligned
from tests.util import assert_ulp_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _unpermute_launches(case):
    from hydrainfer_amd._C.kernel.moe import unpermute_with_index_map, unpermute_with_mask_map
    b = M.unpermute(case)
    fn = unpermute_with_index_map if case.form == "index" else unpermute_with_mask_map
    x, row_map, probs = b.x.to(DEV), b.row_map.to(DEV), b.probs.to(DEV)
    M.check_unpermute(b, fn(x, row_map, probs), what=f"{case.name}, aligned")
    if case.dt == "fp32":
        return 1
    M.check_unpermute(b, fn(misaligned(x), row_map, probs), what=f"{case.name}, misaligned (the scalar form)")
    return 2


@pytest.mark.parametrize("dt", list(M.DTYPES))
@pytest.mark.parametrize("form", ["index", "mask"])
def test_unpermute_pairs_every_row_with_its_own_weight(form, dt):
    """1 to 9 valid rows (index) and 0 to 2 * topk (uneven masks, NaN at every unrouted probability), dim 8 / 64 / 2056
    (two passes of the chunk loop) / 36 (scalar form), 1 / 5 / 300 tokens, 256 experts (the last streaming size) and
    257 / 320 (the scalar fall-back for n_rows > 256).  Tokens routed nowhere come back as zeros."""
    cases = [c for c in M.UNPERMUTE_CASES if c.form == form and c.dt == dt]
    n = sum(_unpermute_launches(case) for case in cases)
    print(f"unpermute {form} {dt}: {n} launches checked")
    assert n == len(cases) * (1 if dt == "fp32" else 2) and len(cases) >= 27


def test_unpermute_with_the_row_cut_over_several_workgroups():
    """5 tokens x 7168: row_splits > 1.  Held to the oracle, aligned and misaligned."""
    n = sum(_unpermute_launches(case) for case in M.UNPERMUTE_SPLIT_CASES)
    print(f"unpermute, row splits: {n} launches checked")
    assert n == 8


def test_unpermute_with_two_chunks_per_thread():
    """1024 tokens x 2056: one row split and 257 chunks, so thread 0 of the streaming form goes round its chunk loop twice."""
    n = sum(_unpermute_launches(case) for case in M.UNPERMUTE_LOOP_CASES)
    print(f"unpermute, two chunks per thread: {n} launches checked")
    assert n == 4


@pytest.mark.parametrize("dt", list(M.DTYPES))
def test_unpermute_without_probabilities(dt):
    """hx_moe_unpermute with probs == NULL (every weight 1; the wrappers always hand probabilities over): the plain sum of
    the valid rows in map order, on the streaming form, the scalar form (dim 36, misaligned) and the fp32 kernel."""
    from hydrainfer_amd import _lib
    n = 0
    for case in (M.UnpermuteCase("index", dt, 5, 64, 7, 7), M.UnpermuteCase("mask", dt, 300, 36, 16, 4, False),
                 M.UnpermuteCase("mask", dt, 5, 2056, 60, 4, True)):
        b = M.unpermute(case)
        want = moe.unpermute_rows(b.x, b.row_map, None)
        row_map = b.row_map.to(DEV)
        for x in (b.x.to(DEV), misaligned(b.x.to(DEV))):
            out = torch.full((case.n_tokens, case.dim), float("nan"), dtype=b.x.dtype, device=DEV)
            _lib.check(_lib.lib().hx_moe_unpermute(x.data_ptr(), out.data_ptr(), row_map.data_ptr(), None, case.n_tokens,
                                                   case.n_rows, case.dim, _lib.dtype_code(x), _lib.current_stream()), "unpermute")
            assert torch.equal(out.cpu(), want), case.name      # fp32 too: adds only, in map order — nothing to fuse
            n += 1
    print(f"unpermute without probabilities {dt}: {n} launches checked")


@pytest.mark.parametrize("n_tokens,topk", M.SORT_SHAPES)
def test_index_row_map_at_every_sort_algorithm(n_tokens, topk):
    """n_tokens * topk = 1024 | 1025 | 32 768 | 1 048 576 | 1 048 584: rocPRIM's one-block sort, merge sort and onesweep
    (thresholds: tests/moe_cases.py, SORT_SHAPES).  Ids from 8 and 256 experts: many equal keys, stability decides the
    map.  The wrapper sizes the workspace with hx_moe_sort_workspace_bytes."""
    from hydrainfer_amd._C.kernel.moe import permute_with_index_map
    n = 0
    for n_experts in M.SORT_EXPERTS:
        tokens, ids, want_p, want_map = M.index_case(n_tokens, topk, n_experts, 8, "fp16")
        p, row_map = permute_with_index_map(tokens.to(DEV), ids.to(DEV))
        M.check_rows(p, row_map, want_p, want_map, f"{n_tokens} x {topk} ids of {n_experts} experts")
        n += 1
    print(f"index row map, {n_tokens * topk} items: {n} launches checked")


@pytest.mark.parametrize("n_tokens", M.MASK_TOKENS)
def test_mask_row_map_on_uneven_masks(n_tokens):
    """Uneven masks over 4, 60 and 257 experts: an empty expert, an expert with every token or a token routed nowhere,
    tokens with more than topk experts; 255 / 256 / 257 tokens are the edges of mask_assign_kernel's 256-token step.
    Only the first `total` permuted rows are compared."""
    from hydrainfer_amd._C.kernel.moe import permute_with_mask_map
    n = 0
    for n_experts in M.MASK_EXPERTS:
        for full in (False, True):
            topk = 2 if n_experts == 4 else 4
            tokens, routing, want_p, want_map = M.mask_case(n_tokens, n_experts, topk, 8, "fp16", full)
            p, row_map = permute_with_mask_map(tokens.to(DEV), routing.to(DEV), topk)
            assert p.shape[0] == n_tokens * topk
            M.check_rows(p, row_map, want_p, want_map, f"{n_tokens} tokens, {n_experts} experts, {'full' if full else 'holes'}")
            n += 1
    print(f"mask row map, {n_tokens} tokens: {n} launches checked")


@pytest.mark.parametrize("dt", list(M.DTYPES))
def test_permute_every_element_width(dt):
    """dim 7 (the element kernels), 4100 (fp32: 1025 16-byte chunks, five passes, the last partial; two-byte: 8200 bytes
    a row, the element kernel at a width above 64) and 4104 (two-byte: 513 chunks), tokens aligned and misaligned
    (uint16_t / uint32_t at every width), index and mask maps."""
    from hydrainfer_amd._C.kernel.moe import permute_with_index_map, permute_with_mask_map
    n = 0
    for dim in (7, 4100, 4104):
        tokens, ids, want_p, want_map = M.index_case(5, 3, 6, dim, dt)
        mtokens, routing, mwant_p, mwant_map = M.mask_case(5, 6, 2, dim, dt, True)
        for shift in (False, True):
            put = (lambda t: misaligned(t.to(DEV))) if shift else (lambda t: t.to(DEV))
            p, row_map = permute_with_index_map(put(tokens), ids.to(DEV))
            M.check_rows(p, row_map, want_p, want_map, f"index, dim {dim} {dt} misaligned={shift}")
            p, row_map = permute_with_mask_map(put(mtokens), routing.to(DEV), 2)
            M.check_rows(p, row_map, mwant_p, mwant_map, f"mask, dim {dim} {dt} misaligned={shift}")
            n += 2
    print(f"permute {dt}: {n} launches checked")


@pytest.mark.parametrize("dt", list(M.DTYPES))
@pytest.mark.parametrize("topk", M.SUM_OUT_TOPK)
def test_sum_out_main_loop_and_tail(topk, dt):
    """topk 5, 6, 7, 9, 16 (none of them a running sum in T), 3 tokens, dim 264 and 4104 (row splits), aligned and
    misaligned.  Inputs whose fp32 sums are exact in any order: bit for bit.  Positive inputs: equal to the oracle or
    1 ulp of T from it (torch's fp32 reduction order is its own); fp32 within 1e-5 relative."""
    from hydrainfer_amd._C.kernel.moe import sum_out
    dtype = M.DTYPES[dt]
    n = 0
    for dim in M.SUM_OUT_DIMS:
        exact, positive = M.sum_out_inputs(3, topk, dim, dt)
        want_exact, want_pos = moe.sum_out(exact), moe.sum_out(positive)
        for shift in (False, True):
            put = (lambda t: misaligned(t.to(DEV))) if shift else (lambda t: t.to(DEV))
            what = f"topk {topk} dim {dim} {dt} misaligned={shift}"
            out = torch.full((3, dim), float("nan"), dtype=dtype, device=DEV)
            sum_out(put(exact), out)
            assert torch.equal(out.cpu(), want_exact), f"{what}: {(out.cpu() != want_exact).sum().item()} elements differ"
            out = torch.full((3, dim), float("nan"), dtype=dtype, device=DEV)
            sum_out(put(positive), out)
            if dtype == torch.float32:
                err = (out.cpu().double() - want_pos.double()).abs()
                assert bool((err <= 1e-5 * want_pos.double().abs()).all()), f"{what}: max abs err {float(err.max()):.3e}"
            else:
                assert_ulp_close(out.cpu(), want_pos, max_ulp=1, what=what)
            n += 2
    print(f"sum_out topk {topk} {dt}: {n} launches checked")


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_sum_out_with_two_chunks_per_thread(dt):
    """1024 tokens x 5 x 2056: one row split, 257 chunks — thread 0 of the streaming form takes two."""
    from hydrainfer_amd._C.kernel.moe import sum_out
    n_tokens, topk, dim = M.SUM_OUT_LOOP_SHAPE
    exact, _ = M.sum_out_inputs(n_tokens, topk, dim, dt)
    out = torch.full((n_tokens, dim), float("nan"), dtype=M.DTYPES[dt], device=DEV)
    sum_out(exact.to(DEV), out)
    assert torch.equal(out.cpu(), moe.sum_out(exact))
    print(f"sum_out, two chunks per thread {dt}: 1 launch checked")


@pytest.mark.parametrize("n_experts", M.TOPK_EXPERTS)
def test_topk_softmax_every_lane_width(n_experts):
    """topk 1, 8 and n_experts (counts <= 65); 1 and 6 tokens (a half-full last workgroup); no ties, two tie groups
    (one of them at the row maximum), a quarter of the experts at -inf.  Indices exact, weights rtol 1e-5, atol 0."""
    from hydrainfer_amd._C.kernel.moe import topk_softmax
    n = 0
    for case in M.topk_cases(n_experts):
        b = M.build_topk(case)
        w = torch.full((case.n_tokens, case.topk), float("nan"), device=DEV)
        i = torch.full((case.n_tokens, case.topk), -1, dtype=torch.int32, device=DEV)
        topk_softmax(b.logits.to(DEV), w, i)
        M.check_topk(b, w, i)
        n += 1
    print(f"topk_softmax, {n_experts} experts: {n} launches checked")


@pytest.mark.parametrize("cfg", M.GROUPED_CASES)
def test_grouped_topk_sigmoid_accepted_shapes(cfg):
    """One group; topk_group == n_groups (the drop loop runs zero times); 64 groups of 16 (1024 experts, 32 KiB of LDS);
    60 experts in 4 groups.  Tie-heavy inputs; indices exact, weights allclose to the oracle and, where it takes the
    shape, to the lane-level emulator."""
    from hydrainfer_amd._C.kernel.moe import grouped_topk_sigmoid
    from tests.moe_lane_emulator import grouped_topk_sigmoid_lanes, tie_heavy_inputs
    n_experts, n_groups, topk_group, topk = cfg
    T = M.GROUPED_TOKENS
    logits, bias = tie_heavy_inputs(n_experts, T, 7 + n_experts + n_groups)
    lt, bt = torch.from_numpy(logits), torch.from_numpy(bias)
    w_ref, i_ref = moe.grouped_topk_sigmoid(lt, bt, n_groups, topk_group, topk)
    w = torch.full((T, topk), float("nan"), device=DEV)
    i = torch.full((T, topk), -1, dtype=torch.int32, device=DEV)
    grouped_topk_sigmoid(lt.to(DEV), bt.to(DEV), n_groups, topk_group, topk, 2.5, w, i)
    assert torch.equal(i.cpu(), i_ref)
    assert torch.allclose(w.cpu(), w_ref, rtol=1e-5, atol=1e-7)
    if M.emulator_accepts(n_groups):
        scores = (1.0 / (1.0 + torch.exp(-lt))).numpy()
        w_emu, i_emu = grouped_topk_sigmoid_lanes(scores, bias, n_groups, topk_group, topk)
        assert np.array_equal(i.cpu().numpy(), i_emu)
        assert np.allclose(w.cpu().numpy(), w_emu, rtol=1e-5, atol=1e-7)
    print(f"grouped_topk_sigmoid {cfg}: 1 launch checked")


def test_host_refusals_and_empty_batches():
    """The early returns of the seven entry points: a refused shape, dtype, pointer or workspace is an error code (nothing
    is launched), and n_tokens == 0 is HX_OK."""
    from hydrainfer_amd import _lib
    l, st = _lib.lib(), _lib.current_stream()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    SHAPE, DTYPE, NULL, WORKSPACE = -2, -1, -4, -6
    calls = [
        (SHAPE, l.hx_topk_softmax(p, p, p, 1, 1025, 1, st)), (SHAPE, l.hx_topk_softmax(p, p, p, 1, 8, 9, st)),
        (SHAPE, l.hx_topk_softmax(p, p, p, 1, 8, 0, st)), (NULL, l.hx_topk_softmax(p, None, p, 1, 8, 1, st)),
        (0, l.hx_topk_softmax(p, p, p, 0, 8, 1, st)),
        (SHAPE, l.hx_grouped_topk_sigmoid(p, p, p, p, 1, 2048, 8, 1, 1, 1.0, st)),
        (SHAPE, l.hx_grouped_topk_sigmoid(p, p, p, p, 1, 130, 65, 1, 1, 1.0, st)),
        (SHAPE, l.hx_grouped_topk_sigmoid(p, p, p, p, 1, 60, 8, 1, 1, 1.0, st)),
        (SHAPE, l.hx_grouped_topk_sigmoid(p, p, p, p, 1, 64, 8, 9, 1, 1.0, st)),
        (SHAPE, l.hx_grouped_topk_sigmoid(p, p, p, p, 1, 64, 8, 2, 17, 1.0, st)),
        (NULL, l.hx_grouped_topk_sigmoid(p, None, p, p, 1, 64, 8, 2, 4, 1.0, st)),
        (0, l.hx_grouped_topk_sigmoid(p, p, p, p, 0, 64, 8, 2, 4, 1.0, st)),
        (SHAPE, l.hx_moe_row_id_map_from_indices(p, p, 4, 0, p, 4096, st)),
        (SHAPE, l.hx_moe_row_id_map_from_indices(p, p, 1 << 30, 4, p, 4096, st)),
        (WORKSPACE, l.hx_moe_row_id_map_from_indices(p, p, 4, 2, p, l.hx_moe_sort_workspace_bytes(4, 2) - 1, st)),
        (NULL, l.hx_moe_row_id_map_from_indices(p, p, 4, 2, None, 4096, st)),
        (0, l.hx_moe_row_id_map_from_indices(p, p, 0, 2, p, 0, st)),
        (SHAPE, l.hx_moe_row_id_map_from_mask(p, p, 4, 65536, p, 1 << 20, st)),
        (WORKSPACE, l.hx_moe_row_id_map_from_mask(p, p, 4, 8, p, 31, st)),
        (NULL, l.hx_moe_row_id_map_from_mask(None, p, 4, 8, p, 32, st)), (0, l.hx_moe_row_id_map_from_mask(p, p, 0, 8, p, 32, st)),
        (DTYPE, l.hx_moe_permute(p, p, p, 1, 1, 8, 7, st)), (SHAPE, l.hx_moe_permute(p, p, p, 1, 0, 8, 1, st)),
        (NULL, l.hx_moe_permute(p, None, p, 1, 1, 8, 1, st)), (0, l.hx_moe_permute(p, p, p, 0, 1, 8, 1, st)),
        (DTYPE, l.hx_moe_unpermute(p, p, p, p, 1, 1, 8, 7, st)), (SHAPE, l.hx_moe_unpermute(p, p, p, p, 1, 1, 0, 1, st)),
        (NULL, l.hx_moe_unpermute(p, p, None, p, 1, 1, 8, 1, st)), (0, l.hx_moe_unpermute(p, p, p, p, 0, 1, 8, 1, st)),
        (DTYPE, l.hx_moe_sum_out(p, p, 1, 2, 8, 7, st)), (SHAPE, l.hx_moe_sum_out(p, p, 1, 0, 8, 1, st)),
        (NULL, l.hx_moe_sum_out(None, p, 1, 2, 8, 1, st)), (0, l.hx_moe_sum_out(p, p, 0, 2, 8, 1, st)),
    ]
    assert l.hx_moe_sort_workspace_bytes(0, 4) == 0
    for n, (want, got) in enumerate(calls):
        assert got == want, f"call {n}: returned {got}, expected {want}"
    torch.cuda.synchronize()
    assert not buf.any(), "a refused call wrote to memory"
    print(f"host refusals: {len(calls)} calls checked, none launched")
