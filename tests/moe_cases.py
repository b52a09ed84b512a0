"""MoE inputs whose answer pairs every expert row with its own weight (pure torch on the CPU, no GPU), shared by
tests/test_moe_cases_cpu.py (which proves every case sound on the oracle and every mutant refused by the checker) and
tests/test_gpu_moe_branches.py (which runs the same cases through every branch of hydrainfer_amd/csrc/moe.hip).

DISTINCT ROWS.  unpermute is handed a fresh random [n_rows_out, dim] "expert output", never the permuted copies of a
token: with copies the result is token * sum(probs) however the probabilities are paired with the rows.  Two-byte types
are held to oracle.moe.unpermute_rows bit for bit (each product and each partial sum rounded to T, in map order); fp32
to a float64 evaluation of sum_r p_r * x_r with the elementwise bound (n_valid + 1) * 2^-23 * sum_r |p_r * x_r| — twice
the first-order bound for n products and n adds in fp32, which leaves room for a fused multiply-add.

UNEVEN MASKS.  0 to 2 * topk experts per token, one expert column all false, and either one column all true ("full")
or one token routed nowhere ("holes": the two exclude each other), thinned until the total is at most n_tokens * topk:
the wrapper allocates that many rows and the kernels write wherever the map points, so the builder asserts it.
Unrouted probabilities are NaN: both kernels skip a negative map entry before they read the probability.

TOPK_SOFTMAX.  Each row is a permutation of distinct multiples of 0.25 from [-20, 20] (0.0625 from [-32, 32] above 161
experts): every difference is exact in fp32, so rounding cannot reorder them.  Deliberate exact ties sit at lanes
l, l + 64, l + 128, ... and across lanes; optionally a quarter of the experts is -inf.  Expected indices are the stable
descending argsort (lower index wins, selected -inf entries last in index order), expected weights the float64 softmax
at rtol 1e-5, atol 0.

MUTANTS map a built case to the output a subtly wrong kernel would give; each returns None where it does not apply."""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from oracle import moe

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
EPS32 = 2.0 ** -23
WEIGHT_RTOL = 1e-5
MIN_SEPARATION = 0.01


def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# uneven masks
# ---------------------------------------------------------------------------------------------------------------------
def uneven_mask(n_tokens: int, n_experts: int, topk: int, g: torch.Generator, full_expert: bool) -> torch.Tensor:
    """[n_tokens, n_experts] bool with at most n_tokens * topk entries set (asserted).  Needs n_experts >= 2."""
    assert n_experts >= 2 and topk >= 1
    kmax = min(2 * topk, n_experts)
    count = torch.randint(0, kmax + 1, (n_tokens,), generator=g)
    order = torch.rand((n_tokens, n_experts), generator=g).topk(kmax, dim=1).indices
    keep = torch.arange(kmax)[None, :] < count[:, None]
    mask = torch.zeros((n_tokens, n_experts), dtype=torch.bool).scatter_(1, order, keep)
    empty = int(torch.randint(0, n_experts, (1,), generator=g))
    full = (empty + 1 + int(torch.randint(0, n_experts - 1, (1,), generator=g))) % n_experts
    mask[:, empty] = False
    if full_expert:
        mask[:, full] = True
    else:
        mask[int(torch.randint(0, n_tokens, (1,), generator=g))] = False
    cap = n_tokens * topk
    excess = int(mask.sum()) - cap
    if excess > 0:
        free = mask.clone()
        if full_expert:
            free[:, full] = False
        cand = free.reshape(-1).nonzero()[:, 0]
        drop = cand[torch.randperm(cand.numel(), generator=g)[:excess]]
        mask.view(-1)[drop] = False
    assert int(mask.sum()) <= cap, "a mask with more than n_tokens * topk entries makes permute write past its output"
    assert not mask[:, empty].any() and (not full_expert or mask[:, full].all())
    return mask


# ---------------------------------------------------------------------------------------------------------------------
# unpermute on distinct rows
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class UnpermuteCase:
    """form "index": n_rows = topk valid rows per token.  form "mask": n_rows = n_experts, `topk` caps the total."""
    form: str
    dt: str
    n_tokens: int
    dim: int
    n_rows: int
    topk: int
    full_expert: bool = False

    @property
    def name(self):
        tail = ("-full" if self.full_expert else "-holes") if self.form == "mask" else ""
        return f"{self.form}-{self.dt}-n{self.n_tokens}-d{self.dim}-r{self.n_rows}-k{self.topk}{tail}"


@dataclass
class Unpermute:
    case: UnpermuteCase
    x: torch.Tensor                      # [n_tokens * topk, dim], the "expert output"
    row_map: torch.Tensor                # [n_rows, n_tokens] int32, -1 where not routed
    probs: torch.Tensor                  # [n_tokens, n_rows] in the case's dtype
    n_valid: torch.Tensor                # [n_tokens]
    expected: torch.Tensor               # two-byte: T, exact; fp32: float64
    bound: Optional[torch.Tensor]        # fp32 only: float64 elementwise bound


def kernel_arithmetic(x, row_map, probs):
    """What a correct kernel returns: oracle.moe.unpermute_rows (T products and T partial sums, map order)."""
    return moe.unpermute_rows(x, row_map, probs)


def _exact_sum(x, row_map, probs):
    """float64 sum_r p_r x_r and sum_r |p_r x_r| over the valid rows."""
    n_rows, n_tokens = row_map.shape
    acc = torch.zeros((n_tokens, x.shape[1]), dtype=torch.float64)
    mag = torch.zeros_like(acc)
    for r in range(n_rows):
        idx = row_map[r].long()
        ok = idx >= 0
        if not ok.any():
            continue
        p = torch.where(ok, probs[:, r].double(), torch.zeros((), dtype=torch.float64))[:, None]
        term = torch.where(ok[:, None], x[idx.clamp_min(0)].double() * p, torch.zeros((), dtype=torch.float64))
        acc += term
        mag += term.abs()
    return acc, mag


def build_unpermute(case: UnpermuteCase) -> Unpermute:
    dt = DTYPES[case.dt]
    n, dim, n_rows, topk = case.n_tokens, case.dim, case.n_rows, case.topk
    g = _gen(11, n, dim, n_rows, topk, case.full_expert, len(case.dt) + ord(case.dt[0]), case.form == "mask")
    if case.form == "index":
        assert n_rows == topk
        gating = torch.randn((n, max(16, topk)), generator=g)
        weights, ids = gating.topk(topk, dim=-1)
        probs = weights.softmax(dim=-1).to(dt)
        _, _, row_map = moe.permute_index(torch.empty((n, 1)), ids.to(torch.int32))
    else:
        routing = uneven_mask(n, n_rows, topk, g, case.full_expert)
        _, _, row_map = moe.permute_mask(torch.empty((n, 1)), routing)
        vals = 0.1 + 0.9 * torch.rand((n, n_rows), generator=g)
        probs = torch.where(routing, vals, torch.full((), float("nan"))).to(dt)
    x = torch.randn((n * topk, dim), generator=g).to(dt)
    assert int(row_map.max()) < x.shape[0]
    n_valid = (row_map >= 0).sum(dim=0)
    if dt == torch.float32:
        expected, mag = _exact_sum(x, row_map, probs)
        bound = (n_valid.double() + 1)[:, None] * EPS32 * mag
    else:
        expected, bound = kernel_arithmetic(x, row_map, probs), None
    return Unpermute(case, x, row_map, probs, n_valid, expected, bound)


def check_unpermute(b: Unpermute, out: torch.Tensor, what: str = "") -> None:
    """THE assertion of the GPU file for unpermute."""
    o = out.detach().cpu()
    what = what or b.case.name
    assert o.shape == b.expected.shape and o.dtype == DTYPES[b.case.dt], what
    if b.bound is None:
        if not torch.equal(o, b.expected):
            bad = (o != b.expected) | torch.isnan(o)
            t, i = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements differ from the oracle bit for bit; first: "
                                 f"token {t} (valid rows {int(b.n_valid[t])}) element {i}: got {float(o[t, i])} want {float(b.expected[t, i])}")
    else:
        err = (o.double() - b.expected).abs()
        bad = ~(err <= b.bound)                       # NaN lands here
        if bad.any():
            t, i = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements outside (n_valid + 1) * 2^-23 * sum|p x|; first: "
                                 f"token {t} (valid rows {int(b.n_valid[t])}) element {i}: got {float(o[t, i])} want "
                                 f"{float(b.expected[t, i])} +- {float(b.bound[t, i]):.3e}")
    dead = b.n_valid == 0
    assert not o[dead].float().abs().gt(0).any() and not torch.isnan(o[dead].float()).any(), f"{what}: a token routed nowhere is not zero"


def mut_flip_probs(b):
    """Probabilities flipped along topk (index form)."""
    if b.case.form != "index" or b.case.n_rows < 2:
        return None
    return kernel_arithmetic(b.x, b.row_map, b.probs.flip(1))


def mut_rotate_routed(b):
    """Routed probabilities rotated by one within each token's routed set (mask form)."""
    if b.case.form != "mask" or int(b.n_valid.max()) < 2:
        return None
    probs = b.probs.clone()
    for t in range(b.case.n_tokens):
        cols = (b.row_map[:, t] >= 0).nonzero()[:, 0]
        if cols.numel() >= 2:
            probs[t, cols] = b.probs[t, cols.roll(1)]
    return kernel_arithmetic(b.x, b.row_map, probs)


def mut_transposed_probs(b):
    """The probability matrix read as [n_rows, n_tokens]: probs[k * n_tokens + t] for probs[t * n_rows + k]."""
    n, r = b.case.n_tokens, b.case.n_rows
    if n < 2 or r < 2 or int(b.n_valid.max()) == 0:
        return None
    return kernel_arithmetic(b.x, b.row_map, b.probs.reshape(-1).view(r, n).t().contiguous())


def mut_reversed_order(b):
    """The sum taken in reversed map order: the same terms, other two-byte roundings."""
    if b.bound is not None or int(b.n_valid.max()) < 3:
        return None
    return kernel_arithmetic(b.x, b.row_map.flip(0), b.probs.flip(1))


def mut_unrouted_prob(b):
    """The j-th valid row of a token weighted with probs[t, j] (the compacted position, not the expert's column)."""
    if b.case.form != "mask" or int(b.n_valid.max()) == 0:
        return None
    probs = b.probs.clone()
    for t in range(b.case.n_tokens):
        cols = (b.row_map[:, t] >= 0).nonzero()[:, 0]
        probs[t, cols] = b.probs[t, :cols.numel()]
    return kernel_arithmetic(b.x, b.row_map, probs)


def mut_drop_last(b):
    """The last valid row of every token dropped (a tail loop that stops one row early)."""
    if int(b.n_valid.max()) == 0:
        return None
    row_map = b.row_map.clone()
    r = b.case.n_rows
    last = (r - 1) - (row_map.flip(0) >= 0).int().argmax(dim=0)
    has = b.n_valid > 0
    row_map[last[has], has.nonzero()[:, 0]] = -1
    return kernel_arithmetic(b.x, row_map, b.probs)


UNPERMUTE_MUTANTS = (("probs flipped along topk", mut_flip_probs), ("routed probs rotated", mut_rotate_routed),
                     ("probs indexed [n_rows, n_tokens]", mut_transposed_probs), ("map order reversed", mut_reversed_order),
                     ("unrouted probability used", mut_unrouted_prob), ("last valid row dropped", mut_drop_last))

_DIMS = (8, 64, 2056, 36)          # 2056: 257 chunks, the chunk loop runs twice; 36: not a multiple of 8, the scalar form
_TOKENS = (1, 5, 300)


def _unpermute_cases():
    out = []
    for dt in DTYPES:
        for topk in range(1, 10):                            # 4-row main loop and tail: 1..9 valid rows
            for di, dim in enumerate(_DIMS):
                out.append(UnpermuteCase("index", dt, _TOKENS[(topk + di) % 3], dim, topk, topk))
        for di, dim in enumerate(_DIMS):                     # uneven masks, topk 4: 0..8 valid rows
            for ti, n in enumerate(_TOKENS):
                for full in (False, True):
                    out.append(UnpermuteCase("mask", dt, n, dim, (8, 16, 60)[(di + ti + full) % 3], 4, full))
        for n_rows in (256, 257, 320):                       # the last size of the streaming form, then the scalar fall-back
            out.append(UnpermuteCase("mask", dt, 5, 64, n_rows, 4, n_rows == 320))
    return out


UNPERMUTE_CASES = _unpermute_cases()
# few tokens, a wide row: row_splits > 1 (the row cut into chunks over blockIdx.y)
UNPERMUTE_SPLIT_CASES = [UnpermuteCase(form, dt, 5, 7168, 8 if form == "index" else 60, 8 if form == "index" else 4, True)
                         for dt in ("fp16", "bf16") for form in ("index", "mask")]
# 1024 tokens: row_splits is min(ceil(1024 / n_tokens), ceil(chunks / 256)) = 1, so at 257 chunks a thread takes two of them
UNPERMUTE_LOOP_CASES = [UnpermuteCase("index", "fp16", 1024, 2056, 5, 5), UnpermuteCase("mask", "bf16", 1024, 2056, 8, 4, True)]

_cache = {}


def unpermute(case: UnpermuteCase) -> Unpermute:
    """build_unpermute(case), memoised; the tensors are read-only."""
    if case not in _cache:
        _cache[case] = build_unpermute(case)
    return _cache[case]


# ---------------------------------------------------------------------------------------------------------------------
# row maps and permute
# ---------------------------------------------------------------------------------------------------------------------
def index_case(n_tokens: int, topk: int, n_experts: int, dim: int, dt: str):
    """(tokens, topk_ids int32 [n_tokens, topk] drawn with repetition from n_experts, permuted, row_id_map)."""
    g = _gen(23, n_tokens, topk, n_experts, dim)
    ids = torch.randint(0, n_experts, (n_tokens, topk), generator=g, dtype=torch.int32)
    tokens = torch.randn((n_tokens, dim), generator=g).to(DTYPES[dt])
    permuted, _, row_map = moe.permute_index(tokens, ids)
    return tokens, ids, permuted, row_map


def mask_case(n_tokens: int, n_experts: int, topk: int, dim: int, dt: str, full_expert: bool):
    """(tokens, routing_map, the first `total` permuted rows, row_id_map) on an uneven mask."""
    g = _gen(29, n_tokens, n_experts, topk, dim, full_expert)
    routing = uneven_mask(n_tokens, n_experts, topk, g, full_expert)
    tokens = torch.randn((n_tokens, dim), generator=g).to(DTYPES[dt])
    permuted, _, row_map = moe.permute_mask(tokens, routing)
    assert permuted.shape[0] == int(routing.sum()) <= n_tokens * topk
    return tokens, routing, permuted, row_map


def check_rows(permuted, row_map, want_permuted, want_map, what: str) -> None:
    """Map identical; the first `total` rows a bit-exact copy (the rest is uninitialised by contract)."""
    m, p = row_map.detach().cpu(), permuted.detach().cpu()
    assert m.shape == want_map.shape and m.dtype == torch.int32, what
    if not torch.equal(m, want_map):
        bad = (m != want_map).nonzero()
        r, t = bad[0].tolist()
        raise AssertionError(f"{what}: {bad.shape[0]} map entries differ; first: row {r} token {t}: got {int(m[r, t])} want {int(want_map[r, t])}")
    total = want_permuted.shape[0]
    assert p.shape[0] >= total and p.dtype == want_permuted.dtype, what
    bits = {2: torch.int16, 4: torch.int32}[p.element_size()]
    assert torch.equal(p[:total].view(bits), want_permuted.view(bits)), f"{what}: permuted rows are not a bit-exact copy"


def mut_unstable_sort(ids: torch.Tensor, row_map: torch.Tensor):
    """Two equal keys swapped in the map (what an unstable sort may do); None if no key occurs twice."""
    n_tokens, topk = ids.shape
    flat = ids.reshape(-1)
    order = flat.argsort(stable=True)
    same = (flat[order][1:] == flat[order][:-1]).nonzero()
    if same.numel() == 0:
        return None
    a, b = int(order[same[0, 0]]), int(order[same[0, 0] + 1])
    out = row_map.clone()
    ia, ib = (a % topk, a // topk), (b % topk, b // topk)
    out[ia], out[ib] = row_map[ib], row_map[ia]
    return out


# rocPRIM's radix_sort_pairs (rocprim/device/device_radix_sort.hpp): one block up to block_size * items_per_thread =
# 256 * 4 = 1024 items (:598-600, :613-615), a merge sort up to merge_sort_limit (:644; 1024 * 1024 by default,
# device_radix_sort_config.hpp:50 — four-byte keys, so the 100 000-item clause of :644 does not apply), onesweep above
# (:666-670).  (n_tokens, topk): 1024 and 1025 straddle the first edge, 1 048 576 and 1 048 584 the second.
SORT_SHAPES = ((128, 8), (205, 5), (4096, 8), (131072, 8), (131073, 8))
SORT_EXPERTS = (8, 256)
MASK_TOKENS = (1, 255, 256, 257, 131073)      # 255 / 256 / 257: the edges of mask_assign_kernel's 256-token step
MASK_EXPERTS = (4, 60, 257)


# ---------------------------------------------------------------------------------------------------------------------
# sum_out
# ---------------------------------------------------------------------------------------------------------------------
def sum_out_inputs(n_tokens: int, topk: int, dim: int, dt: str):
    """(exact, positive) inputs [n_tokens, topk, dim].  exact: signed multiples of 1/16 up to 64 — rounding to T keeps a
    multiple of 1/16 one (the ulp of T is a power of two) and a sum of 16 stays below 2^10, 14 bits in all, so every fp32
    partial sum is exact in any order and the result is the one correct rounding: held bit for bit.  positive: |randn| * 50 — terms of one sign, so any fp32 summation
    order is within 16 * 2^-24 relative of the sum, far below an ulp of a two-byte T: two correct sums differ by at most
    the side of one rounding boundary (1 ulp of T), and by 1e-5 relative in fp32."""
    g = _gen(31, n_tokens, topk, dim)
    exact = (torch.randint(-1023, 1024, (n_tokens, topk, dim), generator=g).float() / 16).to(DTYPES[dt])
    positive = (torch.randn((n_tokens, topk, dim), generator=g).abs() * 50).to(DTYPES[dt])
    return exact, positive


SUM_OUT_TOPK = (5, 6, 7, 9, 16)
SUM_OUT_DIMS = (264, 4104)                    # 4104: 513 chunks, three row splits for 3 tokens, the last one partial
SUM_OUT_LOOP_SHAPE = (1024, 5, 2056)          # (n_tokens, topk, dim): one row split, 257 chunks — two chunks per thread


# ---------------------------------------------------------------------------------------------------------------------
# topk_softmax
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class TopkCase:
    n_tokens: int
    n_experts: int
    topk: int
    ties: int = 0                   # tie groups per row: group g holds the (g + 1)-th largest value of the row
    ninf: bool = False              # a quarter of the experts at -inf

    @property
    def name(self):
        return f"t{self.n_tokens}-e{self.n_experts}-k{self.topk}-ties{self.ties}" + ("-ninf" if self.ninf else "")


@dataclass
class Topk:
    case: TopkCase
    logits: torch.Tensor            # fp32 [n_tokens, n_experts]
    indices: torch.Tensor           # int32 [n_tokens, topk]
    weights: torch.Tensor           # float64 [n_tokens, topk]


def _stable_descending(logits64):
    return torch.argsort(logits64, dim=-1, descending=True, stable=True)


def build_topk(case: TopkCase) -> Topk:
    n, E, topk = case.n_tokens, case.n_experts, case.topk
    assert 1 <= topk <= E <= 1024
    g = _gen(37, n, E, topk, case.ties, case.ninf)
    step, half = (0.25, 80) if E <= 161 else (0.0625, 512)
    logits = torch.empty((n, E), dtype=torch.float32)
    lanes = min(64, E)
    assert 2 * case.ties <= lanes
    for r in range(n):
        row = (torch.randperm(2 * half + 1, generator=g)[:E] - half).float() * step
        if case.ninf:
            row[torch.randperm(E, generator=g)[:E // 4]] = float("-inf")
        finite = row[torch.isfinite(row)].sort(descending=True).values
        lane = torch.randperm(lanes, generator=g).tolist()
        for t in range(case.ties):
            same_lane = list(range(lane[2 * t], E, 64))          # l, l + 64, l + 128, ...: one lane's register slots
            row[same_lane + [lane[2 * t + 1]]] = finite[t]       # ... and another lane
        logits[r] = row
    l64 = logits.double()
    order = _stable_descending(l64)
    p = torch.softmax(l64, dim=-1)
    # the oracle alone: among the top topk + 1 probabilities neighbours are bit-equal logits or 1 % apart
    top = order[:, :min(topk + 1, E)]
    pt, lt = p.gather(1, top), logits.gather(1, top)
    tied = lt[:, 1:] == lt[:, :-1]
    apart = (pt[:, :-1] - pt[:, 1:]) >= MIN_SEPARATION * pt[:, :-1]
    assert bool((tied | apart).all()), f"{case.name}: a broken case — neighbouring probabilities closer than 1 %"
    return Topk(case, logits, order[:, :topk].to(torch.int32), p.gather(1, order[:, :topk]))


def check_topk(b: Topk, weights: torch.Tensor, indices: torch.Tensor, what: str = "") -> None:
    """THE assertion of the GPU file for topk_softmax: indices exact, weights within rtol 1e-5 (atol 0) of float64."""
    w, i = weights.detach().cpu(), indices.detach().cpu()
    what = what or b.case.name
    assert i.dtype == torch.int32 and i.shape == b.indices.shape and w.shape == b.weights.shape, what
    if not torch.equal(i, b.indices):
        t, k = (i != b.indices).nonzero()[0].tolist()
        raise AssertionError(f"{what}: indices differ; first: token {t} slot {k}: got {int(i[t, k])} want {int(b.indices[t, k])}")
    bad = ~((w.double() - b.weights).abs() <= WEIGHT_RTOL * b.weights.abs())
    if bad.any():
        t, k = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} weights off by more than 1e-5 relative; first: token {t} slot {k}: "
                             f"got {float(w[t, k])!r} want {float(b.weights[t, k])!r}")


def oracle_topk(b: Topk) -> Tuple[torch.Tensor, torch.Tensor]:
    return moe.topk_softmax(b.logits, b.case.topk)


def mut_ties_higher(b: Topk):
    """Ties broken to the higher index.  None where no tie reaches the selected set."""
    E = b.case.n_experts
    order = (E - 1) - _stable_descending(b.logits.double().flip(-1))
    idx = order[:, :b.case.topk]
    if torch.equal(idx.to(torch.int32), b.indices):
        return None
    return torch.softmax(b.logits, dim=-1).gather(1, idx), idx.to(torch.int32)


TOPK_EXPERTS = (5, 60, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1024)      # every kPerLane, both sides of each edge
TOPK_VARIANTS = ((0, False), (2, False), (1, True))


def topk_cases(n_experts: int):
    ks = sorted({1, min(8, n_experts)} | ({n_experts} if n_experts <= 65 else set()))
    return [TopkCase(n, n_experts, k, ties, ninf) for k in ks for n in (1, 6) for ties, ninf in TOPK_VARIANTS]


# ---------------------------------------------------------------------------------------------------------------------
# grouped_topk_sigmoid: the shapes the host accepts and nothing launched so far
# ---------------------------------------------------------------------------------------------------------------------
GROUPED_CASES = ((64, 1, 1, 8), (256, 8, 8, 8), (1024, 64, 8, 8), (60, 4, 2, 6))      # (experts, groups, topk_group, topk)
GROUPED_TOKENS = 6                    # one full workgroup of four tokens and a half-full one


def emulator_accepts(n_groups: int) -> bool:
    """tests/moe_lane_emulator.py follows the reference's butterflies: a power of two of at most 32 lanes."""
    return n_groups & (n_groups - 1) == 0 and n_groups <= 32
