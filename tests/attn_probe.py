"""Attention inputs whose answer is known exactly (pure torch, no GPU), shared by tests/test_attn_probe_cpu.py (which
proves each case sound and sensitive on the oracle) and tests/test_gpu_attention_probes.py (which runs the same cases
through every kernel path).

ONE-HOT PROBE.  Key position j of a sequence carries a sign code u_j in {-1, +1}^D per KV head, k_j = c * u_j with c a
power of two; a query row aimed at key t is c * u_t (of its KV head).  Every value is exact in fp16 / bf16 and every
product exact in fp32.  The score at t is c^2 * D * scale; when it exceeds every other visible score by MIN_GAP_LOG2 in
log2 units every other probability is exactly 0 in fp32 (2^-149 is the smallest subnormal), the target's is a power of
two, the row sum equals it, and the output is V[t] bit for bit, whatever the summation order, split count or rounding of
P.  V is small integers (|v| <= 128, exact in bf16) drawn per (physical page, offset, KV head, dim), so a read from a
wrong page, slot or head returns another row.

TRAP.  The slot just past a sequence's end, slot 0 of physical block 0 and slot 0 of a page no table references hold
the stale key 2c * u_x with V = 64.  A trap query is u_x / 4: over the visible keys it gives a broad softmax (scores
~ N(0, 4)), the trap would score 2 sqrt(D) above zero and drag the output towards 64.

POISON.  Every slot that (block_table, kv_len) does not address is NaN, or +inf in K and the largest finite value in V.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from oracle import ops
from tests import alibi_ref
from tests.util import ATTN_TOL, assert_close_t

MIN_GAP_LOG2 = 200.0
LOG2E = 1.4426950408889634
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
TRAP_V = 64.0
X = -2        # "the trap's code": a target no key of the sequence carries


@dataclass(frozen=True)
class Case:
    """aim: "targets" (decode: one explicit key per sequence), "diag" / "first" (last / first visible key of every row),
    "win_left" / "win_right" (the window's edges), and the tolerance-judged trap aims "trap" (decode: u_x),
    "past_right" / "past_left" (the first hidden key on that side of every row), "random" (randn inputs)."""
    name: str
    dt: str
    H: int
    HK: int
    D: int
    q_lens: Tuple[int, ...]
    kv_lens: Tuple[int, ...]
    aim: str
    targets: Tuple[int, ...] = ()
    bs: int = 16                    # 0: dense layout
    causal: bool = True
    window: Optional[Tuple[int, int]] = None
    softcap: float = 0.0
    alibi: bool = False
    c: int = 8
    seed: int = 0

    @property
    def exact(self):
        return self.aim in ("targets", "diag", "first", "win_left", "win_right")

    @property
    def decode(self):
        return self.bs > 0 and all(q == 1 for q in self.q_lens)


@dataclass
class Probe:
    case: Case
    q: torch.Tensor
    kc: torch.Tensor                 # paged [n_blocks, bs, HK, D]; dense [total_k, HK, D]
    vc: torch.Tensor
    cu_q: torch.Tensor
    cu_k: torch.Tensor
    bt: Optional[torch.Tensor]
    cu_b: Optional[torch.Tensor]
    slopes: Optional[torch.Tensor]
    row_target: List[int]            # per query row: key index, X, or -1 (no target)
    expected: torch.Tensor = None    # exact cases: V[t] per row and head; others: the oracle's output
    extra: dict = field(default_factory=dict)

    @property
    def max_q(self):
        return max(self.case.q_lens)

    @property
    def max_k(self):
        return max(max(self.case.kv_lens), 1)


def _signs(shape, g):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def c_for(D, alibi=False):
    """c = 8 gives the gaps of the measured table at D >= 64; short codes correlate more (D = 32: only distinct codes are
    guaranteed, dot <= 30 of 32), and the ALiBi bias eats up to slope * distance, so those take a larger power of two."""
    if D == 32:
        return 32
    return 16 if (D == 96 or alibi) else 8


def alibi_slopes(H):
    """The standard geometric slopes 2^(-8 i / H), i = 1..H (H a power of two), fp32."""
    return torch.tensor([2.0 ** (-8.0 * (i + 1) / H) for i in range(H)], dtype=torch.float32)


def visible_range(case: Case, i: int, lq: int, lk: int):
    """Keys [lo, hi] that query row i of lq sees among lk keys (hi < lo: none)."""
    d = i + lk - lq
    lo, hi = 0, lk - 1
    if case.window is not None:
        l, r = case.window
        if l >= 0:
            lo = max(lo, d - l)
        if r >= 0:
            hi = min(hi, d + r)
    elif case.causal:
        hi = min(hi, d)
    return lo, hi


def _row_targets(case: Case, b: int, lq: int, lk: int):
    out = []
    for i in range(lq):
        lo, hi = visible_range(case, i, lq, lk)
        if case.aim == "targets":
            t = case.targets[b]
        elif case.aim in ("diag", "win_right"):
            t = hi
        elif case.aim in ("first", "win_left"):
            t = lo
        elif case.aim == "trap":
            t = X
        elif case.aim == "past_right":
            t = hi + 1 if hi + 1 < lk else X
        elif case.aim == "past_left":
            t = lo - 1 if lo - 1 >= 0 else X
        else:
            t = -1
        if case.exact:
            assert lo <= t <= hi, (case.name, b, i, t, lo, hi)
        out.append(t)
    return out


def build(case: Case) -> Probe:
    dt = DTYPES[case.dt]
    g = torch.Generator().manual_seed(1000 + case.seed)
    H, HK, D, bs, c = case.H, case.HK, case.D, case.bs, case.c
    group = H // HK
    B = len(case.kv_lens)
    paged = bs > 0
    rand = case.aim == "random"
    cu = lambda ls: torch.tensor([0] + torch.tensor(list(ls)).cumsum(0).tolist(), dtype=torch.int32)
    cu_q, cu_k = cu(case.q_lens), cu(case.kv_lens)
    u_x = _signs((HK, D), g)
    if paged:
        nb = [(l + bs - 1) // bs for l in case.kv_lens]
        n_blocks = 1 + sum(nb) + 3                       # block 0 is never in a table; three pages nobody references
        kc = torch.randn((n_blocks, bs, HK, D), generator=g) if rand else c * _signs((n_blocks, bs, HK, D), g)
        if case.exact:
            vc = torch.randint(-128, 129, (n_blocks, bs, HK, D), generator=g).float()
        else:
            vc = torch.randn((n_blocks, bs, HK, D), generator=g)
        perm = (torch.randperm(n_blocks - 1, generator=g) + 1).tolist()
        tables, used = [], 0
        for n in nb:
            tables.append(perm[used: used + n])
            used += n
        spare = perm[used:]
        bt = torch.tensor([p for t in tables for p in t], dtype=torch.int32)
        cu_b = cu(nb)
        if not rand:
            for b, l in enumerate(case.kv_lens):            # the stale key just past the end, inside the last page
                if l % bs:
                    kc[tables[b][l // bs], l % bs] = 2 * c * u_x
                    vc[tables[b][l // bs], l % bs] = TRAP_V
            for page in (0, spare[0]):
                kc[page, 0] = 2 * c * u_x
                vc[page, 0] = TRAP_V
        slot = lambda b, j: (tables[b][j // bs], j % bs)
    else:
        total = int(cu_k[-1])
        kc = torch.randn((total, HK, D), generator=g) if rand else c * _signs((total, HK, D), g)
        vc = torch.randint(-128, 129, (total, HK, D), generator=g).float() if case.exact else torch.randn((total, HK, D), generator=g)
        bt = cu_b = None
        slot = lambda b, j: (int(cu_k[b]) + j,)
    q = torch.randn((int(cu_q[-1]), H, D), generator=g) if rand else torch.zeros((int(cu_q[-1]), H, D))
    row_target, expected = [], torch.zeros((int(cu_q[-1]), H, D))
    for b, (lq, lk) in enumerate(zip(case.q_lens, case.kv_lens)):
        ts = _row_targets(case, b, lq, lk) if not rand else [-1] * lq
        for i, t in enumerate(ts):
            r = int(cu_q[b]) + i
            if rand:
                continue
            code = u_x if t == X else kc[slot(b, t)] / c                    # [HK, D]
            amp = c if case.exact else 0.25
            q[r] = (amp * code).repeat_interleave(group, dim=0)
            if case.exact:
                expected[r] = vc[slot(b, t)].repeat_interleave(group, dim=0)
        row_target += ts
    slopes = alibi_slopes(H) if case.alibi else None
    p = Probe(case, q.to(dt), kc.to(dt), vc.to(dt), cu_q, cu_k, bt, cu_b, slopes, row_target)
    p.expected = expected.to(dt) if case.exact else oracle(p)
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the oracle, the precondition and the assertion the GPU file applies
# ---------------------------------------------------------------------------------------------------------------------
def oracle(p: Probe, q=None, kc=None, vc=None, cu_k=None, bt=None, window="same") -> torch.Tensor:
    """oracle.ops (tests/alibi_ref.py with slopes) on the probe, any argument replaced — that is how the CPU test moves a
    mask by one key.  Result in the probe's dtype."""
    c = p.case
    q = p.q if q is None else q
    kc = p.kc if kc is None else kc
    vc = p.vc if vc is None else vc
    cu_k = p.cu_k if cu_k is None else cu_k
    bt = p.bt if bt is None else bt
    window = c.window if window == "same" else window
    causal = c.causal and window is None
    if c.bs > 0:
        if p.slopes is not None:      # attend_alibi over the gathered pages (paged_attention_alibi insists on exact tables)
            out = torch.zeros(q.shape, dtype=torch.float32)
            for b in range(len(c.kv_lens)):
                q0, q1, lk = int(p.cu_q[b]), int(p.cu_q[b + 1]), int(cu_k[b + 1]) - int(cu_k[b])
                pages = bt[int(p.cu_b[b]): int(p.cu_b[b + 1])].long()
                k, v = (t[pages].reshape(-1, c.HK, c.D)[:lk] for t in (kc, vc))
                out[q0:q1] = alibi_ref.attend_alibi(q[q0:q1], k, v, 1.0 / math.sqrt(c.D), causal, p.slopes, c.softcap, window)
            return out.to(q.dtype)
        return ops.paged_attention(q, kc, vc, p.cu_q, cu_k, bt, p.cu_b, causal=causal, softcap=c.softcap, window=window)
    if p.slopes is not None:
        return alibi_ref.dense_attention_alibi(q, kc, vc, p.cu_q, cu_k, p.slopes, causal=causal, softcap=c.softcap,
                                               window=window).to(q.dtype)
    return ops.varlen_attention(q, kc, vc, p.cu_q, cu_k, causal=causal, softcap=c.softcap, window=window)


def gather_keys(p: Probe, b: int, kc=None) -> torch.Tensor:
    kc = p.kc if kc is None else kc
    lk = p.case.kv_lens[b]
    if p.case.bs > 0:
        pages = p.bt[int(p.cu_b[b]): int(p.cu_b[b + 1])].long()
        return kc[pages].reshape(-1, *kc.shape[2:])[:lk].float()
    return kc[int(p.cu_k[b]): int(p.cu_k[b]) + lk].float()


def min_gap_log2(p: Probe, q=None, kc=None) -> float:
    """Smallest lead, in log2 units, of the target's (biased) score over every other visible key's, over all rows and
    heads.  inf when no row has a competitor."""
    c = p.case
    q = (p.q if q is None else q).float()
    scale = 1.0 / math.sqrt(c.D)
    worst = float("inf")
    for b, (lq, lk) in enumerate(zip(c.q_lens, c.kv_lens)):
        if lq == 0:
            continue
        k = gather_keys(p, b, kc).repeat_interleave(c.H // c.HK, dim=1)                    # [lk, H, D]
        r0 = int(p.cu_q[b])
        s = torch.einsum("qhd,khd->hqk", q[r0: r0 + lq], k) * scale
        x = torch.arange(lk)[None, None, :]
        y = torch.arange(lq)[None, :, None]
        if p.slopes is not None:
            s = s - p.slopes[:, None, None] * (y + (lk - lq) - x).abs().float()
        for i in range(lq):
            lo, hi = visible_range(c, i, lq, lk)
            t = p.row_target[r0 + i]
            row = s[:, i, lo: hi + 1].clone()
            st = row[:, t - lo].clone()
            row[:, t - lo] = float("-inf")
            if hi > lo:
                worst = min(worst, float(((st - row.max(dim=1).values) * LOG2E).min()))
    return worst


def check(p: Probe, out: torch.Tensor, what: str = "") -> None:
    """THE assertion of the GPU file.  Exact cases: finite and bit-equal to V[t], no tolerance.  The others: finite and
    within ATTN_TOL of the oracle."""
    o = out.detach().cpu()
    what = what or p.case.name
    assert o.shape == p.expected.shape and o.dtype == p.expected.dtype, what
    assert bool(torch.isfinite(o.float()).all()), f"{what}: non-finite output"
    if p.case.exact:
        if not torch.equal(o, p.expected):
            bad = (o != p.expected).any(dim=-1).nonzero()
            r, h = bad[0].tolist()
            raise AssertionError(f"{what}: {bad.shape[0]} (row, head) pairs differ from V[t]; first: row {r} head {h} "
                                 f"target {p.row_target[r]}: got {o[r, h, :4].tolist()} want {p.expected[r, h, :4].tolist()}")
    else:
        assert_close_t(o, p.expected, *ATTN_TOL[o.dtype], what=what)


# ---------------------------------------------------------------------------------------------------------------------
# poison
# ---------------------------------------------------------------------------------------------------------------------
def addressed_mask(p: Probe, drop_last: bool = False) -> torch.Tensor:
    """[n_blocks, bs] bool: slots that (block_table, kv_len) address.  drop_last: without each sequence's last key (the
    slot the fused decode kernel writes before it reads)."""
    n_blocks, bs = p.kc.shape[:2]
    m = torch.zeros((n_blocks, bs), dtype=torch.bool)
    for b, lk in enumerate(p.case.kv_lens):
        pages = p.bt[int(p.cu_b[b]): int(p.cu_b[b + 1])].long()
        n = lk - 1 if drop_last else lk
        flat = torch.zeros(pages.numel() * bs, dtype=torch.bool)
        flat[:n] = True
        m[pages] = flat.view(-1, bs)
    return m


POISONS = ("nan", "inf")


def poisoned(p: Probe, kind: str, drop_last: bool = False, kc=None, vc=None):
    """Copies of the pool with every unaddressed slot NaN ("nan"), or +inf in K and the largest finite value in V."""
    kc = (p.kc if kc is None else kc).clone()
    vc = (p.vc if vc is None else vc).clone()
    dead = ~addressed_mask(p, drop_last)
    kc[dead] = float("nan") if kind == "nan" else float("inf")
    vc[dead] = float("nan") if kind == "nan" else torch.finfo(vc.dtype).max
    return kc, vc


# ---------------------------------------------------------------------------------------------------------------------
# fused decode (RoPE + cache append + attention): inputs from a decode probe
# ---------------------------------------------------------------------------------------------------------------------
def fused_inputs(p: Probe, max_pos: int = 4096):
    """The decode probe as decode_attention_fused takes it: the last key of every sequence leaves the cache (its slot
    holds a finite decoy) and comes in as k_new / v_new, un-rotated.  The kernel rotates q and k_new by position
    kv_len - 1; V is not rotated, so the expected row is still V[t].  A target that is the new token: q and k_new carry
    the same code and get the same rotation.  A cached target: the cache holds the oracle's rotation of c * u_t at
    position kv_len - 1.  Returns (q, k_new, v_new, kc, vc, pos, cos_sin, slots)."""
    c = p.case
    assert c.decode and p.slopes is None
    bs = c.bs
    B = len(c.kv_lens)
    dt = p.q.dtype
    cs = ops.build_cos_sin_cache(c.D, max_pos, 1e4, dt)
    pos = torch.tensor([l - 1 for l in c.kv_lens], dtype=torch.int32)
    kc, vc = p.kc.clone(), p.vc.clone()
    k_new = torch.zeros((B, c.HK, c.D), dtype=dt)
    v_new = torch.zeros((B, c.HK, c.D), dtype=dt)
    slots = []
    g = torch.Generator().manual_seed(77 + c.seed)
    for b, l in enumerate(c.kv_lens):
        page, off = int(p.bt[int(p.cu_b[b]) + (l - 1) // bs]), (l - 1) % bs
        slots.append(page * bs + off)
        k_new[b], v_new[b] = kc[page, off], vc[page, off]
        kc[page, off] = (c.c * _signs((c.HK, c.D), g)).to(dt)
        vc[page, off] = 77
        t = p.row_target[b]
        if 0 <= t < l - 1:
            tp, to = int(p.bt[int(p.cu_b[b]) + t // bs]), t % bs
            _, kr = ops.apply_rotary_pos_emb(p.q[b: b + 1], kc[tp, to][None], pos[b: b + 1], cs, c.D, False)
            kc[tp, to] = kr[0]
    return p.q, k_new, v_new, kc, vc, pos, cs, torch.tensor(slots, dtype=torch.int32)


def fused_oracle(p: Probe, fi, kc=None, vc=None):
    """apply_rotary_pos_emb + set_kv_cache + paged_attention on copies: (out, rotated q, kc, vc)."""
    q, k_new, v_new, kc0, vc0, pos, cs, slots = fi
    kc = (kc0 if kc is None else kc).clone()
    vc = (vc0 if vc is None else vc).clone()
    qr, kr = ops.apply_rotary_pos_emb(q, k_new, pos, cs, p.case.D, False)
    ops.set_kv_cache(slots, kr, v_new, kc, vc)
    return oracle(p, q=qr, kc=kc, vc=vc), qr, kc, vc


# ---------------------------------------------------------------------------------------------------------------------
# mutations: the same case with a mask moved by one key.  Each returns the oracle's output of the moved case, or None
# when it does not apply to the case; tests/test_attn_probe_cpu.py demands that every case has at least one that applies
# and that check() refuses every one.
# ---------------------------------------------------------------------------------------------------------------------
def _mut_kv_minus_1(p):
    """kv_len - 1: in decode the last key vanishes, under a causal mask the diagonal moves one key left."""
    c = p.case
    if c.bs == 0 or c.window is not None or c.aim not in ("targets", "diag"):
        return None
    if c.aim == "targets" and not any(t == l - 1 for t, l in zip(c.targets, c.kv_lens)):
        return None
    lens = [max(l - 1, 0) for l in c.kv_lens]
    return oracle(p, cu_k=torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32))


def _mut_kv_plus_1(p):
    """kv_len + 1 (where the last page has a slot left): the slot past the end (the trap, or NaN in a poisoned pool)
    becomes visible; under a causal mask the diagonal moves one key right."""
    c = p.case
    if c.bs == 0 or c.aim not in ("trap", "past_right", "random") or (c.window is not None and c.aim != "random"):
        return None
    lens = [l + 1 if l % c.bs else l for l in c.kv_lens]
    if lens == list(c.kv_lens):
        return None
    kc, vc = (p.kc, p.vc) if c.aim != "random" else poisoned(p, "nan")
    return oracle(p, kc=kc, vc=vc, cu_k=torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32))


def _mut_window(p):
    """A window edge moved by one key: inwards for the rows aimed at the edge, outwards for those aimed past it."""
    c = p.case
    if c.window is None or c.aim not in ("win_left", "win_right", "past_left", "past_right"):
        return None
    side = 0 if c.aim.endswith("left") else 1
    moved = c.window[side] + (-1 if c.aim.startswith("win") else 1)
    if c.window[side] < 0 or moved < 0:                     # an open side has no edge; a zero side no inward move
        return None
    return oracle(p, window=(moved, c.window[1]) if side == 0 else (c.window[0], moved))


def _mut_table_entry(p):
    """A tile that reads the neighbouring page: the page-table entry of each sequence's (first) target replaced by its
    neighbour's in the flat table.  (A swap of two entries of one sequence only permutes its keys, and attention
    without a mask between them does not see a permutation — it would prove nothing.)"""
    c = p.case
    if c.bs == 0 or not c.exact or p.bt.numel() < 2:
        return None
    bt = p.bt.clone()
    for b in range(len(c.kv_lens)):
        ts = p.row_target[int(p.cu_q[b]): int(p.cu_q[b + 1])]
        if not ts:
            continue
        e = int(p.cu_b[b]) + ts[0] // c.bs
        bt[e] = p.bt[e + 1] if e + 1 < p.bt.numel() else p.bt[e - 1]
    return oracle(p, bt=bt)


def _mut_row_shift(p):
    """Dense layout: every key row read one row off — towards the side that hides the aimed-at code (or, for rows aimed
    past the right edge, shows it)."""
    if p.case.bs != 0:
        return None
    sh = 1 if p.case.aim in ("diag", "win_right") else -1
    return oracle(p, kc=torch.roll(p.kc, sh, dims=0), vc=torch.roll(p.vc, sh, dims=0))


MUTATIONS = (("kv_len - 1", _mut_kv_minus_1), ("kv_len + 1", _mut_kv_plus_1), ("window edge", _mut_window),
             ("page-table entry", _mut_table_entry), ("dense row shift", _mut_row_shift))


# ---------------------------------------------------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------------------------------------------------
EDGE_LENS = (1, 16, 17, 33, 255, 256, 257, 704, 1500, 4095)
TILE_EDGES = (15, 16, 17, 31, 32, 33, 63, 64)
SPLITS = (0, 1, 2, 3, 7, 64)


def split_edges(lk: int, limit: int = 32):
    """First and last key of every split for num_splits in {2, 3, 7, 64}: both decode kernels give a split
    ceil(n_tiles / num_splits) whole tiles (16 keys per tile in the per-head kernel, 32 in the grouped-query one)."""
    edges = set()
    for tile in (16, 32):
        n_tiles = (lk + tile - 1) // tile
        for s in (2, 3, 7, 64):
            per = (n_tiles + s - 1) // s
            bounds = [k * per * tile for k in range(1, s) if k * per * tile < lk]
            if len(bounds) > 6:                              # 64 splits: the first two, the middle one, the last two
                bounds = bounds[:2] + [bounds[len(bounds) // 2]] + bounds[-2:]
            for x in bounds:
                edges.update((x - 1, x))
    return tuple(sorted(edges))[:limit]


def _decode_cases(tag, dt, H, HK, D, bs=16, alibi=False, full=True):
    c = c_for(D, alibi)
    mk = lambda name, lens, ts, seed: Case(f"{tag}-{name}-{dt}-H{H}/{HK}-D{D}-bs{bs}", dt, H, HK, D, (1,) * len(lens),
                                           tuple(lens), "targets", tuple(ts), bs=bs, alibi=alibi, c=c, seed=seed)
    lens = tuple(l for l in EDGE_LENS if not alibi or l <= 704)
    out = [mk("last", lens, [l - 1 for l in lens], 1), mk("first", lens, [0] * len(lens), 2)]
    if full:
        long = 300 if alibi else 704
        out.append(mk("tile", (long,) * 7 + (65,), TILE_EDGES, 3))                     # 64 is also a last key
        be = (bs - 1, bs, 2 * bs - 1, 2 * bs, 4 * bs - 1, 4 * bs)
        out.append(mk("block", (long,) * 5 + (4 * bs + 1,), be, 4))
        if not alibi:
            se = split_edges(1500)
            out.append(mk("split", (1500,) * (len(se) - 1) + (se[-1] + 1,), se, 5))
    return out


def _trap_decode(tag, dt, H, HK, D, bs=16):
    lens = (1, 17, 33, 255, 257, 700, 1499, 4095)
    return Case(f"{tag}-trap-{dt}-H{H}/{HK}-D{D}-bs{bs}", dt, H, HK, D, (1,) * len(lens), lens, "trap", bs=bs, seed=6)


# per-head decode (decode_gqa = 0), the 8-wave form at (32, 32) x 8 sequences; every D, dtype and block size somewhere
PER_HEAD_DECODE = (
    _decode_cases("ph", "fp16", 8, 8, 128) + _decode_cases("ph", "bf16", 8, 8, 64, bs=32) +
    _decode_cases("ph", "bf16", 4, 4, 256, bs=64, full=False) + _decode_cases("ph", "fp16", 8, 2, 128, bs=64) +
    [Case("ph-8wave-bf16", "bf16", 32, 32, 128, (1,) * 8, (1, 16, 17, 100, 255, 256, 33, 704), "targets",
          (0, 15, 16, 99, 0, 255, 31, 703), seed=7),
     _trap_decode("ph", "fp16", 8, 8, 128), _trap_decode("ph", "bf16", 8, 2, 64, bs=32)])

GQA_DECODE = (
    _decode_cases("gqa", "bf16", 8, 4, 128) + _decode_cases("gqa", "fp16", 28, 4, 64, bs=32) +
    _decode_cases("gqa", "fp16", 16, 1, 256, bs=64, full=False) + _decode_cases("gqa", "fp16", 8, 4, 64, bs=64) +
    [_trap_decode("gqa", "bf16", 8, 4, 128), _trap_decode("gqa", "fp16", 16, 1, 64, bs=64)])

ALIBI_DECODE = (_decode_cases("alibi-ph", "fp16", 8, 8, 128, alibi=True) +
                _decode_cases("alibi-gqa", "bf16", 8, 2, 128, bs=32, alibi=True, full=False))

# fused decode: the lengths of test_fused_rope_cache_decode_attention_is_bit_identical; the target is the new token in
# one pass, a cached key in the other (the single-key sequence keeps the new token)
_FUSED_LENS = (1, 16, 17, 100, 255, 256, 33, 704)


def _fused_cases(dt, H, HK, D, bs=16):
    mk = lambda name, ts, seed: Case(f"fused-{name}-{dt}-H{H}/{HK}-D{D}-bs{bs}", dt, H, HK, D, (1,) * 8, _FUSED_LENS,
                                     "targets", tuple(ts), bs=bs, seed=seed)
    return [mk("new", [l - 1 for l in _FUSED_LENS], 8), mk("cached", (0, 14, 15, 0, 253, 239, 16, 31), 9)]


FUSED_DECODE = (_fused_cases("fp16", 8, 8, 128) + _fused_cases("bf16", 8, 2, 64, bs=32) +
                _fused_cases("bf16", 32, 32, 128) + _fused_cases("fp16", 4, 4, 256, bs=64))

# prefill: the q_len / kv_len mixes of the existing prefill tests (cached prefixes, runs of 1, 31, 64, 65, 129, 577,
# 1100, q_len = 0 inside the batch)
_MIX_A = ((1, 129, 64, 0, 31, 128), (77, 129, 300, 17, 31, 1000))
_MIX_B = ((65, 0, 577, 1), (65, 30, 600, 49))
_MIX_LONG = ((1100, 130), (1100, 1500))
_MIX_SMALL = ((1, 40, 7, 0, 31), (1, 40, 100, 5, 77))       # max q_len <= 64: stays on the 16x16x32 kernel


def _prefill(tag, dt, H, HK, D, mix, bs=16, aims=("diag", "first", "past_right"), **kw):
    return [Case(f"{tag}-{a}-{dt}-H{H}/{HK}-D{D}-bs{bs}", dt, H, HK, D, mix[0], mix[1], a, bs=bs,
                 c=c_for(D, kw.get("alibi", False)), seed=10 + i, **kw) for i, a in enumerate(aims)]


PREFILL = (_prefill("pf-a", "fp16", 4, 2, 128, _MIX_A) + _prefill("pf-a", "bf16", 4, 4, 64, _MIX_A, bs=32) +
           _prefill("pf-b", "bf16", 8, 2, 128, _MIX_B, bs=64) + _prefill("pf-b", "fp16", 3, 3, 64, _MIX_B) +
           _prefill("pf-long", "bf16", 2, 2, 128, _MIX_LONG, aims=("diag", "first")))
PREFILL_D256 = _prefill("pf-a", "fp16", 2, 1, 256, _MIX_A, bs=32)
GENERAL = (_prefill("gen", "fp16", 4, 4, 32, _MIX_SMALL) + _prefill("gen", "bf16", 4, 2, 96, _MIX_SMALL, bs=32) +
           _prefill("gen", "fp16", 4, 4, 96, _MIX_A, aims=("diag",)) + _prefill("gen", "bf16", 2, 2, 32, _MIX_B, aims=("diag",)))
ALIBI_PREFILL = _prefill("alibi-pf", "fp16", 8, 2, 128, ((1, 50, 128, 3, 0, 200), (300, 50, 200, 67, 9, 200)),
                         aims=("diag", "first"), alibi=True)
_DENSE_LENS = (1, 17, 64, 65, 200, 577)
DENSE = (_prefill("dense-causal", "fp16", 4, 2, 64, (_DENSE_LENS, _DENSE_LENS), bs=0, aims=("diag", "first", "past_right")) +
         _prefill("dense-full", "bf16", 4, 4, 128, (_DENSE_LENS, _DENSE_LENS), bs=0, aims=("diag", "first"), causal=False) +
         _prefill("dense-full", "fp16", 4, 2, 64, ((70, 33, 130), (70, 90, 130)), bs=0, aims=("diag", "first"), causal=False))

WINDOWS = ((16, 0), (0, 16), (7, 3), (-1, 5))
_WIN_MIXES = (((1, 1, 1), (100, 17, 260)), ((15, 111), (15, 234)), ((130,), (130,)))


def _window_cases():
    out = []
    for wi, w in enumerate(WINDOWS):
        for mi, mix in enumerate(_WIN_MIXES):
            dt = ("fp16", "bf16")[(wi + mi) % 2]
            # decode rows (mix 0) end at the sequence's last key whatever the right edge says: left-side aims only there
            aims = (["win_right", "past_right"] if mi else []) + (["win_left", "past_left"] if w[0] >= 0 else ["first"])
            out += [Case(f"win{w}-{a}-{dt}-mix{mi}", dt, 8, 2, 128, mix[0], mix[1], a, causal=False, window=w,
                         seed=40 + wi) for a in aims]
        out += [Case(f"win{w}-dense-{a}", "fp16", 4, 2, 64, (70, 33), (70, 33), a, bs=0, causal=False, window=w, seed=50 + wi)
                for a in ("win_right", "first" if w[0] < 0 else "win_left")]
    return out


WINDOW = _window_cases()

# random inputs of one representative per path, for the poisoned pool (soft-cap and windows included)
_R = lambda name, dt, H, HK, D, mix, **kw: Case(f"rand-{name}-{dt}", dt, H, HK, D, mix[0], mix[1], "random", **kw)
_DEC_MIX = ((1,) * 6, (1, 17, 33, 255, 700, 1499))
_PF_MIX = ((1, 129, 64, 0, 31, 200), (77, 129, 300, 9, 31, 1001))
RANDOM_DECODE = (_R("decode", "fp16", 8, 8, 128, _DEC_MIX, seed=61), _R("decode-gqa", "bf16", 8, 2, 128, _DEC_MIX, bs=32, seed=62))
RANDOM_PREFILL = (_R("prefill", "bf16", 4, 2, 128, _PF_MIX, seed=63), _R("prefill", "fp16", 4, 4, 64, _PF_MIX, bs=64, seed=64))
RANDOM_GENERAL = (_R("d32", "fp16", 4, 4, 32, _MIX_SMALL, seed=65), _R("d96", "bf16", 4, 2, 96, _PF_MIX, bs=32, seed=66),
                  _R("window", "fp16", 8, 2, 128, ((1, 15, 111), (101, 15, 235)), causal=False, window=(7, 3), seed=67),
                  _R("softcap", "bf16", 4, 4, 64, ((90, 20, 1), (90, 33, 501)), softcap=30.0, seed=68),
                  _R("softcap-decode", "fp16", 8, 8, 128, ((1, 1, 1), (500, 31, 65)), softcap=30.0, seed=69))

GROUPS = {
    "per_head_decode": PER_HEAD_DECODE, "gqa_decode": GQA_DECODE, "alibi_decode": ALIBI_DECODE, "fused_decode": FUSED_DECODE,
    "prefill": PREFILL, "prefill_d256": PREFILL_D256, "general": GENERAL, "alibi_prefill": ALIBI_PREFILL, "dense": DENSE,
    "window": WINDOW, "random_decode": RANDOM_DECODE, "random_prefill": RANDOM_PREFILL, "random_general": RANDOM_GENERAL,
}
ALL_CASES = [(g, c) for g, cs in GROUPS.items() for c in cs]
assert len({c.name for _, c in ALL_CASES}) == len(ALL_CASES), "case names must be unique"

_cache = {}


def probe(case: Case) -> Probe:
    """build(case), memoised (the inputs are read-only: everything that changes them works on copies)."""
    if case.name not in _cache:
        _cache[case.name] = build(case)
    return _cache[case.name]
