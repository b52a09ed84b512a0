"""The sparse MoE block restated in pure torch on the CPU (no GPU): the router, the routed experts and the combine of
hydrainfer_amd/csrc/moe_experts.hip with exactly its rounding points, shared by tests/test_moe_block_cpu.py (which holds it
to the reference's DeepseekV3MoE and to the stored fixture, proves the pairing cases exact and the mutants refused),
tests/test_gpu_moe_experts.py and tests/test_gpu_moe_model.py.

ROUNDING POINTS (T = fp16 / bf16; hydrainfer/model/deepseek_v3.py:61-93, :114-155):
    logits = float(x) @ float(Wr)^T in fp32;  p = softmax (fp32);  top-k, ties to the lower index;
    w = p / (sum p + 1e-20) * scale  (norm_topk_prob and topk > 1)  or  p * scale                       (fp32)
    g = T(x_t . Wg_e[j]),  u = T(x_t . Wu_e[j])           (fp32 accumulation, one rounding: nn.Linear)
    a = T(silu(float(g)));  act = T(float(a) * float(u));  y = T(act . Wd_e[c])
    out = T( float(T( sum_k w_k * float(y_k) )) + float(shared) )      (fp32 products and sum, k order)
Three MODES of the same formulas:
    "T"      every op is the torch CPU op of the reference on T tensors (F.linear, F.silu, *, +): what the reference runs;
    "exact"  sums in float64, rounded to T at the points above: the value of ANY fp32 summation order as long as every
             partial sum is an fp32 number (the pairing cases, whose builder asserts that bound);
    "f64"    no rounding at all: the float64 value the tolerance tests measure against.

THE BLOCK FIXTURE (tests/golden/g15_moe_block.npz, written by tests/golden/generate_moe_block_golden.py): reference
outputs only; weights and inputs are regenerated here from seeds, the kept token rows come from the fixture.

PAIRING CASES.  x[t] is one-hot at a distinct k_t, every gate weight is 32 (silu(32) == 32 in fp32, fp16 and bf16), Wu_e
and Wd_e are independent grid values per expert, routing weights are powers of two, unrouted experts' weights are NaN."""
import functools
import os
from dataclasses import dataclass
from typing import Dict, List

import numpy as np
import torch
import torch.nn.functional as F

from tests import gemm_exact as G

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
TOL = {"bf16": 1e-2, "fp16": 1e-3}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_moe_block.npz")


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def route(x, wr, topk: int, norm_topk_prob: bool, scale: float, f64: bool = False):
    """(weights [n, topk], ids int32 [n, topk], scores [n, E]) — fp32 like the reference, or float64."""
    dt = torch.float64 if f64 else torch.float32
    logits = F.linear(x.to(dt), wr.to(dt))
    p = logits.softmax(dim=-1, dtype=dt)
    ids = torch.argsort(p, dim=-1, descending=True, stable=True)[:, :topk]
    w = p.gather(1, ids)
    if topk > 1 and norm_topk_prob:
        w = w / (w.sum(dim=-1, keepdim=True) + 1e-20) * scale
    else:
        w = w * scale
    return w, ids.to(torch.int32), p


def _linear(x, w, mode: str):
    if mode == "T":
        return F.linear(x, w)
    y = x.double() @ w.double().t()
    return y if mode == "f64" else y.to(x.dtype)


def _silu_mul(g, u, mode: str):
    if mode == "T":
        return F.silu(g) * u
    if mode == "f64":
        return F.silu(g) * u
    a = F.silu(g.float()).to(g.dtype)
    return (a.float() * u.float()).to(g.dtype)


def mlp(x, wgu, wdown, mode: str):
    """down(silu(gate(x)) * up(x)) with wgu = [gate rows; up rows]."""
    inter = wgu.shape[0] // 2
    return _linear(_silu_mul(_linear(x, wgu[:inter], mode), _linear(x, wgu[inter:], mode), mode), wdown, mode)


def expert_rows(x, ids, wgu, wdown, mode: str, expert_of=None, token_of=None):
    """y [n * topk, h] in slot order.  expert_of / token_of: the mutants' hooks (slot -> expert / token)."""
    n, topk = ids.shape
    flat = ids.reshape(-1).long()
    if expert_of is not None:
        flat = expert_of(flat)
    slots = torch.arange(n * topk)
    tok = slots // topk if token_of is None else token_of(slots)
    y = torch.zeros((n * topk, wdown.shape[1]), dtype=torch.float64 if mode == "f64" else x.dtype)
    for e in flat.unique().tolist():
        s = (flat == e).nonzero()[:, 0]
        y[s] = mlp(x[tok[s]], wgu[e], wdown[e], mode)
    return y


def combine(y, w, shared, mode: str):
    n, topk = w.shape
    if mode == "f64":
        out = (y.view(n, topk, -1) * w.double()[..., None]).sum(dim=1)
        return out if shared is None else out + shared.double()
    if mode == "T":
        out = y.view(n, topk, -1).type(w.dtype).mul_(w.unsqueeze(dim=-1)).sum(dim=1).type(y.dtype)
        return out if shared is None else out + shared
    acc = torch.zeros((n, y.shape[1]), dtype=torch.float32)
    yk = y.view(n, topk, -1).float()
    for k in range(topk):                                   # fp32 products, fp32 sum, k order
        acc = yk[:, k] * w[:, k:k + 1] if k == 0 else acc + yk[:, k] * w[:, k:k + 1]
    out = acc.to(y.dtype)
    return out if shared is None else (out.float() + shared.float()).to(y.dtype)


def block(x, wr, wgu, wdown, sgu, sdown, topk, norm_topk_prob, scale, mode: str, ids=None, w=None):
    """The whole MoE block.  ids / w given: the routing is taken, not recomputed (the float64 evaluation of a run)."""
    if ids is None:
        w, ids, _ = route(x, wr, topk, norm_topk_prob, scale, f64=mode == "f64")
    elif w is None:
        dt = torch.float64 if mode == "f64" else torch.float32
        p = F.linear(x.to(dt), wr.to(dt)).softmax(dim=-1, dtype=dt)
        w = p.gather(1, ids.long())
        w = w / (w.sum(dim=-1, keepdim=True) + 1e-20) * scale if (topk > 1 and norm_topk_prob) else w * scale
    xx = x.double() if mode == "f64" else x
    y = expert_rows(xx, ids, wgu, wdown, mode)
    shared = mlp(xx, sgu, sdown, mode) if sgu is not None else None
    return combine(y, w, shared, mode), ids, w


def ulp_distance(a, b) -> torch.Tensor:
    """Distance in units in the last place between two tensors of one two-byte type (sign-magnitude order)."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


# ---------------------------------------------------------------------------------------------------------------------
# the block fixture: config, seeded weights and inputs
# ---------------------------------------------------------------------------------------------------------------------
H, I, E, TOPK, N_SHARED = 256, 128, 8, 3, 2
N_VALUES = (1, 5, 64, 200)
SCALE = 1.0
MIN_GAP = 1e-3
STD_EXPERT, STD_ROUTER = 0.05, 0.2


def fixture_key(dt: str, norm: bool, n: int) -> str:
    return f"{dt}_norm{int(norm)}_n{n}"


@functools.lru_cache(maxsize=4)
def block_weights(dt: str) -> Dict[str, torch.Tensor]:
    """Reference-named state dict of one DeepseekV3MoE (prefix ''), in T: experts N(0, 0.05), router N(0, 0.2)."""
    T = DTYPES[dt]
    g = torch.Generator().manual_seed(1501)
    sd = {}
    for e in range(E):
        for name, shape in (("gate_proj", (I, H)), ("up_proj", (I, H)), ("down_proj", (H, I))):
            sd[f"experts.{e}.{name}.weight"] = (torch.randn(shape, generator=g) * STD_EXPERT).to(T)
    sd["gate.weight"] = (torch.randn((E, H), generator=g) * STD_ROUTER).to(T)
    for name, shape in (("gate_proj", (I * N_SHARED, H)), ("up_proj", (I * N_SHARED, H)), ("down_proj", (H, I * N_SHARED))):
        sd[f"shared_experts.{name}.weight"] = (torch.randn(shape, generator=g) * STD_EXPERT).to(T)
    return sd


def stacked(sd: Dict[str, torch.Tensor], prefix: str = ""):
    """(wr, wgu [E, 2I, h], wdown [E, h, I], sgu, sdown) from reference names."""
    n_e = 1 + max(int(k[len(prefix):].split(".")[1]) for k in sd if k.startswith(prefix + "experts."))
    p = lambda e, n: sd[f"{prefix}experts.{e}.{n}_proj.weight"]
    wgu = torch.stack([torch.cat([p(e, "gate"), p(e, "up")], dim=0) for e in range(n_e)])
    wdown = torch.stack([p(e, "down") for e in range(n_e)])
    s = lambda n: sd[f"{prefix}shared_experts.{n}_proj.weight"]
    return sd[prefix + "gate.weight"], wgu, wdown, torch.cat([s("gate"), s("up")], dim=0), s("down")


def candidate_tokens(dt: str, n: int) -> torch.Tensor:
    """The spare draw the kept rows are taken from: 2 n + 32 rows of N(0, 1) in T."""
    g = torch.Generator().manual_seed(1600 + n)
    return torch.randn((2 * n + 32, H), generator=g).to(DTYPES[dt])


@functools.lru_cache(maxsize=1)
def load_fixture():
    return dict(np.load(GOLDEN))


def from_bits(a: np.ndarray, dt: str) -> torch.Tensor:
    return torch.from_numpy(a.astype(np.int16)).view(DTYPES[dt])


def to_bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy()


@dataclass
class BlockCase:
    dt: str
    norm: bool
    n: int
    x: torch.Tensor             # [n, H] in T
    ref_out: torch.Tensor       # [n, H] in T: the reference's output
    ref_ids: torch.Tensor       # [n, TOPK] int32, the reference's order
    ref_ratio: float            # the reference's own error ratio against float64


def block_case(dt: str, norm: bool, n: int) -> BlockCase:
    fx, key = load_fixture(), fixture_key(dt, norm, n)
    x = candidate_tokens(dt, n)[torch.from_numpy(fx[key + "_keep"]).long()]
    return BlockCase(dt, norm, n, x, from_bits(fx[key + "_out"], dt), torch.from_numpy(fx[key + "_ids"]).to(torch.int32),
                     float(fx[key + "_ratio"]))


def error_ratio(out, y64, tol: float) -> float:
    return float(((out.double() - y64).abs() / (tol * (1 + y64.abs()))).max())


# ---------------------------------------------------------------------------------------------------------------------
# pairing cases
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class PairingCase:
    name: str
    n: int
    topk: int
    E: int
    h: int
    I: int
    routing: str          # "all": every expert once per token; "one": every token to one expert; "spread": seeded


PAIRING_CASES = (
    PairingCase("every-expert-one-row", 1, 8, 8, 128, 128, "all"),
    PairingCase("full-tile-one-expert", 64, 1, 8, 128, 128, "one"),
    PairingCase("two-experts-70-rows", 70, 2, 2, 640, 640, "all"),        # crosses the 64-row tile; two K chunks each
    PairingCase("odd-multiples-e72", 5, 6, 72, 1280, 896, "spread"),
    PairingCase("minimum-sizes", 33, 3, 8, 128, 128, "spread"),
    PairingCase("two-row-blocks", 20, 2, 4, 1152, 1152, "spread"),        # 17 .. 32 tokens: the 32-row tile, 1024-k down chunks
)
GATE_VALUE = 32.0
ROUTE_WEIGHTS = (0.5, 1.0, 2.0)


@dataclass
class Pairing:
    case: PairingCase
    x: torch.Tensor             # [n, h] fp32 holder, one-hot rows
    ids: torch.Tensor           # [n, topk] int32
    w: torch.Tensor             # [n, topk] fp32, powers of two
    wgu: torch.Tensor           # [E, 2I, h] fp32 holder; unrouted experts NaN
    wdown: torch.Tensor         # [E, h, I]
    shared: torch.Tensor        # [n, h] grid values
    routed: torch.Tensor        # bool [E]


@functools.lru_cache(maxsize=8)
def build_pairing(case: PairingCase) -> Pairing:
    n, topk, n_e, h, inter = case.n, case.topk, case.E, case.h, case.I
    assert n <= h, "one-hot rows need a distinct k per token"
    g = torch.Generator().manual_seed(7000 + 131 * n + 17 * topk + n_e)
    # the k that sit on the kernels' chunk borders first (512-k LDS chunks, 64-k column blocks, the last k)
    border = [k for k in dict.fromkeys((0, 63, 64, 511, 512, 1023, 1024, h - 1)) if k < h]
    ks = (border + [k for k in torch.randperm(h, generator=g).tolist() if k not in border])[:n]
    x = G.one_hot_rows(ks, h)
    if case.routing == "all":
        ids = torch.stack([torch.randperm(n_e, generator=g)[:topk] for _ in range(n)])
    elif case.routing == "one":
        ids = torch.full((n, topk), 5 % n_e)
    else:
        ids = torch.stack([torch.randperm(n_e, generator=g)[:topk] for _ in range(n)])
    ids = ids.to(torch.int32)
    w = torch.tensor(ROUTE_WEIGHTS)[torch.randint(0, len(ROUTE_WEIGHTS), (n, topk), generator=g)]
    routed = torch.zeros(n_e, dtype=torch.bool)
    routed[ids.reshape(-1).long()] = True
    wu = G.grid_values((n_e, inter, h), 11 + n_e)
    wgu = torch.cat([torch.full((n_e, inter, h), GATE_VALUE), wu], dim=1)
    wdown = G.grid_values((n_e, h, inter), 23 + n_e)
    wgu[~routed] = float("nan")
    wdown[~routed] = float("nan")
    shared = G.grid_values((n, h), 31 + n)
    # exactness, asserted: gate sums are one product; act = 32 u is a multiple of 8 with |act| <= 32 * 3.75, exact in both
    # types; a down sum of I products of quantum 8 * 1/4 stays an fp32 number; so does the combine's sum of topk terms
    amax, wmax = GATE_VALUE * G.LEVELS * G.STEP, G.LEVELS * G.STEP
    G.assert_exact(inter, amax, wmax, 8 * G.STEP)
    G.assert_exact(topk, inter * amax * wmax, max(ROUTE_WEIGHTS), 8 * G.STEP * min(ROUTE_WEIGHTS))
    return Pairing(case, x, ids, w, wgu, wdown, shared, routed)


def pairing_expected(p: Pairing, T, swap_k=False, next_expert=False, token_mod=False, shared=True) -> torch.Tensor:
    """out [n, h] in T from the "exact" restatement; the flags are the three mutants."""
    n, topk = p.ids.shape
    w = p.w
    if swap_k:
        if topk < 2:
            return None
        w = w.clone()
        w[:, [0, 1]] = w[:, [1, 0]]
    expert_of = (lambda flat: (flat + 1) % p.case.E) if next_expert else None
    token_of = (lambda s: s % n) if token_mod else None
    y = expert_rows(p.x.to(T), p.ids, p.wgu.to(T), p.wdown.to(T), "exact", expert_of, token_of)
    return combine(y, w, p.shared.to(T) if shared else None, "exact")


def silu_of_gate_is_exact() -> bool:
    """silu(32) == 32 in fp32 (and so in both two-byte types): 1 + exp(-32) rounds to 1."""
    v = torch.tensor([GATE_VALUE])
    return bool(F.silu(v) == v) and all(bool(F.silu(v.to(T)) == v.to(T)) for T in DTYPES.values())


# ---------------------------------------------------------------------------------------------------------------------
# the tiny MoE model on the CPU: the oracle's attention composed with the "T" restatement of the block
# ---------------------------------------------------------------------------------------------------------------------
def oracle_moe_model(shape, sd, dtype, drop_routed: bool = False):
    """oracle.model.OracleLlama whose layers >= shape.first_k_dense_replace run block(..., "T") as their MLP
    (deepseek_v3.py:191).  .gaps collects, per sparse MLP call, the smallest difference between a row's k-th and
    (k+1)-th router score; drop_routed zeroes the routed experts' term (what a test must be able to see)."""
    import oracle.ops as ops
    from oracle.model import OracleLlama

    class OracleMoeLlama(OracleLlama):
        gaps: List[float] = []

        def layer(self, l, h, position_ids, meta, key_cache, value_cache, select):
            sh = self.shape
            if l < sh.first_k_dense_replace:
                return super().layer(l, h, position_ids, meta, key_cache, value_cache, select)
            p = f"model.layers.{l}."
            H, HK, D = sh.num_attention_heads, sh.num_key_value_heads, sh.head_dim
            x = ops.rms_norm_torch(h, sd[p + "input_layernorm.weight"], sh.rms_norm_eps)
            q = F.linear(x, sd[p + "self_attn.q_proj.weight"]).view(-1, H, D)
            k = F.linear(x, sd[p + "self_attn.k_proj.weight"]).view(-1, HK, D)
            v = F.linear(x, sd[p + "self_attn.v_proj.weight"]).view(-1, HK, D)
            q, k = ops.apply_rotary_pos_emb(q, k, position_ids, self.cos_sin, D, False)
            ops.set_kv_cache(meta.new_cache_slots, k, v, key_cache, value_cache)
            o = ops.paged_attention(q, key_cache, value_cache, meta.q_cu_seq_lens, meta.kv_cu_seq_lens,
                                    meta.block_tables, meta.cu_blocks_lens)
            h = h + F.linear(o.reshape(-1, H * D), sd[p + "self_attn.o_proj.weight"])
            if select is not None and l == sh.num_hidden_layers - 1:
                h = h[select]
            x = ops.rms_norm_torch(h, sd[p + "post_attention_layernorm.weight"], sh.rms_norm_eps)
            wr, wgu, wdown, sgu, sdown = stacked(sd, p + "mlp.")
            _, _, scores = route(x, wr, sh.num_experts_per_tok, sh.norm_topk_prob, sh.routed_scaling_factor)
            top = scores.sort(dim=-1, descending=True).values
            self.gaps.append(float((top[:, sh.num_experts_per_tok - 1] - top[:, sh.num_experts_per_tok]).min()))
            if drop_routed:
                return h + mlp(x, sgu, sdown, "T")
            m, _, _ = block(x, wr, wgu, wdown, sgu, sdown, sh.num_experts_per_tok, sh.norm_topk_prob,
                            sh.routed_scaling_factor, "T")
            return h + m

    model = OracleMoeLlama(shape, sd, dtype)
    model.gaps = []
    return model
