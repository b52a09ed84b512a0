"""Helpers of tests/test_decode_arms_cpu.py and tests/test_gpu_decode_arms.py: the launch sequences ("arms") that
LlamaForCausalLM._decode_hidden_hip_gemm can choose, as data; one all-decode step built for the HIP model and for
oracle.model.OracleLlama from the same tensors; a spy on the launch wrappers; and oracle mutants, each wrong in one way
a mis-assembled layer would be wrong.

Every model here has three layers (layer 0: qkv from row-major x on the LDS-slice kernel; a middle layer; the last
layer: no next qkv, the final norm written row-major), head_dim 128, H = HK = hidden / 128, vocab 2048, random_init's
default std.  The norm weights are 1 + 0.1 * randn instead of random_init's ones: with ones, a launch that takes the
wrong layer's norm weight computes the right answer."""
import contextlib
import functools
import inspect
import re
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from oracle import ops
from oracle.model import OracleAttnMeta, OracleLlama

BS, HEAD_DIM, LAYERS, VOCAB = 16, 128, 3, 2048
MAX_CTX = 49
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}

# (hidden, inter, heads): the smallest shapes (multiples of 256) that reach each branch of the plan, found through the
# host planning queries (256 CUs are assumed without a device) — tests/test_decode_arms_cpu.py re-derives every row
SHAPES = {"A": (256, 256, 2), "B": (2048, 256, 16), "C": (2304, 256, 18), "D": (256, 3584, 2), "E": (3840, 256, 30)}

LOW_ROWS, HIGH_ROWS, GENERIC_ROWS = (1, 16, 17, 32), (33, 48, 64), 65


@dataclass(frozen=True)
class Switches:
    """The A/B switches of LlamaForCausalLM (set as attributes before prepare_decode)."""
    use_packed: bool = True
    use_xreg: bool = True
    xreg_qkv: bool = True
    fuse_norm: bool = True
    use_wide: bool = True
    use_wide_silu: bool = True

    def apply(self, model) -> None:
        for k, v in self.__dict__.items():
            assert hasattr(model, k), k
            setattr(model, k, v)


def P(xreg=0, fused=0, nf_gu=0, nf_qkv=0, wide=0, wide_silu=0) -> dict:
    """A _decode_plan dict."""
    return {"xreg": bool(xreg), "fused": bool(fused), "nf_gu": bool(nf_gu), "nf_qkv": bool(nf_qkv), "wide": bool(wide),
            "wide_silu": bool(wide_silu)}


# ---------------------------------------------------------------------------------------------------------------------
# launch sequences.  A name is the wrapper as _decode_hidden_hip_gemm calls it; ":fm" marks a call whose activation
# argument is fragment-major (frag_shape= of a GEMM, fragment_major=True of a slab consumer) — that is what tells
# layer 0, a middle layer and the last layer apart where the wrappers are the same.  A qkv GEMM belongs to the layer
# whose attention reads it, except the norm-fused one, which is the last launch of the layer before.
# ---------------------------------------------------------------------------------------------------------------------
ATT, EX, EXF = "decode_attention_fused", "linear_decode_ex", "linear_decode_ex:fm"
RM, LPX = "linear_decode_partial", "linear_decode_partial_xreg:fm"
NORM, NORMF = "add_rms_norm_slabs", "add_rms_norm_slabs:fm"
SILU, SILUF = "silu_and_mul_slabs", "silu_and_mul_slabs:fm"
NLX, NGUS, NGU, NGUSW = "norm_linear_decode_xreg", "norm_gate_up_silu_xreg", "norm_gate_up_xreg", "norm_gate_up_silu_wide_xreg"
GUS, GU = "gate_up_silu_xreg:fm", "gate_up_xreg:fm"


def _three(first_qkv, mid_qkv, body, handover, last):
    """[layer 0, layer 1, layer 2]: qkv launch (None: it came from the layer before), the body, the closing launch."""
    q = lambda x: [x] if x else []
    return [q(first_qkv) + body + [handover], q(mid_qkv) + body + [handover], q(mid_qkv) + body + [last]]


SEQUENCES: Dict[str, List[List[str]]] = {
    # eight launches on LDS-slice GEMMs; the same on row-major weights (use_packed=False)
    "lds8": _three(EX, EX, [ATT, EX, NORM, EX, SILU, EX], NORM, NORM),
    "rowmajor8": _three(RM, RM, [ATT, RM, NORM, RM, SILU, RM], NORM, NORM),
    # <= 32 rows, the MLP on the activations-in-registers kernel
    "xreg7": _three(EX, EXF, [ATT, EX, NORMF, GUS, EXF], NORMF, NORM),
    "xreg5": _three(EX, None, [ATT, EX, NGUS, EXF], NLX, NORM),
    "xreg6_gu": _three(EX, EXF, [ATT, EX, NGUS, EXF], NORMF, NORM),              # nf_gu without nf_qkv
    "xreg6_gu_lds_qkv": _three(EX, EX, [ATT, EX, NGUS, EXF], NORM, NORM),        # xreg_qkv=False: qkv stays on LDS-slice
    "xreg7_lds_qkv": _three(EX, EX, [ATT, EX, NORMF, GUS, EXF], NORM, NORM),     # ... and fuse_norm=False
    "xreg8_silu": _three(EX, EXF, [ATT, EX, NORMF, LPX, SILUF, EXF], NORMF, NORM),   # gate_up_silu unsupported
    # 33 .. 64 rows, the wide kernel
    "wide6": _three(EX, None, [ATT, EX, NGU, SILUF, LPX], NLX, NORM),
    "wide5": _three(EX, None, [ATT, EX, NGUSW, LPX], NLX, NORM),
    "wide7_gu": _three(EX, LPX, [ATT, EX, NGU, SILUF, LPX], NORMF, NORM),
    "wide8": _three(EX, LPX, [ATT, EX, NORMF, GU, SILUF, LPX], NORMF, NORM),
    # ... over a gate|up packing with its halves in order (no silu epilogue at 32 rows: hx_gate_up_xreg would read it as
    # interleaved and scramble the columns — the bug this file found on shape C): the plain wide product
    "wide8_plain_gu": _three(EX, LPX, [ATT, EX, NORMF, LPX, SILUF, LPX], NORMF, NORM),
    # more than 64 rows: the generic loop (library GEMMs are not launches of this library)
    "generic": [[ATT, "add_rms_norm", "silu_and_mul", "add_rms_norm"]] * 3,
}
PLAN_OF = {"lds8": P(), "rowmajor8": P(), "xreg7": P(1, 1), "xreg5": P(1, 1, 1, 1), "xreg6_gu": P(1, 1, 1),
           "xreg6_gu_lds_qkv": P(1, 1, 1), "xreg7_lds_qkv": P(1, 1), "xreg8_silu": P(1), "wide6": P(1, 0, 1, 1, 1),
           "wide5": P(1, 0, 1, 1, 1, 1), "wide7_gu": P(1, 0, 1, 0, 1), "wide8": P(1, 0, 0, 0, 1), "wide8_plain_gu": P(1, 0, 0, 0, 1)}


@dataclass(frozen=True)
class Arm:
    name: str
    shape: str
    sw: Switches
    low: Optional[str]          # the family (key of SEQUENCES / PLAN_OF) at 1 / 16 / 17 / 32 rows; None: not run
    high: Optional[str]         # ... at 33 / 48 / 64 rows
    generic: bool = False       # also runs the 65-row case (once per shape)

    def family(self, n: int) -> Optional[str]:
        return "generic" if n > 64 else self.high if n > 32 else self.low

    def rows(self) -> Tuple[int, ...]:
        return ((LOW_ROWS if self.low else ()) + (HIGH_ROWS if self.high else ())
                + ((GENERIC_ROWS,) if self.generic else ()))


S = Switches()
ARMS: List[Arm] = [
    Arm("A", "A", S, "xreg5", "wide6", generic=True),
    Arm("B", "B", S, "xreg6_gu", "wide7_gu", generic=True),
    Arm("C", "C", S, "xreg8_silu", "wide8_plain_gu", generic=True),
    Arm("D", "D", S, "xreg5", "lds8", generic=True),
    Arm("E", "E", S, "xreg5", "wide5", generic=True),
    Arm("A-no_fuse_norm", "A", replace(S, fuse_norm=False), "xreg7", "wide8"),
    Arm("E-no_fuse_norm", "E", replace(S, fuse_norm=False), "xreg7", "wide8"),
    Arm("B-no_fuse_norm", "B", replace(S, fuse_norm=False), "xreg7", "wide8"),
    Arm("A-no_wide", "A", replace(S, use_wide=False), None, "lds8"),         # <= 32 rows: the switch is not read
    Arm("E-no_wide", "E", replace(S, use_wide=False), None, "lds8"),
    Arm("E-no_wide_silu", "E", replace(S, use_wide_silu=False), None, "wide6"),
    Arm("A-no_xreg_qkv", "A", replace(S, xreg_qkv=False), "xreg6_gu_lds_qkv", "lds8"),
    Arm("E-no_xreg_qkv", "E", replace(S, xreg_qkv=False), "xreg6_gu_lds_qkv", "lds8"),
    Arm("A-no_xreg_qkv-no_fuse_norm", "A", replace(S, xreg_qkv=False, fuse_norm=False), "xreg7_lds_qkv", None),
    Arm("A-no_xreg", "A", replace(S, use_xreg=False), "lds8", "lds8"),
    Arm("E-no_xreg", "E", replace(S, use_xreg=False), "lds8", "lds8"),
    Arm("A-no_packed", "A", replace(S, use_packed=False), "rowmajor8", "rowmajor8"),
    Arm("E-no_packed", "E", replace(S, use_packed=False), "rowmajor8", "rowmajor8"),
]
ARM = {a.name: a for a in ARMS}

# arms that differ only by fusions proven bit-identical at operator level (tests/test_gpu_ops.py): (arm, its twin, rows)
FAMILIES_BIT_IDENTICAL = [("A", "A-no_fuse_norm", LOW_ROWS + HIGH_ROWS), ("E", "E-no_fuse_norm", LOW_ROWS + HIGH_ROWS),
                          ("E", "E-no_wide_silu", HIGH_ROWS), ("B", "B-no_fuse_norm", LOW_ROWS + HIGH_ROWS)]


def llama_shape(key: str):
    from hydrainfer_amd.model.llama import LlamaShape
    hid, inter, heads = SHAPES[key]
    return LlamaShape(hid, inter, LAYERS, heads, heads, HEAD_DIM, VOCAB)


def host_plan(shape_key: str, sw: Switches, n: int) -> Optional[dict]:
    """LlamaForCausalLM._decode_plan after prepare_decode(64), restated on the host planning queries alone (no device,
    no weights): what the table of ARMS was derived with.  The GPU tests hold model._decode_plan to the same table."""
    from hydrainfer_amd import _lib
    l = _lib.lib()
    hid, inter, _ = SHAPES[shape_key]
    qkv_n = 3 * hid
    if n > 64:
        return None
    xs = lambda m, N, K: l.hx_linear_decode_xreg_supported(m, N, K) == 1
    mlp32 = lambda m: xs(m, 2 * inter, hid) and xs(m, hid, inter)
    mlp_packed = sw.use_packed and sw.use_xreg and mlp32(32)                  # l*.wgu / l*.wdown in packed_x
    qkv_packed = mlp_packed and sw.xreg_qkv and xs(32, qkv_n, hid)            # l>=1.wqkv in packed_x
    interleaved = l.hx_gate_up_silu_xreg_supported(32, inter, hid) == 1      # how hx_decode_weight_plan packs gate|up
    gu_wide = l.hx_gate_up_xreg_supported(n, inter, hid, 0) == 1 if interleaved else xs(n, 2 * inter, hid)
    wide_ok = (32 < n <= 64 and sw.use_wide and sw.use_xreg and sw.xreg_qkv and mlp32(32)
               and gu_wide and xs(n, hid, inter) and xs(n, qkv_n, hid)
               and xs(32, qkv_n, hid))
    xreg = bool(sw.use_xreg and (wide_ok if n > 32 else mlp32(n)) and mlp_packed)
    wide = bool(xreg and n > 32)
    fused = bool(xreg and not wide and l.hx_gate_up_silu_xreg_supported(n, inter, hid) == 1)
    if wide:
        nf_gu = bool(sw.fuse_norm and interleaved and l.hx_gate_up_xreg_supported(n, inter, hid, 1) == 1)
    else:
        nf_gu = bool(xreg and sw.fuse_norm and fused and l.hx_norm_xreg_supported(n, 2 * inter, hid, 1) == 1)
    nf_qkv = bool(xreg and sw.fuse_norm and qkv_packed and l.hx_norm_xreg_supported(n, qkv_n, hid, 0) == 1)
    wide_silu = bool(wide and nf_gu and sw.use_wide_silu and l.hx_gate_up_silu_wide_xreg_supported(n, inter, hid) == 1)
    return {"xreg": xreg, "fused": fused, "nf_gu": nf_gu, "nf_qkv": nf_qkv, "wide": wide, "wide_silu": wide_silu}


def host_qkv_packed(shape_key: str, sw: Switches) -> bool:
    """Whether qkv of layers >= 1 gets the activations-in-registers packing (decides ":fm" of the qkv launch)."""
    from hydrainfer_amd import _lib
    l = _lib.lib()
    hid, inter, _ = SHAPES[shape_key]
    xs = lambda m, N, K: l.hx_linear_decode_xreg_supported(m, N, K) == 1
    return bool(sw.use_packed and sw.use_xreg and xs(32, 2 * inter, hid) and xs(32, hid, inter) and sw.xreg_qkv
                and xs(32, 3 * hid, hid))


# ---------------------------------------------------------------------------------------------------------------------
# weights and one decode step
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def weights(shape_key: str, dname: str) -> Dict[str, Tensor]:
    """The fused state dict (CPU, model dtype) of the shape's model: random_init(seed 0) on the CPU generator, so a
    machine without a GPU draws the same weights; norm weights 1 + 0.1 * randn."""
    from hydrainfer_amd.model.llama import LlamaForCausalLM
    dt = DTYPES[dname]
    m = LlamaForCausalLM.random_init(llama_shape(shape_key), dt, "cpu", seed=0)
    g = torch.Generator().manual_seed(1)
    for k in sorted(m.state):
        if k.endswith(("norm", "norm1", "norm2")):
            m.state[k] = (1.0 + 0.1 * torch.randn(m.state[k].shape, generator=g)).to(dt)
    return m.state


@functools.lru_cache(maxsize=2)
def reference_state_dict(shape_key: str, dname: str, T: torch.dtype) -> Dict[str, Tensor]:
    """The same weights under the reference's parameter names, cast to T."""
    from hydrainfer_amd.model.llama import LlamaForCausalLM
    dt = DTYPES[dname]
    sd = LlamaForCausalLM(llama_shape(shape_key), dt, "cpu", weights(shape_key, dname)).to_reference_state_dict()
    return {k: v.to(T) for k, v in sd.items()}


@dataclass
class Case:
    shape: str
    dname: str
    n: int
    ids: Tensor                 # int64 [n]
    ctx: List[int]              # keys per request AFTER the step
    tables: List[List[int]]     # physical blocks per request
    pool: Tensor                # [3, 2, n_blocks, 16, H, 128] in the model dtype (the input pool; never written)

    @property
    def positions(self) -> Tensor:
        return torch.tensor([c - 1 for c in self.ctx], dtype=torch.int32)

    @property
    def slots(self) -> Tensor:
        return torch.tensor([t[(c - 1) // BS] * BS + (c - 1) % BS for c, t in zip(self.ctx, self.tables)], dtype=torch.int32)

    def meta(self) -> OracleAttnMeta:
        i32 = lambda x: torch.tensor(x, dtype=torch.int32)
        cu = lambda xs: [sum(xs[:i]) for i in range(len(xs) + 1)]
        return OracleAttnMeta(i32(list(range(self.n + 1))), i32(cu(self.ctx)), self.slots,
                              i32([b for t in self.tables for b in t]), i32(cu([len(t) for t in self.tables])))

    def permuted(self, perm: List[int]) -> "Case":
        """The same requests in another order (row r of the result is row perm[r] of this case); the pool is shared."""
        return replace(self, ids=self.ids[perm], ctx=[self.ctx[p] for p in perm], tables=[self.tables[p] for p in perm])


def case(shape_key: str, n: int, dname: str, seed: int = 0) -> Case:
    """One all-decode step of n requests from one torch generator: token ids; ragged contexts of 1 .. 49 keys after the
    step, among them 17 (the token lands in the first slot of a fresh block), 16 (the last slot of a block) and 1
    (position 0) as far as n allows, in shuffled order; block tables of block size 16 drawn from a shuffled list of
    physical blocks (non-monotonic) that leaves three pages unreferenced; a randn pool."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    heads = SHAPES[shape_key][2]
    ids = torch.randint(0, VOCAB, (n,), generator=g)
    ctx = ([17, 16, 1] + torch.randint(1, MAX_CTX + 1, (max(n - 3, 0),), generator=g).tolist())[:n]
    ctx = [ctx[i] for i in torch.randperm(n, generator=g).tolist()]
    need = [(c + BS - 1) // BS for c in ctx]
    n_blocks = sum(need) + 3
    phys = torch.randperm(n_blocks, generator=g).tolist()
    tables, off = [], 0
    for k in need:
        tables.append(phys[off: off + k])
        off += k
    pool = torch.randn((LAYERS, 2, n_blocks, BS, heads, HEAD_DIM), generator=g).to(DTYPES[dname])
    return Case(shape_key, dname, n, ids, ctx, tables, pool)


def written_rows(c: Case, pool: Tensor) -> Tensor:
    """[3, 2, n, H, 128]: the cache rows the step writes."""
    return pool.reshape(LAYERS, 2, -1, *pool.shape[4:])[:, :, c.slots.long()]


def reference(c: Case, T: torch.dtype, cls=OracleLlama) -> Tuple[Tensor, Tensor, Tensor]:
    """(logits fp32 [n, vocab], written KV rows fp32 [3, 2, n, H, 128], final pool in T) of the oracle (or a mutant of
    it) with weights and pool cast to T: the model dtype for the project's oracle, torch.float32 for the high-precision
    reference."""
    sd = reference_state_dict(c.shape, c.dname, T)
    pool = c.pool.to(T, copy=True)
    with torch.inference_mode():
        o = cls(llama_shape(c.shape), sd, T)
        logits = o.forward_logits(c.ids, c.positions, c.meta(), [(pool[l, 0], pool[l, 1]) for l in range(LAYERS)]).float()
    return logits, written_rows(c, pool).float(), pool


# how far the HIP path may be from the fp32 reference, in units of the T oracle's own distance E_T from it: the HIP path
# rounds where the T oracle rounds or at fewer points, so its distance should be about E_T; the factor covers the noise
# of a maximum over n x 2048 values (logits) / n x 3 x 2 x hidden (KV rows)
BAR_FACTOR = {"fp16": 4.0, "bf16": 4.0}
MUTANT_MARGIN = 10.0        # every kept mutant misses the fp32 reference by more than this x the bar


# ---------------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------------
class HookedOracle(OracleLlama):
    """OracleLlama.layer restated with one hook per hand-over of the HIP layer.  Without an override it is the oracle,
    bit for bit (tests/test_decode_arms_cpu.py::test_hooked_oracle_is_the_oracle)."""
    MUTATED_LAYER = 1

    def attn_in(self, l, x):
        return x

    def mlp_in(self, l, x):
        return x

    def mlp_residual(self, l, h, m):
        return h + m

    def key_slots(self, l, meta, position_ids):
        return meta.new_cache_slots

    def final_norm_weight(self):
        return self.sd["model.norm.weight"]

    def layer(self, l, h, position_ids, meta, key_cache, value_cache, select):
        import torch.nn.functional as F
        sh, sd = self.shape, self.sd
        p = f"model.layers.{l}."
        H, HK, D = sh.num_attention_heads, sh.num_key_value_heads, sh.head_dim
        x = self.attn_in(l, ops.rms_norm_torch(h, sd[p + "input_layernorm.weight"], sh.rms_norm_eps))
        q = F.linear(x, sd[p + "self_attn.q_proj.weight"]).view(-1, H, D)
        k = F.linear(x, sd[p + "self_attn.k_proj.weight"]).view(-1, HK, D)
        v = F.linear(x, sd[p + "self_attn.v_proj.weight"]).view(-1, HK, D)
        q, k = ops.apply_rotary_pos_emb(q, k, position_ids, self.cos_sin, D, False)
        ks = self.key_slots(l, meta, position_ids)
        if ks is meta.new_cache_slots:
            ops.set_kv_cache(ks, k, v, key_cache, value_cache)
        else:
            ops.set_kv_cache(ks, k, v, key_cache, value_cache.clone())
            ops.set_kv_cache(meta.new_cache_slots, k, v, key_cache.clone(), value_cache)
        o = ops.paged_attention(q, key_cache, value_cache, meta.q_cu_seq_lens, meta.kv_cu_seq_lens,
                                meta.block_tables, meta.cu_blocks_lens)
        h = h + F.linear(o.reshape(-1, H * D), sd[p + "self_attn.o_proj.weight"])
        x = self.mlp_in(l, ops.rms_norm_torch(h, sd[p + "post_attention_layernorm.weight"], sh.rms_norm_eps))
        m = F.linear(ops.silu(F.linear(x, sd[p + "mlp.gate_proj.weight"])) *
                     F.linear(x, sd[p + "mlp.up_proj.weight"]), sd[p + "mlp.down_proj.weight"])
        return self.mlp_residual(l, h, m)

    def forward_hidden(self, input_ids_or_embeds, position_ids, meta, caches, select=None):
        import torch.nn.functional as F
        h = input_ids_or_embeds
        if h.dtype in (torch.int32, torch.int64):
            h = F.embedding(h.long(), self.sd["model.embed_tokens.weight"])
        for l in range(self.n_layers):
            h = self.layer(l, h, position_ids, meta, caches[l][0], caches[l][1], select)
        return ops.rms_norm_torch(h, self.final_norm_weight(), self.shape.rms_norm_eps)


class StaleHandover(HookedOracle):
    """The last row's qkv input of the middle layer is the x the layer before handed over (a stale xf)."""
    def attn_in(self, l, x):
        if l == self.MUTATED_LAYER:
            x = x.clone()
            x[-1] = self._prev[-1]
        self._prev = x
        return x


class SwappedRows(HookedOracle):
    """Rows 16 and 17 of the middle layer's MLP input swapped (a fragment-major row mix-up across a 16-row block)."""
    MIN_ROWS = 18

    def mlp_in(self, l, x):
        if l == self.MUTATED_LAYER:
            x = x.clone()
            x[[16, 17]] = x[[17, 16]]
        return x


class SkippedResidual(HookedOracle):
    """The middle layer's MLP residual add skipped for the last row."""
    def mlp_residual(self, l, h, m):
        out = h + m
        if l == self.MUTATED_LAYER:
            out[-1] = h[-1]
        return out


class WrongFinalNorm(HookedOracle):
    """The final norm applied with layer 0's first norm weight (the last layer took `nxt` of the wrong layer)."""
    def final_norm_weight(self):
        return self.sd["model.layers.0.input_layernorm.weight"]


class KeyOneSlotEarly(HookedOracle):
    """The middle layer's new K written to the slot of position - 1 (rows at position 0 have none: left alone)."""
    def key_slots(self, l, meta, position_ids):
        if l != self.MUTATED_LAYER:
            return meta.new_cache_slots
        out = meta.new_cache_slots.clone()
        for r in range(out.numel()):
            pos = int(position_ids[r]) - 1
            if pos >= 0:
                table = meta.block_tables[int(meta.cu_blocks_lens[r]): int(meta.cu_blocks_lens[r + 1])]
                out[r] = int(table[pos // BS]) * BS + pos % BS
        return out


MUTANTS = [StaleHandover, SwappedRows, SkippedResidual, WrongFinalNorm, KeyOneSlotEarly]

# Where a mutant is NOT caught at more than MUTANT_MARGIN x the bar (by the logits or by the written KV rows) it is
# dropped, never kept as a passing case.  All of these are bf16: its E_T is 8 x fp16's, the bar with it, and a fault in
# one row of one layer moves the logits by the same absolute amount in both dtypes.  Measured margins (miss / bar, the
# larger of logits and KV rows, over n = 1, 17, 33, 64):
#   fp16: every mutant at every shape > 21 (kept everywhere).
#   bf16 StaleHandover 21 .. 57, KeyOneSlotEarly 27 .. 130: kept everywhere.
#   bf16 SwappedRows: D 18 .. 19 (kept); A 7 .. 10, B 13 .. 14, C 13 .. 14, E 13 .. 17 (dropped: E_T is a maximum of
#   rounding errors of the CPU's half-precision products and may move with their summation order; a margin within
#   1.7 x of the threshold is not kept as if it were certain).
#   bf16 SkippedResidual: A 4 .. 7, B 2.5 .. 10, C 3 .. 12, D 12 .. 19, E 3 .. 10 (dropped).
#   bf16 WrongFinalNorm: 2 .. 8 at every shape (dropped) — the final norm leaves no trace in the KV rows, and the norm
#   weights are 1 + 0.1 * randn.
# In bf16 those faults are left to the bit-identity checks of the GPU file (row order, the three feeds, the twins) and
# to the fp16 run of the same arm, which takes the same launches.
DROPPED: Dict[Tuple[str, str], Tuple[str, ...]] = {
    ("SwappedRows", "bf16"): ("A", "B", "C", "E"),
    ("SkippedResidual", "bf16"): ("A", "B", "C", "D", "E"),
    ("WrongFinalNorm", "bf16"): ("A", "B", "C", "D", "E"),
}


def mutant_applies(cls, c: Case) -> bool:
    if c.n < getattr(cls, "MIN_ROWS", 1):
        return False          # rows 16 and 17 do not exist
    if cls is KeyOneSlotEarly and max(c.ctx) == 1:
        return False
    return c.shape not in DROPPED.get((cls.__name__, c.dname), ())


# ---------------------------------------------------------------------------------------------------------------------
# the spy
# ---------------------------------------------------------------------------------------------------------------------
GEMM_WRAPPERS = ("linear_decode", "linear_decode_partial", "linear_decode_partial_packed", "linear_decode_partial_xreg",
                 "gate_up_silu_xreg", "norm_linear_decode_xreg", "norm_gate_up_silu_xreg", "gate_up_xreg",
                 "norm_gate_up_xreg", "norm_gate_up_silu_wide_xreg", "linear_decode_ex")
PLAIN_GEMMS = ("linear_decode", "linear_decode_partial", "linear_decode_partial_packed", "linear_decode_partial_xreg",
               "linear_decode_ex")
LLAMA_WRAPPERS = ("add_rms_norm_slabs", "silu_and_mul_slabs", "decode_attention_fused", "rms_norm", "decode_step_head",
                  "add_rms_norm", "silu_and_mul")
HEAD_NAMES = ("decode_step_head", "rms_norm", "memset_zero")
HEAD = -1                   # the "layer" of the launches in front of layer 0


class Spied(list):
    """The ordered (name, layer) list; .tensors[i] holds clones of call i's tensor arguments and result when the spy
    was asked to keep them."""
    def __init__(self):
        super().__init__()
        self.tensors: List[dict] = []

    def layer(self, l: int) -> List[str]:
        return [n for n, k in self if k == l]

    def names(self) -> set:
        return {n.split(":")[0] for n, _ in self}


@contextlib.contextmanager
def spy(keep_tensors: bool = False, max_elems: int = 1 << 22, stubs: Optional[dict] = None):
    """Wraps, for the duration of the block, the names the decode layer (_decode_hidden_hip_gemm, its _stage_* functions
    and forward_hidden) calls through hydrainfer_amd.model.llama: every launch wrapper of hip_gemm, add_rms_norm_slabs,
    silu_and_mul_slabs, decode_attention_fused, rms_norm, decode_step_head (and the generic loop's add_rms_norm,
    silu_and_mul), and _lib.memset_zero.  Yields the list of (name, layer) seen so far; no hook in product code.
    stubs: {name: function} called in place of the wrapper of that name (a dry run without a device: dry_stubs())."""
    from hydrainfer_amd import _lib
    from hydrainfer_amd.model import llama
    seen = Spied()
    state = {"layer": 0, "attn": 0}
    saved = []

    def wrap(owner, attr):
        orig = getattr(owner, attr)
        call = orig if stubs is None else stubs[attr]

        @functools.wraps(orig)
        def f(*a, **k):
            name = attr
            if k.get("frag_shape") is not None or k.get("fragment_major"):
                name += ":fm"
            if attr == "decode_attention_fused":
                if state["attn"]:
                    state["layer"] += 1
                state["attn"] += 1
                # the qkv GEMM right in front of an attention launch is that layer's
                if seen and seen[-1][0].split(":")[0] in PLAIN_GEMMS and seen[-1][1] != HEAD:
                    seen[-1] = (seen[-1][0], state["layer"])
            idx = len(seen)
            seen.append((name, HEAD if attr in HEAD_NAMES else state["layer"]))
            out = call(*a, **k)
            if keep_tensors:
                grab = lambda t: t.detach().clone() if isinstance(t, Tensor) and t.numel() <= max_elems else None
                seen.tensors.append({"args": [grab(t) for t in a], "kwargs": {n: grab(t) for n, t in k.items()},
                                     "out": grab(out)})
                assert len(seen.tensors) == idx + 1
            return out
        saved.append((owner, attr, orig))
        setattr(owner, attr, f)

    try:
        for n in GEMM_WRAPPERS:
            wrap(llama.hip_gemm, n)
        for n in LLAMA_WRAPPERS:
            wrap(llama, n)
        wrap(_lib, "memset_zero")
        yield seen
    finally:
        for owner, attr, orig in reversed(saved):
            setattr(owner, attr, orig)


def dry_stubs() -> dict:
    """A stub for every name the spy wraps that touches nothing and returns a value of the wrapper's kind: a slab count
    for the GEMMs that return one, an empty tensor of the result's shape for silu_and_mul_slabs (the only result the
    layer passes on as a tensor; fragment-major: flat, rows padded to 16), None for the rest."""
    def silu(partial, n_splits, rows, inter, dtype, fragment_major=False):
        return torch.empty((rows + 15) // 16 * 16 * inter if fragment_major else (rows, inter), dtype=dtype)
    counted = set(PLAIN_GEMMS) - {"linear_decode"} | {"norm_linear_decode_xreg", "gate_up_xreg", "norm_gate_up_xreg"}
    stubs = {n: (lambda *a, **k: 2) if n in counted else (lambda *a, **k: None)
             for n in GEMM_WRAPPERS + LLAMA_WRAPPERS + ("memset_zero",)}
    stubs["silu_and_mul_slabs"] = silu
    return stubs


def decode_layer_functions() -> list:
    """The functions that make up the decode layer: the body, one function per stage, and _partial."""
    from hydrainfer_amd.model.llama import LlamaForCausalLM as M
    return [M._decode_hidden_hip_gemm, M._stage_qkv, M._stage_attention_o, M._stage_mlp_in, M._stage_down, M._stage_close,
            M._partial]


def call_sites() -> set:
    """Every launch wrapper named in the source of the decode layer: hip_gemm.<name>( that is not a host planning query,
    plus the four non-GEMM wrappers."""
    src = "".join(inspect.getsource(f) for f in decode_layer_functions())
    names = {n for n in re.findall(r"hip_gemm\.(\w+)\(", src)
             if not n.endswith(("_supported", "_floats", "_elems"))}
    for n in ("add_rms_norm_slabs", "silu_and_mul_slabs", "decode_attention_fused", "rms_norm"):
        assert re.search(rf"\b{n}\(", src), n
        names.add(n)
    return names


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
def build_model(shape_key: str, dname: str, sw: Switches, device):
    """The HIP model on the shape's weights with the switches set as attributes, decode layouts for <= 64 rows built."""
    from hydrainfer_amd.model.llama import LlamaForCausalLM
    dt = DTYPES[dname]
    state = {k: v.to(device) for k, v in weights(shape_key, dname).items()}
    model = LlamaForCausalLM(llama_shape(shape_key), dt, device, state)
    sw.apply(model)
    model.prepare_decode(max_rows=64)
    return model


def device_step(model, c: Case, device, pool_d: Tensor, feed: str = "int64", keep_tensors: bool = False,
                stubs: Optional[dict] = None):
    """Runs the case's step on the HIP model over pool_d (the case's pool on the device: written in place).  feed: the
    way into the step — "int64" / "int32" token ids, or "embeds" (model.embed(ids) passed as embeddings).  stubs: the
    spy's (a dry run: device "cpu", no launch).  Returns (logits, the spied list)."""
    from hydrainfer_amd._C.kernel.flash_attn import decode_rank
    from hydrainfer_amd.layer.causal_attention import AttentionParameters
    from hydrainfer_amd.memory.kv_cache import KVCache
    from hydrainfer_amd.model.llama import LanguageModelParameters
    m = c.meta()
    d = lambda t: t.to(device)
    q_cu, kv_cu, slots, bt, cu_b = d(m.q_cu_seq_lens), d(m.kv_cu_seq_lens), d(m.new_cache_slots), d(m.block_tables), d(m.cu_blocks_lens)
    rank = decode_rank(kv_cu) if stubs is None else None
    ap = [AttentionParameters(kv_cache=KVCache(pool_d[l, 0], pool_d[l, 1]), q_cu_seq_lens=q_cu, kv_cu_seq_lens=kv_cu,
                              new_cache_slots=slots, block_tables=bt, cu_blocks_lens=cu_b, num_sequences=c.n,
                              all_sequences_decode=True, q_max_seq_len=1, kv_max_seq_len=max(c.ctx), decode_rank=rank)
          for l in range(LAYERS)]
    params = LanguageModelParameters(attention_params=ap, all_sequences_decode=True)
    ids = d(c.ids)
    x = {"int64": lambda: ids, "int32": lambda: ids.to(torch.int32), "embeds": lambda: model.embed(ids)}[feed]()
    with spy(keep_tensors, stubs=stubs) as seen:
        logits = model.forward_logits(x, d(c.positions), params)
    return logits, seen
