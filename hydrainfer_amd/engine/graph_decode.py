"""hipGraph replay of decode-only fill batches inside the engine (the
reference's unfinished attempt is hydrainfer/model_runner/cuda_graph_model_runner.py:1-72).

A decode step of a 7B model is ~260 launches of 5-70 us kernels; issued eagerly the host cannot
keep ahead of the GPU.  Here the step's integer inputs live in ONE static device buffer

    [ input_ids | positions | new_cache_slots | kv_cu | cu_blocks_lens | block_tables ... ]

and the forward over views of that buffer is captured once per padded batch size.  The block tables
are RESIDENT (SURVEY.md §8(f) rank 1 as written: "a persistent device-side block-table buffer with
incremental append"): every live sequence owns a fixed slice of the table region, a step stages its
head (ids, positions, slots, cumulative lengths, table offsets, rank descriptor — 7 words a row) and
only the block ids that are NEW since the sequence's last step (DecodeStager), and one kernel
(hx_stage_decode) applies both from pinned memory.  The reference rebuilds every table and copies
six tensors per step (hydrainfer/engine/parameters_builder.py:46-97, layer/causal_attention.py:147-168).  Batches are padded to a multiple of `pad_to` rows; padding rows are
1-token sequences that write into a scratch block reserved from the pool, so they never touch a
live request.  The attention kernel reads each sequence's true length from kv_cu, so one graph
serves every context length (the captured max length only seeds the split heuristic).

One step of look-ahead: the token a request sampled in launch N is its input in launch N+1, and
only the DEVICE needs it for that.  The graph therefore starts by taking each row's input id either
from the host-written id or from `prev_tokens[src_row]` (the previous launch's samples, kept in a
static buffer the graph itself updates at its end), so the host can build and enqueue launch N+1
while launch N is still running and read N's tokens afterwards (`launch` / `fetch`).  The host work
of a step (scheduler, tables, staging) no longer leaves the GPU idle.

A captured step is keyed (B, bucket, variant), variant one of VARIANTS; the plain step is (B, bucket, "greedy").

Sampled decoding from the graph (`sampled=True`, opt-in): a second variant of the step, keyed (B, bucket, "sampled"), ends
in hx_sample_rows_resident instead of the argmax.  Its records live in a RESIDENT table indexed by launch row; a
record's offset word is `n_out - position`, which decode never changes, and the kernel adds the row's position — the
array the step already reads — so neither a look-ahead launch nor a cohort step restages anything (DESIGN.md,
"Sampled decoding from the captured step").

Penalties from the graph (`penalized=True`, opt-in, needs `sampled`): a third variant, keyed (B, bucket, "penalized"), ends
in hx_sample_rows_resident_penalized.  A penalised request's generated tokens live in a RESIDENT token log, a slot per
request (PenaltyLogTable), which the kernel itself appends to — so the look-ahead launch finds the newest token where it
needs it, and the host uploads tokens only to seed a request the log does not hold ("Penalties from the
captured step")."""
import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from hydrainfer_amd import _lib, launch_plan
from hydrainfer_amd._lib import HydraHipError
from hydrainfer_amd._C.kernel.norm import StepHead
from hydrainfer_amd.layer.causal_attention import RANKED_THR, AttentionParameters, decode_rank_descriptor
from hydrainfer_amd.memory.kv_cache import KVCache
from hydrainfer_amd.model.llama import LanguageModelParameters
from hydrainfer_amd.sampling import (PENALTY_RECORD_WORDS, SAMPLE_LOG_MAX, SAMPLE_MAX_N, SAMPLE_RECORD_WORDS,
                                     pack_penalty_records, pack_resident_records, sample_rows_resident,
                                     sample_rows_resident_penalized)

# The variants of a captured step, each with what the one before it has: the argmax; hx_sample_rows_resident over the
# resident records; hx_sample_rows_resident_penalized over the penalty records and the token log as well.  A decoder
# has a prefix of them (GraphedDecoder.variants).
VARIANTS = ("greedy", "sampled", "penalized")


class CapturedStep(NamedTuple):
    graph: object                  # a hipGraph or a launch plan: .replay()
    out: torch.Tensor              # the step's tokens (a view of prev_tokens)
    err: Optional[torch.Tensor]    # the give-up word of its in-kernel hand-overs, None without any
    logits: Optional[torch.Tensor] # None for the greedy variant


def step_variant(records, penalties, variants=VARIANTS):
    """What launch() was given -> (variant, records, penalties) for a decoder that has `variants`: all None counts as
    None, and what the decoder or the rows cannot serve is refused."""
    if records is not None and all(r is None for r in records):
        records = None
    if records is not None and "sampled" not in variants:
        raise HydraHipError("sampling records for a decoder without a sampled variant (sampled=False, a vocabulary "
                            f"above {SAMPLE_MAX_N}, or logits that are not fp16 / bf16)")
    if penalties is not None and all(p is None for p in penalties):
        penalties = None
    if penalties is not None:
        if "penalized" not in variants:
            raise HydraHipError("penalties for a decoder without a penalised variant (penalized=False, or no sampled variant)")
        if records is None or any(p is not None and r is None for p, r in zip(penalties, records)):
            raise HydraHipError("a penalised row needs a record: (0.0, 1.0, 0, 0, n_out - position) for a greedy one")
    return VARIANTS[(records is not None) + (penalties is not None)], records, penalties


NAMED, ANONYMOUS, PADDING = "named", "anonymous", "padding"


def row_identity(row: tuple, i: int):
    """Launch row i -> (sid, kind).  A row that names its sequence (a sixth element) is NAMED and keyed by it; one that
    does not is ANONYMOUS, keyed ("row", i), and the stager writes its table in full every step; a sixth element of None
    is a PADDING / warm-up row — no table of its own for the stager, ("row", i) for the penalty log."""
    if len(row) <= 5:
        return ("row", i), ANONYMOUS
    if row[5] is None:
        return ("row", i), PADDING
    return row[5], NAMED


class DecodeStager:
    """The host side of a decode step's integer inputs — numpy only, no device (tests/test_decode_stager.py drives it on
    the CPU).  Layout of the static device buffer it fills (word offsets; B = max_batch, cap = blocks per sequence):

        [ ids B | pos B | slots B | src B | kv_cu B+1 | cu_blocks B+1 | rank B+1 | tables (2B + 1) x cap ]

    cu_blocks[r] = the word offset of row r's table INSIDE the tables region (the kernels only ever use it as a start
    offset).  Table slot 0 is the padding rows' ([pad_block]); a sequence (keyed by the scheduler's sid) keeps its slot
    from its first decode step until it has not been seen while the slots ran out (least recently seen goes first).
    stage() writes one staging buffer: the head, then [n_runs] and the runs ([dst word offset] [count] [values]) that bring
    the resident tables up to date — hx_stage_decode's input."""

    def __init__(self, max_batch: int, cap: int, block_size: int, pad_block: int, max_pos: int, vocab: int):
        B = self.max_batch = max_batch
        self.cap, self.block_size, self.pad_block, self.max_pos, self.vocab = cap, block_size, pad_block, max_pos, vocab
        self.off = {"ids": 0, "pos": B, "slots": 2 * B, "src": 3 * B, "kv_cu": 4 * B, "cu_blocks": 5 * B + 1, "rank": 6 * B + 2}
        self.head_words = 7 * B + 3
        self.n_table_slots = 2 * B + 1
        self.tables_off = self.head_words
        self.total_words = self.head_words + self.n_table_slots * cap
        self.staging_words = self.head_words + 1 + (B + 1) * (2 + cap)
        self.slot_of: Dict[int, list] = {}        # sid -> [table slot, blocks written, last block id written, last step seen]
        self.free = list(range(self.n_table_slots - 1, 0, -1))
        self.pad_written = False
        self.step_no = 0
        self._arange = np.arange(max_batch, dtype=np.int32)

    def _alloc(self) -> int:
        if self.free:
            return self.free.pop()
        victim = min((sid for sid, e in self.slot_of.items() if e[3] != self.step_no), key=lambda sid: self.slot_of[sid][3])
        return self.slot_of.pop(victim)[0]

    def stage(self, st: "np.ndarray", rows: List[tuple], B: int) -> int:
        """rows: (token, position, slot, kv_len, block_table, sid) per live sequence (sid None: a padding / warm-up row);
        a token < 0 means "the sample of row -(token + 1) of the previous launch".  Pads to B rows.  Returns the largest
        kv_len."""
        self.step_no += 1
        o, cap, n = self.off, self.cap, len(rows)
        if not all(0 <= r[1] < self.max_pos for r in rows):    # the RoPE / attention kernels index cos_sin unchecked
            raise HydraHipError(f"decode position outside the rotary table (max_position_embeddings = {self.max_pos})")
        if not all(r[0] < self.vocab for r in rows):           # hx_embed_rms_norm would clamp, torch.embedding raises
            raise HydraHipError(f"token id outside the vocabulary ({self.vocab})")
        pad = B - n
        toks = [r[0] for r in rows]
        st[o["ids"]:o["ids"] + B] = [t if t > 0 else 0 for t in toks] + [0] * pad
        st[o["src"]:o["src"] + B] = [-(t + 1) if t < 0 else -1 for t in toks] + [-1] * pad
        st[o["pos"]:o["pos"] + B] = [r[1] for r in rows] + [0] * pad
        st[o["slots"]:o["slots"] + B] = [r[2] for r in rows] + [self.pad_block * self.block_size] * pad
        kv = [r[3] for r in rows] + [1] * pad
        st[o["kv_cu"]] = 0
        np.cumsum(kv, out=st[o["kv_cu"] + 1:o["kv_cu"] + B + 1])
        st[o["rank"]:o["rank"] + B + 1] = decode_rank_descriptor(kv)
        at = self.head_words + 1
        n_runs = 0
        if not self.pad_written:
            st[at:at + 3] = (self.tables_off, 1, self.pad_block)
            at += 3
            n_runs += 1
            self.pad_written = True
        starts = []
        for i, r in enumerate(rows):
            tbl = r[4]
            sid, kind = row_identity(r, i)
            if kind is PADDING:
                starts.append(0)
                continue
            nb = len(tbl)
            if nb > cap:
                raise HydraHipError(f"a sequence of {nb} blocks in a decoder built for {cap}")
            e = self.slot_of.get(sid)
            if e is None:
                e = self.slot_of[sid] = [self._alloc(), 0, -1, self.step_no]
            e[3] = self.step_no
            if kind is ANONYMOUS or nb < e[1] or (e[1] and tbl[e[1] - 1] != e[2]):
                e[1] = 0                       # not the table this slot holds a prefix of: written again in full
            if nb > e[1]:
                new = tbl[e[1]:]
                st[at] = self.tables_off + e[0] * cap + e[1]
                st[at + 1] = len(new)
                st[at + 2:at + 2 + len(new)] = new
                at += 2 + len(new)
                n_runs += 1
                e[1], e[2] = nb, tbl[-1]
            starts.append(e[0] * cap)
        st[o["cu_blocks"]:o["cu_blocks"] + B] = starts + [0] * pad
        st[o["cu_blocks"] + B] = 0
        st[self.head_words] = n_runs
        return max(kv)


    def stage_cohort(self, st: "np.ndarray", n: int, B: int, pos: "np.ndarray", slots: "np.ndarray", starts: "np.ndarray",
                     grown: List[Tuple[int, int, int]]) -> int:
        """The steady-state form of stage(): the SAME n sequences as the previous launch, in the same order, one token
        further — every row's input id is the previous launch's sample of the same row (src[r] = r), positions / slots /
        table offsets come as arrays, and `grown` lists the rows that entered a new block: (sid, blocks before, new
        block id).  No per-row Python except for those."""
        self.step_no += 1
        o, pad = self.off, B - n
        if int(pos[:n].max()) >= self.max_pos:
            raise HydraHipError(f"decode position outside the rotary table (max_position_embeddings = {self.max_pos})")
        st[o["ids"]:o["ids"] + B] = 0
        st[o["src"]:o["src"] + n] = self._arange[:n]
        st[o["pos"]:o["pos"] + n] = pos[:n]
        st[o["slots"]:o["slots"] + n] = slots[:n]
        st[o["cu_blocks"]:o["cu_blocks"] + n] = starts[:n]
        if pad:
            st[o["src"] + n:o["src"] + B] = -1
            st[o["pos"] + n:o["pos"] + B] = 0
            st[o["slots"] + n:o["slots"] + B] = self.pad_block * self.block_size
            st[o["cu_blocks"] + n:o["cu_blocks"] + B] = 0
        st[o["cu_blocks"] + B] = 0
        kv = st[o["kv_cu"] + 1:o["kv_cu"] + B + 1]
        kv[:n] = pos[:n]
        kv[:n] += 1
        kv[n:] = 1
        # the rank descriptor (layer/causal_attention.py::decode_rank_descriptor, the same words) without a Python loop
        kv_max = int(kv.max())
        if B <= 256:
            st[o["rank"]] = 1 if float(kv_max) > float(kv.sum()) / B * RANKED_THR + 16.0 else 0
            st[o["rank"] + 1:o["rank"] + B + 1] = np.argsort(-kv, kind="stable")
        else:
            st[o["rank"]] = 0
            st[o["rank"] + 1:o["rank"] + B + 1] = self._arange[:B]
        st[o["kv_cu"]] = 0
        np.cumsum(kv, out=kv)
        at = self.head_words + 1
        for sid, before, block in grown:
            e = self.slot_of[sid]
            st[at:at + 3] = (self.tables_off + e[0] * self.cap + before, 1, block)
            at += 3
            e[1], e[2] = before + 1, block
        st[self.head_words] = len(grown)
        return kv_max

    def touch(self, sids) -> None:
        """The sequences of a cohort episode were seen until now (least-recently-seen bookkeeping)."""
        for sid in sids:
            e = self.slot_of.get(sid)
            if e is not None:
                e[3] = self.step_no


class PenaltyLogTable:
    """The host side of the resident token log of penalised requests — plain Python, no device
    (tests/test_graph_penalties_cpu.py drives it on the CPU).  A slot of the log belongs to a REQUEST (keyed by the
    scheduler's sid, as DecodeStager.slot_of), not to a launch row: per sid it keeps [slot, next_L, last step seen], next_L
    the generated-token count the request's next launch must come with for the log to hold its tokens already — the
    kernel appended the newest one itself.  Any other count (a first appearance, a return from eager steps, a slot that
    was taken away) makes the request be SEEDED with its tokens [0, L) from the host.  Slots are reused least recently
    seen first, never one seen by this launch or the one before it (which may still be in flight): with at least twice
    as many slots as launch rows there is always another."""

    def __init__(self, n_slots: int, cap: int):
        self.n_slots, self.cap = n_slots, cap
        self.slot_of: Dict[object, list] = {}
        self.free = list(range(n_slots - 1, -1, -1))
        self.step_no = 0
        self.last: List = []              # the sids of the most recent launch's penalised rows
        self.n_seeds = 0                  # seeds so far (tests, the benchmark)

    def continues(self, sid, L: int) -> bool:
        """The log holds tokens [0, L) of this request: a launch at L uploads nothing."""
        e = self.slot_of.get(sid)
        return e is not None and e[1] == L

    def _alloc(self) -> int:
        if self.free:
            return self.free.pop()
        idle = [sid for sid, e in self.slot_of.items() if e[2] < self.step_no - 1]
        if not idle:
            raise HydraHipError(f"no free slot in a token log of {self.n_slots}: every one is in use by this launch or the last")
        return self.slot_of.pop(min(idle, key=lambda sid: self.slot_of[sid][2]))[0]

    def step(self, rows) -> Tuple[List[int], List[Tuple[int, List[int]]]]:
        """rows: per launch row None or (sid, L, tokens) — L the request's generated-token count, tokens a sequence that
        holds its generated tokens (read only when the row must be seeded; may be None otherwise).  -> (the rows' slots,
        -1 for None; the seeds to upload as (slot, tokens [0, L))).  Raises, before anything changes, for an L outside
        [0, cap], for a seed that is not L token ids — a placeholder of a token still on the device among them — and
        when the launch needs more slots than are free or idle."""
        seeds = {}
        for i, row in enumerate(rows):
            if row is None:
                continue
            sid, L, tokens = row
            if not 0 <= L <= self.cap:
                raise HydraHipError(f"a penalised row at generated-token count {L} in a token log of {self.cap} per request")
            if not self.continues(sid, L):
                seed = list(tokens[:L]) if tokens is not None else None
                if seed is None or len(seed) != L or not all(isinstance(t, (int, np.integer)) for t in seed):
                    raise HydraHipError(f"a penalised row must be seeded with its {L} generated tokens, all of them on the "
                                        "host (a placeholder of a token still on the device is none)")
                seeds[i] = seed
        mine = {row[0] for row in rows if row is not None}
        idle = sum(1 for sid, e in self.slot_of.items() if sid not in mine and e[2] < self.step_no)
        if len(mine - self.slot_of.keys()) > len(self.free) + idle:
            raise HydraHipError(f"no slot left in a token log of {self.n_slots}: the others belong to this launch or the last")
        self.step_no += 1
        for row in rows:                  # seen now: no row of this launch loses its slot to another one's
            if row is not None and row[0] in self.slot_of:
                self.slot_of[row[0]][2] = self.step_no
        slots, uploads, self.last = [], [], []
        for i, row in enumerate(rows):
            if row is None:
                slots.append(-1)
                continue
            sid, L, _ = row
            e = self.slot_of.get(sid)
            if e is None:
                slot = self._alloc()
                e = self.slot_of[sid] = [slot, L, self.step_no]
            if i in seeds:
                self.n_seeds += 1
                if L:
                    uploads.append((e[0], seeds[i]))
            e[1], e[2] = L + 1, self.step_no
            slots.append(e[0])
            self.last.append(sid)
        return slots, uploads

    def step_cohort(self) -> None:
        """The same rows as the previous launch, one token further (GraphedDecoder.launch_cohort): nothing to upload."""
        self.step_no += 1
        for sid in self.last:
            e = self.slot_of[sid]
            e[1] += 1
            e[2] = self.step_no


class ResidentTable:
    """A table that stays on the device, one packed row per launch row: `tensor`, the host's copy of what it holds, by
    row (`mirror`), and the pinned double buffer new rows go through — used alternately with the decoder's staging
    buffers and guarded by the same events.  `packer(rows, out=None)` packs a list of rows (None: the row that does
    nothing) into int32 [len(rows), words].  On a CPU device (tests/test_decode_step_cpu.py) nothing is pinned."""

    def __init__(self, packer, words: int, n_rows: int, device):
        self.packer, self.words = packer, words
        empty = torch.from_numpy(packer([None] * n_rows))
        self.tensor = empty.to(device)
        self.mirror: List[Optional[tuple]] = [None] * n_rows
        pinned = torch.device(device).type != "cpu"
        self.staging = [empty.clone().pin_memory() if pinned else empty.clone() for _ in range(2)]
        self.stage = [t.numpy() for t in self.staging]

    def update(self, which: int, want: list) -> Optional[Tuple[int, int, int]]:
        """The first len(want) rows are to hold `want`: None when they do, else the rows are packed into pinned buffer
        `which` and the (dst address, src address, words) copy to enqueue comes back."""
        B = len(want)
        if want == self.mirror[:B]:
            return None
        self.packer(want, self.stage[which][:B])
        self.mirror[:B] = want
        return self.tensor.data_ptr(), self.staging[which].data_ptr(), self.words * B

    def reset(self) -> None:
        """Every row back to None, by a copy in stream order."""
        self.tensor.copy_(torch.from_numpy(self.packer([None] * len(self.mirror))))
        self.mirror = [None] * len(self.mirror)


class GraphedDecoder:
    def __init__(self, language_model, kv_cache_block_manager, max_batch: int = 64,
                 max_blocks_per_seq: int = 256, pad_to: int = 4, executor: str = None, sampled: bool = False,
                 keep_draws: bool = False, penalized: bool = False, penalty_log_cap: int = 1024):
        # how a captured step is replayed: "graph" = a hipGraph (default here), "plan" = a launch plan
        # (hydrainfer_amd/launch_plan.py: the step's launches issued in stream order by a native loop).  The plan costs
        # ~0.65 ms of HOST time per 7B step (170 launches x 3.8 us) where a graph launch costs ~0.1: irrelevant for a
        # GPU-bound decode loop (model/runner.py, where the plan is 0.5-1 % faster), but the engine's one thread also
        # schedules, stages and runs eager prefill steps — at 16 req/s Poisson the plan measured TPOT p50 7.7 ms and
        # TTFT p50 84 ms against 6.5 / 51 for the graph (tools/bench_engine.py, round 3)
        self.executor = executor or os.environ.get("HX_ENGINE_EXECUTOR", "graph")
        self.lm = language_model                       # LlavaLanguageModel
        self.model = language_model.language_model     # LlamaForCausalLM
        self.kv = kv_cache_block_manager
        self.dev = self.kv.device
        self.pad_to = pad_to
        self.max_batch = self._padded(max_batch)
        self.cap = max_blocks_per_seq
        B = self.max_batch
        # scratch block for padding rows
        self.pad_cache = self.kv.allocate_virtual_cache()
        self.kv.realloc(self.pad_cache, 1)
        self.pad_block = self.pad_cache.block_table[0]
        self.stager = DecodeStager(B, self.cap, self.kv.block_size, self.pad_block, self.model.shape.max_position_embeddings,
                                   self.model.shape.vocab_size)
        self.off = self.stager.off
        self.static = torch.zeros(self.stager.total_words, dtype=torch.int32, device=self.dev)
        # two pinned staging buffers used alternately, each with an event recorded behind the kernel that reads it:
        # with one step of look-ahead the host fills launch N+1 while launch N's staging may still be
        # queued (a vision encode or a prefill chunk ahead of it on the stream) — a buffer is
        # refilled only after the launch that last read it has run
        self.staging = [torch.zeros(self.stager.staging_words, dtype=torch.int32).pin_memory() for _ in range(2)]
        self.stage = [t.numpy() for t in self.staging]
        self.copy_done = [torch.cuda.Event(), torch.cuda.Event()]
        self.fills = 0
        self.q_cu = torch.arange(0, B + 1, dtype=torch.int32, device=self.dev)
        self.prev_tokens = torch.zeros(B, dtype=torch.int64, device=self.dev)   # the previous launch's samples
        self.host_tokens = [torch.zeros(B, dtype=torch.int64).pin_memory() for _ in range(2)]
        # word that is nonzero iff an in-kernel hand-over of that launch gave up waiting (csrc/gemm_xreg.hip): it
        # travels to the host with the launch's tokens and is checked in fetch()
        self.host_err = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(2)]
        self.launch_has_err = {}
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        self.launches = 0                  # id of the most recent launch (1-based)
        self.poisoned_until = 0            # launches <= this id were enqueued behind a failed hand-over: fetch raises
        self.launch_rows = {}              # launch id -> number of live rows
        n_layers = self.model.shape.num_hidden_layers
        self.kv_caches = [KVCache.from_token_cache(self.kv.get_layer_cache(l)) for l in range(n_layers)]
        self.graphs: Dict[Tuple[int, int, str], CapturedStep] = {}
        # sampled decoding from the graph: the records of the launch rows, resident; a padding row keeps the greedy record.
        # A vocabulary wider than the sampling kernel's row, or logits it does not read: no sampled variant — `sampled`
        # stays False and the executor keeps such batches eager
        self.sampled = bool(sampled) and self.model.shape.vocab_size <= SAMPLE_MAX_N \
            and self.model.dtype in (torch.float16, torch.bfloat16)
        self.keep_draws = keep_draws and self.sampled      # tests: the sampled graphs also write each row's u
        if self.sampled:
            self.record_table = ResidentTable(pack_resident_records, SAMPLE_RECORD_WORDS, B, self.dev)
            self.records = self.record_table.tensor
        # penalties from the graph: a third variant of the step ends in hx_sample_rows_resident_penalized over a token log
        # that stays on the device — a slot per REQUEST (PenaltyLogTable), twice as many as launch rows — and a table of
        # the launch rows' penalties and slots beside `records`.  Without a sampled variant: off, as `sampled` is
        self.penalized = bool(penalized) and self.sampled
        self.variants = VARIANTS[:1 + self.sampled + self.penalized]
        self.last_variant = "greedy"                       # the variant of the most recent launch (launch_cohort repeats it)
        if self.penalized:
            if not 1 <= penalty_log_cap <= SAMPLE_LOG_MAX:
                raise HydraHipError(f"penalty_log_cap {penalty_log_cap} outside 1 .. {SAMPLE_LOG_MAX}")
            self.penalty_log_cap = cap = int(penalty_log_cap)
            self.log_table = PenaltyLogTable(2 * B, cap)
            self.token_log = torch.zeros(2 * B, cap, dtype=torch.int32, device=self.dev)
            self.penalty_table = ResidentTable(pack_penalty_records, PENALTY_RECORD_WORDS, B, self.dev)
            self.penalty_records = self.penalty_table.tensor
            # the seeds of a fill, back to back (at worst every row of a launch, each with a full log row)
            self.seed_staging = [torch.zeros(B * cap, dtype=torch.int32).pin_memory() for _ in range(2)]
            self.seed_stage = [t.numpy() for t in self.seed_staging]
        if self.keep_draws:
            self.draws = torch.zeros(B, dtype=torch.float32, device=self.dev)
            self.host_draws = [torch.zeros(B, dtype=torch.float32).pin_memory() for _ in range(2)]
            self.draw_rows = {}            # launch id -> number of live rows (sampled launches only)

    @property
    def resident_penalties(self) -> List[Optional[tuple]]:
        """What the penalty table holds, by launch row (the host's copy)."""
        return self.penalty_table.mirror

    def _padded(self, n: int) -> int:
        """The row count of the captured step that serves n live rows."""
        return (n + self.pad_to - 1) // self.pad_to * self.pad_to

    def fits(self, n_seqs: int, max_blocks: int) -> bool:
        """n_seqs rows whose longest block table has max_blocks entries."""
        return self._padded(n_seqs) <= self.max_batch and max_blocks <= self.cap

    def _views(self, B: int):
        o, s = self.off, self.static
        return (s[o["ids"]:o["ids"] + B], s[o["pos"]:o["pos"] + B], s[o["slots"]:o["slots"] + B],
                s[o["kv_cu"]:o["kv_cu"] + B + 1], s[o["cu_blocks"]:o["cu_blocks"] + B + 1],
                s[self.stager.tables_off:], s[o["src"]:o["src"] + B], s[o["rank"]:o["rank"] + B + 1])

    def _kv_bucket(self, B: int, kv_max: int) -> int:
        if B * self.model.shape.num_attention_heads >= 768:
            return 0                       # one split whatever the length (attn_decode.hip heuristic)
        b = 256
        while b < kv_max:
            b *= 2
        return b

    def _params(self, B: int, kv_max: int) -> LanguageModelParameters:
        ids, pos, slots, kv_cu, cu_blocks, tables, _, rank = self._views(B)
        attn = [AttentionParameters(kv_cache=kc, q_cu_seq_lens=self.q_cu[:B + 1], kv_cu_seq_lens=kv_cu,
                                    new_cache_slots=slots, block_tables=tables, cu_blocks_lens=cu_blocks,
                                    num_sequences=B, all_sequences_decode=True, q_max_seq_len=1,
                                    kv_max_seq_len=kv_max, decode_rank=rank) for kc in self.kv_caches]
        return LanguageModelParameters(attention_params=attn, all_sequences_decode=True)

    def _body(self, B: int, params, variant: str):
        """One decode step as library launches only (+ the lm_head GEMM): recordable in a launch plan.  -> (out, err,
        logits).  "sampled": the step ends in hx_sample_rows_resident over the resident records instead of the argmax;
        "penalized": in hx_sample_rows_resident_penalized, over the resident penalty records and the token log as well.
        Both give their logits back, "greedy" gives None."""
        ids, pos = self._views(B)[:2]
        src = self._views(B)[6]
        lib = _lib.lib()
        if self.model.step_head_supported(B):
            # the look-ahead feed rides in the step's first launch (hx_decode_step_head: id = sample of row src[r] of the
            # previous launch when src[r] >= 0, else the host-written id) — one launch less per step
            params.step_head = StepHead(feed_src=src, feed_prev=self.prev_tokens)
            fed = ids
        else:
            params.step_head = None
            fed = torch.empty(B, dtype=torch.int64, device=self.dev)
            _lib.check(lib.hx_decode_feed_ids(fed.data_ptr(), ids.data_ptr(), src.data_ptr(), self.prev_tokens.data_ptr(), B,
                                              _lib.current_stream()), "decode_feed_ids")
        self.model.xreg_sync = None
        # the greedy sampler writes straight into prev_tokens: this launch's feed (above) has read it, the next
        # launch's feed and the D2H copy of the tokens read it after this launch, in stream order
        out = self.prev_tokens[:B]
        self.model.sample_out = out
        logits = None
        try:
            if variant == "penalized":
                logits = self.model.forward_logits(fed, pos, params)
                res = sample_rows_resident_penalized(logits, self.records[:B], pos, self.penalty_records[:B], self.token_log,
                                                     out=out, u_out=self.draws[:B] if self.keep_draws else None)
            elif variant == "sampled":
                logits = self.model.forward_logits(fed, pos, params)
                res = sample_rows_resident(logits, self.records[:B], pos, out=out,
                                           u_out=self.draws[:B] if self.keep_draws else None)
            else:
                res = self.model(fed, pos, params)
        finally:
            self.model.sample_out = None
            params.step_head = None      # consumed: a later direct model(...) call with these params must not feed again
        if res.data_ptr() != out.data_ptr():
            launch_plan.host_op(lambda: out.copy_(res))
        # give-up words of the step's in-kernel hand-overs (norm-fused launches) -> one word
        err = None
        sync = self.model.xreg_sync
        if sync is not None:
            err = torch.empty(1, dtype=torch.int32, device=self.dev)
            _lib.check(lib.hx_collect_errors(err.data_ptr(), sync.data_ptr(), sync.numel() // sync.shape[-1],
                                             sync.shape[-1], 1, None, _lib.current_stream()), "collect_errors")
        return out, err, logits

    def _capture(self, B: int, bucket: int, variant: str) -> CapturedStep:
        params = self._params(B, bucket if bucket else 4096)
        saved = self.prev_tokens.clone()
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            for _ in range(2):             # warm-up outside capture: workspace growth, lazy init
                self.prev_tokens.copy_(saved)
                self._body(B, params, variant)
            self.prev_tokens.copy_(saved)
        torch.cuda.current_stream(self.dev).wait_stream(side)
        graph = None
        if self.executor == "plan":
            graph = launch_plan.LaunchPlan(self.dev)
            try:
                step = graph.capture(lambda: self._body(B, params, variant))
            except launch_plan.PlanNotRecordable:
                graph = None       # a step with torch ops in it (library GEMMs, a shape off the hx fast path): hipGraph
                self.executor = "graph"
        if graph is None:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step = self._body(B, params, variant)
        return CapturedStep(graph, *step)

    def _copy_words(self, copies) -> None:
        """(dst address, src address, words) copies, two to a launch (hx_copy_words2)."""
        for i in range(0, len(copies), 2):
            a, b = copies[i], copies[i + 1] if i + 1 < len(copies) else (None, None, 0)
            _lib.check(_lib.lib().hx_copy_words2(*a, *b, _lib.current_stream()), "copy_words2")

    def _staged(self, fill) -> int:
        """One turn of the pinned double buffers: take the next one, wait for the launch that last read it, let
        fill(which) -> (kv_max, copies) write the staging buffer (and the other pinned buffers of the turn the copies
        read), enqueue the kernel that applies it to the resident buffer, then the copies, and record the turn's event
        behind the last of them.  -> kv_max."""
        which = self.fills % 2
        self.fills += 1
        self.copy_done[which].synchronize()      # no-op until the buffer has been used once
        kv_max, copies = fill(which)
        # (a kernel reading the pinned buffer, not a memcpy: a memcpy between two graph launches left the stream idle
        # for ~0.1 ms per step)
        _lib.check(_lib.lib().hx_stage_decode(self.static.data_ptr(), self.static.numel(), self.staging[which].data_ptr(),
                                              self.stager.head_words, _lib.current_stream()), "stage_decode")
        self._copy_words(copies)
        self.copy_done[which].record()
        return kv_max

    def _fill(self, rows: List[tuple], B: int, records=None, penalties=None) -> int:
        """Stage the step (DecodeStager.stage) and enqueue the kernel that applies it to the resident buffer.  records:
        None, or the sampled step's record per live row — rows of the resident table that hold something else are
        rewritten, through the pinned buffer of this fill.  penalties: None, or per live row None or
        (frequency, presence, repetition[, the request's generated tokens]) — the rows' log slots are looked up, the
        penalty table is rewritten where it differs, and a row the log does not hold the tokens of is seeded, through
        the pinned buffers of this fill as well.  The copies go record table, penalty table, seeds, two to a launch."""
        slots = seeds = None
        if penalties is not None:
            slots, seeds = self.log_table.step([
                None if p is None else (row_identity(row, i)[0], records[i][4] + row[1], p[3] if len(p) > 3 else None)
                for i, (row, p) in enumerate(zip(rows, penalties))])
        pad = [None] * (B - len(rows))            # a padding row is greedy and unpenalised

        def fill(which):
            kv_max = self.stager.stage(self.stage[which], rows, B)
            copies = []
            if records is not None:
                copies.append(self.record_table.update(which, list(records) + pad))
            if penalties is not None:
                copies.append(self.penalty_table.update(
                    which, [None if p is None else (p[0], p[1], p[2], s) for p, s in zip(penalties, slots)] + pad))
                at, cap = 0, self.penalty_log_cap
                for slot, tokens in seeds:
                    self.seed_stage[which][at:at + len(tokens)] = tokens
                    copies.append((self.token_log.data_ptr() + 4 * slot * cap, self.seed_staging[which].data_ptr() + 4 * at,
                                   len(tokens)))
                    at += len(tokens)
            return kv_max, [c for c in copies if c is not None]
        return self._staged(fill)

    def warmup(self, batch_sizes: List[int], kv_max: int = 1024) -> None:
        rows = [(1, 0, self.pad_block * self.kv.block_size, 1, [self.pad_block], None)]
        for n in batch_sizes:
            B = self._padded(n)
            for variant in self.variants:
                key = (B, self._kv_bucket(B, kv_max), variant)
                if key not in self.graphs:
                    self._fill(rows, B)
                    if variant == "penalized" and any(p is not None for p in self.resident_penalties):
                        # a warm-up behind real launches: its padding rows must not write into a live request's log
                        self.penalty_table.reset()
                    self.graphs[key] = self._capture(*key)
        torch.cuda.synchronize(self.dev)

    def launch_cohort(self, n: int, pos, slots, starts, grown) -> int:
        """launch() for the same n sequences as the previous launch, one token further (DecodeStager.stage_cohort)."""
        B = self._padded(n)
        kv_max = self._staged(lambda which: (self.stager.stage_cohort(self.stage[which], n, B, pos, slots, starts, grown), ()))
        # the variant of the launch the cohort was formed behind: the same rows in the same order, so their records
        # are in the table already, and the positions staged above move every row's offset on by one.  Penalised rows:
        # their slots are unchanged and the log holds their newest token already — nothing to upload
        if self.last_variant == "penalized":
            self.log_table.step_cohort()
        return self._replay(n, B, kv_max, self.last_variant)

    def launch(self, rows: List[tuple], records=None, penalties=None) -> int:
        """Enqueue one decode step; returns a launch id for `fetch`.  Does not wait for the GPU.  records (a decoder
        built with sampled=True): per row None — greedy — or (temperature, top_p, top_k, seed, n_out - position); None or
        all None is the greedy step as it ever was.  penalties (a decoder built with penalized=True): per row None or
        (frequency, presence, repetition[, tokens]) — such a row needs a record (a greedy one: (0.0, 1.0, 0, 0, n_out -
        position)), and `tokens`, a sequence holding the request's generated tokens, whenever the log does not continue
        (PenaltyLogTable); None or all None: the launch is the one it is without the argument (step_variant)."""
        n = len(rows)
        B = self._padded(n)
        variant, records, penalties = step_variant(records, penalties, self.variants)
        kv_max = self._fill(rows, B, records, penalties)
        self.last_variant = variant
        return self._replay(n, B, kv_max, variant)

    def sample_logits(self, B: int, bucket: int, variant: str = "sampled"):
        """Tests: the logits tensor the sampled (or "penalized") graph (B, bucket) writes — the graph's own buffer, valid
        until the next replay."""
        return self.graphs[(B, bucket, variant)].logits

    def fetch_draws(self, launch_id: int):
        """Tests (keep_draws=True): the per-row u of a sampled launch, fp32 (waits for it); None for a greedy launch.
        Only the two most recent launches are kept."""
        assert launch_id > self.launches - 2, "draws of an older launch have been overwritten"
        n = self.draw_rows.get(launch_id)
        if n is None:
            return None
        self.events[launch_id % 2].synchronize()
        return self.host_draws[launch_id % 2][:n].numpy().copy()

    def _replay(self, n: int, B: int, kv_max: int, variant: str) -> int:
        key = (B, self._kv_bucket(B, kv_max), variant)
        if key not in self.graphs:
            self.graphs[key] = self._capture(*key)
        graph, out, err, _ = self.graphs[key]
        graph.replay()
        self.launches += 1
        slot = self.launches % 2
        # tokens (int64: 2 words each) and the give-up word leave by one launch, straight into pinned memory
        _lib.check(_lib.lib().hx_copy_words2(self.host_tokens[slot].data_ptr(), out.data_ptr(), 2 * n,
                                             self.host_err[slot].data_ptr() if err is not None else None,
                                             err.data_ptr() if err is not None else None, 1 if err is not None else 0,
                                             _lib.current_stream()), "copy_words2")
        self.launch_has_err[self.launches] = err is not None
        if self.keep_draws:
            self.draw_rows.pop(self.launches - 2, None)
            if variant != "greedy":
                _lib.check(_lib.lib().hx_copy_words2(self.host_draws[slot].data_ptr(), self.draws.data_ptr(), n, None, None,
                                                     0, _lib.current_stream()), "copy_words2")
                self.draw_rows[self.launches] = n
        self.events[slot].record()
        self.launch_rows[self.launches] = n
        return self.launches

    def fetch(self, launch_id: int) -> List[int]:
        """Tokens sampled by a launch (waits for it).  Only the two most recent launches are kept."""
        assert launch_id > self.launches - 2, "tokens of an older launch have been overwritten"
        slot = launch_id % 2
        self.events[slot].synchronize()
        n = self.launch_rows.pop(launch_id)
        if launch_id <= self.poisoned_until:
            self.launch_has_err.pop(launch_id, None)
            raise HydraHipError(f"decode launch {launch_id} was enqueued behind a launch whose in-kernel hand-over gave "
                                "up: its input tokens were invalid, so are its samples")
        if self.launch_has_err.pop(launch_id, False) and int(self.host_err[slot][0]) != 0:
            # a norm-fused launch consumed activations nobody had produced: this step's tokens are garbage.
            # Later steps run with the add+RMSNorm as separate launches (no in-kernel hand-over).
            self.model.fuse_norm = False
            # launch N+1 may already be running out of the same graph / plan, fed from this launch's garbage tokens:
            # let it finish before its buffers (the plan's private pool) go, and refuse its tokens as well
            torch.cuda.synchronize(self.dev)
            self.graphs.clear()
            self.poisoned_until = self.launches
            raise HydraHipError(f"decode launch {launch_id}: an in-kernel hand-over (norm-fused GEMM launch) gave up "
                                "waiting for its producer workgroups; the step's tokens are invalid. Later steps run "
                                "with the add+RMSNorm as separate launches (fuse_norm = False)")
        return self.host_tokens[slot][:n].tolist()

    def run(self, rows: List[Tuple[int, int, int, int, List[int]]], records=None, penalties=None) -> List[int]:
        return self.fetch(self.launch(rows, records, penalties))
