"""hydrainfer.sampling — counterpart of the reference's hydrainfer/sampling/logits_processor.py, and the draw the
reference never makes (its models end in torch.argmax).

`process_logits` (logits_processor.py:49-93) is five steps: frequency / presence and repetition penalties (1-2, lines
65-72), temperature (3), top-k (4), top-p (5).  Two kernels cover it:
- `penalized_argmax_rows` (hx_penalized_argmax_rows, csrc/penalties.hip): steps 1-2 and the argmax in one launch.  For a
  GREEDY request nothing else matters: a positive temperature keeps the order of the logits, top-k and top-p mask
  entries below the maximum.
- `sample_rows` (hx_sample_rows, csrc/sampling.hip): all five steps and a seeded draw in one launch.  A row with
  temperature 0 is greedy there and gets `penalized_argmax_rows`' id bit for bit, which is how greedy requests ride
  along in a batch that also holds sampled ones.  The exact semantics — what a tie at a cut does, where the random
  number comes from — are in include/hydra_hip.h; `temperature` absent means 0 here (OpenAI's default is 1).

The history.  The reference's processor takes one table of (token, count) per sequence and leaves open what goes into
it.  Here it holds the GENERATED tokens only, for all three penalties: prompts contain image placeholders (hundreds of
copies of one id) and chat-template tokens, which a prompt-inclusive repetition penalty would push down; OpenAI's
frequency / presence penalties are defined over the sampled text as well.  The first generated token therefore sees an
empty history.  `PenaltyHistory` is that table on the host, `pack_penalty_step` turns a step's tables into the kernel's
CSR, `pack_sample_step` does the same with the rows' sampling records in front — one buffer, one host-to-device copy.

Token constraints (`logit_bias`, `min_tokens`, `min_p`): `sample_rows_constrained` (hx_sample_rows_constrained) is
`sample_rows` with a per-row (token, bias) table added ahead of the penalties and a min_p cut; `TokenConstraints` is a
request's table on the host (min_tokens: its end-of-sequence ids banned while too few tokens stand), and
`pack_constrained_step` appends the step's bias CSR to `pack_sample_step`'s buffer.

Scores of the processed distribution (`logprobs_mode = "processed_logprobs"`): `sample_rows_logprobs`
(hx_sample_rows_logprobs) is `sample_rows_constrained` that also writes, for the rows that want it, the log-probability
of the chosen token under the distribution it was chosen from and the K most likely alternatives of that distribution,
in `logprob_rows`' packed layout.

Token masks (`allowed_token_ids`, `guided_choice`): `sample_rows_masked` (hx_sample_rows_masked) is the scored launch with
a per-row bitmask of the tokens a row may choose — 32 tokens per int32 word, 1 = allowed, the format grammar engines
exchange — applied as -inf ahead of everything else; `TokenMask` holds a request's masks (one node, or a trie over its
choices' token sequences) and where it stands, and `pack_masked_step` appends `want`, the rows' mask indices and the step's
distinct masks to `pack_constrained_step`'s buffer.

Sampled decoding from a captured decode step: `sample_rows_resident` (hx_sample_rows_resident) is `sample_rows` without a
history whose records stay on the device — `pack_resident_records` writes `n_out - position` where the offset stood, the
launch adds the row's position (engine/graph_decode.py).  `sample_rows_resident_penalized`
(hx_sample_rows_resident_penalized) penalises such a row as well, over a token log that stays on the device and that the
launch itself appends to; `pack_penalty_records` writes the rows' penalties and log slots."""
import math
from array import array
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from hydrainfer_amd import _lib

MAX_VOCAB = 1 << 18             # the widest row hx_penalized_argmax_rows takes (its LDS bitmap)
NO_PENALTIES = (0.0, 0.0, 1.0)  # (frequency, presence, repetition): the identity
SAMPLE_MAX_N = 35840            # the widest row hx_sample_rows takes (HX_SAMPLE_MAX_N: the row as fp32 in LDS)
SAMPLE_RECORD_WORDS = 8         # a row's record: [temperature, top_p (fp32 bits), top_k, 0, seed lo, hi, offset lo, hi]
GREEDY_RECORD = (0.0, 1.0, 0, 0, 0)     # (temperature, top_p, top_k, seed, offset): the row is penalised argmax
MAX_SEED = (1 << 63) - 1
SAMPLE_LOG_MAX = 4096           # the longest row of a resident token log (HX_SAMPLE_LOG_MAX)
PENALTY_RECORD_WORDS = 4        # a row's penalty record: [frequency, presence, repetition (fp32 bits), log slot]


def penalized_argmax_rows(logits: Tensor, hist_ids: Tensor, hist_counts: Tensor, cu_hist: Tensor, penalties: Tensor,
                          out: Optional[Tensor] = None, scores_out: Optional[Tensor] = None) -> Tensor:
    """Greedy ids of fp16 / bf16 logits [rows, n] under per-row penalties, one launch (include/hydra_hip.h:
    hx_penalized_argmax_rows).  hist_ids / hist_counts int32 [total] and cu_hist int32 [rows + 1]: the rows' (token,
    count) tables as a CSR, ids within a row pairwise distinct; penalties fp32 [rows, 3] = (frequency, presence,
    repetition).  Returns int64 [rows] (`out` if given); a row with an empty table gives argmax_rows' id.  scores_out:
    an fp32 [total] tensor that receives the penalised value of every table entry (NaN for an id outside the row)."""
    _lib.require_gpu(logits, hist_ids, hist_counts, cu_hist, penalties, out, scores_out)
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.dtype not in (torch.float16, torch.bfloat16) \
            or logits.shape[0] < 1 or not 1 <= logits.shape[1] <= MAX_VOCAB or logits.stride(0) < logits.shape[1]:
        raise _lib.HydraHipError(f"penalized_argmax_rows: logits must be fp16 / bf16 [rows, n] (rows >= 1, 1 <= n <= {MAX_VOCAB}) "
                                 "with contiguous rows")
    rows, total = logits.shape[0], hist_ids.numel()
    for name, t, shape in (("hist_ids", hist_ids, (total,)), ("hist_counts", hist_counts, (total,)), ("cu_hist", cu_hist, (rows + 1,))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.HydraHipError(f"penalized_argmax_rows: {name} must be a contiguous int32 tensor of shape {list(shape)}")
    if penalties.dtype != torch.float32 or tuple(penalties.shape) != (rows, 3) or not penalties.is_contiguous():
        raise _lib.HydraHipError(f"penalized_argmax_rows: penalties must be a contiguous fp32 tensor of shape [{rows}, 3]")
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=logits.device)
    elif out.dtype != torch.int64 or out.shape != (rows,) or not out.is_contiguous() or out.device != logits.device:
        raise _lib.HydraHipError("penalized_argmax_rows: out must be a contiguous int64 [rows] tensor on the logits' device")
    if scores_out is not None and (scores_out.dtype != torch.float32 or tuple(scores_out.shape) != (total,)
                                   or not scores_out.is_contiguous()):
        raise _lib.HydraHipError(f"penalized_argmax_rows: scores_out must be a contiguous fp32 tensor of shape [{total}]")
    _lib.check(_lib.lib().hx_penalized_argmax_rows(
        out.data_ptr(), scores_out.data_ptr() if scores_out is not None and total else None, logits.data_ptr(), rows,
        logits.shape[1], logits.stride(0), hist_ids.data_ptr() if total else None, hist_counts.data_ptr() if total else None,
        cu_hist.data_ptr(), total, penalties.data_ptr(), _lib.dtype_code(logits), _lib.current_stream()),
        "penalized_argmax_rows")
    return out


def check_penalties(frequency_penalty, presence_penalty, repetition_penalty) -> Tuple[float, float, float]:
    """The three values as floats, or ValueError: each a finite number (a bool is not one), repetition > 0."""
    for name, v in (("frequency_penalty", frequency_penalty), ("presence_penalty", presence_penalty),
                    ("repetition_penalty", repetition_penalty)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} {v!r} must be a finite number")
    if repetition_penalty <= 0:
        raise ValueError(f"repetition_penalty {repetition_penalty!r} must be > 0")
    return float(frequency_penalty), float(presence_penalty), float(repetition_penalty)


def is_penalized(sampling_params) -> bool:
    """False for (0, 0, 1): such a request is sampled by plain argmax and takes the engine's unpenalised paths."""
    return (sampling_params.frequency_penalty != 0 or sampling_params.presence_penalty != 0
            or sampling_params.repetition_penalty != 1)


class PenaltyHistory:
    """The generated tokens of one request as the reference's (unique_token_ids, unique_token_counts) table: parallel
    `ids` / `counts` lists in order of first appearance and an id -> slot dict, so appending a token is O(1).  The lists
    are int32 arrays (array('i')): the packer copies them into a step's buffer as memory, not element by element."""
    __slots__ = ("ids", "counts", "slot")

    def __init__(self, tokens: Sequence[int] = ()):
        self.ids = array("i")
        self.counts = array("i")
        self.slot = {}
        for t in tokens:
            self.append(t)

    def append(self, token: int) -> None:
        j = self.slot.get(token)
        if j is None:
            self.slot[token] = len(self.ids)
            self.ids.append(token)
            self.counts.append(1)
        else:
            self.counts[j] += 1

    def __len__(self) -> int:
        return len(self.ids)


class _PackedStep:
    """A step's tables as one int32 host `buffer`, which the subclass's `views` cuts into a kernel's arguments."""
    __slots__ = ()

    def to_device(self, device):
        """`views` on `device`: the buffer goes through pinned memory in ONE host-to-device copy."""
        host = torch.from_numpy(self.buffer)
        if torch.device(device).type == "cuda":
            host = host.pin_memory()
        return self.views(host.to(device, non_blocking=True))


class PenaltyStep(_PackedStep):
    """A step's packed tables: one int32 host buffer [cu_hist (rows + 1) | penalties (3 rows, fp32 bits) | hist_ids
    (total) | hist_counts (total)] — `views` cuts it (on the host or on the device) into the kernel's four arguments."""
    __slots__ = ("buffer", "rows", "total")

    def __init__(self, buffer: np.ndarray, rows: int, total: int):
        self.buffer, self.rows, self.total = buffer, rows, total

    def views(self, t: Optional[Tensor] = None):
        """(hist_ids, hist_counts, cu_hist, penalties) inside `t`, a tensor holding the buffer (default: a host copy)."""
        if t is None:
            t = torch.from_numpy(self.buffer)
        a, b = self.rows + 1, 4 * self.rows + 1
        return (t[b:b + self.total], t[b + self.total:b + 2 * self.total], t[:a],
                t[a:b].view(torch.float32).view(self.rows, 3))


def pack_penalty_step(entries) -> PenaltyStep:
    """entries: one (PenaltyHistory or None, (frequency, presence, repetition)) per logits row, in row order.  None or
    an empty history: the row is plain argmax (its penalties travel all the same)."""
    rows = len(entries)
    lens = [len(h) if h is not None else 0 for h, _ in entries]
    total = sum(lens)
    buf = np.zeros(4 * rows + 1 + 2 * total, dtype=np.int32)
    np.cumsum(lens, out=buf[1:rows + 1])
    buf[rows + 1:4 * rows + 1] = np.asarray([p for _, p in entries], dtype=np.float32).reshape(-1).view(np.int32)
    at = 4 * rows + 1
    for (h, _), n in zip(entries, lens):
        if n:
            buf[at:at + n] = np.frombuffer(h.ids, dtype=np.int32)
            buf[at + total:at + total + n] = np.frombuffer(h.counts, dtype=np.int32)
            at += n
    return PenaltyStep(buf, rows, total)


def _check_sample_arguments(what: str, logits, sample_params, hist_ids, hist_counts, cu_hist, penalties, out, cut_out, u_out,
                            ids_in_packed: bool = False):
    """The argument checks sample_rows, sample_rows_constrained and sample_rows_logprobs share -> (rows, total, out).
    ids_in_packed: the ids go into the caller's packed buffer (sample_rows_logprobs): no `out` is checked or made."""
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.dtype not in (torch.float16, torch.bfloat16) \
            or logits.shape[0] < 1 or not 1 <= logits.shape[1] <= SAMPLE_MAX_N or logits.stride(0) < logits.shape[1]:
        raise _lib.HydraHipError(f"{what}: logits must be fp16 / bf16 [rows, n] (rows >= 1, 1 <= n <= {SAMPLE_MAX_N}) "
                                 "with contiguous rows")
    rows = logits.shape[0]
    if sample_params.dtype != torch.int32 or tuple(sample_params.shape) != (rows, SAMPLE_RECORD_WORDS) \
            or not sample_params.is_contiguous():
        raise _lib.HydraHipError(f"{what}: sample_params must be a contiguous int32 tensor of shape "
                                 f"[{rows}, {SAMPLE_RECORD_WORDS}]")
    tables = (hist_ids, hist_counts, cu_hist, penalties)
    total = 0
    if any(t is not None for t in tables):
        if any(t is None for t in tables):
            raise _lib.HydraHipError(f"{what}: hist_ids, hist_counts, cu_hist and penalties come together or not at all")
        total = hist_ids.numel()
        for name, t, shape in (("hist_ids", hist_ids, (total,)), ("hist_counts", hist_counts, (total,)),
                               ("cu_hist", cu_hist, (rows + 1,))):
            if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
                raise _lib.HydraHipError(f"{what}: {name} must be a contiguous int32 tensor of shape {list(shape)}")
        if penalties.dtype != torch.float32 or tuple(penalties.shape) != (rows, 3) or not penalties.is_contiguous():
            raise _lib.HydraHipError(f"{what}: penalties must be a contiguous fp32 tensor of shape [{rows}, 3]")
    if ids_in_packed:
        pass
    elif out is None:
        out = torch.empty(rows, dtype=torch.int64, device=logits.device)
    elif out.dtype != torch.int64 or out.shape != (rows,) or not out.is_contiguous() or out.device != logits.device:
        raise _lib.HydraHipError(f"{what}: out must be a contiguous int64 [rows] tensor on the logits' device")
    for name, t in (("cut_out", cut_out), ("u_out", u_out)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (rows,) or not t.is_contiguous()):
            raise _lib.HydraHipError(f"{what}: {name} must be a contiguous fp32 tensor of shape [{rows}]")
    return rows, total, out


def sample_rows(logits: Tensor, sample_params: Tensor, hist_ids: Optional[Tensor] = None,
                hist_counts: Optional[Tensor] = None, cu_hist: Optional[Tensor] = None,
                penalties: Optional[Tensor] = None, out: Optional[Tensor] = None, cut_out: Optional[Tensor] = None,
                u_out: Optional[Tensor] = None) -> Tensor:
    """Sampled ids of fp16 / bf16 logits [rows, n]: penalties, temperature, top-k, top-p and a seeded draw in one launch
    (include/hydra_hip.h: hx_sample_rows).  sample_params: int32 [rows, 8], the rows' records (`pack_sample_records`); a
    row with temperature 0 gets `penalized_argmax_rows`' id.  The four history tensors are those of
    `penalized_argmax_rows`, all given or all None (no row is penalised).  Returns int64 [rows] (`out` if given).
    cut_out / u_out: fp32 [rows] tensors that receive each row's top-p cut v* (NaN for a greedy or degenerate row) and
    its uniform number u."""
    _lib.require_gpu(logits, sample_params, hist_ids, hist_counts, cu_hist, penalties, out, cut_out, u_out)
    rows, total, out = _check_sample_arguments("sample_rows", logits, sample_params, hist_ids, hist_counts, cu_hist, penalties,
                                               out, cut_out, u_out)
    ptr = (lambda t: t.data_ptr()) if total else (lambda t: None)
    _lib.check(_lib.lib().hx_sample_rows(
        out.data_ptr(), cut_out.data_ptr() if cut_out is not None else None, u_out.data_ptr() if u_out is not None else None,
        logits.data_ptr(), rows, logits.shape[1], logits.stride(0), ptr(hist_ids), ptr(hist_counts), ptr(cu_hist), total,
        ptr(penalties), sample_params.data_ptr(), _lib.dtype_code(logits), _lib.current_stream()), "sample_rows")
    return out


def check_sampling(temperature, top_p, top_k, seed) -> Tuple[float, float, int, Optional[int]]:
    """The four values checked, or ValueError: temperature a finite number >= 0 (0: greedy), top_p a number in (0, 1],
    top_k an integer >= 0 (0: off), seed None or an integer in 0 .. 2^63 - 1.  A bool is no number."""
    for name, v in (("temperature", temperature), ("top_p", top_p)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} {v!r} must be a finite number")
    if temperature < 0:
        raise ValueError(f"temperature {temperature!r} must be >= 0")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p {top_p!r} must be in (0, 1]")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k <= 0x7fffffff:
        raise ValueError(f"top_k {top_k!r} must be an integer >= 0")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= MAX_SEED):
        raise ValueError(f"seed {seed!r} must be an integer in 0 .. 2^63 - 1")
    return float(temperature), float(top_p), top_k, seed


def is_sampled(sampling_params) -> bool:
    """False for temperature 0: such a request is greedy and takes the engine's argmax paths."""
    return sampling_params.temperature > 0


def pack_sample_records(records, out: Optional[np.ndarray] = None) -> np.ndarray:
    """records: one (temperature, top_p, top_k, seed, offset) per logits row -> int32 [rows, 8], the layout of
    include/hydra_hip.h (into `out` if given).  A sixth element is the row's min_p (word 3, fp32 bits: read by
    hx_sample_rows_constrained only); a five-element record packs it as 0."""
    rows = len(records)
    if out is None:
        out = np.zeros((rows, SAMPLE_RECORD_WORDS), dtype=np.int32)
    out[:, :2] = np.asarray([(r[0], r[1]) for r in records], dtype=np.float32).reshape(rows, 2).view(np.int32)
    out[:, 2] = [r[2] for r in records]
    out[:, 3] = np.asarray([r[5] if len(r) > 5 else 0.0 for r in records], dtype=np.float32).view(np.int32)
    out[:, 4:].view(np.uint64)[:] = np.asarray([(r[3], r[4]) for r in records], dtype=np.uint64).reshape(rows, 2)
    return out


def pack_resident_records(records, out: Optional[np.ndarray] = None) -> np.ndarray:
    """records: per launch row None (the greedy record) or (temperature, top_p, top_k, seed, offset_base) -> int32
    [rows, 8], the layout hx_sample_rows_resident reads (into `out` if given): `pack_sample_records`' with words [6] and
    [7] holding offset_base as a 64-bit two's-complement number — the row then draws with offset_base + its position,
    so a decode request's record is (.., n_out - position) for as long as it lives.  Word [3] is 0."""
    rows = len(records)
    if out is None:
        out = np.zeros((rows, SAMPLE_RECORD_WORDS), dtype=np.int32)
    recs = [GREEDY_RECORD if r is None else r for r in records]
    out[:, :2] = np.asarray([(r[0], r[1]) for r in recs], dtype=np.float32).reshape(rows, 2).view(np.int32)
    out[:, 2] = [r[2] for r in recs]
    out[:, 3] = 0
    wide = out[:, 4:].view(np.int64)
    wide[:, 0] = [r[3] for r in recs]           # (a seed is at most 2^63 - 1)
    wide[:, 1] = [r[4] for r in recs]
    return out


def sample_rows_resident(logits: Tensor, sample_params: Tensor, positions: Tensor, out: Optional[Tensor] = None,
                         cut_out: Optional[Tensor] = None, u_out: Optional[Tensor] = None) -> Tensor:
    """`sample_rows` without a history for records that stay on the device (include/hydra_hip.h:
    hx_sample_rows_resident): sample_params int32 [rows, 8] from `pack_resident_records`, positions int32 [rows]; row r
    draws with offset = its record's offset_base + positions[r].  Ids, cut and u are `sample_rows`' for a record that
    carries that offset, bit for bit.  Nothing here allocates when `out` is given: the launch a captured decode step
    ends in."""
    _lib.require_gpu(logits, sample_params, positions, out, cut_out, u_out)
    rows, _, out = _check_sample_arguments("sample_rows_resident", logits, sample_params, None, None, None, None, out, cut_out,
                                           u_out)
    if positions.dtype != torch.int32 or tuple(positions.shape) != (rows,) or not positions.is_contiguous():
        raise _lib.HydraHipError(f"sample_rows_resident: positions must be a contiguous int32 tensor of shape [{rows}]")
    _lib.check(_lib.lib().hx_sample_rows_resident(
        out.data_ptr(), cut_out.data_ptr() if cut_out is not None else None, u_out.data_ptr() if u_out is not None else None,
        logits.data_ptr(), rows, logits.shape[1], logits.stride(0), sample_params.data_ptr(), positions.data_ptr(),
        _lib.dtype_code(logits), _lib.current_stream()), "sample_rows_resident")
    return out


def pack_penalty_records(rows, out: Optional[np.ndarray] = None) -> np.ndarray:
    """rows: per launch row None — no penalties, no log slot: (0, 0, 1.0, -1) — or (frequency, presence, repetition, slot)
    -> int32 [rows, 4], the layout hx_sample_rows_resident_penalized reads (into `out` if given): the three penalties as
    fp32 bits, then the row's slot of the resident token log (negative: none)."""
    n = len(rows)
    if out is None:
        out = np.zeros((n, PENALTY_RECORD_WORDS), dtype=np.int32)
    recs = [NO_PENALTIES + (-1,) if r is None else r for r in rows]
    out[:, :3] = np.asarray([r[:3] for r in recs], dtype=np.float32).reshape(n, 3).view(np.int32)
    out[:, 3] = [r[3] for r in recs]
    return out


def sample_rows_resident_penalized(logits: Tensor, sample_params: Tensor, positions: Tensor, penalty_params: Tensor,
                                   token_log: Tensor, out: Optional[Tensor] = None, cut_out: Optional[Tensor] = None,
                                   u_out: Optional[Tensor] = None) -> Tensor:
    """`sample_rows_resident` under penalties over a resident token log (include/hydra_hip.h:
    hx_sample_rows_resident_penalized): penalty_params int32 [rows, 4] from `pack_penalty_records`, token_log int32
    [log_slots, log_cap] on the device (log_cap <= SAMPLE_LOG_MAX).  A row with a slot is penalised over the slot's first
    L words, L = its record's offset_base + its position, and writes its id as word L; a row without one is
    `sample_rows_resident`'s.  Nothing here allocates when `out` is given."""
    _lib.require_gpu(logits, sample_params, positions, penalty_params, token_log, out, cut_out, u_out)
    what = "sample_rows_resident_penalized"
    rows, _, out = _check_sample_arguments(what, logits, sample_params, None, None, None, None, out, cut_out, u_out)
    if positions.dtype != torch.int32 or tuple(positions.shape) != (rows,) or not positions.is_contiguous():
        raise _lib.HydraHipError(f"{what}: positions must be a contiguous int32 tensor of shape [{rows}]")
    if penalty_params.dtype != torch.int32 or tuple(penalty_params.shape) != (rows, PENALTY_RECORD_WORDS) \
            or not penalty_params.is_contiguous():
        raise _lib.HydraHipError(f"{what}: penalty_params must be a contiguous int32 tensor of shape "
                                 f"[{rows}, {PENALTY_RECORD_WORDS}]")
    if token_log.dtype != torch.int32 or token_log.dim() != 2 or not token_log.is_contiguous() or token_log.shape[0] < 1 \
            or not 1 <= token_log.shape[1] <= SAMPLE_LOG_MAX:
        raise _lib.HydraHipError(f"{what}: token_log must be a contiguous int32 tensor [log_slots >= 1, 1 <= log_cap <= "
                                 f"{SAMPLE_LOG_MAX}]")
    _lib.check(_lib.lib().hx_sample_rows_resident_penalized(
        out.data_ptr(), cut_out.data_ptr() if cut_out is not None else None, u_out.data_ptr() if u_out is not None else None,
        logits.data_ptr(), rows, logits.shape[1], logits.stride(0), sample_params.data_ptr(), positions.data_ptr(),
        penalty_params.data_ptr(), token_log.data_ptr(), token_log.shape[0], token_log.shape[1], _lib.dtype_code(logits),
        _lib.current_stream()), what)
    return out


class SampleStep(_PackedStep):
    """A sampled step's packed tables: one int32 host buffer [records (8 rows) | cu_hist (rows + 1) | penalties (3 rows,
    fp32 bits) | hist_ids (total) | hist_counts (total)] — `views` cuts it (on the host or on the device) into
    sample_rows' five table arguments."""
    __slots__ = ("buffer", "rows", "total")

    def __init__(self, buffer: np.ndarray, rows: int, total: int):
        self.buffer, self.rows, self.total = buffer, rows, total

    def views(self, t: Optional[Tensor] = None):
        """(sample_params, hist_ids, hist_counts, cu_hist, penalties) inside `t`, a tensor holding the buffer (default: a
        host copy)."""
        if t is None:
            t = torch.from_numpy(self.buffer)
        r = SAMPLE_RECORD_WORDS * self.rows
        a, b = r + self.rows + 1, r + 4 * self.rows + 1
        return (t[:r].view(self.rows, SAMPLE_RECORD_WORDS), t[b:b + self.total], t[b + self.total:b + 2 * self.total],
                t[r:a], t[a:b].view(torch.float32).view(self.rows, 3))


def pack_sample_step(entries) -> SampleStep:
    """entries: one (PenaltyHistory or None, (frequency, presence, repetition), (temperature, top_p, top_k, seed,
    offset)) per logits row, in row order.  The rows' records come first (8-byte aligned: the seeds are 64-bit), the
    layout of `pack_penalty_step` follows."""
    rows = len(entries)
    tables = pack_penalty_step([(h, p) for h, p, _ in entries])
    r = SAMPLE_RECORD_WORDS * rows
    buf = np.empty(r + tables.buffer.size, dtype=np.int32)
    pack_sample_records([rec for _, _, rec in entries], buf[:r].reshape(rows, SAMPLE_RECORD_WORDS))
    buf[r:] = tables.buffer
    return SampleStep(buf, rows, tables.total)


# ---- token constraints: logit_bias, min_tokens, min_p (hx_sample_rows_constrained, include/hydra_hip.h) ----
MAX_LOGIT_BIAS = 300            # entries of one request's logit_bias (OpenAI's limit)
LOGIT_BIAS_RANGE = 100.0        # |bias| at most this (OpenAI's range)


def _check_bias_arguments(what: str, logits, rows, bias_ids, bias_values, cu_bias) -> int:
    """The checks of the bias CSR that sample_rows_constrained and sample_rows_logprobs share -> bias_total."""
    bias_total = bias_ids.numel()
    for name, t, dtype, shape in (("bias_ids", bias_ids, torch.int32, (bias_total,)),
                                  ("bias_values", bias_values, torch.float32, (bias_total,)),
                                  ("cu_bias", cu_bias, torch.int32, (rows + 1,))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != logits.device:
            raise _lib.HydraHipError(f"{what}: {name} must be a contiguous {str(dtype)[6:]} tensor of shape "
                                     f"{list(shape)} on the logits' device")
    return bias_total


def sample_rows_constrained(logits: Tensor, sample_params: Tensor, bias_ids: Tensor, bias_values: Tensor, cu_bias: Tensor,
                            hist_ids: Optional[Tensor] = None, hist_counts: Optional[Tensor] = None,
                            cu_hist: Optional[Tensor] = None, penalties: Optional[Tensor] = None,
                            out: Optional[Tensor] = None, cut_out: Optional[Tensor] = None,
                            u_out: Optional[Tensor] = None) -> Tensor:
    """`sample_rows` under per-row token constraints, still one launch (include/hydra_hip.h: hx_sample_rows_constrained).
    bias_ids int32 [bias_total], bias_values fp32 [bias_total], cu_bias int32 [rows + 1]: the rows' (token, bias) tables
    as a CSR, ids within a row pairwise distinct; a bias is added to the fp32 logit BEFORE the penalties, -inf bans the
    token.  Word 3 of a row's record is its min_p (`pack_sample_records` with six-element records).  Everything else is
    `sample_rows`': a row with an empty table and min_p 0 gets its id, cut and u bit for bit."""
    _lib.require_gpu(logits, sample_params, bias_ids, bias_values, cu_bias, hist_ids, hist_counts, cu_hist, penalties, out,
                     cut_out, u_out)
    rows, total, out = _check_sample_arguments("sample_rows_constrained", logits, sample_params, hist_ids, hist_counts, cu_hist,
                                               penalties, out, cut_out, u_out)
    bias_total = _check_bias_arguments("sample_rows_constrained", logits, rows, bias_ids, bias_values, cu_bias)
    ptr = (lambda t: t.data_ptr()) if total else (lambda t: None)
    bptr = (lambda t: t.data_ptr()) if bias_total else (lambda t: None)
    _lib.check(_lib.lib().hx_sample_rows_constrained(
        out.data_ptr(), cut_out.data_ptr() if cut_out is not None else None, u_out.data_ptr() if u_out is not None else None,
        logits.data_ptr(), rows, logits.shape[1], logits.stride(0), ptr(hist_ids), ptr(hist_counts), ptr(cu_hist), total,
        ptr(penalties), bptr(bias_ids), bptr(bias_values), bptr(cu_bias), bias_total, sample_params.data_ptr(),
        _lib.dtype_code(logits), _lib.current_stream()), "sample_rows_constrained")
    return out


def sample_rows_logprobs(logits: Tensor, sample_params: Tensor, bias_ids: Tensor, bias_values: Tensor, cu_bias: Tensor,
                         hist_ids: Optional[Tensor] = None, hist_counts: Optional[Tensor] = None,
                         cu_hist: Optional[Tensor] = None, penalties: Optional[Tensor] = None, *, top_k: int,
                         want: Optional[Tensor] = None, out: Optional[Tensor] = None, cut_out: Optional[Tensor] = None,
                         u_out: Optional[Tensor] = None):
    """`sample_rows_constrained` that also scores its choice, still one launch (include/hydra_hip.h:
    hx_sample_rows_logprobs).  Returns (ids int64 [rows] — sample_rows_constrained's, bit for bit —, logprobs fp32 [rows],
    top_ids int32 [rows, K], top_logprobs fp32 [rows, K]): the log-probability of each id under the distribution the
    row's choice rule picks from (after bias, penalties, temperature, top-k, min_p and top-p, renormalised over the kept
    set; a greedy row: the softmax of its biased, penalised logits), and the top_k (0..20) most likely tokens of that
    distribution, -inf for one the truncation dropped.  want: None (every row is scored) or int32 [rows]; a row with
    want < 0 is not scored (NaN, -1, NaN) and costs what it costs in sample_rows_constrained.  The four results are views
    of one uint8 buffer with logprob_rows' layout (`out`, or a new one: logprob_rows_bytes / logprob_rows_views), which
    goes to the host in one copy (logprob_rows_packed)."""
    from hydrainfer_amd._C.kernel.norm import LOGPROB_MAX_TOP_K, logprob_rows_bytes, logprob_rows_views
    _lib.require_gpu(logits, sample_params, bias_ids, bias_values, cu_bias, hist_ids, hist_counts, cu_hist, penalties, want,
                     out, cut_out, u_out)
    what = "sample_rows_logprobs"
    if not isinstance(top_k, int) or isinstance(top_k, bool) or not 0 <= top_k <= LOGPROB_MAX_TOP_K:
        raise _lib.HydraHipError(f"{what}: top_k {top_k!r} outside 0..{LOGPROB_MAX_TOP_K}")
    rows, total, _ = _check_sample_arguments(what, logits, sample_params, hist_ids, hist_counts, cu_hist, penalties, None,
                                             cut_out, u_out, ids_in_packed=True)
    bias_total = _check_bias_arguments(what, logits, rows, bias_ids, bias_values, cu_bias)
    if want is not None and (want.dtype != torch.int32 or tuple(want.shape) != (rows,) or not want.is_contiguous()
                             or want.device != logits.device):
        raise _lib.HydraHipError(f"{what}: want must be a contiguous int32 tensor of shape [{rows}] on the logits' device")
    if out is None:
        out = torch.empty(logprob_rows_bytes(rows, top_k), dtype=torch.uint8, device=logits.device)
    elif out.device != logits.device or out.data_ptr() % 8:
        raise _lib.HydraHipError(f"{what}: out must be an 8-byte aligned buffer on the logits' device")
    ids, lp, top_ids, top_lp = logprob_rows_views(out, rows, top_k)
    ptr = (lambda t: t.data_ptr()) if total else (lambda t: None)
    bptr = (lambda t: t.data_ptr()) if bias_total else (lambda t: None)
    _lib.check(_lib.lib().hx_sample_rows_logprobs(
        ids.data_ptr(), cut_out.data_ptr() if cut_out is not None else None, u_out.data_ptr() if u_out is not None else None,
        logits.data_ptr(), rows, logits.shape[1], logits.stride(0), ptr(hist_ids), ptr(hist_counts), ptr(cu_hist), total,
        ptr(penalties), bptr(bias_ids), bptr(bias_values), bptr(cu_bias), bias_total, sample_params.data_ptr(),
        lp.data_ptr(), top_ids.data_ptr() if top_k else None, top_lp.data_ptr() if top_k else None, top_k,
        want.data_ptr() if want is not None else None, _lib.dtype_code(logits), _lib.current_stream()), what)
    return ids, lp, top_ids, top_lp


def check_constraints(logit_bias, min_tokens, min_p):
    """(logit_bias, min_tokens, min_p) checked, or ValueError.  logit_bias: None or a mapping from int token id >= 0 to
    a finite number in -100 .. 100, at most MAX_LOGIT_BIAS entries (returned as a {int: float} dict, None when empty);
    min_tokens an integer >= 0; min_p a number in [0, 1].  A bool is no number."""
    bias = None
    if logit_bias is not None:
        if not hasattr(logit_bias, "items"):
            raise ValueError(f"logit_bias {logit_bias!r} must be a mapping from token id to bias")
        if len(logit_bias) > MAX_LOGIT_BIAS:
            raise ValueError(f"logit_bias has {len(logit_bias)} entries, at most {MAX_LOGIT_BIAS} are taken")
        bias = {}
        for t, b in logit_bias.items():
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t <= 0x7fffffff:
                raise ValueError(f"logit_bias: token id {t!r} must be an integer >= 0")
            if isinstance(b, bool) or not isinstance(b, (int, float)) or not math.isfinite(b) or abs(b) > LOGIT_BIAS_RANGE:
                raise ValueError(f"logit_bias: the bias {b!r} of token {t} must be a finite number in "
                                 f"-{LOGIT_BIAS_RANGE:g} .. {LOGIT_BIAS_RANGE:g}")
            bias[t] = float(b)
        bias = bias or None
    if isinstance(min_tokens, bool) or not isinstance(min_tokens, int) or min_tokens < 0:
        raise ValueError(f"min_tokens {min_tokens!r} must be an integer >= 0")
    if isinstance(min_p, bool) or not isinstance(min_p, (int, float)) or not 0 <= min_p <= 1:      # (a NaN fails both)
        raise ValueError(f"min_p {min_p!r} must be a number in [0, 1]")
    return bias, min_tokens, float(min_p)


def is_constrained(sampling_params) -> bool:
    """True when one of logit_bias, min_tokens, min_p changes what the request may emit: a non-empty logit_bias, min_p > 0
    on a sampled request (a greedy row ignores it), min_tokens > 0 with an end-of-sequence id to hold back.  False: the
    request takes exactly the paths it took before these fields existed."""
    sp = sampling_params
    return bool(sp.logit_bias) or (sp.min_p > 0 and sp.temperature > 0) or (sp.min_tokens > 0 and bool(sp.eos_token_ids))


class TokenConstraints:
    """A request's constraints on the host.  `ids` / `values`: its static bias table as sorted, pairwise distinct int32 /
    fp32 arrays; `eos_ids`: its end-of-sequence ids (sorted, distinct); `min_tokens`: while fewer tokens have been
    generated, every one of them is banned (a bias of -inf)."""
    __slots__ = ("ids", "values", "eos_ids", "min_tokens", "_held")

    def __init__(self, logit_bias=None, eos_token_ids: Sequence[int] = (), min_tokens: int = 0):
        items = sorted((logit_bias or {}).items())
        self.ids = np.asarray([t for t, _ in items], dtype=np.int32)
        self.values = np.asarray([b for _, b in items], dtype=np.float32)
        self.eos_ids = sorted(set(int(t) for t in eos_token_ids))
        self.min_tokens = min_tokens
        self._held = None         # the table with the bans merged in, built on first use

    def step_entries(self, n_generated: int) -> Tuple[np.ndarray, np.ndarray]:
        """(ids, values) of the row for the step that generates token number n_generated (0: the first).  While
        n_generated < min_tokens the ban of an end-of-sequence id REPLACES a finite bias on the same id: ids stay
        distinct (and sorted)."""
        if n_generated >= self.min_tokens or not self.eos_ids:
            return self.ids, self.values
        if self._held is None:
            table = dict(zip(self.ids.tolist(), self.values.tolist()))
            table.update((t, -math.inf) for t in self.eos_ids)
            items = sorted(table.items())
            self._held = (np.asarray([t for t, _ in items], dtype=np.int32),
                          np.asarray([b for _, b in items], dtype=np.float32))
        return self._held


class ConstrainedStep(_PackedStep):
    """A constrained step's packed tables: SampleStep's buffer with [cu_bias (rows + 1) | bias_ids (bias_total) |
    bias_values (bias_total, fp32 bits)] appended — `views` cuts it (on the host or on the device) into
    sample_rows_constrained's eight table arguments."""
    __slots__ = ("buffer", "rows", "total", "bias_total")

    def __init__(self, buffer: np.ndarray, rows: int, total: int, bias_total: int):
        self.buffer, self.rows, self.total, self.bias_total = buffer, rows, total, bias_total

    def views(self, t: Optional[Tensor] = None):
        """(sample_params, bias_ids, bias_values, cu_bias, hist_ids, hist_counts, cu_hist, penalties) inside `t`, a tensor
        holding the buffer (default: a host copy)."""
        if t is None:
            t = torch.from_numpy(self.buffer)
        c = (SAMPLE_RECORD_WORDS + 4) * self.rows + 1 + 2 * self.total           # where SampleStep's layout ends
        d = c + self.rows + 1
        records, hist_ids, hist_counts, cu_hist, penalties = SampleStep(None, self.rows, self.total).views(t[:c])
        return (records, t[d:d + self.bias_total], t[d + self.bias_total:d + 2 * self.bias_total].view(torch.float32),
                t[c:d], hist_ids, hist_counts, cu_hist, penalties)


def pack_constrained_step(entries) -> ConstrainedStep:
    """entries: one (PenaltyHistory or None, (frequency, presence, repetition), record, bias) per logits row, in row
    order — record: (temperature, top_p, top_k, seed, offset[, min_p]); bias: None or the (ids, values) arrays of
    `TokenConstraints.step_entries`."""
    rows = len(entries)
    step = pack_sample_step([(h, p, rec) for h, p, rec, _ in entries])
    lens = [len(b[0]) if b is not None else 0 for _, _, _, b in entries]
    bias_total = sum(lens)
    c = step.buffer.size
    buf = np.empty(c + rows + 1 + 2 * bias_total, dtype=np.int32)
    buf[:c] = step.buffer
    buf[c] = 0
    np.cumsum(lens, out=buf[c + 1:c + rows + 1])
    at = c + rows + 1
    for (_, _, _, b), n in zip(entries, lens):
        if n:
            buf[at:at + n] = np.asarray(b[0], dtype=np.int32)
            buf[at + bias_total:at + bias_total + n] = np.asarray(b[1], dtype=np.float32).view(np.int32)
            at += n
    return ConstrainedStep(buf, rows, step.total, bias_total)


# ---- token masks: allowed_token_ids, guided_choice (hx_sample_rows_masked, include/hydra_hip.h) ----
MAX_GUIDED_CHOICES = 64         # choices of one request's guided_choice
MAX_CHOICE_TOKENS = 64          # token ids of one choice


def mask_words(n: int) -> int:
    """The int32 words of one mask over n tokens: 32 tokens per word."""
    return (n + 31) // 32


def pack_mask_words(token_ids, n: int) -> np.ndarray:
    """token_ids: distinct integers in 0 .. n - 1 -> uint32 [(n + 31) // 32], the format grammar engines exchange: bit
    t & 31 of word t >> 5 is set when token t may be chosen; no bit at or above n is set.  ValueError otherwise."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"pack_mask_words: n {n!r} must be an integer >= 1")
    ids = list(token_ids)
    for t in ids:
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) or not 0 <= t < n:
            raise ValueError(f"pack_mask_words: token id {t!r} must be an integer in 0 .. {n - 1}")
    if len(set(int(t) for t in ids)) != len(ids):
        raise ValueError("pack_mask_words: a token id stands twice")
    words = np.zeros(mask_words(n), dtype=np.uint32)
    if ids:
        t = np.asarray(ids, dtype=np.int64)
        np.bitwise_or.at(words, t >> 5, np.left_shift(np.uint32(1), (t & 31).astype(np.uint32)))
    return words


def check_token_mask(allowed_token_ids, guided_choice, vocab_size: int):
    """(allowed_token_ids, guided_choice) checked against the vocabulary, as lists of ints (None where not given), or
    ValueError: both at once; allowed_token_ids not a non-empty list of distinct integers in 0 .. vocab_size - 1 (a bool
    is no integer); guided_choice not 1..MAX_GUIDED_CHOICES distinct sequences of 1..MAX_CHOICE_TOKENS such ids (within
    a choice an id may repeat), or a choice that is a prefix of another: the trie would have to decide between stopping
    and going on."""
    if allowed_token_ids is None and guided_choice is None:
        return None, None
    if allowed_token_ids is not None and guided_choice is not None:
        raise ValueError("allowed_token_ids and guided_choice cannot be combined: a request takes one of them")
    if isinstance(vocab_size, bool) or not isinstance(vocab_size, int) or vocab_size < 1:
        raise ValueError("allowed_token_ids / guided_choice need the size of the vocabulary the model scores")

    def ids_of(what, seq, most=None):
        if not isinstance(seq, (list, tuple)) or not seq or (most is not None and len(seq) > most):
            raise ValueError(f"{what} must be a list of 1{'' if most is None else f'..{most}'} token ids")
        for t in seq:
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < vocab_size:
                raise ValueError(f"{what}: token id {t!r} must be an integer in 0 .. {vocab_size - 1}")
        return list(seq)

    if allowed_token_ids is not None:
        allowed = ids_of("allowed_token_ids", allowed_token_ids)
        if len(set(allowed)) != len(allowed):
            raise ValueError("allowed_token_ids: a token id stands twice")
        return allowed, None
    if not isinstance(guided_choice, (list, tuple)) or not 1 <= len(guided_choice) <= MAX_GUIDED_CHOICES:
        raise ValueError(f"guided_choice must be a list of 1..{MAX_GUIDED_CHOICES} token id sequences")
    choices = [ids_of(f"guided_choice[{i}]", c, MAX_CHOICE_TOKENS) for i, c in enumerate(guided_choice)]
    if len(set(tuple(c) for c in choices)) != len(choices):
        raise ValueError("guided_choice: a choice stands twice")
    ordered = sorted(choices)                   # a prefix sorts directly in front of one of its extensions
    for a, b in zip(ordered, ordered[1:]):
        if b[:len(a)] == a:
            raise ValueError(f"guided_choice: {a} is a prefix of {b}: the request could not tell stopping from going on")
    return None, choices


class TokenMask:
    """A request's token masks and where it stands in them, on the host; built ONCE, at admission.  allowed_token_ids:
    one node whose mask holds every step, never finished.  guided_choice: a trie over the choices' token sequences, the
    mask of a node being its children's ids; `advance` follows the delivered token to the child and `finished` turns
    true at a leaf — the end of exactly one choice, no choice being a prefix of another (check_token_mask).
    `current()` is the SAME array object every time for the same node: a step deduplicates masks by identity."""
    __slots__ = ("n", "words", "children", "node", "finished")

    def __init__(self, n: int, allowed_token_ids=None, guided_choice=None):
        if (allowed_token_ids is None) == (guided_choice is None):
            raise ValueError("TokenMask: one of allowed_token_ids and guided_choice")
        self.n, self.node, self.finished = n, 0, False
        if allowed_token_ids is not None:
            self.words, self.children = [pack_mask_words(allowed_token_ids, n)], None
            return
        children = [{}]                         # per node: token -> child node
        for choice in guided_choice:
            at = 0
            for t in choice:
                nxt = children[at].get(t)
                if nxt is None:
                    nxt = children[at][t] = len(children)
                    children.append({})
                at = nxt
        self.children = children
        self.words = [pack_mask_words(c.keys(), n) if c else None for c in children]

    def current(self) -> np.ndarray:
        """The mask words (uint32 [(n + 31) // 32]) of the node the request stands on."""
        if self.finished:
            raise ValueError("TokenMask: the choice is complete, nothing more may be chosen")
        return self.words[self.node]

    def advance(self, token: int) -> None:
        """The request delivered `token`: on to the child (allowed_token_ids: the one node stays)."""
        if self.children is None:
            return
        nxt = self.children[self.node].get(token) if not self.finished else None
        if nxt is None:
            raise ValueError(f"TokenMask: token {token!r} is not among the tokens the request may choose here")
        self.node = nxt
        self.finished = not self.children[nxt]


def sample_rows_masked(logits: Tensor, sample_params: Tensor, bias_ids: Tensor, bias_values: Tensor, cu_bias: Tensor,
                       allow_words: Tensor, mask_row: Tensor, hist_ids: Optional[Tensor] = None,
                       hist_counts: Optional[Tensor] = None, cu_hist: Optional[Tensor] = None,
                       penalties: Optional[Tensor] = None, *, top_k: Optional[int] = None, want: Optional[Tensor] = None,
                       out: Optional[Tensor] = None, cut_out: Optional[Tensor] = None, u_out: Optional[Tensor] = None):
    """`sample_rows_constrained` / `sample_rows_logprobs` under per-row token masks, still one launch
    (include/hydra_hip.h: hx_sample_rows_masked).  allow_words: int32 / uint32 [n_masks, (n + 31) // 32], bit t & 31 of
    word t >> 5 of a mask set when token t may be chosen (`pack_mask_words`); mask_row int32 [rows]: the index of the
    row's mask, < 0 or >= n_masks for a row without one.  A masked row gives bit for bit what the sibling gives for the
    same row with -inf written into the logits at the tokens its mask leaves out; an unmasked row what it gives there.
    top_k None: unscored, returns ids int64 [rows] (`out` if given) as sample_rows_constrained does.  Otherwise
    sample_rows_logprobs' four views over the packed layout, `want` as there."""
    from hydrainfer_amd._C.kernel.norm import LOGPROB_MAX_TOP_K, logprob_rows_bytes, logprob_rows_views
    _lib.require_gpu(logits, sample_params, bias_ids, bias_values, cu_bias, allow_words, mask_row, hist_ids, hist_counts,
                     cu_hist, penalties, want, out, cut_out, u_out)
    what = "sample_rows_masked"
    scored = top_k is not None
    if scored and (not isinstance(top_k, int) or isinstance(top_k, bool) or not 0 <= top_k <= LOGPROB_MAX_TOP_K):
        raise _lib.HydraHipError(f"{what}: top_k {top_k!r} outside 0..{LOGPROB_MAX_TOP_K}")
    if not scored and want is not None:
        raise _lib.HydraHipError(f"{what}: want comes with top_k (an unscored launch scores no row)")
    rows, total, ids = _check_sample_arguments(what, logits, sample_params, hist_ids, hist_counts, cu_hist, penalties,
                                               None if scored else out, cut_out, u_out, ids_in_packed=scored)
    bias_total = _check_bias_arguments(what, logits, rows, bias_ids, bias_values, cu_bias)
    words = mask_words(logits.shape[1])
    if allow_words.dtype not in (torch.int32, torch.uint32) or allow_words.dim() != 2 or not allow_words.is_contiguous() \
            or (allow_words.shape[0] > 0 and allow_words.shape[1] != words) or allow_words.device != logits.device:
        raise _lib.HydraHipError(f"{what}: allow_words must be a contiguous int32 / uint32 tensor of shape [n_masks, {words}] "
                                 "on the logits' device")
    n_masks = allow_words.shape[0]
    for name, t in (("mask_row", mask_row), ("want", want)):
        if (t is not None or name == "mask_row") and (t.dtype != torch.int32 or tuple(t.shape) != (rows,)
                                                      or not t.is_contiguous() or t.device != logits.device):
            raise _lib.HydraHipError(f"{what}: {name} must be a contiguous int32 tensor of shape [{rows}] on the logits' "
                                     "device")
    lp = top_ids = top_lp = None
    if scored:
        if out is None:
            out = torch.empty(logprob_rows_bytes(rows, top_k), dtype=torch.uint8, device=logits.device)
        elif out.device != logits.device or out.data_ptr() % 8:
            raise _lib.HydraHipError(f"{what}: out must be an 8-byte aligned buffer on the logits' device")
        ids, lp, top_ids, top_lp = logprob_rows_views(out, rows, top_k)
    ptr = (lambda t: t.data_ptr()) if total else (lambda t: None)
    bptr = (lambda t: t.data_ptr()) if bias_total else (lambda t: None)
    _lib.check(_lib.lib().hx_sample_rows_masked(
        ids.data_ptr(), cut_out.data_ptr() if cut_out is not None else None, u_out.data_ptr() if u_out is not None else None,
        logits.data_ptr(), rows, logits.shape[1], logits.stride(0), ptr(hist_ids), ptr(hist_counts), ptr(cu_hist), total,
        ptr(penalties), bptr(bias_ids), bptr(bias_values), bptr(cu_bias), bias_total, sample_params.data_ptr(),
        lp.data_ptr() if scored else None, top_ids.data_ptr() if scored and top_k else None,
        top_lp.data_ptr() if scored and top_k else None, top_k if scored else 0,
        want.data_ptr() if want is not None else None, allow_words.data_ptr() if n_masks else None, n_masks,
        mask_row.data_ptr(), _lib.dtype_code(logits), _lib.current_stream()), what)
    return (ids, lp, top_ids, top_lp) if scored else ids


class MaskedStep(_PackedStep):
    """A masked step's packed tables: ConstrainedStep's buffer with [want (rows) | mask_row (rows) | the step's distinct
    masks (n_masks * words)] appended — `views` cuts it (on the host or on the device) into sample_rows_masked's table
    arguments, in its order, with `want` last."""
    __slots__ = ("buffer", "rows", "total", "bias_total", "n_masks", "words")

    def __init__(self, buffer: np.ndarray, rows: int, total: int, bias_total: int, n_masks: int, words: int):
        self.buffer, self.rows, self.total, self.bias_total = buffer, rows, total, bias_total
        self.n_masks, self.words = n_masks, words

    def views(self, t: Optional[Tensor] = None):
        """(sample_params, bias_ids, bias_values, cu_bias, allow_words, mask_row, hist_ids, hist_counts, cu_hist,
        penalties, want) inside `t`, a tensor holding the buffer (default: a host copy)."""
        if t is None:
            t = torch.from_numpy(self.buffer)
        e = t.numel() - 2 * self.rows - self.n_masks * self.words                # where ConstrainedStep's layout ends
        records, bias_ids, bias_values, cu_bias, hist_ids, hist_counts, cu_hist, penalties = \
            ConstrainedStep(None, self.rows, self.total, self.bias_total).views(t[:e])
        m = e + 2 * self.rows
        return (records, bias_ids, bias_values, cu_bias, t[m:].view(self.n_masks, self.words), t[e + self.rows:m],
                hist_ids, hist_counts, cu_hist, penalties, t[e:e + self.rows])


def pack_masked_step(entries) -> MaskedStep:
    """entries: one (PenaltyHistory or None, (frequency, presence, repetition), record, bias, want, mask) per logits row,
    in row order — the first four as in `pack_constrained_step`; want: < 0 for a row that is not scored; mask: None or
    the words of `TokenMask.current()`.  Rows that hand in the SAME array (two requests on one node, one request's node
    step after step) share one mask of the step: masks are told apart by identity, not by content."""
    rows = len(entries)
    step = pack_constrained_step([e[:4] for e in entries])
    slot, masks = {}, []
    mask_row = np.full(rows, -1, dtype=np.int32)
    for r, e in enumerate(entries):
        mask = e[5]
        if mask is not None:
            j = slot.get(id(mask))
            if j is None:
                j = slot[id(mask)] = len(masks)
                masks.append(mask)
            mask_row[r] = j
    words = len(masks[0]) if masks else 0
    if any(len(m) != words for m in masks):
        raise ValueError("pack_masked_step: the step's masks differ in width")
    c = step.buffer.size
    buf = np.empty(c + 2 * rows + len(masks) * words, dtype=np.int32)
    buf[:c] = step.buffer
    buf[c:c + rows] = [e[4] for e in entries]
    buf[c + rows:c + 2 * rows] = mask_row
    at = c + 2 * rows
    for m in masks:
        buf[at:at + words] = np.asarray(m, dtype=np.uint32).view(np.int32)
        at += words
    return MaskedStep(buf, rows, step.total, step.bias_total, len(masks), words)
