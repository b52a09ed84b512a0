"""hydrainfer.sampling — counterpart of the reference's hydrainfer/sampling/logits_processor.py for a greedy engine.

Of `process_logits` (logits_processor.py:49-93) only steps 1-2, the frequency / presence / repetition penalties
(lines 65-72), can change the token a greedy sampler picks: a positive temperature keeps the order of the logits, top-k
and top-p mask entries below the maximum.  `penalized_argmax_rows` (hx_penalized_argmax_rows, csrc/penalties.hip) is
those two steps and the argmax in one launch behind the logits.

The history.  The reference's processor takes one table of (token, count) per sequence and leaves open what goes into
it.  Here it holds the GENERATED tokens only, for all three penalties: prompts contain image placeholders (hundreds of
copies of one id) and chat-template tokens, which a prompt-inclusive repetition penalty would push down; OpenAI's
frequency / presence penalties are defined over the sampled text as well.  The first generated token therefore sees an
empty history.  `PenaltyHistory` is that table on the host, `pack_penalty_step` turns a step's tables into the kernel's
CSR — one buffer, one host-to-device copy."""
import math
from array import array
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from hydrainfer_amd import _lib

MAX_VOCAB = 1 << 18             # the widest row hx_penalized_argmax_rows takes (its LDS bitmap)
NO_PENALTIES = (0.0, 0.0, 1.0)  # (frequency, presence, repetition): the identity


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


class PenaltyStep:
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

    def to_device(self, device):
        """The four arguments on `device`: the buffer goes through pinned memory in ONE host-to-device copy."""
        host = torch.from_numpy(self.buffer)
        if torch.device(device).type == "cuda":
            host = host.pin_memory()
        return self.views(host.to(device, non_blocking=True))


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
