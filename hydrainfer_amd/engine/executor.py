"""Instruction executors — mirror of hydrainfer/engine/executor.py:82-299.

BatchFillExecutor: publish finished blocks to the prefix cache, build the step's inputs, run the
language model on the HIP path, hand each sampled token to its request.
BatchImageEmbedExecutor: run the vision tower + projector and scatter the embeddings into the
image cache.  Both run on the current stream; `InstructionExecutor` can put the vision side on
its own stream (executor.py:247-249)."""
import os
import time
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from hydrainfer_amd._C.kernel.norm import (argmax_rows, logprob_rows, logprob_rows_packed, logprob_rows_views,
                                           token_logprob_rows, token_logprob_rows_packed, token_logprob_rows_views)
from hydrainfer_amd._lib import HydraHipError

from hydrainfer_amd.engine import rcb as rcb_module
from hydrainfer_amd.engine.isa import Fill, TextFill
from hydrainfer_amd.engine.parameters_builder import LanguageModelParametersBuilder
from hydrainfer_amd.engine.rcb import PROCESSED_LOGPROBS, BatchRequest, PromptTokenLogprob, TokenLogprob
from hydrainfer_amd.model.llama import LanguageModelParameters
# (the packers and kernels are reached by name: SAMPLING_MODES)
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, pack_constrained_step, pack_masked_step, pack_penalty_step,
                                     pack_sample_step, penalized_argmax_rows, sample_rows, sample_rows_constrained,
                                     sample_rows_logprobs, sample_rows_masked)


# What the table-driven modes of the eager sampling step (BatchFillExecutor._sample) differ in: how many elements of a
# row's (history, penalties, record, bias) entry the packer takes, the packer, the language model's entry point (logits
# and launch in one call) and the kernel for logits that are already there.  NAMES, looked up when the step runs: tests
# patch executor.<kernel>, and a stand-in for the language model implements only the entry points its test needs.
SAMPLING_MODES = {
    "constrained": (4, "pack_constrained_step", "forward_constrained", "sample_rows_constrained"),
    "drawn": (3, "pack_sample_step", "forward_sampled", "sample_rows"),
    "penalised": (2, "pack_penalty_step", "forward_penalized", "penalized_argmax_rows"),
}


def sampling_rows(batch):
    """The (rcb, inst) pairs of a fill batch that sample a token, in the order of the step's sampled rows."""
    return [(rcb, inst) for rcb, inst in batch if isinstance(inst, Fill) and inst.sample]


def step_mode(rows):
    """rows: the sampling (rcb, inst) pairs of an eager step -> (mode, top_k).  mode: the first that some request asks
    for of "constrained" (logit_bias, min_tokens, min_p), "drawn" (temperature > 0), "penalised", "logprobs", else
    "plain"; each of the first three serves the requests of the modes after it in the same launch.  top_k: the largest
    top_logprobs among the requests that ask for log-probabilities and deliver a token this step (a chunk head's sample
    is discarded), None when there is none."""
    asking = [rcb.sampling_params.top_logprobs for rcb, inst in rows if rcb.sampling_params.logprobs and not inst.is_chunked]
    if any(rcb.token_constraints is not None for rcb, _ in rows):
        mode = "constrained"
    elif any(rcb.sampling_params.temperature > 0 for rcb, _ in rows):
        mode = "drawn"
    elif any(rcb.penalty_history is not None for rcb, _ in rows):
        mode = "penalised"
    else:
        mode = "logprobs" if asking else "plain"
    return mode, max(asking) if asking else None


def asks_processed(rcb) -> bool:
    """The request wants the scores of the distribution its tokens are chosen from (logprobs_mode =
    "processed_logprobs").  Read with a default: a stand-in for the parameters need not carry the field."""
    sp = rcb.sampling_params
    return bool(sp.logprobs) and getattr(sp, "logprobs_mode", None) == PROCESSED_LOGPROBS


def scored_rows(rows) -> bool:
    """rows: the sampling (rcb, inst) pairs of an eager step.  True when some request asks for processed
    log-probabilities and delivers a token this step (a chunk head's sample is discarded): the step then runs ONE
    hx_sample_rows_logprobs launch for the whole batch (BatchFillExecutor._sample_scored), whatever step_mode says —
    this decision is consulted first."""
    return any(asks_processed(rcb) and not inst.is_chunked for rcb, inst in rows)


def masked_rows(rows) -> bool:
    """rows: the sampling (rcb, inst) pairs of an eager step.  True when some request carries a token mask
    (allowed_token_ids, guided_choice) and delivers a token this step (a chunk head's sample is discarded): the step then
    runs ONE hx_sample_rows_masked launch for the whole batch (BatchFillExecutor._sample_masked) — consulted ahead of
    scored_rows.  Read with a default: a stand-in for a request need not carry the attribute."""
    return any(getattr(rcb, "token_mask", None) is not None and not inst.is_chunked for rcb, inst in rows)


class PendingToken:
    """Placeholder for a token that has been sampled on the device but not read back yet
    (graph decode look-ahead): row `row` of decode launch `launch`."""
    __slots__ = ("launch", "row")

    def __init__(self, launch: int, row: int):
        self.launch, self.row = launch, row

    def __repr__(self):
        return f"<pending {self.launch}:{self.row}>"


class DecodeStep(NamedTuple):
    """What BatchFillExecutor._decode_rows hands GraphedDecoder.launch."""
    rows: list
    records: Optional[list]
    penalties: Optional[list]


def decoder_abilities(dec):
    """-> (sampled, log_cap, has_cohort) of a graph decoder: it has a sampled variant; the token log's row when it has
    the penalised one as well, else 0; it has launch_cohort.  Read with defaults — a stand-in for the decoder need
    not carry the attributes — and at every use: tests replace the decoder of a built executor."""
    sampled = bool(getattr(dec, "sampled", False))
    return (sampled, dec.penalty_log_cap if sampled and getattr(dec, "penalized", False) else 0,
            hasattr(dec, "launch_cohort"))


class DecodeCohort:
    """The steady state of a decode batch — the SAME sequences step after step, each one token further — kept as arrays
    instead of being rediscovered from every request's instruction chain every step (the
    reference's per-step Python over every running request, hydrainfer/engine/scheduler.py:99-194 +
    parameters_builder.py:46-97, is what bounds a decode loop once the kernels are fast).  While the cohort lasts a step
    touches a request object only when it enters a new block or streams a token to a client; when it ends (anything
    else wants to happen: an arrival, a request about to finish, a cancelled stream) the requests are brought up to date
    in one pass and the general path goes on as if it had run every step itself."""

    def __init__(self, rcbs, running_ref, bs):
        n = self.n = len(rcbs)
        self.rcbs, self.running_ref, self.bs = rcbs, running_ref, bs
        self.pos = np.zeros(n, dtype=np.int32)          # rotary position of the NEXT launch's token, per row
        self.cid = np.zeros(n, dtype=np.int32)          # its virtual cache id
        self.left = np.zeros(n, dtype=np.int32)         # tokens the row has still to sample, the next launch's included
        self.nblk = np.zeros(n, dtype=np.int32)         # blocks in the row's table
        self.last_block = np.zeros(n, dtype=np.int32)   # the block the next cache id falls into (valid when cid // bs < nblk)
        self.starts = np.zeros(n, dtype=np.int32)       # the row's table offset in the decoder's resident buffer
        self.sids = [r.sid for r in rcbs]
        self.streams = [(i, r.output_token_processors) for i, r in enumerate(rcbs) if r.output_token_processors]
        self.first_inst = [r.current_instruction() for r in rcbs]
        self.eos_rows: List[int] = []                   # rows whose request names end-of-sequence ids
        self.k = 0                                      # cohort launches so far
        self.launch = None                              # the one in flight
        self.tok_log: List[List[int]] = []              # tokens of cohort launches 1 .. k - 1 (resolved)
        self.t_log: List[float] = []
        self.epoch = rcb_module.MUTATIONS[0]


class BatchFillExecutor:
    def __init__(self, language_model, kv_cache_block_manager, image_cache_block_manager,
                 dtype: torch.dtype, device: torch.device, graph_decoder=None):
        self.language_model = language_model            # LlavaLanguageModel
        lm = language_model.language_model
        self.shape = lm.shape
        self.kv_manager, self.image_manager = kv_cache_block_manager, image_cache_block_manager
        self.dtype, self.device = dtype, device
        self.graph_decoder = graph_decoder              # engine.graph_decode.GraphedDecoder or None
        self.pending = None        # (launch id, [(rcb, inst, index into rcb.output_token_ids)])
        self.cohort: Optional[DecodeCohort] = None
        self.cohort_enabled = os.environ.get("HX_DECODE_COHORT", "1") == "1"
        self.cohort_refused = None # the pending launch a cohort could not be formed behind (not tried again until the next one)
        self.n_cohort_steps = 0
        self.ended_rows: Optional[List] = None   # the rows of a cohort that ended inside its own step (an end-of-sequence id came back)

    def _decode_rows(self, batch: BatchRequest) -> Optional[DecodeStep]:
        """The step the captured decoder runs for this batch, or None: the batch runs eagerly (execute()).
        rows: (token, position, slot, kv_len, block_table, sid) per request; a token still on the device is encoded as
        -(row + 1) of the pending launch.  records (a decoder with a sampled variant, else None): per row None — greedy —
        or (temperature, top_p, top_k, seed, n_out - position): the decoder's launch adds the row's position, so the
        draw's offset is n_out, what the eager step computes (placeholders of tokens still on the device count in
        output_token_ids).  penalties (None unless some row is penalised): per row None or (frequency, presence,
        repetition, output_token_ids), the row's record carrying n_out - position for a greedy one too."""
        rows, records, penalties, max_blocks = [], [], [], 0
        bs = self.kv_manager.block_size
        pending_launch = self.pending[0] if self.pending is not None else None
        dec = self.graph_decoder
        sampled, log_cap, _ = decoder_abilities(dec)
        for rcb, inst in batch:
            sp = rcb.sampling_params
            penalised = rcb.penalty_history is not None
            # Who decodes from the captured step: a request that samples from ONE new token; without log-probabilities,
            # token constraints or a token mask (the eager sampling step's business), and not a one-token piece of a
            # prompt that is being scored (decode Fills carry no score list); a drawn one only with the sampled variant;
            # a penalised one only with the penalised variant and a max_tokens that fits a row of the token log —
            # decided once for its whole life
            if (len(inst.token_ids) != 1 or not inst.sample or sp.logprobs or inst.score_targets is not None
                    or rcb.token_constraints is not None or getattr(rcb, "token_mask", None) is not None
                    or (sp.temperature > 0 and not sampled)
                    or (penalised and not (log_cap and sp.max_tokens <= log_cap))):
                return None
            # a penalised row the log does not continue for is seeded from output_token_ids by the decoder: while a token
            # of it is still on the device the step runs eagerly (which reads the pending launch back first)
            if penalised and not dec.log_table.continues(rcb.sid, len(rcb.output_token_ids)) \
                    and any(isinstance(t, PendingToken) for t in rcb.output_token_ids):
                return None
            token = inst.token_ids[0]
            if isinstance(token, PendingToken):
                if token.launch != pending_launch:
                    return None
                token = -(token.row + 1)
            bt = rcb.virtual_kv_cache.block_table
            c = inst.cache_ids[0]
            position = inst.position_ids[0]
            rows.append((token, position, bt[c // bs] * bs + c % bs, c + 1, bt, rcb.sid))      # (v2p inline)
            if sampled:
                records.append((sp.temperature, sp.top_p, sp.top_k, sp.seed, len(rcb.output_token_ids) - position)
                               if sp.temperature > 0 else
                               (0.0, 1.0, 0, 0, len(rcb.output_token_ids) - position) if penalised else None)
                penalties.append((sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty, rcb.output_token_ids)
                                 if penalised else None)
            if len(bt) > max_blocks:
                max_blocks = len(bt)
        if not dec.fits(len(rows), max_blocks):
            return None
        return DecodeStep(rows, records if sampled else None, penalties if any(p is not None for p in penalties) else None)

    def _launch_decode(self, batch: BatchRequest, step: DecodeStep) -> None:
        """Enqueue the step, hand every request a placeholder for its new token, THEN read the
        previous step's tokens: the GPU already has the next step queued while the host catches up."""
        # a decoder without a sampled variant is called as it ever was, with the rows alone: a stand-in for one need
        # not take the other two arguments, as it need not carry the attributes (decoder_abilities)
        launch = self.graph_decoder.launch(*(step if step.records is not None else step[:1]))
        entries = []
        for row, (rcb, inst) in enumerate(batch):
            placeholder = PendingToken(launch, row)
            entries.append((rcb, inst, len(rcb.output_token_ids), placeholder))
            if rcb.eos_hit:
                continue                       # ended by a late-read token; this row's sample is dropped
            rcb.output_token_ids.append(placeholder)
            if inst.sample_dst is not None:
                inst.sample_dst.token_ids = [placeholder]
        batch.step()
        previous, self.pending = self.pending, (launch, entries)
        if previous is not None:
            self._resolve(previous)

    def _resolve(self, pending) -> None:
        launch, entries = pending
        tokens = self.graph_decoder.fetch(launch)
        now = time.perf_counter()
        for (rcb, inst, index, placeholder), token in zip(entries, tokens):
            if rcb.eos_hit:
                continue                       # a step that ran past an end-of-sequence token
            rcb.output_token_ids[index] = token
            if rcb.penalty_history is not None:
                rcb.penalty_history.append(token)   # (penalties from the graph: the host's table stays the truth for eager steps)
            dst = inst.sample_dst
            if dst is not None and dst.token_ids and dst.token_ids[0] is placeholder:
                dst.token_ids = [token]
            rcb.metric.token_times.append(now)
            if token in rcb.sampling_params.eos_token_ids:
                del rcb.output_token_ids[index + 1:]   # whatever ran past it is discarded
                rcb.eos_hit = True
            last = rcb.eos_hit or index + 1 == rcb.sampling_params.max_tokens
            for p in rcb.output_token_processors:
                p.append_token_id(token, last)

    # ------------------------------------------------------------------ the steady-state cohort
    def cohort_step(self, scheduler) -> int:
        """Called by EPDNode.step() in front of the scheduler.  Launches the next decode step of the cohort and returns
        its row count — or ends / declines the cohort and returns 0: the general path then runs the step."""
        dec = self.graph_decoder
        if not self.cohort_enabled or dec is None or not decoder_abilities(dec)[2]:
            return 0
        co = self.cohort
        if co is None:
            if self.pending is None or self.pending[0] == self.cohort_refused:
                return 0
            co = self._cohort_begin(scheduler)
            if co is None:
                self.cohort_refused = self.pending[0]
                return 0
        elif (scheduler.waiting or scheduler.running is not co.running_ref or len(scheduler.running) != co.n
              or co.epoch != rcb_module.MUTATIONS[0] or int(co.left.min()) < 2 or co.n > scheduler.token_budgets):
            self._cohort_end()
            return 0
        bs = co.bs
        # rows whose next token opens a new block: the only per-row work of a step (one row in sixteen)
        grown = []
        need = np.nonzero(co.cid // bs >= co.nblk)[0]
        if len(need):
            if len(need) > len(self.kv_manager.shared_cache.to_be_evicted):
                self._cohort_end()              # the pool cannot give every row its block now: the scheduler's business
                return 0
            for r in need.tolist():
                vc = co.rcbs[r].virtual_kv_cache
                self.kv_manager.realloc(vc, int(co.cid[r]) + 1)
                grown.append((co.sids[r], int(co.nblk[r]), vc.block_table[-1]))
                co.nblk[r] += 1
                co.last_block[r] = vc.block_table[-1]
        slots = co.last_block * bs + co.cid % bs
        launch = dec.launch_cohort(co.n, co.pos, slots, co.starts, grown)
        previous, co.launch = co.launch, launch
        co.k += 1
        co.pos += 1
        co.cid += 1
        co.left -= 1
        self.n_cohort_steps += 1
        if previous is None:                    # the launch the cohort was formed behind: the general bookkeeping
            pending, self.pending = self.pending, None
            self._resolve(pending)
            if co.eos_rows and any(co.rcbs[r].eos_hit for r in co.eos_rows):
                self._cohort_end()              # one of them has just ended: over before it began
        else:
            tokens = dec.fetch(previous)
            co.tok_log.append(tokens)
            co.t_log.append(time.perf_counter())
            ended = [r for r in co.eos_rows if tokens[r] in co.rcbs[r].sampling_params.eos_token_ids] if co.eos_rows else ()
            for r, processors in co.streams:    # tokens go out as they come (a request's last one only as an end-of-sequence id)
                for p in processors:
                    p.append_token_id(tokens[r], r in ended)
            if ended:
                # an end-of-sequence id, read one step late like every token: the launch just made ran past it for those
                # rows — their extra sample is dropped, the general path frees them at its next step (as it would have)
                self._cohort_end()
                for r in ended:
                    rcb = co.rcbs[r]
                    del rcb.output_token_ids[-1:]          # the placeholder of the launch that ran past the end
                    rcb.eos_hit = True
        if self.cohort is None:                 # it ended inside this step: the node looks at every row the way it does after any step
            self.ended_rows = co.rcbs
        return co.n

    def _cohort_begin(self, scheduler) -> Optional[DecodeCohort]:
        launch, entries = self.pending
        rcbs = [e[0] for e in entries]
        if scheduler.waiting or scheduler.running != rcbs or len(rcbs) > scheduler.token_budgets:
            return None
        bs = self.kv_manager.block_size
        co = DecodeCohort(rcbs, scheduler.running, bs)
        slot_of, cap = self.graph_decoder.stager.slot_of, self.graph_decoder.stager.cap
        for r, (rcb, inst) in enumerate(zip(rcbs, co.first_inst)):
            tok = inst.token_ids[0] if isinstance(inst, TextFill) and inst.token_ids and len(inst.token_ids) == 1 else None
            if (not isinstance(tok, PendingToken) or tok.launch != launch or tok.row != r or not inst.sample or rcb.eos_hit
                    or rcb.sid not in slot_of):
                return None
            if rcb.sampling_params.eos_token_ids:
                co.eos_rows.append(r)
            vc = rcb.virtual_kv_cache
            c = inst.cache_ids[0]
            co.pos[r], co.cid[r] = inst.position_ids[0], c
            co.left[r] = rcb.sampling_params.max_tokens - len(rcb.output_token_ids)
            co.nblk[r] = len(vc.block_table)
            co.last_block[r] = vc.block_table[c // bs] if c // bs < len(vc.block_table) else -1
            co.starts[r] = slot_of[rcb.sid][0] * cap
        if int(co.left.min()) < 2:
            return None
        self.cohort = co
        return co

    def _cohort_end(self) -> None:
        """Bring every request of the cohort up to date: tokens, stamps, instruction chain, cache size — and leave the
        last launch pending the way the general path would have."""
        co, self.cohort = self.cohort, None
        if co is None or co.k == 0:
            return
        entries = []
        for r, rcb in enumerate(co.rcbs):
            out = rcb.output_token_ids
            placeholder = PendingToken(co.launch, r)
            if not rcb.eos_hit:                 # (a request that ended at the cohort's first resolve keeps what it has)
                out.extend(t[r] for t in co.tok_log)
                if rcb.penalty_history is not None:
                    for t in co.tok_log:
                        rcb.penalty_history.append(t[r])
                out.append(placeholder)
                rcb.metric.token_times.extend(co.t_log)
            inst = co.first_inst[r]
            for _ in range(co.k - 1):
                inst = inst.next                # the instructions of the launches that have been resolved
            if inst.sample_dst is not None:
                inst.sample_dst.token_ids = [placeholder]
            rcb.instructions.curr = inst.next
            vc = rcb.virtual_kv_cache
            if int(co.cid[r]) > vc.n_cache_tokens:
                vc.n_cache_tokens = int(co.cid[r])
            entries.append((rcb, inst, len(out) - 1, placeholder))
        self.pending = (co.launch, entries)
        self.graph_decoder.stager.touch(co.sids)

    def resolve_pending(self) -> None:
        """Read back the tokens of the decode step that is still in flight (if any)."""
        if self.cohort is not None:
            self._cohort_end()
        if self.pending is not None:
            pending, self.pending = self.pending, None
            self._resolve(pending)

    def _deliver(self, batch: BatchRequest, sampled: List[int], scores=None) -> None:
        """scores: None, or the step's (logprobs, top_ids, top_logprobs) as host lists, one entry per sampled row."""
        now = time.perf_counter()
        for i, (rcb, inst) in enumerate(sampling_rows(batch)):
            token = sampled[i]
            if rcb.eos_hit:
                continue                       # already ended by a token that was read back late
            entry = None
            if not inst.is_chunked:
                if rcb.sampling_params.prompt_logprobs is not None and not rcb.output_token_ids:
                    for p in rcb.output_token_processors:       # the prompt's scores, complete with this step's, once
                        p.set_prompt_logprobs(rcb.prompt_logprobs)
                rcb.metric.token_times.append(now)
                rcb.output_token_ids.append(token)
                if rcb.penalty_history is not None:
                    rcb.penalty_history.append(token)           # generated tokens only: a chunk head's sample never gets here
                if getattr(rcb, "token_mask", None) is not None:
                    rcb.token_mask.advance(token)               # guided_choice: on to the child; a complete choice ends the
                                                                # request (rcb.is_finished), as an end-of-sequence id does
                if scores is not None and rcb.sampling_params.logprobs:
                    k = rcb.sampling_params.top_logprobs        # this request's own count out of the batch's largest
                    entry = TokenLogprob(token, scores[0][i], list(zip(scores[1][i][:k], scores[2][i][:k])))
                    rcb.output_logprobs.append(entry)
            if inst.sample_dst is not None:
                inst.sample_dst.token_ids = [token]
            if not inst.is_chunked:
                last = rcb.is_finished()
                for p in rcb.output_token_processors:
                    if entry is not None:
                        p.append_logprobs(entry)
                    p.append_token_id(token, last)
        batch.step()

    @staticmethod
    def _step_rows(inputs, logits):
        """The row geometry of an eager step -> (sel, decode, n_rows).  logits: None, or the ready logits of the step's
        sampling rows, one row per entry of inputs.selected_token_ids (a step that also scores prompts:
        _execute_scoring) — the forward is not run again, the same kernels follow.  decode: the logits are those of a
        decode batch's own forward, which keeps every input row, the sampling rows at `sel`.  n_rows: the logits' rows."""
        sel, decode = inputs.selected_token_ids, inputs.all_sequences_decode and logits is None
        return sel, decode, inputs.input_ids.shape[0] if decode else len(sel)

    @staticmethod
    def _raw_scores(logits, top_k: int):
        """The side launch for requests that asked for raw log-probabilities (hx_logprob_rows) -> its packed buffer."""
        return logprob_rows_packed(logprob_rows(logits, top_k)[0], top_k)

    @staticmethod
    def _to_host(packed, n_rows: int, top_k: int):
        """A packed buffer -> (ids, logprobs, top_ids, top_logprobs) as host lists: ONE device-to-host copy, a sync."""
        return [t.tolist() for t in logprob_rows_views(packed.cpu(), n_rows, top_k)]

    @staticmethod
    def _pick(geometry, sampled, scores=None):
        """(sampled, scores) per logits row -> per sampling row."""
        sel, decode, n_rows = geometry
        if decode and n_rows != len(sel):
            sampled = [sampled[j] for j in sel]
            scores = scores and tuple([col[j] for j in sel] for col in scores)
        return sampled, scores

    def _sample_with_logprobs(self, inputs, params, top_k: int, logits=None):
        """The eager step of a batch in which some request asked for log-probabilities: the same logits, ids by the same
        rule, and the scores beside them — one launch (hx_logprob_rows), one packed buffer, ONE device-to-host copy:
        the step's only device sync."""
        geometry = self._step_rows(inputs, logits)
        if logits is None:
            ids = self.language_model.forward_logprobs(inputs.input_ids, inputs.image_features, inputs.position_ids,
                                                       params, top_k)[0]
        else:
            ids = logprob_rows(logits, top_k)[0]
        sampled, *scores = self._to_host(logprob_rows_packed(ids, top_k), geometry[2], top_k)
        return self._pick(geometry, sampled, scores)

    def _sample(self, mode: str, batch: BatchRequest, inputs, params, top_k: Optional[int], logits=None):
        """The eager step of a batch that does not end in the plain argmax -> (sampled, scores).  Mode "logprobs" is
        _sample_with_logprobs.  The others (SAMPLING_MODES) are the same logits, then ONE launch for the whole batch in
        place of the argmax: a request the launch is not there for rides along with an empty history and (0, 0, 1),
        temperature 0, an empty bias table and min_p 0, and gets the id it would have got.  A request's offset is the
        number of tokens it has generated so far (the eager path has every token on the host), its bias table is the one
        for THIS step (TokenConstraints.step_entries: the end-of-sequence ids banned while the request has generated
        fewer than min_tokens).  The step's tables reach the device as one pinned buffer in one copy.  top_k: None, or
        the largest top_logprobs of the batch's OTHER requests that asked for log-probabilities (no request has both):
        their scores come from hx_logprob_rows over the same, raw logits."""
        if mode == "logprobs":
            return self._sample_with_logprobs(inputs, params, top_k, logits)
        take, packer, forward, kernel = SAMPLING_MODES[mode]
        geometry = sel, decode, n_rows = self._step_rows(inputs, logits)
        entries, _ = self._step_entries(batch, sel, decode, n_rows, take)
        tables = globals()[packer](entries).to_device(self.device)
        lm, scores = self.language_model, None
        if top_k is None and logits is None:
            sampled = getattr(lm, forward)(inputs.input_ids, inputs.image_features, inputs.position_ids, params, *tables)
        else:
            if logits is None:
                logits = lm.forward_logits(inputs.input_ids, inputs.image_features, inputs.position_ids, params)
            if top_k is not None:
                packed = self._raw_scores(logits, top_k)
            sampled = globals()[kernel](logits, *tables)
        sampled = sampled.tolist()                      # the step's only device sync beside the scores' copy
        if top_k is not None:
            scores = self._to_host(packed, n_rows, top_k)[1:]
        return self._pick(geometry, sampled, scores)

    @staticmethod
    def _step_entries(batch: BatchRequest, sel, decode: bool, n_rows: int, take: int):
        """(entries, at): the step's (history, penalties, record, bias)[:take] per logits row — a row that no request
        samples from rides along as plain greedy — and the logits row of each sampling request, in sampling_rows' order."""
        n_record = 6 if take == 4 else 5        # min_p (word 3 of a record) travels with the bias tables only
        entries = [(None, NO_PENALTIES, GREEDY_RECORD, None)[:take]] * n_rows
        at = []
        for i, (rcb, _) in enumerate(sampling_rows(batch)):
            sp, n_out = rcb.sampling_params, len(rcb.output_token_ids)
            record = (sp.temperature, sp.top_p, sp.top_k, sp.seed, n_out, sp.min_p)[:n_record] if sp.temperature > 0 \
                else GREEDY_RECORD
            bias = rcb.token_constraints.step_entries(n_out) if rcb.token_constraints is not None else None
            at.append(sel[i] if decode else i)
            entries[at[-1]] = (rcb.penalty_history, (sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty),
                               record, bias)[:take]
        return entries, at

    def _sample_scored(self, batch: BatchRequest, inputs, params, logits=None):
        """The eager step of a batch in which some request asked for PROCESSED log-probabilities (scored_rows) ->
        (sampled, scores).  The same logits, then ONE hx_sample_rows_logprobs launch for the whole batch in place of the
        mode's kernel: the four-element entries of the constrained mode, so constrained, drawn, penalised and plain
        requests ride along and get the ids they would have got; want = -1 on every row but those of the processed
        requests that deliver a token, so only those pay for their scores.  K is the largest top_logprobs among them.
        The tables and `want` reach the device as one pinned buffer in one copy, the ids and scores come back in one.
        RAW-mode logprobs requests in the same batch (greedy, unpenalised, unconstrained by admission) keep getting their
        scores from hx_logprob_rows over the raw logits, exactly as in _sample: a mixed batch is two launches and two
        packed buffers."""
        rows = sampling_rows(batch)
        geometry = sel, decode, n_rows = self._step_rows(inputs, logits)
        entries, at = self._step_entries(batch, sel, decode, n_rows, 4)
        step = pack_constrained_step(entries)
        size = step.buffer.size
        host = np.empty(size + n_rows, dtype=np.int32)
        host[:size] = step.buffer
        host[size:] = -1
        top_k, raw = 0, []                      # the processed requests' K; the raw-mode requests' top_logprobs
        for row, (rcb, inst) in zip(at, rows):
            sp = rcb.sampling_params
            if inst.is_chunked or not sp.logprobs:
                continue
            if asks_processed(rcb):
                host[size + row] = 0
                top_k = max(top_k, sp.top_logprobs)
            else:
                raw.append(sp.top_logprobs)
        host = torch.from_numpy(host)
        if torch.device(self.device).type == "cuda":
            host = host.pin_memory()
        dev = host.to(self.device, non_blocking=True)
        tables, want = step.views(dev[:size]), dev[size:]
        lm = self.language_model
        if not raw and logits is None:
            ids = lm.forward_scored(inputs.input_ids, inputs.image_features, inputs.position_ids, params, *tables,
                                    top_k=top_k, want=want)[0]
        else:
            if logits is None:
                logits = lm.forward_logits(inputs.input_ids, inputs.image_features, inputs.position_ids, params)
            if raw:
                raw_packed = self._raw_scores(logits, max(raw))
            ids = sample_rows_logprobs(logits, *tables, top_k=top_k, want=want)[0]
        sampled, *scores = self._to_host(logprob_rows_packed(ids, top_k), n_rows, top_k)
        if raw:
            raw_scores = self._to_host(raw_packed, n_rows, max(raw))[1:]
            for row, (rcb, _) in zip(at, rows):
                if rcb.sampling_params.logprobs and not asks_processed(rcb):
                    for col, raw_col in zip(scores, raw_scores):
                        col[row] = raw_col[row]
        return self._pick(geometry, sampled, scores)

    def _sample_masked(self, batch: BatchRequest, inputs, params, logits=None):
        """The eager step of a batch in which some request carries a token mask (masked_rows) -> (sampled, scores).  The
        same logits, then ONE hx_sample_rows_masked launch for the whole batch, modelled on _sample_scored: the
        four-element entries of the constrained mode, want = -1 on every row but those of the processed-logprobs requests
        that deliver a token, mask_row = -1 on every row without a mask (a chunk head's discarded sample included); rows on
        the same trie node share one mask of the step.  The tables, `want`, `mask_row` and the step's distinct masks reach
        the device as one pinned buffer in one copy.  With no processed request in the batch the launch is unscored and
        only the ids come back.  RAW-mode logprobs requests beside them keep hx_logprob_rows over the raw logits."""
        rows = sampling_rows(batch)
        geometry = sel, decode, n_rows = self._step_rows(inputs, logits)
        entries, at = self._step_entries(batch, sel, decode, n_rows, 4)
        entries = [e + (-1, None) for e in entries]
        top_k, raw = None, []                   # the processed requests' K (None: nobody asks); the raw-mode requests' top_logprobs
        for row, (rcb, inst) in zip(at, rows):
            if inst.is_chunked:
                continue
            sp, mask = rcb.sampling_params, getattr(rcb, "token_mask", None)
            want = -1
            if sp.logprobs and asks_processed(rcb):
                want, top_k = 0, max(top_k or 0, sp.top_logprobs)
            elif sp.logprobs:
                raw.append(sp.top_logprobs)
            entries[row] = entries[row][:4] + (want, mask.current() if mask is not None else None)
        *tables, want = pack_masked_step(entries).to_device(self.device)
        if logits is None:
            logits = self.language_model.forward_logits(inputs.input_ids, inputs.image_features, inputs.position_ids, params)
        if raw:
            raw_packed = self._raw_scores(logits, max(raw))
        if top_k is None:
            sampled, scores = sample_rows_masked(logits, *tables).tolist(), None
            if raw:
                scores = [[float("nan")] * n_rows, [[]] * n_rows, [[]] * n_rows]
        else:
            ids = sample_rows_masked(logits, *tables, top_k=top_k, want=want)[0]
            sampled, *scores = self._to_host(logprob_rows_packed(ids, top_k), n_rows, top_k)
        if raw:
            raw_scores = self._to_host(raw_packed, n_rows, max(raw))[1:]
            for row, (rcb, _) in zip(at, rows):
                if rcb.sampling_params.logprobs and not asks_processed(rcb):
                    for col, raw_col in zip(scores, raw_scores):
                        col[row] = raw_col[row]
        return self._pick(geometry, sampled, scores)

    def _choose(self, batch: BatchRequest, inputs, params, logits=None):
        """What an eager step that samples runs -> (sampled, scores): the ONE place that decides it, for execute and for
        _execute_scoring (logits: as in _step_rows).  masked_rows first, then scored_rows, then step_mode, then the plain
        argmax — the language model's own when it runs the forward, the step's only device sync."""
        rows = sampling_rows(batch)
        if masked_rows(rows):
            return self._sample_masked(batch, inputs, params, logits)
        if scored_rows(rows):
            return self._sample_scored(batch, inputs, params, logits)
        mode, top_k = step_mode(rows)
        if mode != "plain":
            return self._sample(mode, batch, inputs, params, top_k, logits)
        if logits is not None:
            return argmax_rows(logits).tolist(), None
        sampled = self.language_model.forward(inputs.input_ids, inputs.image_features, inputs.position_ids, params)
        if inputs.all_sequences_decode and sampled.numel() != len(inputs.selected_token_ids):
            sampled = sampled[inputs.selected_token_ids_tensor]
        return sampled.tolist(), None

    def _execute_scoring(self, batch: BatchRequest, inputs) -> None:
        """The eager step of a batch in which some request scores its prompt (sampling_params.prompt_logprobs): ONE forward
        whose last layer is narrowed to the union of the sampling and the scoring rows (inputs.score_plan), ONE
        hx_token_logprob_rows launch over all of them — target -1 on the rows that only sample: those workgroups leave at
        once, and nothing is gathered for scoring — then the step's sampling rows (a few) are picked out of the logits and
        go through the kernels the step would have run without scoring.  The scores reach the host in one copy, the
        step's only one beside the sampling's."""
        plan = inputs.score_plan
        params = LanguageModelParameters(inputs.attention_params, inputs.all_sequences_decode, plan.rows_tensor,
                                         inputs.image_row_index)
        logits = self.language_model.forward_logits(inputs.input_ids, inputs.image_features, inputs.position_ids, params)
        k = plan.top_k
        packed = token_logprob_rows_packed(token_logprob_rows(logits, plan.targets_tensor, k)[0], k)
        sampled = scores = None
        if inputs.selected_token_ids:
            sampled, scores = self._choose(batch, inputs, params, logits.index_select(0, plan.sample_pos_tensor))
        lp, ranks, top_ids, top_lp = (t.tolist() for t in token_logprob_rows_views(packed.cpu(), len(plan.rows), k))
        for u, dst in enumerate(plan.dst):
            if dst is not None:
                rcb, index = dst
                own = rcb.sampling_params.prompt_logprobs       # this request's own count out of the step's largest
                rcb.prompt_logprobs[index] = PromptTokenLogprob(plan.targets[u], lp[u], ranks[u],
                                                                list(zip(top_ids[u][:own], top_lp[u][:own])))
        if sampled is None:
            batch.step()                       # nothing samples: the forward ran for its cache writes and its scores
        else:
            self._deliver(batch, sampled, scores)

    def _publish_prefix_blocks(self, batch: BatchRequest) -> None:
        """A block's hash enters the prefix cache in the step that computes its last token
        (executor.py:111-127); decode tokens are never published."""
        bs = self.kv_manager.block_size
        for rcb, inst in batch:
            if inst.hashes is None:
                continue
            vblocks = [c // bs for c in inst.cache_ids if c % bs == bs - 1 and c // bs < len(inst.hashes)]
            self.kv_manager.set_blocks(rcb.virtual_kv_cache, vblocks, [inst.hashes[v] for v in vblocks])

    def execute(self, batch: BatchRequest) -> None:
        if len(batch) == 0:
            return
        self._publish_prefix_blocks(batch)
        if self.graph_decoder is not None:
            step = self._decode_rows(batch)
            if step is not None:
                self._launch_decode(batch, step)
                return
            self.resolve_pending()             # the eager path needs every token on the host
        sh = self.shape
        builder = LanguageModelParametersBuilder(
            self.image_manager, self.kv_manager, sh.num_hidden_layers, sh.num_attention_heads,
            sh.num_key_value_heads, sh.head_dim, self.language_model.image_token_id, self.dtype, self.device)
        builder.add_batch(batch)
        max_pos = getattr(sh, "max_position_embeddings", None)
        if max_pos is not None and builder.position_ids and max(builder.position_ids) >= max_pos:
            # the RoPE / attention kernels index the cos_sin table unchecked (admission normally rejects this:
            # request_processor.InstructionCreator.max_position_embeddings)
            raise HydraHipError(f"position {max(builder.position_ids)} outside the rotary table "
                                f"(max_position_embeddings = {max_pos})")
        inputs = builder.build_language_model_parameters()
        if inputs.score_plan is not None:
            self._execute_scoring(batch, inputs)
            return
        params = LanguageModelParameters(inputs.attention_params, inputs.all_sequences_decode,
                                         inputs.selected_token_ids_tensor, inputs.image_row_index)
        if not inputs.selected_token_ids:
            # nothing samples: the forward still has to run for its cache writes
            self.language_model.language_model.forward_hidden(
                self.language_model.embed(inputs.input_ids, inputs.image_features, inputs.image_row_index),
                inputs.position_ids, params)
            batch.step()
            return
        self._deliver(batch, *self._choose(batch, inputs, params))


class BatchImageEmbedExecutor:
    """use_graphs: the vision tower's shapes depend only on the number of images in the batch, so
    one hipGraph per image count (captured on first use) replaces ~280 eager launches — 5.5 ms of
    host-paced work becomes 3.2 ms for a single image."""

    def __init__(self, vision_model, image_cache_block_manager, n_qo_heads: int, head_dim: int,
                 dtype: torch.dtype, device: torch.device, use_graphs: bool = False):
        self.vision_model = vision_model
        self.manager = image_cache_block_manager
        self.n_qo_heads, self.head_dim = n_qo_heads, head_dim
        self.dtype, self.device = dtype, device
        self.use_graphs = use_graphs and device.type == "cuda"
        self.graphs = {}       # n_images (or (n_images, strategy) for the pruning forward) -> (graph, static inputs, static output)
        self._stages = {}      # (n_images, shape, dtype) -> [(pinned staging buffer, event behind its last copy), ...]

    def _encode(self, pixels: torch.Tensor, n_keep: Optional[torch.Tensor] = None, strategy: str = "rank") -> torch.Tensor:
        """n_keep: None, or the per-image kept counts (int32, on the device): the pruning forward, whose graph takes the
        counts as a second static input — one graph per image count serves every mix of counts."""
        extra = () if n_keep is None else (n_keep, strategy)
        if not self.use_graphs or torch.cuda.is_current_stream_capturing():
            return self.vision_model.forward(pixels, *extra)
        n = pixels.shape[0]
        key = n if n_keep is None else (n, strategy)
        entry = self.graphs.get(key)
        if entry is None:
            static_in = pixels.clone()
            static_extra = () if n_keep is None else (n_keep.clone(), strategy)
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                self.vision_model.forward(static_in, *static_extra)          # warm-up outside capture
            torch.cuda.current_stream(self.device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = self.vision_model.forward(static_in, *static_extra)
            entry = self.graphs[key] = (graph, (static_in,) + static_extra[:1], static_out)
        graph, static_ins, static_out = entry
        static_ins[0].copy_(pixels)
        if n_keep is not None:
            static_ins[1].copy_(n_keep)
        graph.replay()
        return static_out          # consumed (scattered into the image cache) before the next replay: same stream

    def _upload(self, pixels: List[torch.Tensor]) -> torch.Tensor:
        """The step's images as ONE device tensor of the model's dtype.  Host images go through a pinned staging buffer and
        ONE asynchronous copy instead of a synchronous pageable `.to(device)` per image (the runtime locks the pages of
        each first): the burst's 8-image steps are 6 ms shorter (first chunk done at 38 instead of 45 ms,
        tools/burst_timeline.py)."""
        if self.device.type != "cuda" or any(p.is_cuda for p in pixels):
            return torch.cat([p.to(device=self.device, dtype=self.dtype) for p in pixels], dim=0)
        n = sum(p.shape[0] for p in pixels)
        # kept pinned buffers, a few per (image count, shape): one whose last copy has finished is taken, another one is
        # made when all are still in flight — never a wait for the stream (an event wait made the host wait for the decode
        # step queued in front of the copy: Poisson TPOT p50 at 16 req/s 4.4 -> 5.6 ms) and, after the first steps, never
        # an allocation (a fresh pinned block per step is a 10-40 ms hipHostMalloc every now and then)
        key = (n, tuple(pixels[0].shape[1:]), pixels[0].dtype)
        ring = self._stages.setdefault(key, [])
        slot = next((e for e in ring if e[1].query()), None)
        if slot is None:
            slot = (torch.empty((n,) + key[1], dtype=key[2]).pin_memory(), torch.cuda.Event())
            if len(ring) < 8:
                ring.append(slot)
        stage, free = slot
        i = 0
        for p in pixels:
            stage[i:i + p.shape[0]].copy_(p)
            i += p.shape[0]
        dev_px = stage.to(self.device, non_blocking=True)
        free.record(torch.cuda.current_stream(self.device))
        return dev_px.to(self.dtype)

    def warmup(self, pixel_values: torch.Tensor, max_images: int) -> None:
        """Capture the graphs for 1 .. max_images images ahead of serving."""
        px = pixel_values.to(device=self.device, dtype=self.dtype)
        for n in range(1, max_images + 1):
            self._encode(px.expand(n, -1, -1, -1).contiguous())
            if not pixel_values.is_cuda:
                self._upload([pixel_values] * n)         # and the pinned staging buffer of that image count
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def execute(self, batch: BatchRequest) -> None:
        if len(batch) == 0:
            return
        slots: List[int] = []
        pixels = []
        counts: List[Optional[int]] = []
        strategies = set()
        for rcb, inst in batch:
            pixels.append(inst.pixel_values)
            inst.pixel_values = None
            slots += self.manager.v2p(rcb.virtual_image_cache, inst.cache_ids)
            n_keep = getattr(inst, "n_keep", None)
            counts += [n_keep] * pixels[-1].shape[0]
            if n_keep is not None:
                strategies.add(inst.strategy)
        if not strategies:
            feats = self._encode(self._upload(pixels))                      # (n_img, 576, hidden)
            tokens = feats.reshape(-1, self.n_qo_heads, self.head_dim)
            ints = slots
        else:
            # focal token pruning (layer/token_prunning.py): an image that keeps every token rides along with n = all of
            # them (the identity selection), so one forward serves the mixed batch.  Only the kept rows — the first n of
            # each image's block of the padded output — go to the image cache, into the first n slots of its block.
            if len(strategies) > 1:
                raise ValueError(f"one image-embed batch mixes pruning strategies {sorted(strategies)}")
            n_patches = (self.vision_model.shape.image_size // self.vision_model.shape.patch_size) ** 2
            counts = [n_patches if c is None else c for c in counts]
            rows = [b * n_patches + r for b, c in enumerate(counts) for r in range(c)]
            assert len(rows) == len(slots), "kept image tokens and image cache slots differ"
            ints = slots + rows + counts
        slot_t = torch.tensor(ints, dtype=torch.int32)
        if self.device.type == "cuda":
            slot_t = slot_t.pin_memory().to(self.device, non_blocking=True)
        if strategies:
            n_rows = len(slots)
            slot_t, row_t, keep_t = slot_t[:n_rows], slot_t[n_rows:2 * n_rows], slot_t[2 * n_rows:]
            feats = self._encode(self._upload(pixels), keep_t.contiguous(), strategies.pop())
            tokens = feats.reshape(-1, feats.shape[-1]).index_select(0, row_t).reshape(-1, self.n_qo_heads, self.head_dim)
        self.manager.get_layer_cache(layer_id=0).set_caches(slot_t, [tokens])
        batch.step()


class InstructionExecutor:
    def __init__(self, fill_executor: Optional[BatchFillExecutor],
                 image_embed_executor: Optional[BatchImageEmbedExecutor], multi_streams_forward: bool = False):
        self.fill_executor = fill_executor
        self.image_embed_executor = image_embed_executor
        self.vision_stream = torch.cuda.Stream() if multi_streams_forward else None

    def execute_fill(self, batch: BatchRequest) -> None:
        if len(batch):
            self.fill_executor.execute(batch)

    def execute_image_embed(self, batch: BatchRequest) -> None:
        if len(batch) == 0:
            return
        if self.vision_stream is None:
            self.image_embed_executor.execute(batch)
            return
        self.vision_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.vision_stream):
            self.image_embed_executor.execute(batch)
        # the image cache is read by a later step's prefill on the main stream
        torch.cuda.current_stream().wait_stream(self.vision_stream)

    def execute_empty(self, batch: BatchRequest) -> None:
        batch.step()

    def resolve_pending(self) -> None:
        if self.fill_executor is not None:
            self.fill_executor.resolve_pending()
