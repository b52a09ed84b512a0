"""Request control block and batch — mirror of hydrainfer/engine/rcb.py:8-71,
hydrainfer/request/request.py:6-39, hydrainfer/engine/metric.py:5-19 and
hydrainfer/engine/scenario.py:3-16."""
from dataclasses import dataclass, field
from enum import IntEnum
from typing import Dict, List, Optional, Tuple

from hydrainfer_amd.engine.isa import Instruction, InstructionList
from hydrainfer_amd.memory.token_cache import VirtualTokenCache
from hydrainfer_amd.utils import keyword_argument


@keyword_argument("guided_choice")
@keyword_argument("allowed_token_ids")
@keyword_argument("logprobs_mode")
@dataclass
class SamplingParameters:
    max_tokens: int = 50
    eos_token_ids: List[int] = field(default_factory=list)
    logprobs: bool = False      # a TokenLogprob per generated token (OpenAI's `logprobs`); such a request decodes eagerly
    top_logprobs: int = 0       # 0..20 most likely alternatives in each of them; needs logprobs
    # steps 1-2 of the reference's process_logits (hydrainfer/sampling/logits_processor.py:65-72) over the request's
    # GENERATED tokens (hydrainfer_amd/sampling); (0, 0, 1) is the identity: such a request is sampled as before.  A
    # penalised request decodes eagerly (from the captured step under the graph_penalties switch) and can ask for logprobs only with logprobs_mode = "processed_logprobs".
    frequency_penalty: float = 0.0      # subtracted once per earlier occurrence of a token
    presence_penalty: float = 0.0       # subtracted once from every token that occurred
    repetition_penalty: float = 1.0     # > 0: a token that occurred has its logit divided (if negative: multiplied) by it
    # steps 3-5 of process_logits and a seeded draw (hx_sample_rows, include/hydra_hip.h).  temperature 0 is GREEDY
    # (OpenAI's meaning of 0), and an absent temperature means 0 here, where OpenAI's default is 1: every request that does
    # not ask for sampling keeps the argmax paths.  A sampled request decodes eagerly and can ask for logprobs only with
    # logprobs_mode = "processed_logprobs".
    temperature: float = 0.0            # >= 0; > 0: the logits are divided by it and a token is drawn
    top_p: float = 1.0                  # (0, 1]: the smallest set of most likely tokens holding this much probability
    top_k: int = 0                      # >= 0: only the k most likely tokens (ties at the cut are all kept); 0: off
    seed: Optional[int] = None          # 0 .. 2^63 - 1; a sampled request without one is given one at admission
    # token constraints (hx_sample_rows_constrained, include/hydra_hip.h): edits of the logits ahead of the choice, greedy
    # or sampled.  A constrained request decodes eagerly and can ask for logprobs only with logprobs_mode =
    # "processed_logprobs" (hx_logprob_rows scores the raw logits and names the raw argmax); prompt_logprobs stays
    # combinable.  The three are keyword-only — positional
    # construction is what it was — and declared AHEAD of prompt_logprobs, which stays the last field.
    # logit_bias: token id -> a bias in -100 .. 100 added to its logit BEFORE the penalties; min_tokens: every
    # eos_token_ids entry is banned until this many tokens are generated; min_p in [0, 1]: only tokens at least this
    # likely relative to the most likely one, 0: off
    logit_bias: Optional[Dict[int, float]] = field(default=None, kw_only=True)
    min_tokens: int = field(default=0, kw_only=True)
    min_p: float = field(default=0.0, kw_only=True)
    # which distribution `logprobs` scores (vLLM's option of the same name; keyword-only, ahead of prompt_logprobs).  None
    # or "raw_logprobs": the model's softmax over the raw logits (hx_logprob_rows) — such a request cannot be sampled,
    # penalised or constrained.  "processed_logprobs": the distribution the token was actually chosen from — after
    # logit_bias, penalties, temperature, top-k, min_p and top-p, renormalised over the kept set (hx_sample_rows_logprobs,
    # the same launch that chooses the token); needs logprobs, combines with all of the above.  prompt_logprobs stays raw.
    # (init=False and the class's keyword_argument decorator: taken by keyword only, the generated signature as it was)
    logprobs_mode: Optional[str] = field(default=None, init=False)
    # token masks (hx_sample_rows_masked, include/hydra_hip.h; vLLM's names): the request may only emit tokens of a set.
    # allowed_token_ids: one set, every step.  guided_choice: the request emits exactly one of several token SEQUENCES
    # (1..64 of 1..64 ids, none a prefix of another) and ends there; cut short by max_tokens it emits a truncated choice.
    # At most one of the two.  Such a request decodes eagerly and can ask for logprobs only with logprobs_mode =
    # "processed_logprobs" (the scores are then those over the allowed set); prompt_logprobs stays combinable.
    # (init=False and keyword_argument, like logprobs_mode: by keyword only, the generated signature as it was)
    allowed_token_ids: Optional[List[int]] = field(default=None, init=False)
    guided_choice: Optional[List[List[int]]] = field(default=None, init=False)
    # the log-probability of every PROMPT token given what stands before it (vLLM's `prompt_logprobs`;
    # hx_token_logprob_rows over the prefill's logits): None = off, 0..20 = score, with that many alternatives per position.
    # Independent of `logprobs` and of the sampling mode: scoring reads the prompt's rows, sampling the last one.  Such a
    # request's prefill takes no prefix-cache hit (a skipped token has no logits); it decodes like any other.
    prompt_logprobs: Optional[int] = None


MAX_TOP_LOGPROBS = 20
RAW_LOGPROBS, PROCESSED_LOGPROBS = "raw_logprobs", "processed_logprobs"      # the values of logprobs_mode (None: raw)


def check_logprobs_mode(mode, logprobs: bool) -> Optional[str]:
    """The value checked, or ValueError: None or one of the two names; the processed mode needs logprobs."""
    if mode is not None and mode not in (RAW_LOGPROBS, PROCESSED_LOGPROBS):
        raise ValueError(f"logprobs_mode {mode!r} must be {RAW_LOGPROBS!r} or {PROCESSED_LOGPROBS!r}")
    if mode == PROCESSED_LOGPROBS and not logprobs:
        raise ValueError(f"logprobs_mode = {PROCESSED_LOGPROBS!r} needs logprobs = True")
    return mode


@dataclass
class TokenLogprob:
    """One generated token's score: its log-probability under the model's softmax (fp32, hx_logprob_rows) and the
    request's top_logprobs most likely (token id, log-probability) pairs, most likely first (ties: lower id first).
    With logprobs_mode = "processed_logprobs" the distribution is the one the step's choice rule picked the token from
    (fp32, hx_sample_rows_logprobs): the logits after logit_bias, penalties and temperature, cut by top-k, min_p and
    top-p and renormalised over what is left — for a greedy request the softmax of its biased, penalised logits.
    `logprob` is then always finite; an alternative that the truncation dropped is still listed, with -inf."""
    token_id: int
    logprob: float
    top: List[Tuple[int, float]] = field(default_factory=list)


@dataclass
class PromptTokenLogprob:
    """One prompt token's score: its log-probability given everything before it (image included) under the model's
    softmax (fp32, hx_token_logprob_rows), its rank — the number of tokens the model ranks before it, 0: it is the greedy
    choice — and the request's prompt_logprobs most likely (token id, log-probability) pairs at that position."""
    token_id: int
    logprob: float
    rank: int
    top: List[Tuple[int, float]] = field(default_factory=list)


@dataclass
class TokenParameters:
    """hydrainfer/request/request.py:13-18, field for field.  Implemented: token_pruning_policy = 'focal' (the request's
    image enters the prompt as n_embed_output_tokens tokens chosen by layer/token_prunning.py instead of all of them).
    Declared only: the KV-cache eviction policies — InstructionCreator.process refuses anything but None."""
    kv_cache_eviction_policy: Optional[str] = None     # None | 'random' | 'streamingllm'
    window_size: int = 28
    attention_sink_size: int = 4
    token_pruning_policy: Optional[str] = None         # None | 'focal'
    n_embed_output_tokens: int = 64


@dataclass
class RequestMetaData:
    n_images: int
    n_prompt_tokens: int
    n_text_tokens: int
    n_image_tokens: int


@dataclass
class RequestMetric:
    arrival_time: float = 0.0
    token_times: List[float] = field(default_factory=list)
    finished_time: float = 0.0
    # latency breakdown: [begin, end] stamps per phase
    encode_queueing: List[float] = field(default_factory=list)
    encode_execute: List[float] = field(default_factory=list)
    ep_transfer: List[float] = field(default_factory=list)
    prefill_queueing: List[float] = field(default_factory=list)
    prefill_execute: List[float] = field(default_factory=list)
    pd_transfer: List[float] = field(default_factory=list)
    decode_queueing: List[float] = field(default_factory=list)
    decode_execute: List[float] = field(default_factory=list)


class ScenarioType(IntEnum):
    Relaxed = 0
    Strict = 1


class ScenarioClassifier:
    def classify(self, n_text_tokens: int, n_output_tokens: int) -> ScenarioType:
        strict = n_text_tokens < 100 and n_output_tokens < 100
        return ScenarioType.Strict if strict else ScenarioType.Relaxed


# Bumped by whoever changes a live request behind the engine's back (a cancelled stream lowering max_tokens:
# entrypoint/api_server.py).  The executor's steady-state decode cohort (engine/executor.py) compares it instead of
# re-reading every request every step.
MUTATIONS = [0]


class OutputTokenProcessor:
    def append_token_id(self, token_id: int, is_last_token: bool = False) -> None:
        raise NotImplementedError

    def append_logprobs(self, entry: "TokenLogprob") -> None:
        """The score of the token the next append_token_id call delivers (only for requests with
        sampling_params.logprobs).  Processors that do not care ignore it."""

    def set_prompt_logprobs(self, entries: list) -> None:
        """The scores of the request's prompt (rcb.prompt_logprobs; only for requests with sampling_params.prompt_logprobs):
        called once, before the request's first append_token_id.  Processors that do not care ignore it."""

    def fail(self, exc: BaseException) -> None:
        """The request was terminated by the engine (a migration that failed twice, a node that died): the reference
        pushes a None token to the stream (hydrainfer/cluster/epdnode.py:440-442, `(request_id, None)`)."""
        self.append_token_id(None, True)


class LogOutputTokenProcessor(OutputTokenProcessor):
    def __init__(self):
        self.token_ids: List[int] = []

    def append_token_id(self, token_id: int, is_last_token: bool = False) -> None:
        self.token_ids.append(token_id)


class RequestControlBlock:
    def __init__(self):
        self.request_id = None
        self.sampling_params: Optional[SamplingParameters] = None
        self.request_metadata: Optional[RequestMetaData] = None
        self.instructions: Optional[InstructionList] = None
        self.virtual_kv_cache: Optional[VirtualTokenCache] = None
        self.virtual_image_cache: Optional[VirtualTokenCache] = None
        self.sid: int = -1
        self.output_token_processors: List[OutputTokenProcessor] = []
        self.output_token_ids: List[int] = []
        self.output_logprobs: List[TokenLogprob] = []     # parallel to output_token_ids when sampling_params.logprobs, else empty
        # a request with sampling_params.prompt_logprobs: one entry per token of the request's OWN token_ids (not of the
        # prompt with its image expanded) — None for token 0 (no context) and for an image placeholder, else a
        # PromptTokenLogprob, filled in as the prefill's chunks complete; [] for a request that did not ask
        self.prompt_logprobs: List[Optional[PromptTokenLogprob]] = []
        self.penalty_history = None      # sampling.PenaltyHistory of a penalised request (its delivered tokens), else None
        self.token_constraints = None    # sampling.TokenConstraints of a constrained request (logit_bias, min_tokens, min_p), else None
        self.token_mask = None           # sampling.TokenMask of a request with allowed_token_ids / guided_choice, else None
        self.scenario_type: Optional[ScenarioType] = None
        self.metric = RequestMetric()
        self.eos_hit = False      # set when a token read back late (decode look-ahead) was end-of-sequence
        self.stream_rank: Optional[int] = None    # multi-process serving: the rank whose front end streams this request's
                                                  # tokens to a client (engine/distributed.py: the reference pushes them
                                                  # over zmq from every node, hydrainfer/engine/output_token_processor.py:92-140)
        self.path: List[int] = []                 # multi-process serving: the ranks that have owned this request, in order
        self.failed: Optional[str] = None         # why the engine terminated this request (EPDNode.terminate), if it did

    def current_instruction(self) -> Instruction:
        return self.instructions.curr

    def step(self) -> None:
        self.instructions.curr = self.instructions.curr.next

    def is_finished(self) -> bool:
        if self.instructions.curr is None or self.eos_hit:
            return True
        if self.token_mask is not None and self.token_mask.finished:           # guided_choice: the choice is complete
            return True
        if len(self.output_token_ids) >= self.sampling_params.max_tokens:      # (>=: a cancelled stream lowers max_tokens, api_server.py)
            return True
        return bool(self.output_token_ids) and self.output_token_ids[-1] in self.sampling_params.eos_token_ids

    def release_instructions(self) -> None:
        """A finished request's chain is a doubly linked list — reference cycles that only the
        cyclic collector can free, and serving loops run with it off (serve.quiet_gc).  Cut the
        links so plain reference counting reclaims the instructions."""
        if self.instructions is None:
            return
        node = self.instructions.head
        while node is not None:
            nxt = node.next
            node.next = node.prev = None
            if hasattr(node, "sample_dst"):
                node.sample_dst = None
            node = nxt
        self.instructions.curr = None

    def register_output_token_processor(self, p: OutputTokenProcessor) -> None:
        self.output_token_processors.append(p)

    def __repr__(self):
        return f"rcb(sid={self.sid}, {self.instructions})"


class BatchRequest:
    def __init__(self, rcbs: Optional[List[RequestControlBlock]] = None):
        self.rcbs = rcbs if rcbs is not None else []

    def __len__(self):
        return len(self.rcbs)

    def __getitem__(self, idx: int) -> Tuple[RequestControlBlock, Instruction]:
        return self.rcbs[idx], self.rcbs[idx].instructions.curr

    def __iter__(self):
        # (a generator, not the index protocol: `for rcb, inst in batch` runs a dozen times per engine step)
        for rcb in self.rcbs:
            yield rcb, rcb.instructions.curr

    def append(self, rcb: RequestControlBlock) -> None:
        self.rcbs.append(rcb)

    def step(self) -> None:
        for rcb in self.rcbs:
            rcb.step()
