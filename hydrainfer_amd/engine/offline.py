"""Offline inference on one GPU: a checkpoint directory (or two ready models) in, generated token
ids and their timing out — the collocated EPD node of engine/node.py behind a three-line API.
Mirrors what the reference's offline path hands back (hydrainfer/request/offline_inference_output.py:5-12);
prompts are token ids (one image placeholder id where the image goes): there is no tokenizer offline."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import torch

from hydrainfer_amd.engine.node import LocalCluster
from hydrainfer_amd.engine.rcb import PromptTokenLogprob, SamplingParameters, TokenLogprob, TokenParameters
from hydrainfer_amd.engine.request_processor import InstructionCreator, TokenRequest
from hydrainfer_amd.engine.scheduler import BatchSchedulerConfig
from hydrainfer_amd.engine.serve import build_node, quiet_gc, warm_library_gemms
from hydrainfer_amd.memory.shared_cache import compute_image_hash
from hydrainfer_amd.model.processor import ClipImageProcessor
from hydrainfer_amd.utils import keyword_argument


@dataclass
class OfflineInferenceOutput:
    output_token_ids: List[int] = field(default_factory=list)
    arrival_time: float = -1.0
    finished_time: float = -1.0
    token_times: List[float] = field(default_factory=list)
    ttft: float = -1.0
    tpot: List[float] = field(default_factory=list)
    output_logprobs: List[TokenLogprob] = field(default_factory=list)    # one per output token if the request asked, else empty
    # one per token of the request's own token_ids if it asked for prompt_logprobs (None for token 0 and for an image
    # placeholder), else empty
    prompt_logprobs: List[Optional[PromptTokenLogprob]] = field(default_factory=list)


@keyword_argument("guided_choice")
@keyword_argument("allowed_token_ids")
@keyword_argument("logprobs_mode")
@dataclass
class OfflineRequest:
    token_ids: List[int]
    image: object = None          # PIL image or None
    max_tokens: int = 50
    eos_token_ids: Sequence[int] = ()
    token_params: Optional[TokenParameters] = None     # token_pruning_policy='focal': the image as n_embed_output_tokens tokens
    logprobs: bool = False        # the log-probability of every generated token (such a request decodes eagerly)
    top_logprobs: int = 0         # and of its 0..20 most likely alternatives
    frequency_penalty: float = 0.0      # the reference's process_logits steps 1-2 over the generated tokens
    presence_penalty: float = 0.0       # (hydrainfer_amd/sampling); a penalised request decodes eagerly
    repetition_penalty: float = 1.0
    temperature: float = 0.0            # > 0: sampled decoding (steps 3-5 of process_logits and a seeded draw); 0: greedy
    top_p: float = 1.0                  # a sampled request decodes eagerly
    top_k: int = 0
    seed: Optional[int] = None          # None: the engine assigns one (it is in the request's sampling_params afterwards)
    # token constraints — keyword-only, declared ahead of prompt_logprobs (which stays the last field).  logit_bias: token
    # id -> bias in -100 .. 100, added to the logit before the penalties; min_tokens: no eos_token_ids entry is emitted
    # before this many tokens are generated; min_p in [0, 1]: sampled requests keep only tokens with p >= min_p * p_max.
    # A constrained request decodes eagerly and can ask for logprobs only with logprobs_mode = "processed_logprobs"
    logit_bias: Optional[Dict[int, float]] = field(default=None, kw_only=True)
    min_tokens: int = field(default=0, kw_only=True)
    min_p: float = field(default=0.0, kw_only=True)
    # None / "raw_logprobs": `logprobs` scores the model's raw softmax (not combinable with temperature > 0, penalties or
    # constraints); "processed_logprobs": the distribution the token was chosen from, combinable with all of them
    # (init=False and the class's keyword_argument decorator: taken by keyword only, the generated signature as it was)
    logprobs_mode: Optional[str] = field(default=None, init=False)
    # token masks, by keyword only like logprobs_mode.  allowed_token_ids: the only token ids the request may emit;
    # guided_choice: token id SEQUENCES (there is no tokenizer offline) of which the request emits exactly one and ends
    # there.  At most one of the two; such a request decodes eagerly
    allowed_token_ids: Optional[List[int]] = field(default=None, init=False)
    guided_choice: Optional[List[List[int]]] = field(default=None, init=False)
    prompt_logprobs: Optional[int] = None   # 0..20: the log-probability of every prompt token given what stands before it,
                                            # with that many alternatives per position; combinable with everything above


class OfflineInferenceEngine:
    def __init__(self, language_model, vision_model, dtype: torch.dtype, device: str = "cuda:0",
                 max_running_requests: int = 32, token_budgets: int = 2048, image_budgets: int = 8,
                 max_context: int = 4096, kv_cache_gib: Optional[float] = None, warm_up: bool = True,
                 graph_sampling: bool = False, graph_penalties: bool = False):
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        shape = language_model.language_model.shape
        self.n_image_tokens = (vision_model.shape.image_size // vision_model.shape.patch_size) ** 2
        blocks_per_seq = (max_context + 15) // 16
        per_block = shape.num_hidden_layers * 2 * 16 * shape.num_key_value_heads * shape.head_dim * 2
        n_blocks = int(kv_cache_gib * (1 << 30) // per_block) if kv_cache_gib else blocks_per_seq * (max_running_requests + 2)
        sched = BatchSchedulerConfig(priority="prefill", max_running_requests=max_running_requests,
                                     chunked_prefill=True, token_budgets=token_budgets, image_budgets=image_budgets)
        self.node = build_node("EPD0", "EPD", language_model, vision_model, shape, dtype, self.device, n_blocks,
                               2 * max_running_requests + 2, self.n_image_tokens, sched,
                               max_blocks_per_seq=blocks_per_seq, graph_sampling=graph_sampling,
                               graph_penalties=graph_penalties)
        self.cluster = LocalCluster([self.node])
        self.creator = InstructionCreator(image_token_id=language_model.image_token_id,
                                          n_image_tokens_per_image=self.n_image_tokens, block_size=16, ignore_eos=True,
                                          max_position_embeddings=shape.max_position_embeddings)
        self.processor = ClipImageProcessor(size=vision_model.shape.image_size)
        self.vocab_size = getattr(shape, "vocab_size", None)      # logit_bias ids and token masks are checked against it
        if warm_up:
            warm_library_gemms(language_model, token_budgets, max_running_requests)
            size = vision_model.shape.image_size
            self.node.executor.image_embed_executor.warmup(torch.zeros(1, 3, size, size), image_budgets)
            self.node.executor.fill_executor.graph_decoder.warmup(list(range(4, max_running_requests + 1, 4)))

    @classmethod
    def from_checkpoint(cls, model_path: str, dtype: torch.dtype = torch.float16, device: str = "cuda:0", **kw):
        from hydrainfer_amd.model.loader import load_llava
        lm, vm = load_llava(model_path, dtype, device)
        return cls(lm, vm, dtype, device, **kw)

    def generate(self, requests: List[OfflineRequest]) -> List[OfflineInferenceOutput]:
        import time
        rcbs = []
        with quiet_gc():
            for i, r in enumerate(requests):
                pixels = self.processor.process(r.image) if r.image is not None else None
                req = TokenRequest(request_id=i, token_ids=list(r.token_ids), pixel_values=pixels,
                                   image_size=(r.image.size[1], r.image.size[0]) if r.image is not None else (0, 0),
                                   image_hash=compute_image_hash(r.image) if r.image is not None else 0,
                                   sampling_params=SamplingParameters(r.max_tokens, list(r.eos_token_ids), r.logprobs,
                                                                      r.top_logprobs, r.frequency_penalty,
                                                                      r.presence_penalty, r.repetition_penalty,
                                                                      r.temperature, r.top_p, r.top_k, r.seed,
                                                                      prompt_logprobs=r.prompt_logprobs,
                                                                      logit_bias=r.logit_bias, min_tokens=r.min_tokens,
                                                                      min_p=r.min_p, logprobs_mode=r.logprobs_mode,
                                                                      allowed_token_ids=r.allowed_token_ids,
                                                                      guided_choice=r.guided_choice),
                                   token_params=r.token_params)
                rcb = self.creator.process(req, vocab_size=self.vocab_size)
                rcb.metric.arrival_time = time.perf_counter()
                rcbs.append(rcb)
                self.cluster.add_request(rcb)
                if (i + 1) % 8 == 0:
                    self.cluster.step()          # the GPU starts on the first ones while the rest is prepared
            while not self.cluster.idle():
                self.cluster.step()
        outs = []
        for rcb in rcbs:
            t = rcb.metric.token_times
            outs.append(OfflineInferenceOutput(
                output_token_ids=list(rcb.output_token_ids), arrival_time=rcb.metric.arrival_time,
                finished_time=rcb.metric.finished_time, token_times=list(t),
                ttft=t[0] - rcb.metric.arrival_time if t else -1.0,
                tpot=[b - a for a, b in zip(t, t[1:])], output_logprobs=list(rcb.output_logprobs),
                prompt_logprobs=list(rcb.prompt_logprobs)))
        return outs
