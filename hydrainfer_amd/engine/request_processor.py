"""Request -> instruction chain — mirror of hydrainfer/engine/request_processor.py:47-173
(InstructionCreator) without the tokenizer / image processor (the caller passes token ids and
pre-processed pixel values; there are no checkpoints or tokenizers offline)."""
import secrets
from dataclasses import dataclass
from typing import List, Optional, Tuple

import xxhash

from hydrainfer_amd.engine.isa import (EPMigrate, ImageEmbed, ImageEmbedFill, InstructionListBuilder,
                                       PDMigrate, PullCache, TextFill)
from hydrainfer_amd.engine.rcb import (MAX_TOP_LOGPROBS, PROCESSED_LOGPROBS, RequestControlBlock, RequestMetaData,
                                       SamplingParameters, ScenarioClassifier, TokenParameters, check_logprobs_mode)
from hydrainfer_amd.memory.shared_cache import compute_hash
from hydrainfer_amd.sampling import (PenaltyHistory, TokenConstraints, TokenMask, check_constraints, check_penalties,
                                     check_sampling, check_token_mask, is_constrained, is_penalized, is_sampled)


@dataclass
class TokenRequest:
    """What is left of hydrainfer.request.Request once tokenizer and image processor have run."""
    request_id: int
    token_ids: List[int]                       # prompt, one image_token_id per image
    pixel_values: object = None                # (1, C, H, W) tensor or None
    image_size: Tuple[int, int] = (336, 336)   # (height, width) of the original image
    image_hash: int = 0
    sampling_params: SamplingParameters = None
    token_params: Optional[TokenParameters] = None     # None: every image token, no pruning


def pruned_image_hash(image_hash: int, n_tokens: int, strategy: str) -> int:
    """What stands in for a PRUNED image in the prefix-cache block hashes and in ImageEmbed.hashes: a function of (image
    hash, kept count, strategy).  The KV of a block of image placeholders depends on which tokens were kept, so it must
    not share a hash with the unpruned prompt of the same image (whose stand-in stays the image hash itself).  63 bits:
    exact as an int64 beside the token ids."""
    h = xxhash.xxh64()
    h.update(b"focal")
    h.update(int(image_hash).to_bytes(16, "little", signed=True))
    h.update(int(n_tokens).to_bytes(8, "little"))
    h.update(strategy.encode())
    return h.intdigest() >> 1


class InstructionCreator:
    def __init__(self, image_token_id: int = 32000, n_image_tokens_per_image: int = 576,
                 block_size: int = 16, ignore_eos: bool = True, eos_token_id: int = 2,
                 max_position_embeddings: int = 4096, pruning_strategy: str = "rank"):
        self.pruning_strategy = pruning_strategy       # 'rank' | 'row' (layer/token_prunning.py) for 'focal' requests
        self.max_position_embeddings = max_position_embeddings
        self.image_token_id = image_token_id
        self.n_image_tokens_per_image = n_image_tokens_per_image
        self.block_size = block_size
        self.ignore_eos, self.eos_token_id = ignore_eos, eos_token_id
        self.scenario_classifier = ScenarioClassifier()

    def _pruned_count(self, request: TokenRequest) -> Optional[int]:
        """The request's image-token count under its token_params, None = unpruned.  What the reference declares and
        this engine does not implement is refused here, not ignored."""
        tp = request.token_params
        if tp is None:
            return None
        if tp.kv_cache_eviction_policy is not None:
            raise ValueError(f"request {request.request_id}: kv_cache_eviction_policy {tp.kv_cache_eviction_policy!r} is "
                             "declared by the request type but not implemented (only None)")
        if tp.token_pruning_policy is None:
            return None
        if tp.token_pruning_policy != "focal":
            raise ValueError(f"request {request.request_id}: unknown token_pruning_policy {tp.token_pruning_policy!r} "
                             "(None or 'focal')")
        n, full = tp.n_embed_output_tokens, self.n_image_tokens_per_image
        if not isinstance(n, int) or not 1 <= n <= full:
            raise ValueError(f"request {request.request_id}: n_embed_output_tokens {n!r} outside 1..{full}")
        if request.pixel_values is not None:
            from hydrainfer_amd.layer.token_prunning import check_counts
            check_counts([n], full, self.pruning_strategy)
        return n

    def _insert_image_tokens(self, token_ids: List[int], image_hashes: List[int], n_per_image: Optional[int] = None):
        """Each image placeholder becomes n_image_tokens placeholders; the prefix hashes are taken
        over the prompt with the image's content hash standing in for the inserted placeholders
        (request_processor.py:64-81: the LAST placeholder keeps the token id itself).  n_per_image: a pruned
        image's count; image_hashes then already are the pruned stand-ins."""
        out, to_hash, image_id, total = [], [], -1, 0
        for t in token_ids:
            if t == self.image_token_id:
                image_id += 1
                n = self.n_image_tokens_per_image if n_per_image is None else n_per_image
                total += n
                out.extend([self.image_token_id] * (n - 1))
                to_hash.extend([image_hashes[image_id]] * (n - 1))
            out.append(t)
            to_hash.append(t)
        return compute_hash(token_ids=to_hash, block_size=self.block_size, prefix=-1), out, total

    def _score_plan(self, own: List[int], expanded: List[int], n_per_image: int):
        """(score_targets, score_index) of the prompt Fill (engine/isa.py) — own: the request's token_ids, expanded: the
        prompt with every image placeholder repeated n_per_image times.  Row j of the prefill predicts expanded token
        j + 1; it scores it unless that token is an image placeholder; the last row's next token is the generated one."""
        own_index = []                                # expanded position -> index in `own`
        for i, t in enumerate(own):
            own_index += [i] * (n_per_image if t == self.image_token_id else 1)
        assert len(own_index) == len(expanded), "the expanded prompt does not follow the request's tokens"
        targets, index = [-1] * len(expanded), [-1] * len(expanded)
        for j in range(len(expanded) - 1):
            if expanded[j + 1] != self.image_token_id:
                targets[j], index[j] = expanded[j + 1], own_index[j + 1]
        return targets, index

    def process(self, request: TokenRequest, vocab_size: Optional[int] = None) -> RequestControlBlock:
        """vocab_size: None (unchecked), or the number of tokens the model scores: a logit_bias id at or above it is
        refused (the kernel would ignore it: the client would never learn that the bias did nothing).  A request with
        allowed_token_ids or guided_choice needs it: its masks are as wide as the rows they mask."""
        rcb = RequestControlBlock()
        rcb.request_id = request.request_id
        sp = request.sampling_params or SamplingParameters()
        top = sp.top_logprobs
        if not isinstance(sp.logprobs, bool):
            raise ValueError(f"request {request.request_id}: logprobs {sp.logprobs!r} must be a bool")
        if not isinstance(top, int) or isinstance(top, bool) or not 0 <= top <= MAX_TOP_LOGPROBS:
            raise ValueError(f"request {request.request_id}: top_logprobs {top!r} outside 0..{MAX_TOP_LOGPROBS}")
        if top > 0 and not sp.logprobs:
            raise ValueError(f"request {request.request_id}: top_logprobs = {top} needs logprobs = True")
        ask = sp.prompt_logprobs
        if ask is not None and (not isinstance(ask, int) or isinstance(ask, bool) or not 0 <= ask <= MAX_TOP_LOGPROBS):
            raise ValueError(f"request {request.request_id}: prompt_logprobs {ask!r} must be None or an integer "
                             f"0..{MAX_TOP_LOGPROBS}")
        try:
            mode = check_logprobs_mode(getattr(sp, "logprobs_mode", None), sp.logprobs)
            penalties = check_penalties(sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty)
            sampling = check_sampling(sp.temperature, sp.top_p, sp.top_k, sp.seed)
            logit_bias, min_tokens, min_p = check_constraints(sp.logit_bias, sp.min_tokens, sp.min_p)
            allowed, choices = check_token_mask(getattr(sp, "allowed_token_ids", None), getattr(sp, "guided_choice", None),
                                                vocab_size)
        except ValueError as e:
            raise ValueError(f"request {request.request_id}: {e}") from None
        rcb.sampling_params = SamplingParameters(sp.max_tokens, list(sp.eos_token_ids), sp.logprobs, top, *penalties,
                                                 *sampling, prompt_logprobs=ask, logit_bias=logit_bias,
                                                 min_tokens=min_tokens, min_p=min_p, logprobs_mode=mode,
                                                 allowed_token_ids=allowed, guided_choice=choices)
        # raw scores (hx_logprob_rows) describe the raw argmax: refused beside anything that changes the choice.  The
        # processed mode scores the choice itself (hx_sample_rows_logprobs) and combines with all of it.
        raw_scores = sp.logprobs and mode != PROCESSED_LOGPROBS
        hint = f' (logprobs_mode = "{PROCESSED_LOGPROBS}" scores the token under the distribution it was chosen from)'
        if vocab_size is not None and logit_bias and max(logit_bias) >= vocab_size:
            raise ValueError(f"request {request.request_id}: logit_bias names token {max(logit_bias)}, the vocabulary has "
                             f"{vocab_size}")
        if min_tokens > sp.max_tokens:
            raise ValueError(f"request {request.request_id}: min_tokens {min_tokens} exceeds max_tokens {sp.max_tokens}")
        if raw_scores and (logit_bias or min_tokens > 0 or min_p > 0):
            raise ValueError(f"request {request.request_id}: logit_bias / min_tokens / min_p cannot be combined with "
                             "logprobs yet: hx_logprob_rows scores the raw logits and names the raw argmax, not the "
                             "constrained choice (prompt_logprobs, which scores the prompt from raw logits by "
                             "definition, can be)" + hint)
        masked = allowed is not None or choices is not None
        if raw_scores and masked:
            raise ValueError(f"request {request.request_id}: allowed_token_ids / guided_choice cannot be combined with "
                             "logprobs yet: hx_logprob_rows scores the raw logits and names the raw argmax, not the "
                             "masked choice (prompt_logprobs, which scores the prompt from raw logits by definition, "
                             "can be)" + hint)
        if choices is not None and min_tokens > 0:
            raise ValueError(f"request {request.request_id}: min_tokens cannot be combined with guided_choice: the "
                             "request ends where its choice ends")
        if is_sampled(rcb.sampling_params):
            if raw_scores:
                raise ValueError(f"request {request.request_id}: temperature > 0 cannot be combined with logprobs yet: "
                                 "OpenAI reports the log-probability of the sampled token, hx_logprob_rows that of the "
                                 "greedy one" + hint)
            if rcb.sampling_params.seed is None:
                # 63 random bits, kept with the request: a finished request can be replayed from its parameters
                rcb.sampling_params.seed = secrets.randbits(63)
        if is_penalized(rcb.sampling_params):
            if raw_scores:
                raise ValueError(f"request {request.request_id}: frequency / presence / repetition penalties cannot be "
                                 "combined with logprobs yet: the score of a penalised choice needs the log-softmax "
                                 "kernel to see the penalties, a follow-up change" + hint)
            rcb.penalty_history = PenaltyHistory()
        if not self.ignore_eos:
            rcb.sampling_params.eos_token_ids.append(self.eos_token_id)
        if is_constrained(rcb.sampling_params):       # (after the server's own end-of-sequence id: min_tokens holds it back too)
            rcb.token_constraints = TokenConstraints(logit_bias, rcb.sampling_params.eos_token_ids, min_tokens)
        if masked:
            # (after the server's own end-of-sequence id as well) min_tokens bans every end-of-sequence id for a while: a set
            # of nothing else would leave the row all -inf — the kernel's degenerate row, whose id 0 may lie outside the set
            if allowed is not None and min_tokens > 0 and set(allowed) <= set(rcb.sampling_params.eos_token_ids):
                raise ValueError(f"request {request.request_id}: min_tokens = {min_tokens} with allowed_token_ids that are "
                                 "all end-of-sequence ids leaves no token to emit")
            rcb.token_mask = TokenMask(vocab_size, allowed, choices)

        has_image = request.pixel_values is not None
        n_keep = self._pruned_count(request)
        if not has_image:
            n_keep = None
        image_hashes = [request.image_hash] if has_image else []
        if n_keep is not None:
            image_hashes = [pruned_image_hash(h, n_keep, self.pruning_strategy) for h in image_hashes]
        n_images = request.token_ids.count(self.image_token_id)
        hashes, token_ids, n_image_tokens = self._insert_image_tokens(request.token_ids, image_hashes, n_keep)
        n_prompt = len(token_ids)
        # position ids run to n_prompt + max_tokens - 2; the rotary table (cos_sin) has
        # max_position_embeddings rows and the kernels index it unchecked
        if n_prompt + rcb.sampling_params.max_tokens - 1 > self.max_position_embeddings:
            raise ValueError(f"request {request.request_id}: {n_prompt} prompt tokens + "
                             f"{rcb.sampling_params.max_tokens} generated exceed max_position_embeddings "
                             f"= {self.max_position_embeddings}")
        token_ids = token_ids + [-1] * (rcb.sampling_params.max_tokens - 1)   # filled in while decoding
        mask = [t == self.image_token_id for t in token_ids]
        ids = list(range(len(token_ids)))        # position ids == virtual cache ids

        b = InstructionListBuilder()
        if has_image:
            image_cache_ids = list(range(n_image_tokens))
            b.append(ImageEmbed(request.pixel_values, image_cache_ids, [request.image_size], image_hashes,
                                n_keep=n_keep, strategy=self.pruning_strategy))
            b.append(EPMigrate())
            b.append(PullCache())
            prefill = ImageEmbedFill(image_cache_ids, mask[:n_prompt], token_ids[:n_prompt], ids[:n_prompt],
                                     ids[:n_prompt], True, None, hashes)
        else:
            prefill = TextFill(token_ids[:n_prompt], ids[:n_prompt], ids[:n_prompt], True, None, hashes)
        if ask is not None:
            # a skipped token has no logits: the prompt neither matches nor publishes prefix-cache blocks (the image
            # cache's hashes, ImageEmbed.hashes, are another matter and stay)
            prefill.hashes = None
            prefill.score_targets, prefill.score_index = self._score_plan(
                request.token_ids, token_ids[:n_prompt], self.n_image_tokens_per_image if n_keep is None else n_keep)
            rcb.prompt_logprobs = [None] * len(request.token_ids)
        b.append(prefill)
        b.append(PDMigrate())
        b.append(PullCache())
        last = prefill
        for i in range(n_prompt, len(token_ids)):
            decode = TextFill(token_ids[i:i + 1], ids[i:i + 1], ids[i:i + 1], True, None, None)
            b.append(decode)
            last.sample_dst = decode
            last = decode

        rcb.instructions = b.build_instruction_list()
        rcb.request_metadata = RequestMetaData(n_images=n_images, n_prompt_tokens=n_prompt,
                                               n_image_tokens=n_image_tokens,
                                               n_text_tokens=n_prompt - n_image_tokens)
        rcb.scenario_type = self.scenario_classifier.classify(
            n_text_tokens=rcb.request_metadata.n_text_tokens, n_output_tokens=rcb.sampling_params.max_tokens)
        return rcb
