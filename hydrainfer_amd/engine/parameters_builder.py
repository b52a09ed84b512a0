"""Per-step model inputs — mirror of hydrainfer/engine/parameters_builder.py:11-97.

One builder per fill batch: add(rcb, inst) for every request, then
build_language_model_parameters().  Two deliberate differences from the reference:
  * the integer arrays (token ids, positions, sampled rows, and the six attention arrays) reach
    the device in two pinned H2D copies instead of 6 + 4 `torch.tensor(list, device=...)` calls;
  * a sequence's kv length is `max(cache_ids) + 1`, not `virtual_kv_cache.n_cache_tokens`
    (:69).  The two are equal except on the head chunk of a budget-chunked prefill, where the
    reference has already grown the cache to the whole prompt (scheduler.py:137 runs before the
    chunking at :172) and so lets the chunk attend to cache slots that hold no token yet."""
from dataclasses import dataclass
from typing import List, Optional

import torch
from torch import Tensor

from hydrainfer_amd.engine.isa import Fill, ImageEmbedFill
from hydrainfer_amd.engine.rcb import BatchRequest, RequestControlBlock
from hydrainfer_amd.layer.causal_attention import AttentionParameters, AttentionParametersBuilder
from hydrainfer_amd.memory.kv_cache import KVCache


@dataclass
class ScorePlan:
    """Which rows of a step score which prompt token (requests with sampling_params.prompt_logprobs) — pure host data
    plus its three index tensors.  The model narrows its last layer to `rows`, the sorted union of the step's sampling
    rows (FillInputs.selected_token_ids) and its scoring rows; everything else here is per union row."""
    rows: List[int]                   # batch rows that reach the logits, ascending (every row of an all-decode batch)
    targets: List[int]                # the prompt token a union row scores, -1: the row only samples
    dst: list                         # (rcb, index into rcb.prompt_logprobs) of a scoring union row, else None
    sample_pos: List[int]             # where selected_token_ids[i] stands in `rows`
    top_k: int                        # the largest prompt_logprobs of the step's scoring requests
    rows_tensor: Optional[Tensor] = None        # int64 on the device
    targets_tensor: Optional[Tensor] = None     # int32 on the device
    sample_pos_tensor: Optional[Tensor] = None  # int64 on the device, None if nothing samples


@dataclass
class FillInputs:
    input_ids: Tensor                 # int32 [n_tokens]
    position_ids: Tensor              # int32 [n_tokens]
    image_features: Optional[Tensor]  # [n_image_tokens, hidden] or None
    attention_params: List[AttentionParameters]
    all_sequences_decode: bool
    selected_token_ids: List[int]
    selected_token_ids_tensor: Optional[Tensor]   # int64 on the device
    image_row_index: Optional[Tensor] = None      # int64 on the device: rows that are image tokens
    score_plan: Optional[ScorePlan] = None        # None: no request of the step scores its prompt


class LanguageModelParametersBuilder:
    def __init__(self, image_block_manager, kv_cache_block_manager, n_layers: int, n_qo_heads: int,
                 n_kv_heads: int, head_dim: int, image_token_id: int, dtype: torch.dtype,
                 device: torch.device):
        self.image_block_manager = image_block_manager
        self.kv_cache_block_manager = kv_cache_block_manager
        self.n_layers, self.n_qo_heads, self.head_dim = n_layers, n_qo_heads, head_dim
        self.image_token_id = image_token_id
        self.dtype, self.device = dtype, device
        self.image_slot_ids: List[int] = []
        self.token_ids: List[int] = []
        self.position_ids: List[int] = []
        self.selected_token_ids: List[int] = []
        self.score_rows: List[int] = []          # batch rows that score a prompt token, their targets and destinations
        self.score_targets: List[int] = []
        self.score_dst: list = []
        self.score_top_k = 0
        self.all_single = True                   # every fill so far feeds one token (the attention builder's all-decode)
        self.attention_params_builder = AttentionParametersBuilder(
            num_qo_heads=n_qo_heads, num_kv_heads=n_kv_heads, head_dim=head_dim,
            block_size=kv_cache_block_manager.block_size, device=device)

    def add(self, rcb: RequestControlBlock, inst: Fill) -> None:
        assert isinstance(inst, Fill)
        if isinstance(inst, ImageEmbedFill):
            self.image_slot_ids += self.image_block_manager.v2p(rcb.virtual_image_cache,
                                                                inst.image_token_cache_ids)
        if inst.score_targets is not None:
            base = len(self.token_ids)
            for j, t in enumerate(inst.score_targets):
                if t >= 0:
                    self.score_rows.append(base + j)
                    self.score_targets.append(t)
                    self.score_dst.append((rcb, inst.score_index[j]))
            self.score_top_k = max(self.score_top_k, rcb.sampling_params.prompt_logprobs or 0)
        if len(inst.token_ids) != 1:
            self.all_single = False
        self.token_ids += inst.token_ids
        self.position_ids += inst.position_ids
        if inst.sample:
            self.selected_token_ids.append(len(self.token_ids) - 1)
        vc = rcb.virtual_kv_cache
        self.attention_params_builder.add_request(
            q_seq_len=len(inst.token_ids), kv_seq_len=max(inst.cache_ids) + 1,
            new_cache_slots=self.kv_cache_block_manager.v2p(vc, inst.cache_ids),
            block_table=vc.block_table)

    def add_batch(self, batch: BatchRequest) -> None:
        for rcb, inst in batch:
            self.add(rcb, inst)

    def _to_device(self, values: List[int], dtype=torch.int32) -> Tensor:
        t = torch.tensor(values, dtype=dtype)
        if self.device.type == "cuda":
            t = t.pin_memory().to(self.device, non_blocking=True)
        return t

    def build_score_plan(self) -> Optional[ScorePlan]:
        """The step's score plan (host lists only), None if no row scores."""
        if not self.score_rows:
            return None
        # an all-decode batch is never narrowed by the model (forward_hidden): every row reaches the logits
        rows = list(range(len(self.token_ids))) if self.all_single else sorted(set(self.selected_token_ids) | set(self.score_rows))
        at = {r: i for i, r in enumerate(rows)}
        targets, dst = [-1] * len(rows), [None] * len(rows)
        for r, t, d in zip(self.score_rows, self.score_targets, self.score_dst):
            targets[at[r]], dst[at[r]] = t, d
        return ScorePlan(rows, targets, dst, [at[r] for r in self.selected_token_ids], self.score_top_k)

    def build_language_model_parameters(self) -> FillInputs:
        plan = self.build_score_plan()
        n, n_sel, n_img = len(self.token_ids), len(self.selected_token_ids), len(self.image_slot_ids)
        n_image_rows = sum(t == self.image_token_id for t in self.token_ids)
        assert n_image_rows == n_img, "image token rows and cached image embeddings differ"
        image_rows = [i for i, t in enumerate(self.token_ids) if t == self.image_token_id] if n_img else []
        # (a step that scores: the plan's three index lists ride at the end of the same host-to-device copy)
        tail = plan.rows + plan.targets + plan.sample_pos if plan is not None else []
        flat = self._to_device(self.token_ids + self.position_ids + self.selected_token_ids +
                               self.image_slot_ids + image_rows + tail)
        input_ids, position_ids = flat[:n], flat[n:2 * n]
        selected = flat[2 * n:2 * n + n_sel].to(torch.int64) if n_sel else None
        image_features = None
        if n_img:
            cache = self.image_block_manager.get_layer_cache(layer_id=0).get_caches()[0]
            rows = cache.view(-1, self.n_qo_heads * self.head_dim)
            image_features = rows.index_select(0, flat[2 * n + n_sel:2 * n + n_sel + n_img]).to(self.dtype)
        for layer_id in range(self.n_layers):
            self.attention_params_builder.add_kv_cache(
                KVCache.from_token_cache(self.kv_cache_block_manager.get_layer_cache(layer_id)))
        attn = self.attention_params_builder.build_attention_parameters()
        at = 2 * n + n_sel + 2 * n_img          # where the plan's lists begin
        row_index = flat[at - n_img:at].to(torch.int64) if n_img else None
        if plan is not None:
            n_u = len(plan.rows)
            plan.rows_tensor = flat[at:at + n_u].to(torch.int64)
            plan.targets_tensor = flat[at + n_u:at + 2 * n_u].contiguous()
            plan.sample_pos_tensor = flat[at + 2 * n_u:].to(torch.int64) if n_sel else None
            assert attn[0].all_sequences_decode == self.all_single
        return FillInputs(input_ids, position_ids, image_features, attn, attn[0].all_sequences_decode,
                          self.selected_token_ids, selected, row_index, plan)
