"""LLaVA-1.5 language side — mirrors hydrainfer/model/llava.py:110-140 (LlavaLanguageModel):
token embedding, image-token rows overwritten by projected image features, Llama decoder,
greedy token ids out."""
from typing import Optional

import torch
from torch import Tensor

from hydrainfer_amd.model.llama import LanguageModelParameters, LlamaForCausalLM


class LlavaLanguageModel:
    def __init__(self, language_model: LlamaForCausalLM, image_token_id: int = 32000):
        self.language_model = language_model
        self.image_token_id = image_token_id

    def embed(self, input_ids: Tensor, image_features: Optional[Tensor],
              image_row_index: Optional[Tensor] = None) -> Tensor:
        input_embeds = self.language_model.embed(input_ids)
        if image_features is not None:
            feats = image_features.reshape(-1, input_embeds.shape[-1]).to(input_embeds.dtype)
            if image_row_index is not None:       # rows known on the host: no device->host sync
                input_embeds.index_copy_(0, image_row_index, feats)
            else:
                mask = input_ids == self.image_token_id                   # llava.py:133-135
                input_embeds[mask] = feats
        return input_embeds

    def forward_logits(self, input_ids: Tensor, image_features: Optional[Tensor], position_ids: Tensor,
                       model_params: LanguageModelParameters) -> Tensor:
        embeds = self.embed(input_ids, image_features, getattr(model_params, "image_row_index", None))
        return self.language_model.forward_logits(embeds, position_ids, model_params)

    def forward(self, input_ids: Tensor, image_features: Optional[Tensor], position_ids: Tensor,
                model_params: LanguageModelParameters) -> Tensor:
        return torch.argmax(self.forward_logits(input_ids, image_features, position_ids, model_params), dim=-1)

    def forward_logprobs(self, input_ids: Tensor, image_features: Optional[Tensor], position_ids: Tensor,
                         model_params: LanguageModelParameters, top_k: int = 0, out: Optional[Tensor] = None):
        """forward() plus per-token log-probabilities: (ids, logprobs, top_ids, top_logprobs), one launch behind the
        logits (hx_logprob_rows); ids follow the same rule as forward's argmax."""
        from hydrainfer_amd._C.kernel.norm import logprob_rows
        return logprob_rows(self.forward_logits(input_ids, image_features, position_ids, model_params), top_k, out)

    def forward_penalized(self, input_ids: Tensor, image_features: Optional[Tensor], position_ids: Tensor,
                          model_params: LanguageModelParameters, hist_ids: Tensor, hist_counts: Tensor, cu_hist: Tensor,
                          penalties: Tensor, out: Optional[Tensor] = None) -> Tensor:
        """forward() under frequency / presence / repetition penalties: one launch behind the logits
        (hx_penalized_argmax_rows) with the rows' (token, count) tables as a CSR; a row with an empty table gets the id
        forward's argmax gives."""
        from hydrainfer_amd.sampling import penalized_argmax_rows
        return penalized_argmax_rows(self.forward_logits(input_ids, image_features, position_ids, model_params),
                                     hist_ids, hist_counts, cu_hist, penalties, out)

    def forward_sampled(self, input_ids: Tensor, image_features: Optional[Tensor], position_ids: Tensor,
                        model_params: LanguageModelParameters, sample_params: Tensor, hist_ids: Optional[Tensor] = None,
                        hist_counts: Optional[Tensor] = None, cu_hist: Optional[Tensor] = None,
                        penalties: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
        """forward() with sampled decoding: one launch behind the logits (hx_sample_rows) with the rows' sampling records
        and, optionally, their (token, count) tables; a row with temperature 0 gets the id forward_penalized gives."""
        from hydrainfer_amd.sampling import sample_rows
        return sample_rows(self.forward_logits(input_ids, image_features, position_ids, model_params), sample_params,
                           hist_ids, hist_counts, cu_hist, penalties, out)

    def forward_constrained(self, input_ids: Tensor, image_features: Optional[Tensor], position_ids: Tensor,
                            model_params: LanguageModelParameters, sample_params: Tensor, bias_ids: Tensor,
                            bias_values: Tensor, cu_bias: Tensor, hist_ids: Optional[Tensor] = None,
                            hist_counts: Optional[Tensor] = None, cu_hist: Optional[Tensor] = None,
                            penalties: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
        """forward() under token constraints: one launch behind the logits (hx_sample_rows_constrained) with the rows'
        sampling records (min_p in word 3), their (token, bias) tables and, optionally, their (token, count) tables."""
        from hydrainfer_amd.sampling import sample_rows_constrained
        return sample_rows_constrained(self.forward_logits(input_ids, image_features, position_ids, model_params),
                                       sample_params, bias_ids, bias_values, cu_bias, hist_ids, hist_counts, cu_hist,
                                       penalties, out)

    def forward_scored(self, input_ids: Tensor, image_features: Optional[Tensor], position_ids: Tensor,
                       model_params: LanguageModelParameters, sample_params: Tensor, bias_ids: Tensor, bias_values: Tensor,
                       cu_bias: Tensor, hist_ids: Optional[Tensor] = None, hist_counts: Optional[Tensor] = None,
                       cu_hist: Optional[Tensor] = None, penalties: Optional[Tensor] = None, *, top_k: int,
                       want: Optional[Tensor] = None, out: Optional[Tensor] = None):
        """forward_constrained() plus the scores of the processed distribution: (ids, logprobs, top_ids, top_logprobs),
        one launch behind the logits (hx_sample_rows_logprobs); the ids are forward_constrained()'s, a row with
        want < 0 is not scored."""
        from hydrainfer_amd.sampling import sample_rows_logprobs
        return sample_rows_logprobs(self.forward_logits(input_ids, image_features, position_ids, model_params),
                                    sample_params, bias_ids, bias_values, cu_bias, hist_ids, hist_counts, cu_hist,
                                    penalties, top_k=top_k, want=want, out=out)

    __call__ = forward
