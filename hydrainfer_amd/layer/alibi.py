"""ALiBi head slopes (Press et al., "Train Short, Test Long", 2022, section 3): the geometric schedule that BLOOM, MPT
and Baichuan-13B use in place of a rotary embedding.  Pass the result as `alibi_slopes` of
CausalGroupedQueryPageAttentionConfig (or straight to mha_varlen_fwd) after moving it to the device."""
import math

import torch
from torch import Tensor


def _power_of_two_slopes(n: int) -> list:
    # head k (1-based) of n = 2^m heads: 2^(-8k/n)
    return [2.0 ** (-8.0 * k / n) for k in range(1, n + 1)]


def alibi_slopes(n_heads: int) -> Tensor:
    """fp32 [n_heads].  A power-of-two head count n gets 2^(-8k/n), k = 1..n.  Any other count takes the schedule of
    the next lower power of two p, then every second slope (the 1st, 3rd, ...) of the schedule for 2p until n are
    there — the paper's interleaved extension, the one the BLOOM / MPT / Baichuan checkpoints were trained with."""
    if n_heads <= 0:
        raise ValueError("alibi_slopes: n_heads must be positive")
    p = 2 ** int(math.floor(math.log2(n_heads)))
    slopes = _power_of_two_slopes(p)
    if p != n_heads:
        slopes += _power_of_two_slopes(2 * p)[0::2][: n_heads - p]
    return torch.tensor(slopes, dtype=torch.float32)
