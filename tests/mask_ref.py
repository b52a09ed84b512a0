"""Token masks, restated without the library (numpy and plain Python): the bit layout of a mask, and the float64
log-softmax over an allowed set that hx_sample_rows_masked's scores are held to."""
import numpy as np


def words_by_loop(token_ids, n):
    """The mask of `token_ids` over n tokens as a list of Python ints, one per 32 tokens, set bit by bit."""
    words = [0] * ((n + 31) // 32)
    for t in token_ids:
        words[t // 32] |= 1 << (t % 32)
    return words


def allowed_of(words, n):
    """The token ids below n whose bit is set in `words` (any integer sequence), ascending."""
    return [t for t in range(n) if (int(words[t // 32]) >> (t % 32)) & 1]


def masked_log_softmax(row, allowed):
    """row: the logits of one row (any float array); allowed: token ids -> float64 [n]: log-softmax over the allowed
    set, -inf outside it."""
    x = np.asarray(row, dtype=np.float64)
    allowed = np.asarray(sorted(allowed), dtype=np.int64)
    out = np.full(x.shape, -np.inf)
    z = x[allowed]
    m = z.max()
    out[allowed] = (z - m) - np.log(np.exp(z - m).sum())
    return out
