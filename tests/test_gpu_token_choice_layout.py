"""GPU: the scored and the masked step reach their launch through ONE packed buffer (pack_scored_step / pack_masked_step,
to_device) and give bit for bit what the same tables give when each is uploaded on its own.  5 rows of 130 logits: 130 is
no multiple of 8 (the LDS row padding) and none of 32 (the last mask word is partial)."""
import numpy as np
import pytest
import torch

from hydrainfer_amd._C.kernel.norm import logprob_rows_bytes
from hydrainfer_amd.sampling import (GREEDY_RECORD, NO_PENALTIES, PenaltyHistory, TokenMask, pack_constrained_step,
                                     pack_masked_step, pack_scored_step, sample_rows_logprobs, sample_rows_masked)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROWS, N, K = 5, 130, 3


def _entries():
    """(history, penalties, record, bias, want, mask) per row: a row without a history, rows without a bias, rows that are
    not scored, two rows on one mask object (its last allowed token in the partial last word), a row without a mask."""
    a, b = TokenMask(N, allowed_token_ids=[3, 64, 127, 129]), TokenMask(N, guided_choice=[[5, 6], [128, 8]])
    bias = (np.asarray([3, 129], np.int32), np.asarray([2.5, -1.0], np.float32))
    ban = (np.asarray([64], np.int32), np.asarray([-np.inf], np.float32))
    return [(PenaltyHistory([4, 4, 129]), (0.5, 0.25, 1.5), (0.7, 0.9, 50, 77, 4, 0.05), bias, 0, a.current()),
            (None, NO_PENALTIES, GREEDY_RECORD, None, -1, None),
            (PenaltyHistory(), NO_PENALTIES, (1.0, 1.0, 0, (1 << 63) - 1, 1), None, -1, b.current()),
            (PenaltyHistory([127]), (0.0, 0.0, 2.0), GREEDY_RECORD, ban, 0, a.current()),
            (PenaltyHistory([7, 1, 7, 7]), (-0.5, 0.0, 1.0), (0.3, 0.5, 0, 9, 6, 0.0), None, 0, None)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_one_packed_buffer_gives_what_separate_uploads_give(dtype):
    entries = _entries()
    logits = (torch.randn(ROWS, N, generator=torch.Generator().manual_seed(130)) * 3).to(dtype).to(DEV)
    out = lambda: torch.zeros(logprob_rows_bytes(ROWS, K), dtype=torch.uint8, device=DEV)
    alone = lambda views: [v.clone().to(DEV) for v in views]
    # part one: the scored step against the constrained step's tables and a `want` of its own
    *tables, want = pack_scored_step([e[:5] for e in entries]).to_device(DEV)
    packed, by_hand = out(), out()
    sample_rows_logprobs(logits, *tables, top_k=K, want=want, out=packed)
    want_alone = torch.tensor([e[4] for e in entries], dtype=torch.int32).to(DEV)
    sample_rows_logprobs(logits, *alone(pack_constrained_step([e[:4] for e in entries]).views()), top_k=K, want=want_alone,
                         out=by_hand)
    assert torch.equal(packed.cpu(), by_hand.cpu()), "sample_rows_logprobs: the packed scored step differs"
    assert packed.cpu().any(), "the launch wrote nothing"
    # part two: the masked step against its own host views, each uploaded alone
    step = pack_masked_step(entries)
    *tables, want = step.to_device(DEV)
    *tables_alone, want_alone = alone(step.views())
    packed, by_hand = out(), out()
    sample_rows_masked(logits, *tables, top_k=K, want=want, out=packed)
    sample_rows_masked(logits, *tables_alone, top_k=K, want=want_alone, out=by_hand)
    assert torch.equal(packed.cpu(), by_hand.cpu()), "sample_rows_masked: the packed masked step differs"
    ids = packed.cpu()[:8 * ROWS].view(torch.int64).tolist()
    assert ids[0] in (3, 64, 127, 129) and ids[2] in (5, 128) and ids[3] in (3, 127, 129), "a masked row left its mask"
