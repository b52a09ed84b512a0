"""No GPU: the host decisions of the captured decode step, each in its one place — which batches
BatchFillExecutor._decode_rows sends to the decoder as which DecodeStep (every request kind against every decoder
ability), step_variant, and the resident-table helper over a numpy packer.  The expected steps are literals, recorded
from the code as it stood before these decisions were gathered (the rule for a row's identity and what the stager writes
for it: tests/test_decode_stager.py)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

from hydrainfer_amd._lib import HydraHipError
from hydrainfer_amd.engine.executor import DecodeStep, PendingToken, decoder_abilities
from hydrainfer_amd.engine.graph_decode import VARIANTS, ResidentTable, step_variant
from tests.test_graph_penalties_cpu import PenalisedDecoder, penalised
from tests.test_graph_sampling_cpu import Decoder, executor, request

# ---- eligibility: decoder ability x request kind x alone / beside a plain greedy request

DECODERS = {"bare": lambda: NS(fits=lambda n, b: n <= 8 and b <= 4), "off": lambda: Decoder(False),
            "sampled": lambda: Decoder(True), "penalised": lambda: PenalisedDecoder(16)}
KINDS = ("greedy", "drawn", "penalised_16", "penalised_17", "logprobs", "constraints", "mask", "score_targets", "two_tokens",
         "no_sample", "pending_same", "pending_other", "continued_pending", "uncontinued_pending")

ALONE, BESIDE = (5, 20, 660, 21, [4, 41], 1), (5, 17, 641, 18, [3, 40], 0)      # the request's row, the greedy neighbour's
AHEAD = (-3,) + ALONE[1:]                                                       # its input is row 2 of the pending launch
LATER = (-3, 21, 661, 22, [4, 41], 1)                                           # the penalised request one token further
DRAW, AT_T0, PEN = (0.8, 0.9, 20, 7, -17), (0.0, 1.0, 0, 0, -17), (0.7, 0.5, 1.3, "out")
# (decoder, kind) -> the step of the request alone; beside the greedy request every list gains a leading BESIDE / None.
# Every other combination is None: the batch runs eagerly
ELIGIBLE = {
    ("bare", "greedy"): ([ALONE], None, None),
    ("bare", "pending_same"): ([AHEAD], None, None),
    ("off", "greedy"): ([ALONE], None, None),
    ("off", "pending_same"): ([AHEAD], None, None),
    ("sampled", "greedy"): ([ALONE], [None], None),
    ("sampled", "drawn"): ([ALONE], [DRAW], None),
    ("sampled", "pending_same"): ([AHEAD], [None], None),
    ("penalised", "greedy"): ([ALONE], [None], None),
    ("penalised", "drawn"): ([ALONE], [DRAW], None),
    ("penalised", "pending_same"): ([AHEAD], [None], None),
    ("penalised", "penalised_16"): ([ALONE], [AT_T0], [PEN]),
    ("penalised", "continued_pending"): ([LATER], [AT_T0], [PEN]),
}


def make(kind, dec):
    """One request of the kind: sid 1, three tokens out, its next input at position 20."""
    if kind == "greedy":
        return request(1, 3, 20)
    if kind == "drawn":
        return request(1, 3, 20, temperature=0.8, top_p=0.9, top_k=20, seed=7)
    if kind in ("penalised_16", "penalised_17"):
        return penalised(1, 3, 20, max_tokens=int(kind[-2:]))
    if kind == "logprobs":
        return request(1, 3, 20, logprobs=True)
    if kind == "constraints":
        return request(1, 3, 20, token_constraints=object())
    if kind == "mask":
        return request(1, 3, 20, token_mask=object())
    if kind == "score_targets":
        return request(1, 3, 20, score_targets=[1])
    if kind in ("two_tokens", "no_sample"):
        rcb, inst = request(1, 3, 20)
        if kind == "two_tokens":
            inst.token_ids = [5, 6]
        else:
            inst.sample = False
        return rcb, inst
    if kind in ("pending_same", "pending_other"):
        return request(1, 3, 20, token=PendingToken(4 if kind == "pending_same" else 3, 2))
    # a penalised request whose newest token is still on the device, with or without a log that continues for it
    rcb, inst = penalised(1, 4, 21, token=PendingToken(4, 2))
    rcb.output_token_ids[3] = inst.token_ids[0]
    if kind == "continued_pending" and hasattr(dec, "log_table"):
        dec.log_table.step([(1, 3, [0, 1, 2])])
    return rcb, inst


@pytest.mark.parametrize("beside", [False, True], ids=["alone", "beside_greedy"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dec_name", list(DECODERS))
def test_eligibility_table(dec_name, kind, beside):
    fill = executor(False)
    dec = fill.graph_decoder = DECODERS[dec_name]()
    fill.pending = (4, [])
    batch = ([request(0, 1, 17)] if beside else []) + [make(kind, dec)]
    got = fill._decode_rows(batch)
    want = ELIGIBLE.get((dec_name, kind))
    if want is None:
        assert got is None
        return
    if beside:
        want = tuple(None if part is None else [BESIDE if part is want[0] else None] + part for part in want)
    assert type(got) is DecodeStep
    rows, records, penalties = got
    if penalties is not None:                  # the request's own token list goes along, not a copy of it
        penalties = [None if p is None else p[:3] + ("out" if p[3] is rcb.output_token_ids else p[3],)
                     for p, (rcb, _) in zip(penalties, batch)]
    assert (rows, records, penalties) == want


def test_decoder_abilities_default_to_off():
    assert decoder_abilities(NS()) == (False, 0, False)
    assert decoder_abilities(NS(sampled=False, penalized=True, penalty_log_cap=16)) == (False, 0, False)
    assert decoder_abilities(NS(sampled=True, launch_cohort=None)) == (True, 0, True)
    assert decoder_abilities(PenalisedDecoder(16)) == (True, 16, False)


# ---- step_variant

SOME_RECORDS, SOME_PENALTIES = [None, (0.8, 1.0, 0, 7, -3), (0.0, 1.0, 0, 0, -5)], [None, None, (0.7, 0.5, 1.3)]
NO_SAMPLED = "sampling records for a decoder without a sampled variant"
NO_PENALISED = "penalties for a decoder without a penalised variant"
NO_RECORD = "a penalised row needs a record"


@pytest.mark.parametrize("n_variants", [1, 2, 3])
@pytest.mark.parametrize("penalties", [None, [None] * 3, SOME_PENALTIES], ids=["p_none", "p_all_none", "p_some"])
@pytest.mark.parametrize("records", [None, [None] * 3, SOME_RECORDS], ids=["r_none", "r_all_none", "r_some"])
def test_step_variant(records, penalties, n_variants):
    has_records, has_penalties = records is SOME_RECORDS, penalties is SOME_PENALTIES
    if has_records and n_variants < 2:
        error = NO_SAMPLED
    elif has_penalties and n_variants < 3:
        error = NO_PENALISED
    elif has_penalties and not has_records:
        error = NO_RECORD
    else:
        error = None
    if error:
        with pytest.raises(HydraHipError, match=error):
            step_variant(records, penalties, VARIANTS[:n_variants])
        return
    want = "penalized" if has_penalties else "sampled" if has_records else "greedy"
    assert step_variant(records, penalties, VARIANTS[:n_variants]) == \
        (want, records if has_records else None, penalties if has_penalties else None)


def test_step_variant_wants_a_record_on_every_penalised_row():
    with pytest.raises(HydraHipError, match=NO_RECORD):
        step_variant([(0.8, 1.0, 0, 7, -3), None], [None, (0.7, 0.5, 1.3)])
    assert step_variant([(0.8, 1.0, 0, 7, -3), None], [(0.7, 0.5, 1.3), None])[0] == "penalized"


# ---- the resident table


def pack_pairs(rows, out=None):
    """A packer in the manner of pack_resident_records: None is the row (0, -1)."""
    if out is None:
        out = np.empty((len(rows), 2), dtype=np.int32)
    out[:] = [(0, -1) if r is None else r for r in rows]
    return out


def test_resident_table_copies_only_what_differs():
    table = ResidentTable(pack_pairs, 2, 8, "cpu")
    assert table.tensor.tolist() == [[0, -1]] * 8 and table.mirror == [None] * 8
    dst, bufs = table.tensor.data_ptr(), [t.data_ptr() for t in table.staging]
    assert bufs[0] != bufs[1]
    want = [(1, 2), None, (3, 4), None]
    assert table.update(0, want) == (dst, bufs[0], 2 * 4)                     # the full padded size, from this turn's buffer
    assert table.stage[0][:4].tolist() == [[1, 2], [0, -1], [3, 4], [0, -1]] and table.mirror[:4] == want
    assert table.update(1, list(want)) is None                                # the device holds it
    changed = [(1, 2), None, (3, 5), None]
    assert table.update(1, changed) == (dst, bufs[1], 2 * 4)                  # one row differs: the other turn's buffer
    assert table.stage[1][:4].tolist() == [[1, 2], [0, -1], [3, 5], [0, -1]]
    assert table.stage[0][2].tolist() == [3, 4]                               # the first turn's buffer was left alone
    # a smaller step compares only its own rows: rows 2 and 3 keep what they hold, on the device and in the mirror
    assert table.update(0, [(1, 2), None]) is None
    assert table.update(0, [(1, 2), (9, 9)]) == (dst, bufs[0], 2 * 2)
    assert table.mirror == [(1, 2), (9, 9), (3, 5), None] + [None] * 4
    table.reset()
    assert table.mirror == [None] * 8 and table.tensor.tolist() == [[0, -1]] * 8
    assert table.update(1, [None] * 4) is None
