"""No GPU: the host side of penalties from the captured step — pack_penalty_records word for word, the slot table of the
resident token log as a pure host object (PenaltyLogTable), and which batches BatchFillExecutor._decode_rows sends to a
decoder with the penalised variant, with what (stand-ins for the decoder and the requests, in the manner of
tests/test_graph_sampling_cpu.py: nothing here touches a device)."""
import numpy as np
import pytest

from hydrainfer_amd._lib import HydraHipError
from hydrainfer_amd.engine.executor import PendingToken
from hydrainfer_amd.engine.graph_decode import PenaltyLogTable
from hydrainfer_amd.sampling import PenaltyHistory, pack_penalty_records
from tests.test_graph_sampling_cpu import Decoder, executor, f32, request


def test_pack_penalty_records_word_exact():
    got = pack_penalty_records([None, (0.7, 0.5, 1.3, 5), (-0.25, 0.0, 1.0, 0), (0.0, 2.0, 0.5, -1)])
    assert got.dtype == np.int32 and got.shape == (4, 4)
    assert got.view(np.uint32).tolist() == [[f32(0.0), f32(0.0), f32(1.0), 0xFFFFFFFF],
                                            [f32(0.7), f32(0.5), f32(1.3), 5],
                                            [f32(-0.25), f32(0.0), f32(1.0), 0],
                                            [f32(0.0), f32(2.0), f32(0.5), 0xFFFFFFFF]]
    out = np.full((4, 4), 9, dtype=np.int32)
    assert pack_penalty_records([None, (0.7, 0.5, 1.3, 5)], out[1:3]) is not None
    assert np.array_equal(out[1:3], got[:2]) and (out[0] == 9).all() and (out[3] == 9).all()


# ---- the slot table


def test_a_continuing_request_uploads_nothing():
    table = PenaltyLogTable(4, 16)
    slots, seeds = table.step([("a", 1, [11]), None, ("b", 3, [21, 22, 23, 24])])
    assert slots[1] == -1 and slots[0] != slots[2] and min(slots[0], slots[2]) >= 0
    assert sorted(seeds) == sorted([(slots[0], [11]), (slots[2], [21, 22, 23])])       # exactly tokens [0, L)
    assert table.continues("a", 2) and table.continues("b", 4) and not table.continues("a", 1) and not table.continues("c", 1)
    # the next launch: the rows have swapped places, the newest token of each is still on the device — nothing to upload
    again, seeds = table.step([("b", 4, [21, 22, 23, PendingToken(1, 2)]), ("a", 2, None)])
    assert seeds == [] and again == [slots[2], slots[0]] and table.n_seeds == 2
    # cohort steps: one token further each, nothing to upload, and the launch after them continues
    table.step_cohort()
    table.step_cohort()
    assert table.continues("b", 7) and table.continues("a", 5)
    assert table.step([("b", 7, None), ("a", 5, None)]) == (again, [])
    # a first appearance at L = 0 takes a slot and is seeded with nothing
    slots0, seeds0 = table.step([("z", 0, [])])
    assert seeds0 == [] and slots0[0] not in again and table.continues("z", 1)


def test_a_gap_reseeds_with_exactly_the_tokens_so_far():
    table = PenaltyLogTable(4, 16)
    (slot,), _ = table.step([("a", 1, [5])])
    # two eager steps went by: the request comes back at 4 with its tokens on the host, into the slot it had
    slots, seeds = table.step([("a", 4, [5, 6, 7, 8, 99])])
    assert slots == [slot] and seeds == [(slot, [5, 6, 7, 8])] and table.n_seeds == 2
    # a launch that was made twice at the same count (a replayed step): a gap as well
    slots, seeds = table.step([("a", 4, [5, 6, 7, 8])])
    assert seeds == [(slot, [5, 6, 7, 8])] and table.continues("a", 5)


def test_refuses_to_seed_with_a_placeholder_and_changes_nothing():
    table = PenaltyLogTable(4, 16)
    table.step([("a", 1, [5])])
    state = (dict((k, list(v)) for k, v in table.slot_of.items()), list(table.free), table.step_no, table.n_seeds)
    for bad in ([5, 6, PendingToken(3, 0), 8], [5, 6], None):
        with pytest.raises(HydraHipError):
            table.step([("b", 1, [1]), ("a", 4, bad)])
    with pytest.raises(HydraHipError):
        table.step([("a", 17, list(range(17)))])               # past the log's row
    with pytest.raises(HydraHipError):
        table.step([("a", -1, [])])
    assert state == (dict((k, list(v)) for k, v in table.slot_of.items()), list(table.free), table.step_no, table.n_seeds)
    # a placeholder BEYOND [0, L) — the newest token of a continuing row — is nobody's business
    assert table.step([("a", 2, [5, PendingToken(1, 0)])])[1] == []


def test_least_recently_seen_goes_first_never_the_previous_launch():
    table = PenaltyLogTable(4, 16)
    s = {}
    (s["a"], s["b"]), _ = table.step([("a", 1, [1]), ("b", 1, [1])])          # step 1
    (s["c"],), _ = table.step([("c", 1, [1])])                                  # step 2
    (s["d"], _), _ = table.step([("d", 1, [1]), ("b", 2, None)])                # step 3: b seen again
    assert sorted(s.values()) == [0, 1, 2, 3] and not table.free
    # step 4 needs a slot: a (step 1) is the least recently seen; d and b are the previous launch's
    (e,), seeds = table.step([("e", 2, [1, 2])])
    assert e == s["a"] and seeds == [(e, [1, 2])] and "a" not in table.slot_of
    # step 5: c (step 2) goes next — not d or b (step 3), not e (step 4)
    (f,), _ = table.step([("f", 1, [1])])
    assert f == s["c"]
    # step 6: two new ones take d's and b's (step 3), not e's (step 4)
    (g, h), _ = table.step([("g", 1, [1]), ("h", 1, [1])])
    assert {g, h} == {s["d"], s["b"]}
    # step 7: e (step 4) before f (step 5); g and h are the previous launch's
    (i,), _ = table.step([("i", 1, [1])])
    assert i == e
    # a row of THIS launch is never the victim of another row of it, however long ago it was seen, and it needs no seed
    table = PenaltyLogTable(2, 16)
    (a,), _ = table.step([("a", 1, [1])])
    table.step([("b", 1, [1])])
    table.step([("b", 2, None)])
    table.step([("b", 3, None)])
    with pytest.raises(HydraHipError):                          # both slots are this launch's: no room for a third request
        table.step([("c", 1, [1]), ("a", 2, None), ("b", 4, None)])
    slots, seeds = table.step([("b", 4, None), ("a", 2, None)])
    assert slots[1] == a and seeds == []
    # the slots of the launch in flight survive a full turnover: 2 * max_batch slots, max_batch rows
    table = PenaltyLogTable(4, 16)
    previous = set()
    for k in range(6):
        slots, _ = table.step([((k, 0), 1, [1]), ((k, 1), 1, [1])])
        assert len(set(slots)) == 2 and not set(slots) & previous
        previous = set(slots)


# ---- eligibility


class PenalisedDecoder(Decoder):
    def __init__(self, cap=16):
        super().__init__(True)
        self.penalized, self.penalty_log_cap, self.log_table = True, cap, PenaltyLogTable(16, cap)


def penalised(sid, n_out, position, max_tokens=12, penalties=(0.7, 0.5, 1.3), **kw):
    rcb, inst = request(sid, n_out, position, penalty_history=PenaltyHistory(range(n_out)), **kw)
    sp = rcb.sampling_params
    sp.frequency_penalty, sp.presence_penalty, sp.repetition_penalty = penalties
    sp.max_tokens = max_tokens
    return rcb, inst


def with_variant(cap=16):
    fill = executor(True)
    fill.graph_decoder = PenalisedDecoder(cap)
    return fill


def test_a_penalised_request_passes_only_with_the_variant_and_a_fitting_max_tokens():
    batch = [request(0, 1, 17), penalised(1, 3, 20), penalised(2, 2, 9, temperature=0.8, top_k=20, seed=7)]
    assert executor(True)._decode_rows(batch) is None           # GraphedDecoder(sampled=True) alone: as today
    assert executor(False)._decode_rows(batch) is None
    fill = with_variant()
    rows, records, penalties = fill._decode_rows(batch)
    assert [r[5] for r in rows] == [0, 1, 2]
    # a penalised greedy row carries n_out - position at T = 0
    assert records == [None, (0.0, 1.0, 0, 0, 3 - 20), (0.8, 1.0, 20, 7, 2 - 9)]
    assert penalties[0] is None and penalties[1][:3] == (0.7, 0.5, 1.3) and penalties[1][3] is batch[1][0].output_token_ids
    assert penalties[2][3] == [0, 1]
    # max_tokens decides once, for the whole life of the request
    assert fill._decode_rows([penalised(1, 3, 20, max_tokens=16)]) is not None
    assert fill._decode_rows([penalised(1, 3, 20, max_tokens=17)]) is None
    assert with_variant(1024)._decode_rows([penalised(1, 3, 20, max_tokens=1024)]) is not None
    # nothing was taken from the table by asking
    assert fill.graph_decoder.log_table.slot_of == {}


def test_a_row_that_needs_a_seed_waits_for_its_tokens():
    fill = with_variant()
    fill.pending = (4, [])
    rcb, inst = penalised(0, 4, 21, token=PendingToken(4, 0))
    rcb.output_token_ids[3] = inst.token_ids[0]
    # the log does not hold this request and its newest token is still on the device: not this step
    assert fill._decode_rows([(rcb, inst)]) is None
    # it continues (the previous launch was made at 3): the placeholder is the kernel's to know
    fill.graph_decoder.log_table.step([(0, 3, [0, 1, 2])])
    rows, records, penalties = fill._decode_rows([(rcb, inst)])
    assert rows[0][0] == -1 and records == [(0.0, 1.0, 0, 0, 4 - 21)] and penalties[0][3] is rcb.output_token_ids


@pytest.mark.parametrize("odd", [dict(token_constraints=object()), dict(token_mask=object()), dict(logprobs=True),
                                 dict(score_targets=[1])], ids=["constraints", "mask", "logprobs", "score_targets"])
def test_the_other_conditions_are_still_refused(odd):
    fill = with_variant()
    assert fill._decode_rows([request(0, 1, 17), penalised(1, 3, 20, **odd)]) is None
    assert fill._decode_rows([penalised(0, 1, 17), request(1, 3, 20, temperature=0.8, seed=7, **odd)]) is None


def test_without_a_penalised_row_the_return_value_is_todays():
    batch = [request(0, 3, 20, temperature=0.8, top_p=0.9, top_k=20, seed=77), request(1, 1, 17)]
    assert with_variant()._decode_rows(batch) == executor(True)._decode_rows(batch)
    rows, records, penalties = with_variant()._decode_rows(batch)
    assert penalties is None and len(records) == len(rows) == 2
