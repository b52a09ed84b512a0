"""No GPU: the host side of sampled decoding from the captured step — pack_resident_records word for word, and which
batches BatchFillExecutor._decode_rows sends to the decoder with which records (stand-ins for the decoder and the
requests: nothing here touches a device)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest

from hydrainfer_amd.engine.executor import BatchFillExecutor, PendingToken
from hydrainfer_amd.sampling import pack_resident_records, pack_sample_records

BS = 16


def f32(x):
    return int(np.float32(x).view(np.uint32))


def test_pack_resident_records_word_exact():
    seed = (1 << 62) + (5 << 32) + 9
    recs = [None, (0.8, 0.9, 20, seed, -7), (1.3, 1.0, 0, 3, (1 << 32) - 3), (0.5, 0.25, 7, (1 << 63) - 1, -(1 << 40))]
    got = pack_resident_records(recs)
    assert got.dtype == np.int32 and got.shape == (4, 8)
    want = [[f32(0.0), f32(1.0), 0, 0, 0, 0, 0, 0],
            [f32(0.8), f32(0.9), 20, 0, 9, (1 << 30) + 5, 0xFFFFFFF9, 0xFFFFFFFF],
            [f32(1.3), f32(1.0), 0, 0, 3, 0, 0xFFFFFFFD, 0],
            [f32(0.5), f32(0.25), 7, 0, 0xFFFFFFFF, 0x7FFFFFFF, 0, 0xFFFFFF00]]
    assert got.view(np.uint32).tolist() == want
    # a base >= 0 packs as pack_sample_records packs that offset; `out` is filled in place, stale words included
    assert np.array_equal(pack_resident_records([recs[2]]), pack_sample_records([recs[2]]))
    out = np.full((6, 8), -1, dtype=np.int32)
    assert pack_resident_records(recs, out[1:5]) is not None and np.array_equal(out[1:5], got)
    assert (out[0] == -1).all() and (out[5] == -1).all()


class Decoder:
    def __init__(self, sampled):
        self.sampled = sampled

    def fits(self, n, max_blocks):
        return n <= 8 and max_blocks <= 4


def executor(sampled):
    lm = NS(language_model=NS(shape=NS()))
    return BatchFillExecutor(lm, NS(block_size=BS), None, None, None, graph_decoder=Decoder(sampled))


def request(sid, n_out, position, temperature=0.0, top_p=1.0, top_k=0, seed=None, token=5, **odd):
    """a request in decode: n_out tokens stand in output_token_ids, its next input sits at `position`"""
    sp = NS(logprobs=odd.get("logprobs", False), temperature=temperature, top_p=top_p, top_k=top_k, seed=seed)
    rcb = NS(sid=sid, sampling_params=sp, penalty_history=odd.get("penalty_history"),
             token_constraints=odd.get("token_constraints"), token_mask=odd.get("token_mask"),
             output_token_ids=list(range(n_out)), virtual_kv_cache=NS(block_table=[3 + sid, 40 + sid]))
    inst = NS(token_ids=[token], sample=True, score_targets=odd.get("score_targets"), cache_ids=[position],
              position_ids=[position])
    return rcb, inst


def test_decode_rows_gives_records_under_the_switch():
    fill = executor(True)
    batch = [request(0, 3, 20, temperature=0.8, top_p=0.9, top_k=20, seed=77),
             request(1, 1, 17),
             request(2, 6, 9, temperature=1.3, seed=(1 << 40) + 1)]
    rows, records, penalties = fill._decode_rows(batch)
    assert penalties is None
    assert records == [(0.8, 0.9, 20, 77, 3 - 20), None, (1.3, 1.0, 0, (1 << 40) + 1, 6 - 9)]
    assert [r[:4] for r in rows] == [(5, 20, 40 * BS + 4, 21), (5, 17, 41 * BS + 1, 18), (5, 9, 5 * BS + 9, 10)]
    assert [r[5] for r in rows] == [0, 1, 2]
    # the rows are what the decoder gets with the switch off, for a batch the old test lets through
    greedy = [request(1, 1, 17), request(2, 6, 9)]
    assert (fill._decode_rows(greedy)[0], None, None) == executor(False)._decode_rows(greedy)
    assert fill._decode_rows(greedy)[1] == [None, None] and fill._decode_rows(greedy)[2] is None
    # look-ahead: the input still on the device, and the placeholder counts as a generated token
    fill.pending = (4, [])
    rcb, inst = request(0, 4, 21, temperature=0.8, seed=77, token=PendingToken(4, 2))
    rows, records, penalties = fill._decode_rows([(rcb, inst)])
    assert penalties is None
    assert rows[0][0] == -3 and records == [(0.8, 1.0, 0, 77, 4 - 21)]          # the same base one step later
    assert fill._decode_rows([request(0, 4, 21, temperature=0.8, seed=77, token=PendingToken(3, 2))]) is None


@pytest.mark.parametrize("odd", [dict(penalty_history=object()), dict(token_constraints=object()), dict(token_mask=object()),
                                 dict(logprobs=True), dict(score_targets=[1])],
                         ids=["penalties", "constraints", "mask", "logprobs", "score_targets"])
def test_decode_rows_keeps_the_other_conditions(odd):
    fill = executor(True)
    assert fill._decode_rows([request(0, 1, 17), request(1, 3, 20, temperature=0.8, seed=7, **odd)]) is None
    assert fill._decode_rows([request(0, 1, 17), request(1, 3, 20, temperature=0.8, seed=7)]) is not None


def test_decode_rows_with_the_switch_off():
    fill = executor(False)
    assert fill._decode_rows([request(0, 1, 17), request(1, 3, 20, temperature=0.8, seed=7)]) is None
    rows, records, penalties = fill._decode_rows([request(0, 1, 17), request(1, 3, 20)])
    assert records is None and penalties is None
    assert isinstance(rows, list) and len(rows) == 2 and len(rows[0]) == 6
    # a decoder that has no such attribute at all (a stand-in from before the switch): as off
    fill.graph_decoder = NS(fits=lambda n, b: True)
    assert fill._decode_rows([request(1, 3, 20, temperature=0.8, seed=7)]) is None
    rows, records, penalties = fill._decode_rows([request(1, 3, 20)])
    assert len(rows) == 1 and records is None and penalties is None
