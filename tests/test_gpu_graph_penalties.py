"""GPU: the penalised variant of GraphedDecoder's captured step (engine/graph_decode.py) on the tiny llama and the
`decoder()` shape of tests/test_gpu_graph_sampling.py.  Three sequences padded to four rows — row 0 penalised and sampled,
row 1 penalised and greedy, row 2 sampled without penalties — decode six steps and two cohort steps.  After every step
the graph's own logits, through hx_sample_rows with the CSR of the row's tokens so far (counted HERE, on the host) and the
explicit offset, give the tokens the graph gave; the rows of the resident token log equal the tokens fetched so far; only
the first step uploads tokens (the one prefill would have produced), every later one finds the newest token where the
kernel put it."""
from collections import Counter

import numpy as np
import pytest
import torch

from hydrainfer_amd._lib import HydraHipError
from hydrainfer_amd.sampling import pack_sample_records, sample_rows
from tests.test_gpu_graph_sampling import BS, B, DEV, FIRST, decoder, step_rows

pytestmark = pytest.mark.gpu

STEPS = 6
# a request's generated-token count is its position + 1 here: the first token (FIRST) is the one prefill produced
SAMPLING = [(0.8, 0.9, 20, (1 << 40) + 1), (0.0, 1.0, 0, 0), (1.3, 1.0, 0, 77)]
RECORDS = [s + (1,) for s in SAMPLING[:2]] + [SAMPLING[2] + (-2,)]
PENALTIES = [(0.4, 0.3, 1.2), (0.7, 0.5, 1.3), None]


def from_logits(logits, hists, offsets):
    """hx_sample_rows over the first three rows of `logits`: the CSR of each penalised row's tokens, explicit offsets"""
    tables = [Counter(h) if p is not None else {} for h, p in zip(hists, PENALTIES)]
    cu = np.cumsum([0] + [len(t) for t in tables]).astype(np.int32)
    ids = torch.tensor([t for c in tables for t in c], dtype=torch.int32, device=DEV)
    counts = torch.tensor([n for c in tables for n in c.values()], dtype=torch.int32, device=DEV)
    pen = torch.tensor([p or (0.0, 0.0, 1.0) for p in PENALTIES], dtype=torch.float32, device=DEV)
    recs = [s + (o % (1 << 64),) for s, o in zip(SAMPLING, offsets)]
    u = torch.empty(3, device=DEV)
    out = sample_rows(logits[:3], torch.from_numpy(pack_sample_records(recs)).to(DEV), ids, counts,
                      torch.from_numpy(cu).to(DEV), pen, u_out=u)
    return out.tolist(), u.cpu().view(torch.int32).tolist()


def check_step(dec, lid, step, hists, key=(B, 256, "penalized")):
    """the tokens of launch `lid` (made at position `step`) against its own logits; appends them to the histories"""
    tokens = dec.fetch(lid)
    u_graph = dec.fetch_draws(lid)
    logits = dec.sample_logits(*key).clone()
    want, u = from_logits(logits, hists, [step + 1, step + 1, step - 2])
    assert tokens == want, f"step {step}: the graph gave {tokens}, its logits give {want}"
    assert u_graph.view(np.int32).tolist() == u
    for h, t in zip(hists, tokens):
        h.append(t)
    torch.cuda.synchronize()
    for r in (0, 1):
        slot = dec.log_table.slot_of[("row", r)][0]
        assert dec.token_log[slot, :step + 2].tolist() == hists[r], f"step {step}: the log of row {r}"
    return tokens


@pytest.mark.parametrize("executor", ["graph", "plan"])
def test_penalised_steps_reproduce_from_their_logits_and_their_log(executor):
    dec, caches = decoder(sampled=True, penalized=True, penalty_log_cap=64, keep_draws=True, executor=executor)
    assert dec.sampled and dec.penalized and dec.token_log.shape == (2 * B, 64)
    hists = [[t] for t in FIRST]
    previous = None
    for step in range(STEPS):
        penalties = [None if p is None else p + (h,) for p, h in zip(PENALTIES, hists)]
        lid = dec.launch(step_rows(caches, step, previous), RECORDS, penalties)
        previous = check_step(dec, lid, step, hists)
    assert list(dec.graphs) == [(B, 256, "penalized")]
    assert dec.log_table.n_seeds == 2, "a continuing row was seeded again"
    # two cohort steps behind the penalised launch: the same variant, nothing uploaded — the table of the rows' penalties
    # and the log's slots stand as they are
    table = list(dec.resident_penalties)
    for step in (STEPS, STEPS + 1):
        pos = np.full(3, step, dtype=np.int32)
        slots = np.array([vc.block_table[step // BS] * BS + step % BS for vc in caches], dtype=np.int32)
        starts = np.array([dec.stager.slot_of[("row", r)][0] * dec.stager.cap for r in range(3)], dtype=np.int32)
        check_step(dec, dec.launch_cohort(3, pos, slots, starts, []), step, hists)
    assert dec.log_table.n_seeds == 2 and dec.resident_penalties == table and list(dec.graphs) == [(B, 256, "penalized")]
    # the untouched slots of the log are as they were made
    used = {dec.log_table.slot_of[("row", r)][0] for r in (0, 1)}
    assert all(not dec.token_log[s].any() for s in range(2 * B) if s not in used)
    # the padding row has no slot and no penalties
    assert dec.penalty_records[3].tolist()[3] == -1 and dec.penalty_records[2].tolist()[3] == -1


def named_rows(caches, step, order, feed):
    """step_rows with the sequences named (sid = their index) and in `order`; feed[q]: the token, or -(row + 1)"""
    return [(feed[q], step, caches[q].block_table[step // BS] * BS + step % BS, step + 1, list(caches[q].block_table), q)
            for q in order]


def test_rows_that_swap_places_keep_their_slots_and_their_tokens():
    """the log's slots belong to the sequences: a launch whose rows come in another order finds each one's tokens where
    they are, seeds nothing, and samples what the launch in the old order samples"""
    runs = []
    for orders in ([(0, 1, 2)] * 4, [(0, 1, 2), (0, 1, 2), (1, 0, 2), (2, 1, 0)]):
        dec, caches = decoder(sampled=True, penalized=True, penalty_log_cap=64)
        hists = [[t] for t in FIRST]
        feed, before = list(FIRST), None
        for step, order in enumerate(orders):
            if step >= 2:                        # from the device: the row the sequence had in the previous launch
                feed = [-(before.index(q) + 1) for q in range(3)]
            lid = dec.launch(named_rows(caches, step, order, feed), [RECORDS[q] for q in order],
                             [None if PENALTIES[q] is None else PENALTIES[q] + (hists[q],) for q in order])
            tokens = dec.fetch(lid)
            for q, t in zip(order, tokens):
                hists[q].append(t)
            feed, before = [hists[q][-1] for q in range(3)], list(order)
        assert dec.log_table.n_seeds == 2
        for q in (0, 1):
            assert dec.token_log[dec.log_table.slot_of[q][0], :len(hists[q])].tolist() == hists[q]
        runs.append(hists)
    assert runs[0] == runs[1]


def test_without_penalties_the_existing_keys_and_a_warmup_of_all_three():
    dec, caches = decoder(sampled=True, penalized=True, penalty_log_cap=64)
    dec.run(step_rows(caches, 0, None))
    dec.run(step_rows(caches, 0, None), [None] * 3, [None] * 3)
    dec.run(step_rows(caches, 0, None), [r[:4] + (0,) for r in RECORDS], None)
    assert list(dec.graphs) == [(B, 256, "greedy"), (B, 256, "sampled")] and dec.log_table.slot_of == {} and not dec.token_log.any()
    dec.warmup([3], kv_max=64)
    assert list(dec.graphs)[-1] == (B, 256, "penalized") and len(dec.graphs) == 3
    assert not dec.token_log.any()
    # a penalised row needs its record, and a decoder without the variant refuses penalties
    with pytest.raises(HydraHipError):
        dec.launch(step_rows(caches, 0, None), [RECORDS[0], None, None], [None, PENALTIES[1] + ([22],), None])
    plain, plain_caches = decoder(sampled=True)
    assert not plain.penalized and not hasattr(plain, "token_log")
    with pytest.raises(HydraHipError):
        plain.launch(step_rows(plain_caches, 0, None), RECORDS, [PENALTIES[0] + ([11],), None, None])
    off, _ = decoder(penalized=True)
    assert not off.sampled and not off.penalized
