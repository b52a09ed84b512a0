"""GPU: the sampled variant of GraphedDecoder's captured step (engine/graph_decode.py) on the tiny llama of
tests/engine_util.py.  Three sequences padded to four rows — row 0 sampled with a temperature, top-k and top-p, row 1
greedy, row 2 sampled with a temperature only — decode six steps.  After every step the graph's own logits, through
hx_sample_rows with the row's record and the EXPLICIT offset (base + position), give the tokens the graph gave and the u
it drew with; the sampled rows pass tests/sampling_ref.py; the greedy row is the argmax of its logits and equals what a
decoder without the sampled variant gives for that sequence."""
import numpy as np
import pytest
import torch

from hydrainfer_amd._C.kernel.norm import argmax_rows
from hydrainfer_amd._lib import HydraHipError
from hydrainfer_amd.engine.graph_decode import GraphedDecoder
from hydrainfer_amd.sampling import NO_PENALTIES, pack_sample_records, sample_rows
from tests import sampling_ref as ref
from tests.golden import cases as C
from tests.test_gpu_penalties_engine import _models

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BS = C.TINY_BLOCK_SIZE
STEPS, B = 6, 4
FIRST = [11, 22, 33]
# (temperature, top_p, top_k, seed, offset_base): the base is n_out - position of a request, any constant here
RECORDS = [(0.8, 0.9, 20, (1 << 40) + 1, 5), None, (1.3, 1.0, 0, 77, -2)]


def decoder(**kw):
    from hydrainfer_amd.memory.token_cache_manger import (TokenCacheBlockManager, TokenCacheBlockManagerConfig,
                                                          TokenCacheBlockManagerContext)
    lm, _, shape = _models()
    kv = TokenCacheBlockManager(TokenCacheBlockManagerConfig(
        n_layers=shape.num_hidden_layers, n_tokens=2, n_blocks=24, block_size=BS, n_heads=shape.num_key_value_heads,
        head_size=shape.head_dim, dtype="fp16", device=DEV), TokenCacheBlockManagerContext(rank=0, rank2host={0: "localhost"}))
    dec = GraphedDecoder(lm, kv, max_batch=B, max_blocks_per_seq=4, **kw)
    caches = []
    for _ in FIRST:
        vc = kv.allocate_virtual_cache()
        kv.realloc(vc, 2 * BS)
        caches.append(vc)
    return dec, caches


def step_rows(caches, step, previous):
    """step 0: the first tokens; steps 1-2: the previous tokens as the host read them; later: taken on the device from
    the previous launch's samples (the look-ahead feed)"""
    rows = []
    for r, vc in enumerate(caches):
        tok = FIRST[r] if step == 0 else previous[r] if step < 3 else -(r + 1)
        rows.append((tok, step, vc.block_table[step // BS] * BS + step % BS, step + 1, list(vc.block_table)))
    return rows


def explicit(step):
    return [(0.0, 1.0, 0, 0, step) if r is None else r[:4] + ((r[4] + step) % (1 << 64),) for r in RECORDS]


@pytest.mark.parametrize("executor", ["graph", "plan"])
def test_sampled_steps_reproduce_from_their_logits(executor):
    dec, caches = decoder(sampled=True, keep_draws=True, executor=executor)
    assert dec.sampled and dec.keep_draws
    plain, plain_caches = decoder(executor=executor)
    assert not plain.sampled and not hasattr(plain, "records")
    # a step whose records are all None is the greedy step: today's key, today's tokens
    first = dec.run(step_rows(caches, 0, None), [None] * 3)
    assert first == plain.run(step_rows(plain_caches, 0, None))
    assert dec.run(step_rows(caches, 0, None)) == first
    assert list(dec.graphs) == [(B, 256, "greedy")] and list(plain.graphs) == [(B, 256, "greedy")]
    with pytest.raises(HydraHipError):
        plain.launch(step_rows(plain_caches, 0, None), RECORDS)

    tokens, greedy_tokens, previous, greedy_previous = [], [], None, None
    for step in range(STEPS):
        lid = dec.launch(step_rows(caches, step, previous), RECORDS)
        previous = dec.fetch(lid)
        u_graph = dec.fetch_draws(lid)
        logits = dec.sample_logits(B, 256).clone()
        assert logits.shape == (B, C.TINY_LLAMA["vocab_size"])
        tokens.append(previous)
        greedy_previous = plain.run(step_rows(plain_caches, step, greedy_previous))
        greedy_tokens.append(greedy_previous)

        recs = explicit(step)
        cut, u = (torch.empty(3, device=DEV) for _ in range(2))
        ids = sample_rows(logits[:3], torch.from_numpy(pack_sample_records(recs)).to(DEV), cut_out=cut, u_out=u).tolist()
        assert ids == previous, f"step {step}: the graph gave {previous}, its logits give {ids}"
        assert u_graph.dtype == np.float32 and u_graph.view(np.int32).tolist() == u.cpu().view(torch.int32).tolist()
        host = logits.cpu()
        for r in (0, 2):
            kind = ref.check_row(host[r], [], [], NO_PENALTIES, recs[r], previous[r], float(cut[r]), np.float32(u[r].item()),
                                 f"step {step} row {r}")
            assert kind == "sampled"
        assert previous[1] == int(argmax_rows(logits)[1]) == greedy_previous[1]
    assert (B, 256, "sampled") in dec.graphs and len(dec.graphs) == 2 and list(plain.graphs) == [(B, 256, "greedy")]
    assert [t[1] for t in tokens] == [t[1] for t in greedy_tokens]
    assert any(t[r] != g[r] for t, g in zip(tokens, greedy_tokens) for r in (0, 2)), "no draw left the greedy path"
    # the padding row stayed greedy: its record in the resident table is the greedy one
    assert dec.records[3].tolist() == [0, 0x3F800000, 0, 0, 0, 0, 0, 0]


def test_warmup_captures_both_variants_and_cohort_repeats_the_variant():
    dec, caches = decoder(sampled=True, keep_draws=True)
    dec.warmup([3], kv_max=64)
    assert list(dec.graphs) == [(B, 256, "greedy"), (B, 256, "sampled")]
    # a sampled launch, then the cohort form of the next two steps: the records stay resident, the offset moves with
    # the position — the draws are those of base + position
    lid = dec.launch(step_rows(caches, 0, None), RECORDS)
    dec.fetch(lid)
    for step in (1, 2):
        pos = np.full(3, step, dtype=np.int32)
        slots = np.array([vc.block_table[0] * BS + step for vc in caches], dtype=np.int32)
        starts = np.array([dec.stager.slot_of[("row", r)][0] * dec.stager.cap for r in range(3)], dtype=np.int32)
        lid = dec.launch_cohort(3, pos, slots, starts, [])
        dec.fetch(lid)
        u = dec.fetch_draws(lid)
        for r in (0, 2):
            want = ref.uniform(RECORDS[r][3], (RECORDS[r][4] + step) % (1 << 64))
            assert u[r].view(np.uint32) == want.view(np.uint32), f"cohort step {step} row {r}"
