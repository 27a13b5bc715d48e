"""The large keys of the tile sort (csrc/tilesort.h) on the designed input of tests/test_cpu_tilesort_finish.py, which states
what `hubs` reaches -- several large keys in one level-A bucket, a key exactly at the threshold, odd fragments, chunks of both
kinds of records, mirrored halves behind non-empty own halves -- and asserts it on the CPU.  Level B writes those keys' records
in their final form (CSR columns of the mirror; rater records and W+ of the layout).  Here: stage A against the CPU oracle bit
for bit and whole, with the plan (W+ of every item, the large ones included); a second run on the same engine (cursors and W+
are cleared per call); the round-2 route, which has no tile sort; RecommenderSim over the AlterEgo-like twin (24- and 32-byte
records); and the mirror built in two complementary row shares whose cut lies between two large keys of one bucket
(Engine.tri_mirror with rows=, the entry an item-sharded rank uses)."""
import functools

import numpy as np
import pytest

from test_cpu_stage_a_layout import CAP, METHODS, check_plan
from test_cpu_tilesort_finish import hubs, oracle_rows, oracle_sim, rows
from test_gpu_stage_a_layout import check_sim, sorted_sim
from test_gpu_tilesort_shapes import rec_pairs

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def engine():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device  # raises if libxmap_hip.so is missing: no CPU fallback
    r = hubs()[0]
    return device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))


@functools.lru_cache(maxsize=None)
def rows_engine():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device, ids
    ptr, item, rating, I = rows()
    attrs = ids.item_attrs(hubs()[0].item_ids())
    return device.Engine(device.DeviceRatings(ptr, item, rating, np.zeros(len(item), np.int64), I, attrs, "cuda:0", rating64=True))


@pytest.mark.parametrize("method", METHODS)
def test_stage_a_equals_the_oracle_twice(method):
    """plan (W+ of the large keys is added up by level B, one atomic per workgroup and key) and result; the second run on the
    same engine gives the same canonical bytes"""
    eng = engine()
    first = None
    for _ in range(2):
        S = eng.item_sim_tri(method, CAP)
        check_plan(S, hubs()[0], 2048)
        check_sim(S, oracle_sim(method)[1])
        got = tuple(x.tobytes() for x in sorted_sim(S))
        assert len(got[0]) > 0 and (first is None or got == first)
        first = got


@pytest.mark.parametrize("method", METHODS)
def test_round2_route_gives_the_same_bytes(method, monkeypatch):
    eng = engine()
    a = sorted_sim(eng.item_sim_tri(method, CAP))
    monkeypatch.setenv("XMAP_A_V2", "1")
    S = eng.item_sim_tri(method, CAP)
    check_sim(S, oracle_sim(method)[1])
    assert len(a[0]) > 0
    for x, y in zip(a, sorted_sim(S)):
        assert x.tobytes() == y.tobytes()


def test_wide_and_six_column_records():
    """RecommenderSim over the AlterEgo-like twin: 24-byte sort records through the layout, 32-byte records through the mirror
    (a row paired with itself is not routed; large keys are among such rows); twice"""
    ptr, item, rating, I = rows()
    O = oracle_rows()
    orow = np.repeat(np.arange(I, dtype=np.int64), np.diff(O.row_ptr))
    eng = rows_engine()
    first = None
    for _ in range(2):
        S = eng.rec_sim(CAP)
        row, col, sim, ls, nij = rec_pairs(S, I)
        assert np.array_equal(row, orow) and np.array_equal(col, O.col) and np.array_equal(nij, O.nij)
        assert np.array_equal(sim.view(np.uint64), O.sim.view(np.uint64))
        assert np.array_equal(ls.view(np.uint64), O.ls.view(np.uint64))
        assert np.array_equal(S.norm.cpu().numpy(), O.norm)
        got = (row.tobytes(), col.tobytes(), sim.tobytes(), ls.tobytes(), nij.tobytes())
        assert first is None or got == first
        first = got


@pytest.mark.parametrize("method", METHODS)
def test_two_row_shares_make_the_whole(method):
    """the mirror of one half COO, whole and in the row shares [0, cut) and [cut, I) with the cut between the two heaviest hubs
    (large keys of one level-A bucket): a share routes only its rows' records, its large keys keep their place in their rows"""
    eng = engine()
    r, hub = hubs()
    I, cut = r.n_items, hub[3]
    stats, L = eng.layout3(pairs_hint=dict(has_ls=False, split=True, count_mir=True))
    coo, own, n, _, mir, shards = eng.tri_pairs(method, CAP, stats, L, split=True, marks=False, count_mir=True)
    whole = sorted_sim(eng.tri_mirror(coo, own, mir, stats[2], n, shards, counted=True))
    lo = sorted_sim(eng.tri_mirror(coo, own, mir, stats[2], n, shards, rows=(0, cut), counted=True))
    hi = sorted_sim(eng.tri_mirror(coo, own, mir, stats[2], n, shards, rows=(cut, I), counted=True))
    So = oracle_sim(method)[1]
    assert np.array_equal(whole[1], So.col) and np.array_equal(whole[2].view(np.uint64), So.sim.view(np.uint64))
    assert lo[0].max() == cut - 1 and hi[0].min() == cut and len(lo[0]) + len(hi[0]) == len(whole[0])
    for w, a, b in zip(whole, lo, hi):
        assert np.concatenate([a, b]).tobytes() == w.tobytes()
