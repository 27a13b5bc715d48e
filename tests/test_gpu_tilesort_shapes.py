"""The tile sort (csrc/tilesort.h) on the designed inputs of tests/test_cpu_tilesort_shapes.py, which states what each input
reaches -- several level-A buckets and a large key in both transpositions, a bucket without a key (two equal boundaries for the
bisection of level A), tiles of unrated indices, last chunks that are not full, fragments that start and end inside cache
lines, 16-, 24- and 32-byte records -- and asserts it on the CPU.  Here every input runs through stage A (RecommenderSim for
the AlterEgo-like rows) and the result is compared with the CPU oracle's bit for bit and whole, as check_sim does; with the
round-2 sequence (XMAP_A_V2=1: CSC build, CSC-driven rater records, cursor-atomic mirror), which uses neither the tile sort
nor its loaders; and with a second run (the order inside a key is left open, the canonical bytes are not)."""
import functools

import numpy as np
import pytest

from test_cpu_stage_a_layout import CAP, METHODS, check_plan
from test_cpu_tilesort_shapes import oracle_rows, oracle_sim, ratings_of, rows
from test_gpu_stage_a_layout import check_sim, sorted_sim

pytestmark = pytest.mark.gpu

INPUTS = ("buckets", "gap")


@functools.lru_cache(maxsize=None)
def engine(name):
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device  # raises if libxmap_hip.so is missing: no CPU fallback
    r = ratings_of(name)
    return device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))


@functools.lru_cache(maxsize=None)
def rows_engine():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device, ids
    ptr, item, rating, I = rows()
    attrs = ids.item_attrs(ratings_of("buckets").item_ids())
    return device.Engine(device.DeviceRatings(ptr, item, rating, np.zeros(len(item), np.int64), I, attrs, "cuda:0", rating64=True))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", INPUTS)
def test_stage_a_equals_the_oracle(name, method):
    S = engine(name).item_sim_tri(method, CAP)
    check_plan(S, ratings_of(name), 2048)
    check_sim(S, oracle_sim(name, method)[1])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", INPUTS)
def test_round2_route_gives_the_same_bytes(name, method, monkeypatch):
    eng = engine(name)
    a = sorted_sim(eng.item_sim_tri(method, CAP))
    monkeypatch.setenv("XMAP_A_V2", "1")
    S = eng.item_sim_tri(method, CAP)
    check_sim(S, oracle_sim(name, method)[1])
    assert len(a[0]) > 0
    for x, y in zip(a, sorted_sim(S)):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", INPUTS)
def test_two_runs_give_the_same_bytes(name):
    eng = engine(name)
    a = sorted_sim(eng.item_sim_tri("adjust_cosine", CAP))
    b = sorted_sim(eng.item_sim_tri("adjust_cosine", CAP))
    assert len(a[0]) > 0
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def rec_pairs(S, n_items):
    rp = S.row_ptr.cpu().numpy()
    row = np.repeat(np.arange(n_items, dtype=np.int64), np.diff(rp))
    col = S.col.cpu().numpy().astype(np.int64)
    o = np.lexsort((col, row))
    return row[o], col[o], S.sim.cpu().numpy()[o], S.ls.cpu().numpy()[o], S.nij.cpu().numpy()[o]


def test_wide_and_six_column_records():
    """RecommenderSim over AlterEgo-like rows of the same size: 24-byte sort records through the layout, 32-byte records
    (the local sensitivity travels along, a row paired with itself is not routed) through the mirror; twice"""
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
