"""Stage A on the designed layouts of tests/test_cpu_stage_a_layout.py (which states what each family reaches and asserts it on
the CPU): for every family and every (ch_min, slot_target) of RUNS, both methods,

  * the plan the device made -- CH, the heavy set and its dense ids, W+, Q, C and the table class of every row, the unit
    counts per class -- equals the NumPy statement of the plan, element for element (check_plan), and
  * the result equals the CPU oracle's, bit for bit and whole: rows, columns, sim, mutu, nij, item info, user averages, the
    counts of evaluated pairs and contributions (check_sim).

wide_counts carries the one count the other inputs cannot reach: 66 000 co-raters in one slot of a class-4 table, beyond a
16-bit half of the count word.  The hub families also run through the round-2 sequence (XMAP_A_V2=1), with cosine forced onto the double-double kernels
(XMAP_EXACT_COSINE=1: the slot lock of the shared tables in cosine mode) and with non-integer ratings; further: two runs
give the same bytes, a table overflow is answered by a halved slot target, and no input can make a heavy set of more than
1024 rows."""
import functools

import numpy as np
import pytest

from test_cpu_stage_a_layout import (CAP, METHODS, RUNS, RUN_IDS, FULL_HEAVY_CH_MIN, FULL_HEAVY_VARIANTS, HMAX, check_plan, family,
                                     oracle_sim, oracle_rows, overflowing, plan_of)

pytestmark = pytest.mark.gpu

WIDE_RUNS = [run[:3] for run in RUNS if run[0].startswith("wide")]
WIDE_IDS = ["%s-%d-%d" % run for run in WIDE_RUNS]


@functools.lru_cache(maxsize=None)
def engine(name):
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device  # raises if libxmap_hip.so is missing: no CPU fallback
    r = family(name)
    return device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))


def sorted_sim(S):
    row_ptr = S.row_ptr.cpu().numpy()
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))
    col = S.col.cpu().numpy().astype(np.int64)
    o = np.lexsort((col, rows))
    return rows[o], col[o], S.sim.cpu().numpy()[o], S.mutu.cpu().numpy()[o], S.nij.cpu().numpy()[o]


def check_sim(S, So):
    """a stage-A result against the oracle's, whole and bit for bit"""
    assert S.n_eval == So.n_eval and S.n_contrib == So.n_contrib
    rows, cols, sim, mutu, nij = sorted_sim(S)
    assert np.array_equal(rows, oracle_rows(So)) and np.array_equal(cols, So.col)
    assert np.array_equal(mutu, So.mutu) and np.array_equal(nij, So.nij)
    assert np.array_equal(S.info.cpu().numpy(), So.info)
    assert np.array_equal(S.u_avg.cpu().numpy()[:len(So.uavg)], So.uavg)
    assert np.array_equal(sim.view(np.uint64), So.sim.view(np.uint64))


def run_and_check(name, ch_min, slot_target, method):
    S = engine(name).item_sim_tri(method, CAP, slot_target=slot_target, ch_min=ch_min)
    assert S.slot_target == slot_target              # (no table overflowed)
    P = check_plan(S, family(name), ch_min)
    check_sim(S, oracle_sim(name, method)[1])
    return S, P


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,ch_min,slot_target,want", RUNS, ids=RUN_IDS)
def test_plan_and_result(name, ch_min, slot_target, want, method):
    S, P = run_and_check(name, ch_min, slot_target, method)
    assert int((P.cls == 4).sum()) == want["wide"] and P.n_heavy == want["n_heavy"] and P.CH == want["CH"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,ch_min,slot_target", WIDE_RUNS, ids=WIDE_IDS)
def test_round2_sequence(name, ch_min, slot_target, method, monkeypatch):
    """CSC build, CSC-driven rater records and the cursor-atomic mirror around the same pair kernels"""
    monkeypatch.setenv("XMAP_A_V2", "1")
    run_and_check(name, ch_min, slot_target, method)


@pytest.mark.parametrize("name,ch_min,slot_target", WIDE_RUNS, ids=WIDE_IDS)
def test_cosine_on_the_exact_route(name, ch_min, slot_target, monkeypatch):
    """cosine through the double-double kernels: the 16 waves of a class-4 table take the slot lock in cosine mode as well"""
    monkeypatch.setenv("XMAP_EXACT_COSINE", "1")
    run_and_check(name, ch_min, slot_target, "cosine")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,ch_min,slot_target", WIDE_RUNS, ids=WIDE_IDS)
def test_fractional_ratings(name, ch_min, slot_target, method):
    """non-integer ratings: cosine's fp64 sums would round, so the host's predicate selects the exact route on its own; the plan
    does not depend on the ratings"""
    S, P = run_and_check(name + "+fractional", ch_min, slot_target, method)
    assert np.array_equal(P.cls, plan_of(name, ch_min, slot_target).cls)
    r = family(name + "+fractional")
    assert np.any(r.rating != np.round(r.rating))


def test_two_runs_give_the_same_bytes():
    """six class-4 rows, no heavy set: 1 024 lanes add into at most seven slots in an order that differs from run to run"""
    eng = engine("wide_few")
    for method in METHODS:
        a = sorted_sim(eng.item_sim_tri(method, CAP, slot_target=768, ch_min=8192))
        b = sorted_sim(eng.item_sim_tri(method, CAP, slot_target=768, ch_min=8192))
        assert len(a[0]) > 0
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("method", METHODS)
def test_table_overflow_halves_the_slot_target(method, monkeypatch):
    """A partition that meets more partners than its table has slots raises the overflow flag (k_pair_tri returns without
    writing), and the engine plans again with half the slot target.  The plan admits slot targets up to 1024 (one table), so
    the input has a row of exactly 2 048 partners (test_cpu_stage_a_layout.overflowing): two partitions at 1024, one of which
    gets more than half.  Both sequences; the result is the oracle's and that of a direct run at the final slot target."""
    r, lone = overflowing()
    So = oracle_sim("overflowing", method)[1]
    eng = engine("overflowing")
    for v2 in ("0", "1"):
        monkeypatch.setenv("XMAP_A_V2", v2)
        S = eng.item_sim_tri(method, CAP, slot_target=1024)
        assert S.slot_target in (512, 256, 128, 64, 32)
        P = check_plan(S, r, 2048)
        assert P.Q[lone] == 2048 // S.slot_target
        check_sim(S, So)
        D = eng.item_sim_tri(method, CAP, slot_target=S.slot_target)
        assert D.slot_target == S.slot_target
        check_plan(D, r, 2048)
        for x, y in zip(sorted_sim(S), sorted_sim(D)):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("variant", FULL_HEAVY_VARIANTS)
def test_heavy_set_never_exceeds_its_table(variant, monkeypatch):
    """1 024 or 1 025 items above ch_min: the threshold search keeps the heavy set within the 1 024 dense ids, so neither
    sequence refuses ("heavy set larger than 1024") and neither writes a heavy id beyond the list"""
    name = "full_heavy:" + variant
    for v2 in ("0", "1"):
        monkeypatch.setenv("XMAP_A_V2", v2)
        S, P = run_and_check(name, FULL_HEAVY_CH_MIN, 768, "adjust_cosine")        # (an XmapError would fail the test here)
        assert S.layout.n_heavy == P.n_heavy <= HMAX
        assert int(S.layout.hid.max().item()) == P.n_heavy - 1
