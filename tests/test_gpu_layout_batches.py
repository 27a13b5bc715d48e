"""The per-user and per-item kernels of the round-3 layout on the designed inputs of tests/test_cpu_layout_batches.py (which
states what each reaches and asserts it on the CPU):

  * item_sim_tri, both methods, equals the CPU oracle bit for bit and whole (check_sim: info, u_avg, every row), the plan its
    NumPy statement (check_plan), on the whole input, with fractional ratings, and on its first 1, NB - 1, NB, NB + 1 and
    3 NB + 5 users;
  * u_avg and u_norm equal the sequential NumPy statement (with the fractional ratings a reordered sum would not);
  * the sorted profile copy equals the statement of the weight sort, the rater records of every item equal theirs as a
    multiset, W+ its sum -- before the profile copy's flag pass and after it;
  * the item-sharded order (layout3(item_range=...) on two shares, then finish()) gives the one-GPU bytes;
  * two runs give the same bytes;
  * the fp64 path: rows with an item twice in a short, a mid, a long and a very long profile through rec_sim, twice."""
import functools

import numpy as np
import pytest

from test_cpu_layout_batches import (I_MAIN, SMALL_U, fractional, prefix, profiles, sort_statement, user_stats_statement,
                                     wide_rows)
from test_cpu_stage_a_layout import CAP, METHODS, check_plan
from test_gpu_stage_a_layout import check_sim, sorted_sim

pytestmark = pytest.mark.gpu

CH_MIN, SLOT_TARGET = 2048, 768          # two heavy rows (the items of 2 100 and 4 097 raters)
SHARES = ((0, 333), (333, I_MAIN))       # neither share is a whole number of four-item waves


def ratings(name):
    if name.startswith("prefix:"):
        return prefix(int(name.split(":")[1]))
    return dict(main=profiles, fractional=fractional)[name]()


@functools.lru_cache(maxsize=None)
def engine(name):
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device  # raises if libxmap_hip.so is missing: no CPU fallback
    r = ratings(name)
    return device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))


@functools.lru_cache(maxsize=None)
def oracle(name, method):
    from oracle import xmap_oracle as xo
    r = ratings(name)
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
    return xo.item_sim(T, method, CAP, nthreads=8)


@functools.lru_cache(maxsize=None)
def user_stats(name):
    r = ratings(name)
    return user_stats_statement(r.user_ptr, r.rating)


def check_user_stats(stats, name):
    avg, norm = user_stats(name)
    U = len(avg)
    assert np.array_equal(stats[0].cpu().numpy()[:U].view(np.uint64), avg.view(np.uint64))
    assert np.array_equal(stats[1].cpu().numpy()[:U].view(np.uint64), norm.view(np.uint64))


def run_and_check(name, method):
    S = engine(name).item_sim_tri(method, CAP, slot_target=SLOT_TARGET, ch_min=CH_MIN)
    assert S.slot_target == SLOT_TARGET
    check_plan(S, ratings(name), CH_MIN)
    check_sim(S, oracle(name, method))
    check_user_stats((S.u_avg, S.u_norm), name)
    return S


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["main", "fractional"])
def test_result_plan_and_user_statistics(name, method):
    S = run_and_check(name, method)
    assert S.layout.n_heavy == 2 and S.n_kept > 0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("U", SMALL_U)
def test_small_user_counts(U, method):
    run_and_check("prefix:%d" % U, method)


# ------------------------------------------------------------------------------------------- the layout's own arrays
def ub_of(L, nnz):
    return L.ub.cpu().numpy().view(np.int32).reshape(-1, 2)[:nnz]


def rc_of(L, r):
    """the rater records (e0, pos | flag, rating bits, user), those of an item in (user, pos) order"""
    rc = L.rc.cpu().numpy().view(np.int32).reshape(-1, 4)[:r.nnz]
    of_item = np.repeat(np.arange(r.n_items), np.bincount(r.item, minlength=r.n_items))
    return rc[np.lexsort((rc[:, 1] & 0x7fffffff, rc[:, 3], of_item))]


@functools.lru_cache(maxsize=None)
def statements(name):
    """-> (ub without flags, ub with flags, rc with flags in rc_of's order, W+) from the oracle's item averages"""
    r = ratings(name)
    avg = oracle(name, "adjust_cosine").info[:, 0]
    o, pos = sort_statement(r.user_ptr, r.item, r.n_items)
    users = np.repeat(np.arange(r.n_users, dtype=np.int64), np.diff(r.user_ptr))[o]
    it, bits = r.item[o].astype(np.int64), r.rating[o].view(np.int32)
    ge = (r.rating[o].astype(np.float64) >= avg[it]).astype(np.int64) << 31
    ub0 = np.stack([it, bits], 1).astype(np.int32)
    ub1 = np.stack([(it | ge).astype(np.uint32).view(np.int32), bits], 1).astype(np.int32)
    rc = np.stack([r.user_ptr[users].astype(np.int32), (pos | ge).astype(np.uint32).view(np.int32), bits, users.astype(np.int32)], 1)
    rc = rc[np.lexsort((pos, users, it))]
    Wp = np.zeros(r.n_items, np.int64)
    np.add.at(Wp, it, pos)
    return ub0, ub1, rc, Wp


@pytest.mark.parametrize("name", ["main", "fractional", "prefix:%d" % SMALL_U[-1]])
def test_profile_copy_rater_records_and_weights(name):
    r = ratings(name)
    eng = engine(name)
    ub0, ub1, rc, Wp = statements(name)
    stats, L = eng.layout3(SLOT_TARGET, CH_MIN, item_range=(0, r.n_items))
    assert np.array_equal(ub_of(L, r.nnz), ub0)                      # no flag before the flag pass
    assert np.array_equal(rc_of(L, r), rc)                           # the item statistics have set the records' flags
    assert np.array_equal(L.Wp.cpu().numpy()[:r.n_items], Wp)
    check_user_stats(stats, name)
    L.finish()
    assert np.array_equal(ub_of(L, r.nnz), ub1) and not np.array_equal(ub0, ub1)
    assert np.array_equal(rc_of(L, r), rc)
    assert np.array_equal(L.Wp.cpu().numpy()[:r.n_items], Wp)


def test_item_shares_give_the_one_gpu_bytes():
    r = ratings("main")
    eng = engine("main")
    full_stats, full_L = eng.layout3(SLOT_TARGET, CH_MIN)
    info, norms = full_stats[2].clone(), eng.norms.clone()
    want_ub, want_rc = ub_of(full_L, r.nnz).copy(), rc_of(full_L, r)
    assert np.array_equal(info.cpu().numpy(), oracle("main", "adjust_cosine").info)
    for lo, hi in SHARES:
        stats, L = eng.layout3(SLOT_TARGET, CH_MIN, item_range=(lo, hi))
        assert bool((stats[2][lo:hi] == info[lo:hi]).all())                   # this share's statistics ...
        assert bool((eng.norms[lo:hi] == norms[lo:hi]).all())
        assert bool((eng.norms[I_MAIN + lo:I_MAIN + hi] == norms[I_MAIN + lo:I_MAIN + hi]).all())
        stats[2].copy_(info)                                                  # ... and what the all-gather leaves
        eng.norms.copy_(norms)
        L.finish()
        assert np.array_equal(ub_of(L, r.nnz), want_ub) and np.array_equal(rc_of(L, r), want_rc)
        for a, b in ((L.Wp, full_L.Wp), (L.Q, full_L.Q), (L.small, full_L.small), (stats[0], full_stats[0]), (stats[1], full_stats[1])):
            assert bool((a == b).all())


def test_two_runs_give_the_same_bytes():
    r = ratings("fractional")
    eng = engine("fractional")
    for method in METHODS:
        A = eng.item_sim_tri(method, CAP, slot_target=SLOT_TARGET, ch_min=CH_MIN)
        B = eng.item_sim_tri(method, CAP, slot_target=SLOT_TARGET, ch_min=CH_MIN)
        for x, y in zip(sorted_sim(A), sorted_sim(B)):
            assert x.tobytes() == y.tobytes()
        for x, y in ((A.info, B.info), (A.u_avg, B.u_avg), (A.u_norm, B.u_norm), (A.layout.ub, B.layout.ub), (A.layout.Wp, B.layout.Wp)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert rc_of(A.layout, r).tobytes() == rc_of(B.layout, r).tobytes()


def test_fp64_rows_with_repeated_items():
    """the wide instantiations: no user statistics, 16-byte profile entries, ties of equal keys in every sorted class"""
    import types
    from oracle import xmap_oracle as xo
    from test_gpu_recsim import _engine, _oracle_pairs, _pairs
    ptr, item, rating, _ = wide_rows()
    eng = _engine(ptr, item, rating, profiles().item_ids())
    O = xo.rec_sim(ptr, item, rating, I_MAIN, CAP)
    want = _oracle_pairs(O, I_MAIN)
    first = None
    for _ in range(2):
        S = eng.rec_sim(CAP)
        check_plan(S, types.SimpleNamespace(user_ptr=ptr, item=item, n_items=I_MAIN), len(ptr) + 1, dups=True)
        got = _pairs(S, I_MAIN)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[4])
        assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))
        assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))
        assert np.array_equal(S.norm.cpu().numpy(), O.norm)
        first = first or [x.tobytes() for x in got]
        assert first == [x.tobytes() for x in got]
