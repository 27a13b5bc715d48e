"""Stage A with its two host waits taken on events (work queued behind each read-back) against the stepwise sequence: the same
fine-grained calls with a stream synchronisation after each (device.STEPWISE, the value of XMAP_STAGE_A_STEPWISE when the driver
was loaded; switched here on the loaded module).

Compared byte for byte: row_ptr, item info, user averages and the counts as stored; col, sim, mutu, nij (and the local
sensitivities of rec_sim) in (row, column) order, because the pair kernels append to the half COO through atomic cursors and
leave the order inside a row open (tests/test_gpu_stage_a_layout.py compares two runs the same way).

Not covered: a half-COO shard overflow (the slack retry).  A shard holds 1100 pairs plus the mean share, and a wave appends to
the shard of its global index mod 4096, so an overflow at slack 1 needs several full tables on one shard index among tens of
thousands of units of one table class while the other shards stay near empty; no such input was found that runs in seconds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 50
METHODS = ("adjust_cosine", "cosine")


def _device():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device
    return device


def build(n_users, n_items, hubs=(), per_user=5, seed=0):
    """random profiles of per_user items + hub items rated by the first n users each"""
    from xmap.engine import synth
    rng = np.random.default_rng(seed)
    ptr, items = [0], []
    for u in range(n_users):
        mine = set(rng.choice(n_items, min(per_user, n_items), replace=False).tolist()) if n_items else set()
        mine |= {it for it, n in hubs if u < n}
        items += sorted(mine)
        ptr.append(len(items))
    item = np.array(items, np.int32)
    rating = rng.integers(1, 6, len(item)).astype(np.float32)
    return synth.Ratings(np.array(ptr, np.int64), item, rating, np.zeros(len(item), np.int64), n_items, n_items // 2,
                         np.arange(n_items // 2), np.arange(n_items - n_items // 2))


@functools.lru_cache(maxsize=None)
def ratings(name):
    if name == "no_items":
        return build(3, 0)
    if name == "no_ratings":
        r = build(3, 6)
        from xmap.engine import synth
        return synth.Ratings(np.zeros(4, np.int64), r.item[:0], r.rating[:0], r.time[:0], 6, 3, np.arange(3), np.arange(3))
    if name == "one_rating":
        return build(1, 4, per_user=1)
    if name == "plain":
        return build(300, 400, seed=1)
    if name == "one_hub":
        return build(300, 400, hubs=((0, 100),), seed=2)
    if name == "hubs":
        return build(300, 400, hubs=((0, 100), (7, 150), (200, 90), (399, 70)), seed=3)
    if name == "other":
        return build(170, 90, hubs=((5, 80),), per_user=7, seed=4)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def engine(name):
    device = _device()
    r = ratings(name)
    return device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))


def canon(S, with_ls=False):
    """everything the comparison covers, as bytes"""
    I = S.n_items
    row_ptr = S.row_ptr.cpu().numpy()
    rows = np.repeat(np.arange(I, dtype=np.int64), np.diff(row_ptr[:I + 1]))
    col = S.col.cpu().numpy()
    o = np.lexsort((col, rows))
    out = {"row_ptr": row_ptr.tobytes(), "col": col[o].tobytes(), "sim": S.sim.cpu().numpy()[o].tobytes(),
           "nij": S.nij.cpu().numpy()[o].tobytes(), "info": S.info.cpu().numpy().tobytes(), "n_kept": int(S.n_kept)}
    if with_ls:
        out["ls"] = S.ls.cpu().numpy()[o].tobytes()
        out["n_unordered"] = int(S.n_unordered)
    else:
        out["mutu"] = S.mutu.cpu().numpy()[o].tobytes()
        out["u_avg"] = S.u_avg.cpu().numpy().tobytes()
        out["n_eval"] = int(S.n_eval)
    return out


def both(monkeypatch, run):
    """run() on the overlapped and on the stepwise sequence"""
    device = _device()
    monkeypatch.setattr(device, "STEPWISE", False)
    a = run()
    monkeypatch.setattr(device, "STEPWISE", True)
    b = run()
    monkeypatch.setattr(device, "STEPWISE", False)
    return a, b


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], k


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["no_items", "no_ratings", "one_rating"])
def test_nothing_to_plan(name, method, monkeypatch):
    eng = engine(name)
    a, b = both(monkeypatch, lambda: eng.item_sim(method, CAP))
    assert a.n_kept == 0 and b.n_kept == 0 and a.n_eval == 0
    assert a.layout.n_light == 0 and a.layout.n_heavy_units == 0
    same(canon(a), canon(b))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,ch_min,n_heavy", [("hubs", 1 << 20, 0), ("one_hub", 64, 1), ("hubs", 64, 4)],
                         ids=["no_heavy", "one_heavy", "four_heavy"])
def test_heavy_set_sizes(name, ch_min, n_heavy, method, monkeypatch):
    """no heavy set, one heavy row, several (more than 64 raters at ch_min = 64).  A row computes its pairs with HEAVIER items
    only, so the heaviest row of all has no unit: a heavy set of one plans no heavy unit (the heavy launches are skipped), one
    of four plans units for three rows, and the side stream and k_heavy_merge run."""
    eng = engine(name)
    a, b = both(monkeypatch, lambda: eng.item_sim_tri(method, CAP, ch_min=ch_min))
    assert a.layout.n_heavy == n_heavy and b.layout.n_heavy == n_heavy
    assert (a.layout.n_heavy_units > 0) == (n_heavy > 1) and a.layout.n_light > 0 and a.n_kept > 0
    same(canon(a), canon(b))


class CountingLib(object):
    """the library with the phases of every xmap_sim3_layout call noted"""

    def __init__(self, lib):
        self._lib, self.layout_phases = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name != "xmap_sim3_layout":
            return f

        def layout(*args):
            self.layout_phases.append(int(args[5].value))
            return f(*args)
        return layout


@pytest.mark.parametrize("method", METHODS)
def test_table_overflow_replans_without_a_second_flag_pass(method, monkeypatch):
    """The designed overflowing row of tests/test_cpu_stage_a_layout.py (2 048 partners: two partitions at a slot target of 1024,
    one of which gets more than a table holds): the pair kernels raise the overflow flag, the driver plans again at half the
    slot target.  The result is that of a run that started at the smaller target, on both sequences, and the profile copy's flag
    pass (queued under the FIRST plan's wait) ran once per run."""
    from test_cpu_stage_a_layout import overflowing
    device = _device()
    r, _ = overflowing()
    eng = device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
    counting = CountingLib(device.lib)
    monkeypatch.setattr(device, "lib", counting)
    a, b = both(monkeypatch, lambda: eng.item_sim_tri(method, CAP, slot_target=1024))
    assert a.slot_target < 1024 and a.slot_target == b.slot_target
    assert sum(1 for p in counting.layout_phases if p & 4) == 2          # one flag pass per run, retries included
    direct = eng.item_sim_tri(method, CAP, slot_target=a.slot_target)
    assert direct.slot_target == a.slot_target
    same(canon(a), canon(b))
    same(canon(a), canon(direct))


@pytest.mark.parametrize("method", METHODS)
def test_partitioned_rater_count(method, monkeypatch):
    """XMAP_COUNT_PART_MIN=0: the partitioned count (its fills leave with the layout's) on a small input"""
    eng = engine("one_hub")
    plain = canon(eng.item_sim_tri(method, CAP, ch_min=64))
    monkeypatch.setenv("XMAP_COUNT_PART_MIN", "0")
    a, b = both(monkeypatch, lambda: eng.item_sim_tri(method, CAP, ch_min=64))
    same(canon(a), canon(b))
    same(canon(a), plain)


def test_two_engines_and_repeated_calls(monkeypatch):
    """the pinned block and the events are per device and reused: alternating engines and repeated calls read their own counts"""
    device = _device()
    e1, e2 = engine("one_hub"), engine("other")
    monkeypatch.setattr(device, "STEPWISE", True)
    want1, want2 = canon(e1.item_sim_tri("adjust_cosine", CAP, ch_min=64)), canon(e2.item_sim_tri("adjust_cosine", CAP, ch_min=64))
    monkeypatch.setattr(device, "STEPWISE", False)
    assert want1["n_kept"] != want2["n_kept"]
    for eng, want in ((e1, want1), (e2, want2), (e1, want1), (e1, want1), (e2, want2)):
        S = eng.item_sim_tri("adjust_cosine", CAP, ch_min=64)
        same(canon(S), want)
        assert S.layout.n_heavy == 1


def test_rec_sim_with_a_repeated_item(monkeypatch):
    """RecommenderSim over fp64 profiles, one of which holds an item twice (no flag pass, a sixth column, self pairs)"""
    device = _device()
    r = ratings("plain")
    ptr, item, rating = r.user_ptr.copy(), r.item.copy(), r.rating.astype(np.float64) + 0.25
    # user 0 holds its first item twice (adjacent in the sorted profile)
    item = np.concatenate([item[:1], item])
    rating = np.concatenate([[2.5], rating])
    ptr[1:] += 1
    R = device.DeviceRatings(ptr, item, rating, np.zeros(len(item), np.int64), r.n_items, r.item_attrs(), "cuda:0", rating64=True)
    eng = device.Engine(R)
    a, b = both(monkeypatch, lambda: eng.rec_sim(CAP))
    assert a.n_kept > 0
    rows = np.repeat(np.arange(r.n_items), np.diff(a.row_ptr.cpu().numpy()))
    assert np.any(rows == a.col.cpu().numpy())          # the repeated item pairs with itself
    same(canon(a, True), canon(b, True))


@pytest.mark.parametrize("method", METHODS)
def test_item_range_sets_the_flags_in_finish(method, monkeypatch):
    """layout3(item_range=...) then L.finish(): the item-sharded order, where the flags wait for the complete item info and are
    set in finish(), not under the plan's wait"""
    device = _device()
    eng = engine("hubs")
    want = eng.item_sim_tri(method, CAP, ch_min=64)
    I = ratings("hubs").n_items

    def run():
        full_stats, full_L = eng.layout3(ch_min=64)
        norms = eng.norms.clone()
        stats, L = eng.layout3(ch_min=64, item_range=(0, I // 2))
        before = L.ub.clone()
        stats[2].copy_(full_stats[2])          # what the all-gather of the ranks' shares leaves
        eng.norms.copy_(norms)
        L.finish()
        assert not bool((before == L.ub).all())        # finish() set flags ...
        assert bool((L.ub == full_L.ub).all())         # ... the ones the one-GPU order sets under the plan's wait
        S, n_unordered = eng._pairs_to_csr(method, CAP, stats, L)
        S.u_avg, S.n_eval = stats[0], 2 * n_unordered
        return S
    a, b = both(monkeypatch, run)
    same(canon(a), canon(b))
    same(canon(a), canon(want))
