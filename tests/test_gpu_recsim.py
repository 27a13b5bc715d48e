"""RecommenderSim on the GPU: weighted cosine + leave-one-out local sensitivity over AlterEgo rows,
against the reference's own output (tests/golden/small_downstream.json.gz) and, bit for bit, against the CPU oracle."""
import gzip
import json
import os

import numpy as np
import pytest

from golden_util import rows_to_csr

pytestmark = pytest.mark.gpu
REC_RTOL = 1e-9   # exact sums (inner product, squared norms) vs the reference's python sum() / np.sum roundings
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_downstream.json.gz")


def _engine(ptr, item, rating, iids):
    import torch
    assert torch.cuda.is_available()
    from xmap.engine import device, ids
    attrs = ids.item_attrs(iids)
    R = device.DeviceRatings(ptr, item, rating, np.zeros(len(item), np.int64), len(iids), attrs, "cuda:0", rating64=True)
    return device.Engine(R)


def _pairs(S, n_items):
    rp = S.row_ptr.cpu().numpy()
    rows = np.repeat(np.arange(n_items, dtype=np.int64), np.diff(rp))
    col = S.col.cpu().numpy().astype(np.int64)
    o = np.lexsort((col, rows))
    return rows[o], col[o], S.sim.cpu().numpy()[o], S.ls.cpu().numpy()[o], S.nij.cpu().numpy()[o]


def _oracle_pairs(R, n_items):
    rows = np.repeat(np.arange(n_items, dtype=np.int64), np.diff(R.row_ptr))
    return rows, R.col.astype(np.int64), R.sim, R.ls, R.nij


@pytest.mark.parametrize("key,rows_key", [("cosine_item", None), ("cosine_item_float", "rows")])
def test_rec_sim_golden(key, rows_key):
    from oracle import xmap_oracle as xo
    with gzip.open(GOLD, "rt") as f:
        g = json.load(f)
    rows = g[key][rows_key] if rows_key else g["downstream_input"]["rows"]
    uids, iids, ptr, item, rating = rows_to_csr(rows)
    eng = _engine(ptr, item, rating, iids)
    S = eng.rec_sim(50)
    r, c, sim, ls, nij = _pairs(S, len(iids))
    got = {(iids[a], iids[b]): (s, l) for a, b, s, l in zip(r, c, sim, ls)}
    want = {(a, b): (v[0], v[1]) for (a, b), v in g[key]["sim"]}
    assert set(got) == set(want) and len(got) == len(r)
    assert any(a == b for a, b in want)          # an item held twice by a user pairs with itself
    for kk, (s, l) in want.items():
        gs, gl = got[kk]
        assert np.isnan(l) == np.isnan(gl)
        assert gs == pytest.approx(s, rel=REC_RTOL, abs=1e-15)
        if not np.isnan(l):
            assert gl == pytest.approx(l, rel=REC_RTOL, abs=1e-13)
    O = xo.rec_sim(ptr, item, rating, len(iids), 50)
    orow, ocol, osim, ols, onij = _oracle_pairs(O, len(iids))
    assert np.array_equal(r, orow) and np.array_equal(c, ocol) and np.array_equal(nij, onij)
    assert np.array_equal(sim.view(np.uint64), osim.view(np.uint64))
    assert np.array_equal(ls.view(np.uint64), ols.view(np.uint64))
    assert np.array_equal(S.norm.cpu().numpy(), O.norm)


def _alterego_rows(seed, users, items):
    """AlterEgo rows of a synthetic two-domain case straight from the GPU hot path (private mapping, k = 5)."""
    import torch
    from xmap.engine import device, synth
    r = synth.make_two_domain(seed, users, items, items, overlap=0.4)
    R = device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs(), "cuda:0")
    eng = device.Engine(R)
    S = eng.item_sim("cosine", 50)
    E = eng.extend(S, 5)
    _, _, mp = eng.select(E, True)
    G = eng.alterego(mp)
    u, it, ra = G.user.cpu().numpy(), G.item.cpu().numpy(), G.rating.cpu().numpy()
    o = np.argsort(u, kind="stable")
    return u[o], it[o], ra[o], r


# Rows of at least 2 048 entries (class 4 of the pair tables, here in its local-sensitivity form with 32-bit count halves): the
# census of the two inputs below with the plan's statement (test_cpu_stage_a_layout.plan_statement; duplicates allowed, no heavy
# set: ch_min = users + 2) finds none in the smaller one (600 items, 16 278 rows, the longest 940) and three in the larger one
# (3 000 items, 114 749 rows, the longest 4 590), at both slot targets.  The inputs that run the class at full size -- hubs of
# 2 048 entries and more, 198 000 co-ratings in one slot, every rater of a hub holding it twice, every table class at its
# design fill, the overflow ladder -- are the designed rows of tests/rec_sim_rows.py (test_gpu_rec_sim_rows.py).
WIDE_ROWS = {(3000, 600): 0, (20000, 3000): 3}


@pytest.mark.parametrize("users,items", [(3000, 600), (20000, 3000)])
def test_rec_sim_vs_oracle_on_alterego_rows(users, items):
    import types
    from oracle import xmap_oracle as xo
    from test_cpu_stage_a_layout import check_plan
    u, it, ra, r = _alterego_rows(7, users, items)
    # make sure items held twice by a user (a pass-through and a mapped rating of one target item) are present, also
    # three times, also in long profiles: every 7th user repeats its first (and every 21st also its last) item
    first = np.r_[True, u[1:] != u[:-1]]
    last = np.r_[u[1:] != u[:-1], True]
    ex = np.nonzero(first & (u % 7 == 0))[0]
    ex2 = np.nonzero(last & (u % 21 == 0))[0]
    u = np.concatenate([u, u[ex], u[ex], u[ex2]])
    it = np.concatenate([it, it[ex], it[ex], it[ex2]])
    ra = np.concatenate([ra, ra[ex] * 0.5, ra[ex] * 0.75 + 0.125, ra[ex2] / 3.0]).astype(np.float64)    # fp64, incl. thirds
    o = np.argsort(u, kind="stable")
    u, it, ra = u[o], it[o], ra[o]
    uu, uinv = np.unique(u, return_inverse=True)
    ii, iinv = np.unique(it, return_inverse=True)
    ptr = np.zeros(len(uu) + 1, np.int64)
    np.cumsum(np.bincount(uinv, minlength=len(uu)), out=ptr[1:])
    item, rating = iinv.astype(np.int32), ra.astype(np.float64)
    # duplicates (a pass-through and a mapped rating of the same target item) and non-integer means are present -- among
    # them means no float32 holds (13/3, ...): the stage takes the np.float64 values build_alterEgo produces
    dup = sum(len(set(item[ptr[k]:ptr[k + 1]])) < ptr[k + 1] - ptr[k] for k in range(len(uu)))
    assert dup > 0 and np.any(rating != np.round(rating))
    assert np.any(rating != rating.astype(np.float32).astype(np.float64))
    all_ids = r.item_ids()
    iids = [all_ids[x] for x in ii]
    eng = _engine(ptr, item, rating, iids)
    O = xo.rec_sim(ptr, item, rating, len(ii), 50)
    for slot_target in (640, 24):           # 24: rows cut into many hash partitions
        S = eng.rec_sim(50, slot_target=slot_target)
        P = check_plan(S, types.SimpleNamespace(user_ptr=ptr, item=item, n_items=len(ii)), len(uu) + 2, dups=True)
        assert int((P.cls == 4).sum()) == int((P.n >= 2048).sum()) == WIDE_ROWS[(users, items)] and P.n_heavy == 0
        a, b, sim, ls, nij = _pairs(S, len(ii))
        orow, ocol, osim, ols, onij = _oracle_pairs(O, len(ii))
        assert np.array_equal(a, orow) and np.array_equal(b, ocol) and np.array_equal(nij, onij)
        assert np.array_equal(sim.view(np.uint64), osim.view(np.uint64))
        assert np.array_equal(ls.view(np.uint64), ols.view(np.uint64))
    # symmetry: the reference emits both directions with the same values
    key = a * len(ii) + b
    rev = b * len(ii) + a
    o1, o2 = np.argsort(key), np.argsort(rev)
    assert np.array_equal(key[o1], rev[o2])
    assert np.array_equal(sim[o1].view(np.uint64), sim[o2].view(np.uint64))
    assert np.array_equal(ls[o1].view(np.uint64), ls[o2].view(np.uint64))


def test_recommender_pipeline_api():
    """recommender_calculate_sim_pipeline -> recommender_privacy_pipeline -> recommender_prediction_pipeline driven
    like twodomain_demo.py:107-121; the similarity stage runs on the GPU, the result is the reference's up to the
    rounding of the exact sums."""
    import datetime
    from pyspark import SparkContext, SparkConf
    from xmap.core.recommenderSim import RecommenderSim
    from xmap.core.recommenderPrivacy import RecommenderPrivacy
    from xmap.core.recommenderPrediction import RecommenderPrediction
    from xmap.utils.assist import (recommender_calculate_sim_pipeline, recommender_privacy_pipeline,
                                   recommender_prediction_pipeline)
    from xmap.engine.session import RecSimRDD
    with gzip.open(GOLD, "rt") as f:
        g = json.load(f)
    dt = lambda ts: datetime.datetime.utcfromtimestamp(int(ts))
    sc = SparkContext(conf=SparkConf())
    rows = [(u, i, r, dt(t)) for (u, i, r, t) in g["downstream_input"]["rows"]]
    test = [(u, [(i, r, dt(t)) for (i, r, t) in prof]) for u, prof in g["downstream_input"]["test"]]
    method = "cosine_item"
    sim_tool = RecommenderSim(method, 50)
    user_based, item_based, ubd, ibd, uinfo, iinfo, sim = recommender_calculate_sim_pipeline(sc, sim_tool, sc.parallelize(rows))
    assert isinstance(sim, RecSimRDD)
    got = dict((k, v) for k, v in sim.collect())
    want = {(a, b): v for (a, b), v in g[method]["sim"]}
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k][0] == pytest.approx(v[0], rel=REC_RTOL, abs=1e-15) and got[k][1] == pytest.approx(v[1], rel=REC_RTOL, abs=1e-13)
    # downstream consumers (host-side, as in the reference) accept the handle
    sel = recommender_privacy_pipeline(RecommenderPrivacy(10, 0.6, 0.1), sim, False).collect()
    want_sel = dict((i, lst) for i, lst in g[method]["nonprivate"]["selected"])
    assert set(i for i, _ in sel) == set(want_sel)
    same = sum([n for n, _ in lst] == [n for n, _ in want_sel[i]] for i, lst in sel)
    assert same >= 0.9 * len(sel)          # neighbour lists agree except where equal similarities tie differently
    pred_tool = RecommenderPrediction(0.03, method)
    mae = recommender_prediction_pipeline(pred_tool, sim_tool, sc.parallelize(test), sc.broadcast(dict(sel)), ubd, ibd, uinfo, iinfo)
    ref = [float(x) for x in g[method]["nonprivate"]["mae"].split(";")]
    ours = [float(x) for x in mae.split(";")]
    assert np.allclose(ours, ref, atol=0.02)


def test_rec_select_vs_oracle_and_reference():
    """nonprivate_neighbor_selection on the GPU: bit-exact against the oracle; against the reference's lists wherever
    the 10th and 11th similarity of an item differ (equal similarities keep Spark's arrival order there)."""
    from oracle import xmap_oracle as xo
    with gzip.open(GOLD, "rt") as f:
        g = json.load(f)
    rows = g["downstream_input"]["rows"]
    uids, iids, ptr, item, rating = rows_to_csr(rows)
    eng = _engine(ptr, item, rating, iids)
    S = eng.rec_sim(50)
    O = xo.rec_sim(ptr, item, rating, len(iids), 50)
    for keep in (1, 10, 64):
        cnt, col, sim, ls = [x.cpu().numpy() for x in eng.rec_select(S, keep)]
        ocnt, ocol, osim, ols = xo.rec_select(O, keep)
        assert np.array_equal(cnt, ocnt) and np.array_equal(col, ocol)
        assert np.array_equal(sim.view(np.uint64), osim.view(np.uint64)) and np.array_equal(ls.view(np.uint64), ols.view(np.uint64))
    cnt, col, sim, ls = [x.cpu().numpy() for x in eng.rec_select(S, 10)]
    want = dict((i, lst) for i, lst in g["cosine_item"]["nonprivate"]["selected"])
    checked = 0
    for i, name in enumerate(iids):
        ref = want[name]
        assert cnt[i] == len(ref)
        a = np.sort(np.abs(S.sim.cpu().numpy()[S.row_ptr[i]:S.row_ptr[i + 1]]))[::-1]
        if len(a) > 10 and a[9] == a[10]:
            continue                                    # tie at the cut: order-dependent in the reference
        assert {iids[c] for c in col[i, :cnt[i]]} == {n for n, _ in ref}
        checked += 1
    assert checked > 0.8 * len(iids)
    xo.rec_free(O)


class _B(object):
    def __init__(self, value):
        self.value = value


def _prediction_case(seed, n_users=80, n_items=60, uid_fmt="U%05d", dup_user=None):
    import datetime
    rng = np.random.default_rng(seed)
    uids = [uid_fmt % u for u in range(n_users)]
    iids = ["B%04dT:" % i for i in range(n_items)]
    t0 = datetime.datetime(2012, 6, 1)
    ratings = {}
    for i in iids:
        raters = rng.choice(n_users, size=int(rng.integers(5, 60)), replace=False)
        lst = [(uids[u], float(rng.integers(1, 6)) + float(rng.integers(0, 3)) / 3.0,
                t0 + datetime.timedelta(days=int(rng.integers(0, 6)))) for u in raters]      # few distinct days: ties
        if rng.random() < 0.3:                       # an item held twice by a user (AlterEgo rows can)
            u = uids[int(raters[0])]
            lst.append((u, 2.5, t0 + datetime.timedelta(days=int(rng.integers(0, 6)))))
        if dup_user is not None and i == iids[1]:
            lst += [(uids[dup_user], float(1 + q % 5), t0 + datetime.timedelta(hours=q)) for q in range(70)]
        order = rng.permutation(len(lst))
        ratings[i] = [lst[q] for q in order]
    info = {i: (float(np.mean([r[1] for r in ratings[i]])), 1.0, len(ratings[i])) for i in iids}
    sims = {}
    for i in iids[:n_items - 7]:                     # the last items have no neighbour list
        nb = rng.choice(n_items, size=int(rng.integers(1, 11)), replace=False)
        sims[i] = [(iids[n], float(rng.normal()) * (1.0 if rng.random() < 0.9 else 1e-3)) for n in nb if iids[n] != i]
    test = []
    for u in list(rng.choice(n_users, size=60, replace=False)) + [n_users + 5]:          # + a user without any rating
        uid = uid_fmt % u
        pairs = [(iids[int(q)], float(rng.integers(1, 6))) for q in rng.choice(n_items, size=int(rng.integers(1, 6)), replace=False)]
        test.append((uid, pairs))
    return ratings, sims, info, test


@pytest.mark.parametrize("seed,alpha", [(1, 0.2), (2, 0.05), (3, 1.5)])
def test_prediction_on_the_device_equals_the_python_statement(seed, alpha):
    """RecommenderPrediction.item_based_recommendation: the pairs predicted by xmap_predict are the tuples of the Python
    statement of reference core/recommenderPrediction.py:26-105 (itself pinned to the reference in test_cpu_downstream.py),
    exactly: evidence order, sums, time ranks with ties, decay weights, round-half-up and clamping"""
    from xmap.core.recommenderPrediction import RecommenderPrediction
    from xmap.engine.localrdd import LocalRDD
    ratings, sims, info, test = _prediction_case(seed, dup_user=7 if seed == 3 else None)
    tool = RecommenderPrediction(alpha, "cosine_item")
    rb, sb, ib = _B(ratings), _B(sims), _B(info)
    dev = tool._device_recommendation(LocalRDD(test), rb, sb, ib)
    assert dev is not None
    got = dev.collect()
    exp = [tool.item_based_prediction(line, rb, sb, ib) for line in test]
    assert got == exp
    assert any(p == () for _, ps in exp for p in ps)
    if alpha > 1.0:        # a strong decay changes some rounded predictions: the decayed branch is really exercised
        assert any(p != () and p[2] != p[3] for _, ps in exp for p in ps)
    assert tool.calculate_mae(dev) == tool.calculate_mae(LocalRDD(exp))
    # ids of different lengths: `uid in rater_id` is a real substring test, the Python statement decides
    r2, s2, i2, t2 = _prediction_case(seed, uid_fmt="U%d")
    assert tool._device_recommendation(LocalRDD(t2), _B(r2), _B(s2), _B(i2)) is None
    assert tool.item_based_recommendation(LocalRDD(t2), _B(r2), _B(s2), _B(i2)).collect() == \
        [tool.item_based_prediction(line, _B(r2), _B(s2), _B(i2)) for line in t2]
