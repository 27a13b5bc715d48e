"""The device-resident recommender tail: AlterEgo rows -> user-major profiles -> RecommenderSim -> neighbour selection ->
prediction with temporal decay -> MAE, without a host conversion (csrc/stage_e_rows.hip, the xmap_ctx_rec_* / xmap_ctx_predict
calls of csrc/api.hip and csrc/api_tail.hip, Engine.alterego_profiles / predict / mae, session.recommend).

The coarse side is driven as a foreign host drives it (NumPy through ctypes, no torch).  RecommenderSim and the selection
are compared bit for bit with the CPU oracle; the prediction with the Python statement of the reference
(RecommenderPrediction.item_based_prediction, pinned to the reference in test_cpu_downstream.py) fed with dictionaries made
from the DOWNLOADED arrays, tuple for tuple; the MAE with calculate_mae."""
import ctypes as C
import datetime
import gzip
import json
import os
import warnings

import numpy as np
import pytest

from golden_util import CAP, Golden
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_coarse_oracle import CODE, stage_c, upload
from test_gpu_recsim import _B, _prediction_case

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_downstream.json.gz")
RAISES = (ZeroDivisionError, ValueError, OverflowError)       # what the Python statement raises where the device says status 2


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


class _GoldRatings(object):
    """a golden case with the fields of synth.Ratings that the coarse driver reads"""

    def __init__(self, case):
        g = Golden(case)
        self.g, self.user_ptr, self.item, self.rating, self.time, self.n_items = g, g.ptr, g.item, g.rating, g.time, g.I

    def item_attrs(self):
        return self.g.attrs


def _few_times(r, days=5):
    """the same ratings with a handful of distinct times: ties in the time order of every longer evidence list"""
    from xmap.engine import synth
    t = synth.T0 + (np.asarray(r.time, np.int64) % days) * 86400
    return synth.Ratings(r.user_ptr, r.item, r.rating, t, r.n_items, r.n_src_items, r.src_numbers, r.tgt_numbers)


# ------------------------------------------------------------------------------------------------- the coarse driver
def generate(ctx, r, method="cosine", k=5):
    """upload -> stage A -> stage B -> stage C (private mapping); the AlterEgo rows as xmap_ctx_gen_download gives them"""
    upload(ctx, r)
    ctx.call("xmap_ctx_item_sim", CODE[method], CAP, None, None)
    ctx.call("xmap_ctx_extend", k, None, None)
    return stage_c(ctx, r.n_items, True, None)


def rec_sim(ctx, I, U, n_rows, cap=CAP):
    n_pairs = C.c_int64(-1)
    ctx.call("xmap_ctx_rec_sim", cap, C.byref(n_pairs))
    n = n_pairs.value
    ptr, pit, pra, pti = np.zeros(U + 1, np.int64), np.zeros(n_rows, np.int32), np.zeros(n_rows), np.zeros(n_rows, np.int64)
    ctx.call("xmap_ctx_rec_profiles_download", _p(ptr, C.c_int64), _p(pit, C.c_int32), _p(pra, C.c_double), _p(pti, C.c_int64))
    rp, col, sim, ls = np.zeros(I + 1, np.int64), np.zeros(n, np.int32), np.zeros(n), np.zeros(n)
    nij, avg, norm = np.zeros(n, np.int32), np.zeros(I), np.zeros(I)
    ctx.call("xmap_ctx_rec_download", _p(rp, C.c_int64), _p(col, C.c_int32), _p(sim, C.c_double), _p(ls, C.c_double),
             _p(nij, C.c_int32), _p(avg, C.c_double), _p(norm, C.c_double))
    assert rp[-1] == n
    return dict(ptr=ptr, item=pit, rating=pra, time=pti, row_ptr=rp, col=col, sim=sim, ls=ls, nij=nij, avg=avg, norm=norm)


def select(ctx, I, keep):
    ctx.call("xmap_ctx_rec_select", keep)
    return neighbors(ctx, I, keep)


def neighbors(ctx, I, keep):
    cnt, col, sim, ls = np.zeros(I, np.int32), np.zeros((I, keep), np.int32), np.zeros((I, keep)), np.zeros((I, keep))
    ctx.call("xmap_ctx_rec_neighbors_download", _p(cnt, C.c_int32), _p(col, C.c_int32), _p(sim, C.c_double), _p(ls, C.c_double))
    return cnt, col, sim, ls


def wtab(alpha, n_w):
    return np.asarray([np.exp(- alpha * d) for d in range(n_w)], np.float64)      # scalar calls, like the reference's


def predict(ctx, tu, ti, real, alpha, n_w=66):
    T = len(tu)
    tu, ti = np.ascontiguousarray(tu, np.int32), np.ascontiguousarray(ti, np.int32)
    real = None if real is None else np.ascontiguousarray(real, np.float64)
    w = wtab(alpha, n_w)
    plain, decay, status, mae, max_now = np.zeros(T), np.zeros(T), np.full(T, -1, np.int32), np.zeros(3), C.c_int32(-1)
    ctx.call("xmap_ctx_predict", T, _p(tu, C.c_int32), _p(ti, C.c_int32), _p(real, C.c_double), _p(w, C.c_double), n_w,
             _p(plain, C.c_double), _p(decay, C.c_double), _p(status, C.c_int32), _p(mae if real is not None else None, C.c_double),
             C.byref(max_now))
    return plain, decay, status, mae, max_now.value


# ------------------------------------------------------------------------------------ the Python statement's inputs
UID, IID = "U%08d", "B%08dT:"          # ids of one length: `uid in rater_id` is an equality test


def group_by_user(rows, U):
    """NumPy statement of the profiles: a stable group-by-user of the stage-C rows"""
    o = np.argsort(rows["user"], kind="stable")
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(np.bincount(rows["user"], minlength=U), out=ptr[1:])
    return ptr, rows["item"][o], rows["rating"][o], rows["time"][o]


def dicts_from_arrays(rows, I, avg, norm, nb):
    """the three dictionaries of _predict_pair from downloaded arrays: rating lists per item in stage-C row order, the
    selected neighbours, (item average, norm, count)"""
    ratings = {}
    for u, i, r, t in zip(rows["user"].tolist(), rows["item"].tolist(), rows["rating"].tolist(), rows["time"].tolist()):
        ratings.setdefault(IID % i, []).append((UID % u, r, t))
    cnt, col, sim = nb[:3]
    sims = {IID % i: [(IID % col[i, t], float(sim[i, t])) for t in range(cnt[i])] for i in range(I) if cnt[i] > 0}
    n = np.bincount(rows["item"], minlength=I)
    info = {IID % i: (float(avg[i]), float(norm[i]), int(n[i])) for i in range(I) if n[i] > 0}
    return ratings, sims, info


def statement(alpha, tu, ti, real, ratings, sims, info):
    """per test pair the Python statement's tuple, () for an item without a list, or None where it raises"""
    from xmap.core.recommenderPrediction import RecommenderPrediction
    tool = RecommenderPrediction(alpha, "cosine_item")
    rb, sb, ib = _B(ratings), _B(sims), _B(info)
    out = []
    for u, i, r in zip(tu, ti, real):
        try:
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                out.append(tool.item_based_prediction((UID % u, [(IID % i, r)]), rb, sb, ib)[1][0])
        except RAISES:
            out.append(None)
    return out


def device_tuples(ti, real, plain, decay, status):
    return [(IID % i, r, float(p), float(d)) if s == 0 else (() if s == 1 else None)
            for i, r, p, d, s in zip(ti, real, plain.tolist(), decay.tolist(), status.tolist())]


def make_pairs(rng, rows, r, n):
    """test pairs over the target items with rows, + an item without a neighbour list (a source item: it has no AlterEgo
    row) and a user without rows (index -1); integer real ratings"""
    U = len(r.user_ptr) - 1
    items = np.unique(rows["item"])
    tu = rng.integers(0, U, n).astype(np.int32)
    ti = rng.choice(items, n).astype(np.int32)
    ti[::17] = 0                                    # a source item
    tu[5::23] = -1                                  # a user the train set does not know
    real = rng.integers(1, 6, n).astype(np.float64).tolist()
    return tu.tolist(), ti.tolist(), real


def python_mae(tuples):
    from xmap.core.recommenderPrediction import RecommenderPrediction
    from xmap.engine.localrdd import LocalRDD
    return [float(x) for x in RecommenderPrediction(0.1, "cosine_item").calculate_mae(LocalRDD([("u", tuples)])).split(";")]


# ------------------------------------------------------------------------------------------------------ 1. profiles
def _check_profiles(rows, T, U):
    ptr, it, ra, tm = group_by_user(rows, U)
    assert np.array_equal(T["ptr"], ptr) and np.array_equal(T["item"], it) and np.array_equal(T["time"], tm)
    assert np.array_equal(T["rating"].view(np.uint64), ra.view(np.uint64))


@pytest.mark.parametrize("case", ["kat7", "small", "multilabel"])
def test_profiles_of_golden_cases(case):
    r = _GoldRatings(case)
    U = len(r.user_ptr) - 1
    ctx = Ctx()
    try:
        rows = generate(ctx, r, "cosine", r.g.ks("cosine")[0])
        T = rec_sim(ctx, r.n_items, U, len(rows["user"]))
        _check_profiles(rows, T, U)
    finally:
        ctx.close()


# --------------------------------------------------------------- 1-3, 6. synthetic two-domain cases, every step
def _oracle_rec(T, I):
    from oracle import xmap_oracle as xo
    return xo, xo.rec_sim(T["ptr"], T["item"], T["rating"], I, CAP)


def _check_rec_sim(T, O, I):
    rows = np.repeat(np.arange(I, dtype=np.int64), np.diff(T["row_ptr"]))
    o = np.lexsort((T["col"], rows))
    orow = np.repeat(np.arange(I, dtype=np.int64), np.diff(O.row_ptr))
    assert np.array_equal(T["row_ptr"], O.row_ptr)
    assert np.array_equal(rows[o], orow) and np.array_equal(T["col"][o], O.col) and np.array_equal(T["nij"][o], O.nij)
    assert np.array_equal(T["sim"][o].view(np.uint64), O.sim.view(np.uint64))
    assert np.array_equal(T["ls"][o].view(np.uint64), O.ls.view(np.uint64))
    assert np.array_equal(T["norm"], O.norm)


def _check_item_avg(T, I):
    """the average the prediction reads is the exact sum of the item's AlterEgo ratings, rounded once, over their count"""
    import math
    n = np.bincount(T["item"], minlength=I)
    for i in np.nonzero(n)[0][:400]:
        assert T["avg"][i] == math.fsum(T["rating"][T["item"] == i].tolist()) / n[i]
    assert not T["avg"][n == 0].any()


@pytest.mark.parametrize("seed,users,src,tgt,overlap", [(7, 3000, 600, 80, 0.5), (11, 2000, 1000, 100, 0.4)])
def test_tail_through_the_coarse_abi(seed, users, src, tgt, overlap):
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(seed, users, src, tgt, overlap=overlap))
    I, U = r.n_items, users
    rng = np.random.default_rng(seed)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        n_rows = len(rows["user"])
        T = rec_sim(ctx, I, U, n_rows)
        _check_profiles(rows, T, U)
        # users holding an item twice: a pass-through and a mapped rating of one target item.  (A mean that float32 does not
        # hold needs a user with several ratings of ONE source item; stage C's rows cannot be edited through this interface:
        # test_edited_alterego_rows_through_the_engine has that case.)
        key = T["item"].astype(np.int64) + I * np.repeat(np.arange(U, dtype=np.int64), np.diff(T["ptr"]))
        assert len(np.unique(key)) < n_rows
        xo, O = _oracle_rec(T, I)
        _check_rec_sim(T, O, I)
        assert np.any(np.repeat(np.arange(I), np.diff(T["row_ptr"])) == T["col"])        # an item paired with itself
        _check_item_avg(T, I)
        for keep in (1, 10, 64):
            cnt, col, sim, ls = select(ctx, I, keep)
            ocnt, ocol, osim, ols = xo.rec_select(O, keep)
            assert np.array_equal(cnt, ocnt) and np.array_equal(col, ocol)
            assert np.array_equal(sim.view(np.uint64), osim.view(np.uint64)) and np.array_equal(ls.view(np.uint64), ols.view(np.uint64))
        xo.rec_free(O)
        tu, ti, real = make_pairs(rng, rows, r, 1500)
        differs = 0
        for keep, alphas in ((10, (0.05, 0.2, 1.5)), (64, (1.5,))):
            nb = select(ctx, I, keep)
            ratings, sims, info = dicts_from_arrays(rows, I, T["avg"], T["norm"], nb)
            for alpha in alphas:
                want = statement(alpha, tu, ti, real, ratings, sims, info)
                assert None not in want                         # the Python statement raises for none of the inputs
                plain, decay, status, mae, max_now = predict(ctx, tu, ti, real, alpha)
                got = device_tuples(ti, real, plain, decay, status)
                assert got == want
                assert int((status == 2).sum()) == 0 and max_now <= 66
                assert () in want
                if alpha > 1.0:
                    differs += sum(1 for t in want if t != () and t[2] != t[3])
                # MAE: the device's sums against calculate_mae on the same records (integer ratings: exact)
                p_plain, p_decay = python_mae(got)
                assert mae[0] == sum(1 for t in got if t != ())
                assert mae[1] / mae[0] == p_plain and mae[2] / mae[0] == p_decay
        assert differs > 0                                      # a strong decay changes some rounded predictions
        # a decay table that is too short: status 2 for the pairs that need more, and the length that serves them all
        plain2, decay2, status2, _, need = predict(ctx, tu, ti, None, 1.5, n_w=3)
        assert need > 3 and int((status2 == 2).sum()) > 0
        plain3, decay3, status3, _, need3 = predict(ctx, tu, ti, None, 1.5, n_w=need)
        assert need3 == need and int((status3 == 2).sum()) == 0
        assert device_tuples(ti, real, plain3, decay3, status3) == want
        ok = status2 == 0
        assert np.array_equal(plain2[ok], plain3[ok]) and np.array_equal(decay2[ok], decay3[ok])
    finally:
        ctx.close()


def test_edited_alterego_rows_through_the_engine():
    """the construction of test_gpu_recsim.test_rec_sim_vs_oracle_on_alterego_rows -- items held twice and three times, also
    in long profiles, and ratings no float32 holds (thirds) -- as a second row segment behind the rows of the hot path:
    Engine.alterego_profiles groups the two segments by user on the device, Engine(profiles).rec_sim equals the oracle bit
    for bit, the prediction equals the Python statement"""
    import torch
    from oracle import xmap_oracle as xo
    from test_gpu_recsim import _alterego_rows, _oracle_pairs, _pairs
    from xmap.engine import device
    u, it, ra, r = _alterego_rows(7, 3000, 600)
    U, I = r.n_users, r.n_items
    first = np.r_[True, u[1:] != u[:-1]]
    last = np.r_[u[1:] != u[:-1], True]
    ex = np.nonzero(first & (u % 7 == 0))[0]
    ex2 = np.nonzero(last & (u % 21 == 0))[0]
    u2 = np.concatenate([u[ex], u[ex], u[ex2]])
    it2 = np.concatenate([it[ex], it[ex], it[ex2]])
    ra2 = np.concatenate([ra[ex] * 0.5, ra[ex] * 0.75 + 0.125, ra[ex2] / 3.0]).astype(np.float64)
    o2 = np.argsort(u2, kind="stable")
    u2, it2, ra2 = u2[o2], it2[o2], ra2[o2]
    rng = np.random.default_rng(3)
    rows = dict(user=np.concatenate([u, u2]).astype(np.int32), item=np.concatenate([it, it2]).astype(np.int32),
                rating=np.concatenate([ra, ra2]).astype(np.float64), time=rng.integers(0, 4, len(u) + len(u2)).astype(np.int64))
    assert np.any(rows["rating"] != rows["rating"].astype(np.float32).astype(np.float64))
    eng = device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, I, r.item_attrs(), "cuda:0"))
    G = device.GenResult()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    G.user, G.item, G.rating, G.time = to(rows["user"]), to(rows["item"]), to(rows["rating"]), to(rows["time"])
    G.n_rows, G.n_target_rows = len(rows["user"]), len(u)
    G.off_t = to(np.concatenate([[0], np.cumsum(np.bincount(u, minlength=U))]).astype(np.int64))
    G.off_m = to(np.concatenate([[0], np.cumsum(np.bincount(u2, minlength=U))]).astype(np.int64))
    P = eng.alterego_profiles(G)
    ptr, pit, pra, ptm = group_by_user(rows, U)
    T = dict(ptr=P.user_ptr.cpu().numpy(), item=P.user_item.cpu().numpy(), rating=P.user_rating64.cpu().numpy(), time=P.user_time.cpu().numpy())
    _check_profiles(rows, T, U)
    dup = sum(len(set(pit[ptr[k]:ptr[k + 1]])) < ptr[k + 1] - ptr[k] for k in range(U))
    assert dup > 0
    e2 = device.Engine(P)
    S = e2.rec_sim(50)
    O = xo.rec_sim(ptr, pit, pra, I, 50)
    a, b, sim, ls, nij = _pairs(S, I)
    orow, ocol, osim, ols, onij = _oracle_pairs(O, I)
    assert np.array_equal(a, orow) and np.array_equal(b, ocol) and np.array_equal(nij, onij)
    assert np.array_equal(sim.view(np.uint64), osim.view(np.uint64)) and np.array_equal(ls.view(np.uint64), ols.view(np.uint64))
    assert np.array_equal(S.norm.cpu().numpy(), O.norm)
    xo.rec_free(O)
    nb = e2.rec_select(S, 10)
    avg = S.info[:I, 0].contiguous()
    T["avg"] = avg.cpu().numpy()
    _check_item_avg(T, I)
    tu, ti, real = make_pairs(rng, rows, r, 1500)
    w = to(wtab(1.5, 66))
    plain, decay, status, max_now = e2.predict(P, nb, to(np.asarray(tu, np.int32)), to(np.asarray(ti, np.int32)), avg, w)
    ratings, sims, info = dicts_from_arrays(rows, I, T["avg"], S.norm.cpu().numpy(), [x.cpu().numpy() for x in nb])
    want = statement(1.5, tu, ti, real, ratings, sims, info)
    assert None not in want and max_now <= 66
    assert device_tuples(ti, real, plain.cpu().numpy(), decay.cpu().numpy(), status.cpu().numpy()) == want
    assert any(t != () and t[2] != t[3] for t in want)


# ---------------------------------------------------------------------------------- 4. evidence beyond 64 entries
def _case_arrays(ratings, sims, info, test, n_users, n_items, keep):
    """the dictionaries of _prediction_case as the arrays of xmap_predict_rows: profiles in which a user's rows of an item
    keep the order of the item's list, neighbour lists [I][keep], averages, test pairs"""
    uid = {"U%05d" % u: u for u in range(n_users)}
    iid = {"B%04dT:" % i: i for i in range(n_items)}
    per = [[] for _ in range(n_users)]
    epoch = datetime.datetime(1970, 1, 1)
    for name in sorted(ratings):
        for who, rating, when in ratings[name]:
            per[uid[who]].append((iid[name], rating, int((when - epoch).total_seconds())))
    ptr = np.zeros(n_users + 1, np.int64)
    np.cumsum([len(p) for p in per], out=ptr[1:])
    flat = [e for p in per for e in p]
    cnt, col, sim = np.zeros(n_items, np.int32), np.full((n_items, keep), -1, np.int32), np.zeros((n_items, keep))
    for name, lst in sims.items():
        cnt[iid[name]] = len(lst)
        for q, (nid, sv) in enumerate(lst):
            col[iid[name], q], sim[iid[name], q] = iid[nid], sv
    avg = np.zeros(n_items)
    for name, v in info.items():
        avg[iid[name]] = v[0]
    tu = [uid.get(u, -1) for u, pairs in test for _ in pairs]
    ti = [iid[p[0]] for _, pairs in test for p in pairs]
    return (ptr, np.asarray([e[0] for e in flat], np.int32), np.asarray([e[1] for e in flat], np.float64),
            np.asarray([e[2] for e in flat], np.int64), cnt, col, sim, avg, np.asarray(tu, np.int32), np.asarray(ti, np.int32))


def _predict_rows(arrays, n_users, n_items, keep, alpha, n_w):
    import torch
    from xmap.engine import hipabi as abi
    dev = "cuda:0"
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    ptr, pit, pra, pti, cnt, col, sim, avg, tu, ti = d
    T = int(tu.numel())
    w = torch.from_numpy(wtab(alpha, n_w)).to(dev)
    plain, decay = torch.zeros(T, dtype=torch.float64, device=dev), torch.zeros(T, dtype=torch.float64, device=dev)
    status = torch.full((T,), -1, dtype=torch.int32, device=dev)
    h = C.c_int32(-1)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    abi.check(abi.lib.xmap_predict_rows(st, abi.i64(T), abi.vp(tu), abi.vp(ti), abi.i64(n_users), abi.i32(n_items), abi.i32(keep),
                                        abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ptr), abi.vp(pit), abi.vp(pra), abi.vp(pti),
                                        abi.vp(avg), abi.vp(w), abi.i32(n_w), abi.vp(plain), abi.vp(decay), abi.vp(status), C.byref(h)))
    return plain.cpu().numpy(), decay.cpu().numpy(), status.cpu().numpy(), h.value


def _long_evidence_case(copies):
    """the dictionaries of _prediction_case with a user holding one neighbour item `copies` times at distinct times, and a test
    line for that user over an item whose list holds the neighbour: (ratings, sims, info, test, the line, sizes)"""
    n_users, n_items, keep, dup_user = 80, 60, 10, 7
    ratings, sims, info, test = _prediction_case(3, n_users, n_items, dup_user=dup_user)
    held = "B%04dT:" % 1
    if copies > 70:
        t0 = datetime.datetime(2012, 6, 1)
        ratings[held] = ratings[held] + [("U%05d" % dup_user, float(1 + q % 5), t0 + datetime.timedelta(minutes=7 * q + 1))
                                         for q in range(copies - 70)]
        info[held] = (float(np.mean([x[1] for x in ratings[held]])), 1.0, len(ratings[held]))
    owners = [i for i, lst in sims.items() if any(n == held for n, _ in lst)]
    assert owners
    return ratings, sims, info, test, ("U%05d" % dup_user, [(owners[0], 4.0)]), (n_users, n_items, keep)


def _long_evidence_statement(ratings, sims, info, test, alpha):
    """the Python statement over the test lines; per pair the `now` (distinct times of its evidence + 1) and its evidence entries"""
    from xmap.core.recommenderPrediction import RecommenderPrediction
    tool = RecommenderPrediction(alpha, "cosine_item")
    rb, sb, ib = _B(ratings), _B(sims), _B(info)
    want = [t for line in test for t in tool.item_based_prediction(line, rb, sb, ib)[1]]
    nows = []
    for u, pairs in test:
        for p in pairs:
            times = {when for n, _ in sims.get(p[0], []) for who, _, when in ratings[n] if who == u}
            nows.append(len(times) + 1 if times else 0)
    n_ev = [sum(1 for n, _ in sims.get(p[0], []) for who, _, _ in ratings[n] if who == u) for u, pairs in test for p in pairs]
    return want, nows, n_ev


@pytest.mark.parametrize("copies", [70, 300])
def test_evidence_beyond_64_entries(copies):
    """a user holding one neighbour item 70 times with distinct times (the construction xmap_predict hands back to the host
    with status 2), and 300 times: more than the LDS staging of a wave holds, the arena launch"""
    alpha = 1.5
    ratings, sims, info, test, line, (n_users, n_items, keep) = _long_evidence_case(copies)
    test = test + [line]
    want, nows, n_ev = _long_evidence_statement(ratings, sims, info, test, alpha)
    assert max(n_ev) >= copies and n_ev[-1] == max(n_ev) and max(nows) > 66
    arrays = _case_arrays(ratings, sims, info, test, n_users, n_items, keep)
    real = [p[1] for _, pairs in test for p in pairs]
    names = [p[0] for _, pairs in test for p in pairs]
    plain, decay, status, max_now = _predict_rows(arrays, n_users, n_items, keep, alpha, max(nows))
    got = [(n, r, float(p), float(d)) if s == 0 else (() if s == 1 else None) for n, r, p, d, s in zip(names, real, plain, decay, status)]
    assert got == want and status[-1] == 0 and max_now == max(nows)
    # a table that is too short: status 2 for exactly the pairs that need more, and the length that is needed
    plain, decay, status, max_now = _predict_rows(arrays, n_users, n_items, keep, alpha, 66)
    assert max_now == max(nows) and status[-1] == 2
    for q, now in enumerate(nows):
        assert (status[q] == 2) == (now > 66)
        if status[q] != 2:
            assert got[q] == ((names[q], real[q], float(plain[q]), float(decay[q])) if status[q] == 0 else ())


# ------------------------------------------------------------------------------------ 5. host-made neighbour lists
def test_host_made_neighbor_lists():
    """the private route: recommender_privacy_pipeline(..., is_private=True) on the host under a seeded NumPy generator,
    its lists handed to the device with xmap_ctx_rec_set_neighbors"""
    from xmap.engine import synth
    from xmap.engine.localrdd import LocalRDD
    from xmap.core.recommenderPrivacy import RecommenderPrivacy
    from xmap.utils.assist import recommender_privacy_pipeline
    r = _few_times(synth.make_two_domain(5, 1500, 300, 300, overlap=0.4))
    I, U = r.n_items, 1500
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        first = np.repeat(np.arange(I), np.diff(T["row_ptr"]))
        o = np.lexsort((T["col"], first))
        recs = [((IID % a, IID % b), [np.float64(s), np.float64(l)]) for a, b, s, l in zip(first[o], T["col"][o], T["sim"][o], T["ls"][o])]
        np.random.seed(12)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            lists = [(i, list(lst)) for i, lst in recommender_privacy_pipeline(RecommenderPrivacy(10, 0.6, 0.1), LocalRDD(recs), True).collect()]
        keep = max(len(lst) for _, lst in lists)
        assert 1 <= keep <= 64
        cnt, col, sim = np.zeros(I, np.int32), np.full((I, keep), -1, np.int32), np.zeros((I, keep))
        for name, lst in lists:
            i = int(name[1:9])
            cnt[i] = len(lst)
            for q, (nid, sv) in enumerate(lst):
                col[i, q], sim[i, q] = int(nid[1:9]), sv
        ctx.call("xmap_ctx_rec_set_neighbors", keep, _p(cnt, C.c_int32), _p(col, C.c_int32), _p(sim, C.c_double))
        back = neighbors(ctx, I, keep)
        assert np.array_equal(back[0], cnt) and np.array_equal(back[1], col)
        assert np.array_equal(back[2].view(np.uint64), sim.view(np.uint64)) and not back[3].any()
        ratings, sims, info = dicts_from_arrays(rows, I, T["avg"], T["norm"], (cnt, col, sim))
        tu, ti, real = make_pairs(np.random.default_rng(5), rows, r, 1500)
        want = statement(0.2, tu, ti, real, ratings, sims, info)
        plain, decay, status, mae, _ = predict(ctx, tu, ti, real, 0.2)
        assert device_tuples(ti, real, plain, decay, status) == want        # (None = status 2 = the Python statement raises)
        assert sum(1 for t in want if t not in ((), None)) > 100
        # a list with an entry out of range is refused, the context keeps working
        bad = col.copy()
        bad[np.nonzero(cnt)[0][0], 0] = I
        rc = ctx.lib.xmap_ctx_rec_set_neighbors(ctx.h, keep, _p(cnt, C.c_int32), _p(bad, C.c_int32), _p(sim, C.c_double))
        assert rc == ctx.abi.ERR_ARG
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------- 6. MAE against the reference
def test_mae_against_the_reference():
    """the golden downstream case: rows -> RecommenderSim -> 10 neighbours -> prediction (alpha = 0.03) -> MAE on the device,
    within the tolerance test_recommender_pipeline_api uses for the same pair of numbers (ties in the selection are
    order-dependent in the reference)"""
    import torch
    from xmap.engine import device, ids
    with gzip.open(GOLD, "rt") as f:
        g = json.load(f)
    rows = g["downstream_input"]["rows"]
    uids, useen = [], {}
    for u, _, _, _ in rows:
        if u not in useen:
            useen[u] = len(uids)
            uids.append(u)
    iids = sorted({x[1] for x in rows})
    iidx = {s: k for k, s in enumerate(iids)}
    per = [[] for _ in uids]
    for u, i, ra, t in rows:
        per[useen[u]].append((iidx[i], float(ra), int(t)))
    ptr = np.zeros(len(uids) + 1, np.int64)
    np.cumsum([len(p) for p in per], out=ptr[1:])
    flat = [e for p in per for e in p]
    P = device.DeviceRatings(ptr, [e[0] for e in flat], np.asarray([e[1] for e in flat], np.float64), [e[2] for e in flat], len(iids),
                             ids.item_attrs(iids), "cuda:0", rating64=True)
    eng = device.Engine(P)
    S = eng.rec_sim(50)
    nb = eng.rec_select(S, 10)
    test = [(useen.get(u, -1), iidx.get(i, -1), float(ra)) for u, prof in g["downstream_input"]["test"] for (i, ra, t) in prof]
    to = lambda a, t: torch.from_numpy(np.asarray(a, t)).to("cuda:0")
    tu, ti, real = to([x[0] for x in test], np.int32), to([x[1] for x in test], np.int32), to([x[2] for x in test], np.float64)
    plain, decay, status, max_now = eng.predict(P, nb, tu, ti, S.info[:len(iids), 0].contiguous(), to(wtab(0.03, 66), np.float64))
    assert max_now <= 66 and int((status == 2).sum()) == 0
    m = eng.mae(status, real, plain, decay).tolist()
    ref = [float(x) for x in g["cosine_item"]["nonprivate"]["mae"].split(";")]
    assert m[0] > 0 and np.allclose([m[1] / m[0], m[2] / m[0]], ref, atol=0.02)


# --------------------------------------------------------------------------------------------- 7. the Python route
def test_session_recommend_equals_the_python_statement():
    """session.recommend on the AlterEgoRDD of generator_pipeline: the records of item_based_recommendation fed with the
    collected dictionaries; the times are datetimes with ties (the device carries their rank, not the row positions)"""
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.core.recommenderPrediction import RecommenderPrediction
    from xmap.core.recommenderSim import RecommenderSim
    from xmap.engine import session, synth
    from xmap.engine.localrdd import LocalRDD
    from xmap.utils.assist import baseliner_calculate_sim_pipeline, extender_pipeline, generator_pipeline
    r = synth.make_two_domain(9, 1200, 300, 300, overlap=0.4)
    t0 = datetime.datetime(2013, 3, 1)
    # times that do NOT grow with the row position, with ties: a later row is often the earlier rating
    recs = [(u, [(i, ra, t0 + datetime.timedelta(days=(t * 7919) % 6)) for i, ra, t in prof]) for u, prof in r.train_records()]
    sc = SparkContext(conf=SparkConf())
    trainRDD = sc.parallelize(recs, 8).cache()
    tool = BaselinerSim("cosine", CAP)
    sim = baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
    ae = generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True)
    rng = np.random.default_rng(9)
    iids = sorted({row[1] for row in ae.collect()})
    uids = [u for u, _ in recs]
    test = []
    for q in range(300):
        uid = uids[int(rng.integers(0, len(uids)))] if q % 29 else "A%013d" % (10 ** 9 + q)        # + users without any row
        pairs = [(iids[int(x)], float(rng.integers(1, 6)), t0) for x in rng.choice(len(iids), int(rng.integers(1, 5)), replace=False)]
        if q % 13 == 0:
            pairs.append((r.item_ids()[0], 3.0, t0))                                                # an item without a list
        test.append((uid, pairs))
    for alpha in (0.2, 1.5):
        out = session.recommend(ae, LocalRDD(test), CAP, 10, alpha)
        item_based = RecommenderSim("cosine_item", CAP).build_sthbased_profile(ae, "item").collectAsMap()
        ptool = RecommenderPrediction(alpha, "cosine_item")
        want = [ptool.item_based_prediction(line, _B(item_based), _B(out.sim_pairs), _B(out.item_info)) for line in test]
        got = out.collect()
        assert got == want
        assert any(p == () for _, ps in want for p in ps)
        p_plain, p_decay = [float(x) for x in ptool.calculate_mae(out).split(";")]
        assert out.mae[1] / out.mae[0] == p_plain and out.mae[2] / out.mae[0] == p_decay
    assert any(p != () and p[2] != p[3] for _, ps in want for p in ps)
    # neighbour lists made by the caller take the same route
    out2 = session.recommend(ae, LocalRDD(test), CAP, 10, 1.5, neighbors=out.sim_pairs)
    assert out2.collect() == want
    with pytest.raises(TypeError):
        session.recommend(LocalRDD(ae.collect()), LocalRDD(test), CAP, 10, 0.2)


# ---------------------------------------------------------------------------------------------------- 8. lifecycle
def _tail_bytes(ctx, r, tu, ti, real):
    rows = generate(ctx, r)
    T = rec_sim(ctx, r.n_items, len(r.user_ptr) - 1, len(rows["user"]))
    nb = select(ctx, r.n_items, 10)
    P = predict(ctx, tu, ti, real, 0.2)
    o = np.lexsort((T["col"], np.repeat(np.arange(r.n_items), np.diff(T["row_ptr"]))))      # (the order inside a row is not defined)
    for k in ("col", "sim", "ls", "nij"):
        T[k] = T[k][o]
    out = [rows[k] for k in sorted(rows) if isinstance(rows[k], np.ndarray)] + [T[k] for k in sorted(T)] + list(nb) + list(P[:4]) + [np.asarray(P[4])]
    return [np.asarray(a).tobytes() for a in out]


def test_tail_lifecycle():
    from xmap.engine import synth
    ra = _few_times(synth.make_two_domain(3, 800, 200, 200, overlap=0.4))
    rb = _few_times(synth.make_two_domain(4, 500, 150, 120, overlap=0.3))
    rng = np.random.default_rng(1)
    pa = (rng.integers(0, 800, 300).tolist(), rng.integers(200, 400, 300).tolist(), rng.integers(1, 6, 300).astype(float).tolist())
    pb = (rng.integers(0, 500, 300).tolist(), rng.integers(150, 270, 300).tolist(), rng.integers(1, 6, 300).astype(float).tolist())
    fresh = {}
    for name, r, p in (("a", ra, pa), ("b", rb, pb)):
        ctx = Ctx()
        try:
            fresh[name] = _tail_bytes(ctx, r, *p)
        finally:
            ctx.close()
    c1, c2 = Ctx(), Ctx()
    try:
        # calling out of order is an argument error, not a crash
        w, z, zi = wtab(0.2, 8), np.zeros(1), np.zeros(1, np.int32)
        args = (1, _p(zi, C.c_int32), _p(zi, C.c_int32), None, _p(w, C.c_double), 8, _p(z, C.c_double), _p(z, C.c_double), _p(zi, C.c_int32),
                None, None)
        assert c1.lib.xmap_ctx_predict(c1.h, *args) == c1.abi.ERR_ARG                         # nothing uploaded
        assert c1.lib.xmap_ctx_rec_sim(c1.h, CAP, None) == c1.abi.ERR_ARG and b"have_gen" in c1.lib.xmap_last_error()
        # two live contexts interleaved, then one context used twice: the bytes of fresh contexts
        assert _tail_bytes(c1, ra, *pa) == fresh["a"]
        assert _tail_bytes(c2, rb, *pb) == fresh["b"]
        assert c1.lib.xmap_ctx_rec_select(c2.h, 65) == c1.abi.ERR_ARG
        assert _tail_bytes(c1, rb, *pb) == fresh["b"]
        assert _tail_bytes(c2, ra, *pa) == fresh["a"]
        # an earlier stage run again drops the tail
        assert c1.lib.xmap_ctx_predict(c1.h, *args) == 0
        c1.call("xmap_ctx_item_sim", 0, CAP, None, None)
        assert c1.lib.xmap_ctx_predict(c1.h, *args) == c1.abi.ERR_ARG
        assert c1.lib.xmap_ctx_rec_download(c1.h, None, None, None, None, None, None, None) == c1.abi.ERR_ARG
        c1.call("xmap_ctx_extend", 5, None, None)
        stage_c(c1, rb.n_items, True, None)
        assert c1.lib.xmap_ctx_rec_select(c1.h, 10) == c1.abi.ERR_ARG                        # no rec_sim on the new rows yet
        c1.call("xmap_ctx_rec_sim", CAP, None)
        assert c1.lib.xmap_ctx_predict(c1.h, *args) == c1.abi.ERR_ARG                         # no neighbour lists yet
        c1.call("xmap_ctx_rec_select", 10)
        assert c1.lib.xmap_ctx_predict(c1.h, *args) == 0
    finally:
        c1.close()
        c2.close()


# ------------------------------------------------------------------------------------- 9. index spaces with gaps
def _tail_results(ctx, r, tu, ti, real, keep=10):
    """the tail of one upload: the stage-C rows, the profiles and RecommenderSim (rows sorted by column), the neighbour lists
    (entries behind a list's count: -1 / 0), the predictions"""
    I, U = r.n_items, len(r.user_ptr) - 1
    rows = generate(ctx, r)
    T = rec_sim(ctx, I, U, len(rows["user"]))
    pair_row = np.repeat(np.arange(I, dtype=np.int64), np.diff(T["row_ptr"]))
    o = np.lexsort((T["col"], pair_row))
    for name in ("col", "sim", "ls", "nij"):
        T[name] = T[name][o]
    cnt, col, sim, ls = select(ctx, I, keep)
    held = np.arange(keep)[None, :] < cnt[:, None]
    nb = (cnt, np.where(held, col, -1), np.where(held, sim, 0.0), np.where(held, ls, 0.0))
    return rows, T, pair_row, nb, predict(ctx, tu, ti, real, 0.2)


def test_tail_on_index_spaces_with_gaps():
    """xmap_ctx_rec_sim, _rec_select and _predict on an upload whose item and user indices have gaps (golden_util.with_gaps:
    unrated item indices and users without ratings, singly and in runs of more than a thousand): every result equals the
    compact upload's, re-indexed.  The input replaces 54 items (SWEEP_B's s206 at the tail driver's k = 5, cosine, private
    mapping), so the profiles hold rows of replaced items.  (No id strings here: the two tails are compared array by array.)"""
    from golden_util import check_census, with_gaps
    from test_gpu_coarse_oracle import Oracle
    from test_gpu_parity import SWEEP_B, sweep_ratings
    cfg, = [c for c in SWEEP_B if c["seed"] == 206]
    r = _few_times(sweep_ratings(cfg))
    want = Oracle(r, "cosine")
    try:
        want.stage_b(5)
        check_census(want.census(True, None), dict(mapped=50, mapped_rows=1), "the tail's input")
    finally:
        want.close()
    g, item_map, user_map = with_gaps(r, 206)
    I, U, I2, U2 = r.n_items, r.n_users, g.n_items, g.n_users
    rng = np.random.default_rng(206)
    n = 1500
    tu, ti = rng.integers(0, U, n), rng.integers(r.n_src_items, I, n)
    ti[::17] = 0                                     # a source item: no neighbour list
    tu[5::23] = -1                                   # a user the upload does not know
    real = rng.integers(1, 6, n).astype(np.float64)
    tu2, ti2 = np.where(tu >= 0, user_map[np.maximum(tu, 0)], -1), item_map[ti]
    tu2[7::29] = user_map[0] - 1                     # users without ratings: of the run at the start, the middle and the end
    tu2[8::29] = user_map[U // 2] - 1
    tu2[9::29] = U2 - 1
    tu[7::29] = tu[8::29] = tu[9::29] = -1           # (on the compact side: unknown users)
    c1, c2 = Ctx(), Ctx()
    try:
        rows, T, pair_row, nb, P = _tail_results(c1, r, tu, ti, real)
        rows2, T2, pair_row2, nb2, P2 = _tail_results(c2, g, tu2, ti2, real)
    finally:
        c1.close()
        c2.close()
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b))
    items = lambda a: np.where(a >= 0, item_map[np.maximum(a, 0)], -1)

    def scatter(a, m, n, fill=0):
        out = np.full((n,) + a.shape[1:], fill, a.dtype)
        out[m] = a
        return out
    # stage C's rows and the profiles
    assert rows2["n_target_rows"] == rows["n_target_rows"] and len(rows["user"]) > rows["n_target_rows"]
    assert same(rows2["user"], user_map[rows["user"]]) and same(rows2["item"], item_map[rows["item"]])
    assert same(rows2["rating"], rows["rating"]) and same(rows2["time"], rows["time"]) and same(rows2["choice"], scatter(items(rows["choice"]), item_map, I2, -1))
    assert same(np.diff(T2["ptr"]), scatter(np.diff(T["ptr"]), user_map, U2))
    assert same(T2["item"], item_map[T["item"]]) and same(T2["rating"], T["rating"]) and same(T2["time"], T["time"])
    # RecommenderSim
    assert len(T["col"]) > 1000
    assert same(np.diff(T2["row_ptr"]), scatter(np.diff(T["row_ptr"]), item_map, I2))
    assert same(pair_row2, item_map[pair_row]) and same(T2["col"], item_map[T["col"]])
    for name in ("sim", "ls", "nij"):
        assert same(T2[name], T[name]), name
    for name in ("avg", "norm"):
        assert same(T2[name], scatter(T[name], item_map, I2)), name
    # neighbour lists
    assert nb[0].max() == 10
    assert same(nb2[0], scatter(nb[0], item_map, I2)) and same(nb2[1], scatter(items(nb[1]), item_map, I2, -1))
    assert same(nb2[2], scatter(nb[2], item_map, I2)) and same(nb2[3], scatter(nb[3], item_map, I2))
    # predictions: the same numbers, status and sums
    assert int((P[2] == 0).sum()) > 500 and int((P[2] == 1).sum()) > 50
    for a, b, what in zip(P2, P, ("plain", "decayed", "status", "mae", "max_now")):
        assert same(a, b), what
