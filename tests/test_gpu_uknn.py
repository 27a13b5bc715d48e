"""The user-kNN recommender on the device (xmap_uknn_means, xmap_uknn_predict_rows, xmap_uknn_topn_rows, xmap_ctx_uknn_predict /
_recommend, Engine.user_means / uknn_predict / uknn_topn, session.predict_user_knn / recommend_user_knn /
recommend_user_knn_profiles) against tests/uknn_statement.py.  Everything is compared exactly, every pair and every query of every
call: integers with array_equal, doubles through their uint64 views.  The census of the designed inputs is
tests/test_cpu_uknn_statement.py's."""
import ctypes as C
import os

import numpy as np
import pytest

import peers_statement as ps
import uknn_statement as us
from uknn_statement import OWN_MEAN, KEEP_HELD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


# ------------------------------------------------------------------------------------------------------- the drivers
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(DEV)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_doubles(a, b):
    """bit for bit, a NaN equal to any NaN (its payload is nobody's statement; no NaN is ever returned as a score)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


class DevProfiles(object):
    def __init__(self, P):
        self.P, self.ptr, self.item, self.rating = P, _dev(P.ptr), _dev(P.item), _dev(P.rating)


class DevLists(object):
    def __init__(self, lists, qavg, avg):
        self.host = lists
        self.cnt, self.user, self.sim = [_dev(a) for a in lists]
        self.n_query, self.n_nb = lists[1].shape
        self.qavg_host, self.avg_host = np.asarray(qavg, np.float64), np.asarray(avg, np.float64)
        self.qavg, self.avg = _dev(self.qavg_host), _dev(self.avg_host)


def dev_means(D):
    """xmap_uknn_means on device copies; outputs pre-filled with -7"""
    import torch
    from xmap.engine import hipabi as abi
    P = D.P
    avg = torch.full((max(P.n_users, 1),), -7.0, dtype=torch.float64, device=DEV)
    cnt = torch.full((max(P.n_users, 1),), -7, dtype=torch.int32, device=DEV)
    rc = abi.lib.xmap_uknn_means(_stream(), abi.i64(P.n_users), abi.i32(P.n_items), abi.vp(D.ptr), abi.vp(D.item), abi.vp(D.rating),
                                 abi.vp(avg), abi.vp(cnt))
    torch.cuda.synchronize()
    assert rc == 0, abi.lib.xmap_last_error()
    return avg.cpu().numpy()[:P.n_users], cnt.cpu().numpy()[:P.n_users]


def dev_predict(D, L, tq, ti, flags=0, user_avg=True):
    """xmap_uknn_predict_rows on device copies; outputs pre-filled with -7.  -> (score, bound, n, status)"""
    import torch
    from xmap.engine import hipabi as abi
    P, T = D.P, len(tq)
    d_q, d_i = _dev(np.asarray(tq, np.int32)), _dev(np.asarray(ti, np.int32))
    score, bound = [torch.full((max(T, 1),), -7.0, dtype=torch.float64, device=DEV) for _ in range(2)]
    n, status = [torch.full((max(T, 1),), -7, dtype=torch.int32, device=DEV) for _ in range(2)]
    rc = abi.lib.xmap_uknn_predict_rows(_stream(), abi.i64(T), abi.vp(d_q), abi.vp(d_i), abi.i64(L.n_query), abi.vp(L.qavg), abi.i32(L.n_nb),
                                        abi.vp(L.cnt), abi.vp(L.user), abi.vp(L.sim), abi.i64(P.n_users), abi.i32(P.n_items), abi.vp(D.ptr),
                                        abi.vp(D.item), abi.vp(D.rating), abi.vp(L.avg if user_avg else None), abi.i32(flags),
                                        abi.vp(score), abi.vp(bound), abi.vp(n), abi.vp(status))
    torch.cuda.synchronize()
    assert rc == 0, abi.lib.xmap_last_error()
    return score.cpu().numpy()[:T], bound.cpu().numpy()[:T], n.cpu().numpy()[:T], status.cpu().numpy()[:T], (score, bound, status)


def same_pairs(got, want):
    assert np.array_equal(got[3], want[3]), "status"
    assert np.array_equal(got[2], want[2]), "evidence counts"
    assert np.array_equal(bits(got[0]), bits(want[0])), "score bits"
    assert np.array_equal(bits(got[1]), bits(want[1])), "bounded"


def check_predict(D, L, tq, ti, flags=0):
    got = dev_predict(D, L, tq, ti, flags)
    want = us.predict_statement(D.P, L.host, L.qavg_host, L.avg_host, tq, ti, flags)
    same_pairs(got, want)
    return got, want


def dev_topn(D, Q, L, query, n_top, min_support=1, flags=0, allow=None, exclude=None, min_score=None, null_filter=False, max_records=0,
             stats=True):
    """xmap_uknn_topn_rows on device copies; outputs pre-filled with -7.  -> (rc, (cnt, item, score, support, stats))"""
    import torch
    from xmap.engine import filters, hipabi as abi
    P = D.P
    q = _dev(np.asarray(query, np.int32))
    n_q = len(query)
    o_cnt = torch.full((max(n_q, 1),), -7, dtype=torch.int32, device=DEV)
    o_item = torch.full((max(n_q, 1), n_top), -7, dtype=torch.int32, device=DEV)
    o_score = torch.full((max(n_q, 1), n_top), -7.0, dtype=torch.float64, device=DEV)
    o_support = torch.full((max(n_q, 1), n_top), -7, dtype=torch.int32, device=DEV)
    F = alive = None
    if null_filter or allow is not None or exclude is not None or min_score is not None:
        words = None if allow is None else _dev(filters.pack_mask(np.asarray(allow, bool), P.n_items).view(np.int32))
        ptr = ids = None
        if exclude is not None:
            ptr, ids = [_dev(a) for a in (exclude if isinstance(exclude, tuple) else filters.exclusion_csr(exclude))]
        alive = (words, ptr, ids)
        F = abi.rec_filter(words, ptr, ids, min_score)
    h = (C.c_int64 * 6)(*([-7] * 6))
    rc = abi.lib.xmap_uknn_topn_rows(_stream(), abi.i64(n_q), abi.vp(q), abi.i64(Q.P.n_users), abi.vp(Q.ptr), abi.vp(Q.item), abi.vp(L.qavg),
                                     abi.i32(L.n_nb), abi.vp(L.cnt), abi.vp(L.user), abi.vp(L.sim), abi.i64(P.n_users), abi.i32(P.n_items),
                                     abi.vp(D.ptr), abi.vp(D.item), abi.vp(D.rating), abi.vp(L.avg), abi.i32(flags), abi.i32(n_top),
                                     abi.i32(min_support), abi.i64(max_records), abi.vp(o_cnt), abi.vp(o_item), abi.vp(o_score),
                                     abi.vp(o_support), None if F is None else C.byref(F), h if stats else None)
    torch.cuda.synchronize()
    del alive
    return rc, (o_cnt.cpu().numpy()[:n_q], o_item.cpu().numpy()[:n_q], o_score.cpu().numpy()[:n_q], o_support.cpu().numpy()[:n_q],
                [int(x) for x in h])


def same(got, want):
    assert np.array_equal(got[0], want[0]), "counts"
    assert np.array_equal(got[1], want[1]), "items"
    assert np.array_equal(bits(got[2]), bits(want[2])), "score bits"
    assert np.array_equal(got[3], want[3]), "support"
    assert list(got[4]) == list(want[4]), ("stats", got[4], want[4])


def check_topn(D, Q, L, query, n_top, **kw):
    want = us.topn_statement(D.P, Q.P, query, L.host, L.qavg_host, L.avg_host, n_top,
                             **{k: v for k, v in kw.items() if k not in ("max_records", "null_filter")})
    rc, got = dev_topn(D, Q, L, query, n_top, **kw)
    assert rc == 0
    same(got, want)
    return got, want


# ------------------------------------------------------------------------------------------------------- 1. the families
@pytest.fixture(scope="module")
def families():
    out = {}
    for family in ps.FAMILIES:
        c = us.family_case(family)
        c["D"] = DevProfiles(c["P"])
        c["L"] = {n_nb: DevLists(c["lists"][n_nb], c["qavg"], c["avg"]) for n_nb in us.N_NBS}
        out[family] = c
    return out


@pytest.mark.parametrize("family", ps.FAMILIES)
def test_means_against_the_statement(families, family, monkeypatch):
    c = families[family]
    avg, cnt = dev_means(c["D"])
    assert same_doubles(avg, c["avg"]) and np.array_equal(cnt, c["cnt"])
    long = DevProfiles(ps.Profiles.from_lists([[(k % 7 if k % 11 else -1, 0.25 * (k % 13) + 1e-3 * k) for k in range(n)] for n in (0, 63, 64, 65, 300)], 7))
    want = us.means_statement(long.P)
    for span in (None, "3"):                        # (launch ranges of 3 users: XMAP_PAIR_RANGE, test-only)
        if span:
            monkeypatch.setenv("XMAP_PAIR_RANGE", span)
        got = dev_means(long)
        assert same_doubles(got[0], want[0]) and np.array_equal(got[1], want[1]) and 0 < want[1][4] < 300 and want[1][0] == 0
        assert same_doubles(dev_means(c["D"])[0], c["avg"])


@pytest.mark.parametrize("flags", [0, OWN_MEAN])
@pytest.mark.parametrize("family", ps.FAMILIES)
def test_predictions_of_the_families_against_the_statement(families, family, flags):
    c = families[family]
    tq, ti = us.pair_cases(c["P"], len(c["query"]), extra=c["extra"])
    seen = set()
    for n_nb in us.N_NBS:
        got, want = check_predict(c["D"], c["L"][n_nb], tq, ti, flags)
        seen |= set(want[3].tolist())
    assert seen == {0, 1, 2, 3}
    if c["extra"]:
        assert want[3][0] == 2                      # the NaN rating as evidence


def test_the_mae_of_the_predictions_through_xmap_mae(families, monkeypatch):
    import torch
    from xmap.engine import hipabi as abi
    c = families["halves"]
    tq, ti = us.pair_cases(c["P"], len(c["query"]))
    real = np.random.RandomState(8).randint(1, 11, len(tq)) / 2.0
    for span in (None, "64"):
        if span:
            monkeypatch.setenv("XMAP_PAIR_RANGE", span)         # the predictions launched in ranges of 64 pairs: the same bytes
        got, want = check_predict(c["D"], c["L"][65], tq, ti)
        score, bound, status = got[4]
        mae = torch.full((3,), -7.0, dtype=torch.float64, device=DEV)
        assert abi.lib.xmap_mae(_stream(), abi.i64(len(tq)), abi.vp(status), abi.vp(_dev(real)), abi.vp(bound), abi.vp(bound), abi.vp(mae)) == 0
        count, total = us.mae_statement(want[3], real, want[1])
        assert count > 300 and mae.cpu().numpy().tolist() == [count, total, total]


def test_no_user_avg_is_needed_without_own_mean(families):
    c = families["integers"]
    tq, ti = us.pair_cases(c["P"], len(c["query"]))
    same_pairs(dev_predict(c["D"], c["L"][64], tq, ti, 0, user_avg=False), dev_predict(c["D"], c["L"][64], tq, ti, 0))


def test_predictions_against_what_the_reference_recorded():
    g = us.golden_case(os.path.join(HERE, "golden", "uknn_small.json.gz"))
    D, L = DevProfiles(g["P"]), DevLists(g["lists"], g["qavg"], g["avg"])
    got, _ = check_predict(D, L, g["tq"], g["ti"], 0)
    assert us.held_to_golden(g["want"], got[1], got[3], g["tq"])
    assert same_doubles(dev_means(D)[0], g["avg"])


# ------------------------------------------------------------------------------------------------------- 2. top-N of the families
@pytest.mark.parametrize("flags", [0, OWN_MEAN])
@pytest.mark.parametrize("family", ps.FAMILIES)
def test_top_n_of_the_families_against_the_statement(families, family, flags):
    c = families[family]
    D, query = c["D"], c["query"]
    for n_nb in us.N_NBS:
        L = c["L"][n_nb]
        full = us.topn_statement(c["P"], c["P"], query, L.host, L.qavg_host, L.avg_host, 64, flags=flags, full=True)
        for n_top in (1, 5, 64):
            rc, got = dev_topn(D, D, L, query, n_top, flags=flags)
            assert rc == 0
            same(got, us.cut(full, n_top))
    assert us.census(full[5], 5)[0] * 2 > len(query)


@pytest.mark.parametrize("family", ["halves", "magnitudes"])
def test_chunk_edges_leave_every_byte(families, family):
    c = families[family]
    D, query, L = c["D"], c["query"], c["L"][65]
    allow = np.random.RandomState(4).rand(c["P"].n_items) < 0.6
    for kw in (dict(), dict(flags=OWN_MEAN | KEEP_HELD, min_support=2, allow=allow, min_score=2.0)):
        got0, _ = check_topn(D, D, L, query, 5, **kw)
        for max_records in (1, 7, 64, 4096):
            rc, got = dev_topn(D, D, L, query, 5, max_records=max_records, **kw)
            assert rc == 0
            same(got, got0)


def test_rules_support_held_mask_exclusions_floor(families):
    c = families["halves"]
    D, query, P = c["D"], c["query"], c["P"]
    rng = np.random.RandomState(4)
    allow = rng.rand(P.n_items) < 0.6
    exclude = [[int(x) for x in np.random.RandomState(q).randint(0, P.n_items, 6)] + [-1, P.n_items] for q in range(len(query))]
    for n_nb in (1, 65):
        L = c["L"][n_nb]
        plain, _ = check_topn(D, D, L, query, 5)
        rc, nul = dev_topn(D, D, L, query, 5, null_filter=True)
        assert rc == 0
        same(nul, plain)                                        # F = {NULL, NULL, NULL, -inf}: the unfiltered bytes
        for ms in (1, 2, 3):
            _, want = check_topn(D, D, L, query, 5, min_support=ms)
            assert ms == 1 or want[4][1] > 0
        _, held = check_topn(D, D, L, query, 5, flags=KEEP_HELD)
        assert held[4][0] > plain[4][0]
        check_topn(D, D, L, query, 5, allow=allow)
        check_topn(D, D, L, query, 5, exclude=exclude)
        _, want = check_topn(D, D, L, query, 5, min_score=3.0)
        assert want[4][3] > 0
        check_topn(D, D, L, query, 5, allow=allow, exclude=exclude, min_score=2.5, min_support=2, flags=OWN_MEAN)
    # a bad ex_ptr is refused on the device before an output is written; so is a NaN floor, on the host
    from xmap.engine import hipabi as abi
    ptr = np.zeros(len(query) + 1, np.int64)
    ptr[3:] = 5
    ptr[7] = 4
    for kw in (dict(exclude=(ptr, np.zeros(8, np.int32))), dict(min_score=float("nan")), dict(min_support=0)):
        rc, got = dev_topn(D, D, c["L"][65], query, 5, **kw)
        assert rc == abi.ERR_ARG, kw
        assert (got[0] == -7).all() and (got[1] == -7).all() and (got[2] == -7.0).all() and (got[3] == -7).all()


def test_launch_ranges_leave_every_byte(families, monkeypatch):
    """the wave-per-slot kernels (record counts, the expansion) launched in ranges of 3 and 64 slots (XMAP_PAIR_RANGE, test-only)
    return the bytes of the single launch"""
    c = families["means"]
    D, query, L = c["D"], c["query"], c["L"][63]
    allow = np.random.RandomState(4).rand(c["P"].n_items) < 0.6
    calls = (dict(), dict(flags=OWN_MEAN, allow=allow, min_support=2))
    want = [dev_topn(D, D, L, query, 5, **kw)[1] for kw in calls]
    for span in ("3", "64"):
        monkeypatch.setenv("XMAP_PAIR_RANGE", span)
        for kw, w in zip(calls, want):
            rc, got = dev_topn(D, D, L, query, 5, max_records=500, **kw)
            assert rc == 0
            same(got, w)


# ------------------------------------------------------------------------------------------------------- 3. the designed inputs
def _case(P, query, n_nb, cap=1):
    avg, _ = us.means_statement(P)
    lists = us.lists_from_peers(P, P, query, (n_nb,), cap=cap)[n_nb]
    return DevProfiles(P), DevLists(lists, us.gather_means(avg, query), avg)


def test_an_item_held_by_more_than_257_neighbours():
    P = us.crowd_profiles()
    query = [0, 5, 300, 0]
    D, L = _case(P, query, 300)
    assert L.host[0][0] == 280
    for flags in (0, OWN_MEAN):
        got, want = check_predict(D, L, [0, 0, 1, 2, 3, 3], [1, 0, 1, 1, 1, 12], flags)
        assert want[2][0] == 336 and want[2][1] == 280
        for kw in (dict(), dict(flags=KEEP_HELD), dict(min_support=300), dict(max_records=100)):
            kw = dict(kw, flags=kw.get("flags", 0) | flags)
            _, want = check_topn(D, D, L, query, 3, **kw)
        _, want = check_topn(D, D, L, query, 13, flags=flags)    # every candidate: item 1 with its 336 records among them
        assert 336 in want[3][0] and 336 in want[3][3]


@pytest.mark.parametrize("n_top", [1, 5, 256, 1024])
def test_bit_equal_scores_come_out_by_item_index(n_top):
    P = us.tie_item_profiles()
    D, L = _case(P, [0, 0], 8)
    for flags in (0, OWN_MEAN):
        got, want = check_topn(D, D, L, [0, 0], n_top, flags=flags)
        assert want[0].tolist() == [min(n_top, 596)] * 2
        k = want[0][0]
        assert len(set(bits(want[2][0, :k])[want[1][0, :k] != 4].tolist())) == (1 if n_top >= 5 else k - 1)   # every item but 4: one score


def test_item_indices_of_18_bits():
    P, active = us.wide_item_profiles()
    query = list(range(0, 200, 4))
    D, L = _case(P, query, 50)
    allow = np.zeros(P.n_items, bool)
    allow[active[::2]] = True
    allow[P.n_items - 1] = True
    for kw in (dict(), dict(allow=allow, max_records=300), dict(flags=KEEP_HELD | OWN_MEAN, max_records=1)):
        got, want = check_topn(D, D, L, query, 256, **kw)       # every candidate is returned: the items of 18 bits among them
        assert P.n_items - 1 in want[1] and want[0].max() > 64
    check_predict(D, L, [0, 1, 2, 3], [P.n_items - 1, 1 << 17, int(active[5]), P.n_items], 0)


def test_queries_outside_the_csr_repeated_and_folded_in(families):
    c = families["halves"]
    P, D = c["P"], c["D"]
    # the folded-in queries: five profiles nobody trained on, each with the peers of the resident user it was copied from, and means
    # of its own that are no resident user's
    rows = us._rows_of(P)
    src = [10, 11, 12, 13, 14]
    F = ps.Profiles.from_lists([[(i, r) for i, r in rows[u][:-1]] + [(int(P.n_items) - 1, 2.0 ** -9)] for u in src], P.n_items)
    f_avg, _ = us.means_statement(F)
    assert not set(f_avg.tolist()) & set(c["avg"].tolist())
    query = [0, 1, 2, 3, 4, 2, 2, -1, 5, 9]                      # batch indices: repeated, outside the batch
    lists = us.lists_from_peers(P, F, query, (30,), same=False)[30]
    L = DevLists(lists, us.gather_means(f_avg, query), c["avg"])
    Q = DevProfiles(F)
    for flags in (0, OWN_MEAN, KEEP_HELD):
        _, want = check_topn(D, Q, L, query, 7, flags=flags)
        assert np.array_equal(want[1][2], want[1][5]) and want[0][7] == 0 and want[0][0] > 0
    check_predict(D, L, [0, 1, 2, 5, 7, 9, 3], [3, 3, 7, 7, 1, 1, P.n_items - 1], 0)
    # resident queries given lists but an index outside the CSR: they hold nothing
    L2 = c["L"][65]
    query2 = np.asarray(c["query"]).copy()
    query2[5:9] = [-1, P.n_users, P.n_users + 7, -5]
    _, want = check_topn(D, D, L2, query2, 5)
    _, inside = check_topn(D, D, L2, c["query"], 5)
    assert want[4][0] > inside[4][0]


# ------------------------------------------------------------------------------------------------------- 4. the Engine
def test_engine_user_means_predict_and_topn(families):
    import torch
    from types import SimpleNamespace
    from xmap.engine import device
    c = families["integers"]
    P, D, L = c["P"], c["D"], c["L"][65]
    view = SimpleNamespace(n_users=P.n_users, n_items=P.n_items, user_ptr=D.ptr, user_item=D.item, user_rating64=D.rating)
    eng = device.Engine(SimpleNamespace(device=torch.device(DEV)))
    avg, cnt = eng.user_means(view)
    assert same_doubles(avg.cpu().numpy(), c["avg"]) and np.array_equal(cnt.cpu().numpy(), c["cnt"])
    lists = (L.cnt, L.user, L.sim)
    tq, ti = us.pair_cases(P, len(c["query"]))
    for own in (False, True):
        got = eng.uknn_predict(view, lists, L.qavg, _dev(tq), _dev(ti), avg, own)
        same_pairs([x.cpu().numpy() for x in got], us.predict_statement(P, L.host, L.qavg_host, L.avg_host, tq, ti, OWN_MEAN if own else 0))
    allow = np.random.RandomState(2).rand(P.n_items) < 0.7
    got = eng.uknn_topn(view, view, _dev(c["query"]), lists, L.qavg, 10, avg, own_mean=True, min_support=2, allow=_dev(allow), min_score=2.0)
    want = us.topn_statement(P, P, c["query"], L.host, L.qavg_host, L.avg_host, 10, min_support=2, flags=OWN_MEAN, allow=allow, min_score=2.0)
    same([x.cpu().numpy() for x in got[:4]] + [got[4]], want)
    with pytest.raises(ValueError):
        eng.uknn_topn(view, view, _dev(c["query"]), lists, L.qavg, 1025)
    with pytest.raises(ValueError):
        eng.uknn_predict(view, lists, L.qavg, _dev(tq), _dev(ti), None, True)


# ------------------------------------------------------------------------------------------------------- 5. the coarse calls
def _ctx_recommend(ctx, source, queries, n_nb, n_top, peer_flags=0, cap=1, min_common=1, flags=0, min_support=1, filt=None):
    from test_gpu_coarse_abi import _p
    q = np.ascontiguousarray(queries, np.int32)
    n_q = len(q)
    cnt, item = np.full(n_q, -7, np.int32), np.full((n_q, n_top), -7, np.int32)
    score, support, stats = np.full((n_q, n_top), -7.0), np.full((n_q, n_top), -7, np.int32), np.full(6, -7, np.int64)
    F, alive = (None, None) if filt is None else filt.on_host()
    rc = ctx.lib.xmap_ctx_uknn_recommend(ctx.h, source, n_q, _p(q, C.c_int32), n_nb, peer_flags, cap, min_common, flags, n_top, min_support,
                                         _p(cnt, C.c_int32), _p(item, C.c_int32), _p(score, C.c_double), _p(support, C.c_int32),
                                         None if F is None else C.byref(F), _p(stats, C.c_int64))
    del alive
    return rc, (cnt, item, score, support, stats.tolist())


def _ctx_predict(ctx, source, tu, ti, real, n_nb, peer_flags=0, cap=1, min_common=1, flags=0):
    from test_gpu_coarse_abi import _p
    tu, ti, real = np.ascontiguousarray(tu, np.int32), np.ascontiguousarray(ti, np.int32), np.ascontiguousarray(real, np.float64)
    T = len(tu)
    score, bound, n, status, mae = np.full(T, -7.0), np.full(T, -7.0), np.full(T, -7, np.int32), np.full(T, -7, np.int32), np.full(2, -7.0)
    rc = ctx.lib.xmap_ctx_uknn_predict(ctx.h, source, T, _p(tu, C.c_int32), _p(ti, C.c_int32), _p(real, C.c_double), n_nb, peer_flags, cap,
                                       min_common, flags, _p(score, C.c_double), _p(bound, C.c_double), _p(n, C.c_int32), _p(status, C.c_int32),
                                       _p(mae, C.c_double))
    return rc, (score, bound, n, status), mae.tolist()


def _statement_inputs(P, Q, users, n_nb, cap, mc, same, keep_self, centre):
    """what the coarse calls build inside: the peer lists of `users` and the means"""
    flags = (ps.SAME if same else 0) | (ps.KEEP_SELF if keep_self else 0)
    w = ps.peer_rows_statement(P, Q, users, n_nb, cap=cap, min_common=mc, flags=flags, centre=centre)
    avg, _ = us.means_statement(P)
    q_avg = avg if Q is P else us.means_statement(Q)[0]
    return (w[0], w[1], w[2]), us.gather_means(q_avg, users), avg


def test_the_coarse_calls_resident_and_fold_in():
    from test_gpu_coarse_abi import Ctx
    from test_gpu_filter import Filter
    from test_gpu_foldin import foldin, foldin_download
    from test_gpu_tail import _few_times, generate, rec_sim
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(7, 2000, 500, 500))
    I, U = r.n_items, r.n_users
    rng = np.random.RandomState(5)
    ctx = Ctx()
    try:
        ERR = ctx.abi.ERR_ARG
        qs = np.concatenate([rng.randint(0, U, 60), [-1, U + 5]]).astype(np.int32)
        qs[-3] = qs[0]
        assert _ctx_recommend(ctx, 0, qs, 20, 5)[0] == ERR                               # nothing uploaded
        rows = generate(ctx, r)
        assert _ctx_recommend(ctx, 0, qs, 20, 5)[0] == ERR and b"have_rec" in ctx.lib.xmap_last_error()
        T = rec_sim(ctx, I, U, len(rows["user"]))
        P = ps.Profiles(T["ptr"], T["item"], T["rating"], I)
        mask = rng.rand(I) < 0.5
        exclude = [[int(x) for x in rng.randint(0, I, 5)] + [-1, I] for _ in qs]
        for pf, centre, n_nb, cap, mc, fl, n_top, ms, filt, kw in (
                (0, None, 20, 1, 1, 0, 10, 1, None, {}),
                (ps.CENTRED, T["avg"], 65, 5, 2, OWN_MEAN, 64, 2, Filter(allow=mask, exclude=exclude, min_score=2.0),
                 dict(allow=mask, exclude=exclude, min_score=2.0)),
                (ps.CENTRED | ps.KEEP_SELF, T["avg"], 7, 3, 1, KEEP_HELD, 300, 1, Filter(null=True), {})):
            rc, got = _ctx_recommend(ctx, 0, qs, n_nb, n_top, pf, cap, mc, fl, ms, filt)
            assert rc == 0, ctx.lib.xmap_last_error()
            lists, q_avg, avg = _statement_inputs(P, P, qs, n_nb, cap, mc, True, pf & ps.KEEP_SELF, centre)
            want = us.topn_statement(P, P, qs, lists, q_avg, avg, n_top, min_support=ms, flags=fl, **kw)
            same(got, want)
            assert want[4][0] > 0
        # predictions: the held-out pairs of 40 users, some unknown, and their MAE
        tu = np.concatenate([np.repeat(rng.randint(0, U, 40), 5), [-1, U, 3, 3]]).astype(np.int32)
        ti = np.concatenate([rng.randint(0, I, 200), [4, 4, -1, I]]).astype(np.int32)
        real = rng.randint(1, 11, len(tu)) / 2.0
        for pf, centre, n_nb, cap, fl in ((ps.CENTRED, T["avg"], 30, 5, 0), (0, None, 65, 1, OWN_MEAN)):
            rc, got, mae = _ctx_predict(ctx, 0, tu, ti, real, n_nb, pf, cap, 1, fl)
            assert rc == 0, ctx.lib.xmap_last_error()
            users = np.unique(tu)
            lists, q_avg, avg = _statement_inputs(P, P, users, n_nb, cap, 1, True, False, centre)
            want = us.predict_statement(P, lists, q_avg, avg, np.searchsorted(users, tu), ti, fl)
            same_pairs(got, want)
            assert mae == list(us.mae_statement(want[3], real, want[1])) and mae[0] > 100 and set(want[3].tolist()) >= {0, 1, 3}
        # host checks with a context: XMAP_ERR_ARG, the outputs keep every byte
        for kw in (dict(n_nb=0), dict(n_nb=1025), dict(n_top=0), dict(n_top=1025), dict(min_support=0), dict(cap=0), dict(min_common=0),
                   dict(source=2), dict(peer_flags=ps.SAME), dict(flags=4), dict(filt=Filter(min_score=float("nan")))):
            a = dict(source=0, n_nb=5, n_top=5, peer_flags=0, cap=1, min_common=1, flags=0, min_support=1, filt=None)
            a.update(kw)
            rc, got = _ctx_recommend(ctx, a["source"], qs, a["n_nb"], a["n_top"], a["peer_flags"], a["cap"], a["min_common"], a["flags"],
                                     a["min_support"], a["filt"])
            assert rc == ERR, kw
            assert all((np.asarray(o) == -7).all() for o in got), kw
        assert _ctx_recommend(ctx, 1, qs, 20, 5)[0] == ERR and b"have_fold" in ctx.lib.xmap_last_error()
        # a batch of other profiles: their peers are resident users, their means and held items their own
        B = 40
        lens = rng.randint(0, 30, B)
        f_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        f_item = rng.randint(0, I, f_ptr[-1]).astype(np.int32)
        counts = foldin(ctx, f_ptr, f_item, (rng.randint(2, 21, len(f_item)) / 4.0).astype(np.float32), 1000 + rng.randint(0, 7, len(f_item)).astype(np.int64))
        fp = foldin_download(ctx, B, counts[0])
        Fq = ps.Profiles(fp[0], fp[1], fp[2], I)
        bq = np.arange(-1, B + 1).astype(np.int32)
        rc, got = _ctx_recommend(ctx, 1, bq, 25, 10, ps.CENTRED, 5, 1, OWN_MEAN, 2)
        assert rc == 0, ctx.lib.xmap_last_error()
        lists, q_avg, avg = _statement_inputs(P, Fq, bq, 25, 5, 1, False, False, T["avg"])
        want = us.topn_statement(P, Fq, bq, lists, q_avg, avg, 10, min_support=2, flags=OWN_MEAN)
        same(got, want)
        assert want[4][0] > 0
        bu = np.repeat(bq, 3)
        bi = rng.randint(0, I, len(bu)).astype(np.int32)
        rc, got, mae = _ctx_predict(ctx, 1, bu, bi, np.full(len(bu), 2.5), 25, ps.CENTRED, 5, 1, 0)
        assert rc == 0
        same_pairs(got, us.predict_statement(P, lists, q_avg, avg, np.searchsorted(np.unique(bu), bu), bi, 0))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------- 6. the session
def _mae_string(records):
    """calculate_mae of a "user" method: per line sum(errors) and their number, added up as arrays, one division, str"""
    tot = np.zeros(2)
    for _, line in records:
        errs = [abs(p[1] - p[2]) for p in line if p != ()]
        tot = tot + np.array([sum(errs), len(errs)])
    return str(tot[0] / tot[1])


def test_session_user_knn_on_the_small_golden_set():
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from golden_util import CAP, Golden
    from test_gpu_api import records
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.engine import session
    from xmap.utils.assist import baseliner_calculate_sim_pipeline, extender_pipeline, generator_pipeline
    gold = Golden("small")
    recs = records(gold)
    sc = SparkContext(conf=SparkConf())
    trainRDD = sc.parallelize(recs, 4).cache()
    tool = BaselinerSim("cosine", CAP)
    sim = baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
    ae = generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True)
    st, eng2, Pd, X, means = session._uknn_setup(ae, True, "test")
    uids, iids, uidx = st.idt.uids, st.idt.iids, session._user_index(st.idt)
    U, I = len(uids), len(iids)
    n = int(Pd.user_ptr[-1].item())
    P = ps.Profiles(Pd.user_ptr.cpu().numpy(), Pd.user_item.cpu().numpy()[:n], Pd.user_rating64.cpu().numpy()[:n], I)
    centre = X.centre.cpu().numpy()
    avg, _ = us.means_statement(P)
    assert same_doubles(means.cpu().numpy(), avg)
    users = [uids[k] for k in range(0, U, 2)] + ["nobody-knows-me", uids[0]]
    query = [uidx.get(u, -1) for u in users]
    lists, q_avg, _ = _statement_inputs(P, P, query, 12, 3, 1, True, False, centre)
    shop = [iids[k] for k in range(0, I, 3)] + ["unknown-item"]
    allow = np.zeros(I, bool)
    allow[np.arange(0, I, 3)] = True
    excl = {users[0]: [iids[1], iids[2], "unknown-item"], users[3]: list(iids[:20])}
    ex_lists = [[st.idt.iidx[x] for x in excl.get(u, ()) if x in st.idt.iidx] for u in users]
    for kw, skw in ((dict(), dict()), (dict(own_mean=True, keep_held=True, min_support=2), dict(flags=OWN_MEAN | KEEP_HELD, min_support=2)),
                    (dict(allow_items=shop, exclude=excl, min_score=2.0), dict(allow=allow, exclude=ex_lists, min_score=2.0))):
        out = session.recommend_user_knn(ae, users, 12, 7, cap=3, **kw)
        want = us.topn_statement(P, P, query, lists, q_avg, avg, 7, **skw)
        assert out.collect() == [(u, [(iids[want[1][q, t]], float(want[2][q, t]), int(want[3][q, t])) for t in range(want[0][q])])
                                 for q, u in enumerate(users)]
        assert list(out.stats) == want[4] and want[4][0] > 0
    assert out.collect()[-2] == ("nobody-knows-me", [])
    # predictions: every user's first three own records, an unknown user, an unknown item
    test = [(u, [(p[0], float(p[1])) for p in pairs[:3]]) for u, pairs in recs[:60]] + [("nobody-knows-me", [(iids[0], 3.0)]),
                                                                                          (recs[0][0], [("unknown-item", 3.0)])]
    order = {}
    for u, _ in test:
        order.setdefault(u, len(order))
    tusers = sorted(order, key=order.get)
    tlists, tq_avg, _ = _statement_inputs(P, P, [uidx.get(u, -1) for u in tusers], 12, 3, 1, True, False, centre)
    for own in (False, True):
        got, mae = session.predict_user_knn(ae, test, 12, cap=3, own_mean=own)
        tq = [order[u] for u, pairs in test for _ in pairs]
        ti = [st.idt.iidx.get(p[0], -1) for _, pairs in test for p in pairs]
        w = us.predict_statement(P, tlists, tq_avg, avg, tq, ti, OWN_MEAN if own else 0)
        assert not (w[3] == 2).any() and (w[3] == 0).sum() > 100
        lines, t = [], 0
        for u, pairs in test:
            line = []
            for p in pairs:
                line.append((p[0], p[1], float(w[1][t])) if w[3][t] == 0 else ())
                t += 1
            lines.append((u, line))
        assert got.collect() == lines and got.collect()[-2:] == [("nobody-knows-me", [()]), (recs[0][0], [()])]
        assert mae == _mae_string(lines) and got.mae == us.mae_statement(w[3], [p[1] for _, pairs in test for p in pairs], w[1])
    # profiles that are not rows of the train set: 20 train users' own records under new uids, against the statement over the
    # folded-in profiles (no self rule: each finds the train user it was copied from among its neighbours)
    picked = recs[:40:2]
    profs = [("new-" + u, list(p)) for u, p in picked]
    got = session.recommend_user_knn_profiles(ae, profs, 12, 7, cap=3)
    assert [u for u, _ in got.collect()] == ["new-" + u for u, _ in picked] and got.unknown_items == 0
    src = [uidx[u] for u, _ in picked]
    Fd = session._fold_in(st, ae.G, profs)[0]                   # the folded-in profiles the call itself builds
    nF = int(Fd.user_ptr[-1].item())
    F = ps.Profiles(Fd.user_ptr.cpu().numpy(), Fd.user_item.cpu().numpy()[:nF], Fd.user_rating64.cpu().numpy()[:nF], I)
    assert F.n_users == len(src)
    flists, fq_avg, _ = _statement_inputs(P, F, list(range(len(src))), 12, 3, 1, False, False, centre)
    want = us.topn_statement(P, F, list(range(len(src))), flists, fq_avg, avg, 7)
    assert [l for _, l in got.collect()] == [[(iids[want[1][q, t]], float(want[2][q, t]), int(want[3][q, t])) for t in range(want[0][q])]
                                             for q in range(len(src))]
    assert any(l for _, l in got.collect())
