"""The local sensitivity between users on the device (xmap_peer_rows_ls, xmap_ctx_peers_ls, Engine.peers_ls, session.user_sim /
user_sim_from_profiles and the cosine_user drop-in) against tests/user_sim_statement.py: bit for bit, and the four shared
outputs byte for byte against xmap_peer_rows on the same inputs.  The inputs are the builders of tests/peers_statement.py."""
import ctypes as C

import numpy as np
import pytest

import peers_statement as ps
import user_sim_statement as us
from peers_statement import SAME, KEEP_SELF, CENTRED
from test_gpu_peers import DEV, DevProfiles, _dev, _stream, bits, dev_index, dev_rows, same, same_doubles

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


def dev_rows_ls(X, Q, query, n_top, cap=1, min_common=1, flags=0, allow=None, exclude=None, min_score=None, max_records=0):
    """xmap_peer_rows_ls on device copies; outputs pre-filled with -7.  -> (cnt, user, sim, common, stats, ls)"""
    import torch
    from xmap.engine import filters, hipabi as abi
    P = X.D.P
    q = _dev(np.asarray(query, np.int32))
    n_q = len(query)
    o_cnt = torch.full((max(n_q, 1),), -7, dtype=torch.int32, device=DEV)
    o_user = torch.full((max(n_q, 1), n_top), -7, dtype=torch.int32, device=DEV)
    o_sim = torch.full((max(n_q, 1), n_top), -7.0, dtype=torch.float64, device=DEV)
    o_common = torch.full((max(n_q, 1), n_top), -7, dtype=torch.int32, device=DEV)
    o_ls = torch.full((max(n_q, 1), n_top), -7.0, dtype=torch.float64, device=DEV)
    F = alive = None
    if allow is not None or exclude is not None or min_score is not None:
        words = None if allow is None else _dev(filters.pack_mask(np.asarray(allow, bool), P.n_users).view(np.int32))
        ptr = ids = None
        if exclude is not None:
            ptr, ids = [_dev(a) for a in filters.exclusion_csr(exclude)]
        alive = (words, ptr, ids)
        F = abi.rec_filter(words, ptr, ids, min_score)
    h = (C.c_int64 * 6)(*([-7] * 6))
    rc = abi.lib.xmap_peer_rows_ls(_stream(), abi.i64(n_q), abi.vp(q), abi.i64(Q.P.n_users), abi.vp(Q.ptr), abi.vp(Q.item),
                                   abi.vp(Q.rating), abi.i32(flags), abi.i32(n_top), abi.i32(cap), abi.i32(min_common), abi.i64(P.n_users),
                                   abi.i32(P.n_items), abi.vp(X.centre), abi.vp(X.hd_ptr), abi.vp(X.hd_user), abi.vp(X.hd_x), abi.vp(X.nrm),
                                   abi.i64(max_records), abi.vp(o_cnt), abi.vp(o_user), abi.vp(o_sim), abi.vp(o_common), abi.vp(o_ls),
                                   None if F is None else C.byref(F), h)
    torch.cuda.synchronize()
    del alive
    assert rc == 0, abi.lib.xmap_last_error()
    return (o_cnt.cpu().numpy()[:n_q], o_user.cpu().numpy()[:n_q], o_sim.cpu().numpy()[:n_q], o_common.cpu().numpy()[:n_q],
            [int(x) for x in h], o_ls.cpu().numpy()[:n_q])


def cut_ls(want, n_top):
    """the statement's outputs at a smaller n_top: the leading columns of each list (the stats do not depend on n_top)"""
    cnt, user, sim, common, ls, stats = want
    return np.minimum(cnt, n_top).astype(np.int32), user[:, :n_top], sim[:, :n_top], common[:, :n_top], ls[:, :n_top], stats


def check_ls(X, Q, query, n_top, want=None, **kw):
    """the LS call against the statement (want: a statement at a larger n_top, cut here) and against xmap_peer_rows"""
    if want is None:
        want = us.peer_rows_ls_statement(X.D.P, Q.P, query, n_top, centre=X.centre_host, index=X.want,
                                         **{k: v for k, v in kw.items() if k != "max_records"})
    want = cut_ls(want, n_top)
    got = dev_rows_ls(X, Q, query, n_top, **kw)
    rc, plain = dev_rows(X, Q, query, n_top, **kw)
    assert rc == 0
    same(got[:5], plain)                                                # the four shared outputs and the stats: xmap_peer_rows' bytes
    same(got[:5], (want[0], want[1], want[2], want[3], want[5]))
    assert same_doubles(got[5], want[4]), "ls bits"
    return got, want


@pytest.fixture(scope="module")
def families():
    out = {}
    for family in ("halves", "means"):
        P = ps.random_profiles(3, family)
        D = DevProfiles(P)
        out[family] = (D, {False: dev_index(D), True: dev_index(D, ps.item_means(P))})
    return out


@pytest.fixture(scope="module")
def family_wants(families):
    """the statement at n_top = 1024 per (family, centred, cap): computed once, cut per n_top"""
    out = {}
    for family, (D, idx) in families.items():
        query = ps.family_queries(D.P.n_users)
        for centred in (False, True):
            for cap in (1, 5):
                out[family, centred, cap] = us.peer_rows_ls_statement(D.P, D.P, query, 1024, cap=cap, flags=SAME,
                                                                      centre=idx[centred].centre_host, index=idx[centred].want)
    return out


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("family", ["halves", "means"])
def test_random_families_against_the_statement(families, family_wants, family, centred):
    D, idx = families[family]
    query = ps.family_queries(D.P.n_users)
    for cap in (1, 5):
        want = family_wants[family, centred, cap]
        assert (want[3][want[1] >= 0] > 1).any() and (want[4] > 0).any()
        for n_top in (1, 10, 64, 1024):
            got, _ = check_ls(idx[centred], D, query, n_top, want=want, cap=cap, flags=SAME)
            assert (got[5][got[1] < 0] == 0.0).all()                    # 0.0 behind the count


@pytest.mark.parametrize("family", ["halves", "means"])
def test_chunking_leaves_every_byte(families, family_wants, family):
    D, idx = families[family]
    query = ps.family_queries(D.P.n_users)
    for max_records in (1, 7, 64, 0):
        check_ls(idx[True], D, query, 10, want=family_wants[family, True, 5], cap=5, flags=SAME, max_records=max_records)


def test_long_runs_and_runs_of_one_record():
    P = ps.popular_profiles(257)
    rows = [[(int(P.item[p]), float(P.rating[p])) for p in range(P.ptr[u], P.ptr[u + 1])] for u in range(P.n_users)]
    rows[1] = [(0, 4.0), (0, 2.0)] * 40 + rows[1]                      # the query holds the popular item 82 times: runs of 82 and, with a
    rows[6] = [(0, 3.0), (0, 5.0)] * 20 + rows[6]                      # holder that repeats it too, of 164 and 82 * 42 records
    P = ps.Profiles.from_lists(rows, P.n_items)
    D = DevProfiles(P)
    X = dev_index(D)
    got, want = check_ls(X, D, [1, 6, 0, 2], 1024, flags=SAME | KEEP_SELF, cap=3)
    assert want[3][0].max() == 82 * 82 + 1 and (want[3][0] > 64).sum() > 200 and want[0][0] == 257
    got, want = check_ls(X, D, [1, 6], 10, flags=SAME, cap=100, max_records=1000)
    single = [0, 2, 3, 5]                                               # hold the popular item once: against each other, one record
    allow = np.zeros(P.n_users, bool)
    allow[single] = True
    got, want = check_ls(X, D, single, 10, flags=SAME, allow=allow)
    assert (got[3][got[1] >= 0] == 1).all() and got[0].tolist() == [3] * 4
    assert np.array_equal(bits(got[5]), bits(np.abs(got[2])))           # one record: ls == |sim| exactly


def test_rules_keep_the_ls_of_the_unruled_call(families):
    D, idx = families["halves"]
    X = idx[True]
    U = D.P.n_users
    query = ps.family_queries(U)
    rng = np.random.RandomState(8)
    plain = dev_rows_ls(X, D, query, 1024, flags=SAME, cap=5)
    base = {(q, int(v)): plain[5][q, j] for q in range(len(query)) for j, v in enumerate(plain[1][q][:plain[0][q]])}
    exclude = [[int(x) for x in rng.randint(0, U, 6)] + [-1, U] + [int(plain[1][q][0])] for q in range(len(query))]
    for kw in (dict(allow=rng.rand(U) < 0.5), dict(exclude=exclude), dict(min_common=2), dict(min_score=0.25),
               dict(allow=rng.rand(U) < 0.5, exclude=exclude, min_score=-0.1, min_common=2)):
        got, want = check_ls(X, D, query, 10, flags=SAME, cap=5, **kw)
        assert got[0].sum() > 0
        for q in range(len(query)):
            for j in range(got[0][q]):
                assert got[5][q, j].tobytes() == base[q, int(got[1][q, j])].tobytes(), kw


def test_fold_in_queries_are_not_same(families):
    D, idx = families["means"]
    Qp = ps.random_profiles(12, "means", U=40)
    Q = DevProfiles(Qp)
    query = np.arange(-1, Qp.n_users + 1).astype(np.int32)
    for centred in (False, True):
        got, want = check_ls(idx[centred], Q, query, 10, cap=5, flags=0)
        assert got[0].sum() > 100


def test_user_indices_of_18_bits():
    P, active = ps.sparse_wide_profiles()
    D = DevProfiles(P)
    X = dev_index(D, ps.item_means(P))
    query = np.concatenate([active[::3], [P.n_users - 1, 1 << 17, 0, 5]]).astype(np.int32)
    got, want = check_ls(X, D, query, 10, flags=SAME, cap=3)
    assert (got[1] >= (1 << 17)).any()
    other = dev_rows_ls(X, D, query, 10, flags=SAME, cap=3, max_records=5000)
    same(other[:5], got[:5])
    assert same_doubles(other[5], got[5])


def test_identical_profiles_index_order_one_ls():
    P, other = ps.tie_profiles()
    D = DevProfiles(P)
    X = dev_index(D)
    same_users = [u for u in range(P.n_users) if u not in set(other)]
    query = [other[0], same_users[0], same_users[200]]
    got, want = check_ls(X, D, query, 64, flags=SAME, cap=5)
    tied = [u for u, s in zip(got[1][1], got[2][1]) if s == got[2][1][0]]
    assert tied == [u for u in same_users if u != query[1]][:64]
    assert len(set(bits(got[5][1]).tolist())) == 1                      # 64 identical neighbours: one LS value
    check_ls(X, D, query, 401, flags=SAME, cap=5)


def test_engine_peers_ls(families):
    import torch
    from types import SimpleNamespace
    from xmap.engine import device
    D, idx = families["halves"]
    P = D.P
    view = SimpleNamespace(n_users=P.n_users, n_items=P.n_items, user_ptr=D.ptr, user_item=D.item, user_rating64=D.rating)
    eng = device.Engine(SimpleNamespace(device=torch.device(DEV)))
    X = eng.peer_index(view)
    query = ps.family_queries(P.n_users)
    allow = np.random.RandomState(2).rand(P.n_users) < 0.7
    got = eng.peers_ls(X, view, _dev(query), 10, cap=5, min_common=2, same=True, allow=_dev(allow), min_sim=0.05)
    want = us.peer_rows_ls_statement(P, P, query, 10, cap=5, min_common=2, flags=SAME, allow=allow, min_score=0.05)
    same([x.cpu().numpy() for x in got[:4]] + [got[5]], want[:4] + (want[5],))
    assert same_doubles(got[4].cpu().numpy(), want[4])
    plain = eng.peers(X, view, _dev(query), 10, cap=5, min_common=2, same=True, allow=_dev(allow), min_sim=0.05)
    same([x.cpu().numpy() for x in got[:4]] + [got[5]], [x.cpu().numpy() for x in plain[:4]] + [plain[4]])
    with pytest.raises(ValueError):
        eng.peers_ls(X, view, _dev(query), 1025)


def _ctx_peers_ls(ctx, source, queries, n_top, flags=0, cap=1, min_common=1):
    from test_gpu_coarse_abi import _p
    q = np.ascontiguousarray(queries, np.int32)
    n_q = len(q)
    cnt, user = np.full(n_q, -7, np.int32), np.full((n_q, n_top), -7, np.int32)
    sim, common, stats = np.full((n_q, n_top), -7.0), np.full((n_q, n_top), -7, np.int32), np.full(6, -7, np.int64)
    ls = np.full((n_q, n_top), -7.0)
    rc = ctx.lib.xmap_ctx_peers_ls(ctx.h, source, n_q, _p(q, C.c_int32), n_top, flags, cap, min_common, _p(cnt, C.c_int32),
                                   _p(user, C.c_int32), _p(sim, C.c_double), _p(common, C.c_int32), _p(ls, C.c_double), None,
                                   _p(stats, C.c_int64))
    return rc, (cnt, user, sim, common, stats.tolist(), ls)


def test_the_coarse_call_resident_and_fold_in():
    """NumPy only: host arrays in and out"""
    from test_gpu_coarse_abi import Ctx
    from test_gpu_foldin import foldin, foldin_download
    from test_gpu_peers import _ctx_peers, _resident
    from test_gpu_tail import _few_times, generate, rec_sim
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(7, 600, 200, 200))
    I, U = r.n_items, r.n_users
    rng = np.random.RandomState(5)
    ctx = Ctx()
    try:
        ERR = ctx.abi.ERR_ARG
        qs = np.concatenate([rng.randint(0, U, 40), [-1, U + 5]]).astype(np.int32)
        assert _ctx_peers_ls(ctx, 0, qs, 5)[0] == ERR                                  # nothing uploaded
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        P = _resident(T, I)
        for flags, centre in ((0, None), (CENTRED | KEEP_SELF, T["avg"])):
            rc, got = _ctx_peers_ls(ctx, 0, qs, 10, flags, 5, 1)
            assert rc == 0, ctx.lib.xmap_last_error()
            rc, plain = _ctx_peers(ctx, 0, qs, 10, flags, 5, 1)
            assert rc == 0
            same(got[:5], plain)
            want = us.peer_rows_ls_statement(P, P, qs, 10, cap=5, flags=SAME | (flags & KEEP_SELF), centre=centre)
            same(got[:5], want[:4] + (want[5],))
            assert same_doubles(got[5], want[4]) and want[0].sum() > 0
        B = 30
        lens = rng.randint(0, 20, B)
        f_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        f_item = rng.randint(0, I, f_ptr[-1]).astype(np.int32)
        counts = foldin(ctx, f_ptr, f_item, (rng.randint(2, 21, len(f_item)) / 4.0).astype(np.float32),
                        1000 + rng.randint(0, 7, len(f_item)).astype(np.int64))
        fp = foldin_download(ctx, B, counts[0])
        Fq = ps.Profiles(fp[0], fp[1], fp[2], I)
        bq = np.arange(-1, B + 1).astype(np.int32)
        rc, got = _ctx_peers_ls(ctx, 1, bq, 10, CENTRED, 5, 1)
        assert rc == 0
        want = us.peer_rows_ls_statement(P, Fq, bq, 10, cap=5, flags=0, centre=T["avg"])
        same(got[:5], want[:4] + (want[5],))
        assert same_doubles(got[5], want[4]) and want[0].sum() > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------- the drop-in
def b64(x):
    return int(np.float64(x).view(np.uint64))


def test_drop_in_pipeline_on_the_device_against_the_golden():
    from pyspark import SparkContext, SparkConf
    from test_cpu_user_sim_statement import LS_BOUND, golden, golden_rdds, golden_tuples
    from xmap.core.recommenderPrediction import RecommenderPrediction
    from xmap.core.recommenderPrivacy import RecommenderPrivacy
    from xmap.core.recommenderSim import RecommenderSim
    from xmap.engine import session
    from xmap.utils import assist
    g = golden()
    sc = SparkContext(conf=SparkConf())
    train, test = golden_rdds(g, sc)
    sim_tool = RecommenderSim("cosine_user", g["cap"])
    user_based, item_based, user_dict_bd, item_dict_bd, user_info_bd, item_info_bd, alterEgo_sim = \
        assist.recommender_calculate_sim_pipeline(sc, sim_tool, train)
    assert isinstance(alterEgo_sim, session.UserSimRDD) and not alterEgo_sim.by_abs
    lists = assist.recommender_privacy_pipeline(RecommenderPrivacy(g["mapping_range"], 0.6, 0.1), alterEgo_sim, False)
    assert alterEgo_sim._items is None                                  # the selection ran on the device: no row was materialised
    got = lists.collectAsMap()
    want = {u: lst for u, lst in g["lists"]}
    assert sorted(got) == sorted(want)
    for u in want:
        assert [(v, b64(s)) for v, s in got[u]] == [(v, b64(s)) for v, s in want[u]], u
    simpair_bd = sc.broadcast(got)
    tool = RecommenderPrediction(0.0, "cosine_user")
    assert tool.user_based_recommendation(test, user_dict_bd, simpair_bd, user_info_bd).collect() == golden_tuples(g)
    mae = assist.recommender_prediction_pipeline(tool, sim_tool, test, simpair_bd, user_dict_bd, item_dict_bd, user_info_bd, item_info_bd)
    assert mae == g["mae"]
    rows = dict(alterEgo_sim.collect())                                 # the full rows: sim as bits, LS within the CPU test's bound
    assert len(rows) == len(g["pairs"])
    uid = g["uid"]
    for u1, u2, s, l in g["pairs"]:
        sim, ls = rows[uid[u1], uid[u2]]
        assert b64(sim) == b64(s) and abs(ls - l) <= LS_BOUND
    P = ps.Profiles.from_lists([[(i, r) for i, r in prof] for prof in g["profiles"]], g["n_items"])
    stated = us.all_pairs_statement(P, g["cap"])                        # and the statement bit for bit
    assert all(b64(rows[uid[a], uid[b]][1]) == b64(l) for (a, b), (_, l) in stated.items())
    # the private selection and both perturbations work on the handle's rows as they are
    private = assist.recommender_privacy_pipeline(RecommenderPrivacy(g["mapping_range"], 0.6, 0.1), alterEgo_sim, True).collect()
    assert len(private) == len(want)
    # a profile with an item twice is refused, and says why
    twice = sc.parallelize([("u0", [("i0", 1.0, 0), ("i1", 2.0, 0), ("i0", 3.0, 0)]), ("u1", [("i0", 1.0, 0)])])
    with pytest.raises(ValueError, match="twice"):
        session.user_sim_from_profiles(twice, 5)


def test_negative_ratings_are_ranked_by_magnitude_on_the_host():
    from xmap.engine import session
    prof = [("a", [("i0", 1.0, 0), ("i1", 2.0, 0)]), ("b", [("i0", -1.0, 0), ("i1", -2.0, 0)]), ("c", [("i0", 1.0, 0), ("i1", 0.5, 0)]),
            ("d", [("i1", 1.0, 0)])]
    sims = session.user_sim_from_profiles(prof, 1)
    assert sims.by_abs
    rows = dict(sims.collect())
    got = dict(sims.select_neighbors(2))
    for u in "abcd":
        want = sorted([(v, info) for (a, v), info in rows.items() if a == u], key=lambda e: (-abs(e[1][0]), e[0]))[:2]
        assert got[u] == want
    assert [v for v, _ in got["a"]] == ["b", "d"] and got["a"][0][1][0] < -0.99      # last by sim, first by |sim|


def test_handle_selection_equals_the_selection_over_rows():
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from golden_util import CAP, Golden
    from test_gpu_api import records
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.engine import session
    from xmap.utils.assist import baseliner_calculate_sim_pipeline, extender_pipeline, generator_pipeline
    sc = SparkContext(conf=SparkConf())
    trainRDD = sc.parallelize(records(Golden("small")), 4).cache()
    tool = BaselinerSim("cosine", CAP)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), baseliner_calculate_sim_pipeline(sc, tool, trainRDD))
    handle = generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True)
    sims = session.user_sim(handle, 5)
    pos = {u: k for k, u in enumerate(sims.uids)}
    by = {}
    for (u1, u2), info in sims.collect():
        by.setdefault(u1, []).append((u2, info))
    assert len(by) > 100
    for k in (1, 10):
        got = sims.select_neighbors(k)
        want = [(u, sorted(by[u], key=lambda e: (-abs(e[1][0]), pos[e[0]]))[:k]) for u in sorted(by)]
        assert [u for u, _ in got] == [u for u, _ in want]
        for (u, a), (_, b) in zip(got, want):
            assert [(v, b64(i[0]), b64(i[1])) for v, i in a] == [(v, b64(i[0]), b64(i[1])) for v, i in b], u
