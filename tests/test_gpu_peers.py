"""Similar users on the device (xmap_peer_index, xmap_peer_rows, xmap_ctx_peers, Engine.peer_index / peers,
session.similar_users / similar_users_profiles) against tests/peers_statement.py.  Everything is compared exactly, every query of
every call: integers with array_equal, doubles through their uint64 views.  The census of the designed inputs is
tests/test_cpu_peers_statement.py's."""
import ctypes as C

import numpy as np
import pytest

import peers_statement as ps
from peers_statement import SAME, KEEP_SELF, CENTRED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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
    """bit for bit, a NaN equal to any NaN (its payload is nobody's statement; no NaN is ever returned as a sim)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


class DevProfiles(object):
    def __init__(self, P):
        self.P, self.ptr, self.item, self.rating = P, _dev(P.ptr), _dev(P.item), _dev(P.rating)


class DevIndex(object):
    pass


def dev_index(D, centre=None):
    """xmap_peer_index on device copies, held to the statement's index; outputs pre-filled with -7"""
    import torch
    from xmap.engine import hipabi as abi
    P = D.P
    n = len(P.item)
    X = DevIndex()
    X.D, X.centre_host = D, centre
    X.centre = None if centre is None else _dev(np.asarray(centre, np.float64))
    X.hd_ptr = torch.full((P.n_items + 1,), -7, dtype=torch.int64, device=DEV)
    X.hd_user = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    X.hd_x = torch.full((max(n, 1),), -7.0, dtype=torch.float64, device=DEV)
    X.nrm = torch.full((max(P.n_users, 1),), -7.0, dtype=torch.float64, device=DEV)
    rows = C.c_int64(-7)
    rc = abi.lib.xmap_peer_index(_stream(), abi.i64(P.n_users), abi.i32(P.n_items), abi.vp(D.ptr), abi.vp(D.item), abi.vp(D.rating),
                                 abi.vp(X.centre), abi.vp(X.hd_ptr), abi.vp(X.hd_user), abi.vp(X.hd_x), abi.vp(X.nrm), C.byref(rows))
    assert rc == 0, abi.lib.xmap_last_error()
    X.want = want = ps.peer_index_statement(P, centre)
    m = want["rows"]
    assert rows.value == m
    assert np.array_equal(X.hd_ptr.cpu().numpy(), want["hd_ptr"])
    assert np.array_equal(X.hd_user.cpu().numpy()[:m], want["hd_user"])
    assert same_doubles(X.hd_x.cpu().numpy()[:m], want["hd_x"])
    assert same_doubles(X.nrm.cpu().numpy()[:P.n_users], want["nrm"])
    return X


def dev_rows(X, Q, query, n_top, cap=1, min_common=1, flags=0, allow=None, exclude=None, min_score=None, null_filter=False,
             max_records=0, stats=True):
    """xmap_peer_rows on device copies; outputs pre-filled with -7.  -> (rc, (cnt, user, sim, common, stats))"""
    import torch
    from xmap.engine import filters, hipabi as abi
    P = X.D.P
    q = _dev(np.asarray(query, np.int32))
    n_q = len(query)
    o_cnt = torch.full((max(n_q, 1),), -7, dtype=torch.int32, device=DEV)
    o_user = torch.full((max(n_q, 1), n_top), -7, dtype=torch.int32, device=DEV)
    o_sim = torch.full((max(n_q, 1), n_top), -7.0, dtype=torch.float64, device=DEV)
    o_common = torch.full((max(n_q, 1), n_top), -7, dtype=torch.int32, device=DEV)
    F = alive = None
    if null_filter or allow is not None or exclude is not None or min_score is not None:
        words = None if allow is None else _dev(filters.pack_mask(np.asarray(allow, bool), P.n_users).view(np.int32))
        ptr = ids = None
        if exclude is not None:
            ptr, ids = [_dev(a) for a in filters.exclusion_csr(exclude)]
        alive = (words, ptr, ids)
        F = abi.rec_filter(words, ptr, ids, min_score)
    h = (C.c_int64 * 6)(*([-7] * 6))
    rc = abi.lib.xmap_peer_rows(_stream(), abi.i64(n_q), abi.vp(q), abi.i64(Q.P.n_users), abi.vp(Q.ptr), abi.vp(Q.item), abi.vp(Q.rating),
                                abi.i32(flags), abi.i32(n_top), abi.i32(cap), abi.i32(min_common), abi.i64(P.n_users), abi.i32(P.n_items),
                                abi.vp(X.centre), abi.vp(X.hd_ptr), abi.vp(X.hd_user), abi.vp(X.hd_x), abi.vp(X.nrm), abi.i64(max_records),
                                abi.vp(o_cnt), abi.vp(o_user), abi.vp(o_sim), abi.vp(o_common), None if F is None else C.byref(F),
                                h if stats else None)
    torch.cuda.synchronize()
    del alive
    return rc, (o_cnt.cpu().numpy()[:n_q], o_user.cpu().numpy()[:n_q], o_sim.cpu().numpy()[:n_q], o_common.cpu().numpy()[:n_q],
                [int(x) for x in h])


def same(got, want):
    assert np.array_equal(got[0], want[0]), "counts"
    assert np.array_equal(got[1], want[1]), "users"
    assert np.array_equal(bits(got[2]), bits(want[2])), "sim bits"
    assert np.array_equal(got[3], want[3]), "common"
    assert list(got[4]) == list(want[4]), ("stats", got[4], want[4])


def cut(full, n_top):
    """the statement's outputs at a smaller n_top from its kept lists (the stats do not depend on n_top)"""
    kept, stats = full[5], full[4]
    n_q = len(kept)
    cnt, user = np.zeros(n_q, np.int32), np.full((n_q, n_top), -1, np.int32)
    sim, common = np.zeros((n_q, n_top)), np.zeros((n_q, n_top), np.int32)
    for q, k in enumerate(kept):
        cnt[q] = min(len(k), n_top)
        for j in range(cnt[q]):
            user[q, j], sim[q, j], common[q, j] = k[j]
    return cnt, user, sim, common, stats


def check(X, Q, query, n_top, **kw):
    dev_kw = dict(kw)
    want = ps.peer_rows_statement(X.D.P, Q.P, query, n_top, centre=X.centre_host, index=X.want,
                                  **{k: v for k, v in kw.items() if k not in ("max_records", "null_filter")})
    rc, got = dev_rows(X, Q, query, n_top, **dev_kw)
    assert rc == 0
    same(got, want)
    return got, want


# ------------------------------------------------------------------------------------------------------- 1, 2. families, chunks
@pytest.fixture(scope="module")
def families():
    out = {}
    for family in ps.FAMILIES:
        P = ps.random_profiles(3, family)
        D = DevProfiles(P)
        out[family] = (D, {False: dev_index(D), True: dev_index(D, ps.item_means(P))})
    return out


_queries = ps.family_queries


@pytest.mark.parametrize("centred", [False, True])
@pytest.mark.parametrize("family", ps.FAMILIES)
def test_random_families_against_the_statement(families, family, centred):
    D, idx = families[family]
    X = idx[centred]
    query = _queries(D.P.n_users)
    for cap in (1, 5):
        full = ps.peer_rows_statement(D.P, D.P, query, 65, cap=cap, flags=SAME, centre=X.centre_host, index=X.want, full=True)
        assert ps.census(full[5], 10)[0] * 2 >= len(query)
        for n_top in (1, 10, 64, 65):
            rc, got = dev_rows(X, D, query, n_top, cap=cap, flags=SAME)
            assert rc == 0
            same(got, cut(full, n_top))


@pytest.mark.parametrize("family", ["halves", "means"])
def test_chunk_edges_leave_every_byte(families, family):
    D, idx = families[family]
    X = idx[True]
    query = _queries(D.P.n_users)
    allow = np.random.RandomState(4).rand(D.P.n_users) < 0.6
    for kw in (dict(flags=SAME, cap=5), dict(flags=SAME | KEEP_SELF, min_common=2, allow=allow, min_score=0.1)):
        got0, _ = check(X, D, query, 10, **kw)
        for max_records in (1, 7, 64, 4096):
            rc, got = dev_rows(X, D, query, 10, max_records=max_records, **kw)
            assert rc == 0
            same(got, got0)


# ------------------------------------------------------------------------------------------------------- 3. a popular item
SIZES = ps.POPULAR_SIZES
_popular = ps.popular_profiles


@pytest.mark.parametrize("n_holders", SIZES)
def test_popular_item_candidate_counts_at_the_selection_edges(n_holders):
    P = _popular(n_holders)
    assert sum(1 for u in range(250) if P.ptr[u + 1] - P.ptr[u] == 3) == 50
    D = DevProfiles(P)
    X = dev_index(D)
    query = [1, 0, 6, 2, 2999]                      # holds it twice, once, twice, once, (in the larger cases) once or never
    got, want = check(X, D, query, 1024, flags=SAME | KEEP_SELF)
    assert want[4][4] == n_holders and want[0][0] == min(n_holders, 1024)
    got, want = check(X, D, query, 1024, flags=SAME)
    assert want[4][4] == n_holders - 1
    check(X, D, query, 256, flags=SAME | KEEP_SELF, cap=2)


def test_popular_item_held_by_everyone_under_masks():
    P = _popular(3000)
    D = DevProfiles(P)
    X = dev_index(D)
    rng = np.random.RandomState(6)
    for k in SIZES:
        allow = np.zeros(3000, bool)
        allow[rng.choice(3000, k, replace=False)] = True
        got, want = check(X, D, [1, 0, 1500], 1024, flags=SAME | KEEP_SELF, allow=allow)
        rows = k + int(allow[np.arange(1, 250, 5)].sum())               # eligible holder rows of item 0; user 1 holds it twice
        assert want[4][4] == k and want[4][5] == (2 + 1 + 1) * rows + int(allow[[1, 0, 1500]].sum())
    got, want = check(X, D, [1, 0, 1500], 1024, flags=SAME | KEEP_SELF)
    assert want[4][4] == 3000 and want[4][5] == (3000 + 50) * (2 + 1 + 1) + 3


# ------------------------------------------------------------------------------------------------------- 4. ties
def test_identical_profiles_come_out_by_index():
    P, other = ps.tie_profiles()
    D = DevProfiles(P)
    X = dev_index(D)
    same_users = [u for u in range(P.n_users) if u not in set(other)]
    query = [other[0], same_users[0], same_users[200], other[5]]
    for n_top in (64, 10, 399, 400, 401):
        got, want = check(X, D, query, n_top, flags=SAME)
    got, want = check(X, D, query, 64, flags=SAME)
    q = 1                                           # an identical user: the other 399 tie at the top with sim 1 or just below
    tied = [u for u, s in zip(got[1][q], got[2][q]) if s == got[2][q][0]]
    assert len(tied) == 64 and tied == sorted(tied) and tied == [u for u in same_users if u != query[q]][:64]


# ------------------------------------------------------------------------------------------------------- 5. key width
def test_user_indices_of_18_bits_and_hundreds_of_queries_in_one_chunk():
    P, active = ps.sparse_wide_profiles()
    assert P.n_users == (1 << 17) + 3 and P.ptr[-1] - P.ptr[-2] > 0
    D = DevProfiles(P)
    X = dev_index(D, ps.item_means(P))
    query = np.concatenate([active[::3], [P.n_users - 1, 1 << 17, 0, 5]]).astype(np.int32)
    assert len(query) > 300
    got, want = check(X, D, query, 10, flags=SAME, cap=3)
    assert want[4][5] < (1 << 22) and (got[1] >= (1 << 17)).any()
    rc, other = dev_rows(X, D, query, 10, flags=SAME, cap=3, max_records=5000)
    assert rc == 0
    same(other, got)


# ------------------------------------------------------------------------------------------------------- 6. self, order, repeats
def test_self_rule_permuted_and_repeated_queries(families):
    D, idx = families["means"]
    X = idx[True]
    U = D.P.n_users
    query = _queries(U)
    with_self, _ = check(X, D, query, 10, flags=SAME | KEEP_SELF, cap=5)
    without, _ = check(X, D, query, 10, flags=SAME, cap=5)
    foreign, _ = check(X, D, query, 10, flags=0, cap=5)                 # no SAME: nobody is "self"
    same(foreign, with_self)
    kept_self = sum(int(u in row) for u, row in zip(query, with_self[1]) if 0 <= u < U)
    assert kept_self > 50 and not any(int(u in row) for u, row in zip(query, without[1]) if 0 <= u < U)
    perm = np.random.RandomState(7).permutation(len(query))
    perm = np.concatenate([perm, perm[:9]])
    rc, got = dev_rows(X, D, query[perm], 10, flags=SAME, cap=5)
    assert rc == 0
    for k in range(4):
        assert np.array_equal(bits(got[k]) if k == 2 else got[k], bits(without[k][perm]) if k == 2 else without[k][perm])
    rc, again = dev_rows(X, D, query[perm], 10, flags=SAME, cap=5)
    same(again, got)


# ------------------------------------------------------------------------------------------------------- 7. rules
def test_rules_mask_exclusions_floor(families):
    D, idx = families["halves"]
    X = idx[True]
    U = D.P.n_users
    query = _queries(U)
    rng = np.random.RandomState(8)
    plain, want_plain = check(X, D, query, 10, flags=SAME)
    rc, null = dev_rows(X, D, query, 10, flags=SAME, null_filter=True)
    assert rc == 0
    same(null, plain)
    rc, nostats = dev_rows(X, D, query, 10, flags=SAME, stats=False)
    assert rc == 0 and nostats[4] == [-7] * 6
    same(nostats[:4] + (plain[4],), plain)
    allow = np.zeros(U, bool)
    allow[rng.choice(U, 3, replace=False)] = True                       # a 1 % segment
    got, want = check(X, D, query, 10, flags=SAME, allow=allow)
    assert 0 < want[4][5] < want_plain[4][5] // 20 and got[4][5] == want[4][5]
    exclude = [[int(x) for x in rng.randint(0, U, 6)] + [-1, U, U + 7] + [int(plain[1][q][0])] * 2 for q in range(len(query))]
    got, want = check(X, D, query, 10, flags=SAME, exclude=exclude)
    assert want[4][0] < want_plain[4][0]
    got, want = check(X, D, query, 10, flags=SAME, min_score=0.25)
    assert want[4][3] > 0
    got, want = check(X, D, query, 10, flags=SAME, allow=rng.rand(U) < 0.5, exclude=exclude, min_score=-0.1, min_common=2, cap=5)
    assert want[4][1] > 0 and want[4][3] > 0
    # the checks: the host's before any device work, ex_ptr on the device; the outputs keep every byte
    from xmap.engine import hipabi as abi
    for kw in (dict(n_top=0), dict(n_top=1025), dict(cap=0), dict(min_common=0), dict(flags=4), dict(min_score=float("nan")),
               dict(exclude=None, bad_ptr=True)):
        a = dict(n_top=4, cap=1, min_common=1, flags=0)
        a.update(kw)
        if a.pop("bad_ptr", False):
            import torch
            ptr = np.arange(len(query) + 1, dtype=np.int64)[::-1].copy()
            tp, ti = _dev(ptr), _dev(np.zeros(len(query) + 1, np.int32))
            F = abi.rec_filter(None, tp, ti, None)
            o = [torch.full((len(query),), -7, dtype=torch.int32, device=DEV), torch.full((len(query), 4), -7, dtype=torch.int32, device=DEV),
                 torch.full((len(query), 4), -7.0, dtype=torch.float64, device=DEV), torch.full((len(query), 4), -7, dtype=torch.int32, device=DEV)]
            rc = abi.lib.xmap_peer_rows(_stream(), abi.i64(len(query)), abi.vp(_dev(query)), abi.i64(U), abi.vp(D.ptr), abi.vp(D.item),
                                        abi.vp(D.rating), 0, 4, 1, 1, abi.i64(U), abi.i32(D.P.n_items), abi.vp(X.centre), abi.vp(X.hd_ptr),
                                        abi.vp(X.hd_user), abi.vp(X.hd_x), abi.vp(X.nrm), abi.i64(0), abi.vp(o[0]), abi.vp(o[1]), abi.vp(o[2]),
                                        abi.vp(o[3]), C.byref(F), None)
            assert rc == abi.ERR_ARG and b"ex_ptr" in abi.lib.xmap_last_error()
            assert all(bool((t == -7).all()) for t in o)
            continue
        n_top = a.pop("n_top")
        rc, got = _raw_bad(X, D, query, n_top, a)
        assert rc == abi.ERR_ARG, kw
        assert all((np.asarray(x) == -7).all() for x in got), kw


def _raw_bad(X, D, query, n_top, a):
    import torch
    from xmap.engine import hipabi as abi
    w = 4
    o = [torch.full((len(query),), -7, dtype=torch.int32, device=DEV), torch.full((len(query), w), -7, dtype=torch.int32, device=DEV),
         torch.full((len(query), w), -7.0, dtype=torch.float64, device=DEV), torch.full((len(query), w), -7, dtype=torch.int32, device=DEV)]
    F = None if a.get("min_score") is None else abi.rec_filter(None, None, None, a["min_score"])
    rc = abi.lib.xmap_peer_rows(_stream(), abi.i64(len(query)), abi.vp(_dev(query)), abi.i64(D.P.n_users), abi.vp(D.ptr), abi.vp(D.item),
                                abi.vp(D.rating), a["flags"], n_top, a["cap"], a["min_common"], abi.i64(D.P.n_users), abi.i32(D.P.n_items),
                                abi.vp(X.centre), abi.vp(X.hd_ptr), abi.vp(X.hd_user), abi.vp(X.hd_x), abi.vp(X.nrm), abi.i64(0),
                                abi.vp(o[0]), abi.vp(o[1]), abi.vp(o[2]), abi.vp(o[3]), None if F is None else C.byref(F), None)
    torch.cuda.synchronize()
    return rc, [t.cpu().numpy() for t in o]


def test_engine_peer_index_and_peers(families):
    import torch
    from types import SimpleNamespace
    from xmap.engine import device
    D, idx = families["integers"]
    P = D.P
    centre = ps.item_means(P)
    view = SimpleNamespace(n_users=P.n_users, n_items=P.n_items, user_ptr=D.ptr, user_item=D.item, user_rating64=D.rating)
    eng = device.Engine(SimpleNamespace(device=torch.device(DEV)))
    X = eng.peer_index(view, _dev(centre))
    want_X = idx[True].want
    assert X.n_rows == want_X["rows"] and same_doubles(X.nrm.cpu().numpy()[:P.n_users], want_X["nrm"])
    query = _queries(P.n_users)
    allow = np.random.RandomState(2).rand(P.n_users) < 0.7
    got = eng.peers(X, view, _dev(query), 10, cap=5, min_common=2, same=True, allow=_dev(allow), min_sim=0.05)
    want = ps.peer_rows_statement(P, P, query, 10, cap=5, min_common=2, flags=SAME, centre=centre, allow=allow, min_score=0.05)
    same([x.cpu().numpy() for x in got[:4]] + [got[4]], want)
    with pytest.raises(ValueError):
        eng.peers(X, view, _dev(query), 1025)


def test_peer_centre_is_the_exact_item_average(families):
    import torch
    from xmap.engine import hipabi as abi
    for family in ps.FAMILIES:
        D, idx = families[family]
        X = idx[False]
        out = torch.full((D.P.n_items,), -7.0, dtype=torch.float64, device=DEV)
        assert abi.lib.xmap_peer_centre(_stream(), abi.i32(D.P.n_items), abi.vp(X.hd_ptr), abi.vp(X.hd_x), abi.vp(out)) == 0
        assert same_doubles(out.cpu().numpy(), ps.item_means_exact(D.P)), family


def test_launch_ranges_leave_every_byte(families, monkeypatch):
    """the wave-per-item kernels (norms, record counts, the masked expansion, the averages) launched in ranges of 3 and 64 work
    items (XMAP_PAIR_RANGE, test-only) return the bytes of the single launch"""
    import torch
    from xmap.engine import hipabi as abi
    D, idx = families["means"]
    X = idx[True]
    query = _queries(D.P.n_users)
    allow = np.random.RandomState(4).rand(D.P.n_users) < 0.6
    calls = (dict(flags=SAME, cap=5), dict(flags=SAME | KEEP_SELF, allow=allow, min_common=2))
    want = [dev_rows(X, D, query, 10, **kw)[1] for kw in calls]
    for span in ("3", "64"):
        monkeypatch.setenv("XMAP_PAIR_RANGE", span)
        dev_index(D, X.centre_host)                             # (held to the statement inside)
        out = torch.full((D.P.n_items,), -7.0, dtype=torch.float64, device=DEV)
        assert abi.lib.xmap_peer_centre(_stream(), abi.i32(D.P.n_items), abi.vp(idx[False].hd_ptr), abi.vp(idx[False].hd_x), abi.vp(out)) == 0
        assert same_doubles(out.cpu().numpy(), ps.item_means_exact(D.P))
        for kw, w in zip(calls, want):
            rc, got = dev_rows(X, D, query, 10, **kw)
            assert rc == 0
            same(got, w)
    monkeypatch.delenv("XMAP_PAIR_RANGE")


def test_the_sort_hook_sorts_stably():
    import torch
    from xmap.engine import hipabi as abi
    rng = np.random.RandomState(3)
    for n, bits in ((1, 5), (1000, 5), (70001, 27)):
        keys = rng.randint(0, 1 << min(bits, 9), n).astype(np.int64) | (np.int64(1) << 40)     # few distinct low parts; a bit above `bits`
        k, v = _dev(keys), _dev(np.arange(n, dtype=np.int32))
        assert abi.lib.xmap_debug_sort_pairs(_stream(), abi.vp(k), abi.vp(v), abi.i64(n), abi.i32(bits)) == 0
        torch.cuda.synchronize()
        o = np.argsort(keys & ((1 << bits) - 1), kind="stable")
        assert np.array_equal(v.cpu().numpy(), o.astype(np.int32)) and np.array_equal(k.cpu().numpy(), keys[o])


# ------------------------------------------------------------------------------------------------------- 8, 9. the coarse call
def _ctx_peers(ctx, source, queries, n_top, flags=0, cap=1, min_common=1, filt=None):
    from test_gpu_coarse_abi import _p
    q = np.ascontiguousarray(queries, np.int32)
    n_q = len(q)
    cnt, user = np.full(n_q, -7, np.int32), np.full((n_q, n_top), -7, np.int32)
    sim, common, stats = np.full((n_q, n_top), -7.0), np.full((n_q, n_top), -7, np.int32), np.full(6, -7, np.int64)
    F, alive = (None, None) if filt is None else filt.on_host()
    rc = ctx.lib.xmap_ctx_peers(ctx.h, source, n_q, _p(q, C.c_int32), n_top, flags, cap, min_common, _p(cnt, C.c_int32), _p(user, C.c_int32),
                                _p(sim, C.c_double), _p(common, C.c_int32), None if F is None else C.byref(F), _p(stats, C.c_int64))
    del alive
    return rc, (cnt, user, sim, common, stats.tolist())


def _resident(T, I):
    return ps.Profiles(T["ptr"], T["item"], T["rating"], I)


def test_the_coarse_call_fold_in_and_a_changed_model():
    from test_gpu_coarse_abi import Ctx, _p
    from test_gpu_coarse_oracle import stage_c
    from test_gpu_filter import Filter
    from test_gpu_foldin import foldin
    from test_gpu_tail import _few_times, generate, rec_sim
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(7, 2000, 500, 500))       # the shape of test_gpu_foldin: a map with entries, mapped rows
    I, U = r.n_items, r.n_users
    rng = np.random.RandomState(5)
    ctx = Ctx()
    try:
        ERR = ctx.abi.ERR_ARG
        qs = np.concatenate([rng.randint(0, U, 120), [-1, U + 5]]).astype(np.int32)
        qs[-3] = qs[0]
        assert _ctx_peers(ctx, 0, qs, 5)[0] == ERR                                     # nothing uploaded
        rows = generate(ctx, r)
        assert len(rows["user"]) - rows["n_target_rows"] > 1000
        assert _ctx_peers(ctx, 0, qs, 5)[0] == ERR and b"have_rec" in ctx.lib.xmap_last_error()
        T = rec_sim(ctx, I, U, len(rows["user"]))
        P = _resident(T, I)
        mask = rng.rand(U) < 0.5
        exclude = [[int(x) for x in rng.randint(0, U, 5)] + [-1, U] for _ in qs]
        for flags, centre in ((0, None), (CENTRED, T["avg"]), (CENTRED | KEEP_SELF, T["avg"])):
            st_flags = SAME | (flags & KEEP_SELF)
            for n_top, cap, mc, filt, kw in ((10, 1, 1, None, {}), (64, 5, 2, Filter(allow=mask, exclude=exclude, min_score=0.05),
                                                                   dict(allow=mask, exclude=exclude, min_score=0.05)),
                                             (3, 3, 1, Filter(null=True), {})):
                rc, got = _ctx_peers(ctx, 0, qs, n_top, flags, cap, mc, filt)
                assert rc == 0, ctx.lib.xmap_last_error()
                want = ps.peer_rows_statement(P, P, qs, n_top, cap=cap, min_common=mc, flags=st_flags, centre=centre, **kw)
                same(got, want)
                assert want[4][0] > 0
        # host checks: XMAP_ERR_ARG, the outputs keep every byte
        for kw in (dict(n_top=0), dict(n_top=1025), dict(cap=0), dict(min_common=0), dict(source=2), dict(flags=SAME),
                   dict(filt=Filter(min_score=float("nan")))):
            a = dict(source=0, n_top=5, flags=0, cap=1, min_common=1, filt=None)
            a.update(kw)
            q = np.ascontiguousarray(qs, np.int32)
            w = 5
            outs = [np.full(len(q), -7, np.int32), np.full((len(q), w), -7, np.int32), np.full((len(q), w), -7.0), np.full((len(q), w), -7, np.int32)]
            F, alive = (None, None) if a["filt"] is None else a["filt"].on_host()
            rc = ctx.lib.xmap_ctx_peers(ctx.h, a["source"], len(q), _p(q, C.c_int32), a["n_top"], a["flags"], a["cap"], a["min_common"],
                                        _p(outs[0], C.c_int32), _p(outs[1], C.c_int32), _p(outs[2], C.c_double), _p(outs[3], C.c_int32),
                                        None if F is None else C.byref(F), None)
            assert rc == ERR, kw
            assert all((o == -7).all() for o in outs), kw
        assert _ctx_peers(ctx, 1, qs, 5)[0] == ERR and b"have_fold" in ctx.lib.xmap_last_error()
        # 8. the upload folded into itself: a folded-in user's peers are that resident user's own list with KEEP_SELF
        foldin(ctx, r.user_ptr, r.item, r.rating, r.time)
        for flags in (0, CENTRED):
            rc, folded = _ctx_peers(ctx, 1, qs, 10, flags, 5, 1)
            rc2, own = _ctx_peers(ctx, 0, qs, 10, flags | KEEP_SELF, 5, 1)
            assert rc == 0 and rc2 == 0
            same(folded, own)
            assert sum(int(u in row) for u, row in zip(qs, folded[1]) if 0 <= u < U) > 50
        # a batch of other profiles: against the statement
        B = 60
        lens = rng.randint(0, 30, B)
        f_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        f_item = rng.randint(0, I, f_ptr[-1]).astype(np.int32)
        counts = foldin(ctx, f_ptr, f_item, (rng.randint(2, 21, len(f_item)) / 4.0).astype(np.float32), 1000 + rng.randint(0, 7, len(f_item)).astype(np.int64))
        from test_gpu_foldin import foldin_download
        fp = foldin_download(ctx, B, counts[0])
        Fq = ps.Profiles(fp[0], fp[1], fp[2], I)
        bq = np.arange(-1, B + 1).astype(np.int32)
        rc, got = _ctx_peers(ctx, 1, bq, 10, CENTRED, 5, 1)
        assert rc == 0
        same(got, ps.peer_rows_statement(P, Fq, bq, 10, cap=5, flags=0, centre=T["avg"]))
        # 9. generate again with other picks: the cached index goes with the profiles
        before = _ctx_peers(ctx, 0, qs, 10, CENTRED, 5, 1)[1]
        ctx.call("xmap_ctx_extend", 50, None, None)                                   # longer candidate lists: picks to choose from
        n_top = np.zeros(I, np.int32)
        ctx.call("xmap_ctx_candidates", _p(n_top, C.c_int32))
        rows2 = stage_c(ctx, I, False, np.maximum(n_top - 2, 0))                      # the last candidate a caller may draw
        assert _ctx_peers(ctx, 0, qs, 10, CENTRED, 5, 1)[0] == ERR                    # the tail went, and the index with it
        T2 = rec_sim(ctx, I, U, len(rows2["user"]))
        assert T2["rating"].tobytes() != T["rating"].tobytes() or T2["item"].tobytes() != T["item"].tobytes()
        P2 = _resident(T2, I)
        for flags, centre in ((CENTRED, T2["avg"]), (0, None)):
            rc, got = _ctx_peers(ctx, 0, qs, 10, flags, 5, 1)
            assert rc == 0
            same(got, ps.peer_rows_statement(P2, P2, qs, 10, cap=5, flags=SAME, centre=centre))
        assert got[1].tobytes() != before[1].tobytes() or got[2].tobytes() != before[2].tobytes()
    finally:
        ctx.close()


def test_the_coarse_call_on_a_union_context():
    from test_gpu_coarse_abi import Ctx
    from test_gpu_tail import generate, rec_sim
    from test_gpu_union import _trained_domains, _union
    doms = _trained_domains("multi", 2)
    numbers = np.unique(np.concatenate([r.tgt_numbers for r in doms]))
    U, I = doms[0].n_users, len(numbers)
    rng = np.random.RandomState(8)
    srcs, dst = [Ctx(), Ctx()], Ctx()
    try:
        user_maps, item_maps = [], []
        for c, r in zip(srcs, doms):
            generate(c, r)
            user_maps.append(rng.permutation(U).astype(np.int32))
            im = np.full(r.n_items, -1, np.int32)
            im[r.n_src_items:] = np.searchsorted(numbers, r.tgt_numbers)
            item_maps.append(im)
        rc, counts = _union(dst, srcs, user_maps, item_maps, U, I, 1)
        assert rc == 0
        T = rec_sim(dst, I, U, counts[0])
        P = _resident(T, I)
        qs = np.concatenate([rng.randint(0, U, 100), [-1, U]]).astype(np.int32)
        for flags, centre in ((CENTRED, T["avg"]), (KEEP_SELF, None)):
            rc, got = _ctx_peers(dst, 0, qs, 10, flags, 5, 1)
            assert rc == 0, dst.lib.xmap_last_error()
            want = ps.peer_rows_statement(P, P, qs, 10, cap=5, flags=SAME | (flags & KEEP_SELF), centre=centre)
            same(got, want)
            assert want[4][0] > 0
    finally:
        for c in srcs + [dst]:
            c.close()


# ------------------------------------------------------------------------------------------------------- 10. the session
def test_session_similar_users_on_the_small_golden_set():
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
    for centred in (True, False):
        st, eng2, Pd, X = session._peer_setup(ae, centred, "test")
        uids, uidx = st.idt.uids, session._user_index(st.idt)
        U, I = len(uids), len(st.idt.iids)
        n = int(Pd.user_ptr[-1].item())
        P = ps.Profiles(Pd.user_ptr.cpu().numpy(), Pd.user_item.cpu().numpy()[:n], Pd.user_rating64.cpu().numpy()[:n], I)
        centre = None if not centred else X.centre.cpu().numpy()
        if centred:                                     # Engine.peer_centre gives the item averages RecommenderSim computes
            assert np.array_equal(bits(centre), bits(eng2.rec_sim(1).info[:I, 0].cpu().numpy()))
            assert session._peer_setup(ae, centred, "test")[3] is X                      # kept on the handle
        users = [uids[k] for k in range(0, U, 2)] + ["nobody-knows-me", uids[0]]
        query = [uidx.get(u, -1) for u in users]
        segment = [uids[k] for k in range(0, U, 3)] + ["unknown-user"]
        allow = np.zeros(U, bool)
        allow[np.arange(0, U, 3)] = True
        excl = {users[0]: [uids[1], uids[2], "unknown-user"], users[3]: list(uids[:20])}
        ex_lists = [[uidx[x] for x in excl.get(u, ()) if x in uidx] for u in users]
        for kw, skw in ((dict(), dict()), (dict(cap=3, min_common=2, keep_self=True), dict(cap=3, min_common=2, flags=SAME | KEEP_SELF)),
                        (dict(allow_users=segment, exclude=excl, min_sim=0.05), dict(allow=allow, exclude=ex_lists, min_score=0.05))):
            out = session.similar_users(ae, users, 7, centred=centred, **kw)
            skw = dict(skw)
            skw.setdefault("flags", SAME)
            want = ps.peer_rows_statement(P, P, query, 7, centre=centre, **skw)
            lists = [(u, [(uids[want[1][q, t]], float(want[2][q, t]), int(want[3][q, t])) for t in range(want[0][q])]) for q, u in enumerate(users)]
            assert out.collect() == lists
            assert list(out.stats) == want[4] and want[4][0] > 0
        assert out.collect()[-2] == ("nobody-knows-me", [])
        # profiles that are not rows of the train set: 20 train users' own records under new uids = their own lists with keep_self
        picked = recs[:40:2]
        got = session.similar_users_profiles(ae, [("new-" + u, list(p)) for u, p in picked], 7, cap=3, centred=centred)
        own = session.similar_users(ae, [u for u, _ in picked], 7, cap=3, centred=centred, keep_self=True)
        assert [l for _, l in got.collect()] == [l for _, l in own.collect()] and got.unknown_items == 0
        assert [u for u, _ in got.collect()] == ["new-" + u for u, _ in picked]
        assert any(l for _, l in got.collect())
