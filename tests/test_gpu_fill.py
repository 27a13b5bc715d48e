"""The popularity fill on the device (xmap_pop_index, xmap_topn_fill_rows, xmap_ctx_popular, xmap_ctx_recommend_filled, Engine.pop_index
/ Engine.fill, session.recommend_topn(fill=) / evaluate_topn(fill=) / popular_items) against tests/fill_statement.py.  Everything is
exact: integers with array_equal, doubles through their uint64 views, outputs pre-filled with a sentinel.  The census of the
designed inputs is tests/test_cpu_fill_statement.py's."""
import ctypes as C

import numpy as np
import pytest

import fill_statement as fs
from fill_statement import COUNT, KEEP_HELD, MEAN

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


def dev_pop_index(n_items, hd_ptr, hd_x, how, damping, min_count):
    """xmap_pop_index on device copies; outputs pre-filled with -7.  -> (rc, (item, score, pos, counts))"""
    import torch
    from xmap.engine import hipabi as abi
    d_ptr, d_x = _dev(np.ascontiguousarray(hd_ptr, np.int64)), _dev(np.ascontiguousarray(hd_x, np.float64))
    o_item = torch.full((max(n_items, 1),), -7, dtype=torch.int32, device=DEV)
    o_pos = torch.full((max(n_items, 1),), -7, dtype=torch.int32, device=DEV)
    o_score = torch.full((max(n_items, 1),), -7.0, dtype=torch.float64, device=DEV)
    h = (C.c_int64 * 3)(-7, -7, -7)
    rc = abi.lib.xmap_pop_index(_stream(), abi.i32(n_items), abi.vp(d_ptr), abi.vp(d_x), abi.i32(how), C.c_double(damping), abi.i32(min_count),
                                abi.vp(o_item), abi.vp(o_score), abi.vp(o_pos), h)
    torch.cuda.synchronize()
    return rc, (o_item.cpu().numpy()[:n_items], o_score.cpu().numpy()[:n_items], o_pos.cpu().numpy()[:n_items], tuple(int(x) for x in h))


def same_index(got, want):
    assert np.array_equal(got[0], want[0]), "pop_item"
    assert np.array_equal(bits(got[1]), bits(want[1])), "pop_score bits"
    assert np.array_equal(got[2], want[2]), "pop_pos"
    assert tuple(got[3]) == tuple(want[3]), ("counts", got[3], want[3])


class DevFill(object):
    """the resident arrays of a designed fill"""

    def __init__(self, D, ranking=None):
        self.D = D
        self.n_ranked, pop_item, pop_pos = ranking or (D.n_ranked, D.pop_item, D.pop_pos)
        self.h_pop_item = pop_item
        self.query_user, self.prof_ptr, self.prof_item = _dev(D.query_user), _dev(D.prof_ptr), _dev(D.prof_item)
        self.item_avg, self.pop_item, self.pop_pos = _dev(D.item_avg), _dev(pop_item), _dev(pop_pos)


def dev_fill(X, n_top, flags, lists, allow=None, exclude=None, min_score=None, null_filter=False, ex_csr=None, stats=True):
    """xmap_topn_fill_rows over device copies of `lists`; out_src pre-filled with -7.  -> (rc, (cnt, item, plain, decay, src, stats))"""
    import torch
    from xmap.engine import filters, hipabi as abi
    D = X.D
    Q = len(D.query_user)
    cnt, item, plain, decay = [_dev(a) for a in lists]
    src = torch.full((Q, n_top), -7, dtype=torch.int32, device=DEV)
    F = alive = None
    if null_filter or allow is not None or exclude is not None or min_score is not None or ex_csr is not None:
        words = None if allow is None else _dev(fs.mask_words(allow).view(np.int32))
        ptr = ids = None
        if ex_csr is not None:
            ptr, ids = _dev(ex_csr[0]), _dev(ex_csr[1])
        elif exclude is not None:
            ptr, ids = [_dev(a) for a in filters.exclusion_csr(exclude)]
        alive = (words, ptr, ids)
        F = abi.rec_filter(words, ptr, ids, min_score)
    h = (C.c_int64 * 4)(-7, -7, -7, -7)
    rc = abi.lib.xmap_topn_fill_rows(_stream(), abi.i64(Q), abi.vp(X.query_user), abi.i32(n_top), abi.i32(flags), abi.i64(D.n_users),
                                     abi.i32(D.n_items), abi.vp(X.prof_ptr), abi.vp(X.prof_item), abi.vp(X.item_avg), abi.i32(X.n_ranked),
                                     abi.vp(X.pop_item), abi.vp(X.pop_pos), abi.i32(D.n_pop_items), abi.vp(cnt), abi.vp(item), abi.vp(plain),
                                     abi.vp(decay), abi.vp(src), None if F is None else C.byref(F), h if stats else None)
    torch.cuda.synchronize()
    del alive
    return rc, (cnt.cpu().numpy(), item.cpu().numpy(), plain.cpu().numpy(), decay.cpu().numpy(), src.cpu().numpy(), [int(x) for x in h])


def statement(X, n_top, flags, lists, allow=None, exclude=None):
    D = X.D
    return fs.fill_statement(D.query_user, n_top, flags, D.n_users, D.n_items, D.prof_ptr, D.prof_item, D.item_avg, X.n_ranked, X.h_pop_item,
                             D.n_pop_items, *lists, allow=allow, exclude=exclude)


def same_fill(got, want):
    assert np.array_equal(got[0], want[0]), "counts"
    assert np.array_equal(got[1], want[1]), "items"
    assert np.array_equal(bits(got[2]), bits(want[2])), "plain bits"
    assert np.array_equal(bits(got[3]), bits(want[3])), "decayed bits"
    assert np.array_equal(got[4], want[4]), "src"
    assert list(got[5]) == list(want[5]), ("stats", got[5], want[5])


def as_bytes(got):
    return [np.ascontiguousarray(a).tobytes() for a in got[:5]] + [list(got[5])]


# ------------------------------------------------------------------------------------------------------- 1. the ranking
@pytest.mark.parametrize("family", fs.FAMILIES)
def test_the_ranking_of_the_designed_indexes(family):
    X = fs.design_index(family)
    for how in (COUNT, MEAN):
        for damping in fs.DAMPINGS:
            for min_count in fs.MIN_COUNTS:
                rc, got = dev_pop_index(X.n_items, X.hd_ptr, X.hd_x, how, damping, min_count)
                assert rc == 0
                same_index(got, fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, how, damping, min_count))
    rc, again = dev_pop_index(X.n_items, X.hd_ptr, X.hd_x, MEAN, 0.5, 1)        # a pure function of the index
    rc2, once = dev_pop_index(X.n_items, X.hd_ptr, X.hd_x, MEAN, 0.5, 1)
    assert rc == rc2 == 0 and [a.tobytes() for a in again[:3]] == [a.tobytes() for a in once[:3]]


def test_the_ranking_of_small_and_overflowing_indexes():
    from xmap.engine import hipabi as abi
    X = fs.overflow_index()
    for how, damping, min_count in ((MEAN, 0.0, 1), (MEAN, 25.0, 3), (COUNT, 0.0, 1), (COUNT, 0.5, 3)):
        rc, got = dev_pop_index(X.n_items, X.hd_ptr, X.hd_x, how, damping, min_count)
        assert rc == 0
        same_index(got, fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, how, damping, min_count))
    rc, got = dev_pop_index(X.n_items, X.hd_ptr, X.hd_x, MEAN, 0.0, 1)
    assert got[3] == (0, 1, 4)
    # +0.0 and -0.0 among the tied scores (negative denormal sums underflow in the division): they tie as numbers, the item index
    # orders them, pop_score keeps each score's own bits
    Z = fs.zero_index()
    for how, damping, min_count in ((MEAN, 0.0, 1), (MEAN, 0.0, 3), (MEAN, 0.5, 1), (COUNT, 0.0, 1)):
        rc, got = dev_pop_index(Z.n_items, Z.hd_ptr, Z.hd_x, how, damping, min_count)
        assert rc == 0
        same_index(got, fs.pop_statement(Z.n_items, Z.hd_ptr, Z.hd_x, how, damping, min_count))
    rc, got = dev_pop_index(Z.n_items, Z.hd_ptr, Z.hd_x, MEAN, 0.0, 1)
    assert got[0].tolist() == [4, 0, 1, 2, 3, 5] and bits(got[1]).tolist() == bits([2.0, 0.0, -0.0, 0.0, -0.0, -1.0]).tolist()
    for how in (COUNT, MEAN):
        empty = fs.Index(300, [[] for _ in range(300)])                        # an index with no rows
        rc, got = dev_pop_index(300, empty.hd_ptr, empty.hd_x, how, 0.5, 1)
        assert rc == 0 and got[3] == (0, 300, 0) and (got[0] == -1).all() and (got[2] == -1).all() and (bits(got[1]) == 0).all()
        for rows in ([[2.5, 4.0]], [[]]):                                      # n_items = 1
            one = fs.Index(1, rows)
            rc, got = dev_pop_index(1, one.hd_ptr, one.hd_x, how, 0.5, 1)
            assert rc == 0
            same_index(got, fs.pop_statement(1, one.hd_ptr, one.hd_x, how, 0.5, 1))
    X = fs.Index(3, [[1.0], [2.0], []])
    for bad in (dict(how=2), dict(damping=float("nan")), dict(damping=float("inf")), dict(damping=-1.0), dict(min_count=0)):
        a = dict(how=COUNT, damping=0.0, min_count=1)
        a.update(bad)
        rc, got = dev_pop_index(3, X.hd_ptr, X.hd_x, a["how"], a["damping"], a["min_count"])
        assert rc == abi.ERR_ARG and (got[0] == -7).all() and (got[2] == -7).all() and got[3] == (-7, -7, -7)


# ------------------------------------------------------------------------------------------------------- 2. the fill
@pytest.fixture(scope="module")
def designed():
    D = fs.design_fill()
    return D, DevFill(D)


@pytest.mark.parametrize("n_top", fs.N_TOPS)
def test_the_designed_queries_against_the_statement(designed, n_top):
    D, X = designed
    lists = fs.lists_for(D, n_top)
    before = [a.tobytes() for a in lists]
    for flags in (0, KEEP_HELD):
        for allow in (None, D.masks["half"], D.masks["one-percent"]):
            for exclude in (None, D.exclude):
                rc, got = dev_fill(X, n_top, flags, lists, allow=allow, exclude=exclude)
                assert rc == 0
                same_fill(got, statement(X, n_top, flags, lists, allow=allow, exclude=exclude))
    assert [a.tobytes() for a in lists] == before
    # the lists full on entry keep every byte
    rc, got = dev_fill(X, n_top, 0, lists, exclude=D.exclude)
    full = lists[0] == n_top
    assert full.any()
    for a, b in zip(got[:4], lists):
        assert a[full].tobytes() == b[full].tobytes()
    assert (got[4][full] == 0).all()
    # F == NULL, the null filter and a filter that holds a floor only: byte for byte (the floor is one on predictions)
    rc0, none = dev_fill(X, n_top, 0, lists)
    rc1, null = dev_fill(X, n_top, 0, lists, null_filter=True)
    rc2, floor = dev_fill(X, n_top, 0, lists, min_score=1e300)
    assert rc0 == rc1 == rc2 == 0 and as_bytes(none) == as_bytes(null) == as_bytes(floor)
    # the same call twice
    rc3, twice = dev_fill(X, n_top, 0, lists, allow=D.masks["half"], exclude=D.exclude)
    rc4, again = dev_fill(X, n_top, 0, lists, allow=D.masks["half"], exclude=D.exclude)
    assert rc3 == rc4 == 0 and as_bytes(twice) == as_bytes(again)
    rc, quiet = dev_fill(X, n_top, 0, lists, exclude=D.exclude, stats=False)     # h_stats == NULL
    assert rc == 0 and as_bytes(quiet)[:5] == as_bytes(got)[:5]


def test_a_ranking_shorter_than_the_need_and_an_empty_one(designed):
    D, _ = designed
    lists = fs.lists_for(D, 64)
    for n_ranked in (5, 0):
        X = DevFill(D, fs.short_ranking(D, n_ranked))
        for allow in (None, D.masks["half"]):
            rc, got = dev_fill(X, 64, 0, lists, allow=allow, exclude=D.exclude)
            assert rc == 0
            same_fill(got, statement(X, 64, 0, lists, allow=allow, exclude=D.exclude))
    assert got[5][2] == 0 and got[5][3] == got[5][0] > 0


def test_bad_tables_and_arguments_leave_the_outputs(designed):
    from xmap.engine import hipabi as abi
    D, X = designed
    lists = fs.lists_for(D, 10)
    Q = len(D.query_user)
    ptr, ids = np.zeros(Q + 1, np.int64), np.zeros(8, np.int32)
    for bad in ("first", "decreasing"):
        p = ptr.copy()
        if bad == "first":
            p[:] = 1
        else:
            p[3:] = 5
            p[7] = 2
        rc, got = dev_fill(X, 10, 0, lists, ex_csr=(p, ids))
        assert rc == abi.ERR_ARG and "ex_ptr" in (abi.lib.xmap_last_error() or b"").decode()
        assert [a.tobytes() for a in got[:4]] == [a.tobytes() for a in lists] and (got[4] == -7).all() and got[5] == [-7] * 4
    rc, got = dev_fill(X, 10, 0, lists, min_score=float("nan"))
    assert rc == abi.ERR_ARG and (got[4] == -7).all() and got[5] == [-7] * 4
    rc, got = dev_fill(X, 10, 2, lists)
    assert rc == abi.ERR_ARG and (got[4] == -7).all()


# ------------------------------------------------------------------------------------------------------- 3. end to end
def _transposed(ptr, item, rating, I):
    """the item-major transposition of user-major profiles in holder order, as xmap_peer_index leaves it"""
    ok = (item >= 0) & (item < I)
    o = np.flatnonzero(ok)[np.argsort(item[ok], kind="stable")]
    hd_ptr = np.concatenate([[0], np.cumsum(np.bincount(item[ok], minlength=I))]).astype(np.int64)
    return hd_ptr, rating[o]


def _filled(ctx, source, queries, n, rank_by, flags, how, damping, min_count, F=None, n_w=66, alpha=1.5):
    from test_gpu_coarse_abi import _p
    from test_gpu_tail import wtab
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    cnt, ids, src = np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32), np.full((Q, n), -7, np.int32)
    plain, decay, stats = np.full((Q, n), -7.0), np.full((Q, n), -7.0), np.full(10, -7, np.int64)
    ctx.call("xmap_ctx_recommend_filled", source, Q, _p(q, C.c_int32), n, rank_by, flags, _p(w, C.c_double), n_w, how, C.c_double(damping),
             min_count, _p(cnt, C.c_int32), _p(ids, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), _p(src, C.c_int32),
             None if F is None else C.byref(F), _p(stats, C.c_int64))
    return cnt, ids, plain, decay, src, stats.tolist()


def _filtered(ctx, source, queries, n, rank_by, flags, F=None, n_w=66, alpha=1.5):
    from test_gpu_coarse_abi import _p
    from test_gpu_tail import wtab
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    cnt, ids = np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32)
    plain, decay, stats = np.full((Q, n), -7.0), np.full((Q, n), -7.0), np.full(6, -7, np.int64)
    ctx.call("xmap_ctx_recommend_filtered", source, Q, _p(q, C.c_int32), n, rank_by, flags, _p(w, C.c_double), n_w, _p(cnt, C.c_int32),
             _p(ids, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), None if F is None else C.byref(F), _p(stats, C.c_int64))
    return cnt, ids, plain, decay, stats.tolist()


def test_the_coarse_calls_over_the_three_sources():
    from test_gpu_coarse_abi import Ctx, _p
    from test_gpu_foldin import foldin, foldin_download
    from test_gpu_item_foldin import item_foldin, item_foldin_download
    from test_gpu_tail import _few_times, generate, rec_sim, select
    from xmap.engine import hipabi as abi, synth
    seed, users, src_items, tgt_items, overlap = 5, 1500, 300, 300, 0.4          # the small case of the other coarse tail tests
    r = _few_times(synth.make_two_domain(seed, users, src_items, tgt_items, overlap=overlap))
    I, U, keep = r.n_items, users, 1
    rng = np.random.default_rng(seed)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        select(ctx, I, keep)
        B = 120
        lens = rng.integers(0, 30, B)
        f_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        f_item = rng.integers(0, I, f_ptr[-1]).astype(np.int32)
        f_counts = foldin(ctx, f_ptr, f_item, (rng.integers(2, 21, len(f_item)) / 4.0).astype(np.float32),
                          1000 + rng.integers(0, 7, len(f_item)).astype(np.int64))
        fold = foldin_download(ctx, B, f_counts[0])
        NB = 6
        b_lens = rng.integers(3, 25, NB)
        b_ptr = np.concatenate([[0], np.cumsum(b_lens)]).astype(np.int64)
        b_user = np.concatenate([rng.choice(U, k, replace=False) for k in b_lens]).astype(np.int32)
        b_counts = item_foldin(ctx, (b_ptr, b_user, rng.integers(2, 21, len(b_user)) / 4.0))
        b_rows, _ = item_foldin_download(ctx, NB, b_counts[0], keep)
        hd_ptr, hd_x = _transposed(T["ptr"], T["item"], T["rating"], I)
        # ---- xmap_ctx_popular: the head of the statement's ranking, and the ranking rebuilt when its three parameters change
        rankings = {}
        for how, damping, min_count in ((COUNT, 0.0, 1), (MEAN, 5.0, 2), (MEAN, 0.0, 1), (COUNT, 0.0, 1)):
            want = fs.pop_statement(I, hd_ptr, hd_x, how, damping, min_count)
            rankings[(how, damping, min_count)] = want
            for n_max in (0, 7, I + 5):
                out_item, out_score, n_ranked = np.full(max(n_max, 1), -7, np.int32), np.full(max(n_max, 1), -7.0), C.c_int64(-7)
                ctx.call("xmap_ctx_popular", how, C.c_double(damping), min_count, n_max, _p(out_item, C.c_int32), _p(out_score, C.c_double),
                         C.byref(n_ranked))
                assert n_ranked.value == want[3][0]
                m = min(n_max, I)
                assert np.array_equal(out_item[:m], want[0][:m]) and np.array_equal(bits(out_score[:m]), bits(want[1][:m]))
                assert (out_item[m:n_max] == -1).all() and (bits(out_score[m:n_max]) == 0).all()
        # ---- xmap_ctx_recommend_filled over the three sources
        avg_x = np.concatenate([T["avg"], b_rows[5]])
        by_source = {0: (U, T["ptr"], T["item"], I, T["avg"], np.arange(-1, U + 1)), 1: (B, fold[0], fold[1], I, T["avg"], np.arange(-1, B + 1)),
                     2: (U, T["ptr"], T["item"], I + NB, avg_x, np.arange(-1, U + 1))}
        for source, (n_users, p_ptr, p_item, n_ids, avg, qs) in by_source.items():
            qs = np.concatenate([qs, qs[5:8]]).astype(np.int32)
            mask = rng.random(n_ids) < 0.05
            exclude = [rng.integers(-2, n_ids + 2, int(rng.integers(0, 9))).tolist() for _ in qs]
            ex_ptr = np.concatenate([[0], np.cumsum([len(e) for e in exclude])]).astype(np.int64)
            ex_id = np.asarray([x for e in exclude for x in e] + [0], np.int32)
            words = fs.mask_words(mask)
            filters = {"none": (None, None, None), "rules": (abi.RecFilter(words.ctypes.data, ex_ptr.ctypes.data, ex_id.ctypes.data, 3.0), mask,
                                                             exclude)}
            for n, rank_by, flags, spec, which in ((10, 0, 0, (COUNT, 0.0, 1), "none"), (64, 1, 0, (MEAN, 5.0, 2), "rules"),
                                                   (7, 0, KEEP_HELD, (COUNT, 0.0, 1), "rules")):
                F, allow, ex = filters[which]
                base = _filtered(ctx, source, qs, n, rank_by, flags, F)
                got = _filled(ctx, source, qs, n, rank_by, flags, *spec, F=F)
                assert (base[0] < n).any() and got[5][:6] == base[4]
                for a, b in zip(got[1:4], base[1:4]):           # the model's part of every list is the unfilled call's bytes
                    for q in range(len(qs)):
                        assert a[q, :base[0][q]].tobytes() == b[q, :base[0][q]].tobytes()
                pop = rankings[spec]
                want = fs.fill_statement(qs, n, flags, n_users, n_ids, p_ptr, p_item, avg, pop[3][0], pop[0], I, *base[:4], allow=allow, exclude=ex)
                same_fill(got[:5] + (got[5][6:],), want)
                assert (got[1][got[4] == 1] < I).all()          # a batch item is never a fill
            assert got[5][8] > 0
    finally:
        ctx.close()


def test_the_coarse_calls_on_a_union_context():
    """xmap_ctx_union -> xmap_ctx_rec_sim -> xmap_ctx_popular (no neighbour lists yet) -> xmap_ctx_rec_select ->
    xmap_ctx_recommend_filled: the ranking is the statement's over the union's profiles, the lists are the filtered call's plus the
    statement's fills; a new union drops the ranking"""
    from test_gpu_coarse_abi import Ctx, _p
    from test_gpu_tail import generate, rec_sim, select
    from test_gpu_union import _trained_domains, _union
    doms = _trained_domains("multi", 2)
    numbers = np.unique(np.concatenate([r.tgt_numbers for r in doms]))
    U, I = doms[0].n_users, len(numbers)
    rng = np.random.default_rng(8)
    srcs, dst = [Ctx(), Ctx()], Ctx()
    try:
        user_maps, item_maps = [], []
        for c, r in zip(srcs, doms):
            generate(c, r)
            user_maps.append(rng.permutation(U).astype(np.int32))
            im = np.full(r.n_items, -1, np.int32)
            im[r.n_src_items:] = np.searchsorted(numbers, r.tgt_numbers)
            item_maps.append(im)
        qs = np.concatenate([[-1, U], rng.integers(0, U, 150)]).astype(np.int32)
        for flags in (0, 1):                    # the plain union, then the distinct one in its place
            rc, counts = _union(dst, srcs, user_maps, item_maps, U, I, flags)
            assert rc == 0
            T = rec_sim(dst, I, U, counts[0])
            hd_ptr, hd_x = _transposed(T["ptr"], T["item"], T["rating"], I)
            want = fs.pop_statement(I, hd_ptr, hd_x, MEAN, 2.0, 1)
            out_item, out_score, n_ranked = np.full(20, -7, np.int32), np.full(20, -7.0), C.c_int64(-7)
            dst.call("xmap_ctx_popular", MEAN, C.c_double(2.0), 1, 20, _p(out_item, C.c_int32), _p(out_score, C.c_double), C.byref(n_ranked))
            assert n_ranked.value == want[3][0] > 20
            assert np.array_equal(out_item, want[0][:20]) and np.array_equal(bits(out_score), bits(want[1][:20]))
            select(dst, I, 10)
            base = _filtered(dst, 0, qs, 10, 0, 0)
            got = _filled(dst, 0, qs, 10, 0, 0, MEAN, 2.0, 1)
            assert (base[0] < 10).any() and got[5][:6] == base[4]
            same_fill(got[:5] + (got[5][6:],), fs.fill_statement(qs, 10, 0, U, I, T["ptr"], T["item"], T["avg"], want[3][0], want[0], I, *base[:4]))
    finally:
        for c in srcs + [dst]:
            c.close()


def _np(t):
    return t.cpu().numpy()


def test_engine_and_session_fill_equal_the_statement():
    """Engine.topn + Engine.fill, session.recommend_topn(fill=), recommend_topn_profiles(fill=), evaluate_topn(fill=) and
    popular_items on the small golden problem of the other session tests: the model's part of every list is the unfilled call's,
    the filled part is the statement applied to the downloaded lists, fill=None returns what the call returns without it"""
    import datetime
    import torch
    from golden_util import CAP
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.engine import session, synth
    from xmap.utils.assist import baseliner_calculate_sim_pipeline, extender_pipeline, generator_pipeline
    ALPHA = 1.5
    r = synth.make_two_domain(9, 1200, 300, 300, overlap=0.4)
    t0 = datetime.datetime(2013, 3, 1)
    recs = [(u, [(i, ra, t0 + datetime.timedelta(days=(t * 7919) % 6)) for i, ra, t in prof]) for u, prof in r.train_records()]
    sc = SparkContext(conf=SparkConf())
    trainRDD = sc.parallelize(recs, 8).cache()
    tool = BaselinerSim("cosine", CAP)
    sim = baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
    ae = generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True)
    st, eng2, P, S, nb, item_avg = session._tail_setup(ae, CAP, 10, None, "test")
    idt = st.idt
    I, U = len(idt.iids), len(idt.uids)
    p_ptr, p_item, p_rating, avg = _np(P.user_ptr), _np(P.user_item), _np(P.user_rating64), _np(item_avg)
    hd_ptr, hd_x = _transposed(p_ptr, p_item, p_rating, I)
    rng = np.random.default_rng(17)
    no_uid = "A%013d" % (10 ** 9 + 1)
    uids = [recs[int(x)][0] for x in rng.integers(0, len(recs), 80)] + [no_uid]
    uidx = {u: k for k, u in enumerate(idt.uids)}
    query = np.asarray([uidx.get(u, -1) for u in uids], np.int32)
    # ---- Engine.pop_index / Engine.topn + Engine.fill
    X = eng2.peer_index(P)
    n = 20
    for how, code, damping, min_count in (("count", COUNT, 0.0, 1), ("mean", MEAN, 5.0, 2)):
        want_pop = fs.pop_statement(I, hd_ptr, hd_x, code, damping, min_count)
        pop = eng2.pop_index(X, how, damping, min_count)
        same_index((_np(pop.item)[:I], _np(pop.score)[:I], _np(pop.pos)[:I], pop.counts), want_pop)
        assert pop.n_ranked == want_pop[3][0]
        d_q = torch.from_numpy(query).to(DEV)
        wtab = session._decay_table(ALPHA, 66, DEV)
        lists = eng2.topn(P, nb, d_q, item_avg, wtab, n)
        before = [_np(a).copy() for a in lists[:4]]
        got = eng2.fill(lists, pop, P, d_q, item_avg)
        assert [_np(a).tobytes() for a in lists[:4]] == [a.tobytes() for a in before]       # the inputs are left as they are
        want = fs.fill_statement(query, n, 0, U, I, p_ptr, p_item, avg, want_pop[3][0], want_pop[0], I, *before)
        same_fill([_np(a) for a in got[:5]] + [list(got[5])], want)
        assert (before[0] < n).any() and want[5][2] > 0
        # ---- session.recommend_topn(fill=) against the unfilled call and the statement, on id strings
        base = session.recommend_topn(ae, uids, CAP, 10, ALPHA, n)
        assert session.recommend_topn(ae, uids, CAP, 10, ALPHA, n, fill=None).collect() == base.collect()
        assert not hasattr(base, "sources")
        spec = how if (damping, min_count) == (0.0, 1) else dict(how=how, damping=damping, min_count=min_count)
        res = session.recommend_topn(ae, uids, CAP, 10, ALPHA, n, fill=spec, explain=2 if how == "count" else None)
        for q, ((uid, lst), (_, full)) in enumerate(zip(base.collect(), res.collect())):
            c = want[0][q]
            assert full[:len(lst)] == lst and len(full) == c and res.sources[q] == want[4][q, :c].tolist()
            assert [x[0] for x in full] == [idt.iids[i] for i in want[1][q, :c]]
            assert np.array_equal(bits([x[1] for x in full]), bits(want[2][q, :c])) and np.array_equal(bits([x[2] for x in full]), bits(want[3][q, :c]))
        assert list(res.fill_stats) == want[5] and res.stats == base.stats
        if how == "count":                      # a filled pair is explained as any pair without evidence is: nothing behind it
            for (uid, lst), src in zip(res.explanations, res.sources):
                assert len(lst) == len(src) and all(e[1] == [] for e, s in zip(lst, src) if s == 1)
        shelf = session.popular_items(ae, CAP, 15, how, damping, min_count)
        assert [x[0] for x in shelf] == [idt.iids[i] for i in want_pop[0][:15]]
        assert np.array_equal(bits([x[1] for x in shelf]), bits(want_pop[1][:15]))
    # ---- diversify, then fill: fills never enter the re-ranking, .ils stays that of the model's part
    div = session.recommend_topn(ae, uids, CAP, 10, ALPHA, 10, diversify=0.5)
    both = session.recommend_topn(ae, uids, CAP, 10, ALPHA, 10, diversify=0.5, fill="count")
    assert both.ils == div.ils and both.div_stats == div.div_stats
    for (uid, lst), (_, full), src in zip(div.collect(), both.collect(), both.sources):
        assert full[:len(lst)] == lst and src == [0] * len(lst) + [1] * (len(full) - len(lst))
    assert dict(both.collect())[no_uid] and len(dict(both.collect())[no_uid]) == 10
    # ---- fold-in profiles: held is the batch's rows, popularity is the resident users'
    profiles = [("guest-%d" % k, recs[int(x)][1][:int(rng.integers(0, 4))]) for k, x in enumerate(rng.integers(0, len(recs), 12))]
    fbase = session.recommend_topn_profiles(ae, profiles, CAP, 10, ALPHA, 10)
    ffill = session.recommend_topn_profiles(ae, profiles, CAP, 10, ALPHA, 10, fill="count")
    count_pop = fs.pop_statement(I, hd_ptr, hd_x, COUNT, 0.0, 1)
    F, index, _ = session._fold_in(st, ae.G, profiles)
    f_ptr, f_item = _np(F.user_ptr), _np(F.user_item)
    for q, ((uid, lst), (_, full)) in enumerate(zip(fbase.collect(), ffill.collect())):
        held = set(f_item[f_ptr[q]:f_ptr[q + 1]].tolist()) | set(idt.iidx[x[0]] for x in lst)
        head = [idt.iids[i] for i in count_pop[0][:count_pop[3][0]] if i not in held][:10 - len(lst)]
        assert full[:len(lst)] == lst and [x[0] for x in full[len(lst):]] == head
    assert ffill.fill_stats[0] > 0
    # ---- evaluate_topn(fill=): xmap_topn_eval of the statement's lists
    held_out = [(u, [(prof[-1][0], 5.0)]) for u, prof in recs[:300] if prof]
    for fill in (None, "count"):
        ev = session.evaluate_topn(ae, held_out, CAP, 10, ALPHA, 10, cutoffs=(5, 10), fill=fill)
        uidx = {u: k for k, u in enumerate(idt.uids)}
        tu = torch.from_numpy(np.asarray([uidx.get(u, -1) for u, _ in held_out], np.int32)).to(DEV)
        ti = torch.from_numpy(np.asarray([idt.iidx.get(p[0][0], -1) for _, p in held_out], np.int32)).to(DEV)
        tr = torch.from_numpy(np.full(len(held_out), 5.0)).to(DEV)
        n_rel, users, _ = eng2.eval_users(tu, ti, tr, 4.0, U, I)
        lists = eng2.topn(P, nb, users, item_avg, session._decay_table(ALPHA, 66, DEV), 10)
        cnt, item = _np(lists[0]), _np(lists[1])
        if fill:
            out = fs.fill_statement(_np(users), 10, 0, U, I, p_ptr, p_item, avg, count_pop[3][0], count_pop[0], I, *[_np(a) for a in lists[:4]])
            cnt, item = out[0], out[1]
            assert list(ev.fill_stats) == out[5] and out[5][2] > 0
        _, _, agg, cover = eng2.topn_eval(tu, ti, tr, 4.0, n_rel, users, torch.from_numpy(cnt).to(DEV), torch.from_numpy(item).to(DEV), [5, 10], I)
        agg, cover = _np(agg), _np(cover)
        for k, c in enumerate((5, 10)):
            m = float(agg[k, 0])
            assert ev.at[c]["users"] == int(m) and ev.at[c]["coverage"] == int(cover[k])
            assert ev.at[c]["recall"] == (float(agg[k, 4]) / m if m else 0.0) and ev.at[c]["ndcg"] == (float(agg[k, 5]) / m if m else 0.0)
    sc.stop()
