"""Diversified top-N on the device (xmap_div_index, xmap_diversify_rows, xmap_ctx_recommend_diverse, Engine.div_index / diversify,
the diversify= keyword of the session calls) against tests/diversify_statement.py.  Everything is compared exactly: integers with
array_equal, doubles through their uint64 views."""
import ctypes as C
import datetime

import numpy as np
import pytest

import diversify_statement as ds
from golden_util import CAP
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_filter import Filter, _coarse
from test_gpu_tail import _few_times, generate, rec_sim, select, wtab

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA = 1.5


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


def dev_index(n_items, row_ptr, col, sim):
    """xmap_div_index on device copies: (rc, dv_col, dv_abs, dups, the device tensors (row_ptr, dv_col, dv_abs))"""
    import torch
    from xmap.engine import hipabi as abi
    nnz = len(col)
    d_ptr, d_col, d_sim = _dev(np.asarray(row_ptr, np.int64)), _dev(np.asarray(col, np.int32)), _dev(np.asarray(sim, np.float64))
    dv_col = torch.full((max(nnz, 1),), -7, dtype=torch.int32, device=DEV)
    dv_abs = torch.full((max(nnz, 1),), -7.0, dtype=torch.float64, device=DEV)
    dups = C.c_int64(-7)
    rc = abi.lib.xmap_div_index(_stream(), abi.i32(n_items), abi.i64(nnz), abi.vp(d_ptr), abi.vp(d_col), abi.vp(d_sim), abi.vp(dv_col),
                                abi.vp(dv_abs), C.byref(dups))
    return rc, dv_col.cpu().numpy()[:nnz], dv_abs.cpu().numpy()[:nnz], dups.value, (d_ptr, dv_col, dv_abs)


def checked_index(n_items, row_ptr, col, sim):
    """the device index, held to the statement's; returns (statement index, device tensors)"""
    want = ds.div_index(row_ptr, col, sim)
    rc, dv_col, dv_abs, dups, D = dev_index(n_items, row_ptr, col, sim)
    assert rc == 0 and dups == 0 and want[2] == 0
    assert np.array_equal(dv_col, want[0]) and np.array_equal(ds.bits(dv_abs), ds.bits(want[1]))
    return want[:2], D


def dev_rerank(pool, rank_by, w, n_top, n_items, D, stats=True):
    """xmap_diversify_rows on device copies of a pool (cnt [Q], item, plain, decay [Q][n_pool]); outputs pre-filled with -7"""
    import torch
    from xmap.engine import hipabi as abi
    cnt, item, plain, decay = pool
    Q, n_pool = item.shape
    d = [_dev(np.asarray(cnt, np.int32)), _dev(np.asarray(item, np.int32)), _dev(np.asarray(plain, np.float64)), _dev(np.asarray(decay, np.float64))]
    i32o = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    f64o = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=DEV)
    o_cnt, o_item, o_plain, o_decay, o_pos, o_pen, o_ils = i32o(Q), i32o(Q, n_top), f64o(Q, n_top), f64o(Q, n_top), i32o(Q, n_top), f64o(Q, n_top), f64o(Q)
    h = (C.c_int64 * 2)(-7, -7)
    rc = abi.lib.xmap_diversify_rows(_stream(), abi.i64(Q), abi.i32(n_pool), abi.vp(d[0]), abi.vp(d[1]), abi.vp(d[2]), abi.vp(d[3]),
                                     abi.i32(rank_by), C.c_double(w), abi.i32(n_top), abi.i32(n_items), abi.vp(D[0]), abi.vp(D[1]), abi.vp(D[2]),
                                     abi.vp(o_cnt), abi.vp(o_item), abi.vp(o_plain), abi.vp(o_decay), abi.vp(o_pos), abi.vp(o_pen), abi.vp(o_ils),
                                     h if stats else None)
    torch.cuda.synchronize()
    return rc, tuple(x.cpu().numpy() for x in (o_cnt, o_item, o_plain, o_decay, o_pos, o_pen, o_ils)) + ((int(h[0]), int(h[1])),)


def check_rerank(pool, rank_by, w, n_top, n_items, row_ptr, idx, D):
    want = ds.rerank(pool[0], pool[1], pool[2], pool[3], rank_by, w, n_top, n_items, row_ptr, idx[0], idx[1])
    rc, got = dev_rerank(pool, rank_by, w, n_top, n_items, D)
    assert rc == 0
    ds.same(got[:7], want[:7])
    assert got[7] == want[7]
    return want


# ------------------------------------------------------------------------------------------------------- 1. the index
def test_index_of_nothing_and_of_short_rows():
    from xmap.engine import hipabi as abi
    for I in (0, 1):
        rc, dv_col, dv_abs, dups, _ = dev_index(I, np.zeros(I + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
        assert rc == 0 and dups == 0 and len(dv_col) == 0
    checked_index(1, [0, 1], [0], [-0.75])                                  # I = 1 with its self pair
    rows = {0: [], 1: [(4, -0.5)], 2: [(5, 0.25), (1, -1.0)], 3: [(1, 0.5), (2, -0.0)], 5: [(0, 5e-324), (5, -2.0)]}     # lengths 0, 1, 2
    rp, col, sim = ds.csr_of(rows, 6)
    idx, _ = checked_index(6, rp, col, sim)
    assert idx[0].tolist() == [4, 1, 5, 1, 2, 0, 5] and idx[1].tolist() == [0.5, 1.0, 0.25, 0.5, 0.0, 5e-324, 2.0]
    # one repeated (row, column): refused, the count reported
    rp, col, sim = ds.csr_of({0: [(2, 0.5), (1, -0.25), (2, 0.125)], 2: [(0, 1.0)]}, 3)
    rc, _, _, dups, _ = dev_index(3, rp, col, sim)
    assert rc == abi.ERR_ARG and dups == 1 and ds.div_index(rp, col, sim)[2] == 1
    assert b"repeated" in abi.lib.xmap_last_error()


def test_index_under_every_storage_order():
    rng = np.random.default_rng(11)
    rp, col, sim, _ = ds.random_sym_csr(rng, 300, 0.2, lambda g, n: g.random(n) + 0.01)
    base, _ = checked_index(300, rp, col, sim)
    for how in ("asc", "desc", "shuffle"):
        c2, s2 = ds.shuffle_rows(rng, rp, col, sim, how)
        idx, _ = checked_index(300, rp, c2, s2)
        assert np.array_equal(idx[0], base[0]) and np.array_equal(ds.bits(idx[1]), ds.bits(base[1]))


def test_index_with_keys_wider_than_32_bits():
    rng = np.random.default_rng(12)
    I = 70000                                       # 17 bits of row + 17 bits of column
    rows = rng.integers(0, I, 3000).astype(np.int64)
    r = np.repeat(rows, rng.integers(1, 60, len(rows)))
    key = np.unique(np.concatenate([r * I + rng.integers(0, I, len(r)), [0, (I - 1) * I + I - 1]]))     # the first and the last key there are
    r, c = key // I, (key % I).astype(np.int32)
    rp = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=I), out=rp[1:])
    sim = rng.standard_normal(len(c))
    c2, s2 = ds.shuffle_rows(rng, rp, c, sim, "shuffle")
    idx, _ = checked_index(I, rp, c2, s2)
    assert np.array_equal(idx[0], c) and (r.max() << 17) > 2 ** 32


# ------------------------------------------------------------------------------------------------------- 2. the long row
BIG = (1 << 17) + 1


def _long_row_case():
    """I = 2^17 + 10 items; row 7 holds 2^17 + 1 columns: every item but 0, 1, 2, 7 itself, 70001 and the last four.  So column 3
    is its first entry, I - 5 its last, 1 is absent below, I - 2 absent above, 70001 absent between.  Rows 3 and I - 5 hold each
    other and 9; everything is stored shuffled."""
    c = getattr(_long_row_case, "c", None)
    if c is None:
        rng = np.random.default_rng(13)
        I = BIG + 9
        out = np.asarray([0, 1, 2, 7, 70001, I - 4, I - 3, I - 2, I - 1])
        cols = np.setdiff1d(np.arange(I), out)
        assert len(cols) == BIG and cols[0] == 3 and cols[-1] == I - 5
        vals = ds.eighths(rng, BIG) * rng.choice([-1.0, 1.0], BIG)
        rows = {7: list(zip(cols.tolist(), vals.tolist())), 3: [(I - 5, 0.875), (9, -0.125), (7, vals[0])],
                I - 5: [(3, 0.875), (9, 0.5), (7, vals[-1])], 9: [(3, -0.125), (I - 5, 0.5)]}
        rp, col, sim = ds.csr_of(rows, I)
        col, sim = ds.shuffle_rows(rng, rp, col, sim, "shuffle")
        idx, D = checked_index(I, rp, col, sim)
        c = _long_row_case.c = (I, rp, idx, D)
    return c


def test_a_row_of_2_to_the_17_plus_1_entries_and_lookups_at_its_ends():
    I, rp, idx, D = _long_row_case()
    assert rp[8] - rp[7] == BIG
    items = [7, 3, I - 5, 1, I - 2, 70001, 9, 65536, 4, I - 6, 2, I - 1]
    n_pool = len(items)
    plain = np.asarray([[9.0] + [5.0 - 0.125 * k for k in range(n_pool - 1)]])
    pool = (np.asarray([n_pool], np.int32), np.asarray([items], np.int32), plain, plain / 2)
    for w in (0.0, 0.5, 2.0, 1e6):
        for n_top in (2, n_pool):
            want = check_rerank(pool, 0, w, n_top, I, rp, idx, D)
            assert want[1][0, 0] == 7                       # the pick whose row is the long one
    # the penalties the statement finds for the ends: hits at the first and the last entry, none for the three absent columns
    want = ds.rerank(*pool, 0, 1e-300, n_pool, I, rp, idx[0], idx[1])
    pen = dict(zip(want[1][0].tolist(), want[5][0].tolist()))
    assert pen[3] == idx[1][rp[7]] > 0 and pen[1] == 0.0 and pen[I - 2] == 0.0 and pen[70001] == 0.0 and pen[I - 5] >= idx[1][rp[8] - 1] > 0
    # the same row searched from every wave of several blocks, in every pool position
    rng = np.random.default_rng(14)
    Q = 9
    item = np.stack([rng.permutation(items) for _ in range(Q)]).astype(np.int32)
    plain = np.sort(rng.integers(0, 30, (Q, n_pool)) / 8.0, axis=1)[:, ::-1].copy()
    check_rerank((np.full(Q, n_pool, np.int32), item, plain, plain / 2), 0, 2.0, 6, I, rp, idx, D)


# ------------------------------------------------------------------------------------------------------- 3. the re-ranking
def _small_model(family, seed=15, I=90):
    """a symmetric model of 90 items, about half of the pairs present; item 0 has an empty row and is in no row"""
    rng = np.random.default_rng(seed)
    values = dict(equal=lambda g, n: np.full(n, 0.5), eighths=ds.eighths, distinct=lambda g, n: g.random(n) + 1e-3,
                  subnormal=lambda g, n: g.integers(1, 50, n) * 5e-324)[family]
    rp, col, sim, _ = ds.random_sym_csr(rng, I, 0.5, values)
    keep = (np.repeat(np.arange(I), np.diff(rp)) != 0) & (col != 0)
    rows = np.repeat(np.arange(I), np.diff(rp))[keep]
    rp2 = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=I), out=rp2[1:])
    return I, rp2, col[keep], sim[keep]


def _designed_pools(rng, Q, n_pool, I, zero_scores=False):
    """Q pools of width n_pool: counts cycle through 0, 1, n_pool and a random one; query 3 repeats query 2; where the pool is wide
    enough the best-scored entries are an item beyond I, a negative one and item 0 (the empty row)"""
    scores = (lambda g, k: g.choice([0.0, -0.0], k)) if zero_scores else None
    cnt, item, plain, decay = ds.random_pools(rng, Q, n_pool, I, scores, min_cnt=1)
    for q in range(Q):
        cnt[q] = (0, 1, n_pool, cnt[q])[q % 4]
        k = int(cnt[q])
        item[q, :k] = rng.choice(np.arange(1, I), k, replace=False)
        item[q, k:], plain[q, k:], decay[q, k:] = -1, 0.0, 0.0
        if k >= 4:
            item[q, :3] = (I + 3, -2, 0)
    if Q > 3:
        cnt[3], item[3], plain[3], decay[3] = cnt[2], item[2], plain[2], decay[2]
    for q in range(Q):                              # the decayed scores: another draw, in its own descending order
        k = int(cnt[q])
        decay[q, :k] = plain[q, :k] if zero_scores else np.sort(rng.integers(0, 41, k) / 16.0)[::-1]
        decay[q, k:] = 0.0
    return cnt, item, plain, decay


@pytest.mark.parametrize("n_pool", [1, 2, 33, 63, 64])
def test_rerank_against_the_statement(n_pool):
    rng = np.random.default_rng(100 + n_pool)
    I, rp, col, sim = _small_model("eighths")       # many exact ties of obj
    idx, D = checked_index(I, rp, col, sim)
    tops = sorted({1, min(2, n_pool), max(n_pool - 1, 1), n_pool})
    changed = 0
    for Q in (1, 3, 4, 5):                          # the waves of a partial block, one block, two
        pool = _designed_pools(rng, Q, n_pool, I)
        for n_top in tops:
            for w, rank_by in ((0.0, 0), (0.5, 0), (2.0, 1), (1e6, 0), (1e-300, 1)):
                want = check_rerank(pool, rank_by, w, n_top, I, rp, idx, D)
                changed += want[7][0]
                if w == 0.0:                        # the pool's prefix, bit for bit
                    for q in range(Q):
                        n = min(pool[0][q], n_top)
                        assert want[0][q] == n and np.array_equal(want[1][q, :n], pool[1][q, :n]) and np.array_equal(want[4][q, :n], np.arange(n))
                        assert np.array_equal(ds.bits(want[2][q, :n]), ds.bits(pool[2][q, :n]))
    assert changed > 0 or n_pool < 33


@pytest.mark.parametrize("family", ["equal", "eighths", "distinct", "subnormal", "zero_scores"])
def test_rerank_over_the_families_of_values(family):
    rng = np.random.default_rng(7)
    I, rp, col, sim = _small_model("eighths" if family == "zero_scores" else family)
    idx, D = checked_index(I, rp, col, sim)
    pool = _designed_pools(rng, 1000, 64, I, zero_scores=family == "zero_scores")      # many blocks
    moved = 0
    for w, rank_by, n_top in ((0.5, 0, 10), (2.0, 1, 3), (1e6, 0, 5)):
        moved += check_rerank(pool, rank_by, w, n_top, I, rp, idx, D)[7][0]
    assert moved > 0
    rc, got = dev_rerank(pool, 0, 2.0, 10, I, D, stats=False)                          # without the stats: the same lists
    assert rc == 0
    ds.same(got[:7], ds.rerank(*pool, 0, 2.0, 10, I, rp, idx[0], idx[1])[:7])


def test_rerank_argument_errors_start_nothing():
    from xmap.engine import hipabi as abi
    I, rp, col, sim = _small_model("eighths")
    idx, D = checked_index(I, rp, col, sim)
    pool = _designed_pools(np.random.default_rng(1), 4, 8, I)
    for w, n_top in ((float("nan"), 4), (-1.0, 4), (float("inf"), 4), (0.5, 9)):        # the pool is 8 wide
        rc, got = dev_rerank(pool, 0, w, n_top, I, D)
        assert rc == abi.ERR_ARG
        assert all((x == -7).all() for x in got[:7])


def test_the_random_family_of_the_cpu_test():
    row_ptr, col, sim, dense, cnt, item, plain, decay = ds.random_family()
    idx, D = checked_index(400, row_ptr, col, sim)
    ils = {}
    for w in (0.0, 0.5, 2.0):
        want = check_rerank((cnt, item, plain, decay), 0, w, 10, 400, row_ptr, idx, D)
        ils[w] = want[6].mean()
        print("weight %g: %d of %d lists differ from the pool prefix, mean ILS %.4f" % (w, want[7][0], len(cnt), ils[w]))
        assert w == 0.0 or want[7][0] * 2 >= len(cnt)
    assert ils[2.0] < ils[0.0]


# ------------------------------------------------------------------------------------------------------- 4. Engine
def test_engine_div_index_and_diversify():
    from xmap.engine import device, synth
    row_ptr, col, sim, dense, cnt, item, plain, decay = ds.random_family(n_query=40)

    class S(object):
        pass
    S.row_ptr, S.col, S.sim = _dev(row_ptr), _dev(col), _dev(sim)
    r = synth.make_two_domain(7, 200, 50, 50)
    eng = device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs(), DEV))
    X = eng.div_index(S)
    idx = ds.div_index(row_ptr, col, sim)
    assert np.array_equal(X.dv_col.cpu().numpy()[:len(col)], idx[0]) and X.n_items == 400 and X.nnz == len(col)
    lists = (_dev(cnt), _dev(item), _dev(plain), _dev(decay), None)
    got = eng.diversify(lists, X, 2.0, 10, rank_by=1)
    want = ds.rerank(cnt, item, plain, decay, 1, 2.0, 10, 400, row_ptr, idx[0], idx[1])
    ds.same([x.cpu().numpy() for x in got[:7]], want[:7])
    assert got[7] == want[7]
    for bad in (dict(weight=-1.0), dict(weight=float("nan")), dict(n_top=65), dict(n_top=0)):
        with pytest.raises(ValueError):
            eng.diversify(lists, X, bad.get("weight", 1.0), bad.get("n_top", 10))


# ------------------------------------------------------------------------------------------------------- 5. the coarse call
def _diverse(ctx, source, queries, n_pool, n_top, rank_by, weight, filt, flags=0, n_w=66):
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(ALPHA, n_w)
    cnt, ids = np.full(Q, -7, np.int32), np.full((Q, n_top), -7, np.int32)
    plain, decay, pen = np.full((Q, n_top), -7.0), np.full((Q, n_top), -7.0), np.full((Q, n_top), -7.0)
    ils, stats = np.full(Q, -7.0), np.full(8, -7, np.int64)
    F, alive = filt.on_host()
    rc = ctx.lib.xmap_ctx_recommend_diverse(ctx.h, source, Q, _p(q, C.c_int32), n_pool, n_top, rank_by, flags, _p(w, C.c_double), n_w, weight,
                                            None if F is None else C.byref(F), _p(cnt, C.c_int32), _p(ids, C.c_int32), _p(plain, C.c_double),
                                            _p(decay, C.c_double), _p(pen, C.c_double), _p(ils, C.c_double), _p(stats, C.c_int64))
    del alive
    return rc, (cnt, ids, plain, decay, pen, ils, stats.tolist())


def _check_coarse(ctx, T, I, source, qs, n_pool, n_top, rank_by, weight, filt, idx):
    rc, pool = _coarse(ctx, "xmap_ctx_recommend_filtered", source, qs, n_pool, rank_by, 0, filt, alpha=ALPHA)
    assert rc == 0
    want = ds.rerank(pool[0], pool[1], pool[2], pool[3], rank_by, weight, n_top, I, T["row_ptr"], idx[0], idx[1])
    rc, got = _diverse(ctx, source, qs, n_pool, n_top, rank_by, weight, filt)
    assert rc == 0
    ds.same(got[:6], want[:4] + want[5:7])
    assert got[6][:6] == pool[4] and tuple(got[6][6:]) == want[7]
    return want


def test_the_coarse_call_over_both_sources_and_a_changed_model():
    from test_gpu_foldin import foldin
    from xmap.engine import synth
    seed, users = 5, 1500                           # the smallest case of test_gpu_topn.test_recommend_through_the_coarse_abi
    r = _few_times(synth.make_two_domain(seed, users, 300, 300, overlap=0.4))
    I, U = r.n_items, users
    rng = np.random.default_rng(seed)
    ctx = Ctx()
    try:
        ERR = ctx.abi.ERR_ARG
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        select(ctx, I, 10)
        B = 120
        lens = rng.integers(0, 30, B)
        f_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        f_item = rng.integers(0, I, f_ptr[-1]).astype(np.int32)
        foldin(ctx, f_ptr, f_item, (rng.integers(2, 21, len(f_item)) / 4.0).astype(np.float32), 1000 + rng.integers(0, 7, len(f_item)).astype(np.int64))
        idx = ds.div_index(T["row_ptr"], T["col"], T["sim"])
        assert idx[2] == 0
        moved = 0
        for source, qs in ((0, np.concatenate([rng.integers(0, U, 250), [-1, U + 5]])), (1, np.arange(-1, B + 1))):
            qs = np.ascontiguousarray(qs, np.int32)
            qs[-3] = qs[0]                           # a repeated query
            mask = rng.integers(0, 4, I) > 0
            exclude = [[int(x) for x in rng.integers(0, I, 5)] + [-1, I] for _ in qs]
            for n_pool, n_top, rank_by, weight, filt in ((40, 10, 0, 1.0, Filter(null=True)), (64, 10, 1, 4.0, Filter(allow=mask, exclude=exclude)),
                                                         (16, 16, 0, 0.0, Filter(min_score=3.0)), (8, 3, 0, 2.0, Filter())):
                want = _check_coarse(ctx, T, I, source, qs, n_pool, n_top, rank_by, weight, filt, idx)
                moved += want[7][0] if weight else 0
                assert weight or want[7][0] == 0
        assert moved > 0
        # host checks: XMAP_ERR_ARG, outputs untouched, the context as it was
        qs = np.arange(20, dtype=np.int32)
        for kw in (dict(weight=float("nan")), dict(weight=-1.0), dict(weight=float("inf")), dict(n_top=11, n_pool=10), dict(n_pool=65), dict(source=2)):
            a = dict(source=0, n_pool=10, n_top=5, weight=1.0)
            a.update(kw)
            rc, got = _diverse(ctx, a["source"], qs, a["n_pool"], a["n_top"], 0, a["weight"], Filter(null=True))
            assert rc == ERR, kw
            assert all((x == -7).all() for x in got[:6]) and got[6] == [-7] * 8
        # other neighbour lists: the index stays (it belongs to the matrix); the lists change, the statement follows
        select(ctx, I, 3)
        _check_coarse(ctx, T, I, 0, qs, 20, 5, 0, 2.0, Filter(null=True), idx)
        # a changed model: RecommenderSim again with another cap -> the context rebuilds its index
        T2 = rec_sim(ctx, I, U, len(rows["user"]), cap=2)
        assert T2["sim"].tobytes() != T["sim"].tobytes()
        rc, _ = _diverse(ctx, 0, qs, 20, 5, 0, 2.0, Filter(null=True))
        assert rc == ERR and b"have_nb" in ctx.lib.xmap_last_error()
        select(ctx, I, 10)
        idx2 = ds.div_index(T2["row_ptr"], T2["col"], T2["sim"])
        qs = np.ascontiguousarray(rng.integers(0, U, 200), np.int32)
        want = _check_coarse(ctx, T2, I, 0, qs, 40, 10, 0, 2.0, Filter(null=True), idx2)
        assert want[7][0] > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------- 6. the session
def test_session_diversify_equals_the_statement_on_the_plain_lists():
    """the construction of test_gpu_topn.test_session_recommend_topn_equals_the_statement_on_id_strings"""
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.engine import session, synth
    from xmap.utils.assist import baseliner_calculate_sim_pipeline, extender_pipeline, generator_pipeline
    r = synth.make_two_domain(9, 1200, 300, 300, overlap=0.4)
    t0 = datetime.datetime(2013, 3, 1)
    recs = [(u, [(i, ra, t0 + datetime.timedelta(days=(t * 7919) % 6)) for i, ra, t in prof]) for u, prof in r.train_records()]
    sc = SparkContext(conf=SparkConf())
    trainRDD = sc.parallelize(recs, 8).cache()
    tool = BaselinerSim("cosine", CAP)
    sim = baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
    ae = generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True)
    rng = np.random.default_rng(9)
    uids = [recs[int(x)][0] for x in rng.integers(0, len(recs), 120)] + ["A%013d" % (10 ** 9 + 1)]
    # the matrix the lists are re-ranked by: the RecommenderSim result of the same set-up (a pure function of the rows)
    st, _, _, S, _, _ = session._tail_setup(ae, CAP, 10, None, "test")
    iids, iidx, I = st.idt.iids, st.idt.iidx, len(st.idt.iids)
    row_ptr = S.row_ptr.cpu().numpy()
    idx = ds.div_index(row_ptr, S.col.cpu().numpy(), S.sim.cpu().numpy())
    assert idx[2] == 0

    def statement(pool_records, m, n, decay, w):
        Q = len(pool_records)
        cnt, item = np.zeros(Q, np.int32), np.full((Q, m), -1, np.int32)
        plain, dec = np.zeros((Q, m)), np.zeros((Q, m))
        for q, (_, lst) in enumerate(pool_records):
            cnt[q] = len(lst)
            for t, (iid, p, d) in enumerate(lst):
                item[q, t], plain[q, t], dec[q, t] = iidx[iid], p, d
        o = ds.rerank(cnt, item, plain, dec, 1 if decay else 0, w, n, I, row_ptr, idx[0], idx[1])
        lists = [(uid, [(iids[o[1][q, t]], float(o[2][q, t]), float(o[3][q, t])) for t in range(o[0][q])]) for q, (uid, _) in enumerate(pool_records)]
        return lists, o[6], o[7]

    moved = 0
    for n, m, decay, w in ((10, 40, False, 2.0), (5, None, True, 0.5), (3, 64, False, 1e6)):
        width = min(64, 4 * n) if m is None else m
        pool = session.recommend_topn(ae, uids, CAP, 10, ALPHA, width, decay=decay).collect()
        out = session.recommend_topn(ae, uids, CAP, 10, ALPHA, n, decay=decay, diversify=w, pool=m)
        lists, ils, stats = statement(pool, width, n, decay, w)
        assert out.collect() == lists
        assert np.array_equal(ds.bits(np.asarray(out.ils)), ds.bits(ils)) and out.div_stats == stats
        moved += stats[0]
    assert moved > 0 and out.collect()[-1] == (uids[-1], [])
    # diversify = 0: the records of the plain call, bit for bit, with their ILS
    plain = session.recommend_topn(ae, uids, CAP, 10, ALPHA, 10)
    zero = session.recommend_topn(ae, uids, CAP, 10, ALPHA, 10, diversify=0)
    assert zero.collect() == plain.collect() and zero.div_stats[0] == 0 and not hasattr(plain, "ils")
    assert np.array_equal(ds.bits(np.asarray(zero.ils)), ds.bits(statement(session.recommend_topn(ae, uids, CAP, 10, ALPHA, 40).collect(), 40, 10, False, 0.0)[1]))
    for bad in (dict(diversify=-1.0), dict(diversify=float("nan")), dict(diversify=1.0, pool=5), dict(diversify=1.0, pool=65), dict(pool=20)):
        with pytest.raises(ValueError):
            session.recommend_topn(ae, uids, CAP, 10, ALPHA, 10, **bad)
    # profiles folded in: the same statement over the pools of the plain fold-in call
    late = [("late-%d" % k, prof) for k, (_, prof) in enumerate(recs[:40])]
    pool = session.recommend_topn_profiles(ae, late, CAP, 10, ALPHA, 32).collect()
    out = session.recommend_topn_profiles(ae, late, CAP, 10, ALPHA, 8, diversify=2.0)
    lists, ils, stats = statement(pool, 32, 8, False, 2.0)
    assert out.collect() == lists and np.array_equal(ds.bits(np.asarray(out.ils)), ds.bits(ils)) and out.div_stats == stats
    assert any(lst for _, lst in lists)
    # the evaluation takes the re-ranked lists as they are: weight 0 scores what the plain call scores, and .ils is the mean over the
    # evaluated users
    test = [(u, [(i, ra) for i, ra, _ in prof[:3]]) for u, prof in recs[:200]]
    ev = session.evaluate_topn(ae, test, CAP, 10, ALPHA, 10, cutoffs=(5, 10), rel_min=1.0)
    ev0 = session.evaluate_topn(ae, test, CAP, 10, ALPHA, 10, cutoffs=(5, 10), rel_min=1.0, diversify=0)
    ev2 = session.evaluate_topn(ae, test, CAP, 10, ALPHA, 10, cutoffs=(5, 10), rel_min=1.0, diversify=2.0)
    assert ev.ils is None and ev0.at == ev.at and ev0.masks == ev.masks and ev0.at[10]["users"] > 0
    who = list(ev2.masks)
    per_user = session.recommend_topn(ae, who, CAP, 10, ALPHA, 10, diversify=2.0).ils
    assert np.isclose(ev2.ils, np.mean(per_user), rtol=1e-12) and ev0.ils >= 0.0
    print("NDCG@10 %.4f -> %.4f, mean ILS %.4f -> %.4f at weight 2" % (ev0.at[10]["ndcg"], ev2.at[10]["ndcg"], ev0.ils, ev2.ils))
