"""Fused lists on the device (xmap_fuse_rows, xmap_ctx_fuse, xmap_ctx_recommend_hybrid, Engine.fuse, session.recommend_hybrid /
fuse_lists, evaluate_topn(hybrid=...)) against tests/fuse_statement.py.  Everything is compared exactly, every query of every
call: integers with array_equal, doubles through their uint64 views (no NaN is ever returned as a score).  Outputs are pre-filled
with a sentinel.  The census of the designed inputs is tests/test_cpu_fuse_statement.py's."""
import ctypes as C

import numpy as np
import pytest

import fuse_statement as fs
from fuse_statement import MEAN, RRF, SUM

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


class DevLists(object):
    """the lists of a call on the device"""

    def __init__(self, lists):
        self.host = list(lists)
        self.t = [(_dev(L.cnt), _dev(L.item), None if L.score is None else _dev(L.score)) for L in lists]


def dev_fuse(D, n_ids, how, rrf_c, min_lists, n_top, max_records=0, stats=True, n_query=None, n_lists=None, widths=None, weights=None,
             null=()):
    """xmap_fuse_rows on device copies; outputs pre-filled with -7.  -> (rc, (cnt, id, score, lists, stats))"""
    import torch
    from xmap.engine import hipabi as abi
    n_q = len(D.host[0].cnt) if n_query is None else n_query
    rows = max(len(D.host[0].cnt), 1)
    arr = (abi.FuseList * max(len(D.t), 1))()
    for l, (L, t) in enumerate(zip(D.host, D.t)):
        p = [None if x is None else x.data_ptr() for x in t]
        for k, name in enumerate(("cnt", "item", "score")):
            if (l, name) in null:
                p[k] = None
        arr[l] = abi.FuseList(p[0], p[1], p[2], fs.width(L) if widths is None else widths[l], L.weight if weights is None else weights[l])
    o_cnt = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    o_id = torch.full((rows, n_top if 1 <= n_top <= 1024 else 1), -7, dtype=torch.int32, device=DEV)
    o_score = torch.full(tuple(o_id.shape), -7.0, dtype=torch.float64, device=DEV)
    o_lists = torch.full(tuple(o_id.shape), -7, dtype=torch.int32, device=DEV)
    h = (C.c_int64 * 5)(*([-7] * 5))
    rc = abi.lib.xmap_fuse_rows(_stream(), abi.i64(n_q), abi.i32(len(D.t) if n_lists is None else n_lists), C.cast(arr, C.c_void_p),
                                abi.i32(n_ids), abi.i32(how), C.c_double(rrf_c), abi.i32(min_lists), abi.i32(n_top), abi.i64(max_records),
                                abi.vp(None if "out_cnt" in null else o_cnt), abi.vp(o_id), abi.vp(o_score), abi.vp(o_lists),
                                h if stats else None)
    torch.cuda.synchronize()
    n_q = max(n_q, 0)
    return rc, (o_cnt.cpu().numpy()[:n_q], o_id.cpu().numpy()[:n_q], o_score.cpu().numpy()[:n_q], o_lists.cpu().numpy()[:n_q],
                [int(x) for x in h])


def same(got, want):
    assert np.array_equal(got[0], want[0]), "counts"
    assert np.array_equal(got[1], want[1]), "ids"
    assert not np.isnan(got[2]).any()
    assert np.array_equal(bits(got[2]), bits(want[2])), "score bits"
    assert np.array_equal(got[3], want[3]), "masks"
    assert list(got[4]) == list(want[4]), ("stats", got[4], want[4])


def as_bytes(got):
    return [np.ascontiguousarray(a).tobytes() for a in got[:4]] + [list(got[4])]


def untouched(got):
    return all((np.asarray(a) == -7).all() for a in got)


# ------------------------------------------------------------------------------------------------------- 1. the families
@pytest.fixture(scope="module")
def designed():
    """per family: the case, its lists on the device for each route, and the statement of every call (computed once)"""
    out = {}
    for f, make in fs.FAMILIES.items():
        c = make()
        want = {call: fs.fuse_statement(c.lists, c.n_ids, call[0], c.rrf_c, call[1], call[2]) for call in fs.CALLS[f]
                if not (call[0] != RRF and c.lists[0].score is None)}
        out[f] = (c, {"block": DevLists(c.lists), "sorted": DevLists(fs.on_sorted_route(c.lists))}, want)
    return out


@pytest.mark.parametrize("route", ["block", "sorted"])
@pytest.mark.parametrize("family", sorted(fs.FAMILIES))
def test_the_families_against_the_statement(designed, family, route):
    c, D, want = designed[family]
    assert (fs.total_width(D[route].host) <= fs.BLOCK_RECORDS) == (route == "block")
    assert want
    for (how, min_lists, n_top), w in want.items():
        rc, got = dev_fuse(D[route], c.n_ids, how, c.rrf_c, min_lists, n_top)
        assert rc == 0
        same(got, w)
        assert w[4][4] > 0 and w[4][0] > 0


@pytest.mark.parametrize("family", sorted(fs.FAMILIES))
def test_the_two_routes_return_the_same_bytes(designed, family):
    c, D, want = designed[family]
    for (how, min_lists, n_top) in want:
        a = dev_fuse(D["block"], c.n_ids, how, c.rrf_c, min_lists, n_top)
        b = dev_fuse(D["sorted"], c.n_ids, how, c.rrf_c, min_lists, n_top)
        assert a[0] == 0 and b[0] == 0 and as_bytes(a[1]) == as_bytes(b[1])


@pytest.mark.parametrize("family", ["generic", "shapes", "order"])
def test_chunking_leaves_every_byte(designed, family):
    c, D, want = designed[family]
    for call in list(want)[:2]:
        how, min_lists, n_top = call
        ref = None
        for max_records in (0, 1, 7, 64):
            rc, got = dev_fuse(D["sorted"], c.n_ids, how, c.rrf_c, min_lists, n_top, max_records=max_records)
            assert rc == 0
            same(got, want[call])
            ref = ref or as_bytes(got)
            assert as_bytes(got) == ref


def test_launch_ranges_leave_every_byte(designed, monkeypatch):
    """the count and expansion launches of the sorted-runs route go through for_pair_ranges: XMAP_PAIR_RANGE cuts them"""
    c, D, want = designed["generic"]
    call = list(want)[0]
    for span in ("1", "5", "64"):
        monkeypatch.setenv("XMAP_PAIR_RANGE", span)
        rc, got = dev_fuse(D["sorted"], c.n_ids, call[0], c.rrf_c, call[1], call[2])
        assert rc == 0
        same(got, want[call])


# ------------------------------------------------------------------------------------------------------- 2. identities
@pytest.mark.parametrize("route", ["block", "sorted"])
def test_appending_an_empty_list_and_swapping_two_lists(designed, route):
    c, D, want = designed["ties"]
    base = D[route]
    rc, a = dev_fuse(base, c.n_ids, RRF, c.rrf_c, 1, 63)
    more = DevLists(base.host + [fs.empty_list(len(c.lists[0].cnt), w=7, scored=False, weight=3.0)])
    rc2, b = dev_fuse(more, c.n_ids, RRF, c.rrf_c, 1, 63)
    assert rc == 0 and rc2 == 0 and as_bytes(a) == as_bytes(b)
    # two lists under RRF swapped: an addition of two terms commutes, so only the mask bits swap
    g = designed["generic"][0]
    two = [g.lists[0], g.lists[2]]
    if route == "sorted":
        x, y = DevLists(fs.on_sorted_route(two)), DevLists(fs.on_sorted_route(two[::-1]))
    else:
        x, y = DevLists(two), DevLists(two[::-1])
    rc, a = dev_fuse(x, g.n_ids, RRF, 60.0, 1, 100)
    rc2, b = dev_fuse(y, g.n_ids, RRF, 60.0, 1, 100)
    assert rc == 0 and rc2 == 0
    swap = np.array([0, 2, 1, 3], np.int32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(bits(a[2]), bits(b[2]))
    assert np.array_equal(swap[a[3]], b[3]) and set(np.unique(a[3])) == {0, 1, 2, 3} and a[4] == b[4]


def test_one_list_under_sum_returns_the_prefix_of_a_uknn_list():
    """weight 1.0, one record per id: fl(1.0 * s) = s and 0.0 + s = s, so the list comes back (finite scores, selection order)"""
    import torch
    from types import SimpleNamespace
    import uknn_statement as us
    import test_gpu_uknn as tu
    from xmap.engine import device
    c = us.family_case("integers")
    P, query, n_nb = c["P"], c["query"], max(us.N_NBS)
    D, L = tu.DevProfiles(P), tu.DevLists(c["lists"][n_nb], c["qavg"], c["avg"])
    rc, u = tu.dev_topn(D, D, L, query, 40)
    assert rc == 0 and u[0].max() > 5 and u[0].min() == 0      # lists longer and shorter than the n_top below, and empty ones
    eng = device.Engine(SimpleNamespace(device=torch.device(DEV), n_items=P.n_items))
    for n_top in (1, 5, 40):
        cnt, ids, score, mask, st = eng.fuse([(_dev(u[0]), _dev(u[1]), _dev(u[2]))], n_top, how="sum")
        k = np.minimum(u[0], n_top)
        assert np.array_equal(cnt.cpu().numpy(), k)
        assert np.array_equal(ids.cpu().numpy(), np.where(np.arange(n_top)[None, :] < k[:, None], u[1][:, :n_top], -1))
        assert np.array_equal(bits(score.cpu().numpy()), bits(np.where(np.arange(n_top)[None, :] < k[:, None], u[2][:, :n_top], 0.0)))
        assert st[0] == st[4] == int(u[0].sum())


# ------------------------------------------------------------------------------------------------------- 3. arguments
def test_bad_arguments_leave_guarded_outputs_untouched(designed):
    from xmap.engine import hipabi as abi
    c, D, _ = designed["generic"]
    d = D["block"]
    good = dict(how=RRF, rrf_c=60.0, min_lists=1, n_top=10)
    nan, inf = float("nan"), float("inf")
    bad = [(dict(n_lists=0), b"n_lists"), (dict(n_lists=17), b"n_lists"), (dict(widths=[63, 0, 65, 64, 33]), b"lists[1].width"),
           (dict(widths=[63, 64, 1025, 64, 33]), b"lists[2].width"), (dict(weights=[1.0, 1.0, 1.0, nan, 1.0]), b"lists[3].weight"),
           (dict(weights=[inf, 1.0, 1.0, 1.0, 1.0]), b"lists[0].weight"), (dict(rrf_c=-1.0), b"rrf_c"), (dict(rrf_c=nan), b"rrf_c"),
           (dict(rrf_c=inf), b"rrf_c"), (dict(how=3), b"how"), (dict(how=-1), b"how"), (dict(min_lists=0), b"min_lists"),
           (dict(min_lists=6), b"min_lists"), (dict(n_top=0), b"n_top"), (dict(n_top=1025), b"n_top"),
           (dict(how=SUM, null=[(4, "score")]), b"lists[4].score"), (dict(n_query=(1 << 28) + 1), b"n_query"), (dict(n_query=-1), b"n_query"),
           (dict(null=[(2, "cnt")]), b"lists[2].cnt"), (dict(null=[(0, "item")]), b"lists[0].item"), (dict(null=["out_cnt"]), b"out_cnt"),
           (dict(max_records=-1), b"max_records"), (dict(n_ids=-1), b"n_ids")]
    for kw, name in bad:
        a = dict(good)
        a.update(kw)
        n_ids = a.pop("n_ids", c.n_ids)
        rc, got = dev_fuse(d, n_ids, a.pop("how"), a.pop("rrf_c"), a.pop("min_lists"), a.pop("n_top"), **a)
        assert rc == abi.ERR_ARG, kw
        assert name in abi.lib.xmap_last_error(), (kw, abi.lib.xmap_last_error())
        assert untouched(got), kw
    # RRF without scores is fine
    rc, got = dev_fuse(d, c.n_ids, RRF, 60.0, 1, 10, null=[(l, "score") for l in range(5)])
    assert rc == 0
    same(got, fs.fuse_statement(c.lists, c.n_ids, RRF, 60.0, 1, 10))


def test_no_queries_and_no_ids(designed):
    c, D, _ = designed["generic"]
    for route in ("block", "sorted"):
        rc, got = dev_fuse(D[route], c.n_ids, RRF, 60.0, 1, 10, n_query=0)
        assert rc == 0 and got[4] == [0, 0, 0, 0, 0]
        rc, got = dev_fuse(D[route], 0, RRF, 60.0, 1, 10)
        assert rc == 0 and got[4] == [0, 0, 0, 0, 0] and (got[0] == 0).all() and (got[1] == -1).all() and (got[3] == 0).all()
        assert (bits(got[2]) == 0).all()


# ------------------------------------------------------------------------------------------------------- 4. Engine and coarse
def _ctx_fuse(ctx, lists, n_ids, how, rrf_c, min_lists, n_top, n_lists=None, null_ctx=False):
    from test_gpu_coarse_abi import _p
    abi = ctx.abi
    n_q = len(lists[0].cnt)
    arr = (abi.FuseList * len(lists))()
    keep = []
    for l, L in enumerate(lists):
        a = (np.ascontiguousarray(L.cnt, np.int32), np.ascontiguousarray(L.item, np.int32),
             None if L.score is None else np.ascontiguousarray(L.score, np.float64))
        keep.append(a)
        arr[l] = abi.FuseList(a[0].ctypes.data, a[1].ctypes.data, None if a[2] is None else a[2].ctypes.data, fs.width(L), L.weight)
    cnt, ids = np.full(n_q, -7, np.int32), np.full((n_q, max(min(n_top, 1024), 1)), -7, np.int32)
    score, mask, stats = np.full(ids.shape, -7.0), np.full(ids.shape, -7, np.int32), np.full(5, -7, np.int64)
    rc = ctx.lib.xmap_ctx_fuse(None if null_ctx else ctx.h, n_q, len(lists) if n_lists is None else n_lists, C.cast(arr, C.c_void_p), n_ids, how,
                               rrf_c, min_lists, n_top, _p(cnt, C.c_int32), _p(ids, C.c_int32), _p(score, C.c_double), _p(mask, C.c_int32),
                               _p(stats, C.c_int64))
    del keep
    return rc, (cnt, ids, score, mask, stats.tolist())


def test_the_coarse_fuse_equals_the_engine(designed):
    import torch
    from types import SimpleNamespace
    from test_gpu_coarse_abi import Ctx
    from xmap.engine import device
    eng = device.Engine(SimpleNamespace(device=torch.device(DEV), n_items=10))
    ctx = Ctx()
    try:
        for f in ("generic", "special", "shapes"):
            c, D, want = designed[f]
            for (how, min_lists, n_top), w in want.items():
                name = {RRF: "rrf", SUM: "sum", MEAN: "mean"}[how]
                e = eng.fuse(D["block"].t, n_top, how=name, weights=[L.weight for L in c.lists], rrf_c=c.rrf_c, min_lists=min_lists,
                             n_ids=c.n_ids)
                e = [x.cpu().numpy() for x in e[:4]] + [list(e[4])]
                same(e, w)
                rc, got = _ctx_fuse(ctx, c.lists, c.n_ids, how, c.rrf_c, min_lists, n_top)
                assert rc == 0 and as_bytes(got) == as_bytes(e)
        c = designed["generic"][0]
        ERR = ctx.abi.ERR_ARG
        for kw, name in ((dict(n_top=0), b"n_top"), (dict(min_lists=9), b"min_lists"), (dict(how=7), b"how"), (dict(rrf_c=-2.0), b"rrf_c"),
                         (dict(n_lists=0), b"n_lists")):
            a = dict(how=RRF, rrf_c=60.0, min_lists=1, n_top=5)
            a.update(kw)
            rc, got = _ctx_fuse(ctx, c.lists, c.n_ids, a.pop("how"), a.pop("rrf_c"), a.pop("min_lists"), a.pop("n_top"), **a)
            assert rc == ERR and name in ctx.lib.xmap_last_error() and untouched(got), kw
        rc, got = _ctx_fuse(ctx, c.lists, c.n_ids, RRF, 60.0, 1, 5, null_ctx=True)       # good arguments reach the context check
        assert rc == ERR and ctx.lib.xmap_last_error().endswith(b"bad argument: c") and untouched(got)
    finally:
        ctx.close()
    for kw in (dict(n_top=0), dict(n_top=1025), dict(how="borda"), dict(weights=[1.0]), dict(weights=[1.0, float("nan"), 1.0, 1.0, 1.0]),
               dict(rrf_c=-1.0), dict(min_lists=0), dict(min_lists=6), dict(n_ids=-1), dict(max_records=-1)):
        a = dict(n_top=5, n_ids=c.n_ids)
        a.update(kw)
        with pytest.raises(ValueError):
            eng.fuse(designed["generic"][1]["block"].t, a.pop("n_top"), **a)
    with pytest.raises(ValueError):
        eng.fuse([(t[0], t[1], None) for t in designed["generic"][1]["block"].t], 5, how="sum", n_ids=c.n_ids)
    with pytest.raises(ValueError):
        eng.fuse([designed["generic"][1]["block"].t[0]] * 17, 5, n_ids=c.n_ids)


def _ctx_hybrid(ctx, source, qs, n_top, pool_i, rank_by, tflags, w, pool_u, n_nb, pf, cap, mc, uflags, ms, wi, wu, how, rrf_c, min_lists, filt):
    from test_gpu_coarse_abi import _p
    q = np.ascontiguousarray(qs, np.int32)
    n_q, nt = len(q), max(min(n_top, 1024), 1)
    cnt, ids = np.full(n_q, -7, np.int32), np.full((n_q, nt), -7, np.int32)
    score, mask, stats = np.full((n_q, nt), -7.0), np.full((n_q, nt), -7, np.int32), np.full(17, -7, np.int64)
    F, alive = (None, None) if filt is None else filt.on_host()
    rc = ctx.lib.xmap_ctx_recommend_hybrid(ctx.h, source, n_q, _p(q, C.c_int32), n_top, pool_i, rank_by, tflags, _p(w, C.c_double),
                                           0 if w is None else len(w), pool_u, n_nb, pf, cap, mc, uflags, ms, wi, wu, how, rrf_c, min_lists,
                                           None if F is None else C.byref(F), _p(cnt, C.c_int32), _p(ids, C.c_int32), _p(score, C.c_double),
                                           _p(mask, C.c_int32), _p(stats, C.c_int64))
    del alive
    return rc, (cnt, ids, score, mask, stats.tolist())


def test_the_hybrid_call_equals_the_three_coarse_calls_composed():
    from test_gpu_coarse_abi import Ctx
    from test_gpu_filter import Filter, _coarse
    from test_gpu_foldin import foldin
    from test_gpu_tail import _GoldRatings, generate, rec_sim, select, wtab
    from test_gpu_uknn import _ctx_recommend
    r = _GoldRatings("small")
    I, U = r.n_items, len(r.user_ptr) - 1
    rng = np.random.RandomState(3)
    ctx = Ctx()
    try:
        ERR = ctx.abi.ERR_ARG
        rows = generate(ctx, r)
        rec_sim(ctx, I, U, len(rows["user"]))
        select(ctx, I, 10)
        B = 30
        lens = rng.randint(0, 25, B)
        f_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        f_item = rng.randint(0, I, f_ptr[-1]).astype(np.int32)
        foldin(ctx, f_ptr, f_item, (rng.randint(2, 21, len(f_item)) / 4.0).astype(np.float32), 1000 + rng.randint(0, 7, len(f_item)).astype(np.int64))
        mask = rng.rand(I) < 0.7
        w = wtab(1.5, 66)
        masks_seen = set()
        for source, qs in ((0, np.concatenate([np.arange(0, U, 3), [-1, U + 2, 0]])), (1, np.arange(-1, B + 1))):
            exclude = [[int(x) for x in rng.randint(0, I, 4)] for _ in qs]
            for (n_top, pool_i, rank_by, pool_u, n_nb, pf, cap, uflags, ms, wi, wu, how, rrf_c, min_lists, filt) in (
                    (10, 64, 0, 64, 20, 4, 3, 0, 1, 1.0, 1.0, RRF, 60.0, 1, None),
                    (300, 30, 1, 1024, 12, 4, 1, 1, 1, 0.5, 2.0, SUM, 0.0, 1, Filter(allow=mask, exclude=exclude, min_score=1.0)),
                    (7, 64, 0, 100, 20, 0, 2, 1, 2, 1.0, 3.0, MEAN, 0.0, 2, Filter(null=True))):
                rc, got = _ctx_hybrid(ctx, source, qs, n_top, pool_i, rank_by, 0, w, pool_u, n_nb, pf, cap, 1, uflags, ms, wi, wu, how, rrf_c,
                                      min_lists, filt)
                assert rc == 0, ctx.lib.xmap_last_error()
                rc, a = _coarse(ctx, "xmap_ctx_recommend_filtered", source, qs, pool_i, rank_by, 0, filt or Filter(null=True), alpha=1.5)
                assert rc == 0
                rc, b = _ctx_recommend(ctx, source, qs, n_nb, pool_u, pf, cap, 1, uflags, ms, filt)
                assert rc == 0
                lists = [fs.FuseIn(a[0], a[1], a[3] if rank_by else a[2], wi), fs.FuseIn(b[0], b[1], b[2], wu)]
                rc, f = _ctx_fuse(ctx, lists, I, how, rrf_c, min_lists, n_top)
                assert rc == 0
                assert as_bytes(got)[:4] == as_bytes(f)[:4] and got[4] == a[4] + b[4] + f[4]
                same(f, fs.fuse_statement(lists, I, how, rrf_c, min_lists, n_top))
                assert got[0].sum() > 0
                masks_seen |= set(np.unique(got[3]).tolist())
        assert masks_seen >= {0, 1, 2, 3}
        # no queries, on both sources: the three calls return their stats zeroed and start nothing; the composition still holds
        for source in (0, 1):
            none = np.arange(0)
            rc, got = _ctx_hybrid(ctx, source, none, 4, 8, 0, 0, w, 8, 5, 0, 1, 1, 0, 1, 1.0, 1.0, RRF, 60.0, 1, None)
            assert rc == 0 and got[4] == [0] * 17, ctx.lib.xmap_last_error()
            rc, a = _coarse(ctx, "xmap_ctx_recommend_filtered", source, none, 8, 0, 0, Filter(null=True), alpha=1.5)
            assert rc == 0 and a[4] == [0] * 6, ctx.lib.xmap_last_error()
            rc, b = _ctx_recommend(ctx, source, none, 5, 8, 0, 1, 1, 0, 1, None)
            assert rc == 0 and b[4] == [0] * 6 and got[4] == a[4] + b[4] + [0] * 5, ctx.lib.xmap_last_error()
        # every host check: XMAP_ERR_ARG naming its argument, the outputs keep every byte
        good = dict(source=0, n_top=5, pool_i=10, rank_by=0, tflags=0, w=w, pool_u=10, n_nb=5, pf=0, cap=1, mc=1, uflags=0, ms=1, wi=1.0, wu=1.0,
                    how=RRF, rrf_c=60.0, min_lists=1, filt=None)
        nan = float("nan")
        for kw, name in ((dict(n_top=0), b"n_top"), (dict(n_top=1025), b"n_top"), (dict(pool_i=0), b"n_pool_items"), (dict(pool_i=65), b"n_pool_items"),
                         (dict(rank_by=2), b"rank_by"), (dict(tflags=2), b"topn_flags"), (dict(w=None), b"wtab"), (dict(pool_u=0), b"n_pool_users"),
                         (dict(pool_u=1025), b"n_pool_users"), (dict(n_nb=0), b"n_nb"), (dict(n_nb=1025), b"n_nb"), (dict(pf=1), b"peer_flags"),
                         (dict(cap=0), b"cap"), (dict(mc=0), b"min_common"), (dict(uflags=4), b"uknn_flags"), (dict(ms=0), b"min_support"),
                         (dict(wi=nan), b"w_items"), (dict(wu=float("inf")), b"w_users"), (dict(how=3), b"how"), (dict(rrf_c=-1.0), b"rrf_c"),
                         (dict(rrf_c=nan), b"rrf_c"), (dict(min_lists=0), b"min_lists"), (dict(min_lists=3), b"min_lists"),
                         (dict(source=2), b"source"), (dict(filt=Filter(min_score=nan)), b"min_score")):
            a = dict(good)
            a.update(kw)
            rc, got = _ctx_hybrid(ctx, a["source"], np.arange(5), a["n_top"], a["pool_i"], a["rank_by"], a["tflags"], a["w"], a["pool_u"], a["n_nb"],
                                  a["pf"], a["cap"], a["mc"], a["uflags"], a["ms"], a["wi"], a["wu"], a["how"], a["rrf_c"], a["min_lists"], a["filt"])
            assert rc == ERR and name in ctx.lib.xmap_last_error(), (kw, ctx.lib.xmap_last_error())
            assert untouched(got), kw
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------- 5. the session
@pytest.fixture(scope="module")
def small():
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from golden_util import CAP, Golden
    from test_gpu_api import records
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.utils.assist import baseliner_calculate_sim_pipeline, extender_pipeline, generator_pipeline
    recs = records(Golden("small"))
    sc = SparkContext(conf=SparkConf())
    trainRDD = sc.parallelize(recs, 4).cache()
    tool = BaselinerSim("cosine", CAP)
    sim = baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
    return generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True), recs, CAP


def _as_list(result, index, k, width, weight):
    """a collected session result [(label, [(iid, score, ...)*])*] as a FuseIn over the id numbering `index`"""
    rows = result.collect()
    cnt, item, score = np.zeros(len(rows), np.int32), np.full((len(rows), width), -1, np.int32), np.zeros((len(rows), width))
    for q, (_, lst) in enumerate(rows):
        cnt[q] = len(lst)
        for t, e in enumerate(lst):
            item[q, t], score[q, t] = index[e[0]], e[k]
    return fs.FuseIn(cnt, item, score, weight)


WHICH = [(), ("item",), ("user",), ("item", "user")]


def _expect(labels, ids, want, which=lambda m: WHICH[m]):
    return [(u, [(ids[want[1][q, t]], float(want[2][q, t]), which(int(want[3][q, t]))) for t in range(want[0][q])]) for q, u in enumerate(labels)]


def test_session_hybrid_against_the_statement_over_the_two_sessions_own_lists(small):
    from xmap.engine import session
    ae, recs, CAP = small
    idt = ae.state.idt
    iids, I = idt.iids, len(idt.iids)
    users = [idt.uids[k] for k in range(0, len(idt.uids), 2)] + ["nobody-knows-me", idt.uids[0]]
    keep, alpha = 10, 0.3
    excl = {users[0]: list(iids[:5]), users[3]: list(iids[:20])}
    seen = set()
    for decay, how, weights, min_lists, n, kw in ((False, "rrf", (1.0, 1.0), 1, 7, {}), (True, "sum", (0.5, 2.0), 2, 100, dict(exclude=excl)),
                                                  (False, "mean", (1.0, 3.0), 1, 10, dict(own_mean=True, keep_held=True, min_support=2))):
        tk = {k: v for k, v in kw.items() if k in ("exclude", "keep_held")}
        uk = {k: v for k, v in kw.items() if k in ("exclude", "keep_held", "own_mean", "min_support")}
        a = session.recommend_topn(ae, users, CAP, keep, alpha, 64, decay=decay, **tk)
        b = session.recommend_user_knn(ae, users, 12, 64, cap=3, **uk)
        lists = [_as_list(a, idt.iidx, 2 if decay else 1, 64, weights[0]), _as_list(b, idt.iidx, 1, 64, weights[1])]
        want = fs.fuse_statement(lists, I, {"rrf": RRF, "sum": SUM, "mean": MEAN}[how], 60.0, min_lists, n)
        out = session.recommend_hybrid(ae, users, CAP, keep, alpha, n, 12, decay=decay, peer_cap=3, how=how, weights=weights,
                                       min_lists=min_lists, **kw)
        assert out.collect() == _expect(users, iids, want)
        assert list(out.stats[2]) == want[4] and want[4][0] > 0 and list(out.stats[1]) == list(b.stats)
        seen |= {w for _, lst in out.collect() for e in lst for w in [e[2]]}
        # the late fusion of the two collected results: the same lists under fuse_lists' own (sorted) numbering of the iids
        ids = sorted({e[0] for r in (a, b) for _, lst in r.collect() for e in lst})
        index = {x: k for k, x in enumerate(ids)}
        late = [_as_list(a, index, 2 if decay else 1, 64, weights[0]), _as_list(b, index, 1, 64, weights[1])]
        w2 = fs.fuse_statement(late, len(ids), {"rrf": RRF, "sum": SUM, "mean": MEAN}[how], 60.0, min_lists, n)
        got = session.fuse_lists([a, b], n, how=how, weights=weights, min_lists=min_lists, score_index=(2 if decay else 1, 1))
        assert got.collect() == _expect(users, ids, w2, lambda m: tuple(l for l in (0, 1) if (m >> l) & 1)) and list(got.stats) == w2[4]
    assert seen == {("item",), ("user",), ("item", "user")}
    assert out.collect()[-2] == ("nobody-knows-me", [])
    # profiles that are not rows of the train set
    profs = [("new-" + u, list(p)) for u, p in recs[:40:2]]
    a = session.recommend_topn_profiles(ae, profs, CAP, keep, alpha, 30)
    b = session.recommend_user_knn_profiles(ae, profs, 12, 50, cap=3)
    lists = [_as_list(a, idt.iidx, 1, 30, 1.0), _as_list(b, idt.iidx, 1, 50, 1.5)]
    want = fs.fuse_statement(lists, I, RRF, 10.0, 1, 20)
    out = session.recommend_hybrid_profiles(ae, profs, CAP, keep, alpha, 20, 12, peer_cap=3, weights=(1.0, 1.5), rrf_c=10.0, pool_items=30,
                                            pool_users=50)
    assert out.collect() == _expect([u for u, _ in profs], iids, want) and out.unknown_items == 0 and want[4][0] > 0
    for bad in (dict(how="borda"), dict(weights=(1.0,)), dict(pool_items=65), dict(pool_users=0), dict(min_lists=3), dict(rrf_c=-1.0)):
        with pytest.raises(ValueError):
            session.recommend_hybrid(ae, users, CAP, keep, alpha, 7, 12, **bad)


def test_evaluate_topn_scores_the_hybrid_lists(small):
    import torch
    from types import SimpleNamespace
    from xmap.engine import device, session
    ae, recs, CAP = small
    idt = ae.state.idt
    U, I = len(idt.uids), len(idt.iids)
    keep, alpha, n, cuts, rel_min = 10, 0.3, 10, (1, 5, 10), 3.0
    test = [(u, [(p[0], float(p[1])) for p in pairs[:4]]) for u, pairs in recs[:80]]
    hyb = dict(n_nb=12, peer_cap=3, how="rrf", weights=(1.0, 2.0))
    ev = session.evaluate_topn(ae, test, CAP, keep, alpha, n, cutoffs=cuts, rel_min=rel_min, keep_held=True, hybrid=hyb)
    plain = session.evaluate_topn(ae, test, CAP, keep, alpha, n, cutoffs=cuts, rel_min=rel_min, keep_held=True)
    # the same through Engine.topn_eval over the lists recommend_hybrid returns for the evaluated users
    uidx = session._user_index(idt)
    tu = np.asarray([uidx[u] for u, pairs in test for _ in pairs], np.int32)
    ti = np.asarray([idt.iidx[p[0]] for _, pairs in test for p in pairs], np.int32)
    tr = np.asarray([p[1] for _, pairs in test for p in pairs], np.float64)
    eng = device.Engine(SimpleNamespace(device=torch.device(DEV), n_items=I))
    d = [_dev(x) for x in (tu, ti, tr)]
    n_rel, users, counts = eng.eval_users(d[0], d[1], d[2], rel_min, U, I)
    labels = [idt.uids[u] for u in users.cpu().tolist()]
    assert len(labels) > 30 and set(ev.masks) == set(labels)
    out = session.recommend_hybrid(ae, labels, CAP, keep, alpha, n, 12, keep_held=True, **{k: v for k, v in hyb.items() if k != "n_nb"})
    L = _as_list(out, idt.iidx, 1, n, 1.0)
    mask, _, agg, cover = eng.topn_eval(d[0], d[1], d[2], rel_min, n_rel, users, _dev(L.cnt), _dev(L.item), list(cuts), I)
    assert ev.masks == {u: int(b) & 0xffffffffffffffff for u, b in zip(labels, mask.cpu().tolist())}
    agg, cover = agg.cpu().numpy(), cover.cpu().numpy()
    for k, c in enumerate(cuts):
        m = float(agg[k, 0])
        assert ev.at[c] == dict(users=int(m), hit_rate=float(agg[k, 1]) / m, precision=float(agg[k, 3]) / m, recall=float(agg[k, 4]) / m,
                                ndcg=float(agg[k, 5]) / m, map=float(agg[k, 6]) / m, mrr=float(agg[k, 7]) / m, coverage=int(cover[k]))
    assert any(ev.masks.values()) and ev.masks != plain.masks and ev.hybrid_stats[2][0] > 0 and not hasattr(plain, "hybrid_stats")
    for bad in (dict(diversify=0.5), dict(fill="count"), dict(pool=20)):
        with pytest.raises(ValueError):
            session.evaluate_topn(ae, test, CAP, keep, alpha, n, cutoffs=cuts, hybrid=hyb, **bad)
    with pytest.raises(ValueError):
        session.evaluate_topn(ae, test, CAP, keep, alpha, n, cutoffs=cuts, hybrid=dict(peer_cap=3))
    with pytest.raises(ValueError):
        session.evaluate_topn(ae, test, CAP, keep, alpha, n, cutoffs=cuts, hybrid=dict(n_nb=12, borda=True))
