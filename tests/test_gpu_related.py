"""Related items for a basket on the device (xmap_related_rows, xmap_ctx_related, Engine.related, session.related_items) against
tests/related_statement.py.  Everything is compared exactly, every query of every call: integers with array_equal, doubles
through their uint64 views (no NaN is ever returned as a score).  Outputs are pre-filled with a sentinel.  The census of the
designed inputs is tests/test_cpu_related_statement.py's."""
import ctypes as C

import numpy as np
import pytest

import related_statement as rs
from related_statement import KEEP_MEMBERS, MAX, MEAN, SUM

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


class DevMatrix(object):
    def __init__(self, M):
        self.M, self.row_ptr, self.col, self.sim = M, _dev(M.row_ptr), _dev(M.col), _dev(M.sim)


def dev_related(D, b_ptr, b_item, n_top, how=SUM, flags=0, min_support=1, weights=None, allow=None, exclude=None, min_score=None,
                null_filter=False, max_records=0, stats=True):
    """xmap_related_rows on device copies; outputs pre-filled with -7.  -> (rc, (cnt, item, score, support, stats))"""
    import torch
    from xmap.engine import filters, hipabi as abi
    M = D.M
    b_ptr = np.ascontiguousarray(b_ptr, np.int64)
    n_q = len(b_ptr) - 1
    d_ptr, d_item = _dev(b_ptr), _dev(np.ascontiguousarray(b_item, np.int32))
    d_w = None if weights is None else _dev(np.ascontiguousarray(weights, np.float64))
    o_cnt = torch.full((max(n_q, 1),), -7, dtype=torch.int32, device=DEV)
    o_item = torch.full((max(n_q, 1), n_top), -7, dtype=torch.int32, device=DEV)
    o_score = torch.full((max(n_q, 1), n_top), -7.0, dtype=torch.float64, device=DEV)
    o_support = torch.full((max(n_q, 1), n_top), -7, dtype=torch.int32, device=DEV)
    F = alive = None
    if null_filter or allow is not None or exclude is not None or min_score is not None:
        words = None if allow is None else _dev(filters.pack_mask(np.asarray(allow, bool), M.n_items).view(np.int32))
        ptr = ids = None
        if exclude is not None:
            ptr, ids = [_dev(a) for a in (exclude if isinstance(exclude, tuple) else filters.exclusion_csr(exclude))]
        alive = (words, ptr, ids)
        F = abi.rec_filter(words, ptr, ids, min_score)
    h = (C.c_int64 * 6)(*([-7] * 6))
    rc = abi.lib.xmap_related_rows(_stream(), abi.i64(n_q), abi.vp(d_ptr), abi.vp(d_item), abi.vp(d_w), abi.i32(M.n_items), abi.vp(D.row_ptr),
                                   abi.vp(D.col), abi.vp(D.sim), abi.i32(how), abi.i32(flags), abi.i32(n_top), abi.i32(min_support),
                                   abi.i64(max_records), abi.vp(o_cnt), abi.vp(o_item), abi.vp(o_score), abi.vp(o_support),
                                   None if F is None else C.byref(F), h if stats else None)
    torch.cuda.synchronize()
    del alive
    return rc, (o_cnt.cpu().numpy()[:n_q], o_item.cpu().numpy()[:n_q], o_score.cpu().numpy()[:n_q], o_support.cpu().numpy()[:n_q],
                [int(x) for x in h])


def same(got, want):
    assert np.array_equal(got[0], want[0]), "counts"
    assert np.array_equal(got[1], want[1]), "items"
    assert not np.isnan(got[2]).any()
    assert np.array_equal(bits(got[2]), bits(want[2])), "score bits"
    assert np.array_equal(got[3], want[3]), "support"
    assert list(got[4]) == list(want[4]), ("stats", got[4], want[4])


def as_bytes(got):
    return [np.ascontiguousarray(a).tobytes() for a in got[:4]] + [list(got[4])]


def untouched(got):
    return all((np.asarray(a) == -7).all() for a in got)


# ------------------------------------------------------------------------------------------------------- 1. the families
@pytest.fixture(scope="module")
def designed():
    b_ptr, b_item, weights = rs.baskets()
    fam = {}
    for f in rs.FAMILIES:
        M = rs.design(f)
        fam[f] = (DevMatrix(M), rs.raw_records(M, b_ptr, b_item), rs.raw_records(M, b_ptr, b_item, weights))
    return b_ptr, b_item, weights, fam


N_TOPS, SUPPORTS = [1, 7, 256, 1024], [1, 2, 65]            # 65: the size of the largest baskets


@pytest.mark.parametrize("family", rs.FAMILIES)
def test_the_families_against_the_statement(designed, family):
    """every how, with and without weights, members kept and not: twelve calls, under which n_top (k % 4) and min_support (k % 3) run
    through all their twelve pairs, and every how (four consecutive k) meets every value of both"""
    b_ptr, b_item, weights, fam = designed
    D, raw, raw_w = fam[family]
    k, used = 0, set()
    for how in (SUM, MEAN, MAX):
        for w in (None, weights):
            for flags in (0, KEEP_MEMBERS):
                n_top, ms = N_TOPS[k % 4], SUPPORTS[k % 3]
                k += 1
                used.add((how, n_top))
                used.add((how, ms))
                want = rs.related_statement(D.M, b_ptr, b_item, n_top, how, flags, ms, w, raw=raw if w is None else raw_w)
                rc, got = dev_related(D, b_ptr, b_item, n_top, how, flags, ms, w)
                assert rc == 0
                same(got, want)
                assert want[4][0] > 3000 and want[4][5] > 20000
                if ms == 65:                    # the threshold drops nearly every run, and still leaves a list: the basket of 65
                    assert want[4][1] > 10000 and want[0][9] > 0 and want[0].sum() == want[0][9] and (want[3][9, :want[0][9]] >= 65).all()
    assert used == {(how, v) for how in (SUM, MEAN, MAX) for v in N_TOPS + SUPPORTS}


@pytest.mark.parametrize("family", ["generic", "ties"])
def test_chunking_leaves_every_byte(designed, family):
    b_ptr, b_item, weights, fam = designed
    D = fam[family][0]
    for how, n_top in ((SUM, 7), (MAX, 300)):
        ref = None
        for max_records in (0, 1, 3, 64, 1000):
            rc, got = dev_related(D, b_ptr, b_item, n_top, how, 0, 2, weights, max_records=max_records)
            assert rc == 0
            ref = as_bytes(got) if ref is None else ref
            assert as_bytes(got) == ref, max_records
        assert got[4][4] > 2048


def test_launch_ranges_leave_every_byte(designed, monkeypatch):
    """the wave-per-position passes launched in ranges of 5 positions"""
    b_ptr, b_item, weights, fam = designed
    D = fam["generic"][0]
    rc, ref = dev_related(D, b_ptr, b_item, 7, MEAN, 0, 1, weights)
    monkeypatch.setenv("XMAP_PAIR_RANGE", "5")
    rc2, got = dev_related(D, b_ptr, b_item, 7, MEAN, 0, 1, weights, max_records=1000)
    assert rc == 0 and rc2 == 0 and as_bytes(got) == as_bytes(ref)


# ------------------------------------------------------------------------------------------------------- 2. the rules
@pytest.mark.parametrize("family", ["dyadic", "special"])
def test_rules_mask_exclusions_floor(designed, family):
    b_ptr, b_item, weights, fam = designed
    D, raw, _ = fam[family]
    allow, exclude, floor = rs.rules(b_ptr)
    rc, plain = dev_related(D, b_ptr, b_item, 7, SUM, 0, 2)
    assert rc == 0
    for kw in (dict(allow=allow), dict(exclude=exclude), dict(min_score=floor), dict(allow=allow, exclude=exclude, min_score=floor)):
        want = rs.related_statement(D.M, b_ptr, b_item, 7, SUM, 0, 2, raw=raw, **kw)
        rc, got = dev_related(D, b_ptr, b_item, 7, SUM, 0, 2, **kw)
        assert rc == 0
        same(got, want)
        assert plain[4][0] - got[4][0] == want[5]["mask"] + want[5]["excluded"]
    assert want[5]["mask"] > 0 and want[5]["excluded"] > 0 and want[4][3] > 0 and want[4][1] > 0
    # no filter at all, and a filter that asks for nothing: the unfiltered bytes
    for kw in (dict(null_filter=True), dict(min_score=-np.inf), dict(stats=False)):
        rc, got = dev_related(D, b_ptr, b_item, 7, SUM, 0, 2, **kw)
        assert rc == 0 and as_bytes(got)[:4] == as_bytes(plain)[:4] and (not kw.get("stats", True) or got[4] == plain[4])
    # an exclusion table that lists nothing
    rc, got = dev_related(D, b_ptr, b_item, 7, SUM, 0, 2, exclude=(np.zeros(len(b_ptr), np.int64), np.zeros(0, np.int32)))
    assert rc == 0 and as_bytes(got) == as_bytes(plain)


# ------------------------------------------------------------------------------------------------------- 3. an existing kernel
@pytest.mark.parametrize("keep", [1, 10, 64])
def test_one_member_equals_the_selection_kernel(designed, keep):
    """non-negative similarities, one member, no weights, the member left out: the list is xmap_rec_select's row of the member,
    columns and sims bit for bit -- for the rows that hold neither their own index (rule 2 takes it out here) nor a column twice
    (two records of one item here, two entries there)"""
    import torch
    from xmap.engine import hipabi as abi
    D = designed[3]["ties"][0]
    M = D.M
    I = M.n_items
    cnt = torch.full((I,), -7, dtype=torch.int32, device=DEV)
    col = torch.full((I, keep), -7, dtype=torch.int32, device=DEV)
    sim, ls = [torch.full((I, keep), -7.0, dtype=torch.float64, device=DEV) for _ in range(2)]
    zeros = torch.zeros(max(len(M.col), 1), dtype=torch.float64, device=DEV)
    abi.check(abi.lib.xmap_rec_select(_stream(), abi.i32(I), abi.vp(D.row_ptr), abi.vp(D.col), abi.vp(D.sim), abi.vp(zeros), abi.i32(keep),
                                      abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ls)))
    torch.cuda.synchronize()
    cnt, col, sim = cnt.cpu().numpy(), col.cpu().numpy(), sim.cpu().numpy()
    plain = rs.plain_rows(M)
    assert len(plain) > 200
    rc, got = dev_related(D, np.arange(len(plain) + 1), plain, keep)
    assert rc == 0
    for q, i in enumerate(plain):
        n = cnt[i]
        assert got[0][q] == n == min(keep, M.row_ptr[i + 1] - M.row_ptr[i])
        assert np.array_equal(got[1][q, :n], col[i, :n]) and np.array_equal(bits(got[2][q, :n]), bits(sim[i, :n])), i


# ------------------------------------------------------------------------------------------------------- 4. bad input, empty input
def test_bad_tables_are_errors_before_anything_is_indexed(designed):
    """argument checks the library makes on the device before it indexes through a table: XMAP_ERR_ARG, the position named, the
    outputs at their sentinels"""
    from xmap.engine import hipabi as abi
    b_ptr, b_item, _, fam = designed
    D = fam["dyadic"][0]
    n_q = len(b_ptr) - 1
    bad = b_ptr.copy()
    bad[0] = 1
    rc, got = dev_related(D, bad, b_item, 5)
    assert rc == abi.ERR_ARG and b"the first at b_ptr[0]" in abi.lib.xmap_last_error() and untouched(got)
    bad = b_ptr.copy()
    bad[9] = bad[8] - 1
    bad[20] = bad[19] - 1
    rc, got = dev_related(D, bad, b_item, 5)
    assert rc == abi.ERR_ARG and b"b_ptr has 2 bad entries, the first at b_ptr[9]" in abi.lib.xmap_last_error() and untouched(got)
    ex_ptr = np.arange(n_q + 1, dtype=np.int64)
    ex_ptr[4] = 1
    rc, got = dev_related(D, b_ptr, b_item, 5, exclude=(ex_ptr, np.zeros(n_q, np.int32)))
    assert rc == abi.ERR_ARG and b"the first at ex_ptr[4]" in abi.lib.xmap_last_error() and untouched(got)
    rc, got = dev_related(D, b_ptr, b_item, 5, exclude=(ex_ptr + 1, np.zeros(n_q + 1, np.int32)))
    assert rc == abi.ERR_ARG and b"the first at ex_ptr[0]" in abi.lib.xmap_last_error() and untouched(got)
    # the host checks of the fine call
    for kw, name in ((dict(n_top=0), b"n_top"), (dict(n_top=1025), b"n_top"), (dict(how=3), b"how"), (dict(how=-1), b"how"),
                     (dict(flags=2), b"flags"), (dict(min_support=0), b"min_support"), (dict(min_score=float("nan")), b"min_score"),
                     (dict(max_records=-1), b"max_records")):
        if kw.get("n_top") == 0:                # (an output of zero columns cannot be shaped: one column)
            rc, got = _n_top_zero(D, b_ptr, b_item)
        else:
            a = dict(n_top=5)
            a.update(kw)
            rc, got = dev_related(D, b_ptr, b_item, a.pop("n_top"), **a)
        assert rc == abi.ERR_ARG and name in abi.lib.xmap_last_error() and untouched(got), kw


def _n_top_zero(D, b_ptr, b_item):
    import torch
    from xmap.engine import hipabi as abi
    n_q = len(b_ptr) - 1
    outs = [torch.full((n_q,), -7, dtype=torch.int32, device=DEV), torch.full((n_q,), -7, dtype=torch.int32, device=DEV),
            torch.full((n_q,), -7.0, dtype=torch.float64, device=DEV), torch.full((n_q,), -7, dtype=torch.int32, device=DEV)]
    rc = abi.lib.xmap_related_rows(_stream(), abi.i64(n_q), abi.vp(_dev(b_ptr)), abi.vp(_dev(b_item)), None, abi.i32(D.M.n_items),
                                   abi.vp(D.row_ptr), abi.vp(D.col), abi.vp(D.sim), abi.i32(0), abi.i32(0), abi.i32(0), abi.i32(1), abi.i64(0),
                                   *([abi.vp(o) for o in outs] + [None, None]))
    torch.cuda.synchronize()
    return rc, [o.cpu().numpy() for o in outs]


def test_empty_cases(designed):
    b_ptr, b_item, weights, fam = designed
    D = fam["dyadic"][0]
    rc, got = dev_related(D, [0], [], 5)
    assert rc == 0 and got[4] == [0] * 6
    for ptr, item, DD in (([0, 0, 0, 0], [], D), ([0, 1, 3], [-1, D.M.n_items, D.M.n_items + 1], D), ([0, 1, 1, 3], [8, 8, 16], D),
                          ([0, 2, 3], [1, 2, 3], DevMatrix(rs.Matrix(np.zeros(rs.N_ROWS + 1, np.int64), [], []))),
                          ([0, 2, 3], [1, 2, 3], DevMatrix(rs.Matrix([0], [], [])))):
        n_q = len(ptr) - 1
        rc, got = dev_related(DD, ptr, item, 5, MEAN, 0, 1, None if not len(item) else np.ones(len(item)))
        assert rc == 0
        assert not got[0].any() and (got[1] == -1).all() and not bits(got[2]).any() and not got[3].any() and got[4] == [0] * 6
        assert got[0].shape == (n_q,) and got[1].shape == (n_q, 5)


# ------------------------------------------------------------------------------------------------------- 5. the coarse call
def _ctx_related(ctx, b_ptr, b_item, weights, how, flags, n_top, min_support=1, max_records=0, filt=None):
    from test_gpu_coarse_abi import _p
    b_ptr, b_item = np.ascontiguousarray(b_ptr, np.int64), np.ascontiguousarray(b_item, np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float64)
    n_q = len(b_ptr) - 1
    cnt, item = np.full(n_q, -7, np.int32), np.full((n_q, n_top), -7, np.int32)
    score, support, stats = np.full((n_q, n_top), -7.0), np.full((n_q, n_top), -7, np.int32), np.full(6, -7, np.int64)
    F, alive = (None, None) if filt is None else filt.on_host()
    rc = ctx.lib.xmap_ctx_related(ctx.h, n_q, _p(b_ptr, C.c_int64), _p(b_item, C.c_int32), _p(w, C.c_double), how, flags, n_top, min_support,
                                  max_records, _p(cnt, C.c_int32), _p(item, C.c_int32), _p(score, C.c_double), _p(support, C.c_int32),
                                  None if F is None else C.byref(F), _p(stats, C.c_int64))
    del alive
    return rc, (cnt, item, score, support, stats.tolist())


def test_the_coarse_call_equals_the_engine_on_the_downloaded_matrix():
    """NumPy arrays through xmap_ctx_related, right after xmap_ctx_rec_sim (no neighbour list is selected), against Engine.related
    and the statement over the matrix xmap_ctx_rec_download gives"""
    from test_gpu_coarse_abi import Ctx
    from test_gpu_filter import Filter
    from test_gpu_tail import _GoldRatings, generate, rec_sim
    from xmap.engine import device, filters
    r = _GoldRatings("small")
    I, U = r.n_items, len(r.user_ptr) - 1
    rng = np.random.RandomState(3)
    lens = rng.randint(0, 6, 40)
    b_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    b_item = rng.randint(-1, I + 1, b_ptr[-1]).astype(np.int32)
    weights = rng.randint(-3, 9, len(b_item)) / 3.0
    ctx = Ctx()
    try:
        ERR = ctx.abi.ERR_ARG
        rc, got = _ctx_related(ctx, b_ptr, b_item, None, SUM, 0, 5)
        assert rc == ERR and b"have_rec" in ctx.lib.xmap_last_error() and untouched(got[:4])
        rows = generate(ctx, r)
        rc, got = _ctx_related(ctx, b_ptr, b_item, None, SUM, 0, 5)
        assert rc == ERR and b"have_rec" in ctx.lib.xmap_last_error() and untouched(got[:4])
        T = rec_sim(ctx, I, U, len(rows["user"]))
        M = rs.Matrix(T["row_ptr"], T["col"], T["sim"])
        assert M.n_items == I and len(M.col) > 1000
        eng = device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, I, r.item_attrs(), DEV))
        S = (_dev(M.row_ptr), _dev(M.col), _dev(M.sim))
        mask = rng.rand(I) < 0.6
        exclude = [[int(x) for x in rng.randint(0, I, 4)] + [-1, I] for _ in lens]
        import torch
        for how, name, w, flags, n_top, ms, filt, kw, ekw in (
                (SUM, "sum", None, 0, 10, 1, None, {}, {}),
                (MEAN, "mean", weights, KEEP_MEMBERS, 300, 2, Filter(allow=mask, exclude=exclude, min_score=0.01),
                 dict(allow=mask, exclude=exclude, min_score=0.01),
                 dict(allow=torch.from_numpy(mask).to(DEV), min_score=0.01, exclude=tuple(_dev(a) for a in filters.exclusion_csr(exclude)))),
                (MAX, "max", weights, 0, 3, 1, Filter(null=True), {}, {})):
            rc, got = _ctx_related(ctx, b_ptr, b_item, w, how, flags, n_top, ms, 0 if how != MAX else 7, filt)
            assert rc == 0, ctx.lib.xmap_last_error()
            e = eng.related(S, _dev(b_ptr), _dev(b_item)[:len(b_item)], n_top, how=name, weights=None if w is None else _dev(w),
                            keep_members=bool(flags), min_support=ms, **ekw)
            e = [x.cpu().numpy() for x in e[:4]] + [list(e[4])]
            assert as_bytes(got) == as_bytes(e)
            same(got, rs.related_statement(M, b_ptr, b_item, n_top, how, flags, ms, w, **kw))
            assert got[4][0] > 0 and got[0].max() > 0
        # host checks with a context: XMAP_ERR_ARG, the outputs keep every byte
        for kw in (dict(n_top=0), dict(n_top=1025), dict(how=3), dict(flags=2), dict(min_support=0), dict(filt=Filter(min_score=float("nan")))):
            a = dict(how=SUM, flags=0, n_top=5, min_support=1, filt=None)
            a.update(kw)
            n = a["n_top"]
            rc, got = _ctx_related(ctx, b_ptr, b_item, None, a["how"], a["flags"], n if 1 <= n <= 1024 else 5, a["min_support"], 0, a["filt"]) \
                if 1 <= n <= 1024 else _ctx_related_n(ctx, b_ptr, b_item, n)
            assert rc == ERR and untouched(got[:4]), kw
        # a stage run again drops the rows the call reads
        ctx.call("xmap_ctx_item_sim", 0, 50, None, None)
        rc, got = _ctx_related(ctx, b_ptr, b_item, None, SUM, 0, 5)
        assert rc == ERR and b"have_rec" in ctx.lib.xmap_last_error()
    finally:
        ctx.close()


def _ctx_related_n(ctx, b_ptr, b_item, n_top):
    """the coarse call with an n_top the outputs cannot be shaped by: five columns"""
    from test_gpu_coarse_abi import _p
    n_q = len(b_ptr) - 1
    cnt, item = np.full(n_q, -7, np.int32), np.full((n_q, 5), -7, np.int32)
    score, support = np.full((n_q, 5), -7.0), np.full((n_q, 5), -7, np.int32)
    rc = ctx.lib.xmap_ctx_related(ctx.h, n_q, _p(np.ascontiguousarray(b_ptr, np.int64), C.c_int64), _p(np.ascontiguousarray(b_item, np.int32), C.c_int32),
                                  None, 0, 0, n_top, 1, 0, _p(cnt, C.c_int32), _p(item, C.c_int32), _p(score, C.c_double),
                                  _p(support, C.c_int32), None, None)
    return rc, (cnt, item, score, support)


# ------------------------------------------------------------------------------------------------------- 6. the session
def _matrix_of(S):
    n = int(S.row_ptr[-1].item())
    return rs.Matrix(S.row_ptr.cpu().numpy(), S.col.cpu().numpy()[:n], S.sim.cpu().numpy()[:n])


def _lines(want, labels, iids):
    return [(lab, [(iids[want[1][q, t]], float(want[2][q, t]), int(want[3][q, t])) for t in range(want[0][q])])
            for q, lab in enumerate(labels)]


def test_session_related_items_on_the_small_golden_set():
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
    st, _, _, S = session._tail_matrix(ae, CAP, "test")
    M = _matrix_of(S)
    iids, iidx = st.idt.iids, st.idt.iidx
    I = len(iids)
    has_row = [i for i in range(I) if M.row_ptr[i + 1] > M.row_ptr[i]]
    assert len(has_row) > 20
    rng = np.random.RandomState(9)
    picks = [[int(x) for x in rng.choice(has_row, k, replace=False)] for k in (1, 2, 3, 5, 5, 8)]
    baskets = [("cart-%d" % k, [iids[i] for i in p]) for k, p in enumerate(picks)]
    baskets += [("empty", []), ("made-up", ["no-such-item", iids[has_row[0]]]), ("twice", [iids[has_row[1]]] * 2)]
    labels = [lab for lab, _ in baskets]
    known = [[iidx[x] for x in members if x in iidx] for _, members in baskets]
    b_ptr = np.concatenate([[0], np.cumsum([len(k) for k in known])]).astype(np.int64)
    b_item = np.asarray([x for k in known for x in k], np.int32)
    shop = [iids[k] for k in range(0, I, 2)] + ["unknown-item"]
    allow = np.zeros(I, bool)
    allow[np.arange(0, I, 2)] = True
    excl = {"cart-1": [iids[has_row[2]], "unknown-item"], "cart-4": list(iids[:40])}
    ex_lists = [[iidx[x] for x in excl.get(lab, ()) if x in iidx] for lab in labels]
    for kw, skw in ((dict(), dict()), (dict(how="mean", keep_members=True, min_support=2), dict(how=MEAN, flags=KEEP_MEMBERS, min_support=2)),
                    (dict(how="max", allow_items=shop, exclude=excl, min_score=0.0), dict(how=MAX, allow=allow, exclude=ex_lists, min_score=0.0))):
        out = session.related_items(ae, baskets, CAP, 7, **kw)
        want = rs.related_statement(M, b_ptr, b_item, 7, **skw)
        assert out.collect() == _lines(want, labels, iids)
        assert list(out.stats) == want[4] and want[4][0] > 0 and out.unknown_items == 1
    assert dict(session.related_items(ae, baskets, CAP, 7).collect())["empty"] == []
    # weights
    wb = [(lab, [(x, 0.5 + k) for k, x in enumerate(members)]) for lab, members in baskets]
    weights = np.asarray([0.5 + k for _, members in baskets for k, x in enumerate(members) if x in iidx])
    out = session.related_items(ae, wb, CAP, 7)
    assert out.collect() == _lines(rs.related_statement(M, b_ptr, b_item, 7, weights=weights), labels, iids)
    with pytest.raises(ValueError):
        session.related_items(ae, baskets + [("cart-0", [])], CAP, 7)
    # a source member is replaced by its target under the handle's map
    mp, flags = ae.G.map.cpu().numpy(), st.engine.R.flags.cpu().numpy()
    src = [i for i in range(I) if not flags[i] & 2]
    mapped = [i for i in src if mp[i] >= 0 and M.row_ptr[mp[i] + 1] > M.row_ptr[mp[i]]]
    unmapped = [i for i in src if mp[i] < 0]
    assert mapped and unmapped
    movies = [("m", [iids[mapped[0]], iids[unmapped[0]], iids[has_row[0]], "no-such-item"])]
    books = [("m", [iids[mp[mapped[0]]], iids[has_row[0]]])]
    out = session.related_items(ae, movies, CAP, 7, map_sources=True)
    assert out.collect() == session.related_items(ae, books, CAP, 7).collect() and out.collect()[0][1] and out.unknown_items == 2
    assert session.related_items(ae, movies, CAP, 7).unknown_items == 1
    with pytest.raises(TypeError):
        session.related_items(trainRDD, baskets, CAP, 7)


def test_session_related_items_on_a_union_of_two_parts():
    import datetime
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from golden_util import CAP
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.engine import session, synth
    from xmap.utils import assist
    doms = synth.make_multi_domain(17, 600, 200, 150, 2, overlap=0.4)
    t0 = datetime.datetime(2013, 3, 1)
    sc = SparkContext(conf=SparkConf())
    tool = BaselinerSim("cosine", CAP)
    handles = []
    for r in doms:
        recs = [(u, [(i, ra, t0 + datetime.timedelta(days=(t * 7919) % 6)) for i, ra, t in prof]) for u, prof in r.train_records()]
        trainRDD = sc.parallelize(recs, 8).cache()
        sim = assist.baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
        ext = assist.extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
        handles.append(assist.generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True))
    union = session.union_alterego(handles)
    st, _, _, S = session._tail_matrix(union, CAP, "test")
    M = _matrix_of(S)
    iids, iidx = st.idt.iids, st.idt.iidx
    has_row = [i for i in range(len(iids)) if M.row_ptr[i + 1] > M.row_ptr[i]]
    rng = np.random.RandomState(4)
    picks = [[int(x) for x in rng.choice(has_row, k, replace=False)] for k in (1, 3, 5, 5)]
    baskets = [("b%d" % k, [iids[i] for i in p]) for k, p in enumerate(picks)] + [("none", ["no-such-item"])]
    b_ptr = np.concatenate([[0], np.cumsum([len(p) for p in picks] + [0])]).astype(np.int64)
    b_item = np.asarray([x for p in picks for x in p], np.int32)
    out = session.related_items(union, baskets, CAP, 10, min_support=2)
    want = rs.related_statement(M, b_ptr, b_item, 10, min_support=2)
    assert out.collect() == _lines(want, [lab for lab, _ in baskets], iids)
    assert list(out.stats) == want[4] and want[0].max() > 0 and out.unknown_items == 1
    with pytest.raises(TypeError, match="one replacement map per part"):
        session.related_items(union, baskets, CAP, 10, map_sources=True)
