"""Shelves on the device (csrc/stage_e_shelf.hip; xmap_shelf_segments, xmap_shelf_rows, xmap_ctx_set_labels,
xmap_ctx_recommend_shelves, Engine.shelves, session.recommend_shelves) against tests/shelf_statement.py.  Everything is exact:
integers with array_equal, doubles through uint64 views.  The outputs are pre-filled with sentinels and allocated with guard
elements behind them that must survive."""
import ctypes as C

import numpy as np
import pytest

import shelf_statement as ss
from shelf_statement import BEST, LABEL, MEAN, Labels, check_shelf_output, expected_shelf_segments, expected_shelves
from test_gpu_audience import OnDevice
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_filter import Filter, _words, topn_f
from test_gpu_tail import _few_times, generate, rec_sim, select, wtab
from test_gpu_topn import KEEP_HELD, _hand_case, _random_case, score_users

pytestmark = pytest.mark.gpu
GUARD = 5
NO_FILTER = Filter(null=True)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


# ------------------------------------------------------------------------------------------------------- the drivers
def _dev(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a, dtype)
    if a.size == 0:
        a = np.zeros(1, a.dtype)                # (never an empty tensor: its pointer would be NULL)
    return torch.from_numpy(a).to("cuda:0")


class Outs(object):
    """the eight outputs as flat device tensors of -7 with GUARD elements behind each"""
    DT = ("i", "i", "d", "i", "i", "i", "d", "d")

    def __init__(self, Q, n_shelf, n_top):
        import torch
        self.shapes = [(Q,)] + [(Q, n_shelf)] * 4 + [(Q, n_shelf, n_top)] * 3
        self.t = [torch.full((int(np.prod(s)) + GUARD,), -7, dtype=torch.int32 if k == "i" else torch.float64, device="cuda:0")
                  for s, k in zip(self.shapes, self.DT)]

    def host(self):
        """(the eight arrays, every guard element still -7)"""
        flat = [t.cpu().numpy() for t in self.t]
        return [f[:-GUARD].reshape(s) for f, s in zip(flat, self.shapes)], all((f[-GUARD:] == -7).all() for f in flat)

    def untouched(self):
        return all((t.cpu().numpy() == -7).all() for t in self.t)


class LabelsOnDevice(object):
    def __init__(self, labels, lab_allow=None):
        self.n_items, self.n_labels = labels.n_items, labels.n_labels
        self.ptr, self.id = _dev(labels.ptr, np.int64), _dev(labels.id, np.int32)
        self.allow = None if lab_allow is None else _dev(_words(lab_allow).view(np.int32))


class Segments(object):
    """scored segments [[(item, plain, decayed, status)*]*] on the device"""

    def __init__(self, segments, cand_ptr=None):
        self.Q = len(segments)
        ptr = np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.int64) if cand_ptr is None else cand_ptr
        flat = [c for s in segments for c in s]
        self.ptr = _dev(ptr, np.int64)
        self.item, self.plain = _dev([c[0] for c in flat], np.int32), _dev([c[1] for c in flat], np.float64)
        self.decay, self.status = _dev([c[2] for c in flat], np.float64), _dev([c[3] for c in flat], np.int32)


def shelf_segments_rc(S, L, n_shelf, n_top, rank_by, shelf_by, min_fill, min_score=None, max_records=0):
    """xmap_shelf_segments: (rc, message, Outs, stats [4])"""
    import torch
    from xmap.engine import hipabi as abi
    O = Outs(S.Q, n_shelf, n_top)
    h = (C.c_int64 * 4)(*([-7] * 4))
    st = C.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)
    rc = abi.lib.xmap_shelf_segments(st, abi.i64(S.Q), abi.vp(S.ptr), abi.vp(S.item), abi.vp(S.plain), abi.vp(S.decay), abi.vp(S.status),
                                     C.c_double(-np.inf if min_score is None else min_score), abi.i32(L.n_items), abi.i32(L.n_labels),
                                     abi.vp(L.ptr), abi.vp(L.id), abi.vp(L.allow), abi.i32(n_shelf), abi.i32(n_top), abi.i32(rank_by),
                                     abi.i32(shelf_by), abi.i32(min_fill), abi.i64(max_records), *([abi.vp(t) for t in O.t] + [h]))
    torch.cuda.synchronize()
    return rc, (abi.lib.xmap_last_error() or b"").decode(), O, [int(x) for x in h]


def shelf_segments(*a, **kw):
    rc, msg, O, h = shelf_segments_rc(*a, **kw)
    assert rc == 0, msg
    got, guards = O.host()
    assert guards
    return got, h


def shelf_rows_rc(D, U, I, keep, n_w, queries, L, n_shelf, n_top, rank_by, flags, shelf_by, min_fill, filt=NO_FILTER, max_records=0, alpha=1.5):
    """xmap_shelf_rows on an OnDevice of (ptr, item, rating, time, cnt, col, sim, avg): (rc, message, Outs, stats [10])"""
    import torch
    from xmap.engine import hipabi as abi
    ptr, pit, pra, pti, cnt, col, sim, avg = D.t
    q = _dev(queries, np.int32)
    Q = len(queries)
    w = _dev(wtab(alpha, n_w))
    O = Outs(Q, n_shelf, n_top)
    h = (C.c_int64 * 10)(*([-7] * 10))
    st = C.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)
    F, alive = filt.on_device()
    rc = abi.lib.xmap_shelf_rows(st, abi.i64(Q), abi.vp(q), abi.i32(n_top), abi.i32(rank_by), abi.i32(flags), abi.i64(U), abi.i32(I), abi.i32(keep),
                                 abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ptr), abi.vp(pit), abi.vp(pra), abi.vp(pti), abi.vp(avg), abi.vp(w),
                                 abi.i32(n_w), abi.i32(L.n_labels), abi.vp(L.ptr), abi.vp(L.id), abi.vp(L.allow), abi.i32(n_shelf),
                                 abi.i32(shelf_by), abi.i32(min_fill), abi.i64(max_records),
                                 *([abi.vp(t) for t in O.t] + [None if F is None else C.byref(F), h]))
    torch.cuda.synchronize()
    del alive
    return rc, (abi.lib.xmap_last_error() or b"").decode(), O, [int(x) for x in h]


def shelf_rows(*a, **kw):
    rc, msg, O, h = shelf_rows_rc(*a, **kw)
    assert rc == 0, msg
    got, guards = O.host()
    assert guards
    return got, h


@pytest.fixture(scope="module")
def designed():
    """the designed segments, their labels and the designed lab_allow: built and uploaded once"""
    segments, labels = ss.designed()
    allow = ss.designed_allow()
    return dict(segments=segments, labels=labels, allow=allow, S=Segments(segments), L=LabelsOnDevice(labels),
                LA=LabelsOnDevice(labels, allow))


# ---------------------------------------------------------------------------- 1. the designed segments against the statement
@pytest.mark.parametrize("n_top", [1, 10, 63, 64])
def test_designed_segments_against_the_statement(designed, n_top):
    d = designed
    for n_shelf in (1, 3, 64):
        for shelf_by in (BEST, MEAN, LABEL):
            for min_fill in (1, 2, 65):
                want, stats = expected_shelf_segments(d["segments"], d["labels"], n_shelf, n_top, 0, shelf_by, min_fill)
                got, h = shelf_segments(d["S"], d["L"], n_shelf, n_top, 0, shelf_by, min_fill)
                check_shelf_output(got, want, n_shelf, n_top)
                assert tuple(h) == stats, (h, stats)
    # the decayed score, a floor and the designed lab_allow
    for n_shelf, shelf_by, min_fill, rank_by, floor, which in ((3, BEST, 1, 1, None, "L"), (3, MEAN, 2, 0, -0.5, "L"), (64, LABEL, 1, 1, 0.1, "LA"),
                                                               (3, BEST, 1, 0, None, "LA"), (1, MEAN, 1, 1, -0.5, "LA")):
        allow = d["allow"] if which == "LA" else None
        want, stats = expected_shelf_segments(d["segments"], d["labels"], n_shelf, n_top, rank_by, shelf_by, min_fill, min_score=floor,
                                              lab_allow=allow)
        got, h = shelf_segments(d["S"], d[which], n_shelf, n_top, rank_by, shelf_by, min_fill, min_score=floor)
        check_shelf_output(got, want, n_shelf, n_top)
        assert tuple(h) == stats, (h, stats)


# ------------------------------------------------------------- 2. the chunking and a second call do not change a byte
def test_the_bytes_depend_on_no_chunking(designed):
    d = designed
    records = expected_shelf_segments(d["segments"], d["labels"], 3, 10, 0, BEST, 1)[1][0]
    assert records > 64
    for n_shelf, n_top, shelf_by, min_fill in ((3, 10, BEST, 1), (64, 64, MEAN, 2), (1, 1, LABEL, 1)):
        ref, h_ref = shelf_segments(d["S"], d["L"], n_shelf, n_top, 0, shelf_by, min_fill)
        for max_records in (0, 1, 7, 64, records - 1):
            got, h = shelf_segments(d["S"], d["L"], n_shelf, n_top, 0, shelf_by, min_fill, max_records=max_records)
            assert [a.tobytes() for a in got] == [a.tobytes() for a in ref] and h == h_ref, max_records


# ----------------------------------------------------------------- 3. bad tables: an error, a message, untouched outputs
def test_bad_tables_are_refused_before_anything_is_written(designed):
    from xmap.engine import hipabi as abi
    d = designed
    labels = d["labels"]
    good = (labels.ptr.copy(), labels.id.copy())
    two = int(np.flatnonzero(np.diff(labels.ptr) >= 2)[0])          # an item with two labels at least
    k2 = int(labels.ptr[two])

    def table(change):
        ptr, ids = good[0].copy(), good[1].copy()
        change(ptr, ids)
        return Labels(labels.n_items, labels.n_labels, ptr, ids)

    def first(ptr, ids): ptr[0] = 1
    def decreasing(ptr, ids): ptr[7] = ptr[6] - 1 if ptr[6] > 0 else ptr[8] + 1
    def too_large(ptr, ids): ids[3] = labels.n_labels
    def negative(ptr, ids): ids[5] = -1
    def equal(ptr, ids): ids[k2 + 1] = ids[k2]
    def descending(ptr, ids): ids[k2], ids[k2 + 1] = ids[k2 + 1], ids[k2]

    for change, rule, word in ((first, "lab_ptr", "lab_ptr"), (decreasing, "lab_ptr", "lab_ptr"), (too_large, "range", "out of range"),
                               (negative, "range", "out of range"), (equal, "ascending", "strictly ascending"),
                               (descending, "ascending", "strictly ascending")):
        bad = table(change)
        what = ss.check_tables(bad.n_items, bad.n_labels, bad.ptr, bad.id)
        assert what is not None and what[0] == rule
        rc, msg, O, h = shelf_segments_rc(d["S"], LabelsOnDevice(bad), 3, 10, 0, BEST, 1)
        assert rc == abi.ERR_ARG and word in msg and "[%d]" % what[1] in msg, msg
        assert O.untouched() and h == [-7] * 4
    # a decreasing cand_ptr
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in d["segments"]])]).astype(np.int64)
    ptr[4] = ptr[3] - 1
    rc, msg, O, h = shelf_segments_rc(Segments(d["segments"], cand_ptr=ptr), d["L"], 3, 10, 0, BEST, 1)
    assert rc == abi.ERR_ARG and "cand_ptr" in msg and "[4]" in msg, msg
    assert O.untouched() and h == [-7] * 4
    # the host checks of the fine-grained call
    for kw, word in ((dict(n_shelf=0), "n_shelf"), (dict(n_top=65), "n_top"), (dict(shelf_by=3), "shelf_by"), (dict(min_fill=0), "min_fill"),
                     (dict(rank_by=2), "rank_by"), (dict(min_score=float("nan")), "min_score")):
        a = dict(n_shelf=3, n_top=10, rank_by=0, shelf_by=BEST, min_fill=1)
        a.update(kw)
        rc, msg, O, h = shelf_segments_rc(d["S"], d["L"], **a)
        assert rc == abi.ERR_ARG and word in msg and O.untouched(), msg


# ------------------------------------------------------------------------------ 4. xmap_shelf_rows against the filtered top-N
class Case(object):
    def __init__(self, arrays, U, I, keep):
        self.arrays, self.U, self.I, self.keep = arrays, U, I, keep
        self.D = OnDevice(arrays)


@pytest.fixture(scope="module")
def hand():
    arrays, U, I, keep, _ = _hand_case()
    return Case(arrays, U, I, keep)


@pytest.fixture(scope="module")
def rand():
    U, I, keep = 50, 400, 5
    return Case(_random_case(24, U, I, keep, np.arange(0, I, 3), lambda u: 2 + u % 9), U, I, keep)


def _seven_labels(I, seed=2):
    """7 labels: every third item carries two, some carry none"""
    rng = np.random.default_rng(seed)
    per = []
    for i in range(I):
        l = int(rng.integers(0, 7))
        per.append([] if i % 11 == 5 else sorted({l, (l + 1 + int(rng.integers(0, 5))) % 7}) if i % 3 == 0 else [l])
    return Labels.of(per, 7)


def _rules(case, queries, seed=9):
    rng = np.random.default_rng(seed)
    exclude = [rng.integers(-2, case.I + 2, int(rng.integers(0, 9))).tolist() for _ in queries]
    return rng.random(case.I) < 0.8, exclude


@pytest.mark.parametrize("which", ["hand", "rand"])
def test_one_label_and_one_shelf_is_the_filtered_top_n(which, hand, rand):
    c = hand if which == "hand" else rand
    queries = list(range(c.U)) + [c.U + 5, -1, 3, 3]
    L = LabelsOnDevice(Labels.of([[0]] * c.I, 1))
    allow, exclude = _rules(c, queries)
    for n, rank_by, flags, filt in ((10, 0, 0, NO_FILTER), (64, 1, KEEP_HELD, Filter(allow=allow, exclude=exclude, min_score=3.0)),
                                    (1, 0, 0, Filter(exclude=exclude))):
        ref = topn_f(c.D, c.U, c.I, c.keep, 66, queries, n, rank_by, flags, filt)
        whole = topn_f(c.D, c.U, c.I, c.keep, 66, queries, 64, rank_by, flags, filt)
        for shelf_by in (BEST, MEAN, LABEL):
            got, h = shelf_rows(c.D, c.U, c.I, c.keep, 66, queries, L, 1, n, rank_by, flags, shelf_by, 1, filt)
            nshelf, label, sscore, size, cnt, item, plain, decay = got
            assert np.array_equal(cnt[:, 0], ref[0]) and np.array_equal(nshelf, (ref[0] > 0).astype(np.int32))
            assert item[:, 0].tobytes() == ref[1].tobytes() and plain[:, 0].tobytes() == ref[2].tobytes()
            assert decay[:, 0].tobytes() == ref[3].tobytes()
            assert h[:6] == ref[4], (h, ref[4])
            kept = ref[4][0] - ref[4][1] - ref[4][4]                # scored - dropped - below the floor
            assert int(size.sum()) == kept == h[6] and h[7] == int((ref[0] > 0).sum()) and h[8] == 0 and h[9] == 1
            small = whole[0] < 64                                    # the whole list fits: its length is the shelf's size
            assert np.array_equal(size[small, 0], whole[0][small]) and (size[~small, 0] >= 64).all()
            assert np.array_equal(label[:, 0], np.where(ref[0] > 0, 0, -1))
            if shelf_by != MEAN:
                assert sscore[:, 0].tobytes() == (ref[3] if rank_by else ref[2])[:, 0].tobytes()


@pytest.mark.parametrize("which", ["hand", "rand"])
def test_every_shelf_is_the_filtered_top_n_under_its_labels_mask(which, hand, rand):
    c = hand if which == "hand" else rand
    queries = list(range(c.U)) + [c.U + 5, 3]
    labels = _seven_labels(c.I)
    assert (np.diff(labels.ptr) == 0).any() and (np.diff(labels.ptr) == 2).any()
    L = LabelsOnDevice(labels)
    allow, exclude = _rules(c, queries)
    for n, rank_by, flags, a, ex, floor in ((10, 0, 0, None, None, None), (5, 1, KEEP_HELD, allow, exclude, 3.0), (64, 0, 0, allow, None, None)):
        filt = NO_FILTER if a is None and ex is None and floor is None else Filter(allow=a, exclude=ex, min_score=floor)
        got, h = shelf_rows(c.D, c.U, c.I, c.keep, 66, queries, L, 7, n, rank_by, flags, LABEL, 1, filt)
        nshelf, label, sscore, size, cnt, item, plain, decay = got
        seen = 0
        for l in range(7):
            mask = labels.carries(l) & (np.ones(c.I, bool) if a is None else a)
            ref = topn_f(c.D, c.U, c.I, c.keep, 66, queries, n, rank_by, flags, Filter(allow=mask, exclude=ex, min_score=floor))
            for q in range(len(queries)):
                at = np.flatnonzero(label[q] == l)
                if ref[0][q] == 0:
                    assert len(at) == 0
                    continue
                s = int(at[0])
                assert cnt[q, s] == ref[0][q] and item[q, s].tobytes() == ref[1][q].tobytes()
                assert plain[q, s].tobytes() == ref[2][q].tobytes() and decay[q, s].tobytes() == ref[3][q].tobytes()
                seen += 1
        assert seen == int(nshelf.sum()) > 0
        assert all((np.diff(label[q, :nshelf[q]]) > 0).all() for q in range(len(queries)))


@pytest.mark.parametrize("which", ["hand", "rand"])
def test_shelf_rows_against_the_statement(which, hand, rand):
    c = hand if which == "hand" else rand
    queries = list(range(c.U)) + [c.U + 5, -1, 3]
    scored = score_users(1.5, queries, *c.arrays[:8], c.keep)
    labels = _seven_labels(c.I)
    lab_allow = np.asarray([1, 1, 0, 1, 1, 1, 0], bool)
    allow, exclude = _rules(c, queries)
    for n_shelf, n, rank_by, flags, shelf_by, min_fill, la, filt in (
            (3, 10, 0, 0, BEST, 1, None, NO_FILTER), (7, 5, 1, KEEP_HELD, MEAN, 2, lab_allow, Filter(allow=allow, exclude=exclude, min_score=3.0)),
            (2, 64, 0, 0, LABEL, 3, lab_allow, Filter(exclude=exclude)), (64, 3, 1, 0, MEAN, 1, None, Filter(min_score=2.5))):
        want, stats = expected_shelves(scored, queries, labels, n_shelf, n, rank_by, shelf_by, min_fill, bool(flags), 66, lab_allow=la,
                                       **({} if filt.null else filt.statement()))
        got, h = shelf_rows(c.D, c.U, c.I, c.keep, 66, queries, LabelsOnDevice(labels, la), n_shelf, n, rank_by, flags, shelf_by, min_fill, filt)
        check_shelf_output(got, want, n_shelf, n)
        print("stats", h, "statement", stats)
        assert tuple(h) == stats
        assert h[7] > 0


# ------------------------------------------------------------------------------ 5. the coarse entries over the three sources
def _ctx_shelves(ctx, source, queries, n_shelf, n, rank_by, flags, shelf_by, min_fill, lab_allow=None, F=None, n_w=66, alpha=1.5):
    """xmap_ctx_recommend_shelves: (rc, message, the eight outputs pre-filled with -7, stats [10])"""
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    outs = [np.full(Q, -7, np.int32), np.full((Q, n_shelf), -7, np.int32), np.full((Q, n_shelf), -7.0), np.full((Q, n_shelf), -7, np.int32),
            np.full((Q, n_shelf), -7, np.int32), np.full((Q, n_shelf, n), -7, np.int32), np.full((Q, n_shelf, n), -7.0),
            np.full((Q, n_shelf, n), -7.0)]
    stats = np.full(10, -7, np.int64)
    words = None if lab_allow is None else _words(lab_allow)
    rc = ctx.lib.xmap_ctx_recommend_shelves(ctx.h, source, Q, _p(q, C.c_int32), n_shelf, n, rank_by, flags, _p(w, C.c_double), n_w, shelf_by,
                                            min_fill, None if words is None else words.ctypes.data_as(C.c_void_p),
                                            *([o.ctypes.data_as(C.c_void_p) for o in outs] +
                                              [None if F is None else C.byref(F), _p(stats, C.c_int64)]))
    return rc, (ctx.lib.xmap_last_error() or b"").decode(), outs, stats.tolist()


def _ctx_filtered(ctx, source, queries, n, rank_by, flags, F=None, n_w=66, alpha=1.5):
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    cnt, ids = np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32)
    plain, decay, stats = np.full((Q, n), -7.0), np.full((Q, n), -7.0), np.full(6, -7, np.int64)
    ctx.call("xmap_ctx_recommend_filtered", source, Q, _p(q, C.c_int32), n, rank_by, flags, _p(w, C.c_double), n_w, _p(cnt, C.c_int32),
             _p(ids, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), None if F is None else C.byref(F), _p(stats, C.c_int64))
    return cnt, ids, plain, decay, stats.tolist()


def _set_labels(ctx, labels):
    return ctx.lib.xmap_ctx_set_labels(ctx.h, labels.n_labels, _p(labels.ptr, C.c_int64), _p(np.concatenate([labels.id, [0]]).astype(np.int32),
                                                                                              C.c_int32))


def test_the_coarse_calls_over_the_three_sources():
    from test_gpu_foldin import foldin, foldin_download
    from test_gpu_item_foldin import item_foldin
    from xmap.engine import hipabi as abi, synth
    seed, users, src_items, tgt_items, overlap = 5, 1500, 300, 300, 0.4          # the small case of the other coarse tail tests
    r = _few_times(synth.make_two_domain(seed, users, src_items, tgt_items, overlap=overlap))
    I, U, keep = r.n_items, users, 5
    rng = np.random.default_rng(seed)
    labels = _seven_labels(I)
    lab_allow = np.asarray([1, 0, 1, 1, 1, 1, 1], bool)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        # the labels hang on the item space, not on the tail: set before it is trained, they survive it
        assert _set_labels(ctx, labels) == 0
        T = rec_sim(ctx, I, U, len(rows["user"]))
        cnt, col, sim, _ = select(ctx, I, keep)
        B = 60
        lens = rng.integers(0, 30, B)
        f_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        f_item = rng.integers(0, I, f_ptr[-1]).astype(np.int32)
        f_counts = foldin(ctx, f_ptr, f_item, (rng.integers(2, 21, len(f_item)) / 4.0).astype(np.float32),
                          1000 + rng.integers(0, 7, len(f_item)).astype(np.int64))
        fold = foldin_download(ctx, B, f_counts[0])
        NB = 6
        b_lens = rng.integers(10, 40, NB)
        b_ptr = np.concatenate([[0], np.cumsum(b_lens)]).astype(np.int64)
        b_user = np.concatenate([rng.choice(U, k, replace=False) for k in b_lens]).astype(np.int32)
        item_foldin(ctx, (b_ptr, b_user, rng.integers(2, 21, len(b_user)) / 4.0))
        L = LabelsOnDevice(labels, lab_allow)
        # ---- resident and fold-in: the fine-grained call on the same arrays, byte for byte
        for source, (n_users, prof, qs) in {0: (U, (T["ptr"], T["item"], T["rating"], T["time"]), np.arange(-1, 200)),
                                            1: (B, fold, np.arange(-1, B + 1))}.items():
            D = OnDevice(list(prof) + [cnt, col, sim, T["avg"]])
            qs = np.concatenate([qs, qs[5:8]]).astype(np.int32)
            exclude = [rng.integers(-2, I + 2, int(rng.integers(0, 9))).tolist() for _ in qs]
            filt = Filter(allow=rng.random(I) < 0.7, exclude=exclude, min_score=2.5)
            for n_shelf, n, rank_by, flags, shelf_by, min_fill, la, f in ((3, 10, 0, 0, BEST, 1, None, NO_FILTER),
                                                                           (7, 4, 1, KEEP_HELD, MEAN, 2, lab_allow, filt),
                                                                           (7, 64, 0, 0, LABEL, 1, lab_allow, filt)):
                F, alive = f.on_host()
                rc, msg, got, stats = _ctx_shelves(ctx, source, qs, n_shelf, n, rank_by, flags, shelf_by, min_fill, la, F)
                assert rc == 0, msg
                ref, h = shelf_rows(D, n_users, I, keep, 66, qs, L if la is not None else LabelsOnDevice(labels), n_shelf, n, rank_by, flags,
                                    shelf_by, min_fill, f)
                assert [a.tobytes() for a in got] == [a.tobytes() for a in ref] and stats == h
                assert stats[7] > 0 and got[0].max() > 1
        # ---- item fold-in: the batch items carry no label -- every shelf is the coarse filtered list under its label's mask
        qs = np.arange(0, 150).astype(np.int32)
        plain = _ctx_filtered(ctx, 2, qs, 64, 0, 0)
        assert (plain[1] >= I).any()                                 # batch items are candidates of the plain call
        rc, msg, got, stats = _ctx_shelves(ctx, 2, qs, 7, 10, 0, 0, LABEL, 1)
        assert rc == 0, msg
        nshelf, label, sscore, size, s_cnt, item, s_plain, s_decay = got
        assert not (item >= I).any() and nshelf.max() > 1
        for l in range(7):
            words = _words(np.concatenate([labels.carries(l), np.zeros(NB, bool)]))
            ref = _ctx_filtered(ctx, 2, qs, 10, 0, 0, abi.RecFilter(words.ctypes.data, None, None, -np.inf))
            for q in range(len(qs)):
                at = np.flatnonzero(label[q] == l)
                assert len(at) == (1 if ref[0][q] else 0)
                if ref[0][q]:
                    s = int(at[0])
                    assert s_cnt[q, s] == ref[0][q] and item[q, s].tobytes() == ref[1][q].tobytes()
                    assert s_plain[q, s].tobytes() == ref[2][q].tobytes() and s_decay[q, s].tobytes() == ref[3][q].tobytes()
        # ---- the extended table beside a lab_allow: every label allowed is the bytes of lab_allow NULL, which the lists above are
        # the first rows of; no queries: the stats zeroed, nothing else
        few = _ctx_shelves(ctx, 2, qs[:8], 7, 4, 0, 0, LABEL, 1)
        every = _ctx_shelves(ctx, 2, qs[:8], 7, 4, 0, 0, LABEL, 1, np.ones(7, bool))
        assert few[0] == 0 and every[0] == 0, (few[1], every[1])
        assert [a.tobytes() for a in every[2]] == [a.tobytes() for a in few[2]] and every[3] == few[3]
        assert np.array_equal(few[2][1], label[:8]) and np.array_equal(few[2][5], item[:8, :, :4]) and few[2][0].max() > 1
        rc, msg, none, stats = _ctx_shelves(ctx, 2, qs[:0], 7, 4, 0, 0, LABEL, 1, np.ones(7, bool))
        assert rc == 0 and stats == [0] * 10, msg
        # ---- a table that fails leaves the earlier one in place; a second call replaces it; n_labels = 0 drops it
        before = _ctx_shelves(ctx, 0, qs, 3, 10, 0, 0, BEST, 1)
        bad = Labels(I, 7, labels.ptr, np.where(np.arange(len(labels.id)) == 4, 7, labels.id))
        assert _set_labels(ctx, bad) == abi.ERR_ARG and "out of range" in (ctx.lib.xmap_last_error() or b"").decode()
        again = _ctx_shelves(ctx, 0, qs, 3, 10, 0, 0, BEST, 1)
        assert again[0] == 0 and [a.tobytes() for a in again[2]] == [a.tobytes() for a in before[2]]
        assert _set_labels(ctx, Labels.of([[0]] * I, 1)) == 0
        rc, msg, got, stats = _ctx_shelves(ctx, 0, qs, 1, 10, 0, 0, BEST, 1)
        ref = _ctx_filtered(ctx, 0, qs, 10, 0, 0)
        assert rc == 0 and got[4][:, 0].tobytes() == ref[0].tobytes() and got[5][:, 0].tobytes() == ref[1].tobytes()
        assert got[6][:, 0].tobytes() == ref[2].tobytes() and stats[:6] == ref[4]
        assert ctx.lib.xmap_ctx_set_labels(ctx.h, 0, None, None) == 0
        rc, msg, got, stats = _ctx_shelves(ctx, 0, qs, 1, 10, 0, 0, BEST, 1)
        assert rc == abi.ERR_ARG and "labels" in msg and all((o == -7).all() for o in got) and stats == [-7] * 10
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------- 6. the Python routes
def test_engine_shelves_on_tensors(rand, designed):
    import torch
    from xmap.engine import device
    from xmap.engine.labels import label_mask
    from types import SimpleNamespace
    c, d = rand, designed
    eng = device.Engine(SimpleNamespace(device=torch.device("cuda:0"), n_items=c.I))
    # shelves over the random case: the bytes of the fine-grained call
    ptr, pit, pra, pti, cnt, col, sim, avg = c.D.t
    P = SimpleNamespace(n_users=c.U, n_items=c.I, user_ptr=ptr, user_item=pit, user_rating64=pra, user_time=pti)
    queries = list(range(c.U)) + [c.U + 5, 3]
    seven = _seven_labels(c.I)
    lab_allow = np.asarray([1, 1, 0, 1, 1, 1, 0], bool)
    allow, exclude = _rules(c, queries)
    filt = Filter(allow=allow, exclude=exclude, min_score=3.0)
    F, alive = filt.on_device()
    T7 = eng.set_labels(c.I, 7, seven.ptr, seven.id)
    out = eng.shelves(P, (cnt, col, sim), _dev(queries, np.int32), avg, _dev(wtab(1.5, 66)), T7, 7, 5, "mean", min_fill=2, rank_by=1,
                      keep_held=True, lab_allow=torch.from_numpy(lab_allow), allow=alive[0], exclude=(alive[1], alive[2]), min_score=3.0)
    ref, h = shelf_rows(c.D, c.U, c.I, c.keep, 66, queries, LabelsOnDevice(seven, lab_allow), 7, 5, 1, KEEP_HELD, MEAN, 2, filt)
    assert [x.cpu().numpy().tobytes() for x in out[:8]] == [a.tobytes() for a in ref] and list(out[8]) == h and h[7] > 0
    plain = eng.shelves(P, (cnt, col, sim), _dev(queries, np.int32), avg, _dev(wtab(1.5, 66)), T7, 3, 10)
    ref, h = shelf_rows(c.D, c.U, c.I, c.keep, 66, queries, LabelsOnDevice(seven), 3, 10, 0, 0, BEST, 1)
    assert [x.cpu().numpy().tobytes() for x in plain[:8]] == [a.tobytes() for a in ref] and list(plain[8]) == h
    # shelf_segments over the designed segments
    S, labels = d["S"], d["labels"]
    T = eng.set_labels(labels.n_items, labels.n_labels, labels.ptr, labels.id, names=["l%02d" % k for k in range(labels.n_labels)])
    chosen = [n for k, n in enumerate(T.names) if d["allow"][k]]
    for by, name in ((BEST, "best"), (MEAN, "mean"), (LABEL, "label")):
        out = eng.shelf_segments((S.ptr, S.item, S.plain, S.decay, S.status), T, 3, 10, name, min_fill=2, lab_allow=label_mask(T.names, chosen),
                                 min_score=-0.5)
        want, stats = expected_shelf_segments(d["segments"], labels, 3, 10, 0, by, 2, min_score=-0.5, lab_allow=d["allow"])
        check_shelf_output([x.cpu().numpy() for x in out[:8]], want, 3, 10)
        assert out[8] == stats
    with pytest.raises(ValueError):
        eng.shelf_segments((S.ptr, S.item, S.plain, S.decay, S.status), T, 3, 10, "median")
    with pytest.raises(ValueError):
        eng.shelf_segments((S.ptr, S.item, S.plain, S.decay, S.status), T, 65, 10)


def test_session_recommend_shelves_equals_the_statement_on_id_strings():
    """the construction of test_gpu_topn.test_session_recommend_topn_equals_the_statement_on_id_strings; the candidates are scored on
    id strings from the collected dictionaries, the pages are the statement's through the id dictionary (an item's index is its
    rank among the iids)"""
    import datetime
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from golden_util import CAP
    from test_gpu_topn import _tool
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.core.recommenderSim import RecommenderSim
    from xmap.engine import session, synth
    from xmap.engine.localrdd import LocalRDD
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
    uids = [recs[int(x)][0] for x in rng.integers(0, len(recs), 60)] + ["A%013d" % (10 ** 9 + 1)]
    item_based = RecommenderSim("cosine_item", CAP).build_sthbased_profile(ae, "item").collectAsMap()
    alpha, ptool = 1.5, _tool(1.5)
    all_iids = sorted({i for _, prof in recs for i, _, _ in prof})
    names = ["cat%d" % k for k in range(6)]
    by_iid = {}
    for k, iid in enumerate(all_iids):          # unsorted and repeated names, items without a label, an iid nobody knows
        if k % 7 != 3:
            by_iid[iid] = [names[(k * 5 + 2) % 6], names[k % 6], names[k % 6]] if k % 3 == 0 else [names[k % 6]]
    by_iid["no-such-item"] = ["ghost"]
    mine = {uid: {} for uid in uids}
    for iid, lst in item_based.items():
        for who, ra, when in lst:
            if who in mine:
                mine[who].setdefault(iid, []).append((ra, when))
    first = session.recommend_shelves(ae, uids, CAP, 10, alpha, by_iid, 3, 5)
    assert first.label_names == names
    model = session.recommend_topn(ae, uids[:1], CAP, 10, alpha, 1)
    sim_pairs, info = model.sim_pairs, model.item_info
    order = {iid: k for k, iid in enumerate(all_iids)}
    labels = Labels.of([sorted({names.index(x) for x in by_iid.get(iid, ())}) for iid in all_iids], 6)

    def statement(n_shelf, n, shelf_by, min_fill, decay, keep_held, allow_labels=None):
        segments = []
        for uid in uids:
            cand = []
            for iid in sorted(sim_pairs):
                if not keep_held and iid in mine[uid]:
                    continue
                ev = [(s * (ra - info[nid][0]), abs(s), when) for nid, s in sim_pairs[iid] for ra, when in mine[uid].get(nid, ())]
                if ev:
                    base = info[iid][0]
                    cand.append((order[iid], base + sum(e[0] for e in ev) / sum(e[1] for e in ev), float(base + ptool._decayed_ratio(ev)), 0))
            segments.append(sorted(cand))
        la = None if allow_labels is None else np.asarray([x in allow_labels for x in names], bool)
        pages = expected_shelf_segments(segments, labels, n_shelf, n, 1 if decay else 0, ss.SHELF_BY[shelf_by], min_fill, lab_allow=la)[0]
        return [(uid, [(names[l], sc, sz, [(all_iids[e[0]], e[2] if decay else e[1]) for e in entries]) for l, sc, sz, entries in page])
                for uid, page in zip(uids, pages)]

    assert first.collect() == statement(3, 5, "best", 1, False, False)
    assert first.collect()[-1] == (uids[-1], []) and any(len(p) == 3 for _, p in first.collect())
    assert any(sz > len(e) for _, p in first.collect() for _, _, sz, e in p)
    for n_shelf, n, shelf_by, min_fill, decay, keep_held, al in ((6, 3, "label", 2, True, False, None), (2, 64, "mean", 1, False, True, names[1:4] + ["nobody"])):
        out = session.recommend_shelves(ae, LocalRDD(uids), CAP, 10, alpha, LocalRDD(list(by_iid.items())), n_shelf, n, shelf_by=shelf_by,
                                        min_fill=min_fill, decay=decay, keep_held=keep_held, allow_labels=al)
        assert out.collect() == statement(n_shelf, n, shelf_by, min_fill, decay, keep_held, al)
        assert out.stats[7] > 0
    # fold-in: every shelf of a profile outside the train set is its filtered list under the label's items
    late = [("late-%d" % k, list(recs[int(x)][1])) for k, x in enumerate(rng.integers(0, len(recs), 8))]
    page = session.recommend_shelves_profiles(ae, late, CAP, 10, alpha, by_iid, 6, 5, shelf_by="label")
    assert [uid for uid, _ in page.collect()] == [uid for uid, _ in late] and page.unknown_items == 0 and page.stats[7] > 0
    shown = {(uid, name): (size, lst) for uid, shelves in page.collect() for name, _, size, lst in shelves}
    for name in names:
        carrying = [iid for iid, ls in by_iid.items() if name in ls]
        ref = session.recommend_topn_profiles(ae, late, CAP, 10, alpha, 5, allow_items=carrying)
        for uid, lst in ref.collect():
            if lst:
                assert shown[(uid, name)][1] == [(iid, plain) for iid, plain, _ in lst] and shown[(uid, name)][0] >= len(lst)
            else:
                assert (uid, name) not in shown
    assert all([name for name, _, _, _ in shelves] == sorted(name for name, _, _, _ in shelves) for _, shelves in page.collect())
