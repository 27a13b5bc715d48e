"""Label quotas and calibrated lists on the device (csrc/stage_e_quota.hip; xmap_quota_pool, xmap_quota_rows,
xmap_ctx_recommend_quota, Engine.quota_pool / quota_topn, session.recommend_quota) against tests/quota_statement.py.  Everything is
exact: integers with array_equal, doubles through uint64 views.  The outputs are pre-filled with -7 and allocated with guard elements
behind them that must survive."""
import ctypes as C

import numpy as np
import pytest

import quota_statement as qs
from quota_statement import CAP, SHARE, INT32_MAX, Labels, check_quota_output, expected_pool, expected_quota
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
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.size == 0:
        a = np.zeros(1, a.dtype)                # (never an empty tensor: its pointer would be NULL)
    return torch.from_numpy(a).to("cuda:0")


class Outs(object):
    """the six outputs as flat device tensors of -7 with GUARD elements behind each"""
    DT = ("i", "i", "d", "d", "i", "i")

    def __init__(self, Q, n_top):
        import torch
        self.shapes = [(Q,)] + [(Q, n_top)] * 5
        self.t = [torch.full((int(np.prod(s)) + GUARD,), -7, dtype=torch.int32 if k == "i" else torch.float64, device="cuda:0")
                  for s, k in zip(self.shapes, self.DT)]

    def host(self):
        """(the six arrays, every guard element still -7)"""
        flat = [t.cpu().numpy() for t in self.t]
        return [f[:-GUARD].reshape(s) for f, s in zip(flat, self.shapes)], all((f[-GUARD:] == -7).all() for f in flat)

    def untouched(self):
        return all((t.cpu().numpy() == -7).all() for t in self.t)


class LabelsOnDevice(object):
    """a label table on the device; lab_allow: None, a bool array [n_labels] or packed uint32 words"""

    def __init__(self, labels, lab_allow=None):
        self.n_items, self.n_labels = labels.n_items, labels.n_labels
        self.ptr, self.id = _dev(labels.ptr, np.int64), _dev(labels.id, np.int32)
        if lab_allow is not None and np.asarray(lab_allow).dtype == np.bool_:
            lab_allow = _words(lab_allow)
        self.allow = None if lab_allow is None else _dev(lab_allow)


class Pools(object):
    """pools in the top-N layout on the device, with the query users and the profiles of SHARE's history"""

    def __init__(self, cnt, item, plain, decay, user=None, prof=None):
        self.host = (cnt, item, plain, decay, user)
        self.Q, self.n_pool = item.shape
        self.cnt, self.item = _dev(cnt, np.int32), _dev(item, np.int32)
        self.plain, self.decay = _dev(plain, np.float64), _dev(decay, np.float64)
        self.user = None if user is None else _dev(user, np.int32)
        self.n_users = 0 if prof is None else len(prof[0]) - 1
        self.p_ptr = None if prof is None else _dev(prof[0], np.int64)
        self.p_item = None if prof is None else _dev(prof[1], np.int32)


def quota_pool_rc(Pl, L, n_top, mode, cap=1, lab_cap=None, lab_weight=None, stats=True, n_pool=None, rank_by=0, history=True):
    """xmap_quota_pool: (rc, message, Outs, stats [4] or None).  lab_cap / lab_weight: device tensors or None"""
    import torch
    from xmap.engine import hipabi as abi
    O = Outs(Pl.Q, max(n_top, 1))
    h = (C.c_int64 * 4)(*([-7] * 4)) if stats else None
    st = C.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)
    hist = history and Pl.user is not None
    rc = abi.lib.xmap_quota_pool(st, abi.i64(Pl.Q), abi.i32(Pl.n_pool if n_pool is None else n_pool), abi.vp(Pl.cnt), abi.vp(Pl.item),
                                 abi.vp(Pl.plain), abi.vp(Pl.decay), abi.i32(rank_by), abi.i32(mode), abi.i32(cap), abi.vp(lab_cap),
                                 abi.vp(lab_weight), abi.vp(Pl.user if hist else None), abi.i64(Pl.n_users if hist else 0),
                                 abi.vp(Pl.p_ptr if hist else None), abi.vp(Pl.p_item if hist else None), abi.i32(L.n_items),
                                 abi.i32(L.n_labels), abi.vp(L.ptr), abi.vp(L.id), abi.vp(L.allow), abi.i32(n_top),
                                 *([abi.vp(t) for t in O.t] + [h]))
    torch.cuda.synchronize()
    return rc, (abi.lib.xmap_last_error() or b"").decode(), O, None if h is None else [int(x) for x in h]


def quota_pool(*a, **kw):
    rc, msg, O, h = quota_pool_rc(*a, **kw)
    assert rc == 0, msg
    got, guards = O.host()
    assert guards
    return got, h


def quota_rows_rc(D, U, I, keep, n_w, queries, L, n_pool, n_top, rank_by, flags, mode, cap=1, lab_cap=None, lab_weight=None, filt=NO_FILTER,
                  alpha=1.5):
    """xmap_quota_rows on an OnDevice of (ptr, item, rating, time, cnt, col, sim, avg): (rc, message, Outs, stats [10])"""
    import torch
    from xmap.engine import hipabi as abi
    ptr, pit, pra, pti, cnt, col, sim, avg = D.t
    q = _dev(queries, np.int32)
    Q = len(queries)
    w = _dev(wtab(alpha, n_w))
    O = Outs(Q, n_top)
    h = (C.c_int64 * 10)(*([-7] * 10))
    st = C.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)
    F, alive = filt.on_device()
    rc = abi.lib.xmap_quota_rows(st, abi.i64(Q), abi.vp(q), abi.i32(n_top), abi.i32(rank_by), abi.i32(flags), abi.i64(U), abi.i32(I), abi.i32(keep),
                                 abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ptr), abi.vp(pit), abi.vp(pra), abi.vp(pti), abi.vp(avg), abi.vp(w),
                                 abi.i32(n_w), abi.i32(n_pool), abi.i32(mode), abi.i32(cap), abi.vp(lab_cap), abi.vp(lab_weight),
                                 abi.i32(L.n_labels), abi.vp(L.ptr), abi.vp(L.id), abi.vp(L.allow),
                                 *([abi.vp(t) for t in O.t] + [None if F is None else C.byref(F), h]))
    torch.cuda.synchronize()
    del alive
    return rc, (abi.lib.xmap_last_error() or b"").decode(), O, [int(x) for x in h]


def quota_rows(*a, **kw):
    rc, msg, O, h = quota_rows_rc(*a, **kw)
    assert rc == 0, msg
    got, guards = O.host()
    assert guards
    return got, h


@pytest.fixture(scope="module")
def designed():
    """the designed table, its lab_allow, caps, weights and profiles: built and uploaded once"""
    labels, prof = qs.designed_labels(), qs.designed_profiles()
    allow, every = qs.designed_allow(), np.full(qs.N_LABELS // 32, 0xffffffff, np.uint32)
    caps, weights = qs.designed_caps(), qs.designed_weights()
    return dict(labels=labels, prof=prof, allow=allow, every=every, caps=qs.CapOf(caps, 2), weights=weights,
                L=LabelsOnDevice(labels), LA=LabelsOnDevice(labels, allow), LE=LabelsOnDevice(labels, every),
                d_caps=_dev(qs.dense(caps, 2, np.int32)), d_weights=_dev(qs.dense(weights, 0, np.uint32)))


def _variants(d, mode):
    """(statement keywords, device keywords, which labels, h_stats given) of a mode: lab_allow NULL / all / a strict subset,
    lab_cap against the scalar cap, lab_weight against the history, h_stats given and NULL"""
    if mode == CAP:
        return [(dict(lab_cap=d["caps"]), dict(lab_cap=d["d_caps"]), "L", None, True),
                (dict(cap=1), dict(cap=1), "LE", d["every"], True),
                (dict(cap=2), dict(cap=2), "LA", d["allow"], True),
                (dict(lab_cap=d["caps"]), dict(lab_cap=d["d_caps"]), "LA", d["allow"], False)]
    return [(dict(), dict(), "L", None, True),
            (dict(lab_weight=d["weights"]), dict(lab_weight=d["d_weights"]), "LE", d["every"], True),
            (dict(), dict(), "LA", d["allow"], True),
            (dict(lab_weight=d["weights"]), dict(lab_weight=d["d_weights"]), "LA", d["allow"], False)]


# ---------------------------------------------------------------------------- 1. the designed pools against the statement
@pytest.mark.parametrize("mode", [CAP, SHARE], ids=["cap", "share"])
@pytest.mark.parametrize("n_pool", [1, 63, 64, 65, 256, 257, 1024])
def test_designed_pools_against_the_statement(designed, n_pool, mode):
    d = designed
    Q = 5
    cnt, item, plain, decay, user = qs.designed_pool(n_pool, Q)
    assert cnt.min() < 0 and cnt.max() > n_pool and (cnt == 0).any()
    Pl = Pools(cnt, item, plain, decay, user, d["prof"])
    variants = _variants(d, mode)
    seen = [0, 0, 0, 0]
    for k, n_top in enumerate(sorted({1, max(n_pool // 3, 1), n_pool})):
        for v, (skw, dkw, which, allow, with_stats) in enumerate(variants):
            if n_pool >= 256 and v != k and v != 3:      # the wide pools: two variants per n_top, all four over the three
                continue
            want, stats = expected_pool(cnt, item, plain, decay, d["labels"], n_top, mode, lab_allow=allow, query_user=user, prof=d["prof"],
                                        **skw)
            got, h = quota_pool(Pl, d[which], n_top, mode, stats=with_stats, **dkw)
            check_quota_output(got, want, n_top)
            if with_stats:
                print("n_top", n_top, "variant", v, "stats", h, "statement", stats)
                assert tuple(h) == stats
                seen = [a + b for a, b in zip(seen, stats)]
            else:
                assert h is None
    if n_pool >= 63:
        assert seen[0] > 0 and seen[2] > 0       # lists that differ from the prefix; refusals / fills


@pytest.mark.parametrize("Q", [0, 1, 4, 300])
def test_the_number_of_queries(designed, Q):
    d = designed
    n_pool, n_top = 16, 5
    cnt, item, plain, decay, user = qs.designed_pool(n_pool, Q, seed=70)
    Pl = Pools(cnt.reshape(Q), item.reshape(Q, n_pool), plain.reshape(Q, n_pool), decay.reshape(Q, n_pool), user, d["prof"])
    for mode, skw, dkw in ((CAP, dict(lab_cap=d["caps"]), dict(lab_cap=d["d_caps"])), (SHARE, dict(), dict())):
        rc, msg, O, h = quota_pool_rc(Pl, d["L"], n_top, mode, **dkw)
        assert rc == 0, msg
        if Q == 0:
            assert O.untouched() and h == [0, 0, 0, 0]
            continue
        want, stats = expected_pool(cnt, item, plain, decay, d["labels"], n_top, mode, query_user=user, prof=d["prof"], **skw)
        got, guards = O.host()
        assert guards
        check_quota_output(got, want, n_top)
        assert tuple(h) == stats


@pytest.mark.parametrize("mode", [CAP, SHARE], ids=["cap", "share"])
def test_a_pool_of_exactly_max_records(designed, mode):
    """1 024 positions of eight labels each: 8 192 records, the limit"""
    d = designed
    cnt, item, plain, decay, user = qs.designed_pool(1024, 2, eight=True)
    cnt[:] = 1024
    assert sum(len(d["labels"].carried(int(i))) for i in item[0]) == qs.MAX_RECORDS
    Pl = Pools(cnt, item, plain, decay, user, d["prof"])
    for n_top in (40, 1024):
        skw, dkw = (dict(cap=9), dict(cap=9)) if mode == CAP else (dict(lab_weight={l: 1 + l % 5 for l in range(64)}), None)
        if dkw is None:
            dkw = dict(lab_weight=_dev(qs.dense(skw["lab_weight"], 0, np.uint32)))
        want, stats = expected_pool(cnt, item, plain, decay, d["labels"], n_top, mode, **skw)
        got, h = quota_pool(Pl, d["L"], n_top, mode, history=False, **dkw)
        check_quota_output(got, want, n_top)
        assert tuple(h) == stats and stats[0] > 0


def _small_table(per_item, n_labels):
    labels = Labels.of(per_item, n_labels)
    return labels, LabelsOnDevice(labels)


def test_the_hand_checked_cases_and_the_64_bit_products():
    """the hand cases of the issue on the device, and w = {0: 2^31 - 1, 1: 2^30 + 7} over 40 alternating positions: the list of the
    64-bit products, which is not the list 32-bit products give"""
    for per, mode, n_top, rule, positions, claims, third in qs.hand_cases():
        labels, L = _small_table([sorted(l) for l in per], 3)       # (a table's rows ascend; the statement's L(j) is a set)
        m = len(per)
        Pl = Pools(np.asarray([m], np.int32), np.arange(m, dtype=np.int32)[None], np.arange(m, 0, -1.0)[None], np.ones((1, m)))
        kw = dict(cap=rule) if mode == CAP else dict(lab_weight=_dev(np.asarray([rule.get(l, 0) for l in range(3)], np.uint32)))
        got, h = quota_pool(Pl, L, n_top, mode, **kw)
        assert got[0].tolist() == [len(positions)] and got[4][0, :len(positions)].tolist() == positions and h[2] == third
        if claims is not None:
            assert got[5][0, :len(claims)].tolist() == claims
    L40 = qs.alternating()
    labels, L = _small_table([[0], [1]], 2)
    Pl = Pools(np.asarray([40], np.int32), np.asarray([[j & 1 for j in range(40)]], np.int32), np.zeros((1, 40)), np.zeros((1, 40)))
    got, h = quota_pool(Pl, L, 40, SHARE, lab_weight=_dev(np.asarray([qs.W32[0], qs.W32[1]], np.uint32)))
    wide, narrow = qs.share_lists(L40, 40, qs.W32, 64), qs.share_lists(L40, 40, qs.W32, 32)
    assert wide[0] != narrow[0]
    assert got[4][0].tolist() == wide[0] and got[5][0].tolist() == wide[1]


# ------------------------------------------------------------------------------------------------------ 2. identities
def test_identities(designed):
    d = designed
    n_pool, Q = 65, 12
    cnt, item, plain, decay, user = qs.designed_pool(n_pool, Q, seed=90)
    Pl = Pools(cnt, item, plain, decay, user, d["prof"])
    m = np.clip(cnt, 0, n_pool)
    zeros = _dev(np.zeros(qs.N_LABELS, np.uint32))
    for n_top in (1, 20, n_pool):
        for mode, kw in ((CAP, dict(cap=INT32_MAX)), (SHARE, dict(lab_weight=zeros))):
            (o_cnt, o_item, o_plain, o_decay, o_pos, o_label), h = quota_pool(Pl, d["L"], n_top, mode, **kw)
            assert np.array_equal(o_cnt, np.minimum(m, n_top))
            for q in range(Q):
                c = int(o_cnt[q])
                assert o_pos[q, :c].tolist() == list(range(c)) and (o_pos[q, c:] == -1).all()
                assert o_item[q, :c].tobytes() == item[q, :c].tobytes() and (o_item[q, c:] == -1).all()
                assert o_plain[q, :c].tobytes() == plain[q, :c].tobytes() and o_decay[q, :c].tobytes() == decay[q, :c].tobytes()
                if mode == SHARE:
                    assert (o_label[q] == -1).all()
            assert h[0] == 0 and h[1] == int(o_cnt.sum()) and h[2] == (0 if mode == CAP else h[1]) and h[3] == 0
    # shuffling the queries permutes the outputs and changes nothing else
    perm = np.random.default_rng(3).permutation(Q)
    Ps = Pools(cnt[perm], item[perm], plain[perm], decay[perm], user[perm], d["prof"])
    for mode, kw in ((CAP, dict(lab_cap=d["d_caps"])), (SHARE, dict())):
        a, ha = quota_pool(Pl, d["L"], 20, mode, **kw)
        b, hb = quota_pool(Ps, d["L"], 20, mode, **kw)
        assert [x[perm].tobytes() for x in a] == [x.tobytes() for x in b] and ha == hb and ha[0] > 0


# ------------------------------------------------------------------- 3. refusals: an error, a message, untouched outputs
def test_refusals_leave_every_byte(designed):
    import shelf_statement as ss
    from xmap.engine import hipabi as abi
    d = designed
    labels = d["labels"]
    cnt, item, plain, decay, user = qs.designed_pool(64, 4)
    Pl = Pools(cnt, item, plain, decay, user, d["prof"])
    good = (labels.ptr.copy(), labels.id.copy())
    two = int(np.flatnonzero(np.diff(labels.ptr) >= 2)[0])
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

    # a bad label table: the shelves' rules and messages
    for change, rule, word in ((first, "lab_ptr", "lab_ptr"), (decreasing, "lab_ptr", "lab_ptr"), (too_large, "range", "out of range"),
                               (negative, "range", "out of range"), (equal, "ascending", "strictly ascending"),
                               (descending, "ascending", "strictly ascending")):
        bad = table(change)
        what = ss.check_tables(bad.n_items, bad.n_labels, bad.ptr, bad.id)
        assert what is not None and what[0] == rule
        for mode in (CAP, SHARE):
            rc, msg, O, h = quota_pool_rc(Pl, LabelsOnDevice(bad), 10, mode)
            assert rc == abi.ERR_ARG and word in msg and "[%d]" % what[1] in msg, msg
            assert O.untouched() and h == [-7] * 4
    # a negative lab_cap entry: the message names the first label
    caps = qs.dense(qs.designed_caps(), 2, np.int32)
    caps[[40, 12345, 17]] = [-1, -3, -2147483648]
    rc, msg, O, h = quota_pool_rc(Pl, d["L"], 10, CAP, lab_cap=_dev(caps))
    assert rc == abi.ERR_ARG and "lab_cap" in msg and "[17]" in msg, msg
    assert O.untouched() and h == [-7] * 4
    # n_pool x the longest label row above the limit: a property of the table, whatever the pools hold
    nine = Labels.of([[0]] * 30 + [list(range(9))] + [[1]] * 9, 9)
    L9 = LabelsOnDevice(nine)
    for n_pool, ok in ((1024, False), (911, False), (910, True)):
        cnt = np.full(2, n_pool, np.int32)
        items = np.zeros((2, n_pool), np.int32)          # (no pool holds the nine-label item)
        items[1, ::2] = 35
        P9 = Pools(cnt, items, np.zeros((2, n_pool)), np.zeros((2, n_pool)))
        rc, msg, O, h = quota_pool_rc(P9, L9, 10, CAP, cap=3)
        if ok:
            assert rc == 0, msg
            want, stats = expected_pool(cnt, items, np.zeros((2, n_pool)), np.zeros((2, n_pool)), nine, 10, CAP, cap=3)
            check_quota_output(O.host()[0], want, 10)
            assert tuple(h) == stats
        else:
            assert rc == abi.ERR_ARG and "n_pool = %d" % n_pool in msg and "9" in msg and "8192" in msg, msg
            assert O.untouched() and h == [-7] * 4
    # the host checks of the fine-grained call
    for kw, word in ((dict(n_top=0), "n_top"), (dict(n_top=65), "n_top"), (dict(mode=2), "mode"), (dict(cap=0), "cap"),
                     (dict(rank_by=2), "rank_by"), (dict(n_pool=1025), "n_pool")):
        a = dict(n_top=10, mode=CAP)
        a.update(kw)
        rc, msg, O, h = quota_pool_rc(Pl, d["L"], **a)
        assert rc == abi.ERR_ARG and word in msg and O.untouched(), msg
    rc, msg, O, h = quota_pool_rc(Pl, d["L"], 10, SHARE, history=False)       # SHARE with neither weights nor a history
    assert rc == abi.ERR_ARG and "lab_weight" in msg and O.untouched(), msg


# ------------------------------------------------------------------------------ 4. xmap_quota_rows on the small models
class Case(object):
    def __init__(self, arrays, U, I, keep):
        self.arrays, self.U, self.I, self.keep = arrays, U, I, keep
        self.D = OnDevice(arrays)
        self.prof = (arrays[0], arrays[1])


@pytest.fixture(scope="module")
def hand():
    arrays, U, I, keep, _ = _hand_case()
    return Case(arrays, U, I, keep)


@pytest.fixture(scope="module")
def rand():
    U, I, keep = 50, 400, 5
    return Case(_random_case(24, U, I, keep, np.arange(0, I, 3), lambda u: 2 + u % 9), U, I, keep)


@pytest.fixture(scope="module")
def wide():
    """users whose kept candidates number far more than 64: every item has a list, the profiles are long"""
    U, I, keep = 16, 1500, 5
    return Case(_random_case(31, U, I, keep, np.arange(I), lambda u: 2 + (u % 6) * 40), U, I, keep)


def _seven_labels(I, seed=2):
    """7 labels: every third item carries two, some carry none (the table of the shelf tests)"""
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


SEVEN_CAPS = np.asarray([1, 0, 2, 3, INT32_MAX, 1, 2], np.int32)
SEVEN_WEIGHTS = np.asarray([5, 0, 5, 1, 0, 2, 9], np.uint32)


def _rows_settings(c, queries):
    allow, exclude = _rules(c, queries)
    lab_allow = np.asarray([1, 1, 0, 1, 1, 1, 0], bool)
    return ((10, 0, 0, CAP, dict(cap=2), None, NO_FILTER),
            (5, 1, KEEP_HELD, CAP, dict(lab_cap=SEVEN_CAPS), lab_allow, Filter(allow=allow, exclude=exclude, min_score=3.0)),
            (10, 0, 0, SHARE, dict(), None, NO_FILTER),
            (7, 1, 0, SHARE, dict(lab_weight=SEVEN_WEIGHTS), lab_allow, Filter(exclude=exclude)),
            (10, 0, KEEP_HELD, SHARE, dict(), lab_allow, Filter(allow=allow, min_score=2.5)))


def _on_device(kw):
    return {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}


@pytest.mark.parametrize("which", ["hand", "rand"])
def test_quota_rows_against_the_statement(which, hand, rand):
    c = hand if which == "hand" else rand
    queries = list(range(c.U)) + [c.U + 5, -1, 3]
    scored = score_users(1.5, queries, *c.arrays[:8], c.keep)
    labels = _seven_labels(c.I)
    for n_pool in (30, 64):
        for n_top, rank_by, flags, mode, kw, la, filt in _rows_settings(c, queries):
            want, stats = expected_quota(scored, queries, labels, n_pool, n_top, rank_by, bool(flags), 66, mode, lab_allow=la, prof=c.prof,
                                         **kw, **({} if filt.null else filt.statement()))
            got, h = quota_rows(c.D, c.U, c.I, c.keep, 66, queries, LabelsOnDevice(labels, la), n_pool, n_top, rank_by, flags, mode, filt=filt,
                                **_on_device(kw))
            check_quota_output(got, want, n_top)
            print("stats", h, "statement", stats)
            assert tuple(h) == stats
            assert h[7] > 0


def test_quota_rows_with_a_pool_of_300(wide):
    c = wide
    queries = list(range(c.U)) + [c.U, 2]
    scored = score_users(1.5, queries, *c.arrays[:8], c.keep)
    labels = _seven_labels(c.I)
    pools = []
    expected_quota(scored, queries, labels, 300, 10, 0, False, 66, CAP, cap=1, pools=pools)
    assert sum(k > 64 for k, _ in pools) >= 4 and sum(k > 300 for k, _ in pools) >= 1 and sum(64 < k < 300 for k, _ in pools) >= 1
    allow, exclude = _rules(c, queries)
    for n_top, rank_by, mode, kw, filt in ((10, 0, CAP, dict(cap=1), NO_FILTER), (300, 0, CAP, dict(lab_cap=np.asarray([20, 0, 40, 60, INT32_MAX, 20, 40], np.int32)), NO_FILTER),
                                           (100, 1, CAP, dict(cap=15), Filter(allow=allow, exclude=exclude, min_score=2.0)),
                                           (10, 0, SHARE, dict(), NO_FILTER), (120, 1, SHARE, dict(lab_weight=SEVEN_WEIGHTS), Filter(exclude=exclude)),
                                           (300, 0, SHARE, dict(), Filter(allow=allow))):
        want, stats = expected_quota(scored, queries, labels, 300, n_top, rank_by, False, 66, mode, prof=c.prof, **kw,
                                     **({} if filt.null else filt.statement()))
        got, h = quota_rows(c.D, c.U, c.I, c.keep, 66, queries, LabelsOnDevice(labels), 300, n_top, rank_by, 0, mode, filt=filt, **_on_device(kw))
        check_quota_output(got, want, n_top)
        print("stats", h, "statement", stats)
        assert tuple(h) == stats


@pytest.mark.parametrize("which", ["hand", "rand"])
def test_quota_rows_is_quota_pool_over_the_filtered_top_n(which, hand, rand):
    """for n_pool <= 64 the pool is by definition what xmap_topn_rows_filtered returns with n_top = n_pool"""
    c = hand if which == "hand" else rand
    queries = list(range(c.U)) + [c.U + 5, -1, 3, 3]
    labels = _seven_labels(c.I)
    qu = np.asarray(queries, np.int32)
    for n_pool in (1, 17, 64):
        for n_top, rank_by, flags, mode, kw, la, filt in _rows_settings(c, queries):
            n_top = min(n_top, n_pool)
            L = LabelsOnDevice(labels, la)
            ref = topn_f(c.D, c.U, c.I, c.keep, 66, queries, n_pool, rank_by, flags, filt)
            Pl = Pools(ref[0], ref[1].reshape(len(queries), n_pool), ref[2].reshape(len(queries), n_pool),
                       ref[3].reshape(len(queries), n_pool), qu, c.prof)
            back, hb = quota_pool(Pl, L, n_top, mode, rank_by=rank_by, **_on_device(kw))
            got, h = quota_rows(c.D, c.U, c.I, c.keep, 66, queries, L, n_pool, n_top, rank_by, flags, mode, filt=filt, **_on_device(kw))
            assert [a.tobytes() for a in got] == [a.tobytes() for a in back]
            assert h[:6] == list(ref[4]) and h[6:] == hb
        # no cap at all and n_pool = n_top: the lists of the filtered top-N
        allow, exclude = _rules(c, queries)
        filt = Filter(allow=allow, exclude=exclude, min_score=3.0)
        ref = topn_f(c.D, c.U, c.I, c.keep, 66, queries, n_pool, 1, KEEP_HELD, filt)
        got, h = quota_rows(c.D, c.U, c.I, c.keep, 66, queries, LabelsOnDevice(labels), n_pool, n_pool, 1, KEEP_HELD, CAP, cap=INT32_MAX, filt=filt)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
        assert got[2].tobytes() == ref[2].tobytes() and got[3].tobytes() == ref[3].tobytes()
        assert h[:6] == list(ref[4]) and h[6] == 0 and h[8] == 0


# ------------------------------------------------------------------------------ 5. the coarse entry over the three sources
def _ctx_quota(ctx, source, queries, n_pool, n, rank_by, flags, mode, cap=1, lab_cap=None, lab_weight=None, lab_allow=None, F=None, n_w=66,
               alpha=1.5):
    """xmap_ctx_recommend_quota: (rc, message, the six outputs pre-filled with -7, stats [10])"""
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    outs = [np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32), np.full((Q, n), -7.0), np.full((Q, n), -7.0),
            np.full((Q, n), -7, np.int32), np.full((Q, n), -7, np.int32)]
    stats = np.full(10, -7, np.int64)
    words = None if lab_allow is None else _words(lab_allow)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = ctx.lib.xmap_ctx_recommend_quota(ctx.h, source, Q, _p(q, C.c_int32), n_pool, n, rank_by, flags, _p(w, C.c_double), n_w, mode, cap,
                                          vp(lab_cap), vp(lab_weight), vp(words),
                                          *([o.ctypes.data_as(C.c_void_p) for o in outs] + [None if F is None else C.byref(F), _p(stats, C.c_int64)]))
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


def test_the_coarse_call_over_the_three_sources():
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
        T = rec_sim(ctx, I, U, len(rows["user"]))
        cnt, col, sim, _ = select(ctx, I, keep)
        # without labels: an error that says so, nothing written
        rc, msg, got, stats = _ctx_quota(ctx, 0, np.arange(5), 20, 5, 0, 0, CAP)
        assert rc == abi.ERR_ARG and "labels" in msg and all((o == -7).all() for o in got) and stats == [-7] * 10
        assert _set_labels(ctx, labels) == 0
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
        # ---- resident and fold-in: the fine-grained call on the same arrays, byte for byte
        for source, (n_users, prof, qs_) in {0: (U, (T["ptr"], T["item"], T["rating"], T["time"]), np.arange(-1, 200)),
                                             1: (B, fold, np.arange(-1, B + 1))}.items():
            D = OnDevice(list(prof) + [cnt, col, sim, T["avg"]])
            qs_ = np.concatenate([qs_, qs_[5:8]]).astype(np.int32)
            exclude = [rng.integers(-2, I + 2, int(rng.integers(0, 9))).tolist() for _ in qs_]
            filt = Filter(allow=rng.random(I) < 0.7, exclude=exclude, min_score=2.5)
            for n_pool, n, rank_by, flags, mode, kw, la, f in ((40, 10, 0, 0, CAP, dict(cap=2), None, NO_FILTER),
                                                               (300, 12, 1, KEEP_HELD, CAP, dict(lab_cap=SEVEN_CAPS), lab_allow, filt),
                                                               (64, 10, 0, 0, SHARE, dict(), lab_allow, filt),
                                                               (300, 30, 1, 0, SHARE, dict(lab_weight=SEVEN_WEIGHTS), None, NO_FILTER)):
                F, alive = f.on_host()
                rc, msg, got, stats = _ctx_quota(ctx, source, qs_, n_pool, n, rank_by, flags, mode, lab_allow=la, F=F, **kw)
                assert rc == 0, msg
                ref, h = quota_rows(D, n_users, I, keep, 66, qs_, LabelsOnDevice(labels, la), n_pool, n, rank_by, flags, mode, filt=f,
                                    **_on_device(kw))
                assert [a.tobytes() for a in got] == [a.tobytes() for a in ref] and stats == h
                assert stats[7] > 0 and stats[6] > 0
        # ---- item fold-in: the batch items carry no label -- under cap 0 for every label exactly they remain
        qs_ = np.arange(0, 150).astype(np.int32)
        plain = _ctx_filtered(ctx, 2, qs_, 64, 0, 0)
        assert (plain[1] >= I).any()                                 # batch items are candidates of the plain call
        unlabelled = np.concatenate([np.diff(labels.ptr) == 0, np.ones(NB, bool)])
        words = _words(unlabelled)
        ref = _ctx_filtered(ctx, 2, qs_, 10, 0, 0, abi.RecFilter(words.ctypes.data, None, None, -np.inf))
        rc, msg, got, stats = _ctx_quota(ctx, 2, qs_, 300, 10, 0, 0, CAP, lab_cap=np.zeros(7, np.int32))
        assert rc == 0, msg
        small = plain[0] < 64                                        # (the whole candidate list fits the pool of 300 for certain)
        assert small.any()
        assert got[0][small].tobytes() == ref[0][small].tobytes() and got[1][small].tobytes() == ref[1][small].tobytes()
        assert got[2][small].tobytes() == ref[2][small].tobytes() and (got[5] == -1).all()
        # ---- the extended table beside a lab_allow: with every label allowed the same statement holds; no queries: the stats zeroed
        few = qs_[np.flatnonzero(small)[:8]]
        ref = _ctx_filtered(ctx, 2, few, 4, 0, 0, abi.RecFilter(words.ctypes.data, None, None, -np.inf))
        rc, msg, got, stats = _ctx_quota(ctx, 2, few, 300, 4, 0, 0, CAP, lab_cap=np.zeros(7, np.int32), lab_allow=np.ones(7, bool))
        assert rc == 0, msg
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
        assert got[2].tobytes() == ref[2].tobytes() and (got[5] == -1).all()
        rc, msg, got, stats = _ctx_quota(ctx, 2, few[:0], 300, 4, 0, 0, CAP, lab_allow=np.ones(7, bool))
        assert rc == 0 and stats == [0] * 10, msg
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------- 6. the Python routes
def test_engine_quota_on_tensors(rand, designed):
    import torch
    from xmap.engine import device
    from types import SimpleNamespace
    c, d = rand, designed
    eng = device.Engine(SimpleNamespace(device=torch.device("cuda:0"), n_items=c.I))
    ptr, pit, pra, pti, cnt, col, sim, avg = c.D.t
    P = SimpleNamespace(n_users=c.U, n_items=c.I, user_ptr=ptr, user_item=pit, user_rating64=pra, user_time=pti)
    queries = list(range(c.U)) + [c.U + 5, 3]
    seven = _seven_labels(c.I)
    lab_allow = np.asarray([1, 1, 0, 1, 1, 1, 0], bool)
    allow, exclude = _rules(c, queries)
    filt = Filter(allow=allow, exclude=exclude, min_score=3.0)
    F, alive = filt.on_device()
    T7 = eng.set_labels(c.I, 7, seven.ptr, seven.id)
    d_q, d_w = _dev(queries, np.int32), _dev(wtab(1.5, 66))
    out = eng.quota_topn(P, (cnt, col, sim), d_q, avg, d_w, T7, 40, 5, "cap", lab_cap=SEVEN_CAPS, lab_allow=torch.from_numpy(lab_allow),
                         rank_by=1, keep_held=True, allow=alive[0], exclude=(alive[1], alive[2]), min_score=3.0)
    ref, h = quota_rows(c.D, c.U, c.I, c.keep, 66, queries, LabelsOnDevice(seven, lab_allow), 40, 5, 1, KEEP_HELD, CAP, lab_cap=_dev(SEVEN_CAPS),
                        filt=filt)
    assert [x.cpu().numpy().tobytes() for x in out[:6]] == [a.tobytes() for a in ref] and list(out[6]) == h and h[7] > 0
    out = eng.quota_topn(P, (cnt, col, sim), d_q, avg, d_w, T7, 64, 10, "share")
    ref, h = quota_rows(c.D, c.U, c.I, c.keep, 66, queries, LabelsOnDevice(seven), 64, 10, 0, 0, SHARE)
    assert [x.cpu().numpy().tobytes() for x in out[:6]] == [a.tobytes() for a in ref] and list(out[6]) == h
    # quota_pool over what topn() returned: the same lists again (n_pool <= 64)
    pool = eng.topn(P, (cnt, col, sim), d_q, avg, d_w, 64)
    for mode, name, kw in ((SHARE, "share", dict(P=P, query_user=d_q)), (SHARE, "share", dict(lab_weight=SEVEN_WEIGHTS)),
                           (CAP, "cap", dict(cap=2))):
        back = eng.quota_pool(pool, T7, 10, name, **kw)
        dkw = {k: _dev(v) for k, v in kw.items() if k == "lab_weight"}
        ref, h = quota_rows(c.D, c.U, c.I, c.keep, 66, queries, LabelsOnDevice(seven), 64, 10, 0, 0, mode, cap=kw.get("cap", 1), **dkw)
        assert [x.cpu().numpy().tobytes() for x in back[:6]] == [a.tobytes() for a in ref] and list(back[6]) == h[6:]
    # the designed pools through the Engine
    labels = d["labels"]
    T = eng.set_labels(labels.n_items, labels.n_labels, labels.ptr, labels.id)
    cnt_, item, plain, decay, user = qs.designed_pool(65, 6)
    lists = (_dev(cnt_, np.int32), _dev(item, np.int32), _dev(plain), _dev(decay))
    out = eng.quota_pool(lists, T, 20, "cap", lab_cap=d["d_caps"], lab_allow=d["allow"])
    want, stats = expected_pool(cnt_, item, plain, decay, labels, 20, CAP, lab_cap=d["caps"], lab_allow=d["allow"])
    check_quota_output([x.cpu().numpy() for x in out[:6]], want, 20)
    assert out[6] == stats
    for bad in (dict(mode="median"), dict(n_top=66), dict(cap=0), dict(mode="share")):
        a = dict(n_top=20, mode="cap")
        a.update(bad)
        with pytest.raises(ValueError):
            eng.quota_pool(lists, T, **a)


def test_session_recommend_quota_on_id_strings():
    """the set-up of the shelves' session test.  With pool <= 64 the pool of a user is by definition the list recommend_topn returns
    with n = pool: the quota lists are the statement's loops over those lists on id strings; the history of a user is the rows of
    the AlterEgo profile per item, from the collected item-based profile"""
    import datetime
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from golden_util import CAP as SIM_CAP
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
    tool = BaselinerSim("cosine", SIM_CAP)
    sim = baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
    ae = generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True)
    rng = np.random.default_rng(9)
    uids = [recs[int(x)][0] for x in rng.integers(0, len(recs), 40)] + ["A%013d" % (10 ** 9 + 1)]
    item_based = RecommenderSim("cosine_item", SIM_CAP).build_sthbased_profile(ae, "item").collectAsMap()
    alpha = 1.5
    all_iids = sorted({i for _, prof in recs for i, _, _ in prof})
    names = ["cat%d" % k for k in range(6)]
    by_iid = {}
    for k, iid in enumerate(all_iids):          # unsorted and repeated names, items without a label, an iid nobody knows
        if k % 7 != 3:
            by_iid[iid] = [names[(k * 5 + 2) % 6], names[k % 6], names[k % 6]] if k % 3 == 0 else [names[k % 6]]
    by_iid["no-such-item"] = ["ghost"]
    held = {uid: {} for uid in uids}            # uid -> {label name: rows of the AlterEgo profile}
    for iid, lst in item_based.items():
        for who, ra, when in lst:
            if who in held:
                for name in set(by_iid.get(iid, ())):
                    held[who][name] = held[who].get(name, 0) + 1
    pool = 64
    base = session.recommend_topn(ae, uids, SIM_CAP, 10, alpha, pool).collect()

    def statement(n, mode, governed, cap_of=None, weights=None):
        out = []
        for (uid, lst) in base:
            L = [sorted(x for x in set(by_iid.get(iid, ())) if x in governed) for iid, _, _ in lst]
            if mode == "cap":
                pos = qs.cap_lists(L, n, cap_of)[0]
                claims = [L[j][0] if L[j] else None for j in pos]
            else:
                w = weights if weights is not None else {x: k for x, k in held[uid].items() if x in governed}
                pos, claims = qs.share_lists(L, n, w)[:2]
                claims = [None if x == -1 else x for x in claims]
            out.append((uid, [lst[j] + (claims[k],) for k, j in enumerate(pos)]))
        return out

    first = session.recommend_quota(ae, uids, SIM_CAP, 10, alpha, by_iid, 10, pool, at_most=2)
    assert first.label_names == names and first.collect() == statement(10, "cap", set(names), lambda l: 2)
    assert first.collect()[-1] == (uids[-1], []) and first.stats[6] > 0 and first.cut_short == first.stats[9]
    per = {"cat0": 0, "cat3": 1}
    out = session.recommend_quota(ae, LocalRDD(uids), SIM_CAP, 10, alpha, LocalRDD(list(by_iid.items())), 8, pool, per_label=per, at_most=3,
                                  allow_labels=names[:5])
    assert out.collect() == statement(8, "cap", set(names[:5]), lambda l: per.get(l, 3))
    cal = session.recommend_quota(ae, uids, SIM_CAP, 10, alpha, by_iid, 10, pool, mode="share")
    assert cal.collect() == statement(10, "share", set(names)) and cal.stats[6] > 0
    mix = {"cat1": 3, "cat4": 1}
    out = session.recommend_quota(ae, uids, SIM_CAP, 10, alpha, by_iid, 12, pool, mode="share", weights=mix, allow_labels=names[1:])
    assert out.collect() == statement(12, "share", set(names[1:]), weights=mix)
    for kw in (dict(per_label={"ghost": 1}), dict(mode="share", weights={"nobody": 2}), dict(allow_labels=["cat9"])):
        with pytest.raises(ValueError):
            session.recommend_quota(ae, uids, SIM_CAP, 10, alpha, by_iid, 10, pool, **kw)
    # fold-in: profiles outside the train set; the pool is recommend_topn_profiles' list, the history the folded-in profile's rows
    late = [("late-%d" % k, list(recs[int(x)][1])) for k, x in enumerate(rng.integers(0, len(recs), 8))]
    base = session.recommend_topn_profiles(ae, late, SIM_CAP, 10, alpha, pool).collect()
    page = session.recommend_quota_profiles(ae, late, SIM_CAP, 10, alpha, by_iid, 10, pool, at_most=1)
    assert [uid for uid, _ in page.collect()] == [uid for uid, _ in late] and page.unknown_items == 0
    assert page.collect() == statement(10, "cap", set(names), lambda l: 1) and page.stats[6] > 0
    zero = session.recommend_quota_profiles(ae, late, SIM_CAP, 10, alpha, by_iid, 10, pool, mode="share", weights={"cat2": 0})
    assert [(uid, [e[:3] for e in lst]) for uid, lst in zero.collect()] == [(uid, lst[:10]) for uid, lst in base]
    assert all(e[3] is None for _, lst in zero.collect() for e in lst)
