"""The allotment on the device (csrc/stage_e_allot.hip; xmap_allot_pool, xmap_allot_rows, xmap_ctx_recommend_allot,
Engine.allot_pool / allot_topn) against tests/allot_statement.py.  Everything is exact: integers with array_equal, doubles through
uint64 views.  The outputs are pre-filled with -7 and allocated with guard elements behind them that must survive.  The plain
round schedule is built (no threshold cut), so the rounds of the statement are asserted too."""
import ctypes as C

import numpy as np
import pytest

import allot_statement as al
from allot_statement import FAMILIES, INT32_MAX, Pool, allot_rounds, check_allot_output, held_mask, is_stable
from test_gpu_audience import OnDevice
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_filter import Filter, topn_f
from test_gpu_tail import _few_times, generate, rec_sim, select, wtab
from test_gpu_topn import KEEP_HELD, _hand_case, _random_case

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
    """cnt, item, plain, decay, pos and item_taken as flat device tensors of -7 with GUARD elements behind each"""
    DT = ("i", "i", "d", "d", "i", "i")

    def __init__(self, Q, n_top, n_items):
        import torch
        self.shapes = [(Q,)] + [(Q, n_top)] * 4 + [(n_items,)]
        self.t = [torch.full((int(np.prod(s)) + GUARD,), -7, dtype=torch.int32 if k == "i" else torch.float64, device="cuda:0")
                  for s, k in zip(self.shapes, self.DT)]

    def host(self):
        """(the six arrays, every guard element still -7)"""
        flat = [t.cpu().numpy() for t in self.t]
        return [f[:-GUARD].reshape(s) for f, s in zip(flat, self.shapes)], all((f[-GUARD:] == -7).all() for f in flat)

    def untouched(self):
        return all((t.cpu().numpy() == -7).all() for t in self.t)


class DevPool(object):
    def __init__(self, pool):
        self.pool = pool
        self.cnt, self.item, self.plain, self.decay = _dev(pool.cnt), _dev(pool.item), _dev(pool.plain), _dev(pool.decay)


def allot_pool_rc(D, n_top, cap=1, item_cap=None, rank_by=0, stats=True, taken=True, n_query=None, n_pool=None, n_items=None):
    """xmap_allot_pool: (rc, message, Outs, stats [6] or None).  item_cap: a host array or None"""
    import torch
    from xmap.engine import hipabi as abi
    p = D.pool
    I = p.n_items if n_items is None else n_items
    O = Outs(p.Q, max(min(n_top, p.n_pool), 1), max(I, 0))
    h = (C.c_int64 * 6)(*([-7] * 6)) if stats else None
    st = C.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)
    d_cap = None if item_cap is None else _dev(item_cap, np.int32)
    rc = abi.lib.xmap_allot_pool(st, abi.i64(p.Q if n_query is None else n_query), abi.i32(p.n_pool if n_pool is None else n_pool),
                                 abi.vp(D.cnt), abi.vp(D.item), abi.vp(D.plain), abi.vp(D.decay), abi.i32(rank_by), abi.i32(I), abi.i32(cap),
                                 abi.vp(d_cap), abi.i32(n_top), *([abi.vp(t) for t in O.t[:5]] + [abi.vp(O.t[5]) if taken else None, h]))
    torch.cuda.synchronize()
    return rc, (abi.lib.xmap_last_error() or b"").decode(), O, None if h is None else [int(x) for x in h]


def allot_pool(*a, **kw):
    rc, msg, O, h = allot_pool_rc(*a, **kw)
    assert rc == 0, msg
    got, guards = O.host()
    assert guards
    return got, h


def same_lists(got, R):
    for g, w in zip(got[:5], R.lists()):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert g.tobytes() == w.tobytes()


def run_and_check(pool, n_top, cap=1, item_cap=None, rank_by=0, D=None, qid=None):
    """the device against the round statement: lists, item_taken, the six stats; the layout; stability"""
    got, h = allot_pool(D or DevPool(pool), n_top, cap, item_cap, rank_by)
    R = allot_rounds(pool, n_top, cap, item_cap, rank_by)
    check_allot_output(pool, n_top, got[:5])
    same_lists(got, R)
    assert np.array_equal(got[5], R.taken)
    assert np.array_equal(got[5], np.bincount(got[1][got[1] >= 0], minlength=pool.n_items))
    print("stats", h, "statement", R.stats)
    assert h == R.stats
    assert is_stable(pool, n_top, held_mask(pool, got[0], got[4]), cap, item_cap, rank_by)
    return got, h, R


QS = (1, 63, 64, 65, 257)
N_POOLS = (1, 31, 32, 33, 63, 64, 65, 1024)


def _cap_route(k, pool):
    """(cap, item_cap) number k: the scalar route with 1, 2 and INT32_MAX, the array route with every kind of entry"""
    return [(1, None), (2, None), (1, al.designed_caps(pool.n_items, 40 + k)), (INT32_MAX, None)][k % 4]


# ------------------------------------------------------------------------------------------ 1. xmap_allot_pool on the designed pools
@pytest.mark.parametrize("top", ["one", "all"])
@pytest.mark.parametrize("n_pool", N_POOLS)
def test_designed_pools_against_the_statement(n_pool, top):
    """the word and wave edges of the bitmap; every Q with a score family and a cap route that rotate with the shape"""
    n_top = 1 if top == "one" else n_pool
    a = N_POOLS.index(n_pool) + (3 if top == "all" else 0)
    refused = 0
    for k, Q in enumerate(QS):
        pool = al.designed_pool(Q, n_pool, FAMILIES[(a + k) % 5], 100 * a + k)
        cap, item_cap = _cap_route(a + k, pool)
        got, h, R = run_and_check(pool, n_top, cap, item_cap, rank_by=0)
        refused += h[2]
        if cap == INT32_MAX and item_cap is None:
            assert h[2] == 0 and h[4] == 1
    assert refused > 0 or n_pool == 1


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("Q", QS)
def test_every_family_at_every_number_of_queries(Q, family):
    pool = al.designed_pool(Q, 33, family, 7 * Q + len(family))
    for k, n_top in enumerate((1, 5, 33)):
        cap, item_cap = _cap_route(k + Q, pool)
        run_and_check(pool, n_top, cap, item_cap)
    # the decayed column ranks under rank_by 1
    run_and_check(pool, 5, 1, None, rank_by=1)


def test_void_positions_of_every_kind():
    pool = al.designed_pool(65, 65, "descending_random", 11)
    caps = al.designed_caps(pool.n_items, 12)
    assert (pool.item == -1).any() and (pool.item == pool.n_items).any() and (pool.cnt < 0).any() and (pool.cnt > 65).any()
    assert (caps == 0).any() and (caps == INT32_MAX).any()
    got, h, R = run_and_check(pool, 10, 1, caps)
    assert h[3] > 0 and h[2] > 0
    got, h, R = run_and_check(pool, 65, 1, caps)
    assert h[5] > 0
    # every item barred: every list is empty, nothing is refused
    got, h, R = run_and_check(pool, 10, 1, np.zeros(pool.n_items, np.int32))
    assert (got[0] == 0).all() and h[1] == 0 and h[2] == 0 and h[4] == 1 and (got[5] == 0).all()
    # an id space of no items
    empty = Pool(pool.cnt, pool.item, pool.plain, pool.decay, 0)
    got, h, R = run_and_check(empty, 10, 1)
    assert (got[0] == 0).all() and got[5].shape == (0,)


def test_a_repeated_item_inside_a_pool_is_two_positions():
    pool = al.designed_pool(9, 33, "negative", 6, n_items=12, repeat=True)
    assert any(len(set(r)) < len(r) for r in pool.item.tolist())
    for n_top, cap in ((1, 1), (5, 2), (33, 3)):
        run_and_check(pool, n_top, cap)
    got, h, R = run_and_check(pool, 33, INT32_MAX)
    assert any(len(set(r[:c])) < c for r, c in zip(got[1].tolist(), got[0].tolist()))


def test_crowd_a_run_and_a_cap_above_1024():
    pool = al.crowd_pool()
    got, h, R = run_and_check(pool, 2, 1100)
    assert got[5][0] == 1100 and h[2] == 400 and h[4] == 2
    item_cap = np.full(pool.n_items, 1, np.int32)
    item_cap[0] = 1100
    got2, h2, _ = run_and_check(pool, 2, 1, item_cap)
    assert [a.tobytes() for a in got2] == [a.tobytes() for a in got] and h2 == h


def test_ladder_walks_across_the_words_and_waves_of_a_pool_of_1024():
    pool = al.ladder_pool(257, 1024)
    got, h, R = run_and_check(pool, 1, 1)
    assert got[4][:, 0].tolist() == list(range(257)) and h[4] == 257
    got, h, R = run_and_check(pool, 3, 2)
    assert h[2] > 0 and h[4] > 64
    small = al.ladder_pool(65, 33)              # more queries than positions: the last ones end with nothing
    got, h, R = run_and_check(small, 1, 1)
    assert got[0].tolist() == [1] * 33 + [0] * 32 and h[5] == 32


def test_chain_takes_as_many_rounds_as_queries():
    pool = al.chain_pool(64)
    got, h, R = run_and_check(pool, 1, 1)
    assert got[4][:, 0].tolist() == [0] + [1] * 63
    assert h[4] == 64 and h[2] == 63


# ----------------------------------------------------------------------------------------------------------------- 2. identities
def test_byte_identity_under_permuted_queries_and_swapped_columns():
    rng = np.random.RandomState(21)
    for family in ("descending_random", "all_equal"):
        pool = al.designed_pool(257, 33, family, 22)
        caps = al.designed_caps(pool.n_items, 23)
        perm = rng.permutation(pool.Q)
        inv = np.argsort(perm)
        for n_top, cap, item_cap in ((1, 1, None), (5, 1, caps), (33, 2, None)):
            got, h = allot_pool(DevPool(pool), n_top, cap, item_cap)
            gp, hp = allot_pool(DevPool(pool.permuted(perm)), n_top, cap, item_cap)
            # the permuted input is the market of the statement renumbered by qid = perm
            want = allot_rounds(pool, n_top, cap, item_cap, qid=inv)
            for g, w in zip(gp[:5], want.lists()):
                assert g.tobytes() == w[perm].tobytes()
            if family == "descending_random":   # no score ties across queries: the lists do not depend on the numbering at all
                assert len(np.unique(pool.plain)) == pool.plain.size
                assert [a[inv].tobytes() for a in gp[:5]] == [a.tobytes() for a in got[:5]] and gp[5].tobytes() == got[5].tobytes()
                assert hp[:4] == h[:4] and hp[5] == h[5]
            # rank_by 0 against rank_by 1 with the two score columns swapped
            gs, hs = allot_pool(DevPool(pool.swapped()), n_top, cap, item_cap, rank_by=1)
            assert [gs[k].tobytes() for k in (0, 1, 3, 2, 4, 5)] == [a.tobytes() for a in got] and hs == h


def test_abundance_returns_the_prefix_of_the_pool():
    pool = al.designed_pool(65, 64, "inf_and_subnormal", 31, voids=False)
    for n_top in (1, 10, 64):
        got, h, R = run_and_check(pool, n_top, INT32_MAX)
        assert got[0].tolist() == [n_top] * 65
        assert got[1].tobytes() == pool.item[:, :n_top].tobytes() and got[2].tobytes() == pool.plain[:, :n_top].tobytes()
        assert got[3].tobytes() == pool.decay[:, :n_top].tobytes()
        assert h[0] == 0 and h[2] == 0 and h[4] == 1
    got, h, R = run_and_check(pool, 64, 1, np.full(pool.n_items, INT32_MAX, np.int32))
    assert h[0] == 0 and h[4] == 1


def test_no_queries_and_no_optional_outputs():
    pool = al.designed_pool(5, 8, "negative", 41)
    D = DevPool(pool)
    rc, msg, O, h = allot_pool_rc(D, 3, n_query=0)
    assert rc == 0, msg
    got, guards = O.host()
    assert guards and h == [0] * 6 and (got[5] == 0).all() and all((g == -7).all() for g in got[:5])
    ref, _ = allot_pool(D, 3, 1)
    rc, msg, O, h = allot_pool_rc(D, 3, 1, stats=False, taken=False)
    assert rc == 0, msg
    got, guards = O.host()
    assert guards and [a.tobytes() for a in got[:5]] == [a.tobytes() for a in ref[:5]] and (got[5] == -7).all()


# ------------------------------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_leave_every_byte():
    from xmap.engine import hipabi as abi
    pool = al.designed_pool(9, 16, "negative", 51)
    D = DevPool(pool)
    caps = al.designed_caps(pool.n_items, 52)
    # on the device: a negative entry of item_cap, the first one named
    bad = caps.copy()
    bad[[7, 13]] = (-1, -2 ** 31)
    rc, msg, O, h = allot_pool_rc(D, 4, 1, bad)
    assert rc == abi.ERR_ARG and "item_cap[7]" in msg and O.untouched() and h == [-7] * 6
    # on the host
    for kw, name in ((dict(n_top=0), "n_top"), (dict(n_top=17), "n_top"), (dict(n_pool=0), "n_pool"), (dict(n_pool=1025), "n_pool"),
                     (dict(rank_by=2), "rank_by"), (dict(cap=0), "cap"), (dict(cap=-1), "cap"), (dict(n_query=-1), "n_query"),
                     (dict(n_items=-1), "n_items"), (dict(n_query=2 ** 21, n_pool=1024), "n_query * n_pool"),
                     (dict(n_query=2 ** 31 // 16, n_pool=16), "n_query * n_pool")):
        a = dict(n_top=4)
        a.update(kw)
        rc, msg, O, h = allot_pool_rc(D, **a)
        assert rc == abi.ERR_ARG and name in msg and O.untouched() and h == [-7] * 6, (kw, msg)
    got, h = allot_pool(D, 4, 0, caps)          # the scalar is not read where item_cap is given
    assert h[1] > 0


# ----------------------------------------------------------------------------------- 4. xmap_allot_rows on the small models
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


def allot_rows_rc(D, U, I, keep, n_w, queries, n_pool, n_top, rank_by, flags, cap=1, item_cap=None, filt=NO_FILTER, alpha=1.5):
    """xmap_allot_rows on an OnDevice of (ptr, item, rating, time, cnt, col, sim, avg): (rc, message, Outs, stats [12])"""
    import torch
    from xmap.engine import hipabi as abi
    ptr, pit, pra, pti, cnt, col, sim, avg = D.t
    q = _dev(queries, np.int32)
    Q = len(queries)
    w = _dev(wtab(alpha, n_w))
    O = Outs(Q, n_top, I)
    h = (C.c_int64 * 12)(*([-7] * 12))
    st = C.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)
    F, alive = filt.on_device()
    d_cap = None if item_cap is None else _dev(item_cap, np.int32)
    rc = abi.lib.xmap_allot_rows(st, abi.i64(Q), abi.vp(q), abi.i32(n_pool), abi.i32(rank_by), abi.i32(flags), abi.i64(U), abi.i32(I), abi.i32(keep),
                                 abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ptr), abi.vp(pit), abi.vp(pra), abi.vp(pti), abi.vp(avg), abi.vp(w),
                                 abi.i32(n_w), abi.i32(n_top), abi.i32(cap), abi.vp(d_cap),
                                 *([abi.vp(t) for t in O.t] + [None if F is None else C.byref(F), h]))
    torch.cuda.synchronize()
    del alive
    return rc, (abi.lib.xmap_last_error() or b"").decode(), O, [int(x) for x in h]


def _rules(case, queries, seed=9):
    rng = np.random.default_rng(seed)
    exclude = [rng.integers(-2, case.I + 2, int(rng.integers(0, 9))).tolist() for _ in queries]
    return rng.random(case.I) < 0.8, exclude


def _pool_of(ref, Q, n_pool, I):
    return Pool(ref[0], ref[1].reshape(Q, n_pool), ref[2].reshape(Q, n_pool), ref[3].reshape(Q, n_pool), I)


@pytest.mark.parametrize("which", ["hand", "rand"])
def test_allot_rows_is_the_statement_over_the_filtered_top_n(which, hand, rand):
    """the pool is by definition what xmap_topn_rows_filtered returns with n_top = n_pool, with and without a Filter"""
    from xmap.engine import hipabi as abi
    c = hand if which == "hand" else rand
    queries = list(range(c.U)) + [c.U + 5, -1, 3, 3]
    Q = len(queries)
    allow, exclude = _rules(c, queries)
    caps = al.designed_caps(c.I, 61)
    refused = 0
    for n_pool in (1, 17, 64):
        for n_top, rank_by, flags, cap, item_cap, filt in ((10, 0, 0, 1, None, NO_FILTER), (5, 1, KEEP_HELD, 1, caps, Filter(allow=allow, exclude=exclude, min_score=3.0)),
                                                           (64, 0, 0, 2, None, Filter(exclude=exclude)), (3, 1, 0, INT32_MAX, None, Filter(allow=allow))):
            n_top = min(n_top, n_pool)
            ref = topn_f(c.D, c.U, c.I, c.keep, 66, queries, n_pool, rank_by, flags, filt)
            pool = _pool_of(ref, Q, n_pool, c.I)
            R = allot_rounds(pool, n_top, cap, item_cap, rank_by)
            rc, msg, O, h = allot_rows_rc(c.D, c.U, c.I, c.keep, 66, queries, n_pool, n_top, rank_by, flags, cap, item_cap, filt)
            assert rc == 0, msg
            got, guards = O.host()
            assert guards
            check_allot_output(pool, n_top, got[:5])
            same_lists(got, R)
            assert np.array_equal(got[5], R.taken) and h[:6] == list(ref[4]) and h[6:] == R.stats
            assert is_stable(pool, n_top, held_mask(pool, got[0], got[4]), cap, item_cap, rank_by)
            # ... and xmap_allot_pool over that pool: the same bytes
            back, hb = allot_pool(DevPool(pool), n_top, cap, item_cap, rank_by)
            assert [a.tobytes() for a in back] == [a.tobytes() for a in got] and hb == h[6:]
            refused += h[8]
    assert refused > 0
    # refusals: the outputs keep every byte
    for kw, name in ((dict(n_pool=65, n_top=4), "n_pool"), (dict(n_pool=8, n_top=9), "n_top"), (dict(n_pool=8, n_top=4, cap=0), "cap"),
                     (dict(n_pool=8, n_top=4, flags=4), "flags"), (dict(n_pool=8, n_top=4, item_cap=-caps - 1), "item_cap[0]"),
                     (dict(n_pool=8, n_top=4, filt=Filter(min_score=float("nan"))), "")):
        a = dict(rank_by=0, flags=0)
        a.update(kw)
        rc, msg, O, h = allot_rows_rc(c.D, c.U, c.I, c.keep, 66, queries, **a)
        assert rc == abi.ERR_ARG and name in msg and O.untouched(), (kw, msg)


# ------------------------------------------------------------------------------ 5. the coarse entry over the three sources
def _ctx_allot(ctx, source, queries, n_pool, n, rank_by, flags, cap=1, item_cap=None, n_items=0, F=None, taken=True, n_w=66, alpha=1.5):
    """xmap_ctx_recommend_allot: (rc, message, the five outputs and item_taken pre-filled with -7, stats [12])"""
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    outs = [np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32), np.full((Q, n), -7.0), np.full((Q, n), -7.0),
            np.full((Q, n), -7, np.int32), np.full(max(n_items, 1), -7, np.int32)]
    stats = np.full(12, -7, np.int64)
    caps = None if item_cap is None else np.ascontiguousarray(item_cap, np.int32)
    rc = ctx.lib.xmap_ctx_recommend_allot(ctx.h, source, Q, _p(q, C.c_int32), n_pool, n, rank_by, flags, _p(w, C.c_double), n_w, cap,
                                          None if caps is None else caps.ctypes.data_as(C.c_void_p), 0 if caps is None else len(caps),
                                          *([o.ctypes.data_as(C.c_void_p) for o in outs[:5]] +
                                            [outs[5].ctypes.data_as(C.c_void_p) if taken else None, None if F is None else C.byref(F),
                                             _p(stats, C.c_int64)]))
    return rc, (ctx.lib.xmap_last_error() or b"").decode(), outs, stats.tolist()


def _ctx_filtered(ctx, source, queries, n, rank_by, flags, F=None, n_w=66, alpha=1.5):
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    cnt, ids = np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32)
    plain, decay, stats = np.full((Q, n), -7.0), np.full((Q, n), -7.0), np.full(6, -7, np.int64)
    ctx.call("xmap_ctx_recommend_filtered", source, Q, _p(q, C.c_int32), n, rank_by, flags, _p(w, C.c_double), n_w, _p(cnt, C.c_int32),
             _p(ids, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), None if F is None else C.byref(F), _p(stats, C.c_int64))
    return cnt, ids, plain, decay, stats.tolist()


def test_the_coarse_call_over_the_three_sources():
    from test_gpu_foldin import foldin
    from test_gpu_item_foldin import item_foldin
    from xmap.engine import hipabi as abi, synth
    seed, users, src_items, tgt_items, overlap = 5, 1500, 300, 300, 0.4          # the small case of the other coarse tail tests
    r = _few_times(synth.make_two_domain(seed, users, src_items, tgt_items, overlap=overlap))
    I, U, keep = r.n_items, users, 5
    rng = np.random.default_rng(seed)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        rec_sim(ctx, I, U, len(rows["user"]))
        select(ctx, I, keep)
        B = 60
        lens = rng.integers(0, 30, B)
        f_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        f_item = rng.integers(0, I, f_ptr[-1]).astype(np.int32)
        foldin(ctx, f_ptr, f_item, (rng.integers(2, 21, len(f_item)) / 4.0).astype(np.float32), 1000 + rng.integers(0, 7, len(f_item)).astype(np.int64))
        NB = 6
        b_lens = rng.integers(10, 40, NB)
        b_ptr = np.concatenate([[0], np.cumsum(b_lens)]).astype(np.int64)
        b_user = np.concatenate([rng.choice(U, k, replace=False) for k in b_lens]).astype(np.int32)
        item_foldin(ctx, (b_ptr, b_user, rng.integers(2, 21, len(b_user)) / 4.0))
        refused = 0
        for source, n_it, qs_ in ((0, I, np.arange(-1, 200)), (1, I, np.arange(-1, B + 1)), (2, I + NB, np.arange(0, 150))):
            qs_ = np.concatenate([qs_, qs_[5:8]]).astype(np.int32)
            exclude = [rng.integers(-2, n_it + 2, int(rng.integers(0, 9))).tolist() for _ in qs_]
            filt = Filter(allow=rng.random(n_it) < 0.7, exclude=exclude, min_score=2.5)
            caps = al.designed_caps(n_it, 70 + source)
            for n_pool, n, rank_by, flags, cap, item_cap, f in ((40, 10, 0, 0, 2, None, NO_FILTER), (64, 12, 1, KEEP_HELD, 1, caps, filt),
                                                                (17, 17, 0, 0, 1, None, filt)):
                F, alive = f.on_host()
                pool = _pool_of(_ctx_filtered(ctx, source, qs_, n_pool, rank_by, flags, F), len(qs_), n_pool, n_it)
                R = allot_rounds(pool, n, cap, item_cap, rank_by)
                rc, msg, got, stats = _ctx_allot(ctx, source, qs_, n_pool, n, rank_by, flags, cap, item_cap, n_it, F)
                assert rc == 0, msg
                same_lists(got, R)
                assert np.array_equal(got[5], R.taken) and stats[6:] == R.stats
                refused += stats[8]
                rc, msg, again, _ = _ctx_allot(ctx, source, qs_, n_pool, n, rank_by, flags, cap, item_cap, n_it, F, taken=False)
                assert rc == 0 and [a.tobytes() for a in again[:5]] == [a.tobytes() for a in got[:5]] and (again[5] == -7).all()
            # capacities of another item space: refused by the context check, nothing written
            rc, msg, got, stats = _ctx_allot(ctx, source, qs_, 8, 4, 0, 0, 1, np.ones(n_it + 1, np.int32), n_it)
            assert rc == abi.ERR_ARG and "n_cap" in msg and all((o == -7).all() for o in got) and stats == [-7] * 12
        assert refused > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------- 6. the Python routes
def test_engine_allot_on_tensors(rand):
    import torch
    from types import SimpleNamespace
    from xmap.engine import device
    c = rand
    eng = device.Engine(SimpleNamespace(device=torch.device("cuda:0"), n_items=c.I))
    ptr, pit, pra, pti, cnt, col, sim, avg = c.D.t
    P = SimpleNamespace(n_users=c.U, n_items=c.I, user_ptr=ptr, user_item=pit, user_rating64=pra, user_time=pti)
    queries = list(range(c.U)) + [c.U + 5, 3]
    allow, exclude = _rules(c, queries)
    filt = Filter(allow=allow, exclude=exclude, min_score=3.0)
    F, alive = filt.on_device()
    caps = al.designed_caps(c.I, 81)
    d_q, d_w = _dev(queries, np.int32), _dev(wtab(1.5, 66))
    out = eng.allot_topn(P, (cnt, col, sim), d_q, avg, d_w, 40, 5, item_cap=caps, rank_by=1, keep_held=True, allow=alive[0],
                         exclude=(alive[1], alive[2]), min_score=3.0)
    rc, msg, O, h = allot_rows_rc(c.D, c.U, c.I, c.keep, 66, queries, 40, 5, 1, KEEP_HELD, 1, caps, filt)
    assert rc == 0, msg
    ref = O.host()[0]
    assert len(out) == 4 and [x.cpu().numpy().tobytes() for x in list(out) + [out.positions, out.taken]] == [a.tobytes() for a in ref]
    assert list(out.stats) == h and h[8] > 0
    # allot_pool over what topn() returned: the lists of allot_topn again
    pool = eng.topn(P, (cnt, col, sim), d_q, avg, d_w, 64)
    whole = eng.allot_topn(P, (cnt, col, sim), d_q, avg, d_w, 64, 10, cap=2)
    back = eng.allot_pool(pool, 10, cap=2, n_items=c.I)
    assert [x.cpu().numpy().tobytes() for x in list(back) + [back.positions, back.taken]] == \
        [x.cpu().numpy().tobytes() for x in list(whole) + [whole.positions, whole.taken]]
    assert back.stats == whole.stats[6:] and back.stats[2] > 0
    for bad in (dict(n_top=65), dict(n_top=0), dict(cap=0), dict(item_cap=np.ones(3, np.int32)), dict(rank_by=2)):
        a = dict(n_top=10)
        a.update(bad)
        with pytest.raises(ValueError):
            eng.allot_pool(pool, n_items=c.I, **a)


def test_engine_allot_pool_over_user_knn_lists_feeds_fill_and_fuse():
    """pools of width 128 from uknn_topn(); the allotted lists go into fuse() and fill() unchanged: the layout holds"""
    import torch
    from types import SimpleNamespace
    import uknn_statement as us
    import test_gpu_uknn as tu
    from xmap.engine import device
    c = us.family_case("integers")
    P, query, n_nb = c["P"], c["query"], max(us.N_NBS)
    D, L = tu.DevProfiles(P), tu.DevLists(c["lists"][n_nb], c["qavg"], c["avg"])
    view = SimpleNamespace(n_users=P.n_users, n_items=P.n_items, user_ptr=D.ptr, user_item=D.item, user_rating64=D.rating)
    eng = device.Engine(SimpleNamespace(device=torch.device("cuda:0"), n_items=P.n_items))
    d_q = _dev(np.asarray(query, np.int32))
    u = eng.uknn_topn(view, view, d_q, (L.cnt, L.user, L.sim), L.qavg, 128)
    assert u[1].shape[1] == 128
    pool = Pool(*[x.cpu().numpy() for x in (u[0], u[1], u[2], u[2])], n_items=P.n_items)
    for n_top, cap in ((5, 3), (128, 2)):
        A = eng.allot_pool((u[0], u[1], u[2], u[2]), n_top, cap=cap, n_items=P.n_items)
        R = allot_rounds(pool, n_top, cap)
        same_lists([x.cpu().numpy() for x in list(A) + [A.positions]], R)
        assert np.array_equal(A.taken.cpu().numpy(), R.taken) and list(A.stats) == R.stats and R.stats[2] > 0
    A = eng.allot_pool((u[0], u[1], u[2], u[2]), 5, cap=3, n_items=P.n_items)
    a_cnt, a_item, a_score = [x.cpu().numpy() for x in A[:3]]
    # one list fused by "sum" is that list again
    cnt, ids, score, mask, st = eng.fuse([(A[0], A[1], A[2])], 5, how="sum", n_ids=P.n_items)
    assert np.array_equal(cnt.cpu().numpy(), a_cnt) and np.array_equal(ids.cpu().numpy(), a_item)
    assert np.array_equal(score.cpu().numpy().view(np.uint64), a_score.view(np.uint64))
    # the popularity fill completes the short lists behind the allotted entries
    pop = eng.pop_index(eng.peer_index(view), "count", 0.0, 1)
    f = eng.fill(A, pop, view, d_q, _dev(np.zeros(P.n_items)))
    f_cnt, f_item, f_src = f[0].cpu().numpy(), f[1].cpu().numpy(), f[4].cpu().numpy()
    kept = np.arange(5)[None, :] < a_cnt[:, None]
    assert (f_cnt >= a_cnt).all() and (f_cnt > a_cnt).any() and np.array_equal(f_item[kept], a_item[kept]) and (f_src[kept] == 0).all()
