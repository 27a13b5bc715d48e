"""Hold-out evaluation of the top-N lists on the device (csrc/stage_e_eval.hip; xmap_eval_users, xmap_topn_eval,
xmap_ctx_evaluate_topn, Engine.eval_users / topn_eval, session.evaluate_topn).

The expected values are the brute-force statement below: the definition in include/xmap_hip.h with a set per user.  Masks,
counters, cover and the integer columns of agg are compared exactly, q_metric as uint64 views, the sum columns of agg with == against
math.fsum of the per-query values (the double-double sum is exact here: the terms lie in [2^-12, 1], at most 2^20 of them)."""
import ctypes as C
import datetime
import math

import numpy as np
import pytest

from golden_util import CAP
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_coarse_oracle import stage_c
from test_gpu_tail import _few_times, generate, rec_sim, select, wtab
from test_gpu_topn import recommend

pytestmark = pytest.mark.gpu
KEEP_HELD = 1


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


def discounts(n):
    return np.asarray([1.0 / np.log2(r + 2) for r in range(n)], np.float64)


# ---------------------------------------------------------------------------------------------- the brute-force statement
def relevant_sets(tu, ti, tr, rel_min, U, I):
    """(n_rel [U], {user: set of relevant items}, (relevant, ignored, below))"""
    n_rel, rel, relevant, ignored, below = np.zeros(U, np.int32), {}, 0, 0, 0
    for u, i, r in zip(np.asarray(tu).tolist(), np.asarray(ti).tolist(), np.asarray(tr).tolist()):
        if not (0 <= u < U and 0 <= i < I) or r != r:
            ignored += 1
        elif r >= rel_min:
            relevant += 1
            n_rel[u] += 1
            rel.setdefault(u, set()).add(i)
        else:
            below += 1
    return n_rel, rel, (relevant, ignored, below)


def query_metrics(L, R, n, c, dtab):
    """the definition, word for word"""
    h = 0
    dcg = ap = rr = 0.0
    for r in range(min(c, len(L))):
        if L[r] in R:
            h += 1
            dcg = dcg + dtab[r]
            ap = ap + h / (r + 1)
            if rr == 0.0:
                rr = 1.0 / (r + 1)
    idcg = 0.0
    for r in range(min(c, n)):
        idcg = idcg + dtab[r]
    return h, (h / c, h / n, dcg / idcg, ap / min(c, n), rr)


def statement(tu, ti, tr, rel_min, U, I, n_rel, rel, query_user, cnt, item, cuts, dtab):
    """masks [Q] uint64, q_metric [Q][n_cut][5], agg [n_cut][8], cover [n_cut] of lists (cnt [Q], item [Q][n_top])"""
    Q, n_cut = len(query_user), len(cuts)
    dt = [float(x) for x in dtab]
    masks, qm = np.zeros(Q, np.uint64), np.zeros((Q, n_cut, 5))
    ints = np.zeros((n_cut, 3), np.int64)
    terms = [[[] for _ in range(5)] for _ in range(n_cut)]
    seen = [set() for _ in range(n_cut)]
    lists = np.asarray(item).tolist()
    for q, u in enumerate(np.asarray(query_user).tolist()):
        L = lists[q][:int(cnt[q])]
        for k, c in enumerate(cuts):
            seen[k].update(L[:c])
        n = int(n_rel[u]) if 0 <= u < U else 0
        if n == 0:
            continue
        R = rel[u]
        masks[q] = np.uint64(sum(1 << r for r, x in enumerate(L) if x in R))
        for k, c in enumerate(cuts):
            h, m5 = query_metrics(L, R, n, c, dt)
            qm[q, k] = m5
            ints[k] += (1, h > 0, h)
            for x in range(5):
                terms[k][x].append(m5[x])
    agg = np.zeros((n_cut, 8))
    agg[:, :3] = ints
    for k in range(n_cut):
        agg[k, 3:] = [math.fsum(t) for t in terms[k]]
    return masks, qm, agg, np.asarray([len(s) for s in seen], np.int64)


# ------------------------------------------------------------------------------------------------------- the drivers
def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream("cuda:0").cuda_stream)


def eval_users(tu, ti, tr, rel_min, U, I):
    """xmap_eval_users on device copies: (n_rel [U], eval_user [n_eval], counts)"""
    import torch
    from xmap.engine import hipabi as abi
    d = [_dev(tu, np.int32), _dev(ti, np.int32), _dev(tr, np.float64)]
    n_rel = torch.full((max(U, 1),), -7, dtype=torch.int32, device="cuda:0")
    users = torch.full((max(U, 1),), -7, dtype=torch.int32, device="cuda:0")
    h = (C.c_int64 * 4)(-1, -1, -1, -1)
    abi.check(abi.lib.xmap_eval_users(_stream(), abi.i64(len(tu)), abi.vp(d[0]), abi.vp(d[1]), abi.vp(d[2]), C.c_double(rel_min),
                                      abi.i64(U), abi.i32(I), abi.vp(n_rel), abi.vp(users), h))
    return n_rel.cpu().numpy()[:U], users.cpu().numpy()[:int(h[0])], [int(x) for x in h]


def topn_eval_rc(tu, ti, tr, rel_min, U, I, n_rel, query_user, n_top, cnt, item, cuts, per_query=True, null=()):
    """xmap_topn_eval on device copies: (return code, mask, q_metric or None, agg, cover)"""
    import torch
    from xmap.engine import hipabi as abi
    Q, n_cut = len(query_user), len(cuts)
    d = [_dev(tu, np.int32), _dev(ti, np.int32), _dev(tr, np.float64), _dev(n_rel, np.int32), _dev(query_user, np.int32),
         _dev(cnt, np.int32), _dev(np.asarray(item, np.int32).reshape(-1), np.int32), _dev(discounts(n_top if 1 <= n_top <= 64 else 64), np.float64)]
    h_cut = np.ascontiguousarray(cuts, np.int32)
    mask = torch.full((max(Q, 1),), -7, dtype=torch.int64, device="cuda:0")
    qm = torch.full((max(Q, 1), max(n_cut, 1), 5), -7.0, dtype=torch.float64, device="cuda:0") if per_query else None
    agg = torch.full((max(n_cut, 1), 8), -7.0, dtype=torch.float64, device="cuda:0")
    cover = torch.full((max(n_cut, 1),), -7, dtype=torch.int64, device="cuda:0")
    out = dict(mask=mask, agg=agg, cover=cover)
    rc = abi.lib.xmap_topn_eval(_stream(), abi.i64(len(tu)), abi.vp(d[0]), abi.vp(d[1]), abi.vp(d[2]), C.c_double(rel_min), abi.i64(U),
                                abi.i32(I), abi.vp(d[3]), abi.i64(Q), abi.vp(d[4]), abi.i32(n_top), abi.vp(d[5]), abi.vp(d[6]),
                                abi.i32(n_cut), _p(h_cut, C.c_int32), abi.vp(d[7]), *[abi.vp(None if k in null else out[k]) for k in ("mask",)],
                                abi.vp(qm), *[abi.vp(None if k in null else out[k]) for k in ("agg", "cover")])
    return (rc, mask.cpu().numpy()[:Q].view(np.uint64), None if qm is None else qm.cpu().numpy()[:Q], agg.cpu().numpy()[:n_cut],
            cover.cpu().numpy()[:n_cut])


def check_eval(got, want, per_query=True):
    rc, mask, qm, agg, cover = got
    w_mask, w_qm, w_agg, w_cover = want
    assert rc == 0
    assert np.array_equal(mask, w_mask)
    if per_query:
        assert np.array_equal(qm.view(np.uint64), w_qm.view(np.uint64))
    assert np.array_equal(agg[:, :3], w_agg[:, :3]) and cover.tolist() == w_cover.tolist()
    assert agg[:, 3:].tolist() == w_agg[:, 3:].tolist()


# ------------------------------------------------------------------------------------------ 1. fine-grained, hand-built
def _case1(n_top=64):
    rng = np.random.default_rng(31)
    U, I, Q = 200, 500, 150
    qu = rng.permutation(U)[:Q].astype(np.int32)
    cnt = rng.integers(0, n_top + 1, Q).astype(np.int32)
    cnt[:4] = [0, n_top, 1, n_top]
    item = np.full((Q, n_top), -1, np.int32)
    for q in range(Q):
        item[q, :cnt[q]] = rng.permutation(I)[:cnt[q]]
    T = 5000
    tu, ti = rng.integers(-2, U + 2, T), rng.integers(-3, I + 3, T)
    tr = rng.integers(1, 6, T).astype(np.float64)
    tr[rng.choice(T, 40, replace=False)] = np.nan
    keep = ~np.isin(tu, qu[5:15])                # the queries 5..14 keep no pair at all
    tu, ti, tr = tu[keep], ti[keep], tr[keep]
    planted = [(qu[1], item[1, n_top - 1], 5.0), (qu[3], item[3, 0], 4.0), (qu[3], item[3, 0], 4.0), (qu[3], item[3, n_top - 1], 3.999),
               (qu[2], item[2, 0], 5.0)]
    tu = np.concatenate([tu, [p[0] for p in planted]]).astype(np.int32)
    ti = np.concatenate([ti, [p[1] for p in planted]]).astype(np.int32)
    tr = np.concatenate([tr, [p[2] for p in planted]])
    o = rng.permutation(len(tu))
    return U, I, qu, cnt, item, tu[o], ti[o], tr[o]


def test_hand_built_lists_against_the_statement():
    U, I, qu, cnt, item, tu, ti, tr = _case1()
    cuts, dtab = (1, 5, 10, 64), discounts(64)
    n_rel, rel, (relevant, ignored, below) = relevant_sets(tu, ti, tr, 4.0, U, I)
    want = statement(tu, ti, tr, 4.0, U, I, n_rel, rel, qu, cnt, item, cuts, dtab)
    # what the inputs show (so a change of the generator cannot hollow the test out)
    hits = np.asarray([bin(int(m)).count("1") for m in want[0]])
    repeated = len(tu) - len({(u, i) for u, i in zip(tu.tolist(), ti.tolist())})
    rel_rep = sum(n_rel[u] - len(s) for u, s in rel.items())
    print("ignored %d, queries without a relevant pair %d, with a hit %d, with several %d, repeated pairs %d (relevant %d)" % (
        ignored, int((n_rel[qu] == 0).sum()), int((hits > 0).sum()), int((hits > 1).sum()), repeated, rel_rep))
    assert ignored == 194 and (n_rel[qu] == 0).sum() == 10 and (hits > 0).sum() == 71 and (hits > 1).sum() == 23
    assert repeated > 1 and rel_rep > 1                             # random repeated pairs: the occurrence rule
    assert int(want[0][1]) == 1 << 63 and int(want[0][2]) == 1
    assert int(want[0][3]) & 1 and not int(want[0][3]) >> 63 & 1    # 4.0 is relevant, 3.999 is not
    assert n_rel[qu[3]] > len(rel[qu[3]])                           # a repeated relevant pair: twice in n_rel, one hit
    assert want[1][3, 3, 1] == hits[3] / n_rel[qu[3]] and want[1][0].sum() == 0 and not want[0][0]
    # xmap_eval_users
    g_rel, g_users, counts = eval_users(tu, ti, tr, 4.0, U, I)
    assert np.array_equal(g_rel, n_rel) and g_users.tolist() == np.nonzero(n_rel)[0].tolist()
    assert counts == [int((n_rel > 0).sum()), relevant, ignored, below]
    # xmap_topn_eval
    got = topn_eval_rc(tu, ti, tr, 4.0, U, I, n_rel, qu, 64, cnt, item, cuts)
    check_eval(got, want)
    again = topn_eval_rc(tu, ti, tr, 4.0, U, I, n_rel, qu, 64, cnt, item, cuts)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[1:], again[1:]))
    check_eval(topn_eval_rc(tu, ti, tr, 4.0, U, I, n_rel, qu, 64, cnt, item, cuts, per_query=False), want, per_query=False)
    # eight cutoffs
    cuts8 = (1, 2, 3, 5, 8, 13, 21, 64)
    check_eval(topn_eval_rc(tu, ti, tr, 4.0, U, I, n_rel, qu, 64, cnt, item, cuts8),
               statement(tu, ti, tr, 4.0, U, I, n_rel, rel, qu, cnt, item, cuts8, dtab))
    # another threshold: the counts move with it
    n_rel3, rel3, c3 = relevant_sets(tu, ti, tr, 3.0, U, I)
    assert c3[0] > relevant and c3[1] == ignored
    assert eval_users(tu, ti, tr, 3.0, U, I)[2] == [int((n_rel3 > 0).sum())] + list(c3)
    check_eval(topn_eval_rc(tu, ti, tr, 3.0, U, I, n_rel3, qu, 64, cnt, item, cuts),
               statement(tu, ti, tr, 3.0, U, I, n_rel3, rel3, qu, cnt, item, cuts, dtab))


def test_lists_of_one_and_empty_inputs():
    U, I, qu, cnt, item, tu, ti, tr = _case1(n_top=1)
    n_rel, rel, _ = relevant_sets(tu, ti, tr, 4.0, U, I)
    want = statement(tu, ti, tr, 4.0, U, I, n_rel, rel, qu, cnt, item, (1,), discounts(1))
    assert want[2][0, 1] > 0
    check_eval(topn_eval_rc(tu, ti, tr, 4.0, U, I, n_rel, qu, 1, cnt, item, (1,)), want)
    # no query: zero aggregates; no pair: nobody is evaluated, the coverage still counts the lists
    none = topn_eval_rc(tu, ti, tr, 4.0, U, I, n_rel, qu[:0], 1, cnt[:0], item[:0], (1,))
    assert none[0] == 0 and not none[3].any() and not none[4].any()
    zero = np.zeros(U, np.int32)
    e = np.zeros(0)
    got = topn_eval_rc(e, e, e, 4.0, U, I, zero, qu, 1, cnt, item, (1,))
    check_eval(got, statement(e, e, e, 4.0, U, I, zero, {}, qu, cnt, item, (1,), discounts(1)))
    assert not got[1].any() and not got[3].any() and got[4][0] == len(set(item[cnt > 0, 0].tolist()))
    g_rel, g_users, counts = eval_users(e, e, e, 4.0, U, I)
    assert not g_rel.any() and len(g_users) == 0 and counts == [0, 0, 0, 0]


def test_argument_errors_of_the_fine_grained_entry_points():
    from xmap.engine import hipabi as abi
    U, I, qu, cnt, item, tu, ti, tr = _case1()
    n_rel = relevant_sets(tu, ti, tr, 4.0, U, I)[0]
    base = dict(rel_min=4.0, query_user=qu, n_top=64, cuts=(1, 5, 10, 64), null=())

    def rc(**kw):
        a = dict(base, **kw)
        n = a["n_top"]
        return topn_eval_rc(tu, ti, tr, a["rel_min"], U, I, n_rel, a["query_user"], n, cnt, item[:, :max(1, min(n, 64))], a["cuts"],
                            null=a["null"])[0]
    assert rc() == 0
    twice = qu.copy()
    twice[77] = twice[3]
    for kw in (dict(query_user=twice), dict(cuts=(1, 5, 5, 64)), dict(cuts=(5, 1)), dict(cuts=(1, 65)), dict(cuts=(0, 5)), dict(cuts=()),
               dict(cuts=tuple(range(1, 10))), dict(n_top=0, cuts=(1,)), dict(n_top=65, cuts=(1,)), dict(n_top=8, cuts=(1, 10)),
               dict(rel_min=float("nan")), dict(null=("mask",)), dict(null=("agg",)), dict(null=("cover",))):
        assert rc(**kw) == abi.ERR_ARG, kw
        assert abi.lib.xmap_last_error()
    assert b"more than once" in (rc(query_user=twice), abi.lib.xmap_last_error())[1]
    with pytest.raises(abi.XmapError):
        eval_users(tu, ti, tr, float("nan"), U, I)
    assert rc() == 0                                            # and the library goes on working


# --------------------------------------------------------------------------------- 2. more queries than a grid dimension
def test_more_queries_than_a_grid_dimension():
    rng = np.random.default_rng(32)
    U = Q = 70000
    I, n_top, T, cuts = 40, 3, 200000, (1, 3)
    qu = rng.permutation(U).astype(np.int32)
    cnt = rng.integers(0, n_top + 1, Q).astype(np.int32)
    item = np.full((Q, n_top), -1, np.int32)
    perm = np.argsort(rng.random((Q, I)), axis=1)[:, :n_top].astype(np.int32)
    item[np.arange(n_top)[None, :] < cnt[:, None]] = perm[np.arange(n_top)[None, :] < cnt[:, None]]
    tu, ti = rng.integers(0, U, T).astype(np.int32), rng.integers(0, I, T).astype(np.int32)
    tr = rng.integers(1, 6, T).astype(np.float64)
    n_rel, rel, counts = relevant_sets(tu, ti, tr, 4.0, U, I)
    want = statement(tu, ti, tr, 4.0, U, I, n_rel, rel, qu, cnt, item, cuts, discounts(n_top))
    print("queries with a hit %d, without a relevant pair %d" % (want[2][1, 1], (n_rel == 0).sum()))
    assert want[2][1, 1] > 0 and (n_rel == 0).sum() > 0
    g_rel, g_users, g_counts = eval_users(tu, ti, tr, 4.0, U, I)
    assert np.array_equal(g_rel, n_rel) and g_users.tolist() == np.nonzero(n_rel)[0].tolist()
    assert g_counts == [int((n_rel > 0).sum())] + list(counts)
    check_eval(topn_eval_rc(tu, ti, tr, 4.0, U, I, n_rel, qu, n_top, cnt, item, cuts), want)


# ------------------------------------------------------------------------------------------------------ 3. one hot user
def test_one_hot_user():
    rng = np.random.default_rng(33)
    U, I, n_top, hot, cuts = 50, 120000, 64, 7, (1, 32, 64)
    hot_items = rng.choice(I, 100000, replace=False)
    tu, ti = [np.full(len(hot_items), hot)], [hot_items]
    for u in range(U):
        if u != hot:
            k = int(rng.integers(0, 6))
            tu.append(np.full(k, u))
            ti.append(rng.choice(I, k, replace=False))
    tu, ti = np.concatenate(tu).astype(np.int32), np.concatenate(ti).astype(np.int32)
    tr = np.full(len(tu), 5.0)
    o = np.argsort(rng.random(len(tu)) + (tu != hot) * 0.5)       # runs of the hot user and mixed stretches
    tu, ti, tr = tu[o], ti[o], tr[o]
    qu = np.arange(U, dtype=np.int32)
    cnt = np.full(U, n_top, np.int32)
    item = np.stack([rng.choice(I, n_top, replace=False) for _ in range(U)]).astype(np.int32)
    miss = np.setdiff1d(np.arange(I), hot_items)
    item[hot] = rng.choice(miss[miss >= 1 << 16], n_top, replace=False)
    item[hot, [0, 31, 63]] = hot_items[:3]
    n_rel, rel, counts = relevant_sets(tu, ti, tr, 4.0, U, I)
    dtab = discounts(n_top)
    want = statement(tu, ti, tr, 4.0, U, I, n_rel, rel, qu, cnt, item, cuts, dtab)
    assert n_rel[hot] == 100000 and n_rel[np.arange(U) != hot].max() <= 5
    assert int(want[0][hot]) == 1 | 1 << 31 | 1 << 63
    # recall, min(c, n) of ap and idcg follow n_rel = 100000
    assert want[1][hot, 2, 1] == 3 / 100000 and want[1][hot, 2, 3] == (1 / 1 + 2 / 32 + 3 / 64) / 64
    idcg = 0.0
    for r in range(64):
        idcg = idcg + dtab[r]
    assert want[1][hot, 2, 2] == ((dtab[0] + dtab[31]) + dtab[63]) / idcg
    assert len({x for x in item.reshape(-1).tolist() if x >= 1 << 16}) > 64 and want[3][2] > 64
    g_rel, g_users, g_counts = eval_users(tu, ti, tr, 4.0, U, I)
    assert np.array_equal(g_rel, n_rel) and g_counts == [int((n_rel > 0).sum())] + list(counts)
    check_eval(topn_eval_rc(tu, ti, tr, 4.0, U, I, n_rel, qu, n_top, cnt, item, cuts), want)


# ------------------------------------------------------------------------------------------- 4. coarse ABI, NumPy only
def evaluate(ctx, tu, ti, tr, rel_min, n, rank_by, flags, alpha, cuts, U, n_w=66):
    tu, ti = np.ascontiguousarray(tu, np.int32), np.ascontiguousarray(ti, np.int32)
    tr = np.ascontiguousarray(tr, np.float64)
    w, d, cut = wtab(alpha, n_w), discounts(n), np.ascontiguousarray(cuts, np.int32)
    agg, cover = np.full((len(cuts), 8), -7.0), np.full(len(cuts), -7, np.int64)
    nrel, mask, stats = np.full(U, -7, np.int32), np.full(U, 7, np.uint64), np.full(8, -7, np.int64)
    ctx.call("xmap_ctx_evaluate_topn", len(tu), _p(tu, C.c_int32), _p(ti, C.c_int32), _p(tr, C.c_double), C.c_double(rel_min), n, rank_by,
             flags, _p(w, C.c_double), n_w, len(cuts), _p(cut, C.c_int32), _p(d, C.c_double), _p(agg, C.c_double), _p(cover, C.c_int64),
             _p(nrel, C.c_int32), _p(mask, C.c_uint64), _p(stats, C.c_int64))
    return agg, cover, nrel, mask, stats.tolist()


def _held_out(rng, ctx, r, U, alpha):
    """held-out pairs from a first recommendation: every third drawn user rates positions 0, 3 and last of its list 5, 4
    and 3; + 2000 random (user, target item, rating) pairs; every (user, item) once"""
    drawn = np.unique(rng.integers(0, U, 300)).astype(np.int32)
    cnt, item = recommend(ctx, drawn, 10, 0, 0, alpha)[:2]
    pairs = {}
    for q in range(0, len(drawn), 3):
        for pos, rating in ((0, 5.0), (3, 4.0), (int(cnt[q]) - 1, 3.0)):
            if 0 <= pos < cnt[q]:
                pairs.setdefault((int(drawn[q]), int(item[q, pos])), rating)
    for u, i, ra in zip(rng.integers(0, U, 2000).tolist(), rng.integers(r.n_src_items, r.n_items, 2000).tolist(),
                        rng.integers(1, 6, 2000).tolist()):
        pairs.setdefault((u, i), float(ra))
    keys = sorted(pairs)
    o = rng.permutation(len(keys))
    tu = np.asarray([keys[k][0] for k in o], np.int32)
    ti = np.asarray([keys[k][1] for k in o], np.int32)
    return tu, ti, np.asarray([pairs[keys[k]] for k in o], np.float64)


def test_evaluate_topn_through_the_coarse_abi():
    from xmap.engine import synth
    U, alpha, cuts_of = 1500, 1.5, {1: (1,), 10: (1, 5, 10), 64: (5, 10, 20, 64)}
    r = _few_times(synth.make_two_domain(5, U, 300, 300, overlap=0.4))
    I = r.n_items
    rng = np.random.default_rng(5)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        rec_sim(ctx, I, U, len(rows["user"]))
        select(ctx, I, 10)
        tu, ti, tr = _held_out(rng, ctx, r, U, alpha)
        n_rel, rel, counts = relevant_sets(tu, ti, tr, 4.0, U, I)
        users = np.nonzero(n_rel)[0].astype(np.int32)
        assert len(users) > 100 and len({(u, i) for u, i in zip(tu.tolist(), ti.tolist())}) == len(tu)
        hit_any = miss_any = False
        for n in (1, 10, 64):
            for rank_by in (0, 1):
                for flags in (0, KEEP_HELD):
                    cuts = cuts_of[n]
                    cnt, item, _, _, rstats = recommend(ctx, users, n, rank_by, flags, alpha)
                    w_mask, _, w_agg, w_cover = statement(tu, ti, tr, 4.0, U, I, n_rel, rel, users, cnt, item, cuts, discounts(n))
                    agg, cover, g_rel, g_mask, stats = evaluate(ctx, tu, ti, tr, 4.0, n, rank_by, flags, alpha, cuts, U)
                    assert np.array_equal(g_rel, n_rel)
                    full = np.zeros(U, np.uint64)
                    full[users] = w_mask
                    assert np.array_equal(g_mask, full)
                    assert np.array_equal(agg[:, :3], w_agg[:, :3]) and agg[:, 3:].tolist() == w_agg[:, 3:].tolist()
                    assert cover.tolist() == w_cover.tolist()
                    assert stats[:4] == [len(users)] + list(counts) and stats[4:] == rstats
                    assert agg[0, 0] == len(users)
                    hit_any |= bool(w_mask.any())
                    miss_any |= bool((w_mask == 0).any())
        assert hit_any and miss_any
        # nothing held out, and nothing relevant: zeroed outputs
        e = np.zeros(0)
        for a in (evaluate(ctx, e, e, e, 4.0, 10, 0, 0, alpha, (5, 10), U), evaluate(ctx, tu, ti, tr, 6.0, 10, 0, 0, alpha, (5, 10), U)):
            assert not a[0].any() and not a[1].any() and not a[2].any() and not a[3].any() and not any(a[4][4:]) and a[4][0] == 0
        assert a[4][1:4] == [0, counts[1], counts[0] + counts[2]]
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------- 5. lifecycle
def test_evaluate_topn_lifecycle_and_argument_errors():
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(3, 800, 200, 200, overlap=0.4))
    I, U = r.n_items, 800
    rng = np.random.default_rng(2)
    cuts = (5, 10)
    fresh = Ctx()
    try:
        generate(fresh, r)
        fresh.call("xmap_ctx_rec_sim", CAP, None)
        fresh.call("xmap_ctx_rec_select", 10)
        tu, ti, tr = _held_out(rng, fresh, r, U, 0.2)
        ref = evaluate(fresh, tu, ti, tr, 4.0, 10, 1, 0, 0.2, cuts, U)
    finally:
        fresh.close()
    assert ref[0][0, 0] > 0 and ref[0][1, 2] > 0 and ref[4][4] > 0

    def same(a, b):
        return all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    c = Ctx()
    try:
        ERR = c.abi.ERR_ARG
        w, d, cut = wtab(0.2, 8), discounts(4), np.asarray([1, 4], np.int32)
        agg, cover = np.zeros((2, 8)), np.zeros(2, np.int64)
        one_u, one_i, one_r = np.zeros(1, np.int32), np.full(1, I - 1, np.int32), np.full(1, 5.0)

        def raw(n_test=1, pairs=(one_u, one_i, one_r), rel_min=4.0, n=4, rank_by=0, flags=0, tab=w, n_w=8, n_cut=2, cu=cut, dt=d,
                out=(agg, cover)):
            return c.lib.xmap_ctx_evaluate_topn(c.h, n_test, _p(pairs[0], C.c_int32), _p(pairs[1], C.c_int32), _p(pairs[2], C.c_double),
                                                C.c_double(rel_min), n, rank_by, flags, _p(tab, C.c_double), n_w, n_cut,
                                                _p(cu, C.c_int32), _p(dt, C.c_double), _p(out[0], C.c_double), _p(out[1], C.c_int64),
                                                None, None, None)
        assert raw() == ERR                                                 # before upload
        rows = generate(c, r)
        assert raw() == ERR                                                 # before rec_sim
        c.call("xmap_ctx_rec_sim", CAP, None)
        assert raw() == ERR and b"have_nb" in c.lib.xmap_last_error()      # before rec_select
        c.call("xmap_ctx_rec_select", 10)
        assert raw() == 0
        # argument errors leave the context working
        for kw in (dict(n=0), dict(n=65), dict(rank_by=2), dict(rank_by=-1), dict(flags=2), dict(flags=-1), dict(n_w=0), dict(tab=None),
                   dict(n_cut=0), dict(n_cut=9), dict(cu=None), dict(cu=np.asarray([4, 1], np.int32)), dict(cu=np.asarray([1, 5], np.int32)),
                   dict(cu=np.asarray([0, 4], np.int32)), dict(dt=None), dict(out=(None, cover)), dict(out=(agg, None)),
                   dict(rel_min=float("nan")), dict(pairs=(None, one_i, one_r)), dict(pairs=(one_u, None, one_r)),
                   dict(pairs=(one_u, one_i, None)), dict(n_test=-1)):
            assert raw(**kw) == ERR, kw
            assert c.lib.xmap_last_error()
        assert raw(n_test=0, pairs=(None, None, None)) == 0                 # nothing held out
        assert same(evaluate(c, tu, ti, tr, 4.0, 10, 1, 0, 0.2, cuts, U), ref)
        c.call("xmap_ctx_item_sim", 0, CAP, None, None)                     # an earlier stage run again drops the tail
        assert raw() == ERR
        c.call("xmap_ctx_extend", 5, None, None)
        stage_c(c, I, True, None)
        c.call("xmap_ctx_rec_sim", CAP, None)
        assert raw() == ERR
        c.call("xmap_ctx_rec_select", 10)
        assert same(evaluate(c, tu, ti, tr, 4.0, 10, 1, 0, 0.2, cuts, U), ref)   # the reused context: the bytes of a fresh one
        assert len(rows["user"]) > 0
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------- 6. the Python route
def test_session_evaluate_topn_equals_the_statement_on_id_strings():
    """the construction of test_gpu_topn.test_session_recommend_topn_equals_the_statement_on_id_strings; the expected numbers
    from session.recommend_topn's lists for the same users, on id strings"""
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
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
    alpha, n, cuts = 1.5, 10, (1, 5, 10)
    uids = sorted({recs[int(x)][0] for x in rng.integers(0, len(recs), 120)})
    first = session.recommend_topn(ae, uids, CAP, 10, alpha, n).collect()
    # held out: ranks 0 and 2 of every second user's list (5 and 4 stars), rank 1 below the threshold, random target items,
    # a user and an item the train set does not know
    targets = sorted({c[0] for _, l in first for c in l})
    test = []
    for k, (uid, l) in enumerate(first):
        pairs = {}
        if k % 2 == 0:
            for pos, ra in ((0, 5.0), (2, 4.0), (1, 3.0)):
                if pos < len(l):
                    pairs[l[pos][0]] = ra
        for iid in rng.choice(targets, 3, replace=False).tolist():
            pairs.setdefault(iid, float(rng.integers(1, 6)))
        test.append((uid, [(iid, ra) for iid, ra in sorted(pairs.items())]))
    test.append(("A%013d" % (10 ** 9 + 1), [(targets[0], 5.0)]))
    test.append((uids[0], [("no such item", 5.0)]))
    rel = {}
    for uid, pairs in test[:-2]:
        for iid, ra in pairs:
            if ra >= 4.0:
                rel.setdefault(uid, set()).add(iid)
    dtab = discounts(n).tolist()
    for decay, keep_held in ((False, False), (True, True)):
        out = session.evaluate_topn(ae, LocalRDD(test), CAP, 10, alpha, n, cutoffs=cuts, rel_min=4.0, decay=decay, keep_held=keep_held)
        users = sorted(rel)
        lists = dict(session.recommend_topn(ae, users, CAP, 10, alpha, n, decay=decay, keep_held=keep_held).collect())
        masks = {u: sum(1 << p for p, c in enumerate(lists[u]) if c[0] in rel[u]) for u in users}
        assert out.masks == masks
        assert any(masks.values()) and not all(masks.values())
        for c in cuts:
            per = [query_metrics([x[0] for x in lists[u]], rel[u], len(rel[u]), c, dtab) for u in users]
            m = len(users)
            want = dict(users=m, hit_rate=sum(h > 0 for h, _ in per) / m, coverage=len({x[0] for u in users for x in lists[u][:c]}))
            for x, name in enumerate(("precision", "recall", "ndcg", "map", "mrr")):
                want[name] = math.fsum(p[1][x] for p in per) / m
            assert out.at[c] == want, c
        assert out.stats[0] == len(users) and out.stats[1] == sum(len(s) for s in rel.values()) and out.stats[2] == 2
        assert out.stats[5] == 0 and out.stats[4] > 0 and out.sim_pairs and out.item_info
    with pytest.raises(ValueError):
        session.evaluate_topn(ae, LocalRDD(test + [(test[0][0], [test[0][1][0]])]), CAP, 10, alpha, n, cutoffs=cuts)
    with pytest.raises(ValueError):
        session.evaluate_topn(ae, LocalRDD([(uids[0], [(targets[0], float("nan"))])]), CAP, 10, alpha, n, cutoffs=cuts)
    with pytest.raises(TypeError):
        session.evaluate_topn(LocalRDD(ae.collect()), LocalRDD(test), CAP, 10, alpha, n, cutoffs=cuts)
