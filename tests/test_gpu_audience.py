"""The audience of an item on the device (csrc/stage_e_audience.hip; xmap_audience_rows, xmap_ctx_audience,
xmap_ctx_foldin_audience, Engine.audience, session.recommend_audience): per query item the N best users among those whose own
rows give evidence for it, ranked by the unrounded prediction -- the top-N recommendation seen from the item.

The expected lists are the brute-force Python statement of test_gpu_topn.py fed only with downloaded arrays: score_users for
EVERY user with rows, inverted per item ({item: [(user, plain, decayed, now, holds the item)*]} in ascending user order), then
test_gpu_topn.expected over the query items: holders dropped unless kept, None scores and now > n_w dropped and counted,
sorted(key=(-score, user))[:n].  Users are compared exactly, scores as uint64 views, stats as tuples."""
import ctypes as C
import datetime
import os
import re

import numpy as np
import pytest

from golden_util import CAP
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_coarse_oracle import stage_c
from test_gpu_tail import _few_times, generate, neighbors, predict, rec_sim, select, wtab
from test_gpu_topn import KEEP_HELD, _random_case, _tool, check_output, expected, recommend, score_users, topn_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP_HOLDERS = 1
ALPHA = 1.5


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


def _window():
    """users per bitmap pass of the candidate kernel, read from the source"""
    src = open(os.path.join(ROOT, "x-map_amd", "csrc", "stage_e_audience.hip")).read()
    m = re.search(r"constexpr int AU_WINDOW = 1 << (\d+);", src)
    assert m
    return 1 << int(m.group(1))


# ---------------------------------------------------------------------------------------------- the brute-force statement
def by_item(scored):
    """score_users' {user: [(item, plain, decayed, now, held)*]} -> {item: [(user, plain, decayed, now, held)*]}, users ascending"""
    out = {}
    for u in sorted(scored):
        for i, plain, decayed, now, held in scored[u]:
            out.setdefault(i, []).append((u, plain, decayed, now, held))
    return out


def statement(arrays, keep, alpha=ALPHA, users=None):
    """the inverted scores of every user with rows (or of `users`, which must then hold every user with rows)"""
    ptr = arrays[0]
    with_rows = np.nonzero(np.diff(ptr) > 0)[0]
    if users is not None:
        assert set(with_rows.tolist()) <= set(users)
    return by_item(score_users(alpha, with_rows.tolist(), *arrays[:8], keep))


# ------------------------------------------------------------------------------------------------------- the drivers
def audience(ctx, queries, n, rank_by, flags, alpha=ALPHA, n_w=66, name="xmap_ctx_audience"):
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    cnt, user = np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32)
    plain, decay, stats = np.full((Q, n), -7.0), np.full((Q, n), -7.0), np.zeros(4, np.int64)
    ctx.call(name, Q, _p(q, C.c_int32), n, rank_by, flags, _p(w, C.c_double), n_w, _p(cnt, C.c_int32),
             _p(user, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), _p(stats, C.c_int64))
    return cnt, user, plain, decay, stats.tolist()


class OnDevice(object):
    """device copies of (ptr, item, rating, time, cnt, col, sim, avg): uploaded once per case"""

    def __init__(self, arrays):
        import torch
        self.t = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays[:8]]


def audience_rows(arrays, n_users, n_items, keep, alpha, n_w, queries, n, rank_by=0, flags=0):
    """xmap_audience_rows on device copies of (ptr, item, rating, time, cnt, col, sim, avg, ...) or on an OnDevice of them"""
    import torch
    from xmap.engine import hipabi as abi
    dev = "cuda:0"
    ptr, pit, pra, pti, cnt, col, sim, avg = (arrays if isinstance(arrays, OnDevice) else OnDevice(arrays)).t
    q = torch.from_numpy(np.ascontiguousarray(queries, np.int32)).to(dev)
    Q = int(q.numel())
    w = torch.from_numpy(wtab(alpha, n_w)).to(dev)
    o_cnt = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    o_user = torch.full((Q, n), -7, dtype=torch.int32, device=dev)
    o_plain = torch.full((Q, n), -7.0, dtype=torch.float64, device=dev)
    o_decay = torch.full((Q, n), -7.0, dtype=torch.float64, device=dev)
    h = (C.c_int64 * 4)(0, 0, 0, 0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    abi.check(abi.lib.xmap_audience_rows(st, abi.i64(Q), abi.vp(q), abi.i32(n), abi.i32(rank_by), abi.i32(flags), abi.i64(n_users),
                                         abi.i32(n_items), abi.i32(keep), abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ptr),
                                         abi.vp(pit), abi.vp(pra), abi.vp(pti), abi.vp(avg), abi.vp(w), abi.i32(n_w), abi.vp(o_cnt),
                                         abi.vp(o_user), abi.vp(o_plain), abi.vp(o_decay), h))
    return o_cnt.cpu().numpy(), o_user.cpu().numpy(), o_plain.cpu().numpy(), o_decay.cpu().numpy(), [int(x) for x in h]


def _profiles(U, rows):
    """{user: [(item, rating, time)*]} -> ptr, item, rating, time"""
    ptr = np.zeros(U + 1, np.int64)
    for u, l in rows.items():
        ptr[u + 1] = len(l)
    np.cumsum(ptr, out=ptr)
    flat = [x for u in sorted(rows) for x in rows[u]]
    return (ptr, np.asarray([x[0] for x in flat], np.int32), np.asarray([x[1] for x in flat], np.float64),
            np.asarray([x[2] for x in flat], np.int64))


def _lists(I, keep, lists):
    """{item: (cnt, [neighbour*], [sim*])} -> cnt, col, sim"""
    cnt, col, sim = np.zeros(I, np.int32), np.full((I, keep), -1, np.int32), np.zeros((I, keep))
    for i, (c, nbs, ss) in lists.items():
        cnt[i] = c
        col[i, :len(nbs)] = nbs
        sim[i, :len(ss)] = ss
    return cnt, col, sim


# ------------------------------------------------------------------------------------------------------- 1. hand case
TINY = 5e-324       # the smallest subnormal: -TINY / 4 rounds to -0.0


def _hand_case():
    U, I, keep = 24, 8, 4
    rows = {
        0: [(1, 2.0, 0)],                                        # 2.0
        1: [(1, -2.0, 0)],                                       # -2.0: the same magnitude, the other sign
        2: [(1, 2.0, 1), (2, 2.0, 0), (1, 2.0, 2)],              # through two neighbours, one of them held twice: once, 2.0
        3: [(0, 4.0, 0), (1, 3.0, 1)],                           # holds item 0
        4: [(3, 5.0, 0)],                                        # only the neighbour with similarity 0: the statement raises
        5: [(1, 1.0, t) for t in range(5)],                      # five distinct times: now = 6
        6: [],
        10: [(1, 0.0, 0)],                                       # 0.0
        11: [(1, -TINY, 0), (2, 0.0, 0)],                        # -0.0
        12: [(2, 0.0, 1)],                                       # 0.0
        13: [(1, -TINY, 0), (2, 0.0, 0)],                        # -0.0
        15: [(4, 3.0, 0)],                                       # item 5 only
        16: [(1, 1.0, 0), (4, 2.0, 1), (5, 5.0, 2)],             # holds item 5
        20: [(1, 5.0, 3)],
        21: [(2, 4.0, 3)],
        22: [(1, 2.0, 0), (2, 2.0, 0)],                          # 2.0 again
        23: [(1, -2.0, 1)],
    }
    lists = {0: (4, [1, 2, 3, I + 1], [1.0, 3.0, 0.0, 0.7]),
             5: (6, [4, -3, 1, 1], [0.5, 0.9, -0.25, 0.75]),     # cnt beyond keep, an entry below 0, a repeated neighbour
             6: (-1, [1, 2], [1.0, 1.0]),
             7: (0, [1, 2], [1.0, 1.0])}
    avg = np.asarray([-0.0, 0.0, 0.0, 0.0, 1.5, 2.0, 0.25, 3.0])
    return list(_profiles(U, rows)) + list(_lists(I, keep, lists)) + [avg], U, I, keep


@pytest.mark.parametrize("rank_by", [0, 1])
def test_hand_case(rank_by):
    arrays, U, I, keep = _hand_case()
    inv = statement(arrays, keep)
    zero = {c[0]: c[1] for c in inv[0] if c[1] == 0.0}
    assert sorted(zero) == [10, 11, 12, 13] and [bool(np.signbit(zero[u])) for u in (10, 11, 12, 13)] == [False, True, False, True]
    assert [c[0] for c in inv[0]].count(2) == 1 and [c for c in inv[0] if c[0] == 4][0][1] is None
    assert [c[3] for c in inv[0] if c[0] == 5] == [6] and [c[4] for c in inv[0] if c[0] == 3] == [True]
    assert {c[1] for c in inv[0] if c[0] in (0, 2, 22)} == {2.0} and {c[1] for c in inv[0] if c[0] in (1, 23)} == {-2.0}
    queries = [0, 5, -1, I, 7, 6, 0]
    D = OnDevice(arrays)
    for flags in (0, KEEP_HOLDERS):
        for n in (1, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 64, 100, 1024):
            short = audience_rows(D, U, I, keep, ALPHA, 4, queries, n, rank_by, flags)
            want = expected(inv, queries, n, rank_by, bool(flags), 4)
            check_output(short, want, n)
            assert short[4][2] == 6                                 # user 5 asks for a longer table
            assert short[0][2:6].tolist() == [0, 0, 0, 0] and short[1][0].tolist() == short[1][6].tolist()
            full = audience_rows(D, U, I, keep, ALPHA, 6, queries, n, rank_by, flags)
            want = expected(inv, queries, n, rank_by, bool(flags), 6)
            check_output(full, want, n)
            assert short[4][1] > full[4][1] == 2                    # user 4 stays dropped for its zero weight sum (item 0 is asked twice)
            assert (5 in full[1][0]) == (n >= 6 + flags) and 5 not in short[1][0] and (3 in full[1][0]) == (bool(flags) and n >= 3)
            assert n < 64 or any(0 < len(l) < n for l in want[0])   # a segment shorter than n_top
    # the cut between 0.0 and -0.0 falls by user index
    got = audience_rows(D, U, I, keep, ALPHA, 6, queries, 10, rank_by, 0)
    assert got[1][0].tolist() == [20, 21, 0, 2, 22, 5, 16, 10, 11, 12]
    assert 16 not in got[1][1] and 15 in got[1][1]                    # item 5: its holder left out


# ------------------------------------------------------------------------------------------------------ 2. window edge
def test_a_user_space_just_above_the_window():
    W = _window()
    U, I, keep = W + 70, 30, 3
    rng = np.random.default_rng(31)
    users = np.unique(np.concatenate([[0, W - 1, W, W + 69], rng.integers(0, U, 20), rng.integers(W, U, 12)]))
    rows = {int(u): [(int(i), float(rng.integers(2, 21)) / 4.0, int(rng.integers(0, 4))) for i in rng.choice(np.arange(8, I), 5, replace=False)]
            for u in users}
    lists = {i: (keep, rng.choice(np.arange(8, I), keep, replace=False).tolist(), np.round(rng.normal(size=keep), 2).tolist()) for i in range(8)}
    for u, i in ((W - 1, 2), (W, 2), (W + 69, 3)):           # holders of query items at the window's edges, with evidence
        rows[u] += [(i, 3.0, 0), (lists[i][1][0], 2.5, 2)]
    avg = np.round(rng.uniform(1.0, 5.0, I), 1)
    arrays = list(_profiles(U, rows)) + list(_lists(I, keep, lists)) + [avg]
    inv = statement(arrays, keep)
    D = OnDevice(arrays)
    queries = list(range(8)) + [2]
    for n, rank_by, flags in ((64, 0, 0), (64, 1, KEEP_HOLDERS), (5, 0, KEEP_HOLDERS), (100, 1, 0)):
        want = expected(inv, queries, n, rank_by, bool(flags), 66)
        check_output(audience_rows(D, U, I, keep, ALPHA, 66, queries, n, rank_by, flags), want, n)
        if n >= 64:
            got = {c[0] for l in want[0] for c in l}
            assert {0, W - 1, W, W + 69} <= got
            assert all(min(c[0] for c in l) < W <= max(c[0] for c in l) for l in want[0])      # every list spans both windows
            assert (W - 1 in {c[0] for c in want[0][2]}) == bool(flags) and (W + 69 in {c[0] for c in want[0][3]}) == bool(flags)


# --------------------------------------------------------------------------------------------------- 3. long holder rows
def test_long_holder_rows_and_a_tie_across_the_cut():
    U, I, keep = 6000, 5, 2
    rng = np.random.default_rng(32)
    first = rng.permutation(U)[:5000]                   # the holders of neighbour 1: many strides of the block
    r1 = np.concatenate([np.full(40, 5.0), np.full(1000, 4.0), rng.integers(4, 15, 3960) / 4.0])
    r1 = dict(zip(first.tolist(), r1[rng.permutation(5000)].tolist()))
    second = rng.choice(first, 300, replace=False)      # of whom 300 hold neighbour 2 as well, half of them at the same rating
    rows = {u: [(1, r, int(u % 3))] for u, r in r1.items()}
    for k, u in enumerate(second.tolist()):
        rows[u].append((2, r1[u] if k % 2 else float(rng.integers(4, 21)) / 4.0, 1))
    for u in rng.choice(first, 50, replace=False).tolist():
        rows[u].insert(0, (0, 3.0, 0))                  # holders of the query item
    lists = {0: (2, [1, 2], [1.0, 1.0])}
    arrays = list(_profiles(U, rows)) + list(_lists(I, keep, lists)) + [np.asarray([2.5, 0.0, 0.0, 1.0, 1.0])]
    inv = statement(arrays, keep)
    tie = [c for c in inv[0] if c[1] == 6.5 and not c[4]]
    above = [c for c in inv[0] if c[1] > 6.5 and not c[4]]
    print("candidates %d, above the tie %d, in the tie %d" % (len(inv[0]), len(above), len(tie)))
    assert len(inv[0]) == 5000 and len(above) < 64 and len(above) + len(tie) > 1000 and len(tie) > 900
    D = OnDevice(arrays)
    for n in (64, 1000):
        for rank_by, flags in ((0, 0), (1, 0), (0, KEEP_HOLDERS)):
            want = expected(inv, [0], n, rank_by, bool(flags), 66)
            check_output(audience_rows(D, U, I, keep, ALPHA, 66, [0], n, rank_by, flags), want, n)
            assert want[1][3] == 5000 - (0 if flags else 50) and len(want[0][0]) == n


# ------------------------------------------------------------------------- 4. selection edges on designed score orders
@pytest.mark.parametrize("n_top", [1, 63, 64, 65, 1000, 1024])
def test_selection_edges_on_designed_score_orders(n_top):
    """query item q = (length, order) has the single neighbour Q + q with similarity 1, held by the users [0, length) at a rating
    that rises with the user index (every candidate displaces one), falls (none does after the first N) or is a permutation"""
    lengths = [0, 1, n_top - 1, n_top, n_top + 1, 3000]
    cases = [(L, order) for L in lengths for order in ("rising", "falling", "random")]
    Q, U, keep = len(cases), 3000, 1
    I = 2 * Q + 1
    rng = np.random.default_rng(33)
    rows = {u: [] for u in range(U)}
    for q, (L, order) in enumerate(cases):
        score = {"rising": np.arange(L), "falling": np.arange(L)[::-1], "random": rng.permutation(L)}[order] / 8.0
        for u in range(L):
            rows[u].append((Q + q, float(score[u]), u % 2))
    lists = {q: (1, [Q + q], [1.0]) for q in range(Q)}
    arrays = list(_profiles(U, rows)) + list(_lists(I, keep, lists)) + [np.zeros(I)]
    inv = statement(arrays, keep)
    assert [len(inv.get(q, [])) for q in range(Q)] == [L for L, _ in cases]
    queries = list(range(Q)) + [Q - 1, 0]
    D = OnDevice(arrays)
    for rank_by in (0, 1):
        want = expected(inv, queries, n_top, rank_by, False, 66)
        check_output(audience_rows(D, U, I, keep, ALPHA, 66, queries, n_top, rank_by, 0), want, n_top)
    rising, falling = cases.index((3000, "rising")), cases.index((3000, "falling"))
    k = min(n_top, 3000)
    assert [c[0] for c in want[0][rising]] == list(range(2999, 2999 - k, -1)) and [c[0] for c in want[0][falling]] == list(range(k))
    # a small and a large n_top in one sequence of calls on the same arrays: both selection sizes, the same answers
    other = 1024 if n_top <= 256 else 10
    check_output(audience_rows(D, U, I, keep, ALPHA, 66, queries, other, 0, 0), expected(inv, queries, other, 0, False, 66), other)
    check_output(audience_rows(D, U, I, keep, ALPHA, 66, queries, n_top, 1, 0), want, n_top)


# ------------------------------------------------------------------------------------------- 5. coarse ABI, NumPy only
@pytest.mark.parametrize("seed,users,src,tgt,overlap", [(5, 1500, 300, 300, 0.4), (7, 3000, 600, 80, 0.5)])
def test_audience_through_the_coarse_abi(seed, users, src, tgt, overlap):
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(seed, users, src, tgt, overlap=overlap))
    I, U, keep = r.n_items, users, 10
    rng = np.random.default_rng(seed)
    queries = np.concatenate([np.arange(r.n_src_items, I), rng.integers(0, r.n_src_items, 40), [-1, I, I + 3, r.n_src_items]]).astype(np.int32)
    tool = _tool(ALPHA)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        cnt, col, sim, _ = select(ctx, I, keep)
        arrays = [T["ptr"], T["item"], T["rating"], T["time"], cnt, col, sim, T["avg"]]
        inv = statement(arrays, keep)
        sizes = [len(inv.get(int(i), [])) for i in queries]
        print("candidates per query item: 0: %d, 1-10: %d, 11-200: %d, > 200: %d, largest %d" % (
            sum(s == 0 for s in sizes), sum(1 <= s <= 10 for s in sizes), sum(10 < s <= 200 for s in sizes), sum(s > 200 for s in sizes),
            max(sizes)))
        assert max(sizes) > 200 and sum(c[4] for l in inv.values() for c in l) > 0       # a list beyond N = 200; holders with evidence
        listed = {}
        for n in (10, 200):
            for rank_by in (0, 1):
                for flags in (0, KEEP_HOLDERS):
                    want = expected(inv, queries, n, rank_by, bool(flags), 66)
                    got = audience(ctx, queries, n, rank_by, flags)
                    check_output(got, want, n)
                    assert want[1][1] == 0 and want[1][2] <= 66
                    for i, l in zip(queries, want[0]):
                        for u, p, d in l:
                            listed[u, int(i)] = (p, d)
        assert got[0][-4:-1].tolist() == [0, 0, 0] and got[1][-1].tolist() == got[1][0].tolist()   # -1, I, I + 3; the item listed twice
        # the pairs that xmap_ctx_recommend lists for the same user carry the same bits
        us = sorted({u for u, _ in listed})
        rcnt, ritem, rplain, rdecay, _ = recommend(ctx, us, 64, 0, KEEP_HELD, ALPHA)
        shared = 0
        for q, u in enumerate(us):
            for t in range(rcnt[q]):
                mine = listed.get((u, int(ritem[q, t])))
                if mine is not None:
                    assert np.float64(mine[0]).view(np.uint64) == rplain[q, t].view(np.uint64)
                    assert np.float64(mine[1]).view(np.uint64) == rdecay[q, t].view(np.uint64)
                    shared += 1
        print("listed pairs %d, of them in the users' own top-64: %d" % (len(listed), shared))
        assert shared > 100
        # every returned score, rounded, is the prediction of the existing kernel for that pair
        pairs = sorted(listed)[::7]
        p_plain, p_decay, p_status, _, _ = predict(ctx, [p[0] for p in pairs], [p[1] for p in pairs], None, ALPHA)
        assert not p_status.any() and len(pairs) > 100
        assert p_plain.tolist() == [tool.bound_rating(listed[p][0]) for p in pairs]
        assert p_decay.tolist() == [tool.bound_rating(listed[p][1]) for p in pairs]
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------- 6. symmetry
def test_the_pair_set_is_the_one_of_topn():
    U, I, keep = 300, 400, 3
    arrays = _random_case(34, U, I, keep, np.arange(0, I, 2), lambda u: 2 + u % 7)
    for mine, theirs in ((0, 0), (KEEP_HOLDERS, KEEP_HELD)):
        a = audience_rows(arrays, U, I, keep, ALPHA, 66, list(range(I)), 1024, 0, mine)
        t = topn_rows(arrays, U, I, keep, ALPHA, 66, list(range(U)), 64, 0, theirs)
        assert 0 < a[4][3] < 1024 and 0 < t[4][3] < 64 and a[4][1] == t[4][1]            # no list was cut; the same pairs dropped
        from_items = {(int(a[1][i, k]), i): (a[2][i, k].tobytes(), a[3][i, k].tobytes()) for i in range(I) for k in range(a[0][i])}
        from_users = {(u, int(t[1][u, k])): (t[2][u, k].tobytes(), t[3][u, k].tobytes()) for u in range(U) for k in range(t[0][u])}
        assert a[4][0] == t[4][0] > 1000 and len(from_items) == a[4][0] - a[4][1]
        assert from_items == from_users


# ------------------------------------------------------------------------------------------------ 7. fold-in and union
def test_foldin_audience():
    from test_gpu_foldin import _same, foldin, foldin_download
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(3, 800, 200, 200, overlap=0.4))
    I, U, keep = r.n_items, 800, 10
    queries = np.concatenate([np.arange(r.n_src_items, I), [3, -1, I]]).astype(np.int32)
    settings = [(10, 0, 0), (200, 1, KEEP_HOLDERS), (64, 1, 0)]
    ctx = Ctx()
    try:
        generate(ctx, r)
        ctx.call("xmap_ctx_rec_sim", CAP, None)
        ctx.call("xmap_ctx_rec_select", keep)
        before = [audience(ctx, queries, *s) for s in settings]
        assert before[0][4][0] > 0 and before[1][0].max() > 10
        # the upload folded into itself: the resident answers
        counts = foldin(ctx, r.user_ptr, r.item, r.rating, r.time)
        for s, want in zip(settings, before):
            got = audience(ctx, queries, *s, name="xmap_ctx_foldin_audience")
            assert _same(got[:4], want[:4]) and got[4] == want[4], s
        # an ad-hoc batch: the statement over its downloaded profiles
        rng = np.random.default_rng(35)
        B = 150
        lens = rng.integers(0, 40, B)
        ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        item = rng.integers(0, I, ptr[-1]).astype(np.int32)
        rating = (rng.integers(2, 21, len(item)) / 4.0).astype(np.float32)
        time = 1000 + rng.integers(0, 7, len(item)).astype(np.int64)
        counts = foldin(ctx, ptr, item, rating, time)
        fp = foldin_download(ctx, B, counts[0])
        cnt, col, sim, _ = neighbors(ctx, I, keep)
        avg = np.zeros(I)
        ctx.call("xmap_ctx_rec_download", None, None, None, None, None, _p(avg, C.c_double), None)
        inv = statement(list(fp) + [cnt, col, sim, avg], keep)
        for n, rank_by, flags in settings:
            want = expected(inv, queries, n, rank_by, bool(flags), 66)
            got = audience(ctx, queries, n, rank_by, flags, name="xmap_ctx_foldin_audience")
            check_output(got, want, n)
            assert want[1][0] > 0 and got[1].max() < B
        # resident answers are unchanged afterwards
        for s, want in zip(settings, before):
            again = audience(ctx, queries, *s)
            assert _same(again[:4], want[:4]) and again[4] == want[4]
    finally:
        ctx.close()


def test_audience_on_a_union_context():
    from test_gpu_union import _trained_domains, _union
    doms = _trained_domains("multi", 2)
    numbers = np.unique(np.concatenate([r.tgt_numbers for r in doms]))
    U, I, keep = doms[0].n_users, len(numbers), 10
    rng = np.random.default_rng(36)
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
        assert rc == 0 and counts[0] > 0
        T = rec_sim(dst, I, U, counts[0])
        cnt, col, sim, _ = select(dst, I, keep)
        inv = statement([T["ptr"], T["item"], T["rating"], T["time"], cnt, col, sim, T["avg"]], keep)
        queries = np.concatenate([np.arange(I), [-1, I]]).astype(np.int32)
        for n, rank_by, flags in ((10, 0, 0), (100, 1, KEEP_HOLDERS)):
            want = expected(inv, queries, n, rank_by, bool(flags), 66)
            check_output(audience(dst, queries, n, rank_by, flags), want, n)
            assert want[1][0] > 0
        assert dst.lib.xmap_ctx_foldin_audience(dst.h, 0, None, 1, 0, 0, _p(wtab(ALPHA, 4), C.c_double), 4, None, None, None, None,
                                                None) == dst.abi.ERR_ARG          # a union takes no fold-in batch
    finally:
        for c in srcs + [dst]:
            c.close()


# ---------------------------------------------------------------------------------------------- 8. the Python route
def test_session_recommend_audience_equals_the_statement_on_id_strings():
    """the construction of test_gpu_topn.test_session_recommend_topn_equals_the_statement_on_id_strings, inverted: per item the
    users, from the collected dictionaries; equal scores in the order of the train set's users"""
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
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
    order = {uid: k for k, uid in enumerate(ae.state.idt.uids)}
    item_based = RecommenderSim("cosine_item", CAP).build_sthbased_profile(ae, "item").collectAsMap()
    ptool = _tool(ALPHA)
    held = {}                                     # {uid: {iid: [(rating, time)*]}} in the order of the item's list
    for iid, lst in item_based.items():
        for who, ra, when in lst:
            held.setdefault(who, {}).setdefault(iid, []).append((ra, when))
    rng = np.random.default_rng(9)
    known = sorted(item_based)
    iids = [known[int(x)] for x in rng.integers(0, len(known), 60)] + ["B%013dT:" % (10 ** 9 + 1)]

    def statement_ids(sim_pairs, item_info, n, decay, keep_holders):
        out = []
        for iid in iids:
            cand = []
            for uid in sorted(held, key=order.get) if iid in sim_pairs else ():
                if not keep_holders and iid in held[uid]:
                    continue
                ev = [(s * (ra - item_info[nid][0]), abs(s), when) for nid, s in sim_pairs[iid] for ra, when in held[uid].get(nid, ())]
                if ev:
                    base = item_info[iid][0]
                    cand.append((uid, base + sum(e[0] for e in ev) / sum(e[1] for e in ev), float(base + ptool._decayed_ratio(ev))))
            cand.sort(key=lambda c: (- c[2 if decay else 1], order[c[0]]))
            out.append((iid, cand[:n]))
        return out

    first = None
    for n, decay, keep_holders in ((10, False, False), (100, True, False), (3, True, True)):
        out = session.recommend_audience(ae, iids, CAP, 10, ALPHA, n, decay=decay, keep_holders=keep_holders)
        assert out.collect() == statement_ids(out.sim_pairs, out.item_info, n, decay, keep_holders)
        assert out.stats[1] == 0 and out.stats[0] > 0
        if first is None:
            first = out
    assert out.collect()[-1] == (iids[-1], []) and any(len(l) == 10 for _, l in first.collect())
    # the same records under new uids, folded in: the same audiences under the new names
    again = session.recommend_audience_profiles(ae, [("N" + u, prof) for u, prof in recs], LocalRDD(iids), CAP, 10, ALPHA, 10)
    assert again.collect() == [(iid, [("N" + u, p, d) for u, p, d in l]) for iid, l in first.collect()]
    with pytest.raises(TypeError):
        session.recommend_audience(LocalRDD(ae.collect()), iids, CAP, 10, ALPHA, 10)


# ---------------------------------------------------------------------------------------------------- 9. lifecycle
def test_audience_lifecycle_and_argument_errors():
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(3, 800, 200, 200, overlap=0.4))
    I = r.n_items
    queries = np.arange(r.n_src_items, I).astype(np.int32)
    fresh = Ctx()
    try:
        generate(fresh, r)
        fresh.call("xmap_ctx_rec_sim", CAP, None)
        fresh.call("xmap_ctx_rec_select", 10)
        ref = audience(fresh, queries, 100, 1, 0, 0.2)
    finally:
        fresh.close()
    assert ref[4][0] > 0 and ref[0].max() > 10
    c = Ctx()
    try:
        ERR = c.abi.ERR_ARG
        q, w = np.zeros(1, np.int32), wtab(0.2, 8)
        oc, ou, op, od = np.full(1, -7, np.int32), np.full(4, -7, np.int32), np.full(4, -7.0), np.full(4, -7.0)

        def raw(n_query=1, qi=q, n=4, rank_by=0, flags=0, tab=w, n_w=8, out=(oc, ou, op, od), name="xmap_ctx_audience"):
            return getattr(c.lib, name)(c.h, n_query, _p(qi, C.c_int32), n, rank_by, flags, _p(tab, C.c_double), n_w,
                                        _p(out[0], C.c_int32), _p(out[1], C.c_int32), _p(out[2], C.c_double), _p(out[3], C.c_double), None)

        def same_error_as_recommend():
            rc = raw()
            mine = c.lib.xmap_last_error()
            assert rc == ERR and raw(name="xmap_ctx_recommend") == ERR
            theirs = c.lib.xmap_last_error()
            assert re.sub(rb"^\S+", b"", mine) == re.sub(rb"^\S+", b"", theirs)      # the same refused condition, another line
        same_error_as_recommend()                                            # before upload
        rows = generate(c, r)
        same_error_as_recommend()                                            # before rec_sim
        c.call("xmap_ctx_rec_sim", CAP, None)
        same_error_as_recommend()                                            # before rec_select
        assert b"have_nb" in c.lib.xmap_last_error()
        assert raw(name="xmap_ctx_foldin_audience") == ERR and b"have_fold" in c.lib.xmap_last_error()
        c.call("xmap_ctx_rec_select", 10)
        assert raw(name="xmap_ctx_foldin_audience") == ERR                   # no batch
        # argument errors: refused before any device work, the outputs untouched, the context working
        for kw in (dict(n=0), dict(n=1025), dict(rank_by=2), dict(rank_by=-1), dict(flags=2), dict(flags=-1), dict(n_w=0),
                   dict(out=(None, ou, op, od)), dict(out=(oc, None, op, od)), dict(out=(oc, ou, None, od)),
                   dict(out=(oc, ou, op, None)), dict(qi=None), dict(tab=None)):
            assert raw(**kw) == ERR, kw
            assert c.lib.xmap_last_error()
            assert oc[0] == -7 and (ou == -7).all() and (op == -7.0).all() and (od == -7.0).all()
        assert raw(n_query=0, qi=None, out=(None, None, None, None)) == 0    # nothing to do, nothing touched
        assert raw() == 0 and oc[0] != -7
        got = audience(c, queries, 100, 1, 0, 0.2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], ref[:4])) and got[4] == ref[4]
        c.call("xmap_ctx_item_sim", 0, CAP, None, None)                      # an earlier stage run again drops the tail
        same_error_as_recommend()
        c.call("xmap_ctx_extend", 5, None, None)
        stage_c(c, I, True, None)
        c.call("xmap_ctx_rec_sim", CAP, None)
        same_error_as_recommend()
        c.call("xmap_ctx_rec_select", 10)
        got = audience(c, queries, 100, 1, 0, 0.2)                           # the reused context: the bytes of a fresh one
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], ref[:4])) and got[4] == ref[4]
        generate(c, r)                                                       # an upload drops it as well
        same_error_as_recommend()
        assert len(rows["user"]) > 0
    finally:
        c.close()
