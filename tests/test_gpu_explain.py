"""Explanation of a recommendation on the device (csrc/stage_e_explain.hip; xmap_explain_rows, xmap_explain_sources,
xmap_ctx_explain, xmap_ctx_foldin_explain, Engine.explain / explain_sources, session.explain and the explain= option): for
(user, item) pairs the strongest evidence entries of the score with their shares, and for each of those AlterEgo rows the raw
ratings of the user that stage C made it from.

Every expectation is a brute-force Python statement written here, fed only with host arrays: the evidence loop of
test_gpu_topn.score_user extended by shares and ranking, and a plain loop over the raw profile with the map for the sources.
Everything is exact fp64 in a stated order: every comparison is array_equal on the bits.

One case of the issue cannot exist on a resident context: xmap_ctx_upload_ratings refuses an item twice in one profile and the
replacement map sends a source item to one target and no two sources to the same target, so the group behind a resident mapped
row has exactly one member.  Groups larger than n_src are covered where they can occur: a fold-in batch that repeats a source
item, and the fine-grained entry with a hand-made map that merges sources."""
import ctypes as C
import math
import types

import numpy as np
import pytest

from golden_util import CAP
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_foldin import foldin, foldin_download, map_of
from test_gpu_tail import _few_times, generate, rec_sim, select, wtab
from test_gpu_topn import _hand_case, recommend

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PR_CAP = 128


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


# ---------------------------------------------------------------------------------------------- the brute-force statements
def explain_pair(u, i, ptr, pit, pra, pti, cnt, col, sim, avg, keep, w, n_ev, rank_by):
    """one pair: (status, total, score, [(row, slot, share)*] ranked, now or 0)"""
    I, U = len(cnt), len(ptr) - 1
    width = min(max(int(cnt[i]), 0), keep) if 0 <= i < I else 0
    if width <= 0:
        return 1, 0, 0.0, [], 0
    base = float(avg[i])
    a, b = (int(ptr[u]), int(ptr[u + 1])) if 0 <= u < U else (0, 0)
    ev = []                                             # (e0, e1, time, row, slot) in evidence order
    for l in range(width):
        nb = int(col[i, l])
        if not 0 <= nb < I:
            continue
        s, navg = float(sim[i, l]), float(avg[nb])
        for p in range(a, b):
            if pit[p] == nb:
                ev.append((s * (float(pra[p]) - navg), abs(s), int(pti[p]), p, l))
    n = len(ev)
    if n == 0:
        return (0, 0, base, [], 0) if math.isfinite(base) else (2, 0, 0.0, [], 0)
    p0 = p1 = 0.0
    for e in ev:
        p0 += e[0]
        p1 += e[1]
    rank = {t: k + 1 for k, t in enumerate(sorted({e[2] for e in ev}))}
    now = len(rank) + 1
    if now > len(w) or p1 == 0.0:
        return 2, 0, 0.0, [], now
    plain = base + p0 / p1
    d0 = d1 = 0.0
    wt = [float(w[now - rank[e[2]]]) for e in ev]
    for q in sorted(range(n), key=lambda q: ev[q][2]):  # stable: equal times keep the evidence order
        d0 += ev[q][0] * wt[q]
        d1 += ev[q][1] * wt[q]
    if d1 == 0.0:
        return 2, 0, 0.0, [], now
    decayed = base + d0 / d1
    if not (math.isfinite(base) and math.isfinite(plain) and math.isfinite(decayed)):
        return 2, 0, 0.0, [], now
    share = [(ev[q][0] * wt[q]) / d1 if rank_by else ev[q][0] / p1 for q in range(n)]
    best = sorted(range(n), key=lambda q: (- abs(share[q]), q))[:n_ev]
    return 0, n, (decayed if rank_by else plain), [(ev[q][3], ev[q][4], share[q]) for q in best], now


def explain_statement(pu, pi, arrays, keep, w, n_ev, rank_by):
    """the seven outputs + max_now of the pairs, as the device lays them out"""
    ptr, pit, pra, pti, cnt, col, sim, avg = arrays[:8]
    pit, pra, pti = np.asarray(pit).tolist(), np.asarray(pra).tolist(), np.asarray(pti).tolist()
    T = len(pu)
    status, total, n_rep, score = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T)
    row, slot, share = np.full((T, n_ev), -1, np.int64), np.full((T, n_ev), -1, np.int32), np.zeros((T, n_ev))
    max_now = 0
    for t, (u, i) in enumerate(zip(pu, pi)):
        st, n, sc, entries, now = explain_pair(int(u), int(i), ptr, pit, pra, pti, cnt, col, sim, avg, keep, w, n_ev, rank_by)
        status[t], total[t], n_rep[t], score[t] = st, n, len(entries), sc
        for e, (p, l, sh) in enumerate(entries):
            row[t, e], slot[t, e], share[t, e] = p, l, sh
        max_now = max(max_now, now)
    return status, total, n_rep, score, row, slot, share, max_now


def sources_statement(pu, n_rep, row, ptr, pit, cnt_t, raw_ptr, raw_item, flags, m, n_src):
    """(src_total [T][n_ev], src_pos [T][n_ev][n_src]): a plain loop over the user's raw profile"""
    T, n_ev, U, I = len(pu), row.shape[1], len(ptr) - 1, len(flags)
    total, pos = np.zeros((T, n_ev), np.int32), np.full((T, n_ev, n_src), -1, np.int64)
    for t in range(T):
        u = int(pu[t])
        for e in range(min(int(n_rep[t]), n_ev)):
            p = int(row[t, e])
            if not (0 <= u < U and ptr[u] <= p < ptr[u + 1]):
                total[t, e] = -1
                continue
            k = p - int(ptr[u])
            raw = [x for x in range(int(raw_ptr[u]), int(raw_ptr[u + 1])) if 0 <= raw_item[x] < I]
            if k < cnt_t[u]:
                src = [x for x in raw if flags[raw_item[x]] & 2][k:k + 1]
            else:
                src = [x for x in raw if m[raw_item[x]] == pit[p]]
            total[t, e] = len(src)
            pos[t, e, :min(len(src), n_src)] = src[:n_src]
    return total, pos


def same(got, want, what=""):
    for k, (g, x) in enumerate(zip(got, want)):
        g, x = np.asarray(g), np.asarray(x)
        assert g.shape == x.shape and g.dtype == x.dtype, (what, k, g.shape, x.shape, g.dtype, x.dtype)
        assert g.tobytes() == x.tobytes(), (what, k, np.argwhere(g != x)[:5].tolist())


# ------------------------------------------------------------------------------------------------------- the drivers
def _engine():
    from xmap.engine import device
    eng = object.__new__(device.Engine)
    eng.dev, eng.timers, eng._scratch = DEV, None, {}
    return eng


def _to(a, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)


def _view(arrays, U, I):
    ptr, pit, pra, pti = arrays[:4]
    return types.SimpleNamespace(n_users=U, n_items=I, user_ptr=_to(ptr, np.int64), user_item=_to(pit, np.int32),
                                 user_rating64=_to(pra, np.float64), user_time=_to(pti, np.int64))


def engine_explain(arrays, U, I, pu, pi, w, n_ev, rank_by, P=None):
    """Engine.explain on device copies of (ptr, item, rating, time, cnt, col, sim, avg): the eight results as NumPy"""
    eng = _engine()
    P = P or _view(arrays, U, I)
    nb = (_to(arrays[4], np.int32), _to(arrays[5], np.int32), _to(arrays[6], np.float64))
    out = eng.explain(P, nb, _to(pu, np.int32), _to(pi, np.int32), _to(arrays[7], np.float64), _to(w, np.float64), n_ev, rank_by)
    return tuple(x.cpu().numpy() for x in out[:7]) + (out[7],)


def ctx_explain(ctx, pu, pi, rank_by, n_ev, n_src, alpha, n_w=66, entry="xmap_ctx_explain", rc=False):
    pu, pi = np.ascontiguousarray(pu, np.int32), np.ascontiguousarray(pi, np.int32)
    T, w = len(pu), wtab(alpha, n_w)
    status, total, n_rep, score = np.full(T, -7, np.int32), np.full(T, -7, np.int32), np.full(T, -7, np.int32), np.full(T, -7.0)
    row, slot, share = np.full((T, n_ev), -7, np.int64), np.full((T, n_ev), -7, np.int32), np.full((T, n_ev), -7.0)
    s_total = np.full((T, n_ev), -7, np.int32) if n_src else None
    s_pos = np.full((T, n_ev, n_src), -7, np.int64) if n_src else None
    max_now = C.c_int32(-1)
    code = getattr(ctx.lib, entry)(ctx.h, T, _p(pu, C.c_int32), _p(pi, C.c_int32), rank_by, n_ev, n_src, _p(w, C.c_double), n_w,
                                   _p(status, C.c_int32), _p(total, C.c_int32), _p(n_rep, C.c_int32), _p(score, C.c_double),
                                   _p(row, C.c_int64), _p(slot, C.c_int32), _p(share, C.c_double), _p(s_total, C.c_int32),
                                   _p(s_pos, C.c_int64), C.byref(max_now))
    if rc:
        return code
    ctx.abi.check(code)
    return (status, total, n_rep, score, row, slot, share, max_now.value), (s_total, s_pos)


def pairs_of_lists(queries, cnt, item):
    pu = [int(u) for u, c in zip(queries, cnt) for _ in range(int(c))]
    pi = [int(item[q, t]) for q, c in enumerate(cnt) for t in range(int(c))]
    return np.asarray(pu, np.int32), np.asarray(pi, np.int32)


def pairs_over_mapped_rows(T, cnt_t, cnt, col, keep, limit=400):
    """(user, item) pairs whose evidence holds a MAPPED row of the user: for the mapped rows of the profiles, in order, the items
    whose list holds the row's item"""
    lists_with = {}
    for i in range(len(cnt)):
        for x in col[i, :min(max(int(cnt[i]), 0), keep)].tolist():
            lists_with.setdefault(x, []).append(i)
    pu, pi = [], []
    for u in range(len(T["ptr"]) - 1):
        for p in range(int(T["ptr"][u]) + int(cnt_t[u]), int(T["ptr"][u + 1])):
            for i in lists_with.get(int(T["item"][p]), [])[:2]:
                pu.append(u)
                pi.append(i)
        if len(pu) >= limit:
            break
    return np.asarray(pu, np.int32), np.asarray(pi, np.int32)


# -------------------------------------------------------------------------------------------------------- 1. hand case
def _tiny_case():
    """I = 8, keep = 3, three users.  Items 0..3 are target items, 4..7 source items; the hand-made map merges the sources 5 and
    6 onto target 1 and sends 7 to 3.  User 0's raw profile gives the AlterEgo profile (stage C's order: pass-through rows, then
    mapped rows) [(1, 4.0, 10), (2, 2.0, 30), (3, 1.0, 40), (1, 2.0, 20), (3, 5.0, 50)]: neighbour item 1 twice, once as a
    pass-through and once as a mapped row.  User 1 has no rows."""
    I, keep = 8, 3
    flags = np.asarray([2, 2, 2, 2, 1, 1, 1, 1], np.uint8)
    m = np.asarray([-1, -1, -1, -1, -1, 1, 1, 3], np.int32)
    raw = [[(5, 3.0, 20), (1, 4.0, 10), (6, 1.0, 5), (2, 2.0, 30), (7, 5.0, 50), (3, 1.0, 40), (4, 2.0, 60)],
           [(4, 3.0, 7)],
           [(2, 5.0, 11), (7, 2.0, 12), (0, 3.0, 13)]]
    prof, cnt_t = [], []
    for r in raw:
        rows = [(it, float(ra), tm) for it, ra, tm in r if flags[it] & 2]
        cnt_t.append(len(rows))
        groups = {}
        for it, ra, tm in r:
            if m[it] >= 0:
                groups.setdefault(int(m[it]), []).append((float(ra), tm))
        for tgt, g in groups.items():
            s = 0.0
            for x in g:
                s += x[0]
            rows.append((tgt, s / len(g), g[0][1]))
        prof.append(rows)
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in prof])]).astype(np.int64)
    flat = [e for p in prof for e in p]
    pit, pra, pti = np.asarray([e[0] for e in flat], np.int32), np.asarray([e[1] for e in flat]), np.asarray([e[2] for e in flat], np.int64)
    raw_ptr = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
    raw_item = np.asarray([e[0] for r in raw for e in r], np.int32)
    cnt, col, sim = np.zeros(I, np.int32), np.full((I, keep), -1, np.int32), np.zeros((I, keep))
    cnt[0], col[0], sim[0] = 3, [1, 2, 3], [0.5, -0.5, 0.25]
    cnt[5], col[5, :2], sim[5, :2] = 2, [1, 2], [0.0, 0.0]          # a zero weight sum
    cnt[6], col[6], sim[6] = 3, [1, 9, -1], [0.75, 0.5, 0.5]        # list entries out of range
    cnt[7], col[7], sim[7] = 5, [2, 3, 1], [1.0, -0.25, 0.125]      # a count above keep
    avg = np.asarray([3.0, 2.0, 0.0, 1.5, 1.0, 2.5, 3.25, 0.5])
    arrays = [ptr, pit, pra, pti, cnt, col, sim, avg]
    return arrays, 3, I, keep, np.asarray(cnt_t, np.int32), raw_ptr, raw_item, flags, m


TINY_PAIRS = [(0, 0), (0, 4), (0, 5), (0, 6), (0, 7), (1, 0), (-1, 0), (6, 0), (0, -1), (0, 10), (2, 0), (2, 7), (1, 4)]


def test_the_hand_case_holds_what_it_should():
    arrays, U, I, keep = _tiny_case()[:4]
    w = wtab(0.5, 66)
    one = lambda u, i, n_ev, rank_by, tab=w: explain_pair(u, i, *arrays, keep, tab, n_ev, rank_by)
    st, n, score, plain, now = one(0, 0, 16, 0)
    assert (st, n, now) == (0, 5, 6) and [e[1] for e in plain].count(0) == 2          # neighbour 1 twice: two entries of slot 0
    # two entries with exactly equal |share| and opposite signs: the smaller evidence index goes first
    assert plain[0][2] == - plain[1][2] and plain[0][2] > 0 and plain[0][0] < plain[1][0] and plain[0][1] < plain[1][1]
    decayed = one(0, 0, 16, 1)[3]
    assert [e[0] for e in decayed] != [e[0] for e in plain]                            # the decayed ranking differs
    assert one(0, 4, 3, 0)[0] == 1 and one(0, 5, 3, 0)[0] == 2 and one(0, 0, 3, 0, w[:2])[0] == 2
    assert one(1, 0, 3, 0)[:4] == (0, 0, 3.0, []) and one(6, 0, 3, 1)[:4] == (0, 0, 3.0, []) and one(0, 10, 3, 0)[0] == 1
    assert one(0, 6, 16, 0)[1] == 2                                                   # the entries 9 and -1 are skipped


@pytest.mark.parametrize("rank_by", [0, 1])
@pytest.mark.parametrize("n_ev", [1, 2, 16])
def test_hand_case_through_the_engine(n_ev, rank_by):
    arrays, U, I, keep, cnt_t, raw_ptr, raw_item, flags, m = _tiny_case()
    pu, pi = [p[0] for p in TINY_PAIRS], [p[1] for p in TINY_PAIRS]
    for n_w in (66, 2):                                                               # 2: too short for the pair (0, 0)
        w = wtab(0.5, n_w)
        want = explain_statement(pu, pi, arrays, keep, w, n_ev, rank_by)
        got = engine_explain(arrays, U, I, pu, pi, w, n_ev, rank_by)
        same(got[:7], want[:7], "n_w %d" % n_w)
        assert got[7] == want[7] == 6
        assert (want[0] == 2).sum() == 1 if n_w == 66 else (want[0] == 2).sum() > 3
    # the sources of the reported rows, with the hand-made map that merges two sources
    eng, P = _engine(), _view(arrays, U, I)
    got = engine_explain(arrays, U, I, pu, pi, wtab(0.5, 66), n_ev, rank_by, P)
    src = (_to(raw_ptr), _to(raw_item), _to(cnt_t), None, _to(flags), _to(m))
    for n_src in (1, 2, 8):
        total, pos = eng.explain_sources(P, _to(pu, np.int32), _to(got[2]), _to(got[4]), n_src, sources=src)
        want = sources_statement(pu, got[2], got[4], arrays[0], arrays[1], cnt_t, raw_ptr, raw_item, flags, m, n_src)
        same((total.cpu().numpy(), pos.cpu().numpy()), want, "n_src %d" % n_src)
        if n_ev == 16:
            assert (want[0] == 2).any() and (want[0] == 1).any() and (want[0] == 0).any()   # the merged group, single sources, padding
    # the scan of the counts in place of the counts; a row outside the user's profile and a user out of range index nothing
    off_t = np.concatenate([[0], np.cumsum(cnt_t)]).astype(np.int64)
    rows = got[4].copy()
    rows[0, 0] = arrays[0][1]                       # the first row of user 1
    users = np.asarray(pu, np.int32)
    total, pos = eng.explain_sources(P, _to(users), _to(got[2]), _to(rows), 2, sources=(src[0], src[1], None, _to(off_t), src[4], src[5]))
    want = sources_statement(users, got[2], rows, arrays[0], arrays[1], cnt_t, raw_ptr, raw_item, flags, m, 2)
    same((total.cpu().numpy(), pos.cpu().numpy()), want)
    assert want[0][0, 0] == -1 and (want[1][0, 0] == -1).all()


# ------------------------------------------------------------------------------------------- 2. beyond the LDS staging
def _staging_case():
    """test_gpu_topn._hand_case (a user holding one neighbour 300 times) + two more users holding ONE neighbour 129 and 128 times:
    the boundary of the staging.  (arrays, users, items, keep, the 300-row user, the item whose list holds that one neighbour)"""
    arrays, U, I, keep, dup_user = _hand_case(copies=300)
    ptr, pit, pra, pti, cnt, col, sim, avg = arrays[:8]
    star = next(i for i in range(I) if cnt[i] >= 1 and 0 <= col[i, 0] < I and (col[i, :min(cnt[i], keep)] == col[i, 0]).sum() == 1)
    x = int(col[star, 0])
    extra = [129, 128]
    ptr = np.concatenate([ptr, ptr[-1] + np.cumsum(extra)]).astype(np.int64)
    pit = np.concatenate([pit, np.full(sum(extra), x, pit.dtype)])
    pra = np.concatenate([pra, 1.0 + (np.arange(sum(extra)) % 7) / 2.0])
    pti = np.concatenate([pti, (np.arange(sum(extra)) % 50).astype(np.int64) * 3600])
    return [ptr, pit, pra, pti, cnt, col, sim, avg], U + 2, I, keep, dup_user, star


def test_evidence_beyond_the_lds_staging():
    # both launches in one call
    arrays, U2, I, keep, dup_user, star = _staging_case()
    U = U2 - 2
    pu = [dup_user] * I + [U, U + 1, 3, 4, 5]
    pi = list(range(I)) + [star, star, 5, 5, 5]
    assert len(pu) % 4 != 0                             # a last block with idle waves
    w = wtab(1.5, 400)
    for n_ev, rank_by in ((16, 0), (16, 1), (3, 0)):
        want = explain_statement(pu, pi, arrays, keep, w, n_ev, rank_by)
        assert want[1].max() >= 300 > PR_CAP and want[1][I] == 129 and want[1][I + 1] == 128 and not want[0][I:I + 2].any()
        got = engine_explain(arrays, U2, I, pu, pi, w, n_ev, rank_by)
        same(got[:7], want[:7], (n_ev, rank_by))
        assert got[7] == want[7] > 129
        if (n_ev, rank_by) == (16, 0):
            # many equal shares: the reported rows are the first 16 in evidence order among them
            t = int(np.argmax(want[1]))
            tied = np.abs(want[6][t])
            assert len(set(tied.tolist())) < 16
            assert all(want[4][t, e] < want[4][t, e + 1] for e in range(15) if tied[e] == tied[e + 1] and want[5][t, e] == want[5][t, e + 1])
    short = engine_explain(arrays, U2, I, pu, pi, wtab(1.5, 66), 16, 1)                 # the table too short for the big pairs
    want = explain_statement(pu, pi, arrays, keep, wtab(1.5, 66), 16, 1)
    same(short[:7], want[:7])
    assert short[7] == want[7] and (want[0] == 2).sum() >= 1


# -------------------------------------------------------------------------------------------------------- 3. random case
def test_random_case_against_the_statement_the_prediction_and_the_lists():
    import torch
    U, I, keep, alpha = 200, 64, 8, 1.5
    rng = np.random.default_rng(31)
    # items repeat within a profile; every seventh user draws from eight items only: long evidence lists
    per = [rng.integers(0, 8, 40) if u % 7 == 0 else rng.integers(0, I, int(rng.integers(1, 41))) for u in range(U)]
    assert any(len(set(p.tolist())) < len(p) for p in per)
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
    pit = np.concatenate(per).astype(np.int32)
    pra = (rng.integers(1, 6, len(pit)) + rng.integers(0, 3, len(pit)) / 3.0).astype(np.float64)
    pti = rng.integers(0, 6, len(pit)).astype(np.int64)
    cnt = rng.integers(0, keep + 1, I).astype(np.int32)
    col = rng.integers(0, I, (I, keep)).astype(np.int32)
    cnt[8:16], col[8:16] = keep, rng.integers(0, 8, (8, keep))                         # full lists over those eight items
    sim = np.round(rng.normal(size=(I, keep)), 2)
    avg = np.round(rng.uniform(1.0, 5.0, I), 1)
    arrays = [ptr, pit, pra, pti, cnt, col, sim, avg]
    w = wtab(alpha, 66)
    eng, P = _engine(), _view(arrays, U, I)
    nb = (_to(cnt), _to(col), _to(sim))
    queries = np.arange(U, dtype=np.int32)
    for rank_by in (0, 1):
        t_cnt, t_item, t_plain, t_decay, _ = eng.topn(P, nb, _to(queries), _to(avg), _to(w), 5, rank_by, False)
        t_cnt, t_item = t_cnt.cpu().numpy(), t_item.cpu().numpy()
        lu, li = pairs_of_lists(queries, t_cnt, t_item)
        n_list = len(lu)
        assert n_list > 3 * U
        listed = int(np.nonzero(cnt)[0][0])
        pu = np.concatenate([lu, rng.integers(-1, U + 1, 50), [-1, U, 0, 0, 7]]).astype(np.int32)
        pi = np.concatenate([li, rng.integers(-1, I + 1, 50), [listed, listed, -1, 8, 9]]).astype(np.int32)
        for n_ev in (3, 16):
            want = explain_statement(pu, pi, arrays, keep, w, n_ev, rank_by)
            got = engine_explain(arrays, U, I, pu, pi, w, n_ev, rank_by, P)
            same(got[:7], want[:7], (rank_by, n_ev))
            assert got[7] == want[7]
        assert (want[1] > 16).any() and (want[0] == 1).any() and ((want[0] == 0) & (want[1] == 0)).any()
        plain, decay, status, _ = eng.predict(P, nb, _to(pu), _to(pi), _to(avg), _to(w))
        assert np.array_equal(status.cpu().numpy(), got[0])
        lists = (t_decay if rank_by else t_plain).cpu().numpy()
        scores = np.asarray([lists[q, t] for q, c in enumerate(t_cnt) for t in range(int(c))])
        assert np.array_equal(got[3][:n_list].view(np.uint64), scores.view(np.uint64))
    assert torch.cuda.is_available()


# --------------------------------------------------------------------------------------- 4. sources through the coarse ABI
SOURCE_SEED = 7         # of the seeds 1 .. 8 the only one whose two-domain input of this shape (overlap 0.4) has a replacement
                        # map at all: with the others every item is a bridge item and stage B finds no path (seed 5 among them)


def _source_input():
    """the synthetic two-domain input of test_gpu_topn.test_recommend_through_the_coarse_abi (1500 users, 300 + 300 items,
    overlap 0.4) + three hand-made users: one whose raw profile is longer than 64 entries and holds every source item a
    frequent rater might have mapped, one of 16 entries, one of 3"""
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(SOURCE_SEED, 1500, 300, 300, overlap=0.4))
    Is, I = r.n_src_items, r.n_items
    rng = np.random.default_rng(SOURCE_SEED)
    add = [np.concatenate([rng.choice(Is, 60, replace=False), Is + rng.choice(I - Is, 30, replace=False)]),
           np.concatenate([rng.choice(Is, 8, replace=False), Is + rng.choice(I - Is, 8, replace=False)]),
           np.asarray([0, Is, Is + 1])]
    add = [rng.permutation(a) for a in add]
    n = sum(len(a) for a in add)
    ptr = np.concatenate([r.user_ptr, r.user_ptr[-1] + np.cumsum([len(a) for a in add])]).astype(np.int64)
    item = np.concatenate([r.item] + add).astype(np.int32)
    rating = np.concatenate([r.rating, rng.integers(1, 6, n).astype(np.float32)])
    time = np.concatenate([r.time, synth.T0 + rng.integers(0, 5, n).astype(np.int64) * 86400])
    return synth.Ratings(ptr, item, rating, time, r.n_items, r.n_src_items, r.src_numbers, r.tgt_numbers)


def test_sources_through_the_coarse_abi():
    r = _source_input()
    I, U, alpha, keep = r.n_items, r.n_users, 1.5, 10
    flags = r.item_attrs()[3]
    d = np.diff(r.user_ptr)
    assert d.max() > 64 and (d <= 16).any()
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        m = map_of(rows["choice"])
        T = rec_sim(ctx, I, U, len(rows["user"]))
        cnt, col, sim, _ = select(ctx, I, keep)
        queries = np.arange(U, dtype=np.int32)
        lists = recommend(ctx, queries, 5, 0, 0, alpha)
        pu, pi = pairs_of_lists(queries, lists[0], lists[1])
        assert len(pu) > 2 * U and (m >= 0).sum() > 0
        arrays = [T["ptr"], T["item"], T["rating"], T["time"], cnt, col, sim, T["avg"]]
        cnt_t = np.asarray([int((flags[r.item[r.user_ptr[u]:r.user_ptr[u + 1]]] & 2 != 0).sum()) for u in range(U)], np.int32)
        n_list = len(pu)
        mu, mi = pairs_over_mapped_rows(T, cnt_t, cnt, col, keep)      # the lists + pairs that are sure to meet mapped rows
        pu, pi = np.concatenate([pu, mu]), np.concatenate([pi, mi])
        for rank_by in (0, 1):
            got, (s_total, s_pos) = ctx_explain(ctx, pu, pi, rank_by, 4, 2, alpha)
            want = explain_statement(pu, pi, arrays, keep, wtab(alpha, 66), 4, rank_by)
            same(got[:7], want[:7], rank_by)
            assert got[7] == want[7]
            scores = np.asarray([lists[2 + 0][q, t] for q, c in enumerate(lists[0]) for t in range(int(c))])
            if rank_by == 0:
                assert np.array_equal(got[3][:n_list].view(np.uint64), scores.view(np.uint64))   # the lists' own plain scores
            w_total, w_pos = sources_statement(pu, got[2], got[4], T["ptr"], T["item"], cnt_t, r.user_ptr, r.item, flags, m, 2)
            same((s_total, s_pos), (w_total, w_pos), "sources %d" % rank_by)
            # what the positions point at
            seen = dict(passed=0, mapped=0, twice=0, long=0, short=0)
            for t in range(len(pu)):
                u = int(pu[t])
                held = T["item"][T["ptr"][u]:T["ptr"][u + 1]].tolist()
                for e in range(int(got[2][t])):
                    p, n = int(got[4][t, e]), int(s_total[t, e])
                    assert n >= 1
                    src = s_pos[t, e, :min(n, 2)]
                    assert (r.user_ptr[u] <= src).all() and (src < r.user_ptr[u + 1]).all()
                    if n <= 2:                              # the left-to-right fp64 mean of the fp32 ratings is the row's rating
                        s = 0.0
                        for x in src:
                            s += float(r.rating[x])
                        assert np.float64(s / n).tobytes() == T["rating"][p:p + 1].tobytes()
                    if p - T["ptr"][u] < cnt_t[u]:          # a pass-through row's source has the row's item and time
                        assert n == 1 and r.item[src[0]] == T["item"][p] and r.time[src[0]] == T["time"][p]
                        seen["passed"] += 1
                    else:
                        assert (m[r.item[src]] == T["item"][p]).all()
                        seen["mapped"] += 1
                    seen["twice"] += held.count(T["item"][p]) > 1
                    seen["long"] += d[u] > 64
                    seen["short"] += d[u] <= 16
            print("rank_by %d: %r" % (rank_by, seen))
            assert all(v > 0 for v in seen.values()), seen
        # n_src = 0 leaves the source arrays alone and changes nothing else
        again, _ = ctx_explain(ctx, pu, pi, 1, 4, 0, alpha)
        same(again[:7], got[:7])
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------ 5. fold-in
def test_foldin_explain_equals_the_resident_explanation():
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(SOURCE_SEED, 1500, 300, 300, overlap=0.4))
    I, U, alpha = r.n_items, r.n_users, 1.5
    flags = r.item_attrs()[3]
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        m = map_of(rows["choice"])
        T = rec_sim(ctx, I, U, len(rows["user"]))
        cnt, col, _, _ = select(ctx, I, 10)
        queries = np.arange(0, U, 3, dtype=np.int32)
        lists = recommend(ctx, queries, 5, 1, 0, alpha)
        pu, pi = pairs_of_lists(queries, lists[0], lists[1])
        own_t = np.asarray([int((flags[r.item[r.user_ptr[u]:r.user_ptr[u + 1]]] & 2 != 0).sum()) for u in range(U)], np.int32)
        mu, mi = pairs_over_mapped_rows(T, own_t, cnt, col, 10)
        pu, pi = np.concatenate([pu, mu]), np.concatenate([pi, mi])
        assert ctx_explain(ctx, pu, pi, 1, 3, 2, alpha, entry="xmap_ctx_foldin_explain", rc=True) == ctx.abi.ERR_ARG   # no batch yet
        res, (r_total, r_pos) = ctx_explain(ctx, pu, pi, 1, 3, 2, alpha)
        # the upload's own profiles folded in as a batch: the same explanation, positions relative to each user's ptr
        foldin(ctx, r.user_ptr, r.item, r.rating, r.time)
        fold, (f_total, f_pos) = ctx_explain(ctx, pu, pi, 1, 3, 2, alpha, entry="xmap_ctx_foldin_explain")
        same(fold[:7], res[:7])
        same((f_total, f_pos), (r_total, r_pos))
        assert fold[7] == res[7] and (r_total > 0).any()
        # a second batch: users in reverse order, each source item three times (repeats are legal in a batch): groups of three,
        # larger than n_src = 2
        order = np.arange(U)[::-1]
        prof = []
        for u in order:
            it, ra, tm = [x[r.user_ptr[u]:r.user_ptr[u + 1]] for x in (r.item, r.rating, r.time)]
            rep = np.where(m[it] >= 0, 3, 1)
            prof.append((np.repeat(it, rep), (np.repeat(ra, rep) + np.concatenate([np.arange(k) for k in rep])).astype(np.float32),
                         np.repeat(tm, rep)))
        b_ptr = np.concatenate([[0], np.cumsum([len(p[0]) for p in prof])]).astype(np.int64)
        b_item, b_rating, b_time = [np.concatenate([p[k] for p in prof]) for k in range(3)]
        counts = foldin(ctx, b_ptr, b_item, b_rating, b_time)
        F = foldin_download(ctx, U, counts[0])
        nb = [np.zeros(I, np.int32), np.zeros((I, 10), np.int32), np.zeros((I, 10)), np.zeros((I, 10))]
        ctx.call("xmap_ctx_rec_neighbors_download", _p(nb[0], C.c_int32), _p(nb[1], C.c_int32), _p(nb[2], C.c_double), _p(nb[3], C.c_double))
        bu = (U - 1 - pu).astype(np.int32)                                              # the same users, by batch index
        got, (s_total, s_pos) = ctx_explain(ctx, bu, pi, 0, 4, 2, alpha, entry="xmap_ctx_foldin_explain")
        arrays = [F[0], F[1], F[2], F[3], nb[0], nb[1], nb[2], T["avg"]]
        same(got[:7], explain_statement(bu, pi, arrays, 10, wtab(alpha, 66), 4, 0)[:7])
        cnt_t = np.asarray([int((flags[b_item[b_ptr[u]:b_ptr[u + 1]]] & 2 != 0).sum()) for u in range(U)], np.int32)
        want = sources_statement(bu, got[2], got[4], F[0], F[1], cnt_t, b_ptr, b_item, flags, m, 2)
        same((s_total, s_pos), want)
        assert (s_total == 3).any() and (s_total == 1).any()
        # a failed fold-in leaves the batch and its explanation as they were
        bad = b_item.copy()
        bad[5] = I + 3
        code = ctx.lib.xmap_ctx_foldin(ctx.h, U, _p(b_ptr, C.c_int64), _p(bad, C.c_int32), _p(b_rating, C.c_float), _p(b_time, C.c_int64), None)
        assert code == ctx.abi.ERR_ARG
        after, (a_total, a_pos) = ctx_explain(ctx, bu, pi, 0, 4, 2, alpha, entry="xmap_ctx_foldin_explain")
        same(after[:7], got[:7])
        same((a_total, a_pos), (s_total, s_pos))
        # and the resident explanation is what it was before any fold-in
        res2, (t2, p2) = ctx_explain(ctx, pu, pi, 1, 3, 2, alpha)
        same(res2[:7], res[:7])
        same((t2, p2), (r_total, r_pos))
    finally:
        ctx.close()


# -------------------------------------------------------------------------------------------------------------- 6. union
def test_explain_on_a_union_context():
    from test_gpu_union import _trained_domains, _union
    doms = _trained_domains("multi", 2)
    numbers = np.unique(np.concatenate([r.tgt_numbers for r in doms]))
    U, I, alpha = doms[0].n_users, len(numbers), 1.5
    srcs, dst = [Ctx(), Ctx()], Ctx()
    try:
        user_maps, item_maps = [], []
        for c, r in zip(srcs, doms):
            generate(c, r)
            user_maps.append(np.arange(U, dtype=np.int32))
            im = np.full(r.n_items, -1, np.int32)
            im[r.n_src_items:] = np.searchsorted(numbers, r.tgt_numbers)
            item_maps.append(im)
        rc, counts = _union(dst, srcs, user_maps, item_maps, U, I, 1)
        assert rc == 0 and counts[0] > 0
        T = rec_sim(dst, I, U, counts[0])
        cnt, col, sim, _ = select(dst, I, 10)
        queries = np.arange(U, dtype=np.int32)
        lists = recommend(dst, queries, 5, 1, 0, alpha)
        pu, pi = pairs_of_lists(queries, lists[0], lists[1])
        assert len(pu) > U
        arrays = [T["ptr"], T["item"], T["rating"], T["time"], cnt, col, sim, T["avg"]]
        got, _ = ctx_explain(dst, pu, pi, 1, 3, 0, alpha)
        want = explain_statement(pu, pi, arrays, 10, wtab(alpha, 66), 3, 1)
        same(got[:7], want[:7])
        assert got[7] == want[7]
        assert ctx_explain(dst, pu, pi, 1, 3, 1, alpha, rc=True) == dst.abi.ERR_ARG and b"union" in dst.lib.xmap_last_error()
        again, _ = ctx_explain(dst, pu, pi, 1, 3, 0, alpha)                             # the context is unchanged
        same(again[:7], got[:7])
    finally:
        for c in srcs + [dst]:
            c.close()


# ---------------------------------------------------------------------------------------------- 7. lifecycle and arguments
def test_explain_lifecycle_and_argument_errors():
    from test_gpu_coarse_oracle import stage_c
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(3, 800, 200, 200, overlap=0.4))
    I, U, alpha = r.n_items, r.n_users, 0.2
    rng = np.random.default_rng(2)
    c = Ctx()
    try:
        ERR = c.abi.ERR_ARG
        pu, pi = rng.integers(0, U, 203).astype(np.int32), rng.integers(r.n_src_items, I, 203).astype(np.int32)
        w = wtab(alpha, 8)
        o = dict(status=np.zeros(1, np.int32), total=np.zeros(1, np.int32), cnt=np.zeros(1, np.int32), score=np.zeros(1),
                 row=np.zeros(4, np.int64), slot=np.zeros(4, np.int32), share=np.zeros(4), s_total=np.zeros(4, np.int32),
                 s_pos=np.zeros(8, np.int64))
        one = np.zeros(1, np.int32)

        def raw(n_pairs=1, user=one, item=one, rank_by=0, n_ev=4, n_src=2, tab=w, n_w=8, **drop):
            a = {k: (None if k in drop else v) for k, v in o.items()}
            return c.lib.xmap_ctx_explain(c.h, n_pairs, _p(user, C.c_int32), _p(item, C.c_int32), rank_by, n_ev, n_src, _p(tab, C.c_double),
                                          n_w, _p(a["status"], C.c_int32), _p(a["total"], C.c_int32), _p(a["cnt"], C.c_int32),
                                          _p(a["score"], C.c_double), _p(a["row"], C.c_int64), _p(a["slot"], C.c_int32),
                                          _p(a["share"], C.c_double), _p(a["s_total"], C.c_int32), _p(a["s_pos"], C.c_int64), None)
        assert raw() == ERR                                                 # before upload
        generate(c, r)
        assert raw() == ERR                                                 # before rec_sim
        c.call("xmap_ctx_rec_sim", CAP, None)
        assert raw() == ERR and b"have_nb" in c.lib.xmap_last_error()      # before the neighbour lists exist
        c.call("xmap_ctx_rec_select", 10)
        assert raw() == 0
        for kw in (dict(n_ev=0), dict(n_ev=17), dict(n_src=-1), dict(n_src=9), dict(rank_by=2), dict(rank_by=-1), dict(n_w=0),
                   dict(tab=None), dict(user=None), dict(item=None), dict(status=1), dict(total=1), dict(cnt=1), dict(score=1),
                   dict(row=1), dict(slot=1), dict(share=1), dict(s_total=1), dict(s_pos=1)):
            assert raw(**kw) == ERR, kw
            assert c.lib.xmap_last_error()
        assert raw(n_src=0, s_total=1, s_pos=1) == 0                        # no sources asked for: their arrays may be NULL
        assert raw(n_pairs=0, user=None, item=None, status=1, total=1, cnt=1, score=1, row=1, slot=1, share=1, s_total=1, s_pos=1) == 0
        ref = ctx_explain(c, pu, pi, 1, 3, 2, alpha)
        assert (ref[0][0] == 0).any()
        # host-made lists: the device's own lists handed back give the same explanation, edited ones the statement's
        cnt, col, sim, ls = [np.zeros(I, np.int32), np.zeros((I, 10), np.int32), np.zeros((I, 10)), np.zeros((I, 10))]
        c.call("xmap_ctx_rec_neighbors_download", _p(cnt, C.c_int32), _p(col, C.c_int32), _p(sim, C.c_double), _p(ls, C.c_double))
        c.call("xmap_ctx_rec_set_neighbors", 10, _p(cnt, C.c_int32), _p(col, C.c_int32), _p(sim, C.c_double))
        got = ctx_explain(c, pu, pi, 1, 3, 2, alpha)
        same(got[0][:7], ref[0][:7])
        same(got[1], ref[1])
        sim2 = np.ascontiguousarray(- sim[:, ::-1])
        col2 = np.ascontiguousarray(col[:, ::-1])
        col2[cnt < 10] = col[cnt < 10]
        sim2[cnt < 10] = sim[cnt < 10]
        c.call("xmap_ctx_rec_set_neighbors", 10, _p(cnt, C.c_int32), _p(col2, C.c_int32), _p(sim2, C.c_double))
        T = dict(ptr=np.zeros(U + 1, np.int64))
        c.call("xmap_ctx_rec_profiles_download", _p(T["ptr"], C.c_int64), None, None, None)
        n = int(T["ptr"][-1])
        pit, pra, pti, avg = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int64), np.zeros(I)
        c.call("xmap_ctx_rec_profiles_download", None, _p(pit, C.c_int32), _p(pra, C.c_double), _p(pti, C.c_int64))
        c.call("xmap_ctx_rec_download", None, None, None, None, None, _p(avg, C.c_double), None)
        got = ctx_explain(c, pu, pi, 0, 3, 0, alpha)
        want = explain_statement(pu, pi, [T["ptr"], pit, pra, pti, cnt, col2, sim2, avg], 10, wtab(alpha, 66), 3, 0)
        same(got[0][:7], want[:7])
        # a later generate drops what the explanation needs: the call fails cleanly until the tail is rebuilt
        stage_c(c, I, True, None)
        assert raw() == ERR
        c.call("xmap_ctx_rec_sim", CAP, None)
        assert raw() == ERR
        c.call("xmap_ctx_rec_select", 10)
        got = ctx_explain(c, pu, pi, 1, 3, 2, alpha)
        same(got[0][:7], ref[0][:7])
        same(got[1], ref[1])
    finally:
        c.close()


# ----------------------------------------------------------------------------------------------------- 8. the Python route
def test_session_recommend_topn_explain_on_id_strings():
    import datetime
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.engine import session, synth
    from xmap.utils.assist import baseliner_calculate_sim_pipeline, extender_pipeline, generator_pipeline
    r = synth.make_two_domain(7, 600, 150, 150, overlap=0.15)
    t0 = datetime.datetime(2013, 3, 1)
    recs = [(u, [(i, ra, t0 + datetime.timedelta(days=(t * 7919) % 6)) for i, ra, t in prof]) for u, prof in r.train_records()]
    sc = SparkContext(conf=SparkConf())
    trainRDD = sc.parallelize(recs, 8).cache()
    tool = BaselinerSim("cosine", CAP)
    sim = baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
    ae = generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True)
    iids = ae.state.idt.iids
    mp = ae.G.map.cpu().numpy()
    id_map = {iids[s]: iids[mp[s]] for s in range(len(iids)) if mp[s] >= 0}
    assert id_map
    rng = np.random.default_rng(9)
    uids = [recs[int(x)][0] for x in rng.integers(0, len(recs), 150)] + ["A%013d" % (10 ** 9 + 1)]
    raw = dict(recs)
    profile = {}
    for uid, iid, rating, when in ae.collect():          # stage-C order: a user's pass-through rows, then its mapped rows
        profile.setdefault(uid, []).append((iid, float(rating), when))
    alpha, n_ev, n_src = 1.5, 2, 4
    plain = session.recommend_topn(ae, uids, CAP, 10, alpha, 5)
    out = session.recommend_topn(ae, uids, CAP, 10, alpha, 5, explain=n_ev)
    assert out.collect() == plain.collect() and out.stats == plain.stats and not hasattr(plain, "explanations")
    sim_pairs, item_info = out.sim_pairs, out.item_info

    def statement(uid, iid):
        ev = []
        for nid, s in sim_pairs[iid]:
            for k, (it, ra, when) in enumerate(profile.get(uid, [])):
                if it == nid:
                    ev.append((s * (ra - item_info[nid][0]), abs(s), nid, s, ra, k))
        p1 = 0.0
        for e in ev:
            p1 += e[1]
        entries = []
        for q in sorted(range(len(ev)), key=lambda q: (- abs(ev[q][0] / p1), q))[:n_ev]:
            e0, _, nid, s, ra, k = ev[q]
            mine = raw[uid]
            n_pass = sum("T:" in x[0] for x in mine)
            if k < n_pass:
                src = [x for x in mine if "T:" in x[0]][k:k + 1]
            else:
                src = [x for x in mine if id_map.get(x[0]) == nid]
            entries.append((nid, s, ra, e0 / p1, [tuple(x) for x in src[:n_src]], len(src)))
        return entries

    want = [(uid, [(c[0], statement(uid, c[0])) for c in lst]) for uid, lst in out.collect()]
    assert out.explanations == want
    flat = [e for _, l in want for _, es in l for e in es]
    assert flat and any("T:" in s[0] for e in flat for s in e[4])
    # session.explain over the same pairs + pairs whose evidence holds a mapped row: the same entries, the scores of the lists
    listed = [(uid, c[0]) for uid, lst in out.collect() for c in lst][:300]
    lists_with = {}
    for iid, lst in sim_pairs.items():
        for nid, _ in lst:
            lists_with.setdefault(nid, []).append(iid)
    over_mapped = [(uid, iid) for uid in sorted(set(uids[:-1])) for x in raw[uid] if x[0] in id_map
                   for iid in lists_with.get(id_map[x[0]], [])[:2]][:150]
    assert over_mapped
    pairs = listed + over_mapped + [(uids[-1], iids[-1]), (uids[0], "no such item")]
    ex = session.explain(ae, pairs, CAP, 10, alpha, n_ev=n_ev, n_src=n_src).collect()
    scores = {(uid, c[0]): c[1] for uid, lst in out.collect() for c in lst}
    for (uid, iid), got in zip(listed, ex):
        assert got == (uid, iid, scores[uid, iid], statement(uid, iid))
    for (uid, iid), got in zip(over_mapped, ex[len(listed):]):
        assert got[:2] == (uid, iid) and got[3] == statement(uid, iid)
    cited = [s for got in ex for e in got[3] for s in e[4]]
    assert any("S:" in s[0] for s in cited) and any("T:" in s[0] for s in cited)
    assert ex[-1] == (uids[0], "no such item", None, []) and ex[-2][0] == uids[-1] and ex[-2][3] == []
