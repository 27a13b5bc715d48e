"""The statement of the user-kNN calls (include/xmap_hip.h, "user-kNN"; csrc/stage_e_uknn.hip) in plain Python: the means
(means_statement), the predictions (predict_statement) and the top-N lists (topn_statement) exactly as the header words them, with
their own dd_add, and the builders of the designed inputs the GPU test runs (tests/test_gpu_uknn.py), whose census
tests/test_cpu_uknn_statement.py takes on the CPU.  Every layer must reproduce these bit for bit."""
import math

import numpy as np

OWN_MEAN, KEEP_HELD = 1, 2


def dd_add(hi, lo, x):
    """common.h: Knuth two-sum + renormalisation, one fp64 operation per line"""
    s = hi + x
    bb = s - hi
    e = (hi - (s - bb)) + (x - bb)
    e += lo
    h2 = s + e
    return h2, e - (h2 - s)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def bound_rating(r):
    """round half up, clamp to [0, 5]: max(0, min(int(r + 0.5), 5)) of a finite r"""
    x = r + 0.5
    return 5.0 if x >= 5.0 else (0.0 if x < 1.0 else float(int(x)))


def means_statement(P):
    """-> (avg [U], cnt [U]): per user the double-double sum of its valid rows, summed as the device sums it -- lane l of 64 adds
    the rows l, l + 64, .. of the profile, the fixed butterfly folds the lanes (lane l takes lane l + m, m = 32 .. 1; a lane without
    a partner takes itself) -- rounded once, divided by the count; 0.0 and 0 without valid rows"""
    ptr, item, rating = P.ptr.tolist(), P.item.tolist(), P.rating.tolist()
    avg, cnt = np.zeros(P.n_users), np.zeros(P.n_users, np.int32)
    for u in range(P.n_users):
        rows = list(range(ptr[u], ptr[u + 1]))
        lanes, n = [], 0
        for l in range(64):
            hi = lo = 0.0
            for p in rows[l::64]:
                if 0 <= item[p] < P.n_items:
                    hi, lo = dd_add(hi, lo, rating[p])
                    n += 1
            lanes.append((hi, lo))
        m = 32
        while m >= 1:
            nxt = []
            for l in range(64):
                oh, ol = lanes[l + m] if l + m < 64 else lanes[l]
                hi, lo = dd_add(lanes[l][0], lanes[l][1], oh)
                nxt.append(dd_add(hi, lo, ol))
            lanes, m = nxt, m // 2
        avg[u] = _div(1.0 * lanes[0][0], float(n)) if n else 0.0
        cnt[u] = n
    return avg, cnt


def _score(avg_a, entries):
    """entries [(s, d)*] in order -> (score, ok): plain fp64 sums from 0.0 left to right; ok False where the Python statement of
    the reference raises (a zero weight sum, a value that is not finite)"""
    if not entries:
        return avg_a, math.isfinite(avg_a)
    num, den = _sums(entries)
    score = avg_a + _div(num, den)
    return score, den != 0.0 and math.isfinite(score)


def _rows_of(P):
    ptr, item, rating = P.ptr.tolist(), P.item.tolist(), P.rating.tolist()
    return [[(item[p], rating[p]) for p in range(ptr[u], ptr[u + 1])] for u in range(P.n_users)]


def _list_of(lists, q):
    cnt, user, sim = lists
    n_nb = user.shape[1]
    k = min(int(cnt[q]), n_nb)
    return list(zip(user[q, :max(k, 0)].tolist(), sim[q, :max(k, 0)].tolist()))


def predict_statement(P, lists, query_avg, user_avg, test_q, test_item, flags=0):
    """P: the resident profiles; lists = (cnt [n_query], user [n_query][n_nb], sim) as the peers write them; query_avg [n_query];
    user_avg [U].  -> (score, bound, n, status) per test pair"""
    rows = _rows_of(P)
    n_query = len(lists[0])
    T = len(test_q)
    score, bound = np.zeros(T), np.zeros(T)
    n, status = np.zeros(T, np.int32), np.zeros(T, np.int32)
    for t, (q, it) in enumerate(zip((int(x) for x in test_q), (int(x) for x in test_item))):
        if not (0 <= q < n_query and 0 <= it < P.n_items):
            status[t] = 3
            continue
        if lists[0][q] <= 0:
            status[t] = 1
            continue
        a = float(query_avg[q])
        entries = []
        for v, s in _list_of(lists, q):
            if 0 <= v < P.n_users:
                m = float(user_avg[v]) if flags & OWN_MEAN else a
                entries += [(s, r - m) for i, r in rows[v] if i == it]
        sc, ok = _score(a, entries)
        n[t] = len(entries)
        if ok:
            score[t], bound[t] = sc, bound_rating(sc)
        else:
            status[t] = 2
    return score, bound, n, status


def mae_statement(status, real, bound):
    """xmap_mae over the pairs with status 0 -> (count, sum |real - bound|), the exact sum rounded once"""
    hi = lo = 0.0
    for s, r, b in zip(status.tolist(), np.asarray(real, np.float64).tolist(), bound.tolist()):
        if s == 0:
            hi, lo = dd_add(hi, lo, abs(r - b))
    return float(int((status == 0).sum())), hi


def topn_statement(P, Q, query_user, lists, query_avg, user_avg, n_top, min_support=1, flags=0, allow=None, exclude=None,
                   min_score=None, full=False):
    """P: the resident profiles; Q: the profiles query_user indexes (the held items); lists / query_avg per query; allow: bool [I]
    or None; exclude: one list of items per query or None; min_score: the floor or None.  -> (cnt [n_query], item [n_query][n_top],
    score, support, stats [6]); full: also the kept candidates of every query in rank order, [(item, score, support)]"""
    rows = _rows_of(P)
    qrows = _rows_of(Q)
    allow = None if allow is None else np.asarray(allow, bool).tolist()
    n_q = len(query_user)
    cnt = np.zeros(n_q, np.int32)
    item = np.full((n_q, n_top), -1, np.int32)
    score = np.zeros((n_q, n_top))
    support = np.zeros((n_q, n_top), np.int32)
    stats = [0] * 6
    kept_all = []
    for q, a_user in enumerate(int(u) for u in query_user):
        a = float(query_avg[q])
        records = {}                                                # item -> [(s, d)*] in record order
        for v, s in (_list_of(lists, q) if lists[0][q] > 0 else []):
            if not 0 <= v < P.n_users:
                continue
            m = float(user_avg[v]) if flags & OWN_MEAN else a
            for i, r in rows[v]:
                if not 0 <= i < P.n_items or (allow is not None and not allow[i]):
                    continue                                        # the mask acts in the expansion
                records.setdefault(i, []).append((s, r - m))
                stats[5] += 1
        held = set(i for i, _ in qrows[a_user]) if 0 <= a_user < Q.n_users and not flags & KEEP_HELD else set()
        ex = set() if exclude is None or exclude[q] is None else set(int(i) for i in exclude[q])
        kept, cands = [], 0
        for i in sorted(records):
            if i in held or i in ex:
                continue
            cands += 1
            if len(records[i]) < min_support:
                stats[1] += 1
                continue
            sc = a + _div(*_sums(records[i]))
            if not math.isfinite(sc):
                stats[2] += 1
                continue
            if min_score is not None and sc < min_score:
                stats[3] += 1
                continue
            kept.append((i, sc, len(records[i])))
        stats[0] += cands
        stats[4] = max(stats[4], cands)
        kept.sort(key=lambda e: (-(e[1] + 0.0), e[0]))              # as numbers: -0.0 == 0.0; then the item index
        kept_all.append(kept)
        k = min(len(kept), n_top)
        cnt[q] = k
        for j in range(k):
            item[q, j], score[q, j], support[q, j] = kept[j]
    out = (cnt, item, score, support, stats)
    return out + (kept_all,) if full else out


def _sums(entries):
    num = den = 0.0
    for s, d in entries:
        num += s * d
        den += abs(s)
    return num, den


def cut(full, n_top):
    """the statement's outputs at a smaller n_top from its kept lists (the stats do not depend on n_top)"""
    kept, stats = full[5], full[4]
    n_q = len(kept)
    cnt, item = np.zeros(n_q, np.int32), np.full((n_q, n_top), -1, np.int32)
    score, support = np.zeros((n_q, n_top)), np.zeros((n_q, n_top), np.int32)
    for q, k in enumerate(kept):
        cnt[q] = min(len(k), n_top)
        for j in range(cnt[q]):
            item[q, j], score[q, j], support[q, j] = k[j]
    return cnt, item, score, support, stats


def census(kept_all, n_top):
    """what a designed case exercises: (queries with more kept candidates than n_top, queries with equal scores across the cut,
    the longest run = largest support of a kept candidate)"""
    more = sum(1 for k in kept_all if len(k) > n_top)
    ties = sum(1 for k in kept_all if len(k) > n_top and k[n_top - 1][1] == k[n_top][1])
    longest = max([e[2] for k in kept_all for e in k] or [0])
    return more, ties, longest


# ---------------------------------------------------------------------------------------------------- designed inputs
def _profiles(rows, n_items):
    from peers_statement import Profiles
    return Profiles.from_lists(rows, n_items)


def crowd_profiles(n_crowd=280, seed=21):
    """user 0 and a crowd of n_crowd users all hold item 0 (so the crowd are user 0's peers); every member of the crowd also holds
    item 1, every fifth of them twice, and user 0 does not: item 1 is a candidate of user 0 whose run has more than n_crowd
    records.  Items 2 .. 9 are spread thinly; the last 20 users share nothing with user 0.  Ratings are halves."""
    rng = np.random.RandomState(seed)
    half = lambda: float(rng.randint(1, 11)) / 2.0
    rows = [[(0, 4.0), (2, 2.5)]]
    for u in range(1, n_crowd + 1):
        r = [(0, half()), (1, half())]
        if u % 5 == 0:
            r.append((1, half()))
        if u % 7 == 0:
            r.append((2 + u % 8, half()))
        rows.append(r)
    for u in range(20):
        rows.append([(10 + u % 3, half())])
    return _profiles(rows, 13)


def tie_item_profiles(n_items=600, n_nb=6):
    """user 0 holds items 0 .. 3; n_nb neighbours hold them too and, each with ONE rating of its own, every item 4 .. n_items - 1 in
    a different order: the evidence of all those items is the same entries in the same (list) order, so their scores are bit-equal
    and they must come out by item index.  Item 4 carries one more record (user n_nb + 1 holds it twice): it alone differs."""
    rows = [[(0, 5.0), (1, 3.0), (2, 4.0), (3, 1.0)]]
    for k in range(n_nb):
        mine = [5.0, 3.0, 4.0, 1.5 + 0.5 * k]
        own = 2.0 + 0.5 * k
        order = list(range(4, n_items))
        order = order[k::2] + order[:k][::-1] + order[k:][1::2]
        assert sorted(order) == list(range(4, n_items))
        rows.append([(i, mine[i]) for i in range(4)] + [(i, own) for i in order])
    rows.append([(0, 5.0), (1, 3.0), (2, 4.0), (3, 1.0), (4, 5.0), (4, 4.5)])
    return _profiles(rows, n_items)


def wide_item_profiles(I=(1 << 17) + 3, U=200, n_active=300, seed=13):
    """items on a sparse subset of I item indices, the last one among them: item indices need 18 bits of the key"""
    rng = np.random.RandomState(seed)
    active = np.unique(np.concatenate([rng.choice(I, n_active, replace=False), [0, I - 1, 1 << 17]]))
    common = active[:6]
    rows = []
    for u in range(U):
        r = [(int(i), float(rng.randint(1, 11)) / 2.0) for i in rng.choice(common, int(rng.randint(1, 4)), replace=False)]
        r += [(int(i), float(rng.randint(1, 11)) / 2.0) for i in rng.choice(active, int(rng.randint(1, 8)))]
        if u % 9 == 0:
            r.append((I - 1, float(rng.randint(1, 11)) / 2.0))
        rows.append(r)
    return _profiles(rows, I), active


def crafted_lists(lists, U, nan_user=None):
    """a copy of peer lists with the cases no peer call writes: query 1 has count 0 with entries behind it; the sims of query 2 and
    of the first later query with a list are all 0.0 (every pair with evidence raises: status 2); query 3 lists a user outside
    [0, U) and one user twice; query 4's count is larger than n_nb; nan_user (the user with the NaN rating) heads the list of
    the second later query with a list"""
    cnt, user, sim = [np.array(a, copy=True) for a in lists]
    n_nb = user.shape[1]
    cnt[1] = 0
    later = [q for q in range(5, len(cnt)) if cnt[q] > 0]
    sim[2, :] = 0.0
    sim[later[0], :] = 0.0
    if n_nb >= 3 and cnt[3] >= 3:
        user[3, 0], user[3, 2] = U + 4, user[3, 1]
    if cnt[4] == n_nb:
        cnt[4] = n_nb + 9
    if nan_user is not None:
        user[later[1], 0] = nan_user
    return cnt, user, sim


def pair_cases(P, n_query, seed=3, n=400, extra=()):
    """the pairs `extra`, random (q, item) pairs over the lists, then the pairs out of range: status 3"""
    rng = np.random.RandomState(seed)
    q = [e[0] for e in extra] + rng.randint(0, n_query, size=n).tolist() + [-1, n_query, 0, 0]
    it = [e[1] for e in extra] + rng.randint(0, P.n_items, size=n).tolist() + [0, 0, -1, P.n_items]
    return np.asarray(q, np.int32), np.asarray(it, np.int32)


def lists_from_peers(P, Q, query, n_nbs, same=True, cap=5, centre=None):
    """{n_nb: (cnt, user, sim)} for the queries: the lists of the peers statement (tests/peers_statement.py) at the widest n_nb,
    cut to the narrower ones -- a list of n is the prefix of a list of m > n"""
    import peers_statement as ps
    full = ps.peer_rows_statement(P, Q, query, max(n_nbs), cap=cap, flags=ps.SAME if same else 0, centre=centre, full=True)
    out = {}
    for n_nb in n_nbs:
        cnt = np.zeros(len(query), np.int32)
        user, sim = np.full((len(query), n_nb), -1, np.int32), np.zeros((len(query), n_nb))
        for q, kept in enumerate(full[5]):
            cnt[q] = min(len(kept), n_nb)
            for j in range(cnt[q]):
                user[q, j], sim[q, j] = kept[j][0], kept[j][1]
        out[n_nb] = (cnt, user, sim)
    return out


def gather_means(avg, query):
    """query_avg of queries that index the users of avg: 0.0 for an index outside them"""
    return np.asarray([avg[u] if 0 <= u < len(avg) else 0.0 for u in (int(x) for x in query)], np.float64)


N_NBS = (1, 63, 64, 65, 200)


def family_case(family):
    """one random family of tests/peers_statement.py (U = 300, I = 40; repeated and invalid rows, and in `magnitudes` the NaN
    rating) with the lists of the peers statement at every n_nb of N_NBS, crafted (crafted_lists) -> dict"""
    import peers_statement as ps
    P = ps.random_profiles(3, family)
    query = ps.family_queries(P.n_users)
    avg, cnt = means_statement(P)
    nan = np.nonzero(np.isnan(avg))[0]
    lists = {k: crafted_lists(v, P.n_users, int(nan[0]) if len(nan) else None)
             for k, v in lists_from_peers(P, P, query, N_NBS, centre=ps.item_means(P)).items()}
    extra = []                                      # the pair whose evidence is the NaN rating itself
    if len(nan):
        planted = [q for q in range(5, len(query)) if lists[200][0][q] > 0][1]
        extra = [(planted, int(P.item[P.ptr[nan[0]]]))]
    return dict(P=P, query=query, avg=avg, cnt=cnt, lists=lists, qavg=gather_means(avg, query), extra=extra)


def golden_case(path):
    """tests/golden/uknn_small.json.gz (profiles/tools/record_uknn_golden.py: the reference's own user_based_prediction on a small
    designed input) -> dict(P, lists, qavg, avg, tq, ti, want): want[t] = the reference's bounded prediction of pair t, None where it
    skipped the user (no list), "raise" where the user's line raised ZeroDivisionError"""
    import gzip
    import json
    d = json.loads(gzip.open(path).read().decode())
    P = _profiles([[(i, r) for i, r in rows] for rows in d["profiles"]], d["n_items"])
    iidx = {x: k for k, x in enumerate(d["iid"])}
    lists = (np.asarray(d["nb_cnt"], np.int32), np.asarray(d["nb_user"], np.int32), np.asarray(d["nb_sim"], np.float64))
    avg = np.asarray(d["user_avg"], np.float64)
    tq, ti, want = [], [], []
    for q, ((uid, pairs), (uid2, got)) in enumerate(zip(d["test"], d["predicted"])):
        assert uid == uid2 == d["uid"][d["query"][q]]
        for k, pair in enumerate(pairs):
            tq.append(q)
            ti.append(iidx[pair[0]])
            if got == "ZeroDivisionError":
                want.append("raise")
            elif got == [[]]:
                want.append(None)
            else:
                assert got[k][0] == pair[0] and got[k][1] == pair[1]
                want.append(float(got[k][2]))
    return dict(P=P, lists=lists, qavg=gather_means(avg, d["query"]), avg=avg, tq=np.asarray(tq, np.int32), ti=np.asarray(ti, np.int32),
                want=want)


def held_to_golden(want, bound, status, tq):
    """the outputs of a prediction call against the reference's record: equal bounded predictions where it predicted, status 1
    where it skipped the user, and at least one status 2 among the pairs of a user whose line raised"""
    raised = {}
    for t, w in enumerate(want):
        if w is None:
            assert status[t] == 1, t
        elif w == "raise":
            raised.setdefault(int(tq[t]), []).append(int(status[t]))
        else:
            assert status[t] == 0 and bound[t] == w, (t, w, bound[t], status[t])
    assert raised and all(2 in s and set(s) <= {0, 2} for s in raised.values()), raised
    return True
