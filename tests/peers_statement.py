"""The statement of the peers calls (include/xmap_hip.h, "peers"; csrc/stage_e_peers.hip) in plain Python: the index
(peer_index_statement) and the rows (peer_rows_statement) exactly as the header words them, with their own dd_add / dd_sum, and
the builders of the designed inputs the GPU test runs (tests/test_gpu_peers.py), whose census tests/test_cpu_peers_statement.py
takes on the CPU.  Every layer must reproduce these bit for bit."""
import math

import numpy as np

NAN = float("nan")
SAME, KEEP_SELF, CENTRED = 1, 2, 4


def dd_add(hi, lo, x):
    """common.h: Knuth two-sum + renormalisation, one fp64 operation per line"""
    s = hi + x
    bb = s - hi
    e = (hi - (s - bb)) + (x - bb)
    e += lo
    h2 = s + e
    return h2, e - (h2 - s)


def dd_sum(values):
    hi = lo = 0.0
    for x in values:
        hi, lo = dd_add(hi, lo, x)
    return hi


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN            # (a NaN or a negative argument: NaN, as on the device)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def weighted(cs, n, cap):
    return _div(_mul(_mul(1.0, cs), float(min(n, cap))), float(cap))


class Profiles(object):
    """user-major profiles: ptr int64 [U + 1], item int32, rating fp64"""

    def __init__(self, ptr, item, rating, n_items):
        self.ptr = np.ascontiguousarray(ptr, np.int64)
        self.item = np.ascontiguousarray(item, np.int32)
        self.rating = np.ascontiguousarray(rating, np.float64)
        self.n_users, self.n_items = len(self.ptr) - 1, int(n_items)

    @staticmethod
    def from_lists(rows, n_items):
        """rows: per user a list of (item, rating)"""
        ptr = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=ptr[1:])
        flat = [e for r in rows for e in r]
        return Profiles(ptr, [e[0] for e in flat], [e[1] for e in flat], n_items)


def _x(P, centre):
    """x of every row (0.0 for an invalid row, never read)"""
    item, r = P.item.astype(np.int64), P.rating
    valid = (item >= 0) & (item < P.n_items)
    x = r.copy()
    if centre is not None:
        with np.errstate(all="ignore"):
            x[valid] = r[valid] - np.asarray(centre, np.float64)[item[valid]]
    x[~valid] = 0.0
    return x, valid


def _norms(P, x, valid):
    out = np.zeros(P.n_users)
    ptr, item = P.ptr.tolist(), P.item.tolist()
    xs, ok = x.tolist(), valid.tolist()
    for u in range(P.n_users):
        rows = [p for p in range(ptr[u], ptr[u + 1]) if ok[p]]
        by_item = {}
        for p in rows:
            by_item.setdefault(item[p], []).append(p)
        out[u] = _sqrt(dd_sum([_mul(xs[p], xs[r]) for p in rows for r in by_item[item[p]]]))
    return out


def peer_index_statement(P, centre=None):
    """-> dict(hd_ptr [I + 1], hd_user, hd_x [rows indexed], nrm [U], rows)"""
    x, valid = _x(P, centre)
    user_of = np.repeat(np.arange(P.n_users), np.diff(P.ptr))
    rows = np.nonzero(valid)[0]
    order = rows[np.argsort(P.item[rows], kind="stable")]          # holder order: item, then ascending row index
    hd_ptr = np.zeros(P.n_items + 1, np.int64)
    np.cumsum(np.bincount(P.item[rows], minlength=P.n_items), out=hd_ptr[1:])
    return dict(hd_ptr=hd_ptr, hd_user=user_of[order].astype(np.int32), hd_x=x[order], nrm=_norms(P, x, valid), rows=int(len(rows)))


def peer_rows_statement(P, Q, query_user, n_top, cap=1, min_common=1, flags=0, centre=None, allow=None, exclude=None, min_score=None,
                        index=None, full=False):
    """P: the resident profiles, Q: the profiles the queries index (P itself with SAME).  allow: bool [U] or None; exclude: one
    list of ids per query or None; min_score: the floor or None.  -> (cnt [Q], user [Q][n_top], sim, common, stats [6]); full:
    also the kept candidates of every query in rank order, [(user, sim, common)]"""
    X = index or peer_index_statement(P, centre)
    hd_ptr, hd_user, hd_x, nrm = X["hd_ptr"].tolist(), X["hd_user"].tolist(), X["hd_x"].tolist(), X["nrm"].tolist()
    qx, qvalid = _x(Q, centre)
    qn = _norms(Q, qx, qvalid).tolist()
    qx, qvalid, qptr, qitem = qx.tolist(), qvalid.tolist(), Q.ptr.tolist(), Q.item.tolist()
    allow = None if allow is None else np.asarray(allow, bool).tolist()
    n_q = len(query_user)
    cnt = np.zeros(n_q, np.int32)
    user = np.full((n_q, n_top), -1, np.int32)
    sim = np.zeros((n_q, n_top))
    common = np.zeros((n_q, n_top), np.int32)
    stats = [0] * 6
    kept_all = []
    for q, a in enumerate(int(u) for u in query_user):
        records = {}                                                # v -> [t*] in record order
        if 0 <= a < Q.n_users:
            for p in range(qptr[a], qptr[a + 1]):
                if not qvalid[p]:
                    continue
                for h in range(hd_ptr[qitem[p]], hd_ptr[qitem[p] + 1]):
                    v = hd_user[h]
                    if allow is not None and not allow[v]:
                        continue                                    # the mask acts in the expansion
                    records.setdefault(v, []).append(_mul(qx[p], hd_x[h]))
                    stats[5] += 1
        ex = set() if exclude is None or exclude[q] is None else set(int(i) for i in exclude[q])
        kept, cands = [], 0
        for v in sorted(records):
            if (flags & SAME) and not (flags & KEEP_SELF) and v == a:
                continue
            if v in ex:
                continue
            cands += 1
            n = len(records[v])
            if n < min_common:
                stats[1] += 1
                continue
            dot = dd_sum(records[v])
            np_ = _mul(qn[a], nrm[v])
            s = weighted(_div(dot, np_) if np_ != 0.0 else 0.0, n, cap)
            if not math.isfinite(s):
                stats[2] += 1
                continue
            if min_score is not None and s < min_score:
                stats[3] += 1
                continue
            kept.append((v, s, n))
        stats[0] += cands
        stats[4] = max(stats[4], cands)
        kept.sort(key=lambda e: (-(e[1] + 0.0), e[0]))              # as numbers: -0.0 == 0.0; then the user index
        kept_all.append(kept)
        k = min(len(kept), n_top)
        cnt[q] = k
        for j in range(k):
            user[q, j], sim[q, j], common[q, j] = kept[j]
    out = (cnt, user, sim, common, stats)
    return out + (kept_all,) if full else out


# ---------------------------------------------------------------------------------------------------- designed inputs
FAMILIES = ("integers", "halves", "means", "magnitudes")


def random_profiles(seed, family, U=300, I=40, max_rows=12, dup=0.10, invalid=0.03):
    """up to max_rows rows per profile (some users have none), `dup` of the rows repeat an item of the same profile, `invalid` of
    the rows carry an item outside [0, I) (-1 or I)"""
    rng = np.random.RandomState(seed)
    rows = []
    for u in range(U):
        n = 0 if rng.rand() < 0.05 else int(rng.randint(1, max_rows + 1))
        r = []
        for _ in range(n):
            if r and rng.rand() < dup:
                it = r[int(rng.randint(len(r)))][0]
            elif rng.rand() < invalid:
                it = -1 if rng.rand() < 0.5 else I
            else:
                it = int(rng.randint(I))
            if family == "integers":
                val = float(rng.randint(1, 6))
            elif family == "halves":
                val = float(rng.randint(1, 11)) / 2.0
            elif family == "means":
                val = float(np.mean(rng.randint(1, 6, size=int(rng.randint(1, 8))).astype(np.float64)))
            else:
                val = float(rng.choice([-1.0, 1.0]) * (1.0 + rng.rand()) * 10.0 ** int(rng.choice([-150, -75, 0, 75, 150])))
            r.append((it, val))
        rows.append(r)
    if family == "magnitudes":                                      # and one NaN rating: non-finite sims, dropped and counted
        u = max(range(U), key=lambda k: len(rows[k]))
        rows[u][0] = (rows[u][0][0] if 0 <= rows[u][0][0] < I else 0, NAN)
    return Profiles.from_lists(rows, I)


def family_queries(U):
    """the queries of the random families: every third user, then a negative index, two beyond the users, and two repeats"""
    q = np.arange(0, U, 3).tolist()
    return np.asarray(q + [-1, U, U + 5, q[0], q[7]], np.int32)


def item_means_exact(P):
    """the statement of xmap_peer_centre, as item_stats.h sums an item: lane l of 64 adds the entries l, l + 64, ... of the item's
    holder row (holder order) into a double-double, the fixed butterfly of dd_reduce folds the lanes (lane l takes lane l + m, m =
    32 .. 1; a lane without a partner takes itself), lane 0's high word / entries; 0.0 without entries.  Exact to 2^-104 of the
    largest partial sum, rounded once: the exact average wherever the ratings span fewer than 100 bits"""
    by = [[] for _ in range(P.n_items)]
    for it, r in zip(P.item.tolist(), P.rating.tolist()):
        if 0 <= it < P.n_items:
            by[it].append(r)
    out = []
    for v in by:
        lanes = []
        for l in range(64):
            hi = lo = 0.0
            for x in v[l::64]:
                hi, lo = dd_add(hi, lo, x)
            lanes.append((hi, lo))
        m = 32
        while m >= 1:
            nxt = []
            for l in range(64):
                oh, ol = lanes[l + m] if l + m < 64 else lanes[l]
                hi, lo = dd_add(lanes[l][0], lanes[l][1], oh)
                nxt.append(dd_add(hi, lo, ol))
            lanes, m = nxt, m // 2
        out.append(_div(1.0 * lanes[0][0], float(len(v))) if v else 0.0)
    return np.asarray(out, np.float64)


def item_means(P):
    """the centre of the `means` family: fp64 means per item, so that centred sums cancel"""
    item = P.item.astype(np.int64)
    ok = (item >= 0) & (item < P.n_items)
    s = np.bincount(item[ok], weights=P.rating[ok], minlength=P.n_items)
    n = np.bincount(item[ok], minlength=P.n_items)
    with np.errstate(all="ignore"):
        return np.where(n > 0, s / np.maximum(n, 1), 0.0)


def popular_profiles(n_holders, U=3000, seed=5):
    """item 0 held by the first n_holders of U users, twice by 50 of them; every user also holds an item of its own (it enters the
    norm only), so the candidates of a holder are exactly the holders"""
    rng = np.random.RandomState(seed)
    rows = []
    for u in range(U):
        r = [(0, float(rng.randint(1, 6)))] if u < n_holders else []
        r.append((1 + u, float(rng.randint(1, 6))))
        if u < n_holders and u % 5 == 1 and u < 250:
            r.append((0, float(rng.randint(1, 6))))
        rows.append(r)
    return Profiles.from_lists(rows, U + 1)


POPULAR_SIZES = (255, 256, 257, 1023, 1024, 1025, 2 * 1024 + 1)      # around the tile, n_top = 1024 and 2 * (selection capacity) + 1


def tie_profiles(n_same=400, n_other=60, I=12, seed=9):
    """n_same users with one identical profile, interleaved with n_other users with profiles of their own: the identical ones tie
    bit for bit with any query, and must come out by index"""
    rng = np.random.RandomState(seed)
    same = [(1, 4.0), (3, 2.0), (5, 5.0), (3, 1.0)]
    U = n_same + n_other
    other = set(rng.choice(U, n_other, replace=False).tolist())
    rows = []
    for u in range(U):
        if u in other:
            rows.append([(int(rng.randint(I)), float(rng.randint(1, 6))) for _ in range(int(rng.randint(1, 7)))])
        else:
            rows.append(list(same))
    return Profiles.from_lists(rows, I), sorted(other)


def sparse_wide_profiles(U=(1 << 17) + 3, n_active=900, I=30, seed=11):
    """rows on a sparse subset of U users, the last user among them: user indices need 18 bits"""
    rng = np.random.RandomState(seed)
    active = np.unique(np.concatenate([rng.choice(U, n_active, replace=False), [0, U - 1, 1 << 17]]))
    counts = np.zeros(U, np.int64)
    counts[active] = rng.randint(1, 7, size=len(active))
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(counts, out=ptr[1:])
    n = int(ptr[-1])
    return Profiles(ptr, rng.randint(0, I, size=n), rng.randint(1, 11, size=n) / 2.0, I), active


def census(kept_all, n_top, P=None, Q=None, query_user=None):
    """what a designed case exercises: (queries with more kept candidates than n_top, queries with two or more equal sims across
    the cut, the longest run)"""
    more = sum(1 for k in kept_all if len(k) > n_top)
    ties = sum(1 for k in kept_all if len(k) > n_top and k[n_top - 1][1] == k[n_top][1])
    longest = max([e[2] for k in kept_all for e in k] or [0])
    return more, ties, longest
