"""The brute-force statement of the label quotas and calibrated lists (xmap_quota_pool / xmap_quota_rows, include/xmap_hip.h): ONE
list per query with a guaranteed mix of labels, cut from a pool of ranked positions.  Python integers / NumPy only, no device.

  cap_lists, share_lists : the two loops of the header, transcribed literally over L = [governed labels of position j]
  history_weights        : w[l] = rows of a profile whose item carries governed label l
  pool_of                : the kept candidates of a query ranked into a pool
  expected_pool          : over pools in the top-N layout (in_cnt, in_item, in_plain, in_decay)
  expected_quota         : over test_gpu_topn.score_users' {user: [(item, plain, decayed, now, held)*]}: the kept candidates are what
                           filter_statement.expected_filtered keeps with no cut (its rule order, its stats)
  designed()             : the designed families of the device tests, census() what they are meant to hold

A list is [(pos, item, plain, decayed, label)*]; to_arrays() lays lists out as the six output arrays."""
import numpy as np

from filter_statement import allowed, expected_filtered
from shelf_statement import Labels, check_tables

CAP, SHARE = 0, 1
MODE = {"cap": CAP, "share": SHARE}
MAX_POOL, MAX_RECORDS = 1024, 8192
INT32_MAX = 2 ** 31 - 1


def cap_lists(L, n_top, cap):
    """L[j] = the governed labels of position j, cap(l) -> (positions, refused, refused although another label of the position had
    room)"""
    taken, out, refused, partly = {}, [], 0, 0
    for j in range(len(L)):
        if not len(out) < n_top:
            break
        if all(taken.get(l, 0) < cap(l) for l in L[j]):
            out.append(j)
            for l in L[j]:
                taken[l] = taken.get(l, 0) + 1
        else:
            refused += 1
            partly += any(taken.get(l, 0) < cap(l) for l in L[j])
    return out, refused, partly


def share_lists(L, n_top, w, bits=64):
    """w: {label: weight} -> (positions, claims, fills, quotient ties decided by label id).  bits: the width of the products (64 as
    the contract has it; 32 shows what a narrower product would pick)"""
    mask = (1 << bits) - 1
    s, left, out, claims, fills, ties = {}, set(range(len(L))), [], [], 0, 0
    for r in range(min(len(L), n_top)):
        E = sorted({l for j in left for l in L[j] if w.get(l, 0) > 0})
        if not E:
            j, claim = min(left), -1
            fills += 1
        else:
            best = E[0]
            for l in E[1:]:             # ascending ids: a later label wins only when strictly larger
                if ((w[l] * (2 * s.get(best, 0) + 1)) & mask) > ((w[best] * (2 * s.get(l, 0) + 1)) & mask):
                    best = l
            ties += any(l != best and w[l] * (2 * s.get(best, 0) + 1) == w[best] * (2 * s.get(l, 0) + 1) for l in E)
            j, claim = min(j for j in left if best in L[j]), best
        out.append(j)
        claims.append(claim)
        left.remove(j)
        for l in L[j]:
            s[l] = s.get(l, 0) + 1
    return out, claims, fills, ties


def governed(labels, item, lab_ok):
    return [l for l in labels.carried(int(item)) if lab_ok[l]]


def history_weights(labels, lab_ok, prof_items):
    """{label: rows of the profile whose item carries it}: a row held twice counts twice, an item outside the table nothing"""
    w = {}
    for it in prof_items:
        for l in governed(labels, it, lab_ok):
            w[l] = w.get(l, 0) + 1
    return w


def pool_of(kept, rank_by, n_pool):
    """kept [(item, plain, decayed)*] -> the pool: rank_by score descending as numbers (-0.0 equals 0.0), item ascending"""
    return sorted(kept, key=lambda c: (- c[1 + rank_by], c[0]))[:n_pool]


def longest_row(labels):
    return int(np.diff(labels.ptr).max()) if labels.n_items else 0


def quota_of(pool, full, labels, lab_ok, n_top, mode, cap=1, lab_cap=None, w=None, tally=None):
    """one query: pool [(item, plain, decayed)*] of m positions, full = the pool was full -> (list, stats [4])"""
    L = [governed(labels, c[0], lab_ok) for c in pool]
    if mode == CAP:
        pos, third, partly = cap_lists(L, n_top, (lambda l: int(lab_cap[l])) if lab_cap is not None else (lambda l: cap))
        claims = [min(L[j]) if L[j] else -1 for j in pos]
        short = int(len(pos) < n_top and full)
        if tally is not None:
            tally["partly"] = tally.get("partly", 0) + partly
            tally["short_full"] = tally.get("short_full", 0) + short
            tally["short_not_full"] = tally.get("short_not_full", 0) + int(len(pos) < min(n_top, len(L)) and not full)
    else:
        pos, claims, third, ties = share_lists(L, n_top, w)
        short = 0
        if tally is not None:
            tally["ties"] = tally.get("ties", 0) + ties
    differs = int(pos != list(range(min(len(L), n_top))))
    return [(j,) + tuple(pool[j]) + (claims[r],) for r, j in enumerate(pos)], (differs, len(pos), third, short)


def expected_pool(in_cnt, in_item, in_plain, in_decay, labels, n_top, mode, cap=1, lab_cap=None, lab_weight=None, lab_allow=None,
                  query_user=None, prof=None, tally=None):
    """(lists, stats [4]) over pools [Q][n_pool]; prof = (prof_ptr, prof_item) of the users query_user indexes (SHARE without lab_weight)"""
    in_item = np.asarray(in_item)
    Q, n_pool = in_item.shape
    assert 1 <= n_top <= n_pool <= MAX_POOL and n_pool * longest_row(labels) <= MAX_RECORDS
    assert check_tables(labels.n_items, labels.n_labels, labels.ptr, labels.id) is None
    lab_ok = allowed(lab_allow, labels.n_labels)
    lists, tot = [], [0, 0, 0, 0]
    for q in range(Q):
        m = min(max(int(in_cnt[q]), 0), n_pool)
        pool = [(int(in_item[q, j]), float(in_plain[q, j]), float(in_decay[q, j])) for j in range(m)]
        w = None
        if mode == SHARE:
            if lab_weight is not None:
                w = {l: int(x) for l, x in enumerate(lab_weight) if x} if not isinstance(lab_weight, dict) else lab_weight
            else:
                u = int(query_user[q])
                rows = prof[1][prof[0][u]:prof[0][u + 1]] if 0 <= u < len(prof[0]) - 1 else []
                w = history_weights(labels, lab_ok, rows)
        lst, st = quota_of(pool, int(in_cnt[q]) >= n_pool, labels, lab_ok, n_top, mode, cap, lab_cap, w, tally)
        lists.append(lst)
        tot = [a + b for a, b in zip(tot, st)]
    return lists, tuple(tot)


def expected_quota(scored, queries, labels, n_pool, n_top, rank_by, keep, n_w, mode, cap=1, lab_cap=None, lab_weight=None,
                   lab_allow=None, prof=None, allow=None, exclude=None, min_score=None, pools=None):
    """(lists, stats [10]) of the query users: the kept candidates are expected_filtered's with no cut, ranked into a pool of n_pool;
    the history of SHARE mode = the profiles prof = (prof_ptr, prof_item) of the users themselves.  pools (a list, or None) takes
    the size of every query's pool"""
    n_ids = labels.n_items
    kept, stats6 = expected_filtered(scored, queries, max(n_ids, 1), rank_by, keep, n_w, n_ids, allow=allow, exclude=exclude,
                                     min_score=min_score)
    lab_ok = allowed(lab_allow, labels.n_labels)
    lists, tot = [], [0, 0, 0, 0]
    for q, key in enumerate(queries):
        pool = pool_of(kept[q], rank_by, n_pool)
        if pools is not None:
            pools.append((len(kept[q]), len(pool)))
        w = None
        if mode == SHARE:
            if lab_weight is not None:
                w = {l: int(x) for l, x in enumerate(lab_weight) if x}
            else:
                u = int(key)
                rows = prof[1][prof[0][u]:prof[0][u + 1]] if 0 <= u < len(prof[0]) - 1 else []
                w = history_weights(labels, lab_ok, rows)
        lst, st = quota_of(pool, len(pool) == n_pool, labels, lab_ok, n_top, mode, cap, lab_cap, w)
        lists.append(lst)
        tot = [a + b for a, b in zip(tot, st)]
    return lists, tuple(stats6) + tuple(tot)


def to_arrays(lists, n_top):
    """(cnt [Q], item, plain, decayed, pos, label [Q][n_top]) with the padding of the header"""
    Q = len(lists)
    cnt = np.zeros(Q, np.int32)
    item, pos, label = np.full((Q, n_top), -1, np.int32), np.full((Q, n_top), -1, np.int32), np.full((Q, n_top), -1, np.int32)
    plain, decay = np.zeros((Q, n_top)), np.zeros((Q, n_top))
    for q, lst in enumerate(lists):
        cnt[q] = len(lst)
        for r, (j, it, p, d, l) in enumerate(lst):
            pos[q, r], item[q, r], plain[q, r], decay[q, r], label[q, r] = j, it, p, d, l
    return cnt, item, plain, decay, pos, label


NAMES = ("cnt", "item", "plain", "decay", "pos", "label")


def check_quota_output(got, lists, n_top):
    """the six arrays byte for byte (integers with array_equal, doubles through uint64 views)"""
    want = to_arrays(lists, n_top)
    for name, g, w in zip(NAMES, got, want):
        g = np.asarray(g).reshape(w.shape)
        if w.dtype == np.float64:
            g, w = np.ascontiguousarray(g, np.float64).view(np.uint64), w.view(np.uint64)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0].tolist()
            raise AssertionError("%s differs first at %s: got %r, statement %r" % (name, at, g[tuple(at)], w[tuple(at)]))


# ------------------------------------------------------------------------------------------------- the designed families
N_LABELS = 1 << 24
TOP_LABEL = N_LABELS - 1
N_ITEMS = 640
BUSY = 12               # labels 0 .. 11: the busy ones, where caps bind
N_USERS = 24
LAB_DENIED = (1, 4, 9, 21)
W32 = {0: 2 ** 31 - 1, 1: 2 ** 30 + 7}     # 32-bit products of these pick another list than 64-bit ones


def designed_labels(seed=5):
    """items 0 .. 399: one to three of the busy labels; 400 .. 499: none, or one of 20 .. 40; 500 .. 519: the top label 2^24 - 1
    beside a busy one; 520 .. 639: eight labels each (the longest row: 1 024 x 8 = MAX_RECORDS)"""
    rng = np.random.default_rng(seed)
    per = []
    for i in range(400):
        per.append(sorted(rng.choice(BUSY, size=int(rng.integers(1, 4)), replace=False).tolist()))
    for i in range(400, 500):
        per.append([] if i % 2 else [int(rng.integers(20, 41))])
    for i in range(500, 520):
        per.append([int(rng.integers(0, BUSY)), TOP_LABEL])
    for i in range(520, N_ITEMS):
        per.append(sorted(rng.choice(np.arange(0, 64), size=8, replace=False).tolist()))
    return Labels.of(per, N_LABELS)


def designed_allow():
    """the designed lab_allow as packed words (a bool array of 2^24 labels would do, the words are what the device takes)"""
    words = np.full(N_LABELS // 32, 0xffffffff, np.uint32)
    for l in LAB_DENIED:
        words[l >> 5] &= np.uint32(~(1 << (l & 31)) & 0xffffffff)
    return words


def designed_profiles(seed=6):
    """(prof_ptr, prof_item) of N_USERS users: user 0 without rows, user 1 holds item 7 twice, items -1 and N_ITEMS among the rows"""
    rng = np.random.default_rng(seed)
    rows = [[]] + [[7, 3, 7, 500]] + [rng.integers(-1, N_ITEMS + 1, int(rng.integers(1, 40))).tolist() for _ in range(N_USERS - 2)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, np.asarray([x for r in rows for x in r], np.int32)


def designed_pool(n_pool, Q, seed=7, eight=False):
    """a family of Q pools of n_pool positions: (in_cnt, in_item, in_plain, in_decay, query_user).  The counts go through 0, a
    negative one, n_pool + 3 (clamped), n_pool and values below it; the items are drawn with repeats from -1 .. N_ITEMS (both
    ends are outside the table); eight: only the eight-label items (the records reach n_pool x 8)"""
    rng = np.random.default_rng(seed + n_pool)
    lo, hi = (520, N_ITEMS) if eight else (-1, N_ITEMS + 1)
    item = rng.integers(lo, hi, (Q, n_pool)).astype(np.int32)
    if not eight and Q:
        item[0, 0], item[0, -1] = -1, N_ITEMS
        if n_pool >= 3:
            item[0, 2] = item[0, 1]             # a pool holding an item twice
        if n_pool >= 8:
            item[Q - 1, n_pool // 2] = 505      # the top label
    special = [n_pool, 0, -2, n_pool + 3, max(n_pool - 1, 0)]
    cnt = np.asarray([special[q] if q < len(special) else int(rng.integers(0, n_pool + 1)) for q in range(Q)], np.int32)
    plain, decay = np.round(rng.normal(size=(Q, n_pool)), 2) + 0.0, rng.normal(size=(Q, n_pool))
    user = rng.integers(-1, N_USERS + 1, Q).astype(np.int32)
    if Q > 1:
        user[0], user[1] = 1, 0
    return cnt, item, plain, decay, user


def designed_caps(seed=8):
    """lab_cap as {label: cap} over the labels the table uses (every other label: 2): zeros bar labels 2 and 30, INT32_MAX frees 5"""
    rng = np.random.default_rng(seed)
    caps = {l: int(rng.integers(1, 4)) for l in range(64)}
    caps.update({2: 0, 30: 0, 5: INT32_MAX, TOP_LABEL: 1})
    return caps


def designed_weights():
    """an editorial mix over the busy labels; every other label weighs nothing"""
    return {0: 7, 1: 7, 2: 3, 3: 1, 5: 2 ** 31 - 1, 7: 2, TOP_LABEL: 5}


def dense(mapping, default, dtype):
    """a {label: value} of the designed table as the device array [N_LABELS]"""
    a = np.full(N_LABELS, default, dtype)
    for l, v in mapping.items():
        a[l] = v
    return a


def hand_cases():
    """the hand-checked cases of the issue: (per-position labels, mode, n_top, cap or weights, positions, claims or None, third stat)"""
    return [([[0], [0, 1], [1], [0], [1], [], [2, 0]], CAP, 5, 1, [0, 2, 5], None, 4),
            ([[0], [0, 1], [1], [0], [1], [], [2, 0]], CAP, 7, 2, [0, 1, 2, 5], None, 3),
            ([[0], [1], [0], [1], [0], [0]], SHARE, 6, {0: 3, 1: 1}, [0, 2, 1, 4, 5, 3], [0, 0, 1, 0, 0, 1], 0)]


def alternating(n=40):
    """n single-label positions 0, 1, 0, 1, ... for the weights W32"""
    return [[j & 1] for j in range(n)]


class CapOf(object):
    """lab_cap as the statement's array-like: a {label: cap} with a default"""

    def __init__(self, caps, default):
        self.caps, self.default = caps, default

    def __getitem__(self, l):
        return self.caps.get(int(l), self.default)


def census(n_pools=(8, 63, 256), Q=12):
    """what the designed families hold, at the sizes the device tests use: every entry is a condition the tests assert"""
    labels, prof = designed_labels(), designed_profiles()
    cz = dict(differs=0, partly=0, barred=0, short_full=0, short_not_full=0, ties=0, fills=0)
    caps = CapOf(designed_caps(), 2)
    cz["barred"] = sum(v == 0 for v in designed_caps().values())
    for n_pool in n_pools:
        cnt, item, plain, decay, user = designed_pool(n_pool, Q)
        for n_top in sorted({1, max(n_pool // 3, 1), n_pool}):
            tally = {}
            st = expected_pool(cnt, item, plain, decay, labels, n_top, CAP, lab_cap=caps, tally=tally)[1]
            cz["differs"] += st[0]
            for k in ("partly", "short_full", "short_not_full"):
                cz[k] += tally.get(k, 0)
            st = expected_pool(cnt, item, plain, decay, labels, n_top, SHARE, query_user=user, prof=prof, tally=tally)[1]
            cz["differs"] += st[0]
            cz["fills"] += st[2]
            st = expected_pool(cnt, item, plain, decay, labels, n_top, SHARE, lab_weight=designed_weights(), tally=tally)[1]
            cz["ties"] += tally.get("ties", 0)
    L = alternating()
    cz["w32_lists_differ"] = share_lists(L, len(L), W32, 64)[0] != share_lists(L, len(L), W32, 32)[0]
    p_ptr, p_item = prof
    cz["user_holds_item_twice"] = any(len(set(r)) < len(r) for r in (p_item[p_ptr[u]:p_ptr[u + 1]].tolist() for u in range(N_USERS)))
    cnt, item, plain, decay, user = designed_pool(63, Q)
    cz["pool_holds_item_twice"] = any(len(set(item[q, :max(cnt[q], 0)].tolist())) < min(max(cnt[q], 0), 63) for q in range(Q))
    cz["items_outside"] = sorted(set(item[cnt > 0][:, [0, -1]].ravel().tolist()) & {-1, N_ITEMS})
    cz["top_label"] = int(labels.id.max())
    cnt, item, plain, decay, user = designed_pool(1024, 2, eight=True)
    cz["records_at_1024"] = sum(len(labels.carried(int(i))) for i in item[0])
    cz["longest_row"] = longest_row(labels)
    return cz
