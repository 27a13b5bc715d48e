"""The statement of the allotment (include/xmap_hip.h, "allotment"; xmap_allot_pool / xmap_allot_rows / xmap_ctx_recommend_allot) in
NumPy and plain Python, for the tests on both sides.

Inputs: Q pools in the top-N layout (cnt [Q], item / plain / decay [Q][n_pool]), rank_by 0 or 1, n_top <= n_pool, capacities
cap(i) >= 0 per item (0 bars the item, INT32_MAX is no cap).
  m(q) = clamp(cnt[q], 0, n_pool).  Position (q, j) is VOID if j >= m(q), the item is outside [0, n_items), or its capacity is 0.
  The same item at two positions of one pool is two independent positions.
  Offer order: k(q, j) = (order_key(score), qid[q], j), ascending lexicographically = better first (qid[q] = q unless the caller
  renumbers the queries: a permuted input with qid = the original numbers is the same market).
  Outcome: R = the smallest set of refused positions such that
    the proposals P(q) of each query are its first n_top positions that are neither void nor in R;
    the offers of each item i are all proposals holding i;
    every offer of i that is not among its cap(i) best by k is in R.
`allot_rounds` iterates "propose, refuse the excess, add to R" from R = {} in synchronous rounds (vectorised); `allot_sequential`
is an independent formulation: one offer at a time in an order the caller chooses, an over-full item evicting its worst held offer.
R is the least fixed point of a monotone operator, so both give the same lists (tests/test_cpu_allot_statement.py)."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
MAX_POOL = 1024
SIGN = np.uint64(1 << 63)
FAMILIES = ("all_equal", "signed_zero", "negative", "inf_and_subnormal", "descending_random")


def order_key(score):
    """au_key of csrc/au_select.h on uint64 views: ascends where the score descends; -0.0 and 0.0 share a key"""
    b = (np.asarray(score, np.float64) + 0.0).view(np.uint64)
    return np.where((b >> np.uint64(63)).astype(bool), b, ~(b | SIGN))


class Pool(object):
    """pools in the top-N layout on the host"""

    def __init__(self, cnt, item, plain, decay, n_items):
        self.cnt, self.item = np.ascontiguousarray(cnt, np.int32), np.ascontiguousarray(item, np.int32)
        self.plain, self.decay = np.ascontiguousarray(plain, np.float64), np.ascontiguousarray(decay, np.float64)
        self.Q, self.n_pool = self.item.shape
        self.n_items = int(n_items)
        assert self.cnt.shape == (self.Q,) and self.plain.shape == self.item.shape == self.decay.shape

    def score(self, rank_by):
        return self.decay if rank_by else self.plain

    def m(self):
        return np.clip(self.cnt.astype(np.int64), 0, self.n_pool)

    def permuted(self, perm):
        """query q' of the result is query perm[q'] of this pool"""
        return Pool(self.cnt[perm], self.item[perm], self.plain[perm], self.decay[perm], self.n_items)

    def swapped(self):
        return Pool(self.cnt, self.item, self.decay, self.plain, self.n_items)


def caps_of(pool, cap=1, item_cap=None):
    """the capacity of every item as int64 [n_items]"""
    if item_cap is None:
        assert cap >= 1
        return np.full(pool.n_items, int(cap), np.int64)
    c = np.asarray(item_cap, np.int64)
    assert c.shape == (pool.n_items,) and (c >= 0).all()
    return c


def void_mask(pool, caps):
    j = np.arange(pool.n_pool)[None, :]
    inside = (pool.item >= 0) & (pool.item < pool.n_items)
    barred = np.zeros(pool.item.shape, bool)
    barred[inside] = caps[pool.item[inside]] == 0
    return (j >= pool.m()[:, None]) | ~inside | barred


def global_rank(pool, rank_by, qid=None):
    """the place of every position in the offer order k: [Q][n_pool] int64"""
    Q, n_pool = pool.item.shape
    key = order_key(pool.score(rank_by)).ravel()
    q = np.repeat(np.arange(Q) if qid is None else np.asarray(qid), n_pool)
    j = np.tile(np.arange(n_pool), Q)
    o = np.lexsort((j, q, key))
    rank = np.empty(Q * n_pool, np.int64)
    rank[o] = np.arange(Q * n_pool)
    return rank.reshape(Q, n_pool)


class Result(object):
    """cnt [Q], item / plain / decay / pos [Q][n_top], taken [n_items], stats [6], held = the bool mask [Q][n_pool] of P"""

    def __init__(self, pool, n_top, held, refused, void, rounds):
        Q, n_pool = pool.item.shape
        self.held = held
        self.cnt = held.sum(axis=1).astype(np.int32)
        self.item = np.full((Q, n_top), -1, np.int32)
        self.plain, self.decay = np.zeros((Q, n_top)), np.zeros((Q, n_top))
        self.pos = np.full((Q, n_top), -1, np.int32)
        qq, jj = np.nonzero(held)               # (row-major: ascending position inside a query)
        slot = (np.cumsum(held, axis=1) - 1)[qq, jj]
        self.item[qq, slot], self.pos[qq, slot] = pool.item[qq, jj], jj
        self.plain[qq, slot], self.decay[qq, slot] = pool.plain[qq, jj], pool.decay[qq, jj]
        self.taken = np.bincount(pool.item[qq, jj], minlength=pool.n_items).astype(np.int32)
        m = pool.m()
        n = np.minimum(m, n_top)
        prefix = np.arange(n_pool)[None, :] < n[:, None]
        self.stats = [int((held != prefix).any(axis=1).sum()), int(self.cnt.sum()), int(refused.sum()),
                      int((void & (np.arange(n_pool)[None, :] < m[:, None])).sum()), int(rounds),
                      int(((self.cnt < n_top) & (pool.cnt >= n_pool)).sum())]

    def lists(self):
        return [self.cnt, self.item, self.plain, self.decay, self.pos]


def allot_rounds(pool, n_top, cap=1, item_cap=None, rank_by=0, qid=None):
    """the round statement: Result; stats[4] = the rounds of the plain synchronous schedule, the last empty one included"""
    assert 1 <= n_top <= pool.n_pool <= MAX_POOL and rank_by in (0, 1)
    caps = caps_of(pool, cap, item_cap)
    void = void_mask(pool, caps)
    rank = global_rank(pool, rank_by, qid)
    refused = np.zeros(pool.item.shape, bool)
    rounds = 0
    while True:
        live = ~(void | refused)
        prop = live & (np.cumsum(live, axis=1) <= n_top)
        rounds += 1
        qq, jj = np.nonzero(prop)
        it, rk = pool.item[qq, jj].astype(np.int64), rank[qq, jj]
        o = np.lexsort((rk, it))
        its = it[o]
        head = np.ones(len(o), bool)
        head[1:] = its[1:] != its[:-1]
        start = np.maximum.accumulate(np.where(head, np.arange(len(o)), 0))
        excess = (np.arange(len(o)) - start) >= caps[its] if len(o) else np.zeros(0, bool)
        if not excess.any():
            return Result(pool, n_top, prop, refused, void, rounds)
        refused[qq[o][excess], jj[o][excess]] = True


def allot_sequential(pool, n_top, cap=1, item_cap=None, rank_by=0, order="ascending", seed=0, qid=None):
    """An independent statement: one offer at a time.  A query with fewer than n_top held offers and an untried position makes its next
    offer; the item takes it and, over capacity, evicts the worst offer it holds (by k), which is refused for good.  `order` picks
    which such query moves next: "ascending", "descending" or "random" (seeded).  Returns the bool mask [Q][n_pool] of held offers."""
    caps = caps_of(pool, cap, item_cap)
    void = void_mask(pool, caps)
    key = order_key(pool.score(rank_by))
    Q, n_pool = pool.item.shape
    ids = list(range(Q)) if qid is None else [int(x) for x in qid]
    nxt, n_held = [0] * Q, [0] * Q
    held_by = {}                                # item -> list of (key, qid, j, q)
    held = np.zeros((Q, n_pool), bool)
    rng = np.random.RandomState(seed)

    def can_move(q):
        while nxt[q] < n_pool and void[q, nxt[q]]:
            nxt[q] += 1
        return n_held[q] < n_top and nxt[q] < n_pool

    while True:
        able = [q for q in range(Q) if can_move(q)]
        if not able:
            return held
        q = able[0] if order == "ascending" else able[-1] if order == "descending" else able[rng.randint(len(able))]
        j = nxt[q]
        nxt[q] += 1
        i = int(pool.item[q, j])
        offers = held_by.setdefault(i, [])
        offers.append((int(key[q, j]), ids[q], j, q))
        held[q, j] = True
        n_held[q] += 1
        if len(offers) > caps[i]:
            worst = max(offers)
            offers.remove(worst)
            held[worst[3], worst[2]] = False
            n_held[worst[3]] -= 1


def check_allot_output(pool, n_top, got, guard=-7):
    """the layout of (cnt, item, plain, decay, pos): shapes, no pre-fill left, the blanks behind the counts, pos strictly ascending
    below m(q), items and score bits those of the pool at pos"""
    cnt, item, plain, decay, pos = got
    Q = pool.Q
    assert cnt.shape == (Q,) and all(a.shape == (Q, n_top) for a in (item, plain, decay, pos))
    assert cnt.dtype == item.dtype == pos.dtype == np.int32 and plain.dtype == decay.dtype == np.float64
    assert ((cnt >= 0) & (cnt <= n_top)).all()
    behind = np.arange(n_top)[None, :] >= cnt[:, None]
    assert (item[behind] == -1).all() and (pos[behind] == -1).all()
    assert (plain[behind].view(np.uint64) == 0).all() and (decay[behind].view(np.uint64) == 0).all()
    qq, ss = np.nonzero(~behind)
    p = pos[qq, ss]
    assert ((p >= 0) & (p < pool.m()[qq])).all()
    asc = (pos[:, 1:] > pos[:, :-1]) | behind[:, 1:]
    assert asc.all()
    assert np.array_equal(item[qq, ss], pool.item[qq, p])
    assert np.array_equal(plain[qq, ss].view(np.uint64), pool.plain[qq, p].view(np.uint64))
    assert np.array_equal(decay[qq, ss].view(np.uint64), pool.decay[qq, p].view(np.uint64))


def held_mask(pool, cnt, pos):
    held = np.zeros(pool.item.shape, bool)
    qq, ss = np.nonzero(np.arange(pos.shape[1])[None, :] < cnt[:, None])
    held[qq, pos[qq, ss]] = True
    return held


def is_stable(pool, n_top, held, cap=1, item_cap=None, rank_by=0, qid=None):
    """No item is over capacity, and for every non-void position that is not held: either its query is full with positions all
    smaller than it, or its item holds cap offers all better by k."""
    caps = caps_of(pool, cap, item_cap)
    void = void_mask(pool, caps)
    if (held & void).any() or (held.sum(axis=1) > n_top).any():
        return False
    rank = global_rank(pool, rank_by, qid)
    qq, jj = np.nonzero(held)
    it = pool.item[qq, jj]
    taken = np.bincount(it, minlength=pool.n_items)
    if (taken > caps).any():
        return False
    worst = np.full(pool.n_items, -1, np.int64)         # the worst rank an item holds
    np.maximum.at(worst, it, rank[qq, jj])
    n_held = held.sum(axis=1)
    last = np.where(held, np.arange(pool.n_pool)[None, :], -1).max(axis=1)
    uq, uj = np.nonzero(~held & ~void)
    ui = pool.item[uq, uj]
    query_full = (n_held[uq] == n_top) & (last[uq] < uj)
    item_full = (taken[ui] == caps[ui]) & (worst[ui] < rank[uq, uj])
    return bool((query_full | item_full).all())


# ---------------------------------------------------------------------------------------------------------------- the designed pools
def family_scores(family, Q, n_pool, rng):
    """[Q][n_pool] scores of a family, descending inside a pool where the family has an order"""
    if family == "all_equal":
        return np.full((Q, n_pool), 1.0)
    if family == "signed_zero":
        return np.where(rng.randint(0, 2, (Q, n_pool)) == 1, -0.0, 0.0)
    if family == "negative":
        return -np.sort(rng.randint(1, 50, (Q, n_pool)).astype(np.float64) / 8.0, axis=1)
    if family == "inf_and_subnormal":
        vals = np.array([np.inf, 1.0, 2e-310, 5e-324, 0.0, -0.0, -5e-324, -2e-310, -1.0, -np.inf])
        pick = np.sort(rng.randint(0, len(vals), (Q, n_pool)), axis=1)
        return vals[pick]
    assert family == "descending_random"
    return -np.sort(-rng.random_sample((Q, n_pool)), axis=1)


def designed_pool(Q, n_pool, family, seed, n_items=None, voids=True, repeat=False):
    """Q pools over n_items (default n_pool + 7) items, every pool a random draw without repetition (repeat: with), scores of
    `family` in the plain column and of "descending_random" in the decayed one.  voids: item ids -1 and n_items at some positions,
    in_cnt negative, short and above n_pool for some queries."""
    rng = np.random.RandomState(seed)
    I = n_pool + 7 if n_items is None else n_items
    if repeat or I < n_pool:
        item = rng.randint(0, I, (Q, n_pool))
    else:
        item = np.argsort(rng.random_sample((Q, I)), axis=1)[:, :n_pool]
    item = item.astype(np.int32)
    cnt = np.full(Q, n_pool, np.int32)
    if voids:
        holes = rng.random_sample((Q, n_pool))
        item[holes < 0.03] = -1
        item[holes > 0.97] = I
        kind = rng.randint(0, 8, Q)
        cnt[kind == 0] = -3
        cnt[kind == 1] = n_pool + 5
        short = kind == 2
        cnt[short] = rng.randint(0, n_pool + 1, int(short.sum()))
    return Pool(cnt, item, family_scores(family, Q, n_pool, rng), family_scores("descending_random", Q, n_pool, rng), I)


def designed_caps(n_items, seed):
    """an item_cap array with every kind of entry: 0 (barred), 1, 2, INT32_MAX"""
    rng = np.random.RandomState(seed)
    return np.array([0, 1, 2, INT32_MAX, 1, 1, 2], np.int32)[rng.randint(0, 7, n_items)]


def chain_pool(Q=64):
    """Query k holds [item k - 1, item k] with scores 2 (Q - k), 2 (Q - k) - 1; query 0 holds [item 0].  n_top 1, cap 1: query 0
    keeps item 0; query 1 loses item 0 to it (2 Q - 2 < 2 Q) and moves to item 1, which it takes from query 2 in the next round,
    and so on: query 0 ends on position 0, every other query on position 1, one refusal per round: Q rounds with the empty last."""
    item = np.full((Q, 2), -1, np.int32)
    plain = np.zeros((Q, 2))
    cnt = np.full(Q, 2, np.int32)
    for k in range(Q):
        if k == 0:
            item[0, 0], plain[0, 0], cnt[0] = 0, 2.0 * Q, 1
        else:
            item[k] = (k - 1, k)
            plain[k] = (2.0 * (Q - k), 2.0 * (Q - k) - 1.0)
    return Pool(cnt, item, plain, plain.copy(), Q)


def ladder_pool(Q=257, n_pool=1024):
    """every query holds the items 0 .. n_pool - 1 in this order with equal scores: with n_top 1 and cap 1 query q loses item 0 .. q - 1
    to the smaller queries, one per round, and ends on position q -- a walk across the words and the waves of the bitmap, Q rounds"""
    item = np.tile(np.arange(n_pool, dtype=np.int32), (Q, 1))
    plain = np.full((Q, n_pool), 0.5)
    return Pool(np.full(Q, n_pool, np.int32), item, plain, plain.copy(), n_pool)


def crowd_pool(Q=1500, n_pool=3):
    """item 0 first in every pool (cap 1 100 < Q: a run and a cap above 1 024), two private items behind it; scores descend with q"""
    item = np.empty((Q, n_pool), np.int32)
    item[:, 0] = 0
    for j in range(1, n_pool):
        item[:, j] = 1 + (np.arange(Q) * (n_pool - 1) + (j - 1))
    plain = np.empty((Q, n_pool))
    plain[:, 0] = 1.0 + (Q - np.arange(Q)) / 4.0
    for j in range(1, n_pool):
        plain[:, j] = 1.0 / (j + 1)
    return Pool(np.full(Q, n_pool, np.int32), item, plain, plain.copy(), 1 + Q * (n_pool - 1))
