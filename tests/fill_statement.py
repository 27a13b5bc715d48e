"""The popularity fill restated in NumPy / plain Python (no device): the ranking of xmap_pop_index and the completion of short
lists of xmap_topn_fill_rows as include/xmap_hip.h states them, a restatement of the double-double sums in the shape the kernels
add them in (for the census: tests/test_cpu_fill_statement.py), and the builders of the designed inputs of tests/test_gpu_fill.py.
The score sums of the statement are math.fsum, the correctly rounded sum."""
import math

import numpy as np

COUNT, MEAN = 0, 1
KEEP_HELD = 1
FILL_WINDOW = 4096          # XMAP_FILL_WINDOW (tests/test_cpu_fill_abi.py holds it to the header)
NAN = float("nan")


# ------------------------------------------------------------------------------------------------------- the ranking
def fsum(xs):
    """math.fsum; a sum that overflows (or adds opposite infinities) is not a number"""
    try:
        return math.fsum(xs)
    except (OverflowError, ValueError):
        return NAN


def pop_scores(n_items, hd_ptr, hd_x, how, damping, sums=None):
    """(n [I], score [I]) of the header's statement; sums = (S [I], G) replaces the fsum sums (the census passes the kernel-shaped
    double-double sums here)"""
    hd_ptr = np.asarray(hd_ptr, np.int64)
    n = np.diff(hd_ptr[:n_items + 1])
    if sums is None:
        S = np.asarray([fsum(hd_x[hd_ptr[i]:hd_ptr[i + 1]].tolist()) for i in range(n_items)], np.float64)
        T = int(hd_ptr[n_items]) if n_items else 0
        G = fsum(np.asarray(hd_x[:T], np.float64).tolist())
    else:
        S, G = np.asarray(sums[0], np.float64), sums[1]
    T = int(hd_ptr[n_items]) if n_items else 0
    with np.errstate(all="ignore"):
        mu = np.float64(G) / np.float64(T) if T > 0 else np.float64(0.0)
        if how == COUNT:
            score = n.astype(np.float64)
        else:
            a = np.float64(damping) * mu                        # one rounded operation per step
            score = (S + a) / (n.astype(np.float64) + np.float64(damping))
    return n, score


def pop_statement(n_items, hd_ptr, hd_x, how, damping, min_count, sums=None):
    """-> (pop_item [I], pop_score [I], pop_pos [I], (ranked, below min_count, non-finite))"""
    n, score = pop_scores(n_items, hd_ptr, hd_x, how, damping, sums)
    low = n < min_count
    bad = ~low & ~np.isfinite(score)
    ok = np.flatnonzero(~low & ~bad)
    key = score[ok] + 0.0                                       # -0.0 equals 0.0
    order = ok[np.lexsort((ok, -key))]                          # score descending as numbers, item index ascending
    pop_item, pop_score, pop_pos = np.full(n_items, -1, np.int32), np.zeros(n_items), np.full(n_items, -1, np.int32)
    pop_item[:len(order)] = order
    pop_score[:len(order)] = score[order]
    pop_pos[order] = np.arange(len(order))
    return pop_item, pop_score, pop_pos, (len(order), int(low.sum()), int(bad.sum()))


def n_ties(pop_score, n_ranked):
    """ranked positions whose score equals (as a number) the score in front"""
    s = pop_score[:n_ranked]
    return int((s[1:] == s[:-1]).sum())


# ---- the double-double sums in the kernels' shape
def dd_add(hi, lo, x):
    """common.h's dd_add, elementwise"""
    with np.errstate(all="ignore"):
        s = hi + x
        bb = s - hi
        e = (hi - (s - bb)) + (x - bb)
        e = e + lo
        h2 = s + e
        return h2, e - (h2 - s)


def _butterfly(hi, lo):
    """dd_reduce<64> over the last axis (64 lanes): lane 0's sum"""
    hi, lo = hi.copy(), lo.copy()
    m = 32
    while m >= 1:
        oh, ol = hi[..., m:2 * m].copy(), lo[..., m:2 * m].copy()
        h, l = dd_add(hi[..., :m], lo[..., :m], oh)
        h, l = dd_add(h, l, ol)
        hi[..., :m], lo[..., :m] = h, l
        m //= 2
    return hi[..., 0], lo[..., 0]


def dd_sums(n_items, hd_ptr, hd_x):
    """(S [I], G) as k_fl_sums and k_fl_total add them: per item lane l of 64 adds the holders l, l + 64, ... in holder order,
    then the fixed butterfly; G: thread t of 1024 adds the (hi, lo) of the items t, t + 1024, ..., the butterfly per wave, the 16
    wave sums left to right"""
    hd_ptr = np.asarray(hd_ptr, np.int64)
    x = np.concatenate([np.asarray(hd_x, np.float64), [0.0]])
    p0, p1 = hd_ptr[:n_items, None], hd_ptr[1:n_items + 1, None]
    hi, lo = np.zeros((n_items, 64)), np.zeros((n_items, 64))
    lanes = np.arange(64)[None, :]
    for k in range(int((np.diff(hd_ptr[:n_items + 1]).max(initial=0) + 63) // 64)):
        idx = p0 + 64 * k + lanes
        on = idx < p1
        h, l = dd_add(hi, lo, x[np.where(on, idx, len(x) - 1)])
        hi, lo = np.where(on, h, hi), np.where(on, l, lo)
    s_hi, s_lo = _butterfly(hi, lo)
    T = 1024
    pad = (-n_items) % T
    a_hi = np.concatenate([s_hi, np.zeros(pad)]).reshape(-1, T)
    a_lo = np.concatenate([s_lo, np.zeros(pad)]).reshape(-1, T)
    on_all = (np.arange(n_items + pad) < n_items).reshape(-1, T)
    hi, lo = np.zeros(T), np.zeros(T)
    for k in range(a_hi.shape[0]):
        h, l = dd_add(hi, lo, a_hi[k])
        h, l = dd_add(h, l, a_lo[k])
        hi, lo = np.where(on_all[k], h, hi), np.where(on_all[k], l, lo)
    w_hi, w_lo = _butterfly(hi.reshape(16, 64), lo.reshape(16, 64))
    g, glo = np.float64(0.0), np.float64(0.0)
    for w in range(16):
        g, glo = dd_add(g, glo, w_hi[w])
        g, glo = dd_add(g, glo, w_lo[w])
    return s_hi, float(g)


# ------------------------------------------------------------------------------------------------------- the fill
def fill_statement(query_user, n_top, flags, n_users, n_items, prof_ptr, prof_item, item_avg, n_ranked, pop_item, n_pop_items,
                   cnt, item, plain, decay, allow=None, exclude=None):
    """The loop of the header over copies of the lists.  allow = bool array [n_items] or None, exclude = one list of ids per query
    or None.  -> (cnt, item, plain, decay, src, [short on entry, filled to n_top, entries written, still short])"""
    cnt, item, plain, decay = [np.array(a, copy=True) for a in (cnt, item, plain, decay)]
    Q = len(query_user)
    src = np.full((Q, n_top), -1, np.int32)
    stats = [0, 0, 0, 0]
    for q in range(Q):
        u, c0 = int(query_user[q]), int(cnt[q])
        src[q, :c0] = 0
        if c0 >= n_top:
            continue
        skip = set(int(x) for x in item[q, :c0])
        if not (flags & KEEP_HELD) and 0 <= u < n_users:
            skip.update(int(x) for x in prof_item[prof_ptr[u]:prof_ptr[u + 1]])
        if exclude is not None:
            skip.update(int(x) for x in exclude[q] if 0 <= int(x) < n_items)
        c = c0
        for r in range(n_ranked):
            if c >= n_top:
                break
            i = int(pop_item[r])
            if i in skip or (allow is not None and not allow[i]):
                continue
            item[q, c], plain[q, c], decay[q, c], src[q, c] = i, item_avg[i], item_avg[i], 1
            c += 1
        cnt[q] = c
        stats[0] += 1
        stats[1 if c == n_top else 3] += 1
        stats[2] += c - c0
    return cnt, item, plain, decay, src, stats


# ------------------------------------------------------------------------------------------------------- designed indexes
FAMILIES = ("dyadic", "tenths")
INDEX_ITEMS = 2500          # three strides of the 1024 threads of the total, the last one ragged
MIN_COUNTS = (1, 3)
DAMPINGS = (0.0, 0.5, 25.0)
TENTHS_SEED = 11            # chosen so that the double-double sums rounded once equal math.fsum everywhere (asserted by the census)


class Index(object):
    """an item-major index as xmap_peer_index leaves it: hd_ptr [I + 1], hd_x; .special = {name: item}"""

    def __init__(self, n_items, rows, special=None):
        self.n_items = n_items
        self.hd_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        self.hd_x = np.asarray([x for r in rows for x in r], np.float64)
        self.special = special or {}


def design_index(family):
    """2500 items with 0 .. 12 holders (two with 200 and 130: more than one lane stride), 160 items that repeat another item's
    ratings in another order (ties under MEAN), and at the front: a pair whose ratings cancel beside one of -0.0 ratings only (score
    0.0 under MEAN with damping 0), an item with exactly 3 holders and one with 2.  dyadic: ratings k / 2^20, |r| <= 2^10 -- every
    sum is exact whatever the order; tenths: ratings k / 10."""
    rng = np.random.default_rng(TENTHS_SEED if family == "tenths" else 3)
    I = INDEX_ITEMS

    def draw(k):
        if family == "dyadic":
            return (rng.integers(-2 ** 30, 2 ** 30 + 1, k) / 2.0 ** 20).tolist()
        return (rng.integers(5, 51, k) / 10.0).tolist()

    rows = [draw(int(k)) for k in rng.integers(0, 13, I)]
    one = draw(1)[0]
    rows[0] = [one, -one]
    rows[1] = [-0.0, -0.0]
    rows[2] = draw(3)
    rows[3] = draw(2)
    rows[4] = []
    rows[700], rows[1900] = draw(200), draw(130)
    for k in range(160):                        # ties under MEAN: the same ratings, reversed
        rows[2000 + 3 * k] = rows[10 + 5 * k][::-1]
    return Index(I, rows, dict(cancel=0, zeros=1, at_min=2, below_min=3, no_holder=4))


def overflow_index():
    """item 0's ratings sum to infinity: under MEAN its sum, the total and with it every score is not a number"""
    return Index(5, [[1e308, 1e308], [1.0, 2.0], [3.0], [], [1e308, -1e308, 5.0]])


TINY = 5e-324               # the smallest fp64 denormal


def zero_index():
    """Scores of +0.0 and -0.0 side by side under MEAN with damping 0: a sum that is a negative denormal, divided by two or three
    holders, underflows to -0.0 (items 1 and 3); ratings that cancel and ratings that are zero give +0.0 (items 0 and 2).  The four
    tie as numbers, so the item index orders them -- between item 4 (2.0) and item 5 (-1.0) -- while pop_score keeps each score's
    own bits."""
    return Index(6, [[1.0, -1.0], [-TINY, 0.0], [0.0, 0.0, 0.0], [-TINY, 0.0, 0.0], [2.0], [-1.0]], dict(plus=(0, 2), minus=(1, 3)))


# ------------------------------------------------------------------------------------------------------- designed fills
N_TOPS = (1, 10, 63, 64)


class FillDesign(object):
    pass


def design_fill():
    """About 2 * 4096 + 100 ranked ids, 21 batch ids behind them, and the queries of the census: users who hold the first
    FILL_WINDOW - 1 / FILL_WINDOW / FILL_WINDOW + 1 ranked items, a user whose held, listed and excluded ids cover the ranking, an
    empty user, lists that need one entry, full lists, users -1 and n_users, a repeated query with two exclusion lists, ids outside
    the id space, a profile that holds an item twice, a listed item that is held, listed batch ids, and 30 random queries."""
    rng = np.random.default_rng(7)
    W = FILL_WINDOW
    D = FillDesign()
    D.n_pop_items = n_pop = 2 * W + 108
    D.n_items = n_items = n_pop + 21                           # (no multiple of 32: the mask's last word has bits beyond it)
    perm = rng.permutation(n_pop)
    perm = np.concatenate([[5], perm[perm != 5]])              # the head of the ranking is item 5: no mask of the tests allows it
    D.n_ranked = n_ranked = n_pop - 50
    D.pop_item = np.full(n_pop, -1, np.int32)
    D.pop_item[:n_ranked] = perm[:n_ranked]
    D.pop_pos = np.full(n_pop, -1, np.int32)
    D.pop_pos[perm[:n_ranked]] = np.arange(n_ranked)
    D.item_avg = rng.integers(8, 41, n_items) / 8.0 + rng.random(n_items) / 1024.0
    rk = D.pop_item[:n_ranked]
    tail = rk[n_ranked - 30:]
    profiles = {
        "w-1": rk[:W - 1], "w": rk[:W], "w+1": rk[:W + 1], "cover": rk[:n_ranked - 30], "empty": rk[:0],
        "one": rng.choice(n_pop, 40, replace=False), "full": rng.choice(n_pop, 25, replace=False),
        "twice": np.concatenate([rk[:3], rk[:1], rk[7:9]]), "held": rk[10:20], "batch": rk[1:4],
    }
    for k in range(30):
        profiles["r%d" % k] = np.concatenate([rk[:int(rng.integers(0, 90))], rng.choice(rk[:200], int(rng.integers(0, 60)), replace=False)])
    D.users = list(profiles)
    D.n_users = len(D.users)
    rows = [rng.permutation(np.asarray(profiles[u], np.int64)) for u in D.users]      # stage-C row order: not sorted by item
    D.prof_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    D.prof_item = np.concatenate(rows).astype(np.int32)
    uix = {u: k for k, u in enumerate(D.users)}
    far = rk[n_ranked - 400:n_ranked - 100]                    # listed items far down the ranking: no unmasked fill reaches them

    def listed(k):
        return rng.choice(far, k, replace=False)

    # (user index, the list's items, how many of them stand in a list of n_top, the exclusion list)
    queries = [
        (uix["w-1"], listed(3), "k", []), (uix["w"], listed(3), "k", []), (uix["w+1"], listed(3), "k", []),
        (uix["cover"], tail[:10], "short", tail.tolist()),
        (uix["empty"], listed(0), "k", []),
        (uix["one"], listed(64), "one", []), (uix["one"], listed(64), "one", rk[:6].tolist() + [-1, n_items, 2 ** 31 - 1, int(rk[2]), int(rk[2])]),
        (uix["one"], listed(64), "one", rk[3:9].tolist()),
        (uix["full"], listed(64), "full", rk[:5].tolist()),
        (-1, listed(2), "k", []), (D.n_users, listed(0), "k", [int(rk[0])]),
        (uix["twice"], listed(1), "k", []),
        (uix["held"], np.concatenate([rk[12:14], listed(2)]), "k", []),
        (uix["batch"], np.concatenate([[n_pop + 3, n_pop + 7], listed(2)]), "k", [n_pop + 1]),
    ]
    for k in range(30):
        queries.append((uix["r%d" % k], np.concatenate([rk[rng.choice(120, int(rng.integers(0, 8)), replace=False)], listed(int(rng.integers(0, 5)))]),
                        "k", rk[rng.choice(150, int(rng.integers(0, 12)), replace=False)].tolist()))
    D.queries = queries
    D.names = ["w-1", "w", "w+1", "cover", "empty", "one", "one-ex", "one-ex2", "full", "anon", "beyond", "twice", "held", "batch"] + \
              ["r%d" % k for k in range(30)]
    D.query_user = np.asarray([q[0] for q in queries], np.int32)
    D.exclude = [list(q[3]) for q in queries]
    D.list_values = rng.integers(8, 41, (len(queries), 64)) / 8.0
    # masks over the n_items ids: the first three words clear (the ranking's head, item 5, is not allowed: every position shifts),
    # and a 1 % mask
    half = rng.random(n_items) < 0.5
    half[:96] = False
    D.masks = {"half": half, "one-percent": rng.random(n_items) < 0.01}
    return D


def lists_for(D, n_top):
    """the lists of the designed queries at a width: (cnt, item, plain, decay) with -1 / 0.0 behind the count, as the top-N calls
    write them"""
    Q = len(D.queries)
    cnt, item = np.zeros(Q, np.int32), np.full((Q, n_top), -1, np.int32)
    plain, decay = np.zeros((Q, n_top)), np.zeros((Q, n_top))
    for q, (_, items, kind, _) in enumerate(D.queries):
        c = {"k": min(len(items), n_top), "short": min(len(items), n_top - 1), "one": n_top - 1, "full": n_top}[kind]
        cnt[q] = c
        item[q, :c] = items[:c]
        plain[q, :c] = D.list_values[q, :c]
        decay[q, :c] = D.list_values[q, :c] - 0.125
    return cnt, item, plain, decay


def mask_words(on, garbage=True):
    """a bool array [n] as uint32 mask words; the bits at and beyond n SET when garbage (they may hold anything)"""
    n = len(on)
    pad = np.full((n + 31) // 32 * 32, 1 if garbage else 0, np.uint8)
    pad[:n] = on
    return np.packbits(pad, bitorder="little").view("<u4").astype(np.uint32)


def short_ranking(D, n_ranked=5):
    """the ranking cut to its first n_ranked positions: shorter than a need of 64"""
    pop_item, pop_pos = np.full_like(D.pop_item, -1), np.full_like(D.pop_pos, -1)
    pop_item[:n_ranked] = D.pop_item[:n_ranked]
    pop_pos[D.pop_item[:n_ranked]] = np.arange(n_ranked)
    return n_ranked, pop_item, pop_pos
