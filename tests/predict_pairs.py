"""Designed (user, item) pairs for k_predict (csrc/stage_e.hip: xmap_predict) and the statement of what it has to return for
them, status included.  No device and no torch: tests/test_cpu_predict_pairs.py takes the census, tests/test_gpu_predict_pairs.py
uploads the arrays.

The statement is RecommenderPrediction._predict_pair (pinned to the reference by tests/test_cpu_downstream.py) on the three
dictionaries the case's arrays stand for.  Ids have one width, so the reference's `uid in rater` is an equality.  Per pair it
gives (status, plain, decay):

  ()                                                              -> status 1
  more than PRED_EV = 64 evidence entries, or n + 1 > n_w         -> status 2   (the decay table has n_w entries)
  ZeroDivisionError, ValueError, OverflowError, or a NaN returned -> status 2   (the host's pairs: Python raises there)
  otherwise                                                       -> status 0 with the two bounded values

and the outputs of a pair with status != 0 are 0.0.  xmap_predict is called DIRECTLY by the GPU test, so a kernel that hands
back a pair it should have computed -- or computes one it should hand back -- shows; behind
RecommenderPrediction._device_recommendation every status-2 pair goes to the Python statement and the tuples agree either way.

The pairs (ratings, similarities and averages are thirds and sevenths: a changed summation order changes bits):

  counts    n in COUNTS evidence entries, each built three ways (HOWS): `run` one neighbour the user holds n times, a run inside
            the neighbour's raters; `spread` n neighbours held once each (n = 0: an EMPTY neighbour list, the item average);
            `mix` about sqrt(n) neighbours with n / sqrt(n) ratings each and one more with the remainder (64 = 8 x 8).
            With N_WS = (2, 64, 65, 66): at 65, n = 64 is status 0; at 64, n = 64 is 2 and n = 63 is 0; at 2 only n <= 1 is 0.
  times     PATTERNS over 64 entries, `spread` and 8 x 8: all equal (one rank), strictly ascending, strictly descending (the
            insertion sort's longest path), two alternating values, and eight interleaved blocks of eight ties -- inside a tie
            the evidence keeps its list order (the reference's sort is stable).  The rating rises with the time, so the decayed
            value leaves the plain one where the ranks are wrong.
  raters    the user first in a neighbour's raters (as a run of two), last (a run of two), between two raters but absent, below
            all, above all, the only rater; tu = -1 (a user who rated nothing); ti = -1 (an item without a list: ()).
  values    a prediction exactly at x.5 (2.5 -> 3.0, 4.5 -> 5.0), below 0 and above 5, +-1e300 as an average and as a rating;
            every contributing similarity 0.0 or -0.0 (status 2), a neighbour average of inf with evidence (2) and without
            (0), a NaN rating (2), an item average of NaN without evidence (2).  ALPHAS has 800: every weight of the decay
            table but wtab[0] is 0.0, so every pair with evidence is status 2.

n_test is 128 m + 1, pairs repeated in turn: a block has 128 threads, the last block one.
"""
import functools

import numpy as np

PRED_EV = 64
COUNTS = (0, 1, 2, 63, 64, 65, 66, 130)
HOWS = ("run", "spread", "mix")
PATTERNS = ("equal", "ascending", "descending", "alternating", "blocks")
N_WS = (2, 64, 65, 66)
ALPHAS = (0.05, 1.5, 800.0)
N_TEST = 129
USER = 500                      # the query user of the count / time / value pairs
NO_USER, NO_ITEM = "u99999", "i99999"


def uname(u):
    return NO_USER if u < 0 else "u%05d" % u


def iname(i):
    return NO_ITEM if i < 0 else "i%05d" % i


class Case(object):
    """items with their average, neighbour list and raters; pairs (user, item) with a tag each"""
    def __init__(self):
        self.avg, self.nb, self.rt, self.pairs, self.tags = [], [], [], [], []

    def item(self, avg, ratings=(), nb=()):
        """ratings: (user, rating, time)* -- stored by ascending user, a user's ratings in the order given"""
        self.avg.append(float(avg))
        self.nb.append([(int(n), float(s)) for n, s in nb])
        self.rt.append(sorted(((int(u), float(r), float(t)) for u, r, t in ratings), key=lambda x: x[0]))
        return len(self.avg) - 1

    def pair(self, u, it, **tag):
        self.pairs.append((int(u), int(it)))
        self.tags.append(tag)


def groups_of(n, how):
    """ratings the user holds of each neighbour of the list, in list order"""
    if how == "run":
        return [n]
    if how == "spread":
        return [1] * n
    if n <= 2:
        return [0] + [1] * n
    k = int(np.sqrt(n))
    return [n // k] * k + ([n - k * (n // k)] if n % k else [])


def _held_neighbours(c, groups, rating_of, time_of, sim_of=None, navg_of=None):
    """one neighbour item per group: the query user's ratings between (or not) other raters.  -> the neighbour list"""
    nb, e = [], 0
    for j, g in enumerate(groups):
        rows = []
        if j % 3 != 1:
            rows.append((3 + j % 2, 1.0 + 1.0 / 3.0, 5.0))
        for _ in range(g):
            rows.append((USER, rating_of(e), time_of(e)))
            e += 1
        if j % 3 != 2:
            rows.append((900, 4.0 / 3.0, 2.0))
        navg = (2.0 + (j % 3) / 3.0) if navg_of is None else navg_of(j)
        sim = (((j % 5) + 1) / 7.0 * (-1.0 if j % 4 == 3 else 1.0)) if sim_of is None else sim_of(j)
        nb.append((c.item(navg, rows), sim))
    return nb


@functools.lru_cache(maxsize=None)
def case():
    c = Case()
    # ---- evidence counts
    for n in COUNTS:
        for how in HOWS:
            nb = _held_neighbours(c, groups_of(n, how), lambda e: ((e * 7) % 16) / 3.0, lambda e: float((e * 37) % 11))
            c.pair(USER, c.item(2.9, nb=nb), kind="count", n=n, how=how)
    # ---- time patterns over 64 entries
    time_of = dict(equal=lambda e: 7.0, ascending=lambda e: float(e), descending=lambda e: float(64 - e),
                   alternating=lambda e: float(e % 2), blocks=lambda e: float((e * 5) % 8))
    for pattern in PATTERNS:
        tf = time_of[pattern]
        ts = [tf(e) for e in range(64)]
        lo, span = min(ts), max(max(ts) - min(ts), 1.0)
        rating_of = lambda e, tf=tf, lo=lo, span=span: 0.4 + 4.2 * (tf(e) - lo) / span + (e % 3) / 30.0
        for how in ("spread", "mix"):
            nb = _held_neighbours(c, groups_of(64, how), rating_of, tf, sim_of=lambda j: ((j % 5) + 1) / 7.0,
                                  navg_of=lambda j: 2.0 + 1.0 / 3.0)
            c.pair(USER, c.item(2.0 + 2.0 / 3.0, nb=nb), kind="time", pattern=pattern, how=how)
    # ---- the rater search
    x = c.item(3.0 + 1.0 / 3.0, [(10, 1.0 / 3.0, 4.0), (10, 5.0, 1.0), (20, 2.0, 2.0), (30, 4.0, 3.0), (40, 14.0 / 3.0, 9.0), (40, 0.5, 8.0)])
    y = c.item(1.0 + 2.0 / 3.0, [(77, 13.0 / 3.0, 6.0)])
    q = c.item(3.1, nb=[(x, 2.0 / 7.0), (y, -3.0 / 7.0), (x, 5.0 / 7.0)])
    for u, where in ((10, "first"), (40, "last"), (25, "between"), (5, "below"), (45, "above"), (77, "only"), (-1, "no user")):
        c.pair(u, q, kind="rater", where=where)
    c.pair(10, -1, kind="rater", where="no item")
    c.pair(-1, -1, kind="rater", where="neither")
    # ---- values
    for avg in (2.5, 4.5, np.nextafter(2.5, 0.0), -3.0, -0.5, 7.2, 1e300, -1e300, np.nan, np.inf):
        c.pair(USER, c.item(avg), kind="value", what="average %r alone" % avg)
    one = lambda rating, navg=2.0 + 1.0 / 3.0, sim=3.0 / 7.0: (c.item(navg, [(3, 1.0, 1.0), (USER, rating, 3.0), (900, 2.0, 2.0)]), sim)
    c.pair(USER, c.item(4.9, nb=[one(5.0), one(14.0 / 3.0, 1.0 / 3.0)]), kind="value", what="above 5 with evidence")
    c.pair(USER, c.item(0.2, nb=[one(1.0 / 3.0, 4.0), one(0.0, 11.0 / 3.0)]), kind="value", what="below 0 with evidence")
    c.pair(USER, c.item(3.0, nb=[one(1e300), one(2.0)]), kind="value", what="rating 1e300")
    c.pair(USER, c.item(3.0, nb=[one(-1e300), one(2.0)]), kind="value", what="rating -1e300")
    c.pair(USER, c.item(3.0, nb=[one(4.0, sim=0.0), one(1.0, sim=-0.0), one(5.0, sim=0.0)]), kind="value", what="all sims zero")
    c.pair(USER, c.item(3.0, nb=[one(4.0, sim=0.0), one(1.0 / 3.0, sim=-2.0 / 7.0)]), kind="value", what="one sim zero")
    c.pair(USER, c.item(3.0, nb=[one(4.0, navg=np.inf), one(2.0)]), kind="value", what="neighbour average inf")
    c.pair(25, c.item(3.0, nb=[one(4.0, navg=np.inf), one(2.0)]), kind="value", what="neighbour average inf, not held")
    c.pair(USER, c.item(3.0, nb=[one(2.0), one(np.nan)]), kind="value", what="rating nan")
    c.pair(USER, c.item(np.nan, nb=[one(2.0)]), kind="value", what="average nan with evidence")
    for a in (c.avg, c.nb, c.rt, c.pairs, c.tags):
        assert isinstance(a, list)
    return c


class Arrays(object):
    pass


@functools.lru_cache(maxsize=None)
def arrays():
    """what xmap_predict takes: tu, ti [N_TEST] (the pairs repeated in turn), the neighbour lists and the raters as CSR
    by item, the item averages; `pair_of` [N_TEST]: the designed pair of every test pair"""
    c = case()
    I = len(c.avg)
    A = Arrays()
    A.n_items = I
    assert len(c.pairs) < N_TEST and N_TEST % 128 == 1
    A.pair_of = np.arange(N_TEST) % len(c.pairs)
    A.tu = np.asarray([c.pairs[p][0] for p in A.pair_of], np.int32)
    A.ti = np.asarray([c.pairs[p][1] for p in A.pair_of], np.int32)
    A.nb_ptr = np.zeros(I + 1, np.int64)
    np.cumsum([len(l) for l in c.nb], out=A.nb_ptr[1:])
    A.nb_item = np.asarray([n for l in c.nb for n, _ in l], np.int32)
    A.nb_sim = np.asarray([s for l in c.nb for _, s in l], np.float64)
    A.rt_ptr = np.zeros(I + 1, np.int64)
    np.cumsum([len(l) for l in c.rt], out=A.rt_ptr[1:])
    A.rt_user = np.asarray([u for l in c.rt for u, _, _ in l], np.int32)
    A.rt_rating = np.asarray([r for l in c.rt for _, r, _ in l], np.float64)
    A.rt_time = np.asarray([t for l in c.rt for _, _, t in l], np.float64)
    A.avg = np.asarray(c.avg, np.float64)
    assert A.nb_item.min() >= 0 and A.nb_item.max() < I
    for i in range(I):
        assert np.all(np.diff(A.rt_user[A.rt_ptr[i]:A.rt_ptr[i + 1]]) >= 0)      # the kernel searches a row by bisection
    for a in vars(A).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return A


def wtab(alpha, n_w):
    """the decay table as RecommenderPrediction._device_recommendation makes it: scalar np.exp calls, like the reference's"""
    return np.asarray([np.exp(- alpha * d) for d in range(n_w)], np.float64)


class _B(object):
    def __init__(self, value):
        self.value = value


@functools.lru_cache(maxsize=None)
def dictionaries():
    """(rating_bd, sim_bd, item_bd) of RecommenderPrediction._predict_pair, from the ARRAYS: every item has a list (it may be
    empty), its raters in row order, Python floats throughout"""
    A = arrays()
    ratings, sims, info = {}, {}, {}
    for i in range(A.n_items):
        lo, hi = int(A.rt_ptr[i]), int(A.rt_ptr[i + 1])
        ratings[iname(i)] = [(uname(int(A.rt_user[p])), float(A.rt_rating[p]), float(A.rt_time[p])) for p in range(lo, hi)]
        lo, hi = int(A.nb_ptr[i]), int(A.nb_ptr[i + 1])
        sims[iname(i)] = [(iname(int(A.nb_item[p])), float(A.nb_sim[p])) for p in range(lo, hi)]
        info[iname(i)] = (float(A.avg[i]), 0.0, 0)
    return _B(ratings), _B(sims), _B(info)


def evidence_of(p):
    """the evidence list of designed pair p as _predict_pair gathers it: (sim * (rating - neighbour average), |sim|, time)*"""
    c = case()
    u, it = c.pairs[p]
    if it < 0:
        return []
    rating_bd, sim_bd, item_bd = dictionaries()
    out = []
    for niid, nsim in sim_bd.value[iname(it)]:
        navg = item_bd.value[niid][0]
        for rater, rating, when in rating_bd.value[niid]:
            if uname(u) in rater:
                out.append((nsim * (rating - navg), abs(nsim), when))
    return out


@functools.lru_cache(maxsize=None)
def designed_statement(alpha):
    """per designed pair (status before the n_w rule, plain, decay, n): _predict_pair itself, its raises made status 2"""
    from xmap.core.recommenderPrediction import RecommenderPrediction
    c = case()
    tool = RecommenderPrediction(alpha, "cosine")
    bds = dictionaries()
    out = []
    for p, (u, it) in enumerate(c.pairs):
        n = len(evidence_of(p))
        try:
            with np.errstate(all="ignore"):
                got = tool._predict_pair(uname(u), (iname(it), 0.0), *bds)
        except (ZeroDivisionError, ValueError, OverflowError):
            out.append((2, 0.0, 0.0, n))
            continue
        if got == ():
            out.append((1, 0.0, 0.0, n))
        elif got[2] != got[2] or got[3] != got[3]:
            out.append((2, 0.0, 0.0, n))
        else:
            assert got[:2] == (iname(it), 0.0)
            out.append((0, float(got[2]), float(got[3]), n))
    return out


def expected(alpha, n_w):
    """(status int32, plain, decay) [N_TEST] for one call of xmap_predict"""
    A = arrays()
    rows = designed_statement(alpha)
    status = np.zeros(N_TEST, np.int32)
    plain, decay = np.zeros(N_TEST), np.zeros(N_TEST)
    for t, p in enumerate(A.pair_of):
        s, a, b, n = rows[p]
        if s != 1 and (n > PRED_EV or n + 1 > n_w):
            s, a, b = 2, 0.0, 0.0
        status[t], plain[t], decay[t] = s, a, b
    return status, plain, decay


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
