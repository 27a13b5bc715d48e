"""Designed inputs for RecommenderSim on the device (Engine.rec_sim / xmap_ctx_rec_sim: the LS instantiation of the pair kernels,
k_pair_tri<XMAP_ADJUST_COSINE, LOG_SLOTS, NW, LS = true> in csrc/tri_pairs.hip), a plain Python statement of one row of the
result, and the helpers the census needs.  No device and no torch: tests/test_cpu_rec_sim_rows.py takes the census of these
inputs and holds the CPU oracle to the statement, tests/test_gpu_rec_sim_rows.py uploads them.

The statement (rec_row_statement) follows reference core/recommenderSim.py:64-133 in index space for ONE item i: every
combinations() pair of a profile's rows that involves i, both orders (so a row paired with itself is listed twice per
unordered pair); inner product and squared norms with math.fsum over fp64 products -- the exact sum rounded once, DESIGN.md
section 2 -- and everything behind them in the reference's order of operations, in Python floats.  rec_rows_by_combinations is
the same thing written with itertools.combinations over whole profiles, for the small inputs: the two must agree.

Domain.  fsum is correctly rounded; the oracle and the kernels sum in double-double, which is exact while the exact sum
fits the pair.  sum_bits(...) bounds, for every summed list of an input at once, (largest - smallest exponent of the non-zero
terms) + 53 + ceil(log2 n): the terms are products of two ratings, so their exponents span at most twice the span of the
ratings' plus one, and n is at most the longest list (the largest n_ij or rater count).  The census asserts <= 100.

Value families (small; every row is checked against the statement) -- value_family(name, cap):
  single           items with exactly one rater: n - 1 = 0 weights every leave-one-out variant by 0 and ls = |sim|.  The variant's
                   norm is sqrt((nx nx - r r) ny ny) with nx = fl(sqrt(fl(r r))); a negative difference would make it, and ls,
                   NaN.  It cannot be negative: fl(sqrt(fl(r r))) = |r| for every double whose square neither overflows nor
                   underflows, and in general a correctly rounded sum of squares is >= each of them and rounding is monotonic,
                   so nx nx - r r >= 0 for every rating of the item.  The census asserts the sign (zero for all sixty values,
                   thirds, sevenths, tenths and eighths) and that no ls is NaN
  nan_rating       the only way to a NaN: a rating that is one.  Every pair of the item that holds it has sim = ls = NaN (NaN
                   ranks above every distance in the slot's running maximum), the pairs beside it in the same profiles are
                   untouched
  cap_edges        pairs with n_ij in {1, 2, cap - 1, cap, cap + 1, 3 cap}: min(n, cap) and min(n - 1, cap) differ, agree and
                   both saturate; at cap = 1 every variant of an n = 1 pair is weighted by 0
  self_pairs       users holding an item 2, 3 and 4 times (1, 3, 6 unordered self pairs each); an item whose only pairs are with
                   itself; an item held twice by one user and once by others (the self pair beside ordinary pairs in one table);
                   repeats with equal and with different ratings
  signs_and_zeros  ratings of both signs; an inner product that cancels to exactly 0.0 and one that leaves a last-bit residue; an
                   all-zero item (norm 0, sim 0.0, both leave-one-out norms 0); +0.0 and -0.0 ratings; thirds and other values no
                   float32 holds
  slot_chains      one row of a single rater whose partners are chosen by the kernel's own hash: nine share one home slot of the
                   128-slot table, eight more sit at homes 126 and 127 so that their chain wraps to slot 0 -- the second walk's
                   lookup has to follow the chains

Layout families -- layout_family(name): the inputs of tests/test_cpu_stage_a_layout.py re-rated in fp64 ("<family>+fp64":
an integer rating r becomes r - 1/3, r + 0.125, ... by a rule on the entry), planned without a heavy set (ch_min = U + 2, as
Engine.rec_sim plans), and two more:
  wide_self        wide_counts+fp64 with one more item held three times by 33 000 users: its self pair is met 99 000 times
                   (beyond 16 bits) and reported as 198 000, beside the ordinary pair of the two hubs with 66 000 co-raters
  wide_repeat      2 100 users who hold every item of their profile twice, with different ratings; two hubs of 2 050 and 2 100
                   raters: the lighter hub is a class-4 row whose every rater holds the row's item twice, so the doubling of the
                   self pair and the 16-wave table are in one unit
"""
import functools
import itertools
import math

import numpy as np

NAN = float("nan")
CAPS = (1, 2, 50)
VALUE_FAMILIES = ("single", "cap_edges", "self_pairs", "signs_and_zeros", "slot_chains", "nan_rating")
LAYOUT_FAMILIES = ("fill+fp64", "wide_few+fp64", "wide_many+fp64", "wide_counts+fp64", "overflowing+fp64", "full_heavy:chunks+fp64",
                   "wide_self", "wide_repeat")
SMALL_TARGET = 24          # a slot target that cuts rows into many hash partitions
SUM_BITS_MAX = 100         # what a double-double sum holds with room to spare (2 x 53 bits)
# ratings for the value families: thirds, sevenths, decimals, eighths -- most of them no float32 holds
VALUES = (1.0 / 3.0, 2.0 / 3.0, 1.125, 1.7, 2.1, 7.0 / 3.0, 2.875, 3.3, 11.0 / 3.0, 4.2, 4.9, 5.0, 0.1, 13.0 / 7.0, 2.5)
FP64_OFFSETS = (-1.0 / 3.0, 0.125, 1.0 / 3.0, -0.3, 0.0, 0.7, -0.125)


class Input(object):
    """user-major profiles: user_ptr [U + 1], item [nnz], rating fp64 [nnz] (read-only), n_items; anything else in `meta`"""

    def __init__(self, user_ptr, item, rating, n_items, **meta):
        self.user_ptr = np.ascontiguousarray(user_ptr, np.int64)
        self.item = np.ascontiguousarray(item, np.int32)
        self.rating = np.ascontiguousarray(rating, np.float64)
        self.n_items, self.n_users, self.nnz = int(n_items), len(self.user_ptr) - 1, len(self.item)
        assert self.user_ptr[0] == 0 and self.user_ptr[-1] == self.nnz == len(self.rating)
        assert self.nnz == 0 or (0 <= self.item.min() and self.item.max() < self.n_items)
        self.time = np.zeros(self.nnz, np.int64)
        self.meta = meta
        for a in (self.user_ptr, self.item, self.rating, self.time):
            a.setflags(write=False)

    def item_attrs(self):
        """every item a target item of one domain (RecommenderSim reads none of this)"""
        I = self.n_items
        return np.zeros(I, np.int32), np.zeros(I, np.int32), np.full(I, 1, np.uint32), np.full(I, 2, np.uint8)


def from_profiles(profiles, n_items, **meta):
    """profiles: per user a list of (item, rating)"""
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in profiles])]).astype(np.int64)
    flat = [x for p in profiles for x in p]
    return Input(ptr, [x[0] for x in flat], [x[1] for x in flat], n_items, **meta)


def shuffled(r, seed):
    """the same ratings with the users permuted and the entries of every profile permuted"""
    rng = np.random.default_rng(seed)
    d = np.diff(r.user_ptr)
    order = rng.permutation(r.n_users)
    users = np.repeat(np.arange(r.n_users), d)
    place = np.empty(r.n_users, np.int64)
    place[order] = np.arange(r.n_users)
    o = np.lexsort((rng.random(r.nnz), place[users]))
    ptr = np.concatenate([[0], np.cumsum(d[order])]).astype(np.int64)
    return Input(ptr, r.item[o], r.rating[o], r.n_items)


# ------------------------------------------------------------------------------------------------------ the statement
def rec_norms_statement(item, rating, n_items):
    """sqrt(fsum(r r)) per item"""
    sq = [[] for _ in range(int(n_items))]
    for j, r in zip(np.asarray(item).tolist(), np.asarray(rating, np.float64).tolist()):
        sq[j].append(r * r)
    return [math.sqrt(math.fsum(s)) for s in sq]


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN            # np.sqrt of a negative number (or of NaN): NaN


def _cosine(dot, norms):
    return 1.0 * dot / norms if norms else 0.0          # NaN is truthy: it divides


def _weighting(sim, count, cap):
    return 1.0 * sim * min(count, cap) / cap


def _pair_statement(rec, nx, ny, cap):
    """(sim, ls, n) of one directed pair from its records [(r0, r1)*]: recommenderSim.py:98-132"""
    n = len(rec)
    inner = math.fsum(r0 * r1 for r0, r1 in rec)
    sim = _weighting(_cosine(inner, nx * ny), n, cap)
    ls, nan = 0.0, False
    for r0, r1 in rec:
        m_inner = inner - r0 * r1
        m1 = _sqrt((nx * nx - r0 * r0) * (ny * ny))
        m2 = _sqrt((nx * nx) * (ny * ny - r1 * r1))
        for m in (m1, m2):
            d = abs(_weighting(_cosine(m_inner, m), n - 1, cap) - sim)
            if d != d:
                nan = True                              # max() of an array that holds a NaN is NaN
            elif d > ls:
                ls = d
    return sim, (NAN if nan else ls), n


def pair_records(ptr, item, rating, i):
    """{j: [(r_i, r_j)*]}: every combinations() pair of a profile's rows that involves item i, both orders -- per entry a that
    holds i, every OTHER entry b of the same profile gives (r_a, r_b) under item(b); two entries that both hold i meet twice"""
    ptr, item = np.asarray(ptr, np.int64), np.asarray(item)
    rating = np.asarray(rating, np.float64)
    out = {}
    entries = np.nonzero(item[:ptr[-1]] == i)[0]
    users = np.searchsorted(ptr, entries, side="right") - 1
    for a, u in zip(entries.tolist(), users.tolist()):
        lo, hi = int(ptr[u]), int(ptr[u + 1])
        if hi - lo < 2:
            continue
        r0 = float(rating[a])
        its, rs = item[lo:hi].tolist(), rating[lo:hi].tolist()
        for k in range(hi - lo):
            if lo + k != a:
                out.setdefault(its[k], []).append((r0, rs[k]))
    return out


def rec_row_statement(ptr, item, rating, norms, i, cap):
    """{j: (sim, ls, n_ij)}: the row of item i"""
    rec = pair_records(ptr, item, rating, i)
    return {j: _pair_statement(rec[j], norms[i], norms[j], cap) for j in rec}


def rec_rows_by_combinations(ptr, item, rating, norms, cap):
    """{(i, j): (sim, ls, n_ij)} of a whole (small) input, written as produce_pairwise writes it: recommenderSim.py:64-75"""
    ptr, item, rating = np.asarray(ptr).tolist(), np.asarray(item).tolist(), np.asarray(rating, np.float64).tolist()
    pairs = {}
    for u in range(len(ptr) - 1):
        ratings = [(item[e], rating[e]) for e in range(ptr[u], ptr[u + 1])]
        if len(ratings) < 2:
            continue
        for x1, x2 in itertools.combinations(ratings, 2):
            pairs.setdefault((x1[0], x2[0]), []).append((x1[1], x2[1]))
            pairs.setdefault((x2[0], x1[0]), []).append((x2[1], x1[1]))
    return {k: _pair_statement(rec, norms[k[0]], norms[k[1]], cap) for k, rec in pairs.items()}


# ------------------------------------------------------------------------------------------------- comparing doubles
def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_doubles(a, b):
    """equal as bit patterns, every NaN equal to every NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def row_of(row_ptr, col, sim, ls, nij, i):
    """row i of a CSR result (columns ascending) as the statement's dictionary"""
    a, b = int(row_ptr[i]), int(row_ptr[i + 1])
    return {int(j): (float(s), float(l), int(n)) for j, s, l, n in zip(col[a:b], sim[a:b], ls[a:b], nij[a:b])}


def same_row(got, want):
    """two rows {j: (sim, ls, n)}: the same columns and counts, sim and ls bit for bit (NaN = NaN)"""
    if sorted(got) != sorted(want):
        return False
    keys = sorted(want)
    return ([got[j][2] for j in keys] == [want[j][2] for j in keys] and same_doubles([got[j][0] for j in keys], [want[j][0] for j in keys])
            and same_doubles([got[j][1] for j in keys], [want[j][1] for j in keys]))


def sum_bits(rating, longest):
    """an upper bound, for every list of products of two ratings of up to `longest` terms, of
    (largest - smallest exponent of the non-zero terms) + 53 + ceil(log2 n)"""
    a = np.abs(np.asarray(rating, np.float64))
    a = a[(a != 0.0) & ~np.isnan(a)]          # (nan_rating: a NaN term makes the sum NaN in any arithmetic)
    if len(a) == 0:
        return 0
    assert np.all(np.isfinite(a))
    e = np.frexp(a)[1]
    return 2 * int(e.max() - e.min()) + 1 + 53 + int(math.ceil(math.log2(max(int(longest), 1))))


def home_slot(j, log_slots):
    """the kernel's hash restated: ((uint32)j * 0x9E3779B1u) >> (32 - LOG_SLOTS)"""
    return ((int(j) * 0x9E3779B1) & 0xffffffff) >> (32 - log_slots)


def probe_slots(partners, log_slots):
    """{j: slot} after inserting the partners in the order given, linear probing (the set of taken slots does not depend on
    the order; which partner sits where does)"""
    taken, mask = {}, (1 << log_slots) - 1
    for j in partners:
        h = home_slot(j, log_slots)
        while h in taken:
            h = (h + 1) & mask
        taken[h] = j
    return {j: h for h, j in taken.items()}


def unordered_self_pairs(r):
    """per item the number of unordered pairs of entries of one profile that both hold it"""
    users = np.repeat(np.arange(r.n_users, dtype=np.int64), np.diff(r.user_ptr))
    key, k = np.unique(users * r.n_items + r.item, return_counts=True)
    out = np.zeros(r.n_items, np.int64)
    np.add.at(out, key % r.n_items, k * (k - 1) // 2)
    return out


# ------------------------------------------------------------------------------------------------------ value families
def single_sign(r):
    """the sign of fl(sqrt(fl(r r)))^2 - fl(r r): what decides the leave-one-out norm of a single-rater item"""
    nx = math.sqrt(math.fsum([r * r]))
    d = nx * nx - r * r
    return (d > 0) - (d < 0)


def _single():
    """60 single-rater items, three per user"""
    vals = [k / 3.0 for k in range(1, 16)] + [k / 7.0 for k in range(1, 16)] + [0.1 * k for k in range(1, 16)] + [k / 8.0 for k in range(1, 16)]
    order = np.random.default_rng(61).permutation(60)
    profiles = [[(int(q), vals[q]) for q in order[3 * u:3 * u + 3]] for u in range(20)]
    return from_profiles(profiles, 60, sign=[single_sign(v) for v in vals])


def _nan_rating():
    """item 0 holds a NaN among its four ratings; items 1 .. 5 are co-rated with it and with each other"""
    rng = np.random.default_rng(68)
    profiles = [[(0, NAN), (1, 2.1), (2, 1.0 / 3.0)], [(0, 3.3), (1, 4.9), (3, 1.7)], [(0, 2.5), (0, 1.125), (4, 4.2)]]
    for u in range(8):
        its = rng.choice(np.arange(1, 6), size=3, replace=False)
        profiles.append([(int(j), VALUES[int(rng.integers(len(VALUES)))]) for j in its])
    return from_profiles(profiles, 6)


def cap_targets(cap):
    return sorted(set(n for n in (1, 2, cap - 1, cap, cap + 1, 3 * cap) if n >= 1))


def _cap_edges(cap):
    """per target n two items that exactly the users 0 .. n - 1 hold: n_ij = n for the pair, min(n, m) across targets"""
    targets = cap_targets(cap)
    rng = np.random.default_rng(62 + cap)
    profiles = []
    for u in range(max(targets)):
        prof = []
        for t, n in enumerate(targets):
            if u < n:
                prof += [(2 * t, VALUES[int(rng.integers(len(VALUES)))]), (2 * t + 1, VALUES[int(rng.integers(len(VALUES)))])]
        profiles.append(prof)
    return from_profiles(profiles, 2 * len(targets), targets=targets)


def _self_pairs():
    third = 1.0 / 3.0
    profiles = [
        [(0, 2.5), (0, 2.5)],                                        # item 0: its only pairs are with itself; equal ratings
        [(0, third), (0, 1.7), (0, 4.2), (0, 2.875)],                # ... four times: 6 unordered pairs
        [(3, 1.125), (1, 2.1), (4, 3.3), (1, 2.1), (1, 11.0 / 3.0)], # item 1 three times (two equal ratings), beside 3 and 4
        [(2, 4.9), (3, third), (2, 4.9)],                            # item 2 twice by one user, equal ratings ...
    ] + [[(2, VALUES[q]), (3, VALUES[q + 1]), (4 + q % 2, VALUES[q + 2])] for q in range(6)] + [      # ... and once by six others
        [(5, 2.0 / 3.0), (4, 1.7), (5, 13.0 / 7.0)],                 # item 5 twice, different ratings
        [(6, 2.5)],                                                  # a profile of one rating: no pair
        [(6, 1.125), (6, 0.1), (5, 5.0)],
    ]
    return from_profiles(profiles, 8)                                # item 7 has no rater


def _signs_and_zeros():
    profiles = [
        # items 0, 1: 1.5 * 2.0 + (-3.0) * 1.0 = 0.0 exactly
        [(0, 1.5), (1, 2.0)], [(0, -3.0), (1, 1.0)],
        # items 2, 3: fl(0.1 * 3.0) - 0.3 = 2^-54: a last-bit residue
        [(2, 0.1), (3, 3.0)], [(2, -0.3), (3, 1.0)],
        # item 4: all zero (one of them -0.0), beside items 5 and 6
        [(4, 0.0), (5, 1.0 / 3.0), (6, -2.1)], [(4, -0.0), (5, -4.2), (6, 7.0 / 3.0)], [(4, 0.0), (5, 2.875)],
        # a +0.0 and a -0.0 rating inside items that are not zero
        [(5, 0.0), (6, -0.0), (7, 1.7)], [(5, -0.0), (7, -1.7), (6, 3.3)],
    ]
    rng = np.random.default_rng(63)
    signed = [v for v in VALUES] + [-v for v in VALUES]
    for u in range(24):                                              # both signs at random over items 5 .. 13
        its = rng.choice(np.arange(5, 14), size=int(rng.integers(2, 6)), replace=False)
        profiles.append([(int(j), signed[int(rng.integers(len(signed)))]) for j in its])
    return from_profiles(profiles, 14)


CHAIN_ITEMS = 2048         # index space of slot_chains: 16 items per home slot of a 128-slot table to choose from
CHAIN_LOG_SLOTS = 7


def _slot_chains():
    """item 0 has one rater, who also holds: nine items of one home slot, three of home 126 and five of home 127.  Item 0
    is the lightest item (one rater, the lowest index), so all seventeen are partners in ITS table: 128 slots (bound 17)."""
    by_home = {}
    for j in range(1, CHAIN_ITEMS):
        by_home.setdefault(home_slot(j, CHAIN_LOG_SLOTS), []).append(j)
    crowded = by_home[min(h for h, v in by_home.items() if 32 <= h < 100 and len(v) >= 9)][:9]     # (clear of the wrapped chain)
    tail = by_home[126][:3] + by_home[127][:5]
    partners = crowded + tail
    rng = np.random.default_rng(64)
    val = lambda: VALUES[int(rng.integers(len(VALUES)))]
    profiles = [[(0, 13.0 / 7.0)] + [(j, val()) for j in partners]]
    for u in range(6):                                               # other raters of the partners: different counts
        its = rng.choice(partners, size=5 + u, replace=False)
        profiles.append([(int(j), val()) for j in its])
    order = rng.permutation(len(profiles[0]))
    profiles[0] = [profiles[0][q] for q in order]
    return from_profiles(profiles, CHAIN_ITEMS, partners=partners, crowded=crowded, tail=tail)


@functools.lru_cache(maxsize=None)
def value_family(name, cap=50):
    """the input of a value family; only cap_edges depends on the cap"""
    if name == "cap_edges":
        return _cap_edges(cap)
    return dict(single=_single, nan_rating=_nan_rating, self_pairs=_self_pairs, signs_and_zeros=_signs_and_zeros, slot_chains=_slot_chains)[name]()


# ----------------------------------------------------------------------------------------------------- layout families
def fp64_ratings(item, rating):
    """the "+fp64" rule: entry e, of item j, gets rating + FP64_OFFSETS[(3 e + j) mod 7]: thirds, tenths and eighths"""
    e = np.arange(len(item), dtype=np.int64)
    off = np.asarray(FP64_OFFSETS)[(3 * e + np.asarray(item, np.int64)) % len(FP64_OFFSETS)]
    return np.asarray(rating, np.float64) + off


SELF_USERS = 33000         # wide_self: holders of the item held three times
REPEAT_USERS, REPEAT_HUBS = 2100, (2050, 2100)


def _wide_self():
    from test_cpu_stage_a_layout import family, wide_counts
    r = family("wide_counts")
    X = r.n_items                                                    # the new item
    users = np.repeat(np.arange(r.n_users, dtype=np.int64), np.diff(r.user_ptr))
    add_u = np.repeat(np.arange(SELF_USERS, dtype=np.int64), 3)
    add_r = np.tile(np.asarray([2.0 - 1.0 / 3.0, 3.125, 4.7]), SELF_USERS)
    u = np.concatenate([users, add_u])
    it = np.concatenate([r.item.astype(np.int64), np.full(len(add_u), X)])
    ra = np.concatenate([fp64_ratings(r.item, r.rating), add_r])
    o = np.lexsort((np.random.default_rng(65).random(len(u)), u))    # the copies anywhere in the profile
    ptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=r.n_users))]).astype(np.int64)
    return Input(ptr, it[o], ra[o], X + 1, self_item=X, hubs=tuple(i for i, _ in wide_counts()[1]))


@functools.lru_cache(maxsize=None)
def repeat_parts():
    """wide_repeat before the repetition: (user_ptr, item, first ratings, second ratings, hubs) -- every user holds the hub H1,
    the first 2 050 also H0, and two of sixty light items, each once"""
    rng = np.random.default_rng(66)
    U, n_light = REPEAT_USERS, 60
    H0, H1 = n_light, n_light + 1                                    # the hubs behind the light items
    ptr, item, ra, rb = [0], [], [], []
    for u in range(U):
        its = [H1] + ([H0] if u < REPEAT_HUBS[0] else []) + [int(j) for j in rng.choice(n_light, size=2, replace=False)]
        first = [float(rng.integers(1, 6)) for _ in its]
        item += its
        ra += first
        rb += [r + FP64_OFFSETS[(u + j) % 4] for j, r in zip(its, first)]         # (the first four offsets: none is zero)
        ptr.append(len(item))
    return np.asarray(ptr, np.int64), np.asarray(item, np.int32), np.asarray(ra), np.asarray(rb), (H0, H1)


def _wide_repeat():
    ptr, item, ra, rb, hubs = repeat_parts()
    users = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    u, it, r = np.concatenate([users, users]), np.concatenate([item, item]), np.concatenate([ra, rb])
    o = np.lexsort((np.random.default_rng(69).random(len(u)), u))    # the two copies anywhere in the profile
    return Input(2 * ptr, it[o], r[o], int(item.max()) + 1, hubs=hubs)


@functools.lru_cache(maxsize=None)
def layout_family(name):
    if name == "wide_self":
        return _wide_self()
    if name == "wide_repeat":
        return _wide_repeat()
    assert name.endswith("+fp64")
    from test_cpu_stage_a_layout import family
    r = family(name[:-len("+fp64")])
    return Input(r.user_ptr, r.item, fp64_ratings(r.item, r.rating), r.n_items)


@functools.lru_cache(maxsize=None)
def rec_plan(name, slot_target):
    """the plan Engine.rec_sim makes of a layout family, stated: no heavy set (ch_min above every rater count), duplicates"""
    from test_cpu_stage_a_layout import plan_statement
    r = layout_family(name)
    return plan_statement(r.user_ptr, r.item, r.n_items, r.n_users + 2, slot_target, dups=True)


def chosen_rows(name, n_random=16):
    """the rows of a layout family that are held to the statement: per table class the rows of the smallest and the largest
    partner bound, the hubs (2 048 entries and more; the three lightest and the three heaviest), the rows paired with themselves (up to four, the most repeated first)
    and n_random rows with work drawn with a fixed seed"""
    r, P = layout_family(name), rec_plan(name, 768)
    rows = []
    for c in range(5):
        of = np.nonzero((P.cls == c) & (P.Q >= 1))[0]
        if len(of):
            rows += [int(of[np.argmin(P.bound[of])]), int(of[np.argmax(P.bound[of])])]
    hubs = np.nonzero(P.n >= 2048)[0]
    hubs = hubs[np.argsort(P.n[hubs], kind="stable")]
    rows += hubs[:3].tolist() + hubs[-3:].tolist()                   # (wide_many has 48 of them: the lightest and the heaviest)
    selfs = unordered_self_pairs(r)
    rows += [int(i) for i in np.argsort(-selfs, kind="stable")[:4] if selfs[i] > 0]
    work = np.nonzero(P.n > 0)[0]
    rng = np.random.default_rng(67 + LAYOUT_FAMILIES.index(name))
    rows += rng.choice(work, size=min(n_random, len(work)), replace=False).tolist()
    return sorted(set(rows))


# -------------------------------------------------------------------------------------------------------- the oracle
class OracleRows(object):
    pass


def oracle_rec(r, cap):
    """the CPU oracle's RecommenderSim of an input, as NumPy arrays (rows: the row of every pair; columns ascending)"""
    from oracle import xmap_oracle as xo
    R = xo.rec_sim(r.user_ptr, r.item, r.rating, r.n_items, cap)
    O = OracleRows()
    O.row_ptr, O.col, O.sim, O.ls, O.nij, O.norm = R.row_ptr, R.col, R.sim, R.ls, R.nij, R.norm
    O.rows = np.repeat(np.arange(r.n_items, dtype=np.int64), np.diff(R.row_ptr))
    xo.rec_free(R)
    return O


@functools.lru_cache(maxsize=None)
def oracle_value(name, cap):
    return oracle_rec(value_family(name, cap), cap)


@functools.lru_cache(maxsize=2)        # (the largest result, overflowing+fp64, holds 7.8 million pairs: not kept for the session)
def oracle_layout(name, cap=50):
    return oracle_rec(layout_family(name), cap)


@functools.lru_cache(maxsize=None)
def norms_of(kind, name, cap=50):
    r = value_family(name, cap) if kind == "value" else layout_family(name)
    return rec_norms_statement(r.item, r.rating, r.n_items)
