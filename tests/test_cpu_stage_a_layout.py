"""Designed inputs for the layout and the plan of stage A (csrc/tri_layout.hip, tri_pairs.hip, tri_mirror.hip): the builders
tests/test_gpu_stage_a_layout.py imports, a plain NumPy statement of the plan (heavy threshold, heavy set, W+, partner bound,
partitions, chunks and table class of every row: DESIGN.md §4, "Stage A"), and the conditions these inputs have to meet on
the statement's and on the CPU oracle's side before a comparison with the GPU says anything about the kernels they aim at.

The plan in words.  n_i = raters of item i.  Items are ordered by weight (n, index); a rater of i contributes the prefix of its
profile in front of i, i.e. its heavier items, so W+_i = sum over the raters of i (profiles of at least two ratings) of the
number of heavier items in the rater's profile.  CH = the least v >= ch_min with #{n > v} <= 1024; the heavy set is n > CH (it
gets dense ids below 1024 and is summed in chunks of CH raters: C = ceil(n / CH)); every other row with W+ > 0 is light and
cut into Q = ceil(bound / slot_target) hash partitions, bound = min(W+, #{n' >= n} - 1 (+ 1 where a profile may hold an item
twice)) bounding the row's distinct partners.  A light row goes to an LDS table class: 4 (16 waves on one 1024-slot table)
with n >= 2048 raters; else 0 (1024 slots) unless Q == 1; else by bound: 1 (128 slots) up to 96, 3 (256) up to 192, 2 (512)
up to 384, else 0.  The light units are listed class-major in the order 4, 0, 2, 3, 1.

Families (every census figure asserted below was derived with plan_statement and is written next to its input):

  wide_few     eight hub items with 2 047 .. U raters: the only light rows of 2 048 raters and more that the suite plans at
               the default threshold, with at most seven partners each -- 1 024 lanes on a handful of slots
  wide_many    24 hubs per domain with distinct counts from 2 048: 47 class-4 rows, 15 of them cut into two partitions at
               slot_target = 32, or 47 heavy rows next to one class-4 row at the default threshold
  full_heavy   rater counts designed around ch_min = 64: a full heavy set (all 1 024 dense ids), 1 025 candidates with a tie
               run at the threshold (CH rises), heavy rows of m CH and m CH + 1 raters
  wide_counts  66 000 users who all rate two hubs, planned without a heavy set: one slot of a class-4 table counts 66 000
               co-raters, more than a 16-bit half of the count word holds
  fill         rows with exactly 96, 97, 192, 193, 384, 385, 768 and 769 distinct partners (both sides of every class edge, every
               table at its design load), profiles on the edges of the profile sort, rater counts on the walk's block edges
"""
import functools

import numpy as np
import pytest

HMAX = 1024               # dense ids of the heavy set
WIDE_MIN = 2048           # light rows with at least this many raters: class 4
NO_HEAVY = 0x7f7f7f7f     # the CH word where no threshold was searched (ch_min above every possible rater count)
CLASS_ORDER = (4, 0, 2, 3, 1)      # the light units are listed class-major in this order
CAP = 50
METHODS = ("cosine", "adjust_cosine")


class Plan(object):
    pass


def plan_statement(user_ptr, item, n_items, ch_min, slot_target, dups=False):
    """The plan of stage A as the module docstring states it, in NumPy.  Returns a Plan: n, CH, heavy (mask), n_heavy, Wp,
    bound, Q, C, cls (per item), units (light units per class in CLASS_ORDER), cls_ptr (their running sum, 6 entries),
    n_light, n_heavy_units."""
    user_ptr = np.asarray(user_ptr, np.int64)
    item = np.asarray(item, np.int64)
    I, U = int(n_items), len(user_ptr) - 1
    P = Plan()
    n = np.bincount(item, minlength=I).astype(np.int64)
    # CH: v runs from ch_min to U (no item has more than U raters, so v = U always qualifies)
    CH = NO_HEAVY
    if ch_min <= U:
        above = I - np.searchsorted(np.sort(n), np.arange(ch_min, U + 1), side="right")        # #{n > v}
        CH = int(ch_min + np.nonzero(above <= HMAX)[0][0])
    heavy = n > CH
    # W+: position of every entry in its profile sorted heaviest first (copies of an item: in any order, the sum is the same)
    d = np.diff(user_ptr)
    users = np.repeat(np.arange(U, dtype=np.int64), d)
    weight = n[item] * I + item
    o = np.lexsort((-weight, users))
    pos = np.arange(len(item), dtype=np.int64) - user_ptr[users[o]]
    pos[d[users[o]] < 2] = 0
    Wp = np.zeros(I, np.int64)
    np.add.at(Wp, item[o], pos)
    ge = I - np.searchsorted(np.sort(n), n, side="left")                                        # #{n' >= n}
    bound = np.minimum(Wp, ge - 1 + (1 if dups else 0))
    work = Wp > 0
    Q = np.where(work & ~heavy, -(-bound // slot_target), 0)
    C = np.where(work & heavy, -(-n // CH), 0)
    by_bound = np.where(bound <= 96, 1, np.where(bound <= 192, 3, np.where(bound <= 384, 2, 0)))
    cls = np.where((Q >= 1) & (n >= WIDE_MIN), 4, np.where(Q != 1, 0, by_bound))
    P.n, P.CH, P.heavy, P.n_heavy, P.Wp, P.bound, P.Q, P.C, P.cls = n, CH, heavy, int(heavy.sum()), Wp, bound, Q, C, cls
    P.units = np.array([int(Q[cls == c].sum()) for c in CLASS_ORDER], np.int64)
    P.cls_ptr = np.concatenate([[0], np.cumsum(P.units)])
    P.n_light, P.n_heavy_units = int(Q.sum()), int(C.sum())
    return P


def census(P):
    """the figures written next to the inputs: CH, heavy rows and units, rows and units of every class, partitions"""
    rows = {c: int(((P.cls == c) & (P.Q >= 1)).sum()) for c in CLASS_ORDER}
    return dict(CH=P.CH, n_heavy=P.n_heavy, heavy_units=P.n_heavy_units, rows=rows, units=dict(zip(CLASS_ORDER, P.units.tolist())),
                wide_split=int(((P.cls == 4) & (P.Q > 1)).sum()), max_Q=int(P.Q.max()))


# ------------------------------------------------------------------------------------------------------------ builders
def _extended(r, add_user, add_item, rng, n_new_users=0, n_new_items=0):
    """r with the entries (add_user, add_item) appended to their users' profiles (in the order given), integer ratings 1..5
    and times drawn from rng; new users get the indices behind the last one, new items the last indices of the target domain"""
    from xmap.engine import synth
    add_user, add_item = np.asarray(add_user, np.int64), np.asarray(add_item, np.int64)
    U = r.n_users + n_new_users
    users = np.concatenate([np.repeat(np.arange(r.n_users, dtype=np.int64), np.diff(r.user_ptr)), add_user])
    o = np.argsort(users, kind="stable")
    k = len(add_user)
    item = np.concatenate([r.item, add_item.astype(np.int32)])[o]
    rating = np.concatenate([r.rating, rng.integers(1, 6, size=k).astype(np.float32)])[o]
    time = np.concatenate([r.time, rng.integers(synth.T0, synth.T1 + 1, size=k, dtype=np.int64)])[o]
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(np.bincount(users, minlength=U), out=ptr[1:])
    top = int(r.tgt_numbers.max()) if len(r.tgt_numbers) else 0
    tgt_numbers = np.concatenate([r.tgt_numbers, top + 1 + np.arange(n_new_items, dtype=r.tgt_numbers.dtype)])
    return synth.Ratings(ptr, item.astype(np.int32), rating, time, r.n_items + n_new_items, r.n_src_items, r.src_numbers, tgt_numbers)


def with_exact_raters(r, counts, seed):
    """r with every item of `counts` appended to randomly chosen users that lack it until it has exactly counts[item] raters
    (test_gpu_parity.hub_ratings, with a count)"""
    rng = np.random.default_rng(seed)
    users = np.repeat(np.arange(r.n_users, dtype=np.int64), np.diff(r.user_ptr))
    o = np.argsort(r.item, kind="stable")
    iptr = np.concatenate([[0], np.cumsum(np.bincount(r.item, minlength=r.n_items))])
    add_u, add_i = [], []
    for it in sorted(counts):
        have = users[o[iptr[it]:iptr[it + 1]]]
        need = counts[it] - len(have)
        assert need >= 0, "item %d has %d raters already, more than %d" % (it, len(have), counts[it])
        lacking = np.setdiff1d(np.arange(r.n_users, dtype=np.int64), have)
        add_u.append(rng.choice(lacking, need, replace=False))
        add_i.append(np.full(need, it, np.int64))
    out = _extended(r, np.concatenate(add_u), np.concatenate(add_i), rng)
    assert all(int(c) == counts[it] for it, c in zip(sorted(counts), np.bincount(out.item, minlength=out.n_items)[sorted(counts)]))
    return out


def _base41():
    from xmap.engine import synth
    return synth.make_two_domain(41, 4300, 1500, 1500, overlap=0.3)


def _quiet_items(r, lo, hi, k, below):
    """the first k items of [lo, hi) with fewer than `below` raters"""
    n = np.bincount(r.item, minlength=r.n_items)
    pick = lo + np.nonzero(n[lo:hi] < below)[0][:k]
    assert len(pick) == k
    return [int(x) for x in pick]


WIDE_FEW_SRC = (2048, 2049, 3072, 4300)       # 4300 = U: rated by every user
WIDE_FEW_TGT = (2047, 2048, 3073, 4300)


@functools.lru_cache(maxsize=None)
def wide_few():
    """-> (ratings, hubs): hubs[k] = (item, raters), the source hubs first"""
    r = _base41()
    assert r.n_users == 4300
    items = _quiet_items(r, 0, r.n_src_items, 4, 2000) + _quiet_items(r, r.n_src_items, r.n_items, 4, 2000)
    counts = dict(zip(items, WIDE_FEW_SRC + WIDE_FEW_TGT))
    return with_exact_raters(r, counts, 411), tuple(sorted(counts.items()))


@functools.lru_cache(maxsize=None)
def wide_many():
    r = _base41()
    items = _quiet_items(r, 0, r.n_src_items, 24, 2000) + _quiet_items(r, r.n_src_items, r.n_items, 24, 2000)
    counts = dict(zip(items, [2048 + 23 * t for t in range(24)] + [2050 + 23 * t for t in range(24)]))
    assert len(set(counts.values())) == 48
    return with_exact_raters(r, counts, 412), tuple(sorted(counts.items()))


FULL_HEAVY_CH_MIN = 64
FULL_HEAVY_VARIANTS = ("full", "ties", "chunks")
CHUNK_EDGES = (128, 129, 192, 193, 320, 321)       # m CH and m CH + 1 raters at CH = 64: the last chunk is whole / one rater


@functools.lru_cache(maxsize=None)
def full_heavy(variant):
    """Every item the base leaves at or below ch_min = 64 raters gets a designed count (about a thousand items), so that
    together with the 478 items the base has above it
      full    exactly 1 024 items have n > 64, the designed ones 65 .. 70 raters; the others exactly 64 or what they had
      ties    1 025 items have n > 64, twelve designed ones with exactly 65: CH rises to 65, past the whole run of ties
      chunks  `full` with six of the designed heavy rows at 128, 129, 192, 193, 320 and 321 raters
    -> (ratings, designed counts)"""
    from xmap.engine import synth
    r = synth.make_two_domain(43, 3000, 700, 700, overlap=0.4, mu=3.3, sigma=0.5)
    n = np.bincount(r.item, minlength=r.n_items)
    natural = int((n > FULL_HEAVY_CH_MIN).sum())
    low = np.nonzero(n <= FULL_HEAVY_CH_MIN)[0]
    want = (1025 if variant == "ties" else 1024) - natural
    assert 0 < want + 6 <= len(low)
    low = low[np.argsort(-n[low], kind="stable")]             # the fullest first: the fewest ratings to add
    counts = {}
    for q, it in enumerate(low[:want]):
        counts[int(it)] = 66 + q % 5 if variant == "ties" else 65 + q % 6
    if variant == "ties":
        for it in low[:12]:
            counts[int(it)] = 65
    if variant == "chunks":
        for it, c in zip(low[want - 6:want], CHUNK_EDGES):
            counts[int(it)] = c
    for it in low[want:want + 6]:                             # right at the threshold: n == ch_min is not heavy
        counts[int(it)] = FULL_HEAVY_CH_MIN
    return with_exact_raters(r, counts, 430 + FULL_HEAVY_VARIANTS.index(variant)), counts


FILL_L = (97, 98, 193, 194, 385, 386, 769, 770)             # profiles around the class edges: their lone item has L - 1 partners
FILL_SORT = (16, 17, 64, 65, 256, 257, 1024, 1025)          # edges of the profile sort
FILL_RATERS = (32, 33, 64, 65, 1024, 1025)                  # block edges of the walk over an item's raters
# (L, class, partitions, slots of the table) of the FILL_L rows at slot_target = 768
FILL_EXPECT = ((97, 1, 1, 128), (98, 3, 1, 256), (193, 3, 1, 256), (194, 2, 1, 512), (385, 2, 1, 512), (386, 0, 1, 1024),
               (769, 0, 1, 1024), (770, 0, 2, 1024))


@functools.lru_cache(maxsize=None)
def fill():
    """-> (ratings, lone[L] = the item only the profile of length L holds, sort_user[L], rater_item[count]).
    Six items of the base get exact rater counts first; then sixteen users are added whose profiles avoid those six items, so
    that counts and lengths are both exact.  A FILL_L profile is L - 1 base items (each of which has a rater in the base, so at
    least two now) and one new item: the new item is the lightest of the profile, W+ = L - 1, and as all items have a rater
    #{n' >= 1} - 1 = I - 1 > L - 1: bound = L - 1."""
    r = _base41()
    half = len(FILL_RATERS) // 2
    items = _quiet_items(r, 0, r.n_src_items, half, 32) + _quiet_items(r, r.n_src_items, r.n_items, half, 32)
    rater_item = dict(zip(FILL_RATERS, items))
    r = with_exact_raters(r, {it: c for c, it in rater_item.items()}, 413)
    rng = np.random.default_rng(414)
    pool = np.setdiff1d(np.arange(r.n_items), items)
    add_u, add_i, lone, sort_user = [], [], {}, {}
    for q, L in enumerate(FILL_L):
        u, new = r.n_users + q, r.n_items + q
        prof = np.concatenate([rng.choice(pool, L - 1, replace=False), [new]])
        rng.shuffle(prof)
        add_u.append(np.full(L, u)); add_i.append(prof)
        lone[L] = new
    for q, L in enumerate(FILL_SORT):
        u = r.n_users + len(FILL_L) + q
        add_u.append(np.full(L, u)); add_i.append(rng.choice(pool, L, replace=False))
        sort_user[L] = u
    out = _extended(r, np.concatenate(add_u), np.concatenate(add_i), rng, len(FILL_L) + len(FILL_SORT), len(FILL_L))
    return out, lone, sort_user, rater_item


OVERFLOW_L = 2049         # a profile whose lone item has 2 048 partners: two full 1 024-slot tables at slot_target = 1024


@functools.lru_cache(maxsize=None)
def overflowing():
    """The long-profiles input of test_gpu_parity (seed 21: profiles of up to 1 100 ratings, rows with bound near 3 000 but at most
    2 279 distinct partners, which no partition of a plan the entry points admit (slot_target <= 1024) overflows with) plus one
    user of OVERFLOW_L ratings built like a `fill` profile: its lone item has W+ = bound = 2 048 distinct partners, Q = 2 at
    slot_target = 1024, and so a partition of more than 1 024 partners unless the hash deals them exactly in half; at 512 its
    four partitions hold about 512 each.  -> (ratings, the lone item)"""
    from xmap.engine import synth
    r = synth.make_two_domain(21, 600, 1500, 1500, overlap=0.5, mu=4.0, sigma=1.6)
    rng = np.random.default_rng(415)
    prof = np.concatenate([rng.choice(r.n_items, OVERFLOW_L - 1, replace=False), [r.n_items]])
    rng.shuffle(prof)
    return _extended(r, np.full(OVERFLOW_L, r.n_users), prof, rng, 1, 1), r.n_items


COUNT_USERS = 66000       # more than 65 535: what a 16-bit half of a slot's count word could not hold


@functools.lru_cache(maxsize=None)
def wide_counts():
    """66 000 users with one or two ratings of the generator's (one per domain they are active in) and two hubs, one per domain,
    that every user rates: planned without a heavy set (ch_min above the user count, as the raw step of a user share and
    RecommenderSim plan), the lighter hub is a class-4 row whose slot for the other hub counts all 66 000 raters -- n_ij and the
    mutuality count of one slot both beyond 16 bits, which is why the class keeps them in 32-bit halves.  About 220 000 ratings.
    -> (ratings, hubs)"""
    from xmap.engine import synth
    r = synth.make_two_domain(45, COUNT_USERS, 1500, 1500, overlap=0.3, d_min=1, mu=-3.0, sigma=0.5)
    items = _quiet_items(r, 0, r.n_src_items, 1, 2000) + _quiet_items(r, r.n_src_items, r.n_items, 1, 2000)
    counts = {it: COUNT_USERS for it in items}
    return with_exact_raters(r, counts, 416), tuple(sorted(counts.items()))


def family(name):
    """ratings of a family by name: "wide_few", "wide_many", "wide_counts", "fill", "overflowing", "full_heavy:<variant>";
    "<name>+fractional": the same structure with synth.fractional's ratings"""
    if name.startswith("full_heavy:"):
        return full_heavy(name.split(":")[1])[0]
    if name.endswith("+fractional"):             # non-integer ratings: cosine mode takes the exact route on its own
        from xmap.engine import synth
        return synth.fractional(family(name[:-len("+fractional")]), seed=41)
    return dict(wide_few=wide_few, wide_many=wide_many, wide_counts=wide_counts, fill=fill, overflowing=overflowing)[name]()[0]


# (family, ch_min, slot_target): every plan the GPU tests run, with the census plan_statement gives for it: CH, heavy rows, heavy
# units (chunks), class-4 rows, class-4 rows cut into more than one partition, the most partitions of a row, and the light rows
# and light units of every class in CLASS_ORDER (4, 0, 2, 3, 1).  Inputs: wide_few 4 300 users, 2 987 items, 65 472 ratings;
# wide_many 153 200 ratings; full_heavy 3 000 users, 1 400 items, 137 863 | 138 133 | 138 741 ratings; fill 4 316 users, 2 995
# items, 50 434 ratings; wide_counts 66 000 users, 2 999 items, 217 831 ratings.
def _census(CH, n_heavy, heavy_units, wide, wide_split, max_Q, rows, units):
    return dict(CH=CH, n_heavy=n_heavy, heavy_units=heavy_units, wide=wide, wide_split=wide_split, max_Q=max_Q, rows=rows, units=units)


_FEW, _MANY = (0, 417, 1204, 1359), (496, 1285, 838, 320)
RUNS = [
    # the heavy rows are the five hubs above 2 048 raters; the heavier of the two all-user hubs has no heavier partner and so no
    # work: 2 + 2 + 2 + 3 chunks.  The two hubs of exactly 2 048 raters are light and class 4, the one of 2 047 is not.
    ("wide_few", 2048, 768, _census(2048, 5, 9, 2, 0, 1, (2,) + _FEW, (2,) + _FEW)),
    ("wide_few", 4096, 768, _census(4096, 2, 2, 5, 0, 1, (5,) + _FEW, (5,) + _FEW)),
    # ch_min above the user count: no threshold is searched, no heavy set
    ("wide_few", 8192, 768, _census(NO_HEAVY, 0, 0, 6, 0, 1, (6,) + _FEW, (6,) + _FEW)),
    ("wide_many", 4096, 768, _census(4096, 0, 0, 47, 0, 1, (47,) + _MANY, (47,) + _MANY)),
    # the 15 lightest hubs have 33 .. 47 heavier hubs: two partitions each; the base's rows are cut into up to 18
    ("wide_many", 4096, 32, _census(4096, 0, 0, 47, 15, 18, (47, 2910, 0, 0, 29), (62, 23838, 0, 0, 29))),
    ("wide_many", 2048, 768, _census(2048, 47, 92, 1, 0, 1, (1,) + _MANY, (1,) + _MANY)),
    # no heavy set (ch_min above the 66 000 users).  Class 4: the lighter all-user hub (one partner: the other hub, 66 000
    # co-raters in one slot) and two popular items of the base (2 524 and 2 533 raters, the hubs and each other as partners)
    ("wide_counts", 1 << 17, 768, _census(NO_HEAVY, 0, 0, 3, 0, 1, (3, 0, 0, 234, 2761), (3, 0, 0, 234, 2761))),
    ("full_heavy:full", 64, 768, _census(64, 1024, 2746, 0, 0, 2, (0, 376, 0, 0, 0), (0, 752, 0, 0, 0))),
    ("full_heavy:ties", 64, 768, _census(65, 1006, 2699, 0, 0, 2, (0, 394, 0, 0, 0), (0, 788, 0, 0, 0))),
    ("full_heavy:chunks", 64, 768, _census(64, 1024, 2757, 0, 0, 2, (0, 376, 0, 0, 0), (0, 752, 0, 0, 0))),
    ("fill", 2048, 768, _census(2048, 0, 0, 0, 0, 4, (0, 1954, 467, 259, 314), (0, 3446, 467, 259, 314))),
]
RUN_IDS = ["%s-%d-%d" % run[:3] for run in RUNS]


@functools.lru_cache(maxsize=None)
def plan_of(name, ch_min, slot_target):
    r = family(name)
    return plan_statement(r.user_ptr, r.item, r.n_items, ch_min, slot_target)


@functools.lru_cache(maxsize=None)
def oracle_sim(name, method):
    """the CPU oracle's stage A on a family, computed once and shared (never freed: a few MB)"""
    from oracle import xmap_oracle as xo
    r = family(name)
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
    return T, xo.item_sim(T, method, CAP, nthreads=8)


def oracle_rows(So):
    return np.repeat(np.arange(So.I, dtype=np.int64), np.diff(So.row_ptr))


def check_plan(S, r, ch_min, dups=False):
    """The plan behind a stage-A result of the engine (S.layout: device tensors, at the slot target the run ended with) against
    plan_statement, element for element.  r: anything with user_ptr, item and n_items; dups: profiles may hold an item twice
    (RecommenderSim over AlterEgo rows).  Used by the GPU tests; it runs nothing on the device itself."""
    L, I = S.layout, r.n_items
    P = plan_statement(r.user_ptr, r.item, I, ch_min, L.slot_target, dups)
    ctl = L.ctl.cpu().numpy()
    assert (int(ctl[0]), int(ctl[1])) == (P.CH, P.n_heavy) == (L.CH, L.n_heavy)
    assert np.array_equal(L.Wp.cpu().numpy()[:I], P.Wp)
    assert np.array_equal(L.Q.cpu().numpy()[:I], P.Q)
    assert np.array_equal(L.C.cpu().numpy()[:I], P.C)
    assert np.array_equal(L.small.cpu().numpy()[:I], P.cls)
    assert [int(x) for x in L.cls_ptr] == P.cls_ptr.tolist()
    assert (L.n_light, L.n_heavy_units) == (P.n_light, P.n_heavy_units)
    # the dense ids are handed out by atomics: any bijection between the heavy rows and 0 .. |H| - 1, hlist its inverse
    hid, hlist = L.hid.cpu().numpy()[:I], L.hlist.cpu().numpy()[:P.n_heavy]
    heavy = np.nonzero(P.heavy)[0]
    assert np.array_equal(hid >= 0, P.heavy)
    assert np.array_equal(np.sort(hid[heavy]), np.arange(P.n_heavy)) and np.array_equal(hlist[hid[heavy]], heavy)
    return P


# ------------------------------------------------------------------------------------------------------ the statement
def test_statement_on_a_hand_made_input():
    """three users, four items.  Profiles {0, 1, 2}, {1, 2}, {2, 3}: n = (1, 2, 3, 1); weights (n, index) descending:
    2, 1, 3, 0.  W+: item 2 leads every profile (0); item 1 follows item 2 twice (1 + 1); item 3 follows item 2 (1); item 0 is
    last of three (2).  #{n' >= n} - 1 = (3, 1, 0, 3), so bound = (2, 1, 0, 1)."""
    P = plan_statement([0, 3, 5, 7], [0, 1, 2, 1, 2, 2, 3], 4, 64, 1)
    assert P.n.tolist() == [1, 2, 3, 1] and P.CH == NO_HEAVY and P.n_heavy == 0
    assert P.Wp.tolist() == [2, 2, 0, 1] and P.bound.tolist() == [2, 1, 0, 1]
    assert P.Q.tolist() == [2, 1, 0, 1] and P.C.tolist() == [0, 0, 0, 0]
    assert P.cls.tolist() == [0, 1, 0, 1] and P.units.tolist() == [0, 2, 0, 0, 2] and P.cls_ptr.tolist() == [0, 0, 2, 2, 2, 4]
    # a profile of one rating contributes nothing; with duplicates a row may pair with itself: one more partner
    P = plan_statement([0, 1, 4], [2, 0, 1, 2], 3, 1, 768, dups=True)
    assert P.Wp.tolist() == [2, 1, 0] and P.bound.tolist() == [2, 1, 0]
    # a threshold: 3 users, ch_min = 1, item 2 has more than one rater -> CH = 1, one heavy row without work (it is the heaviest)
    assert P.CH == 1 and P.heavy.tolist() == [False, False, True] and P.C.tolist() == [0, 0, 0]


# --------------------------------------------------------------------------------------------------------- the census
@pytest.mark.parametrize("name,ch_min,slot_target,want", RUNS, ids=RUN_IDS)
def test_census(name, ch_min, slot_target, want):
    P = plan_of(name, ch_min, slot_target)
    c = census(P)
    got = dict(c, wide=c["rows"][4], rows=tuple(c["rows"][k] for k in CLASS_ORDER), units=tuple(c["units"][k] for k in CLASS_ORDER))
    assert got == want
    assert P.n_heavy <= HMAX and P.n_light == sum(want["units"]) and P.cls_ptr[-1] == P.n_light
    assert np.all(P.n[P.cls == 4] >= WIDE_MIN) and np.all(P.Q[P.cls == 4] >= 1)


def test_wide_few_hubs():
    """the hubs' own rows: which are heavy, which class 4, and that class 4 has a handful of partners"""
    r, hubs = wide_few()
    items = np.array([i for i, _ in hubs])
    assert sorted(c for _, c in hubs) == sorted(WIDE_FEW_SRC + WIDE_FEW_TGT) and r.n_users == 4300
    assert sum(i < r.n_src_items for i in items) == 4
    for ch_min, heavy_n, wide_n in ((2048, {2049, 3072, 3073, 4300}, {2048}), (4096, {4300}, {2048, 2049, 3072, 3073}),
                                    (8192, set(), {2048, 2049, 3072, 3073, 4300})):
        P = plan_of("wide_few", ch_min, 768)
        assert set(P.n[items[P.heavy[items]]].tolist()) == heavy_n
        assert set(P.n[items[P.cls[items] == 4]].tolist()) == wide_n
        assert np.array_equal(np.nonzero(P.cls == 4)[0], np.sort(items[P.cls[items] == 4]))      # no other row is class 4
        assert P.bound[P.cls == 4].max() <= 7 and P.Wp[P.cls == 4].min() >= 2048                # thousands of co-ratings on <= 7 slots
        low = items[P.n[items] == 2047]
        assert len(low) == 1 and P.cls[low[0]] != 4 and P.Q[low[0]] == 1
        # the heavier of the two all-user hubs is the heaviest item: nothing in front of it in any profile, no work
        top = items[P.n[items] == 4300].max()
        assert P.Wp[top] == 0 and P.Q[top] == 0 and P.C[top] == 0


def test_full_heavy_counts():
    r, counts = full_heavy("full")
    P = plan_of("full_heavy:full", 64, 768)
    assert int((P.n > 64).sum()) == 1024 and P.CH == 64 and P.n_heavy == 1024            # every dense id from 0 to 1023 is live
    assert int((P.n == 64).sum()) >= 6 and not P.heavy[P.n == 64].any()                  # n == CH is light
    assert int((P.C > 0).sum()) == 1023                                                  # all but the heaviest item have work
    r, counts = full_heavy("ties")
    P = plan_of("full_heavy:ties", 64, 768)
    ties = int((P.n == 65).sum())
    assert int((P.n > 64).sum()) == 1025 and ties == 19                                  # 12 designed, 7 of the base
    assert P.CH == 65 and P.n_heavy == 1025 - ties == 1006 and not P.heavy[P.n == 65].any()
    r, counts = full_heavy("chunks")
    P = plan_of("full_heavy:chunks", 64, 768)
    assert P.CH == 64 and P.n_heavy == 1024
    for c in CHUNK_EDGES:                        # m CH raters: m whole chunks; m CH + 1: the last chunk holds one rater
        rows = np.nonzero(P.n == c)[0]
        assert len(rows) >= 1 and np.all(P.heavy[rows]) and np.all(P.C[rows] == -(-c // 64)) and np.all(P.Wp[rows] > 0)
    assert sorted(P.C[[i for i, c in counts.items() if c in CHUNK_EDGES]].tolist()) == [2, 3, 3, 4, 5, 6]


def test_fill_rows():
    """class and load of the eight designed rows (FILL_EXPECT), the sort and walk edges"""
    r, lone, sort_user, rater_item = fill()
    P = plan_of("fill", 2048, 768)
    d = np.diff(r.user_ptr)
    users = np.repeat(np.arange(r.n_users), d)
    for L, cls, Q, slots in FILL_EXPECT:
        i = lone[L]
        u, = users[r.item == i]                   # its one rater
        assert P.n[i] == 1 and d[u] == L
        prof = r.item[r.user_ptr[u]:r.user_ptr[u + 1]]
        assert len(set(prof.tolist())) == L and P.n[prof[prof != i]].min() >= 2      # the lightest of its profile
        assert P.Wp[i] == L - 1 == P.bound[i] and P.Q[i] == Q and P.cls[i] == cls
        assert (L - 1) / Q <= 0.75 * slots + 0.5         # the design load of a table: three quarters (Q = 2: half of that)
    assert [int(d[sort_user[L]]) for L in FILL_SORT] == list(FILL_SORT)
    assert [int(P.n[rater_item[c]]) for c in FILL_RATERS] == list(FILL_RATERS)
    assert np.all(P.Wp[[rater_item[c] for c in FILL_RATERS]] > 0)


def test_overflowing_row():
    r, lone = overflowing()
    P = plan_statement(r.user_ptr, r.item, r.n_items, 2048, 1024)
    assert P.n[lone] == 1 and P.Wp[lone] == P.bound[lone] == 2048 and P.Q[lone] == 2 and P.cls[lone] == 0
    P = plan_statement(r.user_ptr, r.item, r.n_items, 2048, 512)
    assert P.Q[lone] == 4


# ------------------------------------------------------------------------------------------------- the oracle's side
ORACLE_FAMILIES = ("wide_few", "wide_many", "wide_counts", "full_heavy:full", "full_heavy:ties", "full_heavy:chunks", "fill")


def _shuffled(r, seed):
    """the same ratings with the users permuted and the entries of every profile permuted -> (ratings, new index of every user)"""
    from xmap.engine import synth
    rng = np.random.default_rng(seed)
    d = np.diff(r.user_ptr)
    order = rng.permutation(r.n_users)                       # order[k] = the user stored k-th
    users = np.repeat(np.arange(r.n_users), d)
    place = np.empty(r.n_users, np.int64)
    place[order] = np.arange(r.n_users)
    o = np.lexsort((rng.random(r.nnz), place[users]))
    ptr = np.concatenate([[0], np.cumsum(d[order])]).astype(np.int64)
    return synth.Ratings(ptr, r.item[o], r.rating[o], r.time[o], r.n_items, r.n_src_items, r.src_numbers, r.tgt_numbers), place


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ORACLE_FAMILIES)
def test_oracle_does_not_depend_on_storage_order(name, method):
    """stage A's result is a function of the set of ratings: users and the entries inside profiles permuted, the oracle gives
    the same bytes -- and so does the plan"""
    from oracle import xmap_oracle as xo
    r = family(name)
    T, So = oracle_sim(name, method)
    g, place = _shuffled(r, 99)
    assert not np.array_equal(g.item, r.item)
    Tg = xo.Train(g.user_ptr, g.item, g.rating, g.time, g.n_items, *g.item_attrs())
    Sg = xo.item_sim(Tg, method, CAP, nthreads=8)
    for key in ("row_ptr", "col", "sim", "mutu", "nij", "info"):
        assert np.array_equal(getattr(Sg, key), getattr(So, key)), key
    assert Sg.n_eval == So.n_eval and Sg.n_contrib == So.n_contrib
    assert np.array_equal(Sg.uavg[place], So.uavg)
    xo.sim_free(Sg)
    ch_min, slot_target = [(c, s) for nm, c, s, _ in RUNS if nm == name][0]
    P, Pg = plan_of(name, ch_min, slot_target), plan_statement(g.user_ptr, g.item, g.n_items, ch_min, slot_target)
    for key in ("n", "Wp", "bound", "Q", "C", "cls", "heavy"):
        assert np.array_equal(getattr(P, key), getattr(Pg, key)), key
    assert So.n_contrib == 2 * int(P.Wp.sum())               # the contributions the layout counts are the oracle's


# Two hubs of a and b raters among U users share a b / U raters on average: the 48 hubs of wide_many (2 048 .. 2 579 raters, 4 300
# users) share 975 .. 1 547 with one another (standard deviation of the hypergeometric count: below 17), never 2 048 -- only
# an all-user hub shares a row's every rater.  The condition "a kept pair with n_ij >= 2048" is therefore met by wide_few (two
# all-user hubs), in every plan that makes its hubs class 4; wide_many's rows are held to 900, four deviations below the
# smallest mean.
WIDE_NIJ = dict(wide_few=2048, wide_many=900)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["wide_few", "wide_many"])
def test_class4_rows_count_thousands_of_raters_per_slot(name, method):
    T, So = oracle_sim(name, method)
    rows = oracle_rows(So)
    for nm, ch_min, slot_target, _ in RUNS:
        if nm != name:
            continue
        P = plan_of(name, ch_min, slot_target)
        wide = np.nonzero(P.cls == 4)[0]
        assert len(wide) > 0
        for i in wide:
            # the pairs row i computes itself are those with a heavier partner
            own = (rows == i) & ((P.n[So.col] > P.n[i]) | ((P.n[So.col] == P.n[i]) & (So.col > i)))
            assert own.any() and So.nij[own].max() >= WIDE_NIJ[name], (i, P.n[i])


@pytest.mark.parametrize("method", METHODS)
def test_a_class4_slot_counts_beyond_16_bits(method):
    """wide_counts: the lighter all-user hub is class 4 and keeps its pair with the other hub, n_ij = 66 000 >= 2^16 -- a count a
    16-bit half of the slot's count word would wrap (to 464, spilling into the mutuality half); the other class-4 rows count
    their every rater against the hubs"""
    r, hubs = wide_counts()
    (lo, n_lo), (hi, n_hi) = hubs
    assert n_lo == n_hi == COUNT_USERS >= 1 << 16
    P = plan_of("wide_counts", 1 << 17, 768)
    T, So = oracle_sim("wide_counts", method)
    rows = oracle_rows(So)
    assert P.cls[lo] == 4 and P.bound[lo] == 1 and P.Wp[lo] == COUNT_USERS and P.Q[hi] == 0      # the pair is computed in row lo
    pair = (rows == lo) & (So.col == hi)
    assert pair.sum() == 1 and So.nij[pair][0] == COUNT_USERS and 0 < So.mutu[pair][0] < COUNT_USERS
    for i in np.nonzero(P.cls == 4)[0]:
        assert So.nij[(rows == i) & (So.col == hi)].tolist() == [min(P.n[i], COUNT_USERS)] and P.n[i] >= WIDE_MIN


@pytest.mark.parametrize("method", METHODS)
def test_fill_rows_evaluate_one_pair_per_slot(method):
    """the designed rows meet exactly L - 1 distinct partners (the oracle's count of evaluated pairs of that row alone): the
    table holds L - 1 slots whatever the filter keeps of them (a pair with one co-rater is kept when both ratings lie on the
    same side of their item's average)"""
    from oracle import xmap_oracle as xo
    r, lone, _, _ = fill()
    T, So = oracle_sim("fill", method)
    for L in FILL_L:
        i = lone[L]
        one = xo.item_sim(T, method, CAP, uavg=So.uavg, info=So.info, rows=(i, i + 1))
        assert one.n_eval == L - 1 and one.n_contrib == L - 1
        xo.sim_free(one)
        kept = int(So.row_ptr[i + 1] - So.row_ptr[i])
        assert 1 <= kept <= L - 1


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("variant", FULL_HEAVY_VARIANTS)
def test_full_heavy_rows_keep_heavy_partners(variant, method):
    """every heavy row keeps a pair with another heavy row: the dense table of the heavy kernel, the chunk partials and their
    merge decide entries of every one of the (up to 1 024) dense ids"""
    name = "full_heavy:" + variant
    T, So = oracle_sim(name, method)
    P = plan_of(name, FULL_HEAVY_CH_MIN, 768)
    rows = oracle_rows(So)
    both = P.heavy[rows] & P.heavy[So.col]
    assert np.array_equal(np.unique(rows[both]), np.nonzero(P.heavy)[0])
