"""The packed pair kernel of stage A (csrc/tri_pairs.hip: k_pair_pack -- G consecutive units of the 128- or 256-slot class in
one wave, sums by rank within the slot) against the CPU oracle and against k_pair_tri on the same units (XMAP_PAIR_PACKS=0
sends every class down the old route), both methods.  Every comparison is array_equal: row_ptr, the columns sorted within a
row, sim (bit patterns), mutu and nij; between the two routes also n_eval, n_kept and the final slot target.

What the inputs reach (asserted on the host from the NumPy statement of the plan, test_cpu_stage_a_layout.plan_statement,
before anything runs -- the units of a class are listed by item index, so pack b of a class holds its units G b .. G b + G - 1;
G = 2 in both classes, E = 3 rounds of 64 co-ratings in the 128-slot class and 6 in the 256-slot class):

  fill          the designed layouts of test_cpu_stage_a_layout: 259 units of the 256-slot class, 314 of the 128-slot class.
                Class ranges of 1, G - 1, G, G + 1 and 2 G + 1 units through the unit range of the call, at the start, at an odd
                offset and at the end of the class; the whole unit list cut at non-multiples of G inside both classes, the
                pieces together against the full call
  tiny_catalogue  40 items, 2 500 users: every row has at most 39 partners (128-slot class), thousands of co-ratings and
                hundreds of raters -- more than the 64 raters and the 64 E co-ratings a wave holds: every pack takes the
                member-by-member route
  small_catalogue  180 items, 1 500 users: 83 rows of the 256-slot class (97 .. 179 heavier items) with 224 .. 561 co-ratings
                each, so no pack of that class fits a wave either, some of them with fewer than 64 raters
  designed      rows placed by item index so that the packs of the 128-slot class are known (DESIGN below: raters and shared
                partners of every row, two rows per pack):
                  pack 0   64 raters and 192 co-ratings, both exactly at what a wave holds; the 32 raters of a row all hold
                           the same three partners: every slot is met by 32 lanes of one round
                  pack 2   60 + 4 raters sharing ONE partner: a slot that hands out ranks 0 .. 59 in one round
                  pack 3   a one-rater row next to a hub row (hundreds of raters, thousands of co-ratings): the pack goes
                           member by member as a whole
                  pack 5-7 rows of 40 raters with one partner each: 80 raters per pack, 80 co-ratings -- over the rater
                           limit alone
                  pack 8   a row of 100 raters (more raters than lanes) with a one-rater row
                  pack 9   60 raters, 240 co-ratings: over the co-rating limit alone
                  then     one-rater rows (packed route) and the hubs (member by member)
                with synth.fractional's ratings: the sums of the shared slots are inexact in fp64 in any order, so the
                double-double sums by rank have to give the oracle's bits; in cosine mode the host's predicate sends such
                ratings to the exact route, which follows adjusted cosine through the packed kernel.  Rows that keep no pair
                stand next to rows that keep some (asserted from the oracle)
  designed:int  the same structure with integer ratings: cosine mode's own template of the packed kernel

Shapes are the smallest that reach these paths; a case takes well under a second on the device.
"""
import functools

import numpy as np
import pytest

from test_cpu_stage_a_layout import CAP, METHODS, family, oracle_rows, plan_of, plan_statement

pytestmark = pytest.mark.gpu

G128, G256 = 2, 2           # rows per wave of the two packed classes (tri_pairs.hip: PACK_G128, PACK_G256)
CAP_128, CAP_256 = 64 * 3, 64 * 6      # co-ratings a wave holds (64 PACK_E128, 64 PACK_E256)
RANK_256, RANK_128 = 3, 4   # position of the two classes in the class-major unit list (order 4, 0, 2, 3, 1)
NO_HEAVY = 1 << 17          # a ch_min above every rater count: no heavy set
ROUTES = ("packed", "old")


# ------------------------------------------------------------------------------------------------------------ inputs
def _ratings(profiles, n_items, seed):
    """synth.Ratings from explicit profiles (lists of item indices), integer ratings 1..5 and times drawn from a seed"""
    from xmap.engine import synth
    rng = np.random.default_rng(seed)
    d = np.array([len(p) for p in profiles], np.int64)
    ptr = np.concatenate([[0], np.cumsum(d)]).astype(np.int64)
    item = np.concatenate([np.asarray(p, np.int64) for p in profiles]).astype(np.int32)
    rating = rng.integers(1, 6, size=len(item)).astype(np.float32)
    time = rng.integers(synth.T0, synth.T1 + 1, size=len(item), dtype=np.int64)
    n_src = n_items // 2
    return synth.Ratings(ptr, item, rating, time, n_items, n_src, np.arange(n_src), np.arange(n_items - n_src))


N_HUBS, N_HUB_USERS = 24, 2400
HUB = "hub"
# the designed rows in item order, two per pack of the 128-slot class: (raters, heavier partners every rater holds)
DESIGN = [
    (32, 3), (32, 3),       # pack 0: 64 raters and 192 co-ratings, both at the limit; every slot met by 32 lanes of a round
    (16, 4), (16, 4),       # pack 1: 32 raters, 128 co-ratings
    (60, 1), (4, 1),        # pack 2: ONE shared partner: a slot that hands out ranks 0 .. 59 in one round
    (1, 3), HUB,            # pack 3: a one-rater row and the lightest hub (hundreds of raters, thousands of co-ratings)
    (1, 2), (2, 2),         # pack 4
    (40, 1), (40, 1), (40, 1), (40, 1), (40, 1), (40, 1),     # packs 5-7: 80 raters, 80 co-ratings: over the rater limit alone
    (100, 1), (1, 5),       # pack 8: more raters than lanes in one row
    (30, 4), (30, 4),       # pack 9: 60 raters, 240 co-ratings: over the co-rating limit alone
]
HUB_ITEM = DESIGN.index(HUB)
LIGHT = len(DESIGN) + 60    # the designed rows, then sixty one-rater rows


@functools.lru_cache(maxsize=None)
def designed(fractional=True):
    """-> ratings.  Items 0 .. LIGHT - 1 are the light rows in pack order (item HUB_ITEM is the lightest hub); the other hubs
    follow.  A hub has several hundred raters, the heaviest about a thousand."""
    from xmap.engine import synth
    rng = np.random.default_rng(77)
    hubs = [HUB_ITEM] + list(range(LIGHT, LIGHT + N_HUBS - 1))
    profiles = []
    # hub users: 4 .. 10 hubs each; hub k is picked with a weight that rises with k, so hubs[0] is the lightest by far
    w = np.linspace(0.35, 1.0, N_HUBS)
    for _ in range(N_HUB_USERS):
        k = int(rng.integers(4, 11))
        profiles.append([hubs[x] for x in rng.choice(N_HUBS, k, replace=False, p=w / w.sum())])
    heavy_hubs = hubs[-8:]
    for it, row in enumerate(DESIGN):
        if row != HUB:
            for _ in range(row[0]):             # the raters of a row all hold the same partners
                profiles.append([it] + heavy_hubs[it % 3:it % 3 + row[1]])
    # sixty one-rater rows with one to eight hubs: small rows of different sizes
    for it in range(len(DESIGN), LIGHT):
        profiles.append([it] + [hubs[x] for x in rng.choice(N_HUBS, int(rng.integers(1, 9)), replace=False)])
    order = rng.permutation(len(profiles))
    r = _ratings([profiles[x] for x in order], LIGHT + N_HUBS - 1, 78)
    return synth.fractional(r, seed=79) if fractional else r


@functools.lru_cache(maxsize=None)
def tiny_catalogue():
    from xmap.engine import synth
    return synth.make_two_domain(61, 2500, 20, 20, overlap=0.5)


@functools.lru_cache(maxsize=None)
def small_catalogue():
    from xmap.engine import synth
    return synth.make_two_domain(62, 1500, 90, 90, overlap=0.5)


def ratings_of(name):
    if name == "small_catalogue":
        return small_catalogue()
    if name == "designed":
        return designed(True)
    if name == "designed:int":
        return designed(False)
    if name == "tiny_catalogue":
        return tiny_catalogue()
    return family(name)


# (name, ch_min): the plans of the full calls
FULL = [("fill", 2048), ("tiny_catalogue", NO_HEAVY), ("small_catalogue", NO_HEAVY), ("designed", NO_HEAVY), ("designed:int", NO_HEAVY)]
FULL_IDS = [f[0] for f in FULL]


@functools.lru_cache(maxsize=None)
def plan(name, ch_min):
    if name == "fill":
        return plan_of("fill", ch_min, 768)
    r = ratings_of(name)
    return plan_statement(r.user_ptr, r.item, r.n_items, ch_min, 768)


def class_units(P, cls):
    """the items of a class's units in list order (one unit per row: Q == 1 in the packed classes)"""
    rows = np.nonzero((P.cls == cls) & (P.Q >= 1))[0]
    assert np.all(P.Q[rows] == 1)
    return rows


@functools.lru_cache(maxsize=None)
def design_holds():
    """the properties the module docstring claims for its inputs, from the statement of the plan"""
    P = plan("fill", 2048)
    assert P.cls_ptr.tolist() == [0, 0, 3446, 3913, 4172, 4486] and P.n_heavy == 0
    assert len(class_units(P, 3)) == 259 and len(class_units(P, 1)) == 314
    P = plan("tiny_catalogue", NO_HEAVY)
    u = class_units(P, 1)
    assert P.n_light == len(u) == 39 and P.n.max() < 2048 and P.bound.max() <= 39            # one class, no wide row
    assert P.Wp[u].min() > CAP_128 and P.n[u].min() > 64                                      # every row alone is too much for a pack
    P = plan("small_catalogue", NO_HEAVY)
    u = class_units(P, 3)
    assert P.cls_ptr.tolist() == [0, 0, 0, 0, 83, 179] and len(u) == 83 and P.n.max() < 2048
    assert all(P.Wp[u[k:k + G256]].sum() > CAP_256 for k in range(0, len(u) - 1, G256))       # no pack of the 256-slot class fits a wave
    assert any(P.n[u[k:k + G256]].sum() <= 64 for k in range(0, len(u) - 1, G256))           # some by their co-ratings alone
    for name in ("designed", "designed:int"):
        P = plan(name, NO_HEAVY)
        u = class_units(P, 1)
        assert P.n_heavy == 0 and P.n_light == len(u) and np.array_equal(u[:LIGHT], np.arange(LIGHT))   # pack b = items 2 b, 2 b + 1
        n, W = P.n, P.Wp
        for it, row in enumerate(DESIGN):
            if row != HUB:
                assert (n[it], W[it]) == (row[0], row[0] * row[1])
        assert n[HUB_ITEM] > 64 and W[HUB_ITEM] > CAP_128
        assert n[0:2].sum() == 64 and W[0:2].sum() == CAP_128                  # pack 0: at both limits, packed
        assert n[18:20].sum() <= 64 and W[18:20].sum() > CAP_128               # pack 9: over the co-rating limit alone
        assert n[10:12].sum() > 64 and W[10:12].sum() <= CAP_128               # packs 5-7: over the rater limit alone
        rest = u[len(DESIGN):]
        packs = [rest[k:k + G128] for k in range(0, len(rest), G128)]
        small = [p for p in packs if n[p].sum() <= 64 and W[p].sum() <= CAP_128]
        big = [p for p in packs if n[p].sum() > 64]
        assert len(small) >= 25 and len(big) >= 8                              # both routes after the designed packs
    return True


# ------------------------------------------------------------------------------------------------------------ running
@functools.lru_cache(maxsize=None)
def engine(name):
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device  # raises if libxmap_hip.so is missing: no CPU fallback
    r = ratings_of(name)
    return device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))


@functools.lru_cache(maxsize=None)
def oracle(name, method):
    """the CPU oracle's stage A, computed once per input and method and shared"""
    from oracle import xmap_oracle as xo
    r = ratings_of(name)
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
    return xo.item_sim(T, method, CAP, nthreads=8)


def on_route(monkeypatch, route, fn):
    if route == "old":
        monkeypatch.setenv("XMAP_PAIR_PACKS", "0")
    else:
        monkeypatch.delenv("XMAP_PAIR_PACKS", raising=False)
    out = fn()
    monkeypatch.delenv("XMAP_PAIR_PACKS", raising=False)
    return out


def csr_sorted(S):
    row_ptr = S.row_ptr.cpu().numpy()
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))
    col = S.col.cpu().numpy().astype(np.int64)
    o = np.lexsort((col, rows))
    return row_ptr, col[o], S.sim.cpu().numpy()[o].view(np.uint64), S.mutu.cpu().numpy()[o], S.nij.cpu().numpy()[o]


def coo_sorted(coo):
    """the valid entries of a half COO (unused ones are marked -1), sorted by (row, partner)"""
    i = coo[0].cpu().numpy().astype(np.int64)
    ok = i >= 0
    i, j = i[ok], coo[1].cpu().numpy().astype(np.int64)[ok]
    o = np.lexsort((j, i))
    return (i[o], j[o], coo[2].cpu().numpy()[ok][o].view(np.uint64), coo[3].cpu().numpy()[ok][o], coo[4].cpu().numpy()[ok][o])


def own_half(So, P, items):
    """the oracle's pairs that the rows `items` compute themselves (those with a heavier partner), sorted by (row, partner)"""
    rows, col = oracle_rows(So), So.col.astype(np.int64)
    sel = np.zeros(So.I, bool)
    sel[items] = True
    own = sel[rows] & ((P.n[col] > P.n[rows]) | ((P.n[col] == P.n[rows]) & (col > rows)))
    return rows[own], col[own], So.sim[own].view(np.uint64), So.mutu[own], So.nij[own]


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@functools.lru_cache(maxsize=None)
def laid_out(name, ch_min):
    eng = engine(name)
    stats, L = eng.layout3(768, ch_min)
    return eng, stats, L


def range_pairs(monkeypatch, route, name, ch_min, method, lo, hi):
    eng, stats, L = laid_out(name, ch_min)
    coo, rowcnt, n, n_unordered = on_route(monkeypatch, route,
                                           lambda: eng.tri_pairs(method, CAP, stats, L, unit_range=(lo, hi), do_heavy=False))
    out = coo_sorted(coo)
    assert len(out[0]) == n
    # a row-count add per member; the call adds the mirrored counts (taken from the partner column) on top
    cnt = rowcnt.cpu().numpy()
    assert np.array_equal(np.bincount(out[0], minlength=len(cnt)) + np.bincount(out[1], minlength=len(cnt)), cnt)
    return out, n_unordered


# ------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,ch_min", FULL, ids=FULL_IDS)
def test_full_call(name, ch_min, method, monkeypatch):
    """stage A whole: both routes against the oracle and against each other"""
    assert design_holds()
    So = oracle(name, method)
    eng = engine(name)
    res = {}
    for route in ROUTES:
        S = on_route(monkeypatch, route, lambda: eng.item_sim_tri(method, CAP, ch_min=ch_min))
        assert [int(x) for x in S.layout.cls_ptr] == plan(name, ch_min).cls_ptr.tolist()
        got = csr_sorted(S)
        assert np.array_equal(got[0], So.row_ptr) and np.array_equal(got[1], So.col)
        assert np.array_equal(got[2], So.sim.view(np.uint64))
        assert np.array_equal(got[3], So.mutu) and np.array_equal(got[4], So.nij)
        assert S.n_eval == So.n_eval
        res[route] = (got, S.n_eval, S.n_kept, S.slot_target)
    same(res["packed"][0], res["old"][0])
    assert res["packed"][1:] == res["old"][1:] and res["packed"][3] == 768


@pytest.mark.parametrize("name", ["designed", "designed:int"])
def test_rows_without_pairs_stand_next_to_rows_with_pairs(name):
    """(the input's side of test_full_call: among the packed-route packs of one-rater rows, some members keep nothing)"""
    assert design_holds()
    P = plan(name, NO_HEAVY)
    for method in METHODS:
        So = oracle(name, method)
        own = np.bincount(own_half(So, P, np.arange(So.I))[0], minlength=So.I)
        u = class_units(P, 1)
        mixed = 0
        for k in range(0, len(u) - G128 + 1, G128):
            p = u[k:k + G128]
            if P.n[p].sum() <= 64 and P.Wp[p].sum() <= CAP_128 and own[p].min() == 0 and own[p].max() > 0:
                mixed += 1
        assert mixed >= 3


RANGE_N = {RANK_128: sorted({1, G128 - 1, G128, G128 + 1, 2 * G128 + 1}), RANK_256: sorted({1, G256 - 1, G256, G256 + 1, 2 * G256 + 1})}


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("rank", [RANK_128, RANK_256], ids=["128", "256"])
def test_class_ranges_of_a_few_units(rank, method, monkeypatch):
    """1, G - 1, G, G + 1 and 2 G + 1 units of one packed class: the unit range of the call cuts them out of `fill`, at the
    start of the class, at an odd offset and at its end"""
    assert design_holds()
    P = plan("fill", 2048)
    So = oracle("fill", method)
    c0, c1 = int(P.cls_ptr[rank]), int(P.cls_ptr[rank + 1])
    units = class_units(P, 1 if rank == RANK_128 else 3)
    assert c1 - c0 == len(units)
    for n in RANGE_N[rank]:
        for lo in (c0, c0 + 7, c1 - n):
            want = own_half(So, P, units[lo - c0:lo - c0 + n])
            got, n_un = {}, {}
            for route in ROUTES:
                got[route], n_un[route] = range_pairs(monkeypatch, route, "fill", 2048, method, lo, lo + n)
                same(got[route], want)
            same(got["packed"], got["old"])
            assert len(want[0]) <= n_un["packed"] == n_un["old"] <= int(P.bound[units[lo - c0:lo - c0 + n]].sum())


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name,ch_min", [("fill", 2048), ("designed", NO_HEAVY)], ids=["fill", "designed"])
def test_unit_list_cut_inside_the_packed_classes(name, ch_min, method, monkeypatch):
    """the shares of item-sharded ranks: the unit list cut at non-multiples of G inside both packed classes; the pieces
    together are the full call, on both routes"""
    assert design_holds()
    P = plan(name, ch_min)
    c3, c1, end = int(P.cls_ptr[RANK_256]), int(P.cls_ptr[RANK_128]), int(P.cls_ptr[5])
    cuts = sorted(set(x for x in (0, c3 + 1, c3 + 4, c1 - 1, c1 + 1, c1 + 6, c1 + 9, c1 + 27, end - 2, end) if 0 <= x <= end))
    assert any((x - c1) % G128 for x in cuts if c1 < x < end)
    full = {}
    for route in ROUTES:
        full[route], n_un_full = range_pairs(monkeypatch, route, name, ch_min, method, 0, end)
        parts, n_un = [], 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part, k = range_pairs(monkeypatch, route, name, ch_min, method, lo, hi)
            parts.append(part)
            n_un += k
        cat = [np.concatenate([p[x] for p in parts]) for x in range(5)]
        o = np.lexsort((cat[1], cat[0]))
        same([c[o] for c in cat], full[route])
        assert n_un == n_un_full
    same(full["packed"], full["old"])
    So = oracle(name, method)
    same(full["packed"], own_half(So, P, np.arange(So.I)))
    assert 2 * n_un_full == So.n_eval
