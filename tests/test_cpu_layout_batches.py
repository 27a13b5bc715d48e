"""Designed inputs for the per-user and per-item kernels of the round-3 layout (x-map_amd/csrc/tri_layout.hip), with what each
reaches asserted here on the CPU; tests/test_gpu_layout_batches.py runs them.

The sort (k_sort_profiles3) gives a wave NB = 16 consecutive users: user u is place u % NB of its batch, place k belongs to
round k // 4 and to 16-lane group k % 4.  A profile is short (up to 16 ratings: one group's network), mid (17 .. 64: a network
on the whole wave, requested MB = 4 at a time), long (65 .. 256: counting ranks, keys in LDS) or very long (above 256: keys
in the global scratch); an empty profile sorts nothing.  The user statistics (k_user_stats) are sequential sums in profile
order.

The item statistics (k_item_stats3) give a wave four consecutive items of [lo, hi), one per 16-lane group: up to 64 raters on
the group (one to four records a lane, all requested together), 65 .. 512 on the whole wave, more in chunks of CHK = 2 048
raters (the tail: one wave a chunk, the chunk sums merged in chunk order).

`profiles()` is the one input: 4 613 users, 701 items, about 245 000 ratings.  Its users: a cycle of the fifteen LENS over the
batch places (period 15, batches of 16: every length at every place), then one batch of long profiles only, one of short ones
only, one of mid ones only (four requests of MB), one with MB + 1 mid ones, then random lengths, then 2 000 users of one or two
ratings (raters for the item of three chunks); the last batch has 5 users.
Its items 0 .. 39 have designed rater counts (DESIGNED); the others are drawn at random.  `prefix(U)` is its first U users."""
import functools

import numpy as np
import pytest

NB, MB = 16, 4                    # users per wave of the sort; mid profiles requested together
STAT_BIG, CHK = 512, 2048         # most raters of an item summed by one wave; raters per chunk of a bigger one
LENS = (0, 1, 2, 15, 16, 17, 32, 33, 63, 64, 65, 255, 256, 257, 300)
LONG, SHORT, MID = (65, 255, 256, 257, 300), (0, 1, 2, 15, 16), (17, 32, 33, 63, 64)
CYCLE_USERS = 1200                # 5 periods of lcm(15, 16) = 240
U_MAIN, I_MAIN, U_FILL = 4613, 701, 2000
SMALL_U = (1, NB - 1, NB, NB + 1, 3 * NB + 5)

# item -> raters.  Items 0 .. 3: a block of four whole-wave items; 4 .. 7: the three chunked ones (one above 2 048, one above
# two chunks -- its third holds one rater --, one of STAT_BIG + 1) and the smallest whole-wave count; 8 .. 39: one to four records a lane at every group
GROUP_COUNTS = (1, 16, 17, 32, 33, 48, 49, 64)
DESIGNED = {0: 100, 1: 200, 2: 300, 3: 512, 4: 513, 5: 2 * CHK + 1, 6: 2100, 7: 65}
DESIGNED.update({8 + 4 * c + g: GROUP_COUNTS[(c + g) % 8] for c in range(8) for g in range(4)})


def user_class(d):
    return "empty" if d == 0 else "short" if d <= 16 else "mid" if d <= 64 else "long" if d <= 256 else "very_long"


def lengths():
    rng = np.random.default_rng(4201)
    lens = [LENS[(u + 5) % 15] for u in range(CYCLE_USERS)]           # user 0 has 17 ratings
    lens += [LONG[k % 5] for k in range(NB)]
    lens += [SHORT[k % 5] for k in range(NB)]
    lens += [MID[k % 5] for k in range(NB)]
    lens += [MID[k % 5] if k % 3 == 0 and k < 3 * (MB + 1) else SHORT[1 + k % 4] for k in range(NB)]
    lens += [int(x) for x in rng.choice(LENS, U_MAIN - U_FILL - len(lens))]
    lens += [1 + k % 2 for k in range(U_FILL)]
    return np.array(lens, np.int64)


@functools.lru_cache(maxsize=None)
def profiles():
    from xmap.engine import synth
    rng = np.random.default_rng(4202)
    d = lengths()
    U, I = len(d), I_MAIN
    mine = [[] for _ in range(U)]
    room = d.copy()
    for it in sorted(DESIGNED, key=lambda x: -DESIGNED[x]):
        cand = rng.permutation(U)
        cand = cand[room[cand] > 0][:DESIGNED[it]]
        assert len(cand) == DESIGNED[it]
        for u in cand:
            mine[u].append(it)
        room[cand] -= 1
    pool = np.setdiff1d(np.arange(I), sorted(DESIGNED))
    items = []
    for u in range(U):
        prof = np.concatenate([np.array(mine[u], np.int64), rng.choice(pool, room[u], replace=False)])
        rng.shuffle(prof)
        items.append(prof)
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(d, out=ptr[1:])
    item = np.concatenate(items).astype(np.int32)
    rating = rng.integers(1, 6, len(item)).astype(np.float32)
    time = rng.integers(synth.T0, synth.T1 + 1, size=len(item), dtype=np.int64)
    return synth.Ratings(ptr, item, rating, time, I, I // 2, np.arange(I // 2), np.arange(I - I // 2))


@functools.lru_cache(maxsize=None)
def prefix(U):
    """the first U users of profiles() (all its items: those nobody rates any more have no rater)"""
    from xmap.engine import synth
    r = profiles()
    n = int(r.user_ptr[U])
    return synth.Ratings(r.user_ptr[:U + 1].copy(), r.item[:n].copy(), r.rating[:n].copy(), r.time[:n].copy(), r.n_items,
                         r.n_src_items, r.src_numbers, r.tgt_numbers)


@functools.lru_cache(maxsize=None)
def fractional():
    from xmap.engine import synth
    return synth.fractional(profiles(), seed=43)


@functools.lru_cache(maxsize=None)
def wide_rows():
    """AlterEgo-like rows for the fp64 path: the first 6 NB + 3 users of profiles() with fp64 ratings that no float32 holds;
    one short, one mid, one long and one very long profile hold an item twice (appended copies, other ratings).
    -> (ptr, item, rating, users with a repeated item)"""
    r = prefix(6 * NB + 3)
    d = np.diff(r.user_ptr)
    twice = [int(np.nonzero(d == L)[0][0]) for L in (15, 33, 255, 300)]           # -> 16, 34, 256, 301 ratings
    rows = []
    for u in range(r.n_users):
        a, b = int(r.user_ptr[u]), int(r.user_ptr[u + 1])
        it, ra = r.item[a:b].astype(np.int64), r.rating[a:b].astype(np.float64) / 3.0 + 0.125
        if u in twice:
            it, ra = np.concatenate([it, it[:1]]), np.concatenate([ra, ra[:1] * 0.5 + 1.0])
        rows.append((it, ra))
    ptr = np.concatenate([[0], np.cumsum([len(it) for it, _ in rows])]).astype(np.int64)
    return ptr, np.concatenate([it for it, _ in rows]).astype(np.int32), np.concatenate([ra for _, ra in rows]), twice


# ------------------------------------------------------------------------------------------------------- the statements
def user_stats_statement(user_ptr, rating):
    """u_avg, u_norm as get_universal_user_info sums them: s += r, q += r * r in profile order, in fp64"""
    U = len(user_ptr) - 1
    avg, norm = np.zeros(U), np.zeros(U)
    r = rating.astype(np.float64)
    for u in range(U):
        a, b = int(user_ptr[u]), int(user_ptr[u + 1])
        if b > a:
            avg[u] = np.cumsum(r[a:b])[-1] / (b - a)           # np.cumsum adds one by one, in order
            norm[u] = np.sqrt(np.cumsum(r[a:b] * r[a:b])[-1])
    return avg, norm


def sort_statement(user_ptr, item, n_items):
    """-> (order, pos): every profile by weight (raters of the item, then its index) descending; the place of every sorted
    entry in its profile (0 for users of one rating).  Items held twice keep their storage order."""
    d = np.diff(user_ptr)
    users = np.repeat(np.arange(len(d), dtype=np.int64), d)
    n = np.bincount(item, minlength=n_items).astype(np.int64)
    o = np.lexsort((np.arange(len(item)), -item.astype(np.int64), -n[item], users))
    pos = np.arange(len(item), dtype=np.int64) - user_ptr[users[o]]
    pos[d[users[o]] < 2] = 0
    return o, pos


def pairwise_sum(x):
    return x[0] if len(x) == 1 else pairwise_sum(x[:len(x) // 2]) + pairwise_sum(x[len(x) // 2:])


def strided_sum(x, lanes=16):
    """lane-strided partial sums added up by a butterfly"""
    part = [np.float64(0.0)] * lanes
    for k, v in enumerate(x):
        part[k % lanes] = part[k % lanes] + v
    while len(part) > 1:
        part = [part[k] + part[k + len(part) // 2] for k in range(len(part) // 2)]
    return part[0]


# ------------------------------------------------------------------------------------------------------------ coverage
def test_every_length_at_every_place_of_a_batch():
    d = np.diff(profiles().user_ptr)
    assert len(d) == U_MAIN and U_MAIN % NB == 5 and CYCLE_USERS % NB == 0 and U_FILL % NB == 0
    seen = {(u % NB, int(d[u])) for u in range(len(d))}
    assert seen >= {(k, L) for k in range(NB) for L in LENS}
    # ... and so every class in every round and every group; also for batches cut one user earlier or later
    for off in (-1, 0, 1):
        cls = {((u + off) % NB // 4, (u + off) % NB % 4, user_class(int(d[u]))) for u in range(len(d))}
        assert cls >= {(r, g, c) for r in range(NB // 4) for g in range(4) for c in ("empty", "short", "mid", "long", "very_long")}


def test_designed_batches():
    d = np.diff(profiles().user_ptr)
    b = CYCLE_USERS
    assert all(user_class(int(x)) in ("long", "very_long") for x in d[b:b + NB])
    assert all(user_class(int(x)) in ("empty", "short") for x in d[b + NB:b + 2 * NB])
    assert all(user_class(int(x)) == "mid" for x in d[b + 2 * NB:b + 3 * NB])
    assert sum(user_class(int(x)) == "mid" for x in d[b + 3 * NB:b + 4 * NB]) == MB + 1
    # the batches of the cycle ask for their mid profiles in two requests, some of the random ones in one; several long ones
    mids = [sum(user_class(int(x)) == "mid" for x in d[k:k + NB]) for k in range(0, len(d), NB)]
    assert all(MB < m <= 2 * MB for m in mids[:CYCLE_USERS // NB])
    assert any(1 <= m <= MB for m in mids[CYCLE_USERS // NB + 4:])
    assert max(sum(int(x) > 64 for x in d[k:k + NB]) for k in range(0, CYCLE_USERS, NB)) >= 2


@pytest.mark.parametrize("U", SMALL_U)
def test_small_variants(U):
    r = prefix(U)
    assert r.n_users == U and r.nnz > 0 and r.n_items == I_MAIN
    assert int(np.diff(r.user_ptr)[0]) == 17


def test_item_classes():
    r = profiles()
    n = np.bincount(r.item, minlength=r.n_items)
    assert all(int(n[it]) == c for it, c in DESIGNED.items())
    assert all(len(set(r.item[a:b].tolist())) == b - a for a, b in zip(r.user_ptr[:-1], r.user_ptr[1:]))
    assert all(64 < n[it] <= STAT_BIG for it in range(4))                          # a block of whole-wave items only
    assert n[4] == STAT_BIG + 1 and n[5] == 2 * CHK + 1 and CHK < n[6] < 2 * CHK and n[3] == STAT_BIG
    # one to four records a lane (1 .. 16, 17 .. 32, 33 .. 48, 49 .. 64 raters) in every group, with both ends
    for g in range(4):
        assert {int(n[it]) for it in range(8, 40) if it % 4 == g} == set(GROUP_COUNTS)
    assert r.n_items % 4 == 1 and r.n_items % 16 != 0                              # the last wave has one item
    assert int((n[40:] > 64).sum()) > 600 and n.min() >= 1


def test_sequential_sums_differ_from_reordered_ones():
    """fractional ratings: for some users the sequential fp64 sum of r * r differs in its bits from a pairwise sum and from a
    lane-strided one, and so does its square root -- user statistics summed in another order than profile order could not
    give user_stats_statement's u_norm"""
    r = fractional()
    assert np.any(r.rating != np.round(r.rating))
    sq = r.rating.astype(np.float64) ** 2
    assert np.array_equal(sq, r.rating.astype(np.float64) * r.rating.astype(np.float64))
    differ = {"pairwise": {}, "strided": {}}
    for u in range(r.n_users):
        a, b = int(r.user_ptr[u]), int(r.user_ptr[u + 1])
        if b - a < 2:
            continue
        seq = np.cumsum(sq[a:b])[-1]
        for name, f in (("pairwise", pairwise_sum), ("strided", strided_sum)):
            if np.float64(f(list(sq[a:b]))).tobytes() != np.float64(seq).tobytes():
                differ[name].setdefault(user_class(b - a), u)
    _, norm = user_stats_statement(r.user_ptr, r.rating)
    for name, f in (("pairwise", pairwise_sum), ("strided", strided_sum)):
        assert set(differ[name]) >= {"mid", "long", "very_long"}, (name, differ[name])
        users = differ[name].values()
        assert any(np.sqrt(np.float64(f(list(sq[int(r.user_ptr[v]):int(r.user_ptr[v + 1])])))) != norm[v] for v in users)


def test_wide_rows_repeat_an_item_in_every_sorted_class():
    ptr, item, rating, twice = wide_rows()
    d = np.diff(ptr)
    assert sorted(int(d[u]) for u in twice) == [16, 34, 256, 301]
    for u in twice:
        prof = item[ptr[u]:ptr[u + 1]]
        assert len(set(prof.tolist())) == len(prof) - 1 and prof[0] == prof[-1]
    assert np.any(rating != rating.astype(np.float32).astype(np.float64))
    o, pos = sort_statement(ptr, item, I_MAIN)
    # the copies are neighbours in the sorted profile, in storage order
    for u in twice:
        so = o[ptr[u]:ptr[u + 1]]
        k = np.nonzero(item[so] == item[ptr[u]])[0]
        assert len(k) == 2 and k[1] == k[0] + 1 and so[k[0]] == ptr[u] and so[k[1]] == ptr[u + 1] - 1


def test_statements_on_a_hand_made_input():
    """three users {0, 1, 2}, {1, 2}, {2}: raters (1, 2, 3); sorted profiles (2, 1, 0), (2, 1), (2)"""
    ptr, item = np.array([0, 3, 5, 6]), np.array([0, 1, 2, 1, 2, 2], np.int32)
    o, pos = sort_statement(ptr, item, 3)
    assert item[o].tolist() == [2, 1, 0, 2, 1, 2] and pos.tolist() == [0, 1, 2, 0, 1, 0]
    avg, norm = user_stats_statement(ptr, np.array([1, 2, 3, 4, 5, 3], np.float32))
    assert avg.tolist() == [2.0, 4.5, 3.0] and norm.tolist() == [np.sqrt(14.0), np.sqrt(41.0), 3.0]
