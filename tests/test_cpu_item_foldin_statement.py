"""The statement of the item fold-in (include/xmap_hip.h, "item fold-in"; csrc/stage_e_itemfold.hip) in plain Python, checked on
the CPU: one row of RecommenderSim for an item that arrived after training, against frozen user-major profiles and norms.

item_foldin_statement is what every layer must reproduce bit for bit; tests/test_gpu_item_foldin.py imports it.  Here it is held
to the oracle's RecommenderSim (oracle.rec_sim): a resident item folded in as a copy of itself -- its raters are its holders'
entries, users ascending, profile order -- gets the oracle's resident row for every partner j != i, bit for bit (the resident
self pair pairs entries inside one profile, the fold-in pairs the copy with every holder: j = i is excluded).  Then the edges,
by hand."""
import math

import numpy as np
import pytest

NAN = float("nan")


# ------------------------------------------------------------------------------------------------------ the statement
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


def weighted(cs, n, cap):
    return 1.0 * cs * float(min(n, cap)) / float(cap)


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN            # (a NaN or a negative argument: NaN, as on the device)


def _div(a, b):
    """a / b for b != 0 the way fp64 hardware divides (Python raises nothing here: b is never zero)"""
    return float(np.float64(a) / np.float64(b))


def _ls_max(a, b):
    """the larger of two non-negative distances, NaN above everything"""
    if a != a or b != b:
        return NAN
    return a if a > b else b


def item_foldin_statement(ptr, user, rating, prof_ptr, prof_item, prof_rating, item_norm, cap):
    """-> (row_ptr [n_new + 1], col, sim, ls, nij [pairs] with every row sorted by col, avg [n_new], norm [n_new])"""
    ptr, user, rating = [np.asarray(a).tolist() for a in (ptr, user, rating)]
    prof_ptr, prof_item, prof_rating = [np.asarray(a).tolist() for a in (prof_ptr, prof_item, prof_rating)]
    item_norm = np.asarray(item_norm, np.float64).tolist()
    n_new = len(ptr) - 1
    row_ptr, col, sim, ls, nij, avg, norm = [0], [], [], [], [], [], []
    with np.errstate(all="ignore"):
        for q in range(n_new):
            entries = list(range(ptr[q], ptr[q + 1]))
            r0s = [float(rating[e]) for e in entries]
            avg.append(_div(1.0 * dd_sum(r0s), float(len(r0s))) if r0s else 0.0)
            nx = _sqrt(dd_sum([r * r for r in r0s]))
            norm.append(nx)
            records = {}                                        # j -> [(r0, r1)*] in expansion order
            for e in entries:
                u = user[e]
                for p in range(prof_ptr[u], prof_ptr[u + 1]):
                    records.setdefault(prof_item[p], []).append((float(rating[e]), float(prof_rating[p])))
            for j in sorted(records):
                rec = records[j]
                n = len(rec)
                inner = dd_sum([r0 * r1 for r0, r1 in rec])
                ny = item_norm[j]
                np_ = nx * ny
                s = weighted(_div(1.0 * inner, np_) if np_ != 0.0 else 0.0, n, cap)
                best = 0.0
                for r0, r1 in rec:
                    rest = inner - r0 * r1
                    m1 = _sqrt((nx * nx - r0 * r0) * (ny * ny))
                    m2 = _sqrt((nx * nx) * (ny * ny - r1 * r1))
                    d1 = abs(weighted(_div(1.0 * rest, m1) if m1 != 0.0 else 0.0, n - 1, cap) - s)
                    d2 = abs(weighted(_div(1.0 * rest, m2) if m2 != 0.0 else 0.0, n - 1, cap) - s)
                    best = _ls_max(best, _ls_max(d1, d2))
                col.append(j); sim.append(s); ls.append(best); nij.append(n)
            row_ptr.append(len(col))
    return (np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(sim, np.float64), np.asarray(ls, np.float64),
            np.asarray(nij, np.int32), np.asarray(avg, np.float64), np.asarray(norm, np.float64))


def copy_batch(items, prof_ptr, prof_item, prof_rating):
    """the batch that folds resident items in as copies of themselves: per item its holders' entries, users ascending, profile order"""
    ptr, user, rating = [0], [], []
    prof_ptr, prof_item, prof_rating = np.asarray(prof_ptr), np.asarray(prof_item), np.asarray(prof_rating)
    owner = np.repeat(np.arange(len(prof_ptr) - 1), np.diff(prof_ptr))
    for i in items:
        rows = np.nonzero(prof_item[:prof_ptr[-1]] == i)[0]
        user += owner[rows].tolist()
        rating += prof_rating[rows].tolist()
        ptr.append(len(user))
    return np.asarray(ptr, np.int64), np.asarray(user, np.int32), np.asarray(rating, np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_doubles(a, b):
    """equal as bit patterns, every NaN equal to every NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


FAMILIES = {
    "halves": lambda rng, n: rng.integers(1, 11, n) / 2.0,
    "thirds": lambda rng, n: rng.integers(1, 16, n) / 3.0,
    "decimals": lambda rng, n: rng.choice(np.asarray([0.1, 1.7, 2.9, 3.3, 4.9]), n),
}


def random_profiles(rng, U, I, max_rows, family):
    """profiles of 0 .. max_rows rows, items drawn with repeats"""
    lens = rng.integers(0, max_rows + 1, U)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    item = rng.integers(0, I, int(ptr[-1])).astype(np.int32)
    return ptr, item, np.asarray(FAMILIES[family](rng, int(ptr[-1])), np.float64)


# --------------------------------------------------------------------------------- a copy of a resident item is its row
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_a_copy_of_a_resident_item_gets_the_resident_row(family):
    from oracle import xmap_oracle as xo
    U, I, cap = 120, 40, 5
    rng = np.random.default_rng(sorted(FAMILIES).index(family) + 41)
    ptr, item, rating = random_profiles(rng, U, I, 8, family)
    R = xo.rec_sim(ptr, item, rating, I, cap)
    try:
        batch = copy_batch(range(I), ptr, item, rating)
        row_ptr, col, sim, ls, nij, avg, norm = item_foldin_statement(*batch, ptr, item, rating, R.norm, cap)
        compared = 0
        for i in range(I):
            a, b = int(R.row_ptr[i]), int(R.row_ptr[i + 1])
            o = np.argsort(R.col[a:b], kind="stable") + a
            o = o[R.col[o] != i]
            mine = np.arange(row_ptr[i], row_ptr[i + 1])
            mine = mine[col[mine] != i]
            assert col[mine].tolist() == R.col[o].tolist(), i
            assert np.array_equal(bits(sim[mine]), bits(R.sim[o])), i
            assert same_doubles(ls[mine], R.ls[o]), i
            assert nij[mine].tolist() == R.nij[o].tolist(), i
            compared += len(mine)
        assert np.array_equal(bits(norm), bits(R.norm))
        held = [rating[item == i].tolist() for i in range(I)]           # the correctly rounded sum, divided once
        assert np.array_equal(bits(avg), bits([math.fsum(h) / len(h) if h else 0.0 for h in held]))
        assert compared > 1000
    finally:
        xo.rec_free(R)


# ------------------------------------------------------------------------------------------------------------- by hand
def _profiles(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = [x for r in rows for x in r]
    return ptr, np.asarray([x[0] for x in flat], np.int32), np.asarray([x[1] for x in flat], np.float64)


def _batch(items):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in items])]).astype(np.int64)
    flat = [x for r in items for x in r]
    return ptr, np.asarray([x[0] for x in flat], np.int32), np.asarray([x[1] for x in flat], np.float64)


def test_hand_checked_edges():
    # users: 0 holds item 0 twice and item 1; 1 holds nothing; 2 holds item 1; 3 .. 8 hold item 2 once each
    prof = _profiles([[(0, 2.0), (1, 4.0), (0, 1.0)], [], [(1, 3.0)]] + [[(2, 1.0)]] * 6)
    norms = np.asarray([math.sqrt(5.0), 5.0, math.sqrt(6.0)])
    cap = 3
    batch = _batch([
        [],                                     # 0: an item without raters
        [(1, 5.0)],                             # 1: a rater without rows
        [(2, 2.0), (2, 2.0)],                   # 2: a rater listed twice
        [(0, 3.0)],                             # 3: a partner held twice (item 0), and n = 1 (item 1)
        [(0, 0.0), (2, 0.0)],                   # 4: all-zero ratings
        [(3, 1.0), (4, 1.0)],                   # 5: n = 2 < cap
        [(3, 1.0), (4, 1.0), (5, 1.0)],         # 6: n = 3 = cap
        [(3, 1.0), (4, 1.0), (5, 1.0), (6, 1.0), (7, 1.0)],     # 7: n = 5 > cap
    ])
    row_ptr, col, sim, ls, nij, avg, norm = item_foldin_statement(*batch, *prof, norms, cap)
    rows = [dict((int(col[k]), (float(sim[k]), float(ls[k]), int(nij[k]))) for k in range(row_ptr[q], row_ptr[q + 1])) for q in range(8)]
    assert rows[0] == {} and avg[0] == 0.0 and norm[0] == 0.0
    assert rows[1] == {} and avg[1] == 5.0 and norm[1] == 5.0
    # the rater listed twice: two records against item 1, inner = 2 * 3 + 2 * 3, nx = sqrt(8)
    assert list(rows[2]) == [1] and rows[2][1][2] == 2 and avg[2] == 2.0 and norm[2] == math.sqrt(8.0)
    assert rows[2][1][0] == 1.0 * (12.0 / (math.sqrt(8.0) * 5.0)) * 2.0 / 3.0
    # the partner held twice: records (3, 2) and (3, 1) in profile order; item 1 once
    assert sorted(rows[3]) == [0, 1] and rows[3][0][2] == 2 and rows[3][1][2] == 1
    assert rows[3][0][0] == 1.0 * (9.0 / (3.0 * math.sqrt(5.0))) * 2.0 / 3.0
    s1 = 1.0 * (12.0 / (3.0 * 5.0)) * 1.0 / 3.0
    assert rows[3][1] == (s1, abs(s1), 1)                                   # n = 1: ls = |sim|
    # all-zero ratings: nx = 0, sim = 0.0, still an entry per partner
    assert norm[4] == 0.0 and avg[4] == 0.0 and sorted(rows[4]) == [0, 1]
    assert all(v[0] == 0.0 for v in rows[4].values()) and rows[4][0][2] == 2 and rows[4][1][2] == 2
    # n below, at and above the cap
    for q, n in ((5, 2), (6, 3), (7, 5)):
        cs = float(n) / (math.sqrt(float(n)) * math.sqrt(6.0))
        assert list(rows[q]) == [2] and rows[q][2][2] == n
        assert rows[q][2][0] == 1.0 * cs * float(min(n, cap)) / float(cap)
    assert rows[5][2][0] < rows[6][2][0] and rows[7][2][0] > rows[6][2][0]     # the weight stops growing at the cap, the cosine does not


def test_nan_ranks_above_every_distance():
    prof = _profiles([[(0, 1.0)], [(0, NAN)]])
    row_ptr, col, sim, ls, nij, avg, norm = item_foldin_statement(*_batch([[(0, 1.0), (1, 2.0)]]), *prof, np.asarray([1.5]), 5)
    assert nij.tolist() == [2] and np.isnan(sim[0]) and np.isnan(ls[0])
    assert _ls_max(NAN, 3.0) != _ls_max(NAN, 3.0) and _ls_max(2.0, 3.0) == 3.0 and _ls_max(3.0, NAN) != 3.0
