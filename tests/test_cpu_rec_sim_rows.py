"""The designed inputs of tests/rec_sim_rows.py on the CPU: the statement by hand, the census of every family (what the input is
for, asserted on the plan's statement and on the CPU oracle's output, before a comparison with the GPU says anything about the
kernel it aims at), and the oracle (oracle.rec_sim: double-double sums) held to the statement (math.fsum) -- every row of the
value families, the chosen rows of the layout families -- with sim and ls compared as bit patterns (NaN = NaN)."""
import math

import numpy as np
import pytest

import rec_sim_rows as rs
from rec_sim_rows import CAPS, LAYOUT_FAMILIES, SMALL_TARGET, VALUE_FAMILIES, bits, same_doubles, same_row
from test_cpu_stage_a_layout import census

CAP = 50


# ------------------------------------------------------------------------------------------------------ the statement
def test_statement_on_a_hand_made_input():
    """five items, four users, cap = 2.  Norms: items 0 and 1 hold (3, 4) and (4, 3): 5 each; item 2 holds 1; item 3 is held
    twice by one user, (2, 2): sqrt(8); item 4 sits alone in a profile of one rating and forms no pair."""
    r = rs.from_profiles([[(0, 3.0), (1, 4.0)], [(0, 4.0), (1, 3.0), (2, 1.0)], [(3, 2.0), (3, 2.0)], [(4, 5.0)]], 5)
    norms = rs.rec_norms_statement(r.item, r.rating, 5)
    s8 = math.sqrt(8.0)
    assert norms == [5.0, 5.0, 1.0, s8, 5.0]
    rows = [rs.rec_row_statement(r.user_ptr, r.item, r.rating, norms, i, 2) for i in range(5)]
    assert [sorted(x) for x in rows] == [[1, 2], [0, 2], [0, 1], [3], []]
    # (0, 1): records (3, 4), (4, 3); inner = 24, n = 2 = cap: sim = 24 / 25.  Without (3, 4): 12 over sqrt((25 - 9) 25) = 20 and
    # over sqrt(25 (25 - 16)) = 15, each weighted by min(1, 2) / 2; without (4, 3) the same two values.  The farthest is 0.3
    sim = 1.0 * (24.0 / 25.0) * 2 / 2
    assert rows[0][1] == rows[1][0] == (sim, abs(1.0 * (12.0 / 20.0) * 1 / 2 - sim), 2)
    assert abs(1.0 * (12.0 / 15.0) * 1 / 2 - sim) < rows[0][1][1]
    # (0, 2): one record (4, 1): sim = 4 / (5 1) / 2; the variants are 0 / 3 and (norm 0) 0.0, both weighted by 0: ls = |sim|
    assert rows[0][2] == rows[2][0] == (1.0 * (4.0 / 5.0) * 1 / 2, 0.4, 1)
    assert rows[1][2] == rows[2][1] == (1.0 * (3.0 / 5.0) * 1 / 2, 0.3, 1)
    # (3, 3): one unordered pair of entries, listed in both orders: n = 2, inner = 4 + 4; either variant leaves 4 over
    # sqrt((8' - 4) 8'), 8' = fl(sqrt(8)^2)
    e8 = s8 * s8
    sim = 1.0 * (8.0 / e8) * 2 / 2
    assert rows[3][3] == (sim, abs(1.0 * (4.0 / math.sqrt((e8 - 4.0) * e8)) * 1 / 2 - sim), 2)
    assert rs.rec_rows_by_combinations(r.user_ptr, r.item, r.rating, norms, 2) == {(i, j): v for i in range(5) for j, v in rows[i].items()}
    # a negative argument of the square root gives NaN, NaN divides (it is truthy) and the maximum propagates it
    assert math.isnan(rs._pair_statement([(2.0, 1.0)], 1.0, 1.0, 2)[1]) and not math.isnan(rs._pair_statement([(1.0, 1.0)], 1.0, 1.0, 2)[1])
    assert rs.same_doubles([rs.NAN, 1.0, -0.0], [-rs.NAN, 1.0, -0.0]) and not rs.same_doubles([0.0], [-0.0])


def test_the_hash_and_the_probe_restated():
    assert rs.home_slot(1, 7) == 0x9E3779B1 >> 25 == 79 and rs.home_slot(2, 7) == ((2 * 0x9E3779B1) & 0xffffffff) >> 25 == 30
    assert rs.home_slot(1, 10) == 0x9E3779B1 >> 22
    same = [j for j in range(1, 2048) if rs.home_slot(j, 7) == 127][:3]
    assert sorted(rs.probe_slots(same, 7).values()) == [0, 1, 127]


# ------------------------------------------------------------------------------------------------------ value families
def _oracle_rows_equal_the_statement(r, O, norms, cap, rows):
    assert np.array_equal(bits(norms), bits(O.norm))
    for i in rows:
        want = rs.rec_row_statement(r.user_ptr, r.item, r.rating, norms, i, cap)
        assert same_row(rs.row_of(O.row_ptr, O.col, O.sim, O.ls, O.nij, i), want), i


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", VALUE_FAMILIES)
def test_value_family_oracle_equals_the_statement(name, cap):
    """every row, and the statement written with combinations() gives the same rows"""
    r, O, norms = rs.value_family(name, cap), rs.oracle_value(name, cap), rs.norms_of("value", name, cap)
    _oracle_rows_equal_the_statement(r, O, norms, cap, range(r.n_items))
    whole = rs.rec_rows_by_combinations(r.user_ptr, r.item, r.rating, norms, cap)
    assert len(whole) == len(O.col)
    for i in range(r.n_items):
        assert same_row(rs.row_of(O.row_ptr, O.col, O.sim, O.ls, O.nij, i), {j: v for (a, j), v in whole.items() if a == i})
    assert rs.sum_bits(r.rating, max(int(O.nij.max()), int(np.bincount(r.item).max()))) <= rs.SUM_BITS_MAX


def _abs_bits(a):
    return bits(np.abs(a))


def test_census_single():
    r = rs.value_family("single")
    assert np.bincount(r.item, minlength=r.n_items).tolist() == [1] * 60
    # the sign of fl(sqrt(fl(r r)))^2 - fl(r r): zero for every value (rec_sim_rows: why it cannot be negative)
    assert r.meta["sign"] == [0] * 60 and [rs.single_sign(v) for v in r.rating.tolist()] == [0] * 60
    assert np.any(r.rating != r.rating.astype(np.float32))
    for cap in CAPS:
        O = rs.oracle_value("single", cap)
        negative = sum(1 for a, b in zip(O.rows, O.col) if r.meta["sign"][a] < 0 or r.meta["sign"][b] < 0)
        assert len(O.col) == 120 and np.all(O.nij == 1) and int(np.isnan(O.ls).sum()) == negative == 0
        assert np.array_equal(bits(O.ls), _abs_bits(O.sim)) and np.all(O.sim > 0)         # n - 1 = 0: ls = |sim|


@pytest.mark.parametrize("cap", CAPS)
def test_census_cap_edges(cap):
    r, O = rs.value_family("cap_edges", cap), rs.oracle_value("cap_edges", cap)
    targets = r.meta["targets"]
    assert targets == {1: [1, 2, 3], 2: [1, 2, 3, 6], 50: [1, 2, 49, 50, 51, 150]}[cap]
    for t, n in enumerate(targets):
        assert O.nij[(O.rows == 2 * t) & (O.col == 2 * t + 1)].tolist() == [n]
    assert set(O.nij.tolist()) == set(targets) and not np.isnan(O.ls).any()
    weight = lambda n: min(n, cap) / cap
    assert any(weight(n) != weight(n - 1) for n in targets) and any(weight(n) == weight(n - 1) == 1.0 for n in targets)
    one = O.nij == 1
    assert one.any() and np.array_equal(bits(O.ls[one]), _abs_bits(O.sim[one]))           # variants weighted by 0
    two = O.nij == 2
    if cap == 1:           # n = 2: sim and the variants carry the same weight 1 -- the distance is the cosines' alone
        assert np.all(O.ls[two] < np.abs(O.sim[two]))


def test_census_self_pairs():
    r = rs.value_family("self_pairs")
    unordered = rs.unordered_self_pairs(r)
    assert unordered.tolist() == [1 + 6, 3, 1, 0, 0, 1, 1, 0]
    held = sorted(np.unique(np.repeat(np.arange(r.n_users), np.diff(r.user_ptr)) * 8 + r.item, return_counts=True)[1].tolist())
    assert {2, 3, 4} <= set(held)                                                         # an item 2, 3 and 4 times in a profile
    for cap in CAPS:
        O = rs.oracle_value("self_pairs", cap)
        for i in range(r.n_items):
            assert O.nij[(O.rows == i) & (O.col == i)].tolist() == ([2 * unordered[i]] if unordered[i] else [])
        assert O.col[O.rows == 0].tolist() == [0]                                         # only pairs with itself
        assert O.col[O.rows == 2].tolist() == [2, 3, 4, 5]                                # the self pair beside ordinary pairs
        assert len(O.col[O.rows == 7]) == 0 and O.norm[7] == 0.0


def test_census_signs_and_zeros():
    r, O = rs.value_family("signs_and_zeros"), rs.oracle_value("signs_and_zeros", CAP)
    pair = lambda a, b: (O.rows == a) & (O.col == b)
    assert bits(O.sim[pair(0, 1)]).tolist() == [0] and O.nij[pair(0, 1)].tolist() == [2]       # cancels to +0.0 exactly
    rec = rs.pair_records(r.user_ptr, r.item, r.rating, 2)[3]
    assert math.fsum(a * b for a, b in rec) == 2.0 ** -54                                      # a last-bit residue
    assert 0.0 < O.sim[pair(2, 3)][0] < 1e-17
    assert O.norm[4] == 0.0 and len(O.sim[O.rows == 4]) == 2 and not bits(O.sim[O.rows == 4]).any() and not bits(O.ls[O.rows == 4]).any()
    zero = r.rating == 0.0
    assert int((bits(r.rating[zero]) != 0).sum()) >= 3 and int((bits(r.rating[zero]) == 0).sum()) >= 3    # -0.0 and +0.0
    assert (O.sim < 0).any() and (O.sim > 0).any() and (r.rating < 0).any()
    assert np.any(r.rating != r.rating.astype(np.float32)) and 1.0 / 3.0 in r.rating.tolist()
    assert not np.isnan(O.ls).any()


def test_census_slot_chains():
    from test_cpu_stage_a_layout import plan_statement
    r, O = rs.value_family("slot_chains"), rs.oracle_value("slot_chains", CAP)
    partners, crowded, tail = r.meta["partners"], r.meta["crowded"], r.meta["tail"]
    assert O.col[O.rows == 0].tolist() == sorted(partners) and len(partners) == 17 and np.all(O.nij[O.rows == 0] == 1)
    for target in (768, SMALL_TARGET):        # the lightest item: every partner is summed in ITS table, 128 slots, one partition
        P = plan_statement(r.user_ptr, r.item, r.n_items, r.n_users + 2, target, dups=True)
        assert P.n[0] == 1 and P.Wp[0] == P.bound[0] == 17 and P.Q[0] == 1 and P.cls[0] == 1
    homes = [rs.home_slot(j, rs.CHAIN_LOG_SLOTS) for j in partners]
    h = homes[0]
    assert homes[:9] == [h] * 9 and homes[9:] == [126] * 3 + [127] * 5 and h + 9 < 126
    for order in (partners, partners[::-1]):
        slots = rs.probe_slots(order, rs.CHAIN_LOG_SLOTS)
        assert sorted(slots[j] for j in crowded) == list(range(h, h + 9))                      # a chain of nine
        assert sorted(slots[j] for j in tail) == [0, 1, 2, 3, 4, 5, 126, 127]                  # ... and one that wraps
        assert max((slots[j] - rs.home_slot(j, rs.CHAIN_LOG_SLOTS)) % 128 for j in partners) >= 7


def test_census_nan_rating():
    r = rs.value_family("nan_rating")
    assert int(np.isnan(r.rating).sum()) == 1 and np.isnan(r.rating[r.item == 0]).any()
    for cap in CAPS:
        O = rs.oracle_value("nan_rating", cap)
        of0 = (O.rows == 0) | (O.col == 0)
        assert np.isnan(O.norm[0]) and not np.isnan(O.norm[1:]).any()
        assert np.isnan(O.sim[of0]).all() and np.isnan(O.ls[of0]).all() and int(of0.sum()) == 9
        assert not np.isnan(O.sim[~of0]).any() and not np.isnan(O.ls[~of0]).any() and int((~of0).sum()) == 20


# ----------------------------------------------------------------------------------------------------- layout families
@pytest.mark.parametrize("name", LAYOUT_FAMILIES)
def test_layout_family_census_and_oracle_rows(name):
    """the plan without a heavy set, the domain of the sums, and the oracle's chosen rows against the statement"""
    r, O, norms = rs.layout_family(name), rs.oracle_layout(name), rs.norms_of("layout", name)
    P, Ps = rs.rec_plan(name, 768), rs.rec_plan(name, SMALL_TARGET)
    assert P.n_heavy == Ps.n_heavy == 0 and P.n_heavy_units == 0 and not P.heavy.any()
    assert np.array_equal(P.cls == 4, (P.n >= 2048) & (P.Wp > 0))
    assert np.any(r.rating != r.rating.astype(np.float32)) and np.any(r.rating != np.round(r.rating))
    assert rs.sum_bits(r.rating, max(int(O.nij.max()), int(P.n.max()))) <= rs.SUM_BITS_MAX
    if name not in ("wide_repeat",):
        assert Ps.Q.max() >= 4                                        # rows cut into many partitions at the small target
    rows = rs.chosen_rows(name)
    assert len(rows) >= 16 and all(P.n[i] > 0 for i in rows)
    assert {int(P.cls[i]) for i in rows if P.Q[i] >= 1} == {c for c in range(5) if ((P.cls == c) & (P.Q >= 1)).any()}
    _oracle_rows_equal_the_statement(r, O, norms, CAP, rows)
    # every pair is listed in both rows with the same values
    assert len(O.col) == int(O.row_ptr[-1]) and np.array_equal(np.bincount(O.col, minlength=r.n_items), np.diff(O.row_ptr))


def test_layout_families_reach_every_class_without_a_heavy_set():
    """on the plan's statement alone: every table class is populated, class 4 holds rows of 2 048 and 2 049 raters and the hub
    every user rates, and a class-4 row is cut into several partitions"""
    populated = set()
    for name in LAYOUT_FAMILIES:
        c = census(rs.rec_plan(name, 768))
        assert c["n_heavy"] == 0 and c["heavy_units"] == 0
        populated |= {k for k, v in c["rows"].items() if v > 0}
    assert populated == {0, 1, 2, 3, 4}
    P = rs.rec_plan("wide_few+fp64", 768)
    r = rs.layout_family("wide_few+fp64")
    assert {2048, 2049, r.n_users} <= set(P.n[P.cls == 4].tolist()) and 2047 not in P.n[P.cls == 4].tolist()
    assert census(rs.rec_plan("wide_few+fp64", 768))["rows"][4] == 6
    many = census(rs.rec_plan("wide_many+fp64", SMALL_TARGET))
    assert many["rows"][4] == 47 and many["wide_split"] == 24 and many["units"][4] == 71 and many["max_Q"] == 24
    # the reused families of test_cpu_stage_a_layout at the small target: rows of 114, 14, 24, 8, 125 and 58 partitions
    assert [census(rs.rec_plan(n, SMALL_TARGET))["max_Q"] for n in LAYOUT_FAMILIES[:6]] == [114, 14, 24, 8, 125, 58]
    # full_heavy has no item of 2 048 raters: without a heavy set its hubs are class-0 rows of up to 58 partitions, not class 4
    assert census(rs.rec_plan("full_heavy:chunks+fp64", 768))["rows"] == {4: 0, 0: 1017, 2: 191, 3: 96, 1: 95}


def test_census_wide_self():
    """the self pair of the item held three times: met 3 x 33 000 times, reported twice that; the hubs' pair beside it"""
    r, O, P = rs.layout_family("wide_self"), rs.oracle_layout("wide_self"), rs.rec_plan("wide_self", 768)
    X, (lo, hi) = r.meta["self_item"], r.meta["hubs"]
    assert rs.unordered_self_pairs(r)[X] == 3 * rs.SELF_USERS == 99000 > 65535
    assert O.nij[(O.rows == X) & (O.col == X)].tolist() == [198000]
    assert P.cls[X] == 4 and P.n[X] == 3 * rs.SELF_USERS and P.cls[lo] == 4
    assert O.nij[(O.rows == lo) & (O.col == hi)].tolist() == [66000] and O.nij[(O.rows == X) & (O.col == hi)].tolist() == [99000]
    assert X in rs.chosen_rows("wide_self") and lo in rs.chosen_rows("wide_self")


def test_census_wide_repeat():
    """every rater of the class-4 rows holds the row's item twice, with different ratings"""
    r, O, P = rs.layout_family("wide_repeat"), rs.oracle_layout("wide_repeat"), rs.rec_plan("wide_repeat", 768)
    H0, H1 = r.meta["hubs"]
    assert np.nonzero(P.cls == 4)[0].tolist() == [H0, H1] and P.n[[H0, H1]].tolist() == [2 * 2050, 2 * 2100]
    users = np.repeat(np.arange(r.n_users), np.diff(r.user_ptr))
    for h, raters in ((H0, 2050), (H1, 2100)):
        u, k = np.unique(users[r.item == h], return_counts=True)
        assert len(u) == raters >= 2048 and np.all(k == 2)
        a = r.rating[r.item == h][np.argsort(users[r.item == h], kind="stable")].reshape(-1, 2)
        assert np.all(a[:, 0] != a[:, 1])
        assert O.nij[(O.rows == h) & (O.col == h)].tolist() == [2 * raters]
    assert O.nij[(O.rows == H0) & (O.col == H1)].tolist() == [4 * 2050]
    assert H0 in rs.chosen_rows("wide_repeat") and H1 in rs.chosen_rows("wide_repeat")


# ------------------------------------------------------------------------------------------------------ storage order
@pytest.mark.parametrize("kind,name", [("value", "self_pairs"), ("value", "slot_chains"), ("layout", "wide_repeat"), ("layout", "fill+fp64")])
def test_oracle_does_not_depend_on_storage_order(kind, name):
    """users permuted, the entries of every profile permuted: the same bytes"""
    r = rs.value_family(name, CAP) if kind == "value" else rs.layout_family(name)
    O = rs.oracle_value(name, CAP) if kind == "value" else rs.oracle_layout(name)
    g = rs.shuffled(r, 99)
    assert not np.array_equal(g.item, r.item)
    G = rs.oracle_rec(g, CAP)
    assert np.array_equal(G.row_ptr, O.row_ptr) and np.array_equal(G.col, O.col) and np.array_equal(G.nij, O.nij)
    assert same_doubles(G.sim, O.sim) and same_doubles(G.ls, O.ls) and np.array_equal(bits(G.norm), bits(O.norm))
