"""The statement of the peers calls (tests/peers_statement.py) on the CPU: the edges by hand at U = 6, I = 5, and the census of
every designed input tests/test_gpu_peers.py runs, so that the GPU test cannot pass vacuously."""
import math

import numpy as np
import pytest

import peers_statement as ps
from peers_statement import Profiles, peer_index_statement, peer_rows_statement, SAME, KEEP_SELF

I = 5
# user 0: item 1 twice; user 1: item 1 once, item 2; user 2: item 1 twice, an item -1 and an item I; user 3: no rows;
# user 4: item 3 with rating 0 (zero norm); user 5: item 2 with a NaN rating, item 4
ROWS = [[(1, 2.0), (1, 3.0), (4, 1.0)],
        [(1, 4.0), (2, 1.0)],
        [(1, 1.0), (-1, 9.0), (1, 2.0), (I, 9.0)],
        [],
        [(3, 0.0)],
        [(2, float("nan")), (4, 2.0)]]
P = Profiles.from_lists(ROWS, I)


def test_index_holder_order_and_invalid_rows():
    X = peer_index_statement(P)
    assert X["rows"] == 10                              # the rows with items -1 and I are not indexed
    assert X["hd_ptr"].tolist() == [0, 0, 5, 7, 8, 10]
    assert X["hd_user"].tolist() == [0, 0, 1, 2, 2, 1, 5, 4, 0, 5]     # a user who holds an item twice appears twice
    assert X["hd_x"].tolist()[:5] == [2.0, 3.0, 4.0, 1.0, 2.0]
    # norm2 is bilinear: user 0 = (2 + 3)^2 + 1, user 2 = (1 + 2)^2
    assert X["nrm"][0] == math.sqrt(26.0) and X["nrm"][2] == 3.0 and X["nrm"][3] == 0.0 and X["nrm"][4] == 0.0
    assert math.isnan(X["nrm"][5])


def test_duplicates_on_either_side_multiply_out():
    cnt, user, sim, common, stats = peer_rows_statement(P, P, [1, 0], 5, flags=SAME)
    # query 1 (item 1 once) against user 0 (twice): 2 records; against user 2 (twice): 2; user 5 through item 2: NaN, dropped
    assert user[0].tolist()[:2] == [2, 0] and common[0].tolist()[:2] == [2, 2] and cnt[0] == 2
    assert sim[0, 1] == (4.0 * 2.0 + 4.0 * 3.0) / (math.sqrt(17.0) * math.sqrt(26.0))        # 0.951
    assert sim[0, 0] == (4.0 * 1.0 + 4.0 * 2.0) / (math.sqrt(17.0) * 3.0)                    # 0.970
    # query 0 (twice) against user 2 (twice): 4 records; against user 1: 2; user 5 through item 4: NaN norm, dropped
    assert dict(zip(user[1].tolist(), common[1].tolist()))[2] == 4
    assert stats[2] == 2 and stats[5] == (5 + 2) + (5 + 5 + 2)


def test_self_is_the_norm_bit_for_bit():
    cnt, user, sim, common, stats, kept = peer_rows_statement(P, P, [0, 2], 5, flags=SAME | KEEP_SELF, full=True)
    X = peer_index_statement(P)
    for q, (u, rows) in enumerate(((0, [2.0, 3.0]), (2, [1.0, 2.0]))):
        me = [e for e in kept[q] if e[0] == u][0]
        recs = [a * b for a in rows for b in rows] + ([1.0] if u == 0 else [])
        dot = ps.dd_sum(recs)                           # dot(u, u): the records of u against its own rows
        assert math.sqrt(dot) == X["nrm"][u]            # ... is norm2(u), bit for bit
        assert me[1] == dot / (X["nrm"][u] * X["nrm"][u]) and me[2] == len(recs)
    without = peer_rows_statement(P, P, [0, 2], 5, flags=SAME)
    assert 0 not in without[1][0].tolist() and 2 not in without[1][1].tolist()
    assert 0 in user[0].tolist() and 2 in user[1].tolist()


def test_zero_norm_gives_zero_and_a_user_without_rows_gives_nothing():
    Q = Profiles.from_lists([[(3, 2.0)], []], I)
    cnt, user, sim, common, stats = peer_rows_statement(P, Q, [0, 1, 7, -1], 3)
    assert cnt.tolist() == [1, 0, 0, 0] and user[0, 0] == 4 and sim[0, 0] == 0.0 and common[0, 0] == 1
    assert user[1].tolist() == [-1, -1, -1] and sim[1].tolist() == [0.0] * 3 and common[1].tolist() == [0] * 3


def test_nan_is_dropped_and_counted():
    cnt, user, sim, common, stats = peer_rows_statement(P, P, [5], 4, flags=SAME)
    assert cnt[0] == 0 and stats[0] == 2 and stats[2] == 2        # users 1 (item 2) and 0 (item 4): the query's norm is NaN


def test_cap_and_min_common():
    a = peer_rows_statement(P, P, [1], 5, cap=1, flags=SAME)
    b = peer_rows_statement(P, P, [1], 5, cap=3, flags=SAME)
    assert b[2][0, 0] == 1.0 * a[2][0, 0] * 2.0 / 3.0 and b[3][0, 0] == 2
    c = peer_rows_statement(P, P, [1], 5, min_common=2, flags=SAME)
    assert c[0][0] == 2 and c[4][1] == 1 and c[4][0] == 3        # user 5 (one record) leaves by min_common before its NaN is met


def test_rules_order_mask_exclusion_floor():
    allow = np.ones(6, bool)
    allow[0] = False
    cnt, user, sim, common, stats = peer_rows_statement(P, P, [1], 5, flags=SAME, allow=allow, exclude=[[2, 2, 99, -4]])
    assert cnt[0] == 0 and stats[0] == 1 and stats[5] == 5         # records of users 1, 2, 2 (item 1), 1, 5 (item 2): none of user 0
    cnt, user, sim, common, stats = peer_rows_statement(P, P, [1], 5, flags=SAME, min_score=0.96)
    assert user[0].tolist()[:1] == [2] and stats[3] == 1


# ---------------------------------------------------------------------------------------------------- census of the GPU inputs
@pytest.mark.parametrize("family", ps.FAMILIES)
def test_census_random_families(family):
    """every case of the GPU test's families -- the same queries, both centrings, cap 1 and 5, n_top 1, 10, 64, 65"""
    Pf = ps.random_profiles(3, family)
    q = ps.family_queries(Pf.n_users)
    for c in (None, ps.item_means(Pf)):
        for cap in (1, 5):
            out = peer_rows_statement(Pf, Pf, q, 65, cap=cap, flags=SAME, centre=c, full=True)
            cens = [ps.census(out[5], n_top) for n_top in (1, 10, 64, 65)]
            assert all(more * 2 >= len(q) for more, _, _ in cens), (family, cap, cens)     # more kept candidates than n_top
            assert any(ties >= 1 for _, ties, _ in cens), (family, cap, cens)               # equal sims across a cut
            assert cens[0][2] > 4                                                           # a run longer than 4 records
            assert out[4][5] > 0
            if family == "magnitudes":
                assert out[4][2] > 0                                # the family's NaN rating: non-finite, dropped and counted
    it = Pf.item
    assert ((it < 0) | (it >= Pf.n_items)).sum() > 0
    dup = sum(len(set(r)) < len(r) for r in (it[Pf.ptr[u]:Pf.ptr[u + 1]].tolist() for u in range(Pf.n_users)))
    assert dup > 10


def test_item_means_exact_is_the_rounded_exact_sum():
    Pm = Profiles.from_lists([[(0, 0.1), (1, 1e16)], [(0, 0.2), (1, 1.0)], [(0, 0.3), (1, -1e16), (7, 5.0)], []], 3)
    got = ps.item_means_exact(Pm)
    assert got.tolist() == [math.fsum([0.1, 0.2, 0.3]) / 3.0, 1.0 / 3.0, 0.0]


def test_census_ties_and_popular():
    Pt, other = ps.tie_profiles()
    q = [other[0], 0, 1]
    out = peer_rows_statement(Pt, Pt, q, 64, flags=SAME, full=True)
    more, ties, longest = ps.census(out[5], 64)
    assert more >= 2 and ties >= 2 and longest > 4
    for k in ps.POPULAR_SIZES:
        Pp = ps.popular_profiles(k)
        assert sum(1 for u in range(250) if Pp.ptr[u + 1] - Pp.ptr[u] == 3) == 50
        out = peer_rows_statement(Pp, Pp, [1, 0], 1024, flags=SAME | KEEP_SELF, full=True)
        assert out[4][4] == k and out[3][0].max() == 5 and set(out[3][0, :k].tolist()) == {2, 4, 5} and len(out[5][0]) == k
        if k > 1024:
            assert out[5][0][1023][1] == out[5][0][1024][1]            # equal sims across the cut
    out = peer_rows_statement(Pp, Pp, [1], 5, flags=SAME, min_common=3, min_score=0.9)
    assert out[4][1] > 0 and out[4][3] > 0
