"""The census of the designed inputs of tests/test_gpu_uknn.py, taken on the CPU with the statement (tests/uknn_statement.py): every
case provably reaches what it is meant to reach, so a GPU run that passes has passed on these paths."""
import math

import numpy as np
import pytest

import peers_statement as ps
import uknn_statement as us


@pytest.fixture(scope="module")
def halves():
    return us.family_case("halves")


def test_bound_rating_and_the_means():
    assert [us.bound_rating(x) for x in (-3.0, 0.49, 0.5, 2.5, 4.49, 4.5, 7.0)] == [0.0, 0.0, 1.0, 3.0, 4.0, 5.0, 5.0]
    P = ps.Profiles.from_lists([[(0, 1.0), (2, 2.5), (-1, 100.0), (3, 100.0), (2, 4.0)], [], [(3, 9.0)]], 3)
    avg, cnt = us.means_statement(P)
    assert avg.tolist() == [2.5, 0.0, 0.0] and cnt.tolist() == [3, 0, 0]                # the valid rows only
    long = ps.Profiles.from_lists([[(k % 5, 0.5 * (k % 9)) for k in range(200)]], 5)   # more rows than lanes: halves sum exactly
    assert us.means_statement(long)[0][0] == sum(0.5 * (k % 9) for k in range(200)) / 200.0


def test_the_formula_on_a_case_worked_by_hand():
    """a = 3.0; neighbours (1, 0.5) holding item 7 as 4.0 and 5.0, (2, -0.25) holding it as 1.0: the query's mean is subtracted,
    OWN_MEAN subtracts the neighbour's"""
    P = ps.Profiles.from_lists([[(0, 3.0)], [(7, 4.0), (0, 1.0), (7, 5.0)], [(7, 1.0)]], 8)
    lists = (np.asarray([2], np.int32), np.asarray([[1, 2]], np.int32), np.asarray([[0.5, -0.25]]))
    avg, _ = us.means_statement(P)
    score, bound, n, status = us.predict_statement(P, lists, [3.0], avg, [0, 0], [7, 5])
    want = 3.0 + ((0.0 + 0.5 * 1.0 + 0.5 * 2.0) + -0.25 * -2.0) / (0.5 + 0.5 + 0.25)
    assert score.tolist() == [want, 3.0] and n.tolist() == [3, 0] and status.tolist() == [0, 0] and bound.tolist() == [5.0, 3.0]
    own = us.predict_statement(P, lists, [3.0], avg, [0], [7], us.OWN_MEAN)[0][0]
    m1 = 10.0 / 3.0
    assert own == 3.0 + ((0.5 * (4.0 - m1) + 0.5 * (5.0 - m1)) + -0.25 * 0.0) / 1.25


def test_the_families_reach_every_status_and_both_sides_of_a_wave(halves):
    c = halves
    for n_nb in us.N_NBS:
        cnt = c["lists"][n_nb][0]
        assert cnt[1] == 0 and cnt.max() >= n_nb                                        # a count of 0; full lists (one above n_nb)
    assert (c["lists"][200][0] > 65).sum() > 50 and (c["lists"][200][0] < 64).sum() >= 3
    tq, ti = us.pair_cases(c["P"], len(c["query"]))
    score, bound, n, status = us.predict_statement(c["P"], c["lists"][65], c["qavg"], c["avg"], tq, ti)
    assert set(status.tolist()) == {0, 1, 2, 3}
    assert ((status == 0) & (n > 0)).sum() > 100
    one = us.predict_statement(c["P"], c["lists"][1], c["qavg"], c["avg"], tq, ti)      # one neighbour: most pairs lack evidence
    assert ((one[3] == 0) & (one[2] == 0)).sum() > 100 and ((one[3] == 0) & (one[2] > 0)).sum() > 5
    assert (status[-4:] == 3).all() and (status[tq == 2][n[tq == 2] > 0] == 2).all()    # the zero sims: ZeroDivisionError
    held_twice = 0                                                                      # a neighbour holding the test item twice
    rows = us._rows_of(c["P"])
    for q, it in zip(tq[:-4].tolist(), ti[:-4].tolist()):
        held_twice += any(sum(1 for i, _ in rows[v] if i == it) > 1 for v, _ in us._list_of(c["lists"][65], q) if 0 <= v < c["P"].n_users)
    assert held_twice > 5
    own = us.predict_statement(c["P"], c["lists"][65], c["qavg"], c["avg"], tq, ti, us.OWN_MEAN)
    assert (own[0] != score).sum() > 100 and np.array_equal(own[3], status)


def test_the_nan_rating_of_the_magnitudes_family_raises_where_it_is_evidence():
    c = us.family_case("magnitudes")
    assert np.isnan(c["avg"]).sum() == 1
    tq, ti = us.pair_cases(c["P"], len(c["query"]), n=1500, extra=c["extra"])
    status = us.predict_statement(c["P"], c["lists"][200], c["qavg"], c["avg"], tq, ti)[3]
    assert (status == 2).sum() >= 5 and set(status.tolist()) == {0, 1, 2, 3}
    planted = [q for q in range(5, len(c["query"])) if c["lists"][200][0][q] > 0][1]
    assert c["lists"][200][1][planted, 0] == np.nonzero(np.isnan(c["avg"]))[0][0]
    assert c["extra"][0][0] == planted and status[0] == 2 and ((tq == planted) & (status == 0)).sum() > 0
    full = us.topn_statement(c["P"], c["P"], c["query"], c["lists"][200], c["qavg"], c["avg"], 5, full=True)
    assert full[4][2] > 0                                                               # candidates dropped as non-finite


def test_the_top_n_of_the_families_is_cut_and_the_rules_bite(halves):
    c = halves
    P, query, L = c["P"], c["query"], c["lists"][65]
    full = us.topn_statement(P, P, query, L, c["qavg"], c["avg"], 5, full=True)
    more, ties, longest = us.census(full[5], 5)
    assert more * 2 > len(query) and longest > 5
    kept = us.topn_statement(P, P, query, L, c["qavg"], c["avg"], 5, flags=us.KEEP_HELD)
    assert kept[4][0] > full[4][0] + 100                                                # held items among the candidates
    for ms in (2, 3):                                                                   # few neighbours: few records per item
        assert us.topn_statement(P, P, query, c["lists"][1], c["qavg"], c["avg"], 5, min_support=ms)[4][1] > 20
    assert us.topn_statement(P, P, query, L, c["qavg"], c["avg"], 5, min_support=3)[4][1] >= 10
    allow = np.random.RandomState(4).rand(P.n_items) < 0.6
    exclude = [[int(x) for x in np.random.RandomState(q).randint(0, P.n_items, 6)] + [-1, P.n_items] for q in range(len(query))]
    ruled = us.topn_statement(P, P, query, L, c["qavg"], c["avg"], 5, allow=allow, exclude=exclude, min_score=3.0)
    assert 0 < ruled[4][0] < full[4][0] and ruled[4][3] > 0 and ruled[4][5] < full[4][5]


def test_the_crowd_has_a_run_longer_than_257_records():
    P = us.crowd_profiles()
    L = us.lists_from_peers(P, P, [0, 5, 300], (300,), cap=1)[300]
    assert L[0][0] == 280                                                               # 280 neighbours of user 0
    avg, _ = us.means_statement(P)
    full = us.topn_statement(P, P, [0, 5, 300], L, us.gather_means(avg, [0, 5, 300]), avg, 3, full=True)
    item1 = [e for e in full[5][0] if e[0] == 1]
    assert item1 and item1[0][2] == 280 + 56 and us.census(full[5], 3)[2] > 257
    n = us.predict_statement(P, L, us.gather_means(avg, [0, 5, 300]), avg, [0, 0], [1, 0])[2]
    assert n.tolist() == [336, 280]


def test_the_tie_items_are_bit_equal_across_every_cut():
    P = us.tie_item_profiles()
    L = us.lists_from_peers(P, P, [0], (8,), cap=1)[8]
    assert L[0][0] == 7
    avg, _ = us.means_statement(P)
    for flags in (0, us.OWN_MEAN):
        full = us.topn_statement(P, P, [0], L, us.gather_means(avg, [0]), avg, 1024, flags=flags, full=True)
        kept = full[5][0]
        assert len(kept) == 596
        scores = [e[1] for e in kept if e[0] != 4]
        assert len(set(scores)) == 1 and [e[0] for e in kept if e[0] != 4] == list(range(5, 600))
        for n_top in (5, 256):
            assert us.census(full[5], n_top)[1] == 1                                   # equal scores across the cut
        assert kept[0][0] == 4 or kept[-1][0] == 4                                      # item 4 alone differs


def test_the_wide_item_space_needs_18_bits():
    P, active = us.wide_item_profiles()
    assert P.n_items > (1 << 17) and int(P.item.max()) == P.n_items - 1
    query = list(range(0, 200, 4))
    L = us.lists_from_peers(P, P, query, (50,), cap=1)[50]
    avg, _ = us.means_statement(P)
    full = us.topn_statement(P, P, query, L, us.gather_means(avg, query), avg, 10, full=True)
    got = set(e[0] for k in full[5] for e in k)
    assert P.n_items - 1 in got and us.census(full[5], 10)[0] > 40
    assert all(math.isfinite(e[1]) for k in full[5] for e in k)


def test_the_statement_gives_what_the_reference_recorded():
    import os
    g = us.golden_case(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uknn_small.json.gz"))
    score, bound, n, status = us.predict_statement(g["P"], g["lists"], g["qavg"], g["avg"], g["tq"], g["ti"])
    assert us.held_to_golden(g["want"], bound, status, g["tq"])
    assert sum(1 for w in g["want"] if isinstance(w, float)) > 100 and None in g["want"] and (n[status == 0] == 0).sum() > 3
    avg, _ = us.means_statement(g["P"])
    assert np.array_equal(avg, g["avg"])
