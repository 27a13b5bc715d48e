"""A census of the designed inputs of tests/fuse_statement.py: that they reach what they are for, checked without a device."""
import numpy as np
import pytest

import fuse_statement as fs
from fuse_statement import MEAN, RRF, SUM


@pytest.fixture(scope="module")
def cases():
    return {f: make() for f, make in fs.FAMILIES.items()}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_ties_pairs_and_the_cut(cases):
    c = cases["ties"]
    assert [fs.width(L) for L in c.lists] == [64, 64] and c.rrf_c == 60.0 and c.lists[0].weight == c.lists[1].weight
    how, min_lists, n_top = fs.CALLS["ties"][0]
    assert how == RRF and n_top % 2 == 1 and n_top < 64
    cnt, ids, score, mask, st = fs.fuse_statement(c.lists, c.n_ids, RRF, c.rrf_c, 1, 64)
    for q in range(len(cnt)):
        assert cnt[q] == 64 and (mask[q] == 3).all()
        b = bits(score[q])
        assert all(b[2 * k] == b[2 * k + 1] for k in range(32)) and len(set(b.tolist())) == 32      # 32 pairs of bit-equal scores
        assert all(ids[q, 2 * k] < ids[q, 2 * k + 1] for k in range(32))       # the id decides inside a pair
        assert {int(ids[q, 0]), int(ids[q, 1])} == {int(c.lists[0].item[q, 0]), int(c.lists[0].item[q, 63])}
    # the odd cut splits a pair: the last entry's partner is the first one left out
    cut = fs.fuse_statement(c.lists, c.n_ids, RRF, c.rrf_c, 1, n_top)
    assert np.array_equal(cut[1], ids[:, :n_top]) and (bits(score[:, n_top - 1]) == bits(score[:, n_top])).all()


def test_order_sensitive_sum(cases):
    c = cases["order"]
    designed = c.n_ids - 1
    seen = set()
    for q in range(len(c.lists[0].cnt)):
        vals = tuple(float(c.lists[l].score[q, list(c.lists[l].item[q]).index(designed)]) for l in range(3))
        assert sorted(vals) == [-1e300, 1.0, 1e300]
        want = (np.float64(vals[0]) + np.float64(vals[1])) + np.float64(vals[2])
        fwd = fs.scores(c.lists, c.n_ids, q, SUM, 0.0)[designed]
        rev = fs.scores(c.lists, c.n_ids, q, SUM, 0.0, reverse=True)[designed]
        assert fwd == (want, 7)
        seen.add((float(fwd[0]), float(rev[0])))
    assert (1.0, 0.0) in seen and (0.0, 1.0) in seen        # 1.0 in record order and 0.0 otherwise, and the other way round


def test_generic_rrf_share_that_an_unstable_sort_changes(cases):
    c = cases["generic"]
    assert len(c.lists) == 5 and len({L.weight for L in c.lists}) == 5
    n = differ = 0
    per_query_lists = set()
    for q in range(len(c.lists[0].cnt)):
        per_query_lists.add(sum(1 for L in c.lists if L.cnt[q] > 0))
        fwd, rev = fs.scores(c.lists, c.n_ids, q, RRF, c.rrf_c), fs.scores(c.lists, c.n_ids, q, RRF, c.rrf_c, reverse=True)
        for i in fwd:
            n += 1
            differ += bits(fwd[i][0]) != bits(rev[i][0])
    assert per_query_lists == {3, 4, 5}
    assert n > 1500 and differ / n >= 0.1, (differ, n)         # on random ranks about a quarter


def test_special_values(cases):
    c = cases["special"]
    s = np.concatenate([L.score.ravel() for L in c.lists])
    assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any()
    assert (s == 0.0).any() and np.signbit(s[s == 0.0]).any() and not np.signbit(s[s == 0.0]).all()
    assert ((np.abs(s) > 0) & (np.abs(s) < 2.2250738585072014e-308)).any()
    w = [L.weight for L in c.lists]
    assert min(w) < 0 and w[0] + w[1] == 0.0
    got = fs.fuse_statement(c.lists, c.n_ids, MEAN, 0.0, 1, 256)
    assert got[4][2] > 10                                   # den == 0.0, inf, NaN: dropped as non-finite
    assert not np.isnan(got[2]).any() and np.isfinite(got[2]).all()
    # query 0: zeros of both signs (a sum from 0.0 is never -0.0; 0.0 / a negative den is), selected by id, the sign bit kept
    z = got[2][0, :got[0][0]]
    assert len(z) > 4 and (z == 0.0).all() and np.signbit(z).any() and not np.signbit(z).all()
    assert (np.diff(got[1][0, :got[0][0]]) > 0).all()
    got = fs.fuse_statement(c.lists, c.n_ids, SUM, 0.0, 1, 256)
    assert got[4][2] > 5


def test_shapes(cases):
    c = cases["shapes"]
    assert [fs.width(L) for L in c.lists] == [1, 63, 64, 65, 1024]
    kinds = set()
    for L in c.lists:
        w = fs.width(L)
        for x in L.cnt:
            kinds.add("neg" if x < 0 else "zero" if x == 0 else "full" if x == w else "above" if x > w else "part")
    assert kinds == {"neg", "zero", "full", "above", "part"}
    allid = np.concatenate([L.item.ravel() for L in c.lists])
    assert (allid == -1).any() and (allid == c.n_ids).any() and (allid > c.n_ids).any()
    cand = fs.candidate_counts(c.lists, c.n_ids)
    assert cand[2] == 0 and cand[5] == 0 and cand[1] > 0 and cand[3] > 0 and cand[4] > 0 and cand[6] > 0     # empty between full
    q = 0                                                   # an id twice in one list: two records, one bit
    dup = int(c.lists[3].item[q, 2])
    recs = [r for r in fs.records(c.lists, c.n_ids, q) if r[0] == dup and r[1] == 3]
    assert len(recs) == 2
    assert {len(cs.lists) for cs in cases.values()} >= {1, 2, 16}
    ml = {(m, len(cases[f].lists)) for f, calls in fs.CALLS.items() for (_, m, _) in calls}
    assert any(m == 1 for m, n in ml) and any(m == 2 for m, n in ml) and any(m == n and n > 2 for m, n in ml)
    assert {n for calls in fs.CALLS.values() for (_, _, n) in calls} >= set(fs.N_TOPS)


def test_candidate_counts_around_every_n_top(cases):
    c = cases["one"]
    cand = fs.candidate_counts(c.lists, c.n_ids)
    assert cand == fs.CAND_COUNTS
    for n_top in fs.N_TOPS:
        assert any(x < n_top for x in cand) and any(x == n_top for x in cand) and (n_top == 1024 or any(x > n_top for x in cand))
    # above 1 024 candidates: the sixteen lists together
    assert max(fs.candidate_counts(cases["sixteen"].lists, cases["sixteen"].n_ids)) <= 200
    big = fs.candidate_counts(cases["shapes"].lists, cases["shapes"].n_ids)
    assert max(big) > 1024


def test_both_sides_of_the_block_route(cases):
    assert fs.total_width(cases["sixteen"].lists) == fs.BLOCK_RECORDS
    for f, c in cases.items():
        assert fs.total_width(c.lists) <= fs.BLOCK_RECORDS
        s = fs.on_sorted_route(c.lists)
        assert fs.total_width(s) > fs.BLOCK_RECORDS and len(s) <= fs.MAX_LISTS
        for q in range(len(c.lists[0].cnt)):
            assert fs.records(s, c.n_ids, q) == fs.records(c.lists, c.n_ids, q)
    assert fs.total_width(fs.on_sorted_route(cases["sixteen"].lists)) == fs.BLOCK_RECORDS + 1        # by padding a width
    assert len(fs.on_sorted_route(cases["ties"].lists)) > 2                                          # by the empty extra list


def test_the_statement_on_a_hand_made_call():
    cnt = np.array([3], np.int32)
    a = fs.FuseIn(cnt, np.array([[4, 2, 9]], np.int32), np.array([[3.0, 2.0, 1.0]]), 1.0)
    b = fs.FuseIn(cnt, np.array([[2, 7, 4]], np.int32), np.array([[5.0, 4.0, 0.5]]), 2.0)
    got = fs.fuse_statement([a, b], 10, SUM, 0.0, 1, 4)
    assert list(got[1][0]) == [2, 7, 4, 9] and list(got[2][0]) == [12.0, 8.0, 4.0, 1.0] and list(got[3][0]) == [3, 2, 3, 1]
    assert got[4] == [4, 0, 0, 4, 6]
    got = fs.fuse_statement([a, b], 10, MEAN, 0.0, 2, 4)
    assert list(got[1][0]) == [2, 4, -1, -1] and list(got[2][0]) == [4.0, 4.0 / 3.0, 0.0, 0.0] and got[4] == [4, 2, 0, 4, 6]
    got = fs.fuse_statement([a, b], 10, RRF, 0.0, 1, 2)
    assert list(got[1][0]) == [2, 4] and got[2][0, 0] == 0.5 + 2.0 and got[2][0, 1] == 1.0 + 2.0 / 3.0
