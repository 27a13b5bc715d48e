"""The statement of the group lists (tests/group_statement.py; xmap_group_topn_rows in include/xmap_hip.h) on values worked by
hand: what tests/test_gpu_group.py holds the device to.  No device."""
import math
import struct

import numpy as np

import group_statement as gs
from group_statement import MAX, MEAN, MIN, expected_group


def _bits(x):
    return struct.pack("<d", x)


# three members, five items; (item, plain, decayed, now, held); decayed = plain - 0.25 keeps the two columns apart
PLAIN = {0: {0: 4.0, 1: 5.0, 2: 3.0, 3: 2.0, 4: 3.75},
         1: {0: 4.0, 1: 5.0, 2: 3.5, 3: 5.5, 4: 3.75},
         2: {0: 4.0, 1: 1.0, 2: 4.75, 3: 2.5, 4: 3.75}}
AVG = np.asarray([3.0, 3.0, 3.0, 3.25, 3.0, 2.0])


def _scored(plain=PLAIN):
    return {u: [(i, s, s - 0.25, 2, False) for i, s in sorted(d.items())] for u, d in plain.items()}


def _run(groups, how, scored=None, held=None, **kw):
    scored = _scored() if scored is None else scored
    held = [set(), set(), set()] if held is None else held
    kw.setdefault("n", 10)
    kw.setdefault("rank_by", 0)
    kw.setdefault("keep_held", False)
    return expected_group(scored, held, groups, AVG, kw.pop("n"), kw.pop("rank_by"), kw.pop("keep_held"), 66, how, len(AVG), **kw)


def test_mean_min_and_max_order_three_members_differently():
    order = {}
    for how in (MEAN, MIN, MAX):
        lists, stats = _run([[0, 1, 2]], how)
        order[how] = [c[0] for c in lists[0]]
        assert stats == [15, 0, 2, 5, 0, 0, 0, 5]
    # means 4, 11/3, 3.75, 10/3, 3.75: items 2 and 4 tie exactly (3 + 3.5 + 4.75 = 11.25 = 3 * 3.75), the index decides
    assert order[MEAN] == [0, 2, 4, 1, 3]
    assert order[MIN] == [0, 4, 2, 3, 1]
    assert order[MAX] == [3, 1, 2, 0, 4]
    lists, _ = _run([[0, 1, 2]], MEAN)
    by = {c[0]: c for c in lists[0]}
    assert by[2][1] == by[4][1] == 3.75 and by[1][1] == ((5.0 + 5.0) + 1.0) / 3.0 and by[3][1] == ((2.0 + 5.5) + 2.5) / 3.0
    assert by[1][2] == ((4.75 + 4.75) + 0.75) / 3.0                 # the decayed column by the same rule, separately
    assert [by[i][3] for i in range(5)] == [0, 2, 0, 0, 0]          # the least-happy member; all equal: the first
    # ranked by the decayed column the order is the decayed one
    lists, _ = _run([[0, 1, 2]], MIN, rank_by=1)
    assert [c[0] for c in lists[0]] == [0, 4, 2, 3, 1] and lists[0][0][2] == 3.75


def test_a_veto_removes_exactly_one_item_under_each_how():
    for how in (MEAN, MIN, MAX):
        full, _ = _run([[0, 1, 2]], how)
        lists, stats = _run([[0, 1, 2]], how, veto=1.5)             # only item 1 has a member score below 1.5
        assert [c[0] for c in lists[0]] == [c[0] for c in full[0] if c[0] != 1]
        assert stats[6] == 1 and stats[7] == 5
        assert _run([[0, 1, 2]], how, veto=1.0)[1][6] == 0          # equal to the score: it stays
        assert _run([[0, 1, 2]], how, veto=math.nextafter(1.0, 2.0))[1][6] == 1
    # the order of the drops: status 2, then the veto, then the floor
    scored = _scored()
    scored[2][1] = (1, None, None, 2, False)
    lists, stats = _run([[0, 1, 2]], MEAN, scored=scored, veto=2.25, min_score=3.8)
    assert stats[1] == 1 and stats[6] == 1 and stats[4] == 2 and [c[0] for c in lists[0]] == [0]
    scored[2][1] = (1, 1.0, 0.75, 67, False)                        # now > n_w: status 2 as well
    assert _run([[0, 1, 2]], MEAN, scored=scored)[1][1:3] == [1, 67]


def test_the_least_happy_member_on_a_tie_of_two():
    assert gs.least([2.0, 1.0, 1.0]) == 1 and gs.least([1.0, 1.0, 2.0]) == 0 and gs.least([0.0, -0.0]) == 0
    plain = {0: {0: 2.0}, 1: {0: 1.0}, 2: {0: 1.0}}
    lists, _ = _run([[0, 1, 2], [2, 1, 0], [0]], MAX, scored=_scored(plain))
    assert [l[0][3] for l in lists] == [1, 0, 0]


def test_a_repeated_member_acts_as_a_weight():
    lists, stats = _run([[0, 2], [0, 0, 2]], MEAN)
    once, twice = {c[0]: c[1] for c in lists[0]}, {c[0]: c[1] for c in lists[1]}
    assert once[1] == (5.0 + 1.0) / 2.0 and twice[1] == ((5.0 + 5.0) + 1.0) / 3.0
    assert stats[0] == 10 + 15                                      # scored once per listing
    lo, _ = _run([[0, 2], [0, 0, 2]], MIN)
    assert [c[:2] for c in lo[0]] == [c[:2] for c in lo[1]]         # min and max do not weigh


def test_a_ghost_member_and_a_member_without_evidence_predict_the_item_average():
    plain = {u: dict(d) for u, d in PLAIN.items()}
    del plain[1][3]                                                 # member 1 has no evidence for item 3
    lists, stats = _run([[0, 1, 2], [0, 7], [-1, 9], []], MEAN, scored=_scored(plain))
    by = {c[0]: c for c in lists[0]}
    assert by[3][1] == ((2.0 + 3.25) + 2.5) / 3.0 and by[3][2] == ((1.75 + 3.25) + 2.25) / 3.0
    assert by[3][3] == 0
    ghost = {c[0]: c for c in lists[1]}                             # user 7 does not exist: the average everywhere
    assert ghost[1][1] == (5.0 + 3.0) / 2.0 and ghost[1][3] == 1 and ghost[3][3] == 0
    assert lists[2] == [] and lists[3] == []                        # nobody with evidence: no candidates; no members: none
    assert stats[0] == 14 + 5 and stats[7] == 10 and stats[3] == 5
    # a non-finite average drops the candidate for a group with a member lacking evidence, and only for such a group
    avg = AVG.copy()
    avg[3] = np.inf
    lists, stats = expected_group(_scored(plain), [set()] * 3, [[0, 1, 2], [0, 2]], avg, 10, 0, False, 66, MEAN, len(avg))
    assert 3 not in [c[0] for c in lists[0]] and 3 in [c[0] for c in lists[1]] and stats[1] == 1


def test_held_items_exclusions_the_mask_and_the_floor():
    held = [{4}, set(), {0, 5}]
    lists, stats = _run([[0, 1], [1, 2], [1]], MEAN, held=held)
    assert [sorted(c[0] for c in l) for l in lists] == [[0, 1, 2, 3], [1, 2, 3, 4], [0, 1, 2, 3, 4]]
    assert stats[0] == (4 + 5) + (5 + 4) + 5                        # a member's own held item is not scored
    lists, stats = _run([[0, 1], [1, 2], [1]], MEAN, held=held, keep_held=True)
    assert all(len(l) == 5 for l in lists) and stats[0] == 25
    allow = np.asarray([True, False, True, True, True, True])
    lists, stats = _run([[0, 1, 2], [1]], MEAN, allow=allow, exclude=[[2, 2, -4, 99, 1], None])
    assert [[c[0] for c in l] for l in lists] == [[0, 4, 3], [3, 0, 4, 2]]
    assert stats[5] == 1 and stats[0] == 12 + 4 and stats[7] == 3 + 4   # the masked item 1 was no candidate to exclude
    lists, stats = _run([[0, 1, 2]], MEAN, min_score=3.75)          # the floor on a tie of aggregates: both stay
    assert [c[0] for c in lists[0]] == [0, 2, 4] and stats[4] == 2
    assert _run([[0, 1, 2]], MEAN, min_score=math.nextafter(3.75, 4.0))[1][4] == 4


def test_minus_zero_against_zero():
    z, mz = 0.0, -0.0
    assert _bits(gs.aggregate([z, mz], MIN)) == _bits(z) and _bits(gs.aggregate([mz, z], MIN)) == _bits(mz)
    assert _bits(gs.aggregate([z, mz], MAX)) == _bits(z) and _bits(gs.aggregate([mz, z], MAX)) == _bits(mz)
    assert _bits(gs.aggregate([mz], MEAN)) == _bits(mz)             # the sum starts from s_0, not from 0.0 + s_0
    assert _bits(gs.aggregate([mz, mz], MEAN)) == _bits(mz) and _bits(gs.aggregate([mz, z], MEAN)) == _bits(z)
    plain = {0: {0: -0.0}, 1: {0: 0.0}}
    scored = {u: [(i, s, s, 2, False) for i, s in d.items()] for u, d in plain.items()}
    for how, first in ((MIN, mz), (MAX, mz), (MEAN, mz)):
        lists, _ = _run([[0], [0, 1], [1, 0]], how, scored=scored)
        assert _bits(lists[0][0][1]) == _bits(first) and lists[0][0][3] == 0
        assert _bits(lists[1][0][1]) == _bits(z if how == MEAN else mz) and lists[1][0][3] == 0
        assert _bits(lists[2][0][1]) == _bits(z) and lists[2][0][3] == 0


def test_a_group_of_one_is_the_top_n_statement():
    from test_gpu_topn import expected
    rng = np.random.default_rng(5)
    scored = {}
    for u in range(6):
        items = sorted(rng.choice(40, size=int(rng.integers(0, 25)), replace=False).tolist())
        scored[u] = [(i, None, None, 3, bool(k % 5 == 0)) if k % 7 == 3 else
                     (i, float(np.round(rng.normal(3, 1), 1)), float(np.round(rng.normal(3, 1), 1)), int(rng.integers(2, 70)), bool(k % 5 == 0))
                     for k, i in enumerate(items)]
    held = [{c[0] for c in scored[u] if c[4]} for u in range(6)]
    queries = [3, 0, 5, 9, 1, 1, 2, 4, -1]
    avg = np.full(40, 3.0)
    for n, rank_by, keep_held in ((10, 0, False), (64, 1, True), (5, 1, False)):
        lists, stats = expected(scored, queries, n, rank_by, keep_held, 66)
        assert stats[1] > 0 and stats[2] > 66
        for how in (MEAN, MIN, MAX):
            got, gstats = expected_group(scored, held, [[u] for u in queries], avg, n, rank_by, keep_held, 66, how, 40)
            assert [[c[:3] for c in l] for l in got] == lists and all(c[3] == 0 for l in got for c in l)
            assert tuple(gstats[:4]) == tuple(stats) and gstats[4:7] == [0, 0, 0] and gstats[7] == stats[0]
