"""The statement of the allotment (tests/allot_statement.py) against itself: the synchronous rounds and the sequential
one-offer-at-a-time formulation give the same lists under every proposer order -- the refused set is the least fixed point of a
monotone operator -- and every outcome is stable.  Hand cases, and the census of the designed pools the device tests use."""
import numpy as np
import pytest

import allot_statement as al
from allot_statement import INT32_MAX, Pool, allot_rounds, allot_sequential, is_stable


def _tiny(seed):
    """Q <= 8, pool <= 6, I <= 7, caps 0..3; odd seeds: descending pools, even seeds: scores in {0, 1, 2} in any order (ties
    dominate); duplicates inside a pool, void ids and short counts included"""
    rng = np.random.RandomState(seed)
    Q, n_pool, I = rng.randint(1, 9), rng.randint(1, 7), rng.randint(1, 8)
    item = rng.randint(-1, I + 1, (Q, n_pool))
    if seed & 1:
        plain = -np.sort(-rng.random_sample((Q, n_pool)), axis=1)
    else:
        plain = rng.randint(0, 3, (Q, n_pool)).astype(np.float64)
    decay = rng.randint(0, 3, (Q, n_pool)).astype(np.float64)
    cnt = rng.randint(-1, n_pool + 2, Q)
    caps = rng.randint(0, 4, I)
    return Pool(cnt, item, plain, decay, I), int(rng.randint(1, n_pool + 1)), caps, int(rng.randint(0, 2))


@pytest.mark.parametrize("block", range(6))
def test_rounds_equal_sequential_under_every_order_and_are_stable(block):
    for seed in range(block * 500, block * 500 + 500):
        pool, n_top, caps, rank_by = _tiny(seed)
        R = allot_rounds(pool, n_top, item_cap=caps, rank_by=rank_by)
        for order in ("ascending", "descending", "random"):
            held = allot_sequential(pool, n_top, item_cap=caps, rank_by=rank_by, order=order, seed=seed)
            assert np.array_equal(held, R.held), (seed, order)
        assert is_stable(pool, n_top, R.held, item_cap=caps, rank_by=rank_by), seed
        al.check_allot_output(pool, n_top, R.lists())
        assert np.array_equal(al.held_mask(pool, R.cnt, R.pos), R.held)
        assert np.array_equal(R.taken, np.bincount(R.item[R.item >= 0], minlength=pool.n_items))
        assert (R.taken <= caps).all()


def test_order_key_is_the_score_order():
    s = np.array([np.inf, 3.0, 2e-310, 5e-324, 0.0, -0.0, -5e-324, -1.0, -np.inf])
    k = al.order_key(s)
    assert k[4] == k[5]                         # -0.0 equals 0.0
    assert (k[:4][1:] > k[:4][:-1]).all() and k[3] < k[4] and (k[5:][1:] > k[5:][:-1]).all()
    assert k.dtype == np.uint64


def test_hand_cases():
    """(a) two queries want item 0 first, cap 1, n_top 1: scores 5 and 7.  Query 1 (7) keeps it; query 0 moves on to item 1.
       Round 1 refuses (0, 0), round 2 is empty: 2 rounds, |R| = 1, one list changed.
    (b) the same with equal scores: the tie goes to the smaller query index, so query 0 keeps item 0 and query 1 moves on.
    (c) n_top 2, cap 1, three queries [0, 1], [0, 1], [0, 1] with scores q0: 3, 1; q1: 2, 3; q2: 1, 2.  Round 1: item 0 keeps q0 (3),
        item 1 keeps q1 (3); everything else is refused and no query has a position left: q0 = [0], q1 = [1], q2 = [].
        |R| = 4, 2 rounds, q2's pool was full and its list is short: stats[5] counts q1 too (one entry of two), and q0.
    (d) a void head: item -1 at position 0 is skipped without a refusal; cap 0 bars item 1 the same way."""
    a = Pool([2, 2], [[0, 1], [0, 2]], [[5.0, 1.0], [7.0, 1.0]], np.zeros((2, 2)), 3)
    R = allot_rounds(a, 1)
    assert R.pos.tolist() == [[1], [0]] and R.item.tolist() == [[1], [0]] and R.stats == [1, 2, 1, 0, 2, 0]
    b = Pool([2, 2], [[0, 1], [0, 2]], [[7.0, 1.0], [7.0, 1.0]], np.zeros((2, 2)), 3)
    R = allot_rounds(b, 1)
    assert R.pos.tolist() == [[0], [1]] and R.stats == [1, 2, 1, 0, 2, 0]
    R = allot_rounds(b, 1, qid=[1, 0])          # renumbered: query 1 is the smaller recipient
    assert R.pos.tolist() == [[1], [0]]
    c = Pool([2, 2, 2], [[0, 1]] * 3, [[3.0, 1.0], [2.0, 3.0], [1.0, 2.0]], np.zeros((3, 2)), 2)
    R = allot_rounds(c, 2)
    assert R.cnt.tolist() == [1, 1, 0] and R.pos.tolist() == [[0, -1], [1, -1], [-1, -1]]
    assert R.stats == [3, 2, 4, 0, 2, 3] and R.taken.tolist() == [1, 1]
    d = Pool([3], [[-1, 1, 2]], [[9.0, 8.0, 7.0]], np.zeros((1, 3)), 3)
    R = allot_rounds(d, 1, item_cap=[1, 0, 1])
    assert R.pos.tolist() == [[2]] and R.stats == [1, 1, 0, 2, 1, 0]
    R = allot_rounds(d, 3, cap=INT32_MAX)
    assert R.pos.tolist() == [[1, 2, -1]] and R.stats == [1, 2, 0, 1, 1, 1]


def test_census_of_the_designed_pools():
    chain = al.chain_pool(64)
    R = allot_rounds(chain, 1, cap=1)
    assert R.pos[:, 0].tolist() == [0] + [1] * 63 and R.stats[4] == 64 and R.stats[2] == 63
    assert is_stable(chain, 1, R.held)
    ladder = al.ladder_pool(257, 1024)
    R = allot_rounds(ladder, 1, cap=1)
    assert R.pos[:, 0].tolist() == list(range(257)) and R.stats[4] == 257 and R.stats[2] == 257 * 256 // 2
    crowd = al.crowd_pool()
    R = allot_rounds(crowd, 2, cap=1100)
    assert crowd.Q == 1500 and (crowd.item[:, 0] == 0).all()
    assert R.taken[0] == 1100 > 1024 and R.stats[2] == 400 and R.stats[4] == 2
    assert (R.pos[:1100, 0] == 0).all() and (R.pos[1100:, 0] == 1).all()
    for family in al.FAMILIES:
        p = al.designed_pool(65, 33, family, 3)
        caps = al.designed_caps(p.n_items, 4)
        assert set(np.unique(caps)) == {0, 1, 2, INT32_MAX}
        assert (p.cnt < 0).any() and (p.cnt > 33).any() and (p.item == -1).any() and (p.item == p.n_items).any()
        R = allot_rounds(p, 33, item_cap=caps)
        assert R.stats[2] > 0 and R.stats[3] > 0 and is_stable(p, 33, R.held, item_cap=caps)
    ties = al.designed_pool(65, 33, "signed_zero", 5)
    assert len(np.unique(al.order_key(ties.plain))) == 1 and np.signbit(ties.plain).any() and not np.signbit(ties.plain).all()
    rep = al.designed_pool(9, 33, "negative", 6, n_items=12, repeat=True)
    assert any(len(set(r)) < len(r) for r in rep.item.tolist())
    # a permuted input with the original numbers as qid is the same market
    p = al.designed_pool(65, 33, "all_equal", 7)
    perm = np.random.RandomState(8).permutation(65)
    A, B = allot_rounds(p, 1, cap=1), allot_rounds(p.permuted(perm), 1, cap=1, qid=perm)
    assert np.array_equal(A.pos[perm], B.pos) and not np.array_equal(allot_rounds(p.permuted(perm), 1, cap=1).pos, B.pos)
