"""The census of the designed inputs of tests/test_gpu_fill.py (tests/fill_statement.py builds them): every condition that makes
them worth running is asserted here, on the host, none is assumed.

The +0.0 / -0.0 pair among the tied MEAN scores: a SUM is never -0.0 (a double-double sum starts from +0.0, and in
round-to-nearest x + y is -0.0 only when both are), so ratings that cancel, or that are all -0.0, give +0.0.  The DIVISION gives
it: a sum that is a negative denormal over two or more holders underflows to -0.0.  fill_statement.zero_index() holds such items
beside +0.0 ones; the key's `score + 0.0` makes them tie, the item index orders them, and pop_score keeps the -0.0 bits."""
import numpy as np
import pytest

import fill_statement as fs
from fill_statement import COUNT, FILL_WINDOW, MEAN


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def indexes():
    return {f: fs.design_index(f) for f in fs.FAMILIES}


def test_every_dyadic_sum_is_exact(indexes):
    """multiples of 2^-20 up to 2^10: any correct summation gives the same bits"""
    X = indexes["dyadic"]
    k = X.hd_x * 2.0 ** 20
    assert (k == np.round(k)).all() and (np.abs(X.hd_x) <= 2.0 ** 10).all()
    ints = np.round(k).astype(np.int64)
    exact = np.asarray([int(ints[X.hd_ptr[i]:X.hd_ptr[i + 1]].sum()) for i in range(X.n_items)], np.int64)
    assert np.abs(exact).max() < 2 ** 53 and abs(int(ints.sum())) < 2 ** 53
    S, G = fs.dd_sums(X.n_items, X.hd_ptr, X.hd_x)
    assert np.array_equal(bits(S), bits(exact / 2.0 ** 20 + 0.0))
    assert G == int(ints.sum()) / 2.0 ** 20
    assert np.array_equal(bits(S), bits(np.asarray([fs.fsum(X.hd_x[X.hd_ptr[i]:X.hd_ptr[i + 1]].tolist()) for i in range(X.n_items)])))


def test_the_kernel_shaped_sums_of_the_tenths_equal_fsum(indexes):
    """ratings k / 10: the double-double sums rounded once, added in the kernels' shape, are the correctly rounded sums for every
    item and for the total (TENTHS_SEED is chosen so)"""
    X = indexes["tenths"]
    assert not (X.hd_x * 2.0 ** 20 == np.round(X.hd_x * 2.0 ** 20)).all()
    S, G = fs.dd_sums(X.n_items, X.hd_ptr, X.hd_x)
    want = np.asarray([fs.fsum(X.hd_x[X.hd_ptr[i]:X.hd_ptr[i + 1]].tolist()) for i in range(X.n_items)])
    assert np.array_equal(bits(S), bits(want))
    assert G == fs.fsum(X.hd_x.tolist())
    for damping in fs.DAMPINGS:                 # and with them the statement's scores
        a = fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, MEAN, damping, 1)
        b = fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, MEAN, damping, 1, sums=(S, G))
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("family", fs.FAMILIES)
def test_ties_min_count_and_the_zero_pair(indexes, family):
    X = indexes[family]
    n = np.diff(X.hd_ptr)
    assert n.max() > 128 and (n == 0).sum() > 50                # more than one stride of the lanes; items nobody holds
    assert n[X.special["at_min"]] == 3 and n[X.special["below_min"]] == 2 and n[X.special["no_holder"]] == 0
    for how in (COUNT, MEAN):
        for min_count in fs.MIN_COUNTS:
            item, score, pos, counts = fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, how, 0.0, min_count)
            assert fs.n_ties(score, counts[0]) >= 100, (how, min_count)
            assert counts[0] + counts[1] + counts[2] == X.n_items and counts[1] == (n < min_count).sum() and counts[2] == 0
            assert pos[X.special["at_min"]] >= 0
            assert (pos[X.special["below_min"]] >= 0) == (min_count == 1)
            ranked = item[:counts[0]]
            s = score[:counts[0]]
            assert (np.diff(s) <= 0).all() and (np.diff(ranked)[np.diff(s) == 0] > 0).all()       # descending, index ascending on ties
            assert np.array_equal(pos[ranked], np.arange(counts[0])) and (item[counts[0]:] == -1).all()
    # ratings that cancel beside ratings that are all -0.0: both SUMS are +0.0 (see the module docstring), a tie by item index
    item, score, pos, counts = fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, MEAN, 0.0, 1)
    a, b = X.special["cancel"], X.special["zeros"]
    assert bits(score[pos[[a, b]]]).tolist() == [0, 0] and pos[b] == pos[a] + 1
    assert np.signbit(X.hd_x[X.hd_ptr[b]:X.hd_ptr[b + 1]]).all()
    S, _ = fs.dd_sums(X.n_items, X.hd_ptr, X.hd_x)
    assert not np.signbit(S).any() or (S[np.signbit(S)] != 0).all()     # no sum is -0.0


def test_the_zero_index_ties_plus_and_minus_zero():
    """the +0.0 / -0.0 pair in the tied scores of MEAN, damping 0: negative denormal sums over 2 and 3 holders underflow to -0.0 in
    the division, between items whose score is +0.0 with a smaller and a larger index; the tie is ordered by item index"""
    X = fs.zero_index()
    n = np.diff(X.hd_ptr)
    S, G = fs.dd_sums(X.n_items, X.hd_ptr, X.hd_x)
    want_S = np.asarray([fs.fsum(X.hd_x[X.hd_ptr[i]:X.hd_ptr[i + 1]].tolist()) for i in range(X.n_items)])
    assert np.array_equal(bits(S), bits(want_S)) and G == fs.fsum(X.hd_x.tolist())      # the kernel-shaped sums are the exact ones
    minus, plus = X.special["minus"], X.special["plus"]
    assert all(S[i] == -fs.TINY and n[i] >= 2 for i in minus) and all(bits(S[[i]])[0] == 0 for i in plus)
    item, score, pos, counts = fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, MEAN, 0.0, 1)
    assert counts == (6, 0, 0) and item.tolist() == [4, 0, 1, 2, 3, 5]
    assert bits(score).tolist() == bits([2.0, 0.0, -0.0, 0.0, -0.0, -1.0]).tolist()
    assert plus[0] < minus[0] < plus[1] < minus[1]              # +0.0 with a smaller and a larger index around each -0.0
    same = fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, MEAN, 0.0, 1, sums=(S, G))
    assert np.array_equal(item, same[0]) and np.array_equal(bits(score), bits(same[1]))
    # without `+ 0.0` in the key the -0.0 items would sort behind every +0.0 item: the order the statement must NOT give
    assert item.tolist() != [4, 0, 2, 1, 3, 5]
    assert fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, MEAN, 0.0, 3)[0].tolist()[:2] == [2, 3]      # min_count 3: +0.0 then -0.0


def test_the_overflowing_index():
    X = fs.overflow_index()
    S, G = fs.dd_sums(X.n_items, X.hd_ptr, X.hd_x)
    assert not np.isfinite(S[0]) and not np.isfinite(G) and S[4] == 5.0
    assert fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, MEAN, 0.0, 1)[3] == (0, 1, 4)
    assert fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, MEAN, 25.0, 3)[3] == (0, 4, 1)
    assert fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, COUNT, 0.0, 1)[3] == (4, 1, 0)
    sums = fs.pop_statement(X.n_items, X.hd_ptr, X.hd_x, MEAN, 0.5, 1, sums=(S, G))
    assert sums[3] == (0, 1, 4)


@pytest.fixture(scope="module")
def D():
    return fs.design_fill()


def _first_fill(D, q, n_top, **kw):
    """the rank position of the first fill of query q (None: none)"""
    lists = fs.lists_for(D, n_top)
    out = fs.fill_statement(D.query_user, n_top, 0, D.n_users, D.n_items, D.prof_ptr, D.prof_item, D.item_avg, D.n_ranked, D.pop_item,
                            D.n_pop_items, *lists, **kw)
    c0 = lists[0][q]
    return (int(D.pop_pos[out[1][q, c0]]) if out[0][q] > c0 else None), out


def test_the_window_edges(D):
    W = FILL_WINDOW
    assert D.n_ranked > 2 * W and D.n_pop_items >= 2 * W + 100
    held = lambda u: set(D.prof_item[D.prof_ptr[u]:D.prof_ptr[u + 1]].tolist())
    for name, k in (("w-1", W - 1), ("w", W), ("w+1", W + 1)):
        q = D.names.index(name)
        assert held(D.query_user[q]) == set(D.pop_item[:k].tolist())
        first, out = _first_fill(D, q, 10, exclude=D.exclude)
        assert first == k                       # the last position of window 0, the first and the second of window 1
        assert out[0][q] == 10
    rows = np.diff(D.prof_ptr)
    assert sorted(rows)[-4:-1] == [W - 1, W, W + 1]
    assert not (np.diff(D.prof_item[D.prof_ptr[0]:D.prof_ptr[1]]) > 0).all()      # row order, not sorted by item


def test_the_queries_of_the_census(D):
    names, qu = D.names, D.query_user
    for n_top in fs.N_TOPS:
        cnt, item, plain, decay = fs.lists_for(D, n_top)
        out = fs.fill_statement(qu, n_top, 0, D.n_users, D.n_items, D.prof_ptr, D.prof_item, D.item_avg, D.n_ranked, D.pop_item,
                                D.n_pop_items, cnt, item, plain, decay, exclude=D.exclude)
        q = names.index("cover")                # held + listed + excluded cover the ranking: the list stays short
        u = qu[q]
        covered = set(D.prof_item[D.prof_ptr[u]:D.prof_ptr[u + 1]].tolist()) | set(item[q, :cnt[q]].tolist()) | set(D.exclude[q])
        assert set(D.pop_item[:D.n_ranked].tolist()) <= covered
        assert cnt[q] < n_top and out[0][q] == cnt[q] and out[5][3] >= 1
        q = names.index("empty")
        assert cnt[q] == 0 and out[0][q] == n_top and (out[4][q] == 1).all()      # n_top fills from an empty list (64 at n_top = 64)
        q = names.index("one")
        assert cnt[q] == n_top - 1 and out[0][q] == n_top and (out[4][q] == 1).sum() == 1
        q = names.index("full")
        assert cnt[q] == n_top and (out[4][q] == 0).all()
        assert all(np.array_equal(a[q], b[q]) for a, b in zip(out[:4], (cnt, item, plain, decay)))
        assert out[5][0] == (cnt < n_top).sum() and out[5][0] == out[5][1] + out[5][3] and out[5][2] == (out[4] == 1).sum()
    assert qu[names.index("anon")] == -1 and qu[names.index("beyond")] == D.n_users
    a, b, c = names.index("one"), names.index("one-ex"), names.index("one-ex2")     # a repeated query, its own exclusion list each time
    assert qu[a] == qu[b] == qu[c] and D.exclude[b] != D.exclude[c] and D.exclude[b] and D.exclude[c]
    ex = D.exclude[b]
    assert min(ex) < 0 and max(ex) >= D.n_items and len(set(ex)) < len(ex)          # ids outside the id space, repeated ids
    q = names.index("twice")
    row = D.prof_item[D.prof_ptr[qu[q]]:D.prof_ptr[qu[q] + 1]].tolist()
    assert len(set(row)) < len(row)
    q = names.index("held")
    row = D.prof_item[D.prof_ptr[qu[q]]:D.prof_ptr[qu[q] + 1]].tolist()
    assert set(fs.lists_for(D, 10)[1][q, :2].tolist()) <= set(row)                  # listed and held (KEEP_HELD on the top-N side)
    q = names.index("batch")
    assert D.n_pop_items < D.n_items and (fs.lists_for(D, 10)[1][q, :2] >= D.n_pop_items).all()
    assert (D.pop_pos == -1).sum() == D.n_pop_items - D.n_ranked > 0
    assert len(qu) > 4 * 8                      # more than a few blocks of four waves


def test_the_masks_and_the_short_ranking(D):
    half, one = D.masks["half"], D.masks["one-percent"]
    assert not half[:96].any() and D.pop_item[0] < 96           # the head of the ranking is masked: the compaction shifts every position
    assert (fs.mask_words(half)[:3] == 0).all()
    assert D.n_items % 32 != 0 and fs.mask_words(half)[-1] >> (D.n_items % 32) == (1 << (32 - D.n_items % 32)) - 1      # garbage beyond
    assert 0 < one.sum() < 0.02 * D.n_items
    first, out = _first_fill(D, D.names.index("empty"), 64, allow=one)
    assert out[0][D.names.index("empty")] == 64 and D.pop_pos[out[1][D.names.index("empty"), 63]] > FILL_WINDOW     # past window 0 unmasked
    n_ranked, pop_item, pop_pos = fs.short_ranking(D)
    lists = fs.lists_for(D, 64)
    out = fs.fill_statement(D.query_user, 64, 0, D.n_users, D.n_items, D.prof_ptr, D.prof_item, D.item_avg, n_ranked, pop_item,
                            D.n_pop_items, *lists)
    q = D.names.index("empty")
    assert out[0][q] == n_ranked < 64 and out[5][3] > 0         # a ranking shorter than the need
