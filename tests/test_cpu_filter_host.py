"""The host side of the eligibility rules: xmap.engine.filters packs the mask and the exclusion lists in the layouts of
xmap_rec_filter, and tests/filter_statement.py states the rules the GPU tests compare against.  Both on hand-worked cases."""
import numpy as np
import pytest

from filter_statement import allowed, expected_filtered


def _bits(on, n):
    pad = np.zeros((n + 31) // 32 * 32, np.uint8)
    pad[:n] = on
    return np.packbits(pad, bitorder="little").view("<u4")


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 100, 1 << 12])
def test_pack_mask_against_packbits(n):
    from xmap.engine.filters import pack_mask
    rng = np.random.default_rng(n)
    on = rng.integers(0, 2, n).astype(bool)
    want = _bits(on, n)
    got = pack_mask(on, n)
    assert got.dtype == np.uint32 and got.shape == ((n + 31) // 32,) and np.array_equal(got, want)
    ids = rng.permutation(np.nonzero(on)[0])
    assert np.array_equal(pack_mask(np.concatenate([ids, ids[:3]]), n), want)             # any order, repeats
    assert np.array_equal(allowed(got, n), on)                                              # the statement reads it back


def test_pack_mask_edges():
    from xmap.engine.filters import pack_mask
    assert pack_mask([], 40).tolist() == [0, 0] and pack_mask(np.zeros(0, np.int64), 0).shape == (0,)
    assert pack_mask([39], 40).tolist() == [0, 1 << 7]                                      # the id at n - 1
    assert pack_mask([31, 32], 64).tolist() == [1 << 31, 1]
    assert pack_mask([-1, 40, 41, 10 ** 12, 3], 40).tolist() == [1 << 3, 0]                 # out of range: ignored
    assert pack_mask(np.ones(33, bool), 33).tolist() == [0xffffffff, 1]                     # nothing set at or beyond n
    with pytest.raises(ValueError):
        pack_mask(np.ones(5, bool), 6)
    with pytest.raises(ValueError):
        pack_mask([1.5], 6)


def test_exclusion_csr():
    from xmap.engine.filters import exclusion_csr
    ptr, ids = exclusion_csr([[3, 1, 3], [], None, (7,), np.asarray([-1, 9], np.int64)])
    assert ptr.dtype == np.int64 and ids.dtype == np.int32
    assert ptr.tolist() == [0, 3, 3, 3, 4, 6] and ids.tolist() == [3, 1, 3, 7, -1, 9]
    ptr, ids = exclusion_csr([[], None])
    assert ptr.tolist() == [0, 0, 0] and ids.shape == (0,) and ids.dtype == np.int32
    ptr, ids = exclusion_csr([])
    assert ptr.tolist() == [0] and ids.shape == (0,)
    with pytest.raises(ValueError):
        exclusion_csr([[1 << 31]])


# {query key: [(id, plain, decayed, now, held)*]}: key 0 has five candidates, id 2 held, id 4 without numbers (status 2)
SCORED = {0: [(1, 3.0, 1.0, 2, False), (2, 5.0, 5.0, 2, True), (3, 3.0, 4.0, 3, False), (4, None, None, 2, False), (6, 2.0, 2.5, 9, False)],
          1: [(1, 1.0, 1.0, 2, False)]}


def test_statement_a_held_item_that_is_also_excluded_does_not_count():
    # without keep the held id 2 has left before the exclusions: only id 3 counts as removed
    lists, stats = expected_filtered(SCORED, [0], 10, 0, False, 66, 8, exclude=[[2, 3]])
    assert [c[0] for c in lists[0]] == [1, 6] and stats == (3, 1, 9, 3, 0, 1)
    # with keep it is a candidate, and its exclusion counts
    lists, stats = expected_filtered(SCORED, [0], 10, 0, True, 66, 8, exclude=[[2, 3]])
    assert [c[0] for c in lists[0]] == [1, 6] and stats == (3, 1, 9, 3, 0, 2)
    # no rule: the unfiltered numbers, [5] = their [0] minus this [0]
    assert expected_filtered(SCORED, [0], 10, 0, True, 66, 8)[1] == (5, 1, 9, 5, 0, 0)


def test_statement_a_repeated_exclusion_counts_once_and_lists_go_by_query():
    lists, stats = expected_filtered(SCORED, [0, 1, 0], 10, 0, False, 66, 8, exclude=[[1, 1, -1, 8, 100, 1], None, [7]])
    assert [[c[0] for c in l] for l in lists] == [[3, 6], [1], [1, 3, 6]]          # the same key twice, another list; 7 is no candidate
    assert stats == (3 + 1 + 4, 2, 9, 4, 0, 1)
    # the mask acts behind the exclusions: id 1 is excluded AND masked for query 0 -- once
    mask = np.ones(8, bool)
    mask[[1, 6]] = False
    lists, stats = expected_filtered(SCORED, [0, 1], 10, 0, False, 66, 8, allow=mask, exclude=[[1], []])
    assert [[c[0] for c in l] for l in lists] == [[3], []] and stats == (2, 1, 3, 2, 0, 3)
    words = np.asarray([0xffffff00 | 0b10111101], np.uint32)                        # the same mask, garbage beyond n = 8
    assert expected_filtered(SCORED, [0, 1], 10, 0, False, 66, 8, allow=words, exclude=[[1], []]) == (lists, stats)


def test_statement_a_floor_exactly_at_a_score():
    # plain: ids 1 and 3 score 3.0 = the floor, both kept, id order; id 6 (2.0) is below; id 4 has status 2: [1], never [4]
    lists, stats = expected_filtered(SCORED, [0], 10, 0, False, 66, 8, min_score=3.0)
    assert lists[0] == [(1, 3.0, 1.0), (3, 3.0, 4.0)] and stats == (4, 1, 9, 4, 1, 0)
    # decayed: id 1 (1.0) and id 6 (2.5) fall below the same floor, id 3 (4.0) stays
    lists, stats = expected_filtered(SCORED, [0], 10, 1, False, 66, 8, min_score=3.0)
    assert lists[0] == [(3, 3.0, 4.0)] and stats == (4, 1, 9, 4, 2, 0)
    # a short table drops id 6 (now 9 > 4) as status 2 before the floor sees it
    assert expected_filtered(SCORED, [0], 10, 0, False, 4, 8, min_score=3.0)[1] == (4, 2, 9, 4, 0, 0)
    # +inf: nothing is kept, [4] = scored - dropped; the cut at n
    assert expected_filtered(SCORED, [0], 10, 0, True, 66, 8, min_score=np.inf) == ([[]], (5, 1, 9, 5, 4, 0))
    assert expected_filtered(SCORED, [0], 1, 0, False, 66, 8, min_score=3.0)[0] == [[(1, 3.0, 1.0)]]
