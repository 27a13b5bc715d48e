"""A designed input for the large keys of the tile sort (csrc/tilesort.h).  Level B of the sort writes the records of a large key
(at least 2^ts_log records) in their final form itself -- the mirrored halves of the CSR in tri_mirror.hip, the rater records
and their W+ in tri_layout.hip -- while the small parts of the same chunk still go to the buffer level C reads.  What that
path can get wrong, and the inputs of test_cpu_tilesort_shapes.py do not reach: several large keys in one level-A bucket (and
so in one chunk), a key exactly at the threshold next to one just below it, odd fragment lengths, chunks that hold both kinds
of records, rows whose mirrored half does not start at the row's start.  The builder `hubs`, the conditions it has to meet
(asserted here with the NumPy statement of the geometry, before tests/test_gpu_tilesort_finish.py compares anything with the
GPU) and its AlterEgo-like twin for the 24- and 32-byte records.

  hubs    3 000 users over 2 x 1 500 items.  Four consecutive item indices near the end of the item range are rated by 2 048,
          2 047, 2 401 and 2 600 users (the last strictly the most): three large keys of the rater records, the first exactly
          at the threshold, its neighbour one record short of it, the third with an odd count, the last two in consecutive
          tiles.  The generator's own items stay far below the threshold, so the first level-A bucket has no large key, and the
          last bucket, which is not full, holds the hubs' 7 049 records among few others.  Every other item is a lighter
          partner of the hubs, so they are large keys of the mirror as well, in one bucket, and all but the heaviest have
          pairs of their own (with the heavier hubs) in front of their mirrored half.
  rows    `hubs` as AlterEgo-like rows, built as test_cpu_tilesort_shapes.rows builds its input: fp64 ratings, items repeated
          in a profile.  The heaviest hub is the last item of the users it was added to, so it is among the rows paired with
          themselves.
"""
import functools

import numpy as np
import pytest

from test_cpu_stage_a_layout import CAP, METHODS, with_exact_raters
from test_cpu_tilesort_shapes import CH_NARROW, CH_OTHER, mirrored_counts, ts_tables, with_unrated_blocks

THRESHOLD = 2048                                   # 2^ts_log of every geometry below (asserted)
HUB_COUNTS = (THRESHOLD, THRESHOLD - 1, 2401, 2600)     # raters of the four consecutive indices, in index order
FIRST_HUB = 2960                                   # index (before the unrated block goes in) of the first of the four
PAD = (100, 20)                                    # (in front of item, unrated indices): moves the hubs inside their tiles


@functools.lru_cache(maxsize=None)
def hubs():
    """-> (ratings, indices of the four hub items)"""
    from xmap.engine import synth
    r = synth.make_two_domain(53, 3000, 1500, 1500, overlap=0.5, d_min=38, mu=2.5, sigma=0.6, zipf=0.5)
    assert r.n_items > FIRST_HUB + len(HUB_COUNTS)
    r = with_exact_raters(r, {FIRST_HUB + x: c for x, c in enumerate(HUB_COUNTS)}, 530)
    g, item_map = with_unrated_blocks(r, (PAD,))
    return g, tuple(int(item_map[FIRST_HUB + x]) for x in range(len(HUB_COUNTS)))


def rows_of(r):
    """r as AlterEgo-like rows -> (user_ptr, item, rating (fp64), n_items), as test_cpu_tilesort_shapes.rows: every 7th user
    holds its first item twice more, every 21st its last item once more; ratings in thirds and eighths"""
    d = np.diff(r.user_ptr)
    u = np.repeat(np.arange(r.n_users, dtype=np.int64), d)
    first = np.r_[True, u[1:] != u[:-1]]
    last = np.r_[u[1:] != u[:-1], True]
    ex, ex2 = np.nonzero(first & (u % 7 == 0))[0], np.nonzero(last & (u % 21 == 0))[0]
    ra = r.rating.astype(np.float64)
    ra = ra + (np.arange(len(ra)) % 3) / 3.0
    uu = np.concatenate([u, u[ex], u[ex], u[ex2]])
    it = np.concatenate([r.item, r.item[ex], r.item[ex], r.item[ex2]])
    ra = np.concatenate([ra, ra[ex] * 0.5, ra[ex] * 0.75 + 0.125, ra[ex2] / 3.0])
    o = np.argsort(uu, kind="stable")
    ptr = np.zeros(r.n_users + 1, np.int64)
    np.cumsum(np.bincount(uu, minlength=r.n_users), out=ptr[1:])
    return ptr, it[o].astype(np.int32), ra[o], r.n_items


@functools.lru_cache(maxsize=None)
def rows():
    return rows_of(hubs()[0])


@functools.lru_cache(maxsize=None)
def oracle_sim(method):
    """the CPU oracle's stage A on `hubs`, computed once and shared"""
    from oracle import xmap_oracle as xo
    r = hubs()[0]
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
    return T, xo.item_sim(T, method, CAP, nthreads=8)


@functools.lru_cache(maxsize=None)
def oracle_rows():
    """the CPU oracle's RecommenderSim on `rows`, computed once and shared"""
    from oracle import xmap_oracle as xo
    ptr, item, rating, I = rows()
    return xo.rec_sim(ptr, item, rating, I, CAP)


def own_counts(n, row_ptr, col):
    """kept pairs per LIGHTER item (the own half of its row; a pair of a row with itself is in it)"""
    I = len(row_ptr) - 1
    row = np.repeat(np.arange(I, dtype=np.int64), np.diff(row_ptr))
    col = np.asarray(col, np.int64)
    lighter = (n[col] > n[row]) | ((n[col] == n[row]) & (col >= row))
    return np.bincount(row[lighter], minlength=I)


def large_share(G, count):
    """per level-A bucket: (records, records of large keys)"""
    rec = np.bincount(G.bucket, weights=count, minlength=G.NA).astype(np.int64)
    big = np.bincount(G.bucket, weights=np.where(G.large, count, 0), minlength=G.NA).astype(np.int64)
    return rec, big


def test_hubs_layout():
    """the rater records (236 440 over 3 020 item indices, key weight 19, 144 tiles in 2 level-A buckets): three large keys in
    tiles 137, 139 and 140 of the last bucket, which is not full -- 7 049 of its 27 512 records are theirs; none among the
    208 928 records of the first bucket"""
    r, hub = hubs()
    n = np.bincount(r.item, minlength=r.n_items)
    G = ts_tables(n)
    assert G.ts_log == 11 and 1 << G.ts_log == THRESHOLD and G.NA >= 2 and r.n_users == 3000
    assert hub == tuple(range(hub[0], hub[0] + 4)) and tuple(int(n[h]) for h in hub) == HUB_COUNTS
    assert np.sort(n)[-2] < n[hub[3]]                                         # strictly the most raters
    # exactly at the threshold: large; one record short of it: not
    assert n[hub[0]] == THRESHOLD and G.large[hub[0]] and n[hub[1]] == THRESHOLD - 1 and not G.large[hub[1]]
    assert G.large.sum() >= 3 and G.large[[hub[0], hub[2], hub[3]]].all()
    # two large keys in consecutive tiles of one bucket; a large key is the last key of its tile
    assert G.tile[hub[3]] == G.tile[hub[2]] + 1 and G.bucket[hub[3]] == G.bucket[hub[2]] == G.bucket[hub[0]]
    assert all(G.tile[h + 1] > G.tile[h] for h in (hub[0], hub[2]))
    assert n[hub[2]] % 2 == 1                                                 # fragments of odd length
    rec, big = large_share(G, n)
    assert np.any((big == 0) & (rec > CH_NARROW))                              # a bucket of several chunks without a large key
    b = G.bucket[hub[3]]
    assert 0.2 * rec[b] <= big[b] <= 0.8 * rec[b] and rec[b] > 2 * CH_NARROW   # chunks that hold both kinds of records
    assert r.nnz % CH_NARROW != 0


@pytest.mark.parametrize("method", METHODS)
def test_hubs_mirror(method):
    """the kept pairs by heavier item (2.43 million in 12 level-A buckets; nearly every pair of items is kept, so the 270 items
    with at least 2 048 lighter partners are all large keys, several in every bucket): the four hubs have 2 997, 2 996, 2 998
    and 2 999 mirrored entries in the last bucket, behind own halves of 2, 3, 1 and 0 entries"""
    r, hub = hubs()
    n = np.bincount(r.item, minlength=r.n_items)
    So = oracle_sim(method)[1]
    mir, n_pairs = mirrored_counts(n, So.row_ptr, So.col)
    assert 2 * n_pairs == len(So.col)
    G = ts_tables(mir)
    assert G.ts_log == 11 and G.NA >= 2
    big = [h for h in hub if G.large[h]]
    assert len(big) >= 2 and hub[3] in big and hub[2] in big
    assert G.bucket[hub[2]] == G.bucket[hub[3]]                                # two large keys in one bucket
    assert any(mir[h] % 2 == 1 for h in big)                                   # a large key with an odd mirrored count
    own = own_counts(n, So.row_ptr, So.col)
    assert np.array_equal(own + mir, np.diff(So.row_ptr))
    assert own[hub[3]] == 0 and own[hub[2]] >= 1                               # (the strictly heaviest has none by construction)
    assert all(own[h] >= 1 for h in big if h != hub[3])
    rec, lrg = large_share(G, mir)
    assert 0 < lrg[G.bucket[hub[3]]] < rec[G.bucket[hub[3]]] and n_pairs % CH_OTHER != 0


def test_rows_twin():
    """the wide layout (24-byte sort records) and the mirror with a sixth column (32-byte records) of the same input: large keys
    in both, and a large key of the mirror among the rows paired with themselves (such a pair has an own entry and no mirrored
    one, so the row's counts differ from the symmetric case)"""
    ptr, item, rating, I = rows()
    r, hub = hubs()
    assert I == r.n_items and len(item) > r.nnz and np.any(rating != rating.astype(np.float32).astype(np.float64))
    n = np.bincount(item, minlength=I)
    G = ts_tables(n)
    assert G.ts_log == 11 and G.NA >= 2 and G.large[[hub[0], hub[2], hub[3]]].all() and len(item) % CH_OTHER != 0
    assert G.bucket[hub[2]] == G.bucket[hub[3]]
    O = oracle_rows()
    mir, n_pairs = mirrored_counts(n, O.row_ptr, O.col, self_pairs=True)
    Gm = ts_tables(mir, n_pairs)
    assert Gm.ts_log == 11 and Gm.NA >= 2 and n_pairs % CH_OTHER != 0
    row = np.repeat(np.arange(I, dtype=np.int64), np.diff(O.row_ptr))
    with_self = np.zeros(I, bool)
    with_self[row[O.col == row]] = True
    assert with_self.sum() >= 2 and np.any(with_self & Gm.large)
    assert Gm.large[hub[2]] and Gm.large[hub[3]] and Gm.bucket[hub[2]] == Gm.bucket[hub[3]]
