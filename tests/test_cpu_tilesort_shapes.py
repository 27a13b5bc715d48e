"""Designed inputs for the tile sort (csrc/tilesort.h: the two transpositions of stage A -- rater records by item, kept pairs by
heavier item): the builders tests/test_gpu_tilesort_shapes.py imports, a NumPy statement of the sort's geometry (ts_geometry,
k_ts_plan: tile measure, key weight, tile and level-A bucket of every key, large keys, first key of every tile) and the
conditions each input has to meet before a comparison with the GPU says anything about the binning kernels.

The geometry in words.  K keys, M records, ptr = first position of every key.  Measure of key k = ptr[k] + k KW with
KW = max(M / (4 K), 2^ts_log / 518 + 1, 4); tile = measure >> ts_log (ts_log = 11 unless that gives more than 256 x 128 tiles);
a level-A bucket = 128 consecutive tiles, NA = ceil(tiles / 128) of them with tiles = ((M + K KW) >> ts_log) + 1; a key with
at least 2^ts_log records is large.  tile_key0[x] = the first key whose tile is at least x.  Level A finds a record's bucket
as the last b with tile_key0[128 b] <= key; a bucket no key falls into repeats its successor's boundary.

Inputs (the figures asserted below were derived with this statement and are written next to each input):

  buckets   3 000 users x about 70 ratings over 2 x 1 200 items, one hub rated by 2 400 users (strictly the most), blocks of
            600 and 40 unrated item indices between rated ones and across the domain boundary: several level-A buckets and a
            large key in both transpositions, tiles that hold keys and no records, last chunks that are not full
  gap       300 000 users who all rate one hub in the middle of the item range: the hub's records alone are longer than a
            level-A bucket, so one bucket holds no key and two consecutive boundaries are equal (layout only: a mirrored key
            of 2^18 kept pairs needs as many items)
  rows      `buckets` as AlterEgo-like rows: fp64 ratings that no float32 holds, an item twice or three times in a profile --
            the 24-byte sort records of the wide layout and the 32-byte records of the mirror with a sixth column
"""
import functools
import types

import numpy as np
import pytest

from test_cpu_stage_a_layout import CAP, METHODS, with_exact_raters

NB_LOG, NB, NA_MAX, NK_MAX = 7, 128, 256, 520        # csrc/tilesort.h
CH_NARROW, CH_OTHER = 4096, 2048                     # records per chunk of a binning level: 16-byte records / 24 and 32 bytes
LINE = 128                                           # bytes of a cache line


def ts_geometry(K, M):
    """ts_geometry of csrc/tri_mirror.hip -> namespace(ts_log, KW, tiles, NA, T)"""
    ts_log = 11
    while True:
        TS = 1 << ts_log
        kw = max(M // (4 * max(K, 1)), TS // (NK_MAX - 2) + 1, 4)
        tiles = ((M + K * kw) >> ts_log) + 1
        if tiles <= NA_MAX * NB or ts_log >= 30:
            NA = min(max((tiles + NB - 1) // NB, 1), NA_MAX)
            return types.SimpleNamespace(ts_log=ts_log, KW=int(kw), tiles=int(tiles), NA=int(NA), T=int(NA * NB))
        ts_log += 1


def ts_tables(count, M=None):
    """k_ts_plan over the per-key record counts -> the geometry plus ptr, tile, bucket and large (per key), tile_key0 [T + 1]
    and bkey0 [NA] = the first key of every level-A bucket.  M: the record count the geometry is sized from where it is
    an upper bound (the mirror: the kept pairs, of which a row paired with itself has no mirrored record)"""
    count = np.asarray(count, np.int64)
    K, M = len(count), int(count.sum()) if M is None else int(M)
    assert M >= count.sum()
    G = ts_geometry(K, M)
    G.K, G.M = K, M
    G.ptr = np.concatenate([[0], np.cumsum(count)])
    G.tile = (G.ptr[:K] + np.arange(K, dtype=np.int64) * G.KW) >> G.ts_log
    assert G.tile.max() < G.T
    G.bucket = G.tile >> NB_LOG
    G.large = count >= (1 << G.ts_log)
    G.tile_key0 = np.searchsorted(G.tile, np.arange(G.T + 1), side="left")
    G.bkey0 = G.tile_key0[np.arange(G.NA) << NB_LOG]
    return G


def bucket_by_bisection(G, key):
    """what level A computes: the last b with bkey0[b] <= key"""
    return np.searchsorted(G.bkey0, key, side="right") - 1


def chunk_fragments(G, key, ch):
    """records per (chunk of ch consecutive records, level-A bucket) of a record stream `key` -> [chunks, NA]"""
    n_ch = -(-len(key) // ch)
    out = np.zeros((n_ch, G.NA), np.int64)
    np.add.at(out, (np.arange(len(key)) // ch, G.bucket[key]), 1)
    return out


# ------------------------------------------------------------------------------------------------------------ builders
def with_unrated_blocks(r, blocks):
    """r with runs of unrated item indices put in: blocks = ((index of r the run goes in front of, length), ...); a run in
    front of the first target item is split between the domains.  The order of the items is kept."""
    from xmap.engine import synth
    gap = np.zeros(r.n_items + 1, np.int64)
    for at, n in blocks:
        gap[at] += n
    item_map = np.cumsum(gap[:-1] + 1) - 1
    n_items = r.n_items + int(gap.sum())
    n_src = int(item_map[r.n_src_items]) - int(gap[r.n_src_items]) // 2
    return synth.Ratings(r.user_ptr, item_map[r.item].astype(np.int32), r.rating, r.time, n_items, n_src, np.arange(n_src),
                         np.arange(n_items - n_src)), item_map


HUB_RATERS = 2600
BLOCKS = ((300, 600), (301, 40), (1200, 600), (1900, 40), (2100, 600))       # (in front of item, unrated indices)


@functools.lru_cache(maxsize=None)
def buckets():
    """-> (ratings, hub)"""
    from xmap.engine import synth
    r = synth.make_two_domain(51, 3000, 1200, 1200, overlap=0.5, d_min=38, mu=3.1, sigma=0.6)
    n = np.bincount(r.item, minlength=r.n_items)
    hub = int(np.nonzero(n[500:] < 1000)[0][0]) + 500
    r = with_exact_raters(r, {hub: HUB_RATERS}, 510)
    g, item_map = with_unrated_blocks(r, tuple((min(at, r.n_items), n) for at, n in BLOCKS))
    return g, int(item_map[hub])


GAP_USERS = 300000


@functools.lru_cache(maxsize=None)
def gap():
    """-> (ratings, hub): every user rates the hub; the hub is the first item (from the middle of the range on) whose records
    pass over a whole level-A bucket"""
    from xmap.engine import synth
    r = synth.make_two_domain(52, GAP_USERS, 1500, 1500, overlap=0.3, d_min=1, mu=-3.0, sigma=0.5)
    n = np.bincount(r.item, minlength=r.n_items).astype(np.int64)
    for hub in range(r.n_items // 2, r.n_items):
        c = n.copy()
        c[hub] = GAP_USERS
        G = ts_tables(c)
        if G.NA >= 3 and np.any(np.diff(G.bkey0) == 0):
            return with_exact_raters(r, {hub: GAP_USERS}, 520), hub
    raise AssertionError("no item's records pass over a whole bucket")


@functools.lru_cache(maxsize=None)
def rows():
    """`buckets` as AlterEgo-like rows -> (user_ptr, item, rating (fp64), n_items): every 7th user holds its first item twice
    more, every 21st its last item once more; ratings in thirds and eighths"""
    r, _ = buckets()
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


def ratings_of(name):
    return dict(buckets=buckets, gap=gap)[name]()[0]


@functools.lru_cache(maxsize=None)
def oracle_sim(name, method):
    """the CPU oracle's stage A on an input, computed once and shared (never freed)"""
    from oracle import xmap_oracle as xo
    r = ratings_of(name)
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
    return T, xo.item_sim(T, method, CAP, nthreads=8)


@functools.lru_cache(maxsize=None)
def oracle_rows():
    """the CPU oracle's RecommenderSim on `rows`, computed once and shared"""
    from oracle import xmap_oracle as xo
    ptr, item, rating, I = rows()
    return xo.rec_sim(ptr, item, rating, I, CAP)


def layout_tables(name):
    r = ratings_of(name)
    return ts_tables(np.bincount(r.item, minlength=r.n_items))


def mirrored_counts(n, row_ptr, col, self_pairs=False):
    """kept pairs per heavier item: of a symmetric CSR, the entries (i, j) whose column is the heavier one by (raters,
    index) -- each unordered pair once; a pair of a row with itself has no mirrored entry"""
    I = len(row_ptr) - 1
    row = np.repeat(np.arange(I, dtype=np.int64), np.diff(row_ptr))
    col = np.asarray(col, np.int64)
    heavier = (n[col] > n[row]) | ((n[col] == n[row]) & (col > row))
    assert not self_pairs or np.any(col == row)
    return np.bincount(col[heavier], minlength=I), int(heavier.sum()) + int((col == row).sum())


def mirror_tables(name, method):
    """geometry of the mirror: keys = items, records = the kept unordered pairs (xmap_sim3_mirror sizes it from their count)"""
    r = ratings_of(name)
    So = oracle_sim(name, method)[1]
    mir, n_pairs = mirrored_counts(np.bincount(r.item, minlength=r.n_items), So.row_ptr, So.col)
    assert 2 * n_pairs == len(So.col)
    return ts_tables(mir)


# ---------------------------------------------------------------------------------------------------- the statement
def test_statement_on_a_hand_made_input():
    """5 keys with 0, 3000, 0, 0, 5 records: M = 3005, KW = max(150, 4, 4) = 150; measures 0, 150, 3300, 3450, 3600 -> tiles 0, 0, 1,
    1, 1; key 1 is large; one bucket"""
    G = ts_tables([0, 3000, 0, 0, 5])
    assert (G.ts_log, G.KW, G.tiles, G.NA, G.T) == (11, 150, 2, 1, 128)
    assert G.tile.tolist() == [0, 0, 1, 1, 1] and G.large.tolist() == [False, True, False, False, False]
    assert G.tile_key0[:3].tolist() == [0, 2, 5] and np.all(G.tile_key0[2:] == 5) and G.bkey0.tolist() == [0]
    # the key weight keeps a tile's keys within the LDS tables of level C whatever the counts
    G = ts_tables(np.zeros(100000, np.int64))
    assert G.KW == 4 and np.bincount(G.tile).max() <= NK_MAX - 2
    # a key of 2^19 records between small ones: its records pass over the whole of bucket 1, whose boundary repeats
    G = ts_tables([10] * 200 + [1 << 19] + [10] * 200)
    assert (G.KW, G.NA) == (329, 3) and G.bkey0.tolist() == [0, 201, 201]
    assert np.array_equal(bucket_by_bisection(G, np.arange(G.K)), G.bucket) and G.bucket[[200, 201]].tolist() == [0, 2]


@pytest.mark.parametrize("name", ["buckets", "gap"])
def test_bisection_finds_every_keys_bucket(name):
    """the bucket is monotone in the key, so the last boundary at or below a key is its bucket's -- also where boundaries
    repeat and for the keys that ARE a boundary"""
    G = layout_tables(name)
    keys = np.arange(G.K)
    assert np.array_equal(bucket_by_bisection(G, keys), G.bucket)
    assert np.all(np.diff(G.bkey0) >= 0) and G.bkey0[0] == 0
    assert np.array_equal(bucket_by_bisection(G, G.bkey0), G.bucket[np.minimum(G.bkey0, G.K - 1)])


# ------------------------------------------------------------------------------------------------------- the census
def test_buckets_layout():
    """246 101 rater records over 4 280 item indices, key weight 14: 150 tiles in 2 level-A buckets, the hub (and the two most
    popular items of the generator) large, tiles of unrated indices only"""
    r, hub = buckets()
    G = layout_tables("buckets")
    n = np.bincount(r.item, minlength=r.n_items)
    assert r.n_users == 3000 and G.M == r.nnz == 246101 and G.tiles >= 129 and G.ts_log == 11
    assert G.NA >= 2 and len(np.unique(G.bucket[r.item])) == G.NA              # records in every bucket
    assert n[hub] == HUB_RATERS >= 2100 and np.sort(n)[-2] < HUB_RATERS          # strictly the most raters
    assert G.large[hub] and G.large.sum() >= 1
    assert int((n > 0).sum()) > 2100
    # blocks of unrated indices between rated ones: tiles whose keys have no records (equal position boundaries), and a
    # bucket boundary's key without records
    recs = np.bincount(G.tile, weights=n, minlength=G.T)[:G.tile.max() + 1]
    keys = np.bincount(G.tile, minlength=G.T)[:G.tile.max() + 1]
    assert int(((recs == 0) & (keys > 0)).sum()) >= 3
    assert n[:np.nonzero(n)[0][0]].size == 0 and np.any(n[1:-1] == 0)
    # the last chunk of level A is not full, holds more than one bucket's records, and its fragments are longer than a line
    # and not all whole lines: wherever the cursors put them, fragments start and end inside lines
    F = chunk_fragments(G, r_records("buckets"), CH_NARROW)
    assert r.nnz % CH_NARROW != 0 and int((F[-1] > 0).sum()) >= 2
    assert F[-1].max() > LINE // 16 and np.any(F % (LINE // 16) != 0) and np.any(F % 2 == 1)


def r_records(name):
    """the item column in the order the profile sort emits the sort records: user-major (the order inside a profile does not
    change a chunk's fragment sizes unless the profile straddles chunks; the storage order is taken)"""
    return ratings_of(name).item


@pytest.mark.parametrize("method", METHODS)
def test_buckets_mirror(method):
    """the kept pairs by heavier item: several level-A buckets, the hub a large key (it is the heavier partner of every pair
    it is in), 24-byte records whose fragments cannot all start on a 16-byte boundary"""
    r, hub = buckets()
    G = mirror_tables("buckets", method)
    So = oracle_sim("buckets", method)[1]
    assert G.M >= 129 << 11 and G.NA >= 2 and G.ts_log == 11
    assert G.large[hub] and int(G.ptr[hub + 1] - G.ptr[hub]) == int(So.row_ptr[hub + 1] - So.row_ptr[hub]) >= 2048
    occupied = np.unique(G.bucket[np.repeat(np.arange(G.K), np.diff(G.ptr))])
    assert len(occupied) == G.NA >= 2
    assert np.array_equal(bucket_by_bisection(G, np.arange(G.K)), G.bucket)
    assert np.any(np.diff(G.ptr) % 2 == 1)


def test_gap_layout():
    """the hub's 300 000 records are longer than a bucket (2^18 positions): a bucket without a key, two equal boundaries"""
    r, hub = gap()
    G = layout_tables("gap")
    n = np.bincount(r.item, minlength=r.n_items)
    assert n[hub] == GAP_USERS > NB << G.ts_log and G.ts_log == 11 and G.NA >= 3
    empty = np.nonzero(np.diff(G.bkey0) == 0)[0]
    assert len(empty) >= 1 and G.bkey0[empty[0]] == hub + 1 and G.bucket[hub] < empty[0] < G.bucket[hub + 1]
    assert 0 < hub < r.n_items - 1 and n[:hub].sum() > 0 and n[hub + 1:].sum() > 0
    assert r.nnz % CH_NARROW != 0
    # runs of tiles without a key (equal tile boundaries) inside the hub's range
    assert int((np.diff(G.tile_key0[:G.tile.max() + 1]) == 0).sum()) >= NB


def test_rows_are_alterego_like():
    """the wide layout (24-byte sort records, chunks of 2 048) and the mirror with a sixth column (32-byte records)"""
    ptr, item, rating, I = rows()
    r, hub = buckets()
    assert len(item) > r.nnz and np.any(rating != rating.astype(np.float32).astype(np.float64))
    dup = sum(len(set(item[ptr[k]:ptr[k + 1]].tolist())) < ptr[k + 1] - ptr[k] for k in range(0, len(ptr) - 1, 7))
    assert dup >= (len(ptr) - 1) // 7
    n = np.bincount(item, minlength=I)
    G = ts_tables(n)
    assert G.NA >= 2 and G.large[hub] and len(item) % CH_OTHER != 0
    assert np.array_equal(bucket_by_bisection(G, np.arange(I)), G.bucket)
    O = oracle_rows()
    mir, n_pairs = mirrored_counts(n, O.row_ptr, O.col, self_pairs=True)
    Gm = ts_tables(mir, n_pairs)
    assert Gm.NA >= 2 and Gm.large[hub] and n_pairs % CH_OTHER != 0
    assert np.array_equal(bucket_by_bisection(Gm, np.arange(I)), Gm.bucket)
