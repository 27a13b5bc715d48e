"""Designed RecommenderSim rows for k_rec_select (csrc/stage_e.hip: xmap_rec_select, xmap_ctx_rec_select, the lists of
xmap_ctx_item_foldin) and a plain NumPy statement of nonprivate_neighbor_selection on them.  No device and no torch: the builders
tests/test_cpu_rec_select_rows.py takes the census of and tests/test_gpu_rec_select_rows.py uploads.

The statement: per row np.lexsort((col, -|sim|))[:keep] -- |sim| descending, column ascending -- gives cnt = min(len, keep)
and col / sim / ls of the chosen entries, sim with its sign bit; the padding behind cnt is -1 / 0.0 / 0.0.  Two deliberately
WRONG variants sit behind keyword arguments: `tie_by_position` breaks a |sim| tie by the position in the row instead of by
the column, `signed_key` ranks by sim instead of |sim|.  They exist to prove that the inputs tell such a kernel from a right
one (the rows of rec_sim itself do not: ascending columns, no negative and no zero similarity).

Rows, the same for every family: one per length in LENS -- the edges of the kernel's 64-entry chunk (63, 64, 65; 127 ... 129;
191 ... 193), of keep = 10 / 63 / 64 against the row length (9 ... 11, 62 ... 66) and one row of 41 chunks (2561 = 40 * 64 + 1) --
with an empty row first, one between the two longest rows and one last, and short rows until the row count is 4 n + 1 (a block
takes four rows: the last block holds one).  The columns of a row are distinct -- the order of two entries equal in
(|sim|, column) is not defined -- and drawn from [0, 2^31 - 1); the longest row holds both 0 and 2^31 - 2 (the kernel pads a
chunk with column 2^31 - 1).  ls is a position code, 0.5 p + 0.25 for the entry at position p of its row as stored: it proves
WHICH entry was taken.  No NaN anywhere: its place is undefined in the oracle's comparator (neither greater nor smaller).

FAMILIES give the values of the entries (signs are random in all of them), ORDERS the storage order inside every row:
`abs_asc` is the exact reverse of the sorted order, so every entry of every chunk passes the threshold and is inserted at
lane 0; under `abs_desc` nothing is inserted after the first `keep` entries.
"""
import functools

import numpy as np

LENS = (0, 1, 2, 9, 10, 11, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 2561)
SHORT = (3, 4, 5, 7)                # the rows that make the row count 4 n + 1
FAMILIES = ("one", "levels4", "zeros", "distinct", "extremes")
TIED = ("one", "levels4", "zeros", "extremes")
ORDERS = ("col_asc", "col_desc", "abs_asc", "abs_desc", "shuffle")
KEEPS = (1, 2, 10, 63, 64)          # 63 | 64: the lane mask of the kept list is (1 << keep) - 1 below 64 and all ones at 64
SEED = 11
COL_END = 2 ** 31 - 1               # columns are < COL_END
DBL_MAX, DBL_MIN = np.finfo(np.float64).max, np.finfo(np.float64).tiny
EXTREMES = (np.inf, DBL_MAX, 1.0, np.nextafter(1.0, 0.0), DBL_MIN, 1e-310, 5e-324, 0.0)


def row_lengths():
    """an empty row, the LENS rows but the longest, an empty row, the longest, the SHORT rows, an empty row"""
    n = [0] + list(LENS[:-1]) + [0, LENS[-1]] + list(SHORT) + [0]
    assert len(n) % 4 == 1
    return np.asarray(n, np.int64)


class Rows(object):
    """row_ptr [I + 1], col / sim / ls per entry, and `rows`: the row of every entry"""
    def __init__(self, row_ptr, col, sim, ls):
        self.row_ptr = np.ascontiguousarray(row_ptr, np.int64)
        self.col, self.sim, self.ls = np.ascontiguousarray(col, np.int32), np.ascontiguousarray(sim, np.float64), np.ascontiguousarray(ls, np.float64)
        self.I = len(self.row_ptr) - 1
        self.rows = np.repeat(np.arange(self.I), np.diff(self.row_ptr))
        for a in (self.row_ptr, self.col, self.sim, self.ls, self.rows):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _structure():
    """(row_ptr, rows, cols) with ascending columns inside every row"""
    n = row_lengths()
    rng = np.random.RandomState(SEED)
    row_ptr = np.zeros(len(n) + 1, np.int64)
    np.cumsum(n, out=row_ptr[1:])
    cols = []
    for length in n:
        c = np.unique(rng.randint(0, COL_END, size=2 * int(length) + 2).astype(np.int64))
        c = c[rng.permutation(len(c))[:length]]
        if length == max(LENS):
            c[:2] = (0, COL_END - 1)
        c = np.sort(c)
        assert len(np.unique(c)) == length
        cols.append(c)
    cols = np.concatenate(cols)
    assert cols.min() == 0 and cols.max() == COL_END - 1
    return row_ptr, np.repeat(np.arange(len(n)), n), cols


@functools.lru_cache(maxsize=None)
def _values(family):
    """sim of every entry in (row, column ascending) order"""
    _, rows, _ = _structure()
    D = len(rows)
    rng = np.random.RandomState(SEED + 1 + FAMILIES.index(family))
    sign = np.where(rng.randint(0, 2, D) != 0, -1.0, 1.0)
    if family == "one":
        mag = np.full(D, 1.0 / 3.0)
    elif family == "levels4":
        mag = np.asarray([1.0, 1.0 / 3.0, 0.3, 1e-3])[rng.randint(0, 4, D)]
    elif family == "zeros":
        mag = np.where(rng.rand(D) < 0.7, 0.0, np.asarray([1.0, 0.5, 0.25])[rng.randint(0, 3, D)])
    elif family == "distinct":
        mag = (rng.permutation(D) + 1.0) / (D + 1.0)
    else:
        mag = np.asarray(EXTREMES)[rng.randint(0, len(EXTREMES), D)]
    sim = sign * mag
    assert not np.isnan(sim).any()
    sim.setflags(write=False)
    return sim


@functools.lru_cache(maxsize=None)
def design(family, order):
    """the designed rows of one family with every row stored in one order: Rows (read-only arrays)"""
    row_ptr, rows, cols = _structure()
    sim = _values(family)
    a = np.abs(sim)
    if order == "col_asc":
        o = np.arange(len(rows))
    elif order == "col_desc":
        o = np.lexsort((-cols, rows))
    elif order == "abs_asc":
        o = np.lexsort((-cols, a, rows))
    elif order == "abs_desc":
        o = np.lexsort((cols, -a, rows))
    else:
        assert order == "shuffle"
        o = np.lexsort((np.random.RandomState(SEED + 100).rand(len(rows)), rows))
    assert np.array_equal(rows[o], rows)
    pos = np.arange(len(rows)) - row_ptr[:-1][rows]           # the position inside the row, as stored
    return Rows(row_ptr, cols[o], sim[o], 0.5 * pos + 0.25)


def take_rows(R, which):
    """the rows `which` of R (in that order) as a CSR of their own"""
    which = np.asarray(which, np.int64)
    n = np.diff(R.row_ptr)[which]
    row_ptr = np.zeros(len(which) + 1, np.int64)
    np.cumsum(n, out=row_ptr[1:])
    e = np.concatenate([np.arange(R.row_ptr[i], R.row_ptr[i + 1]) for i in which] + [np.zeros(0, np.int64)]).astype(np.int64)
    return Rows(row_ptr, R.col[e], R.sim[e], R.ls[e])


def statement(R, keep, tie_by_position=False, signed_key=False):
    """(cnt [I], col [I][keep], sim, ls): the selection stated in NumPy.  The two keyword arguments are the WRONG variants."""
    cnt = np.zeros(R.I, np.int32)
    col = np.full((R.I, keep), -1, np.int32)
    sim = np.zeros((R.I, keep), np.float64)
    ls = np.zeros((R.I, keep), np.float64)
    for i in range(R.I):
        lo, hi = int(R.row_ptr[i]), int(R.row_ptr[i + 1])
        c, s, l = R.col[lo:hi], R.sim[lo:hi], R.ls[lo:hi]
        key = -s if signed_key else -np.abs(s)
        o = np.lexsort((np.arange(hi - lo) if tie_by_position else c, key))[:keep]
        n = len(o)
        cnt[i] = n
        col[i, :n], sim[i, :n], ls[i, :n] = c[o], s[o], l[o]
    return cnt, col, sim, ls


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, want):
    """exact: integers as integers, doubles through their uint64 views (the sign of a zero counts)"""
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
            and np.array_equal(bits(got[3]), bits(want[3])))


def rows_that_differ(got, want):
    """rows whose (count, columns, sims, position codes) are not all identical"""
    d = (got[0] != want[0]) | (got[1] != want[1]).any(1) | (bits(got[2]) != bits(want[2])).any(1) | (bits(got[3]) != bits(want[3])).any(1)
    return np.nonzero(d)[0]
