"""Designed similarity matrices that reach every shape class of k_paths4 (csrc/paths4.hip), one concern per family, fed to
both sides: xo.sim_from_arrays + xo.extend on the CPU, Engine.sim_from_host + Engine.extend on the device.  The classes a
family reaches are counted by tests/paths_statement.py (column_census) and written below (CENSUS); tests/
test_cpu_paths_columns.py holds the counts, tests/test_gpu_paths_columns.py compares the device with the oracle and the
statement.

The pattern.  Source items come first: columns X (non-bridge, attached to source bridge items s), fillers F (neighbours of
columns only: they have no bridge neighbour, so the classification drops them, yet they end paths) and the s; then the target
items: bridge items t and the heads P (non-bridge, attached to t).  Every t of a family's live group is a neighbour of every s
of it, so every (t, s) is joint; X_j is attached to the first r_j of the s and P_i to the first q_i of the t, hence the tile
(P_i, X_j) has q_i * r_j records.  A column's ends are X_j and all its neighbours (NB_NN keeps every neighbour, the s
included): ne = 1 + min(k, degree) >= 2 -- a column of ONE end does not exist, the narrowest designed one has two.  The heads
of a start P_i are P_i and its P neighbours, those of a start t the P attached to it.

Values: sim = a hash of the unordered pair in +-[0.05, 0.95], mutu = nij in 1 .. 7, info[:, 3] = 50: symmetric bit for
bit, and inside the range of the bare division (fast_div_ok).  The ratings object only supplies the item domains (one user
per item, one rating each)."""
import functools

import numpy as np

from paths_statement import column_census, statement


def _mix(x):
    x = x.copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xbf58476d1ce4e5b9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94d049bb133111eb)
    x ^= x >> np.uint64(31)
    return x


def pair_values(rows, cols, seed):
    """(sim, mutu) of the directed pairs: a function of the unordered pair and the seed"""
    a, b = np.minimum(rows, cols).astype(np.uint64), np.maximum(rows, cols).astype(np.uint64)
    h = _mix(((a << np.uint64(32)) | b) + np.uint64((0x9e3779b97f4a7c15 * (seed + 1)) & 0xffffffffffffffff))
    mag = 0.05 + 0.9 * ((h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)
    sim = np.where((h >> np.uint64(3)) & np.uint64(1), -mag, mag)
    mutu = (1 + (h % np.uint64(7))).astype(np.int32)
    return np.ascontiguousarray(sim, np.float64), mutu


class Design(object):
    """named groups of source and of target items in index order, and undirected edges between them"""

    def __init__(self, src, tgt):
        self.ix, off = {}, 0
        for name, n in src:
            self.ix[name] = np.arange(off, off + n)
            off += n
        self.n_src = off
        for name, n in tgt:
            self.ix[name] = np.arange(off, off + n)
            off += n
        self.I = off
        self.edges = set()

    def link(self, a, b):
        a, b = int(a), int(b)
        assert a != b
        self.edges.add((min(a, b), max(a, b)))

    def first(self, A, counts, B):
        """A[i] ~ the first counts[i] of B"""
        for a, n in zip(A, counts):
            assert n <= len(B)
            for b in B[:n]:
                self.link(a, b)

    def arrays(self, seed, order="asc"):
        """(row_ptr, col, sim, mutu, nij, info); order: how the pairs of a row are listed (asc, desc, or a seed to shuffle)"""
        e = np.array(sorted(self.edges), np.int64).reshape(-1, 2)
        rows, cols = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
        if order == "asc":
            o = np.lexsort((cols, rows))
        elif order == "desc":
            o = np.lexsort((-cols, rows))
        else:
            o = np.lexsort((np.random.default_rng(order).permutation(len(rows)), rows))
        rows, cols = rows[o], cols[o]
        row_ptr = np.zeros(self.I + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=self.I), out=row_ptr[1:])
        sim, mutu = pair_values(rows, cols, seed)
        info = np.zeros((self.I, 4))
        info[:, 3] = 50.0
        return row_ptr, cols.astype(np.int32), sim, mutu, mutu.copy(), info

    def ratings(self):
        from xmap.engine import synth
        I = self.I
        return synth.Ratings(np.arange(I + 1, dtype=np.int64), np.arange(I, dtype=np.int32), np.ones(I, np.float32),
                             np.zeros(I, np.int64), I, self.n_src, np.arange(self.n_src), np.arange(I - self.n_src))


def _columns(D, X, F, S, r, ne):
    """column X[j]: attached to the first r[j] of S, and F neighbours up to ne[j] ends in all"""
    D.first(X, r, S)
    D.first(X, [n - 1 - a for n, a in zip(ne, r)], F)


# ---- wide (k = 100): every width class of a column, few heads, few records ---------------------------------------------------
# columns of exactly 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100 and 101 ends (S = 4 | 2 | 1 slices on both sides of 16 and 32;
# one and two chunks of 64 ends on both sides of 64; k + 1 = 101), and one column of 121 neighbours that the list cuts to 101
# ends.  Odd columns are attached to two s.  Three heads in a chain with 1, 2 and 2 of the two t: at most 3 heads and
# (1 + 2 + 2) * 2 = 10 records per visit.
WIDE_NE = [2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 101, 122]


def wide():
    D = Design([("X", len(WIDE_NE)), ("F", 120), ("s", 2)], [("t", 2), ("P", 3)])
    ix = D.ix
    r = [1 + (j % 2) for j in range(len(WIDE_NE))]
    _columns(D, ix["X"], ix["F"], ix["s"], r, WIDE_NE)
    D.first(ix["t"], [2, 2], ix["s"])
    D.first(ix["P"], [1, 2, 2], ix["t"])
    D.link(ix["P"][0], ix["P"][1]); D.link(ix["P"][1], ix["P"][2])
    return D, 100, 21, None


# ---- records (k = 100): every record-count class of a visit, on narrow and on wide columns --------------------------------
# 64 t x 43 s.  Columns (r, ne): (1, 2) (1, 101) (2, 20) (13, 14) (43, 50) (2, 70).  Heads:
#   eight alone with q = 1, 3, 5, 15, 16, 17, 63, 64: one head per visit, R = q * r -- 1, 15, 16, 17, 63, 64 on r = 1,
#       65 = 5 * 13, 128 = 64 * 2, 129 = 3 * 43; q = 17 and 5 * 13 = 65 are one head alone with more than a group / a round
#   a pair with q = 64 + 63: R = 127 on r = 1;  a pair with q = 10 + 10: the second head's records straddle a group edge
#   a hub with 16 leaves and one with 32, q = 1 each: 17 and 33 participating heads of one record
# R > 64 meets every width class: (13, 14) from q = 5, (2, 20) from q = 63, (43, 50) from q = 3, (1, 101) from the 64 + 63 pair.
REC_COLS = [(1, 2), (1, 101), (2, 20), (13, 14), (43, 50), (2, 70)]
REC_SINGLE = [1, 3, 5, 15, 16, 17, 63, 64]


def records():
    D = Design([("X", len(REC_COLS)), ("F", 99), ("s", 43)],
               [("t", 64), ("single", len(REC_SINGLE)), ("p127", 2), ("p10", 2), ("hub17", 17), ("hub33", 33)])
    ix = D.ix
    _columns(D, ix["X"], ix["F"], ix["s"], [c[0] for c in REC_COLS], [c[1] for c in REC_COLS])
    D.first(ix["t"], [43] * 64, ix["s"])
    D.first(ix["single"], REC_SINGLE, ix["t"])
    D.first(ix["p127"], [64, 63], ix["t"])
    D.first(ix["p10"], [10, 10], ix["t"])
    D.link(*ix["p127"]); D.link(*ix["p10"])
    for hub in ("hub17", "hub33"):
        D.first(ix[hub], [1] * len(ix[hub]), ix["t"])
        for leaf in ix[hub][1:]:
            D.link(ix[hub][0], leaf)
    return D, 100, 22, ("single", "hub33")


# ---- heads (k = 6): every head-count class of a start, later batches ---------------------------------------------------------
# 40 columns in a chain (X_i ~ X_i+1, all attached to the live s: 3 or 4 ends, and X_i is the home column of X_i+1); hubs
# with n - 1 leaves for n = 1, 4, 5, 16, 17, 64, 65, 128, 129 heads, every one attached to the live t (one record per tile).
# The LAST leaf of every hub -- the head in lane n - 1 of the hub's batch, lanes 3 | 4, 15 | 16 and 63 among them -- is also
# attached to a t of its own kind whose s has the private column Xp, the lowest of all: a column that one lane alone holds, so
# the minimum over the lanes has to see that lane.
# `late`: a hub with 63 live leaves and, behind them in index order, 10 leaves attached to a t whose only s has no column -- they
# are heads without a tile, so the hub's second batch has no column at all.  The hub of 65 has a second batch of one head.  The
# live t itself starts with every live P that lists it as a head (487 heads, 8 batches).
HEAD_HUBS = [1, 4, 5, 16, 17, 64, 65, 128, 129]


def heads():
    D = Design([("Xp", 1), ("X", 40), ("s", 3)],
               [("t", 3)] + [("hub%d" % n, n) for n in HEAD_HUBS] + [("late", 64), ("dead", 10)])
    ix = D.ix
    X = ix["X"]
    for i in range(len(X)):
        D.link(X[i], ix["s"][0])
        if i + 1 < len(X):
            D.link(X[i], X[i + 1])
    D.link(ix["t"][0], ix["s"][0])
    D.link(ix["t"][1], ix["s"][1])            # the dead pair: s[1] has no column, so (t[1], s[1]) is no source record
    D.link(ix["t"][2], ix["s"][2])            # the private pair
    D.link(ix["Xp"][0], ix["s"][2])
    for name in ["hub%d" % n for n in HEAD_HUBS] + ["late"]:
        g = ix[name]
        for p in g:
            D.link(p, ix["t"][0])
        for leaf in g[1:]:
            D.link(g[0], leaf)
        if name != "late" and len(g) >= 4:
            D.link(g[-1], ix["t"][2])
    for p in ix["dead"]:
        D.link(p, ix["t"][1])
        D.link(ix["late"][0], p)
    return D, 6, 23, None


BUILDERS = dict(wide=wide, records=records, heads=heads)

# What column_census finds on each family: the exact figures of every class it names that the family reaches (a quantity not
# listed is zero there), held by tests/test_cpu_paths_columns.py.  PATHS: the oracle's path count, which MAX_PATHS bounds
# (about 2 s of the one-thread oracle at the 5-6e6 paths/s it runs at).  `records` is cut to the starts that are heads (the
# oracle's starts=, the engine's start_range=): its 64 t as starts would add 4.6e7 paths of the same classes.
MAX_PATHS = 10 ** 7
PATHS = dict(wide=21505, records=1658592, heads=241779)
CENSUS = dict(
    wide={'visits': 65, 'nloc<=4': 65, 'ne<=16': 15, 'ne17-32': 15, 'ne33-64': 15, 'ne>64': 20, 'ne=16': 5, 'ne=17': 5, 'ne=32': 5,
          'ne=33': 5, 'ne=64': 5, 'ne=65': 5, 'ne=k+1': 10, 'max_ne': 101, 'max_R': 10, 'max_nH': 3},
    records={'visits': 372, 'nloc<=4': 360, 'nloc17-64': 12, 'ne<=16': 124, 'R>64&ne<=16': 14, 'ne17-32': 62, 'R>64&ne17-32': 5,
             'ne33-64': 62, 'R>64&ne33-64': 61, 'ne>64': 124, 'R>64&ne>64': 7, 'ne=k+1': 62, 'R=16': 2, 'R=17': 4, 'R=64': 2,
             'R=65': 1, 'R=128': 2, 'R=129': 1, 'R>128': 28, 'head>16': 101, 'head>64': 29, 'straddle': 155, 'p>=17': 12,
             'max_ne': 101, 'max_R': 5461, 'max_nH': 33, 'nH=1': 8, 'nH=17': 1},
    heads={'visits': 20302, 'nloc<=4': 19531, 'nloc5-16': 123, 'nloc17-64': 648, 'batch>0': 447, 'ne<=16': 20302, 'R=16': 40,
           'R=17': 40, 'R=64': 560, 'p>=17': 640, 'last_lane@4': 1, 'last_lane@5': 1, 'last_lane@16': 1, 'last_lane@17': 1,
           'last_lane@64': 2, 'max_ne': 4, 'max_R': 64, 'late_home': 444, 'late_home_own': 433, 'later_batches': 12,
           'later_empty': 1, 'later_one_head': 2, 'max_nH': 487, 'nH=1': 437, 'nH=4': 1, 'nH=5': 1, 'nH=16': 1, 'nH=17': 1,
           'nH=64': 1, 'nH=65': 1, 'nH=128': 1, 'nH=129': 1})
# what a family is for, beyond the census: (p, R) of visits that must occur, widths that must occur
MUST_NE = dict(wide=[2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 101])
MUST_R = dict(records=[1, 15, 16, 17, 63, 64, 65, 127, 128, 129])
MUST_PR = dict(records=[(1, 17), (1, 65), (2, 20), (17, 17), (33, 33)])      # one head alone with 17 and 65 records, 10 + 10, 17 and 33 heads

# ---- heavy: the records and heads matrices with the starts cut into G units -------------------------------------------------
# (family, chunk, n_slots, range_census of the plan, h_out = units, heavy starts, rows, paths, chunk).  The chunks are read off
# the statement's P: ceil(P of the heaviest start / G) for G = 2, 24, 25 (records) and 2, 12, 13, 25 (heads), which leaves the
# lighter starts with the smaller G.  Both sides of MERGE_GROUP = 12: G = 12 | 13 and 24 | 25 (odd_group: a G that leaves
# a merge group of one row).  rx1: RX = 1 (G <= batches: the heads matrix, whose heavy starts have up to 8 batches); rx>1:
# column ranges, hi_range = visits found through the directory bisection (xlo > 0).  n_slots = 1 sends every unit through one
# accumulator row (the finalisation's reset), 3 is no multiple of a block's four waves.  deep_rows: rows with work at position
# >= MERGE_GROUP of their start.  The heavy starts of `records` have one batch and few columns, so their G units are column
# ranges of which only the first three hold a column: nothing lands beyond row 11 there, and a second merge level that folds
# the wrong rows in goes unnoticed.  The heaviest start of `heads` has 487 heads, whose per-head paths are dealt over all G
# units: at G = 13 the one row of the second group, at G = 25 all thirteen rows beyond the first group hold sums.
HEAVY = [
    ("records", 168783, 64, {'G': [2], 'rx1': 0, 'hi_range': 0, 'odd_group': 0, 'deep_rows': 0, 'rx>1': 3}, [65, 3, 6, 1658592, 168783]),
    ("records", 14066, 1, {'G': [3, 4, 7, 12, 13, 24], 'rx1': 0, 'hi_range': 10, 'odd_group': 1, 'deep_rows': 0, 'rx>1': 11}, [154, 11, 103, 1658592, 14066]),
    ("records", 13503, 3, {'G': [3, 4, 7, 13, 25], 'rx1': 0, 'hi_range': 10, 'odd_group': 4, 'deep_rows': 0, 'rx>1': 11}, [157, 11, 106, 1658592, 13503]),
    ("heads", 38808, 3, {'G': [2], 'rx1': 1, 'hi_range': 0, 'odd_group': 0, 'deep_rows': 0, 'rx>1': 0}, [497, 1, 2, 241779, 38808]),
    ("heads", 6468, 1, {'G': [2, 4, 12], 'rx1': 2, 'hi_range': 0, 'odd_group': 0, 'deep_rows': 0, 'rx>1': 4}, [516, 6, 26, 241779, 6468]),
    ("heads", 5971, 64, {'G': [2, 4, 13], 'rx1': 2, 'hi_range': 0, 'odd_group': 1, 'deep_rows': 1, 'rx>1': 4}, [517, 6, 27, 241779, 5971]),
    ("heads", 3105, 3, {'G': [4, 7, 25], 'rx1': 0, 'hi_range': 0, 'odd_group': 1, 'deep_rows': 13, 'rx>1': 6}, [541, 6, 51, 241779, 3105]),
]


class Case(object):
    pass


@functools.lru_cache(maxsize=None)
def family_case(name):
    """A family and everything the oracle and the statement make of it (computed once per process, shared, read-only)"""
    from oracle import xmap_oracle as xo
    c = Case()
    c.name = c.family = name
    c.method = "designed"
    c.D, c.k, c.seed, cut = BUILDERS[name]()
    c.I = c.D.I
    # cut: the starts of the groups [first, last] only (the oracle's starts=, the engine's start_range=)
    c.start_range = None if cut is None else (int(c.D.ix[cut[0]][0]), int(c.D.ix[cut[1]][-1]) + 1)
    c.starts = None if cut is None else np.arange(*c.start_range)
    c.r = c.D.ratings()
    c.attrs = c.r.item_attrs()
    c.T = xo.Train(c.r.user_ptr, c.r.item, c.r.rating, c.r.time, c.I, *c.attrs)
    c.row_ptr, c.col, c.sim, c.mutu, c.nij, c.info = c.D.arrays(c.seed)
    c.So = xo.sim_from_arrays(c.I, c.row_ptr, c.col, c.sim, c.mutu, c.nij, c.info)
    c.Xo = xo.extend(c.T, c.So, c.k, starts=c.starts)
    c.n_top, c.choice, c.map = xo.select(c.T, c.Xo, True, None)
    c.St = statement(c.Xo.cls, c.Xo.cnt, c.Xo.col, c.attrs[3], starts=c.starts)
    c.census = column_census(c.St)
    for a in (c.row_ptr, c.col, c.sim, c.mutu, c.nij, c.info, c.Xo.xs_val, c.Xo.xs_end, c.Xo.val, c.Xo.col, c.Xo.cnt, c.Xo.cls):
        a.setflags(write=False)
    return c
