"""Designed similarity rows for the three places that pick "the k best of a row by (|sim| descending, column ascending)":
k_knn_classify (csrc/knn.hip), the threshold test of k_reverse / k_reverse_long (csrc/reverse.hip: in_list) and -- in
tests/test_gpu_dense.py -- k_dense_topk.  This file holds the builders tests/test_gpu_topk_rows.py imports, a plain NumPy
statement of the classified top-k lists, and the conditions the CPU oracle's tables have to meet on these inputs before a
comparison with the GPU says anything.

Item space: the predicates (item_attrs) and the item count of one synth.make_two_domain input; the ratings are not used.
The kept-pair matrix is built here.  nij = 1, mutu = 1, info[:, 3] = 5, so every frac_mutu is 1 / 9.

Designed rows, one per length in LENS and kind (the length counts every partner and is exact):

  sb   source-domain bridge hub of length n: min(n, n % 12 + 1) target bridge hubs (a bipartite graph with that degree on both
       sides), the `nb` hubs that chose it, and same-domain fillers for the rest
  tb   target-domain bridge hub: the mirror image (no `nb` partners)
  nb   source-domain NON-bridge hub: min(n, 4) `sb` hubs of at least 63 entries and same-domain fillers; no partner of the
       other domain, so the row runs the `isbb == false` predicates (list A = the bridge partners: short of every k > 4)

Fillers are the other items of a domain.  A filler is a partner of designed rows of its own domain only: it stays non-bridge
and its row stays short (a few dozen entries at the most).

LENS sits on every structural edge of k_knn_classify: the one-wave sort (N <= 128 after padding to a power of two: 64, 65,
127, 128, 129), the 512-entry instance split K_CH_SMALL (511, 512, 513), the 2048-entry chunk K_CH (2047, 2048, 2049), the
1024-entry stream window K_WIN behind it (3071 = 2048 + 1023, 3072, 3073, 4095, 4096, 4097, 5121 = 2048 + 3 * 1024 + 1), and on
the 4096-entry default of k_reverse_long (4096, 4097).

Values are a function of the unordered pair (the matrix is symmetric bit for bit) -- FAMILIES -- and every row is stored in
each of ORDERS.  `abs_asc` is the exact reverse of the sorted order (|sim| ascending, columns descending inside a tie): every
later entry sorts before every earlier one, so in the stream of k_knn_classify every entry survives the stale threshold, the
survivor buffer fills within a window and the early exit (CH - f < K_WIN) is taken; for `one` (all |sim| equal) `col_desc`
does the same.
"""
import functools

import numpy as np
import pytest

from test_cpu_fed_sim import _mix

LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072,
        3073, 4095, 4096, 4097, 5121, 6200)
KINDS = ("sb", "tb", "nb")
FAMILIES = ("one", "levels4", "zeros", "distinct")
ORDERS = ("col_asc", "col_desc", "abs_asc", "abs_desc", "shuffle")
KS = (1, 3, 5, 50, 64, 65)          # 64 / 65: the last k on the 8 KB instance and the first one with every row on the 32 KB one
K_MAX = 512                         # the largest k xmap_knn_classify admits: the carried 2 k entries fill half a chunk
BIG_K_FAMILIES = ("levels4", "one")       # k = 512 on these two only: a set of tables takes 0.4 GB of host memory
CASES = [(f, k) for f in FAMILIES for k in KS] + [(f, K_MAX) for f in BIG_K_FAMILIES]
SEED = 7          # (a seed at which `one` meets the minima of the census at k = 3: not every seed does)
NB_LINKS = 4
BUSY = 4200


def hub_degree(n):
    """hubs of the other domain in a bridge hub's row of length n"""
    return min(n, n % 12 + 1)


class Rows(object):
    pass


def _bipartite(deg, rng):
    """edges (i, j) of a bipartite graph with degree deg[i] on the left AND deg[j] on the right (Gale-Ryser's construction:
    left nodes by descending degree, each to the right nodes with the most degree left; ties by a seeded order)"""
    left = np.asarray(deg).copy()
    right = np.asarray(deg).copy()
    tie = rng.permutation(len(deg))
    edges = []
    for i in np.argsort(-left, kind="stable"):
        pick = np.lexsort((tie, -right))[:left[i]]
        assert np.all(right[pick] > 0), "degree sequence not realisable"
        right[pick] -= 1
        edges += [(int(i), int(j)) for j in pick]
    assert not right.any()
    return edges


@functools.lru_cache(maxsize=None)
def structure():
    """The item space and the kept-pair structure: Train of the oracle (predicates only), I, the designed rows
    hub[kind][n] = item, and the directed pairs (rows, cols) in (row, column) order with their row_ptr."""
    from oracle import xmap_oracle as xo
    from xmap.engine import synth
    r = synth.make_two_domain(3, 8000, 8000, 8000, overlap=0.5)
    I, Is = r.n_items, r.n_src_items
    assert Is >= 7000 and I - Is >= 7000
    rng = np.random.RandomState(SEED)
    src = rng.permutation(Is)
    tgt = Is + rng.permutation(I - Is)
    nL = len(LENS)
    # Which hub gets which item matters where |sim| ties: a filler lists its partners of one |sim| by ascending column, so at
    # k = 3 and `one` it lists its three lowest hubs and nothing else.  The rows of more than 4096 entries get the lowest items
    # of the hubs of their domain, the longest row the highest of them: a long row is then listed by at least the fillers
    # that miss three of the (shorter) long rows below it, and its reverse lists are long (test_oracle_is_the_numpy_statement).
    long_n = [n for n in LENS if n > 4096]
    rest_n = [n for n in LENS if n <= 4096]
    s_items, t_items = np.sort(src[:2 * nL]).tolist(), np.sort(tgt[:nL]).tolist()
    s_hubs = [(kind, n) for n in long_n for kind in ("sb", "nb")]
    s_rest = [(kind, n) for n in rest_n for kind in ("sb", "nb")]
    s_hubs += [s_rest[q] for q in rng.permutation(len(s_rest))]
    t_hubs = long_n + [rest_n[q] for q in rng.permutation(len(rest_n))]
    hub = dict(sb={}, nb={}, tb=dict(zip(t_hubs, t_items)))
    for (kind, n), item in zip(s_hubs, s_items):
        hub[kind][n] = item
    fill = dict(s=src[2 * nL:], t=tgt[nL:])
    partners = {(kind, n): [] for kind in KINDS for n in LENS}
    for i, j in _bipartite([hub_degree(n) for n in LENS], rng):
        partners[("sb", LENS[i])].append(hub["tb"][LENS[j]])
        partners[("tb", LENS[j])].append(hub["sb"][LENS[i]])
    big = [n for n in LENS if n >= 63]
    for q, n in enumerate(LENS):
        for t in range(min(n, NB_LINKS)):
            m = big[(3 * q + 7 * t) % len(big)]          # (7 and len(big) = 26 are coprime: four different hubs)
            partners[("nb", n)].append(hub["sb"][m])
            partners[("sb", m)].append(hub["nb"][n])
    a, b = [], []
    for kind in KINDS:
        pool = fill["t" if kind == "tb" else "s"]
        for n in LENS:
            fixed = partners[(kind, n)]
            assert len(set(fixed)) == len(fixed) <= n, (kind, n)
            # rows of up to 4096 entries draw from the first BUSY fillers of the domain (a seeded order), longer ones from all:
            # the other fillers have a handful of long rows as their only partners, and list most of them at k = 3
            mine = np.concatenate([np.asarray(fixed, np.int64),
                                   rng.choice(pool if n > 4096 else pool[:BUSY], n - len(fixed), replace=False)])
            a.append(np.full(n, hub[kind][n], np.int64))
            b.append(mine)
    a, b = np.concatenate(a), np.concatenate(b)
    hubs = np.array([hub[kind][n] for kind in KINDS for n in LENS])
    both = np.isin(a, hubs) & np.isin(b, hubs)           # hub-hub pairs were listed from both ends
    first = both & (a < b)
    a, b = a[~both | first], b[~both | first]
    rows, cols = np.concatenate([a, b]), np.concatenate([b, a])
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    assert len(np.unique(rows * I + cols)) == len(rows) and np.all(rows != cols)
    c = Rows()
    c.r, c.I, c.Is, c.hub = r, I, Is, hub
    c.T = xo.Train(r.user_ptr, r.item, r.rating, r.time, I, *r.item_attrs())
    c.rows, c.cols = rows, cols
    c.row_ptr = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=I), out=c.row_ptr[1:])
    c.info = np.zeros((I, 4))
    c.info[:, 3] = 5.0
    c.is_hub = np.zeros(I, bool)
    c.is_hub[hubs] = True
    for x in (c.rows, c.cols, c.row_ptr, c.info, c.is_hub):
        x.setflags(write=False)
    return c


def family_values(family, rows, cols, seed=SEED):
    """sim of the directed pairs (rows[p], cols[p]): a function of the unordered pair, the seed and (`distinct`) the set"""
    a, b = np.minimum(rows, cols).astype(np.uint64), np.maximum(rows, cols).astype(np.uint64)
    key = (a << np.uint64(32)) | b
    h = _mix(key + np.uint64((0x9e3779b97f4a7c15 * (seed + 1)) & 0xffffffffffffffff))
    sign = np.where((h >> np.uint64(8)) & np.uint64(1), -1.0, 1.0)
    lvl = ((h >> np.uint64(16)) % np.uint64(4)).astype(np.int64)
    if family == "one":
        mag = np.full(len(key), 0.5)
    elif family == "levels4":
        mag = np.ldexp(1.0, -lvl)
    elif family == "zeros":
        mag = np.where(lvl == 3, 0.0, np.ldexp(1.0, -lvl))
    else:
        u, inv = np.unique(key, return_inverse=True)
        mag = (np.random.RandomState(seed).permutation(len(u))[inv] + 1.0) / (len(u) + 1.0)
    return np.ascontiguousarray(sign * mag, np.float64)


@functools.lru_cache(maxsize=None)
def family_sim(family):
    c = structure()
    sim = family_values(family, c.rows, c.cols)
    sim.setflags(write=False)
    return sim


@functools.lru_cache(maxsize=None)
def order_perm(family, order):
    """permutation of the entries (inside every row) from (row, column ascending) order to the storage order"""
    c = structure()
    a = np.abs(family_sim(family))
    if order == "col_asc":
        o = np.arange(len(c.rows))
    elif order == "col_desc":
        o = np.lexsort((-c.cols, c.rows))
    elif order == "abs_asc":
        o = np.lexsort((-c.cols, a, c.rows))
    elif order == "abs_desc":
        o = np.lexsort((c.cols, -a, c.rows))
    else:
        o = np.lexsort((np.random.RandomState(SEED + 1).rand(len(c.rows)), c.rows))
    assert np.array_equal(c.rows[o], c.rows)
    o.setflags(write=False)
    return o


def stored(family, order):
    """(row_ptr, col, sim, mutu, nij, info) of a family with every row in the given storage order: fresh arrays"""
    c = structure()
    o = order_perm(family, order)
    n = len(o)
    return (c.row_ptr.copy(), c.cols[o].astype(np.int32), family_sim(family)[o].copy(), np.ones(n, np.int32), np.ones(n, np.int32),
            c.info.copy())


def oracle_tables(family, k, order="col_asc"):
    """xo.extend(..., do_paths=False) of one family: Ext with bb, cls, cnt, col, val (the tails of col / val are unwritten)"""
    from oracle import xmap_oracle as xo
    c = structure()
    S = xo.sim_from_arrays(c.I, *stored(family, order))
    X = xo.extend(c.T, S, k, do_paths=False)
    xo.ext_free(X)          # (the arrays were copied out)
    xo.sim_free(S)
    return X


def numpy_tables(family, k):
    """The classified top-k lists, stated in NumPy from the definition: per row np.lexsort((col, -|sim|)); a bridge row's
    list A holds the partners of the other domain and list B those of its own; a non-bridge row's list A its bridge partners
    and list B every partner; the first k of each; a non-bridge row with an empty list A is dropped (class 0, counts 0).
    Returns (bb, cls, cnt [I][2], col [I][2][k], val [I][2][k][3]) with the tails zero."""
    c = structure()
    I, rows, cols, sim = c.I, c.rows, c.cols, family_sim(family)
    prefix, suffix, mask, _ = c.r.item_attrs()
    bb = np.zeros(I, np.uint8)
    bb[rows[prefix[rows] != prefix[cols]]] = 1
    o = np.lexsort((cols, -np.abs(sim), rows))
    r_, c_, s_ = rows[o], cols[o], sim[o]
    has = ((mask[c_] >> suffix[r_].astype(np.uint32)) & 1) != 0
    isbb = bb[r_] != 0
    pred = [np.where(isbb, ~has, bb[c_] != 0), np.where(isbb, has, True)]
    cnt = np.zeros((I, 2), np.int32)
    col = np.zeros((I, 2, k), np.int32)
    val = np.zeros((I, 2, k, 3), np.float64)
    for l in (0, 1):
        p = pred[l].astype(np.int64)
        before = np.cumsum(p) - p
        rank = before - before[c.row_ptr[:-1][r_]] if len(r_) else before      # class members earlier in the same row
        keep = pred[l] & (rank < k)
        cnt[:, l] = np.bincount(r_[keep], minlength=I)
        col[r_[keep], l, rank[keep]] = c_[keep]
        val[r_[keep], l, rank[keep], 0] = s_[keep]
        val[r_[keep], l, rank[keep], 1] = 1.0
        val[r_[keep], l, rank[keep], 2] = 1.0 * 1.0 / (5.0 + 5.0 - 1.0)
    n = np.diff(c.row_ptr)
    cls = np.where(bb != 0, 1, np.where(cnt[:, 0] > 0, 2, 0)).astype(np.uint8)
    cls[n == 0] = 0
    dropped = cls == 0
    full_cnt = cnt.copy()           # (what a dropped row WOULD list: the device writes those entries, the counts say 0)
    cnt[dropped] = 0
    return bb, cls, cnt, col, val, full_cnt


def held(cnt, k):
    return np.arange(k)[None, None, :] < cnt[:, :, None]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def thresholds(cnt, col, val):
    """(count, |value| of the last entry, its column) of every list, 0 for an empty one: KnnThr of csrc/paths.h"""
    I = cnt.shape[0]
    last = np.maximum(cnt - 1, 0)[:, :, None]
    la = np.abs(np.take_along_axis(val[..., 0], last, 2)[..., 0])
    lc = np.take_along_axis(col, last, 2)[..., 0]
    return cnt.copy(), np.where(cnt > 0, la, 0.0), np.where(cnt > 0, lc, 0).astype(np.int32)


def reverse_census(I, cls, cnt, col, flags):
    """entries per item of the attach and rnn lists, and the (src, joint) record counts, from the knn tables alone"""
    k = col.shape[2]
    h = held(cnt, k) & (cls == 2)[:, None, None]
    att = np.bincount(col[:, 0][h[:, 0]], minlength=I)
    rnn = np.bincount(col[:, 1][h[:, 1]], minlength=I)
    hh = held(cnt, k)
    r_all = np.broadcast_to(np.arange(I, dtype=np.int64)[:, None, None], hh.shape)
    s_ok = (cls == 1) & ((flags & 1) != 0) & (att > 0)          # src(t) = [s : s a source bridge with an attach list, s lists t]
    hs = hh & s_ok[:, None, None]
    s, t = r_all[hs], col[hs].astype(np.int64)
    m = (flags[t] & 2) != 0
    s, t = s[m], t[m]
    t_ok = hh & ((cls == 1) & (att > 0))[:, None, None]         # joint: t is such a bridge too and lists s
    joint = int(np.isin(t * I + s, r_all[t_ok] * I + col[t_ok]).sum())
    return att, rnn, len(s), joint


# ---------------------------------------------------------------------------------------------------------------- tests
def test_designed_row_lengths_are_exact():
    c = structure()
    n = np.diff(c.row_ptr)
    prefix = c.r.item_attrs()[0]
    for kind in KINDS:
        assert [int(n[c.hub[kind][m]]) for m in LENS] == list(LENS), kind
    assert len({c.hub[kind][m] for kind in KINDS for m in LENS}) == 3 * len(LENS)
    assert int((n > 2048).sum()) == 27 and int((n > 4096).sum()) == 9
    assert int(n[~c.is_hub].max()) <= 3 * len(LENS) and int((n[~c.is_hub] > 0).sum()) > 14000      # fillers: short rows
    # bridges are the sb / tb hubs with a partner, and nothing else (a filler or an nb hub has no partner of the other domain)
    cross = np.zeros(c.I, bool)
    cross[c.rows[prefix[c.rows] != prefix[c.cols]]] = True
    want = np.zeros(c.I, bool)
    want[[c.hub[kind][m] for kind in ("sb", "tb") for m in LENS if m > 0]] = True
    assert np.array_equal(cross, want)
    for m in LENS:          # hubs of the other domain per bridge hub: 1 to 12
        for kind in ("sb", "tb"):
            i = c.hub[kind][m]
            other = c.cols[c.row_ptr[i]:c.row_ptr[i + 1]]
            assert int((prefix[other] != prefix[i]).sum()) == hub_degree(m)
    # symmetric structure
    fwd = set(zip(c.rows.tolist(), c.cols.tolist()))
    assert all((b, a) in fwd for a, b in fwd)


@pytest.mark.parametrize("family", FAMILIES)
def test_family_values_and_storage_orders(family):
    c = structure()
    sim = family_sim(family)
    assert np.isfinite(sim).all() and (sim > 0).any() and (sim < 0).any()
    back = dict(zip(zip(c.rows.tolist(), c.cols.tolist()), bits(sim).tolist()))
    assert all(back[(b, a)] == v for (a, b), v in back.items())         # bit for bit, the sign of a zero included
    a = np.abs(sim)
    if family == "one":
        assert np.all(a == 0.5)
    elif family == "levels4":
        assert sorted(np.unique(a).tolist()) == [0.125, 0.25, 0.5, 1.0]
    elif family == "zeros":
        z = sim[a == 0.0]
        assert sorted(np.unique(a).tolist()) == [0.0, 0.25, 0.5, 1.0] and 0.2 < len(z) / len(sim) < 0.3
        assert np.signbit(z).any() and not np.signbit(z).all()
    else:
        assert len(np.unique(a)) == len(sim) // 2 and a.min() > 0.0
    seen = set()
    for order in ORDERS:
        row_ptr, col, s, mutu, nij, info = stored(family, order)
        rows = np.repeat(np.arange(c.I), np.diff(row_ptr))
        assert np.array_equal(rows, c.rows)
        o = np.lexsort((col, rows))
        assert np.array_equal(col[o], c.cols) and np.array_equal(bits(s[o]), bits(sim))       # the same matrix
        seen.add(col.tobytes())
        i = c.hub["nb"][6200]
        lo, hi = row_ptr[i], row_ptr[i + 1]
        key = np.abs(s[lo:hi]) * 2.0 ** 40 - col[lo:hi]       # (|sim| desc, col asc) as one number: |sim| steps are >= 2^-18
        if order == "abs_asc":
            assert np.all(np.diff(key) > 0)                   # every entry sorts before all the earlier ones
        if order == "abs_desc":
            assert np.all(np.diff(key) < 0)
    assert len(seen) == (5 if family != "one" else 3)         # (`one`: abs_asc is col_desc, abs_desc is col_asc)
    if family == "one":
        assert np.array_equal(order_perm(family, "abs_asc"), order_perm(family, "col_desc"))


@pytest.mark.parametrize("family,k", CASES)
def test_oracle_is_the_numpy_statement(family, k):
    """xo.extend on the designed rows = the NumPy statement, and the census of what the tables hold"""
    c = structure()
    I = c.I
    X = oracle_tables(family, k)
    bb, cls, cnt, col, val, full_cnt = numpy_tables(family, k)
    assert np.array_equal(X.bb, bb) and np.array_equal(X.cls, cls) and np.array_equal(X.cnt, cnt)
    h = held(cnt, k)
    assert np.array_equal(X.col[h], col[h]) and np.array_equal(bits(X.val[h]), bits(val[h]))
    assert not val[~held(full_cnt, k)].any() and not col[~held(full_cnt, k)].any()

    n = np.diff(c.row_ptr)
    flags = c.r.item_attrs()[3]
    sim = family_sim(family)
    long_rows = np.nonzero(n > 4096)[0]
    assert len(long_rows) >= 9 and int((n > 2048).sum()) >= 20
    # non-bridge rows whose FULL list 0 is cut inside a tie: an unlisted bridge partner has the |sim| of the last listed one
    nonb = cls == 2
    full0 = nonb & (cnt[:, 0] == k)
    la = np.abs(val[np.arange(I), 0, np.maximum(cnt[:, 0] - 1, 0), 0])
    cand = (bb[c.cols] != 0) & full0[c.rows] & (np.abs(sim) == la[c.rows])          # bridge partners at the last listed |sim|
    at_la = np.bincount(c.rows[cand], minlength=I)
    listed_at_la = ((np.abs(val[:, 0, :, 0]) == la[:, None]) & h[:, 0]).sum(1)
    cut_in_tie = int((full0 & (at_la > listed_at_la)).sum())
    print("%s k=%d: %d non-bridge rows, %d with a full list 0, %d cut inside a tie" % (family, k, nonb.sum(), full0.sum(), cut_in_tie))
    if family == "distinct":
        assert cut_in_tie == 0
    elif k in (3, 5):
        # a filler has about six bridge hubs as partners and `levels4` four levels: most full lists of 3 are cut in a tie
        assert cut_in_tie >= 1000
    if k >= 50:
        assert int(full0.sum()) == 0            # no non-bridge row has 50 bridge partners: list A stays short of k
    # every bridge hub row has one list shorter than 50: the <= 12 partners of the other domain ("threshold never set")
    for kind in ("sb", "tb"):
        for m in LENS:
            i = c.hub[kind][m]
            assert int(cls[i]) == (1 if m else 0)
            assert int(cnt[i, 0]) == min(k, hub_degree(m))
            if k >= 50 and m:
                assert cnt[i, 0] < k
    for m in LENS:                              # the non-bridge hubs: list A = the NB_LINKS bridge partners
        i = c.hub["nb"][m]
        assert int(cls[i]) == (2 if m else 0) and int(cnt[i, 0]) == min(k, m, NB_LINKS) and int(cnt[i, 1]) == min(k, m)
    # the reverse lists these tables lead to
    att, rnn, n_src, n_joint = reverse_census(I, cls, cnt, col, flags)
    print("%s k=%d: attach of the long rows %s, rnn %s, %d src records, %d joint" % (family, k, att[long_rows].tolist(),
                                                                                    rnn[long_rows].tolist(), n_src, n_joint))
    if k >= 3:
        # (a non-bridge item is in nobody's list A: the attach list of an `nb` hub is empty by definition)
        assert np.all(att[long_rows][bb[long_rows] != 0] >= 1000) and int((bb[long_rows] != 0).sum()) == 6
        assert np.all(att[long_rows][bb[long_rows] == 0] == 0)
        assert np.all(rnn[long_rows] >= 1000)
        assert n_src >= 50 and n_joint >= 30
    if family == "zeros" and k >= 3:            # (at k = 1 a zero is listed only where every partner's value is one)
        z = val[..., 0][h]
        z = z[z == 0.0]
        assert len(z) >= 100 and np.signbit(z).any() and not np.signbit(z).all()


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_ignores_the_storage_order(family):
    """B1-B4 of xo_extend sort with an explicit column tie-break: the same tables for every order inside a row"""
    for k in (3, 65):
        first = oracle_tables(family, k)
        h = held(first.cnt, k)
        for order in ORDERS[1:]:
            X = oracle_tables(family, k, order)
            assert np.array_equal(X.bb, first.bb) and np.array_equal(X.cls, first.cls) and np.array_equal(X.cnt, first.cnt)
            assert np.array_equal(X.col[h], first.col[h]) and np.array_equal(bits(X.val[h]), bits(first.val[h])), order
