"""The NumPy / Python statement of diversified top-N (include/xmap_hip.h: xmap_div_index, xmap_diversify_rows; DESIGN.md 4
"Diversified lists") and the builders of the designed inputs the tests feed to it and to the device.  No device, no torch.

Index: every row's entries by column ascending, dv_abs = fabs(sim); row_ptr is shared.  Re-ranking of one query: greedy
maximal marginal relevance over the pool -- obj = score - w * pen with one fp64 multiply and one fp64 subtract, the largest obj
wins and the smallest position on equal obj, pen = the largest |sim| to an item picked so far, the intra-list similarity is the
sum, in pick order, of the |sim| of every picked item to the ones picked before it over n (n - 1) / 2.  Python floats are fp64
and neither NumPy nor Python fuses, so the device must give the same bits."""
import numpy as np


def div_index(row_ptr, col, sim):
    """(dv_col, dv_abs, dups): dups = repeated (row, column) entries (the device refuses a CSR with any)"""
    row_ptr, col, sim = np.asarray(row_ptr, np.int64), np.asarray(col, np.int32), np.asarray(sim, np.float64)
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))
    o = np.lexsort((col, rows))             # (stable: equal keys keep their storage order)
    dv_col, dv_abs = col[o].copy(), np.abs(sim[o])
    dups = int(np.sum((rows[o][1:] == rows[o][:-1]) & (dv_col[1:] == dv_col[:-1]))) if len(o) > 1 else 0
    return dv_col, dv_abs, dups


def rerank_one(cnt, item, plain, decay, rank_by, w, n_top, n_items, row_ptr, dv_col, dv_abs):
    """one query: (n, [(item, plain, decay, pos, pen)*n], ils)"""
    cnt = int(cnt)
    n = min(cnt, int(n_top))
    score = [float(x) for x in (decay if rank_by else plain)[:cnt]]
    w = float(w)
    live = list(range(cnt))
    pen, tot, pairsum, out = [0.0] * cnt, [0.0] * cnt, 0.0, []
    for r in range(n):
        best, bo = -1, 0.0
        for j in live:                      # ascending: an equal obj keeps the smaller position
            t = w * pen[j]
            o = score[j] - t
            if best < 0 or o > bo:
                best, bo = j, o
        j = best
        out.append((int(item[j]), float(plain[j]), float(decay[j]), j, pen[j]))
        pairsum = pairsum + tot[j]
        live.remove(j)
        p = int(item[j])
        if r + 1 < n and 0 <= p < n_items:
            a, b = int(row_ptr[p]), int(row_ptr[p + 1])
            row = dv_col[a:b]
            for c in live:
                k = int(np.searchsorted(row, item[c]))
                if k < b - a and row[k] == item[c]:
                    v = float(dv_abs[a + k])
                    if v > pen[c]:
                        pen[c] = v
                    tot[c] = tot[c] + v
    ils = pairsum / (n * (n - 1) / 2) if n >= 2 else 0.0
    return n, out, ils


def rerank(cnt, item, plain, decay, rank_by, w, n_top, n_items, row_ptr, dv_col, dv_abs):
    """the arrays xmap_diversify_rows writes: (cnt [Q], item, plain, decay, pos, pen [Q][n_top], ils [Q], stats (changed, sum cnt))"""
    cnt = np.asarray(cnt)
    Q, n_top = len(cnt), int(n_top)
    item, plain, decay = (np.asarray(x).reshape(Q, -1) for x in (item, plain, decay))
    o_cnt = np.zeros(Q, np.int32)
    o_item, o_pos = np.full((Q, n_top), -1, np.int32), np.full((Q, n_top), -1, np.int32)
    o_plain, o_decay, o_pen, o_ils = np.zeros((Q, n_top)), np.zeros((Q, n_top)), np.zeros((Q, n_top)), np.zeros(Q)
    changed = 0
    for q in range(Q):
        n, out, ils = rerank_one(cnt[q], item[q], plain[q], decay[q], rank_by, w, n_top, n_items, row_ptr, dv_col, dv_abs)
        o_cnt[q], o_ils[q] = n, ils
        for r, (i, p, d, pos, pen) in enumerate(out):
            o_item[q, r], o_plain[q, r], o_decay[q, r], o_pos[q, r], o_pen[q, r] = i, p, d, pos, pen
        changed += any(e[3] != r for r, e in enumerate(out))
    return o_cnt, o_item, o_plain, o_decay, o_pos, o_pen, o_ils, (changed, int(o_cnt.sum()))


def bits(a):
    """the uint64 view of an fp64 array: the comparisons of the tests are array_equal on it"""
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same(got, want):
    """every array of a device result against the statement's, doubles by their bits"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if w.dtype == np.float64:
            assert g.dtype == np.float64 and np.array_equal(bits(g), bits(w)), k
        else:
            assert np.array_equal(g, w), k


# ---- designed inputs ------------------------------------------------------------------------------------------------------

def csr_of(rows, n_items):
    """{row: [(col, sim)*]} in the given storage order -> (row_ptr, col, sim)"""
    row_ptr = np.zeros(n_items + 1, np.int64)
    col, sim = [], []
    for i in range(n_items):
        for c, s in rows.get(i, ()):
            col.append(c); sim.append(s)
        row_ptr[i + 1] = len(col)
    return row_ptr, np.asarray(col, np.int32), np.asarray(sim, np.float64)


def shuffle_rows(rng, row_ptr, col, sim, how="shuffle"):
    """the same CSR with another order inside every row: 'shuffle', 'asc' or 'desc' by column"""
    col, sim = col.copy(), sim.copy()
    for i in range(len(row_ptr) - 1):
        a, b = int(row_ptr[i]), int(row_ptr[i + 1])
        if how == "shuffle":
            o = rng.permutation(b - a)
        else:
            o = np.argsort(col[a:b], kind="stable")
            o = o[::-1] if how == "desc" else o
        col[a:b], sim[a:b] = col[a:b][o], sim[a:b][o]
    return col, sim


def random_sym_csr(rng, n_items, density, values):
    """a symmetric similarity matrix without a diagonal: every unordered pair present with probability `density`, its value
    values(rng, count) with a random sign; rows in shuffled storage order.  Returns (row_ptr, col, sim, dense |sim| [I][I])"""
    iu, ju = np.triu_indices(n_items, 1)
    keep = rng.random(len(iu)) < density
    iu, ju = iu[keep], ju[keep]
    v = values(rng, len(iu)) * rng.choice([-1.0, 1.0], len(iu))
    r = np.concatenate([iu, ju]); c = np.concatenate([ju, iu]); s = np.concatenate([v, v])
    o = rng.permutation(len(r))
    o = o[np.argsort(r[o], kind="stable")]
    row_ptr = np.zeros(n_items + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n_items), out=row_ptr[1:])
    dense = np.zeros((n_items, n_items))
    dense[r, c] = np.abs(s)
    return row_ptr, c[o].astype(np.int32), s[o], dense


def eighths(rng, n):
    return rng.integers(1, 9, n) / 8.0


def random_pools(rng, n_query, n_pool, n_items, scores=None, min_cnt=2):
    """pools as xmap_topn_rows writes them: min_cnt..n_pool distinct items per query, scores sorted descending (plain in eighths
    by default, decayed = plain / 2), -1 / 0.0 behind the count"""
    cnt = rng.integers(min_cnt, n_pool + 1, n_query).astype(np.int32)
    item = np.full((n_query, n_pool), -1, np.int32)
    plain, decay = np.zeros((n_query, n_pool)), np.zeros((n_query, n_pool))
    for q in range(n_query):
        k = int(cnt[q])
        item[q, :k] = rng.choice(n_items, k, replace=False)
        s = (rng.integers(0, 41, k) / 8.0) if scores is None else scores(rng, k)
        plain[q, :k] = np.sort(s)[::-1]
        decay[q, :k] = plain[q, :k] / 2.0
    return cnt, item, plain, decay


def random_family(seed=20, n_items=400, density=0.30, n_query=200, n_pool=64):
    """the random family of the tests: 400 items, 30 % symmetric density, |sim| in eighths, pools of 2 .. 64 distinct items, scores
    in eighths sorted descending; re-ranked 64 -> 10"""
    rng = np.random.default_rng(seed)
    row_ptr, col, sim, dense = random_sym_csr(rng, n_items, density, eighths)
    return (row_ptr, col, sim, dense) + random_pools(rng, n_query, n_pool, n_items)
