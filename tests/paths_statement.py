"""An independent statement of what k_paths4 (csrc/paths4.hip) is given and what it does with it, in plain Python / NumPy from
the classified knn tables alone (cls [I], cnt [I][2], col [I][2][k]) and the item flags: the reverse lists, the tile directory
of the middle lists, the heads / batches / column visits of every start, the classes of code those visits reach
(column_census), the counters n_paths and n_updates, the per-start path counts and candidate counts, and the work-unit
plan (plan_statement: csrc/plan.hip).  Semantics from csrc/paths.h, mid_rows.hip, reverse.hip and oracle/xmap_oracle.c.
Nothing here imports the engine: Engine.ext_tables_from_knn is code under test.

List order.  rnn(y) and src(t) are built from row y / row t of the similarity matrix in the row's storage order
(reverse.hip); the designed matrices (tests/paths_families.py) and stage A store a row with ascending columns, so both lists
are ascending here.  The order decides which heads share a batch of 64, hence the visits and n_updates -- not n_paths.

Terms.  A column is a non-bridge item x; its ends are x and NN(x) = list 1 of x, ne = 1 + |NN(x)| of them.  A tile (x', x)
holds the records (t, s) with t in NB_BB(x') carrying the T flag, (t, s) joint and x in attach(s).  The heads of a start are
the start itself when it is a non-bridge record, then rnn(start); a batch is 64 consecutive heads; a visit is one (start,
batch, column): p participating heads (those with a tile on the column), R records, ne ends."""
import numpy as np

FLAG_S, FLAG_T = 1, 2
COST_CAP = (1 << 44) - 1
MERGE_GROUP = 12


class Statement(object):
    pass


def reverse_lists(cls, cnt, col, flags):
    """attach(b) = [x : x non-bridge record, b in NB_BB(x)], rnn(y) = [x : y in NB_NN(x)], both with x ascending;
    src(t) = [(s, joint)] with s ascending: s a bridge record carrying the S flag with a non-empty attach list and t (T flag)
    in either list of s; joint iff t is a bridge record with a non-empty attach list and s is in either list of t."""
    I = len(cls)
    attach, rnn, src = [[] for _ in range(I)], [[] for _ in range(I)], [[] for _ in range(I)]
    for x in np.nonzero(cls == 2)[0]:
        for b in col[x, 0, :cnt[x, 0]]:
            attach[b].append(int(x))
        for y in col[x, 1, :cnt[x, 1]]:
            rnn[y].append(int(x))
    both = lambda i: set(col[i, 0, :cnt[i, 0]].tolist()) | set(col[i, 1, :cnt[i, 1]].tolist())
    for s in np.nonzero(cls == 1)[0]:
        if not (flags[s] & FLAG_S) or not attach[s]:
            continue
        for t in sorted(both(s)):
            if flags[t] & FLAG_T:
                joint = cls[t] == 1 and len(attach[t]) > 0 and int(s) in both(t)
                src[t].append((int(s), bool(joint)))
    return attach, rnn, src


def statement(cls, cnt, col, flags, starts=None):
    """Everything the tests compare, as one object:
      attach, rnn, src          the reverse lists
      nb                        the non-bridge items, ascending (nb_list)
      dir_ptr [n_nb + 1], dir_x, dir_ne, dir_cnt   the tile directory, rows in nb order, tiles of a row in ascending x
      n_tiles, n_records
      visits                    int64 [n][10]: start, batch, column x, nloc, ne, R, p, largest head, straddle (a head whose records
                                cross a multiple of 16 in the visit's record order = lane order of the heads), lane of the first
                                participating head
      heads                     {start: [x' ...]} of the starts that have a head
      P [I]                     paths per start (xmap_path_weights), split as P_tiles + P_adds
      n_paths, n_updates        the counters of a pass over `starts` (default: all)
      n_cand [I]                distinct ends per start"""
    cls, cnt, col, flags = np.asarray(cls), np.asarray(cnt), np.asarray(col), np.asarray(flags)
    I = len(cls)
    St = Statement()
    St.I, St.k = I, col.shape[2]
    attach, rnn, src = reverse_lists(cls, cnt, col, flags)
    St.attach, St.rnn, St.src = attach, rnn, src
    nb = np.nonzero(cls == 2)[0]
    St.nb = nb
    ne_of = 1 + cnt[:, 1].astype(np.int64)
    # records behind every t, by column: J[t] = {x: joint (t, s) with x in attach(s)}
    J, njoint = {}, np.zeros(I, np.int64)
    for t in range(I):
        if not src[t]:
            continue
        d = {}
        for s, joint in src[t]:
            if joint:
                njoint[t] += 1
                for x in attach[s]:
                    d[x] = d.get(x, 0) + 1
        J[t] = d
    tiles = {}
    dir_ptr, dx, dn, dc = [0], [], [], []
    head_s = np.zeros(I, np.int64)            # paths x' - t - s of one head (head_S)
    for xp in nb:
        row = {}
        for t in col[xp, 0, :cnt[xp, 0]]:
            if flags[t] & FLAG_T:
                head_s[xp] += njoint[t]
                for x, n in J.get(int(t), {}).items():
                    row[x] = row.get(x, 0) + n
        xs = sorted(row)
        tiles[int(xp)] = (xs, [row[x] for x in xs])
        dx += xs; dn += [int(ne_of[x]) for x in xs]; dc += [row[x] for x in xs]
        dir_ptr.append(len(dx))
    St.tiles, St.head_s, St.flags = tiles, head_s, flags
    St.dir_ptr, St.dir_x, St.dir_ne, St.dir_cnt = (np.array(a, np.int64) for a in (dir_ptr, dx, dn, dc))
    St.n_tiles, St.n_records = len(dx), int(sum(dc))
    # tails behind (t, s): end s, then x and NN(x) for x in attach(s)
    tail = np.zeros(I, np.int64)
    for s in range(I):
        if attach[s]:
            tail[s] = 1 + sum(int(ne_of[x]) for x in attach[s])
    visits, heads_of = [], {}
    P_tiles, P_adds, upd_tiles = np.zeros(I, np.int64), np.zeros(I, np.int64), np.zeros(I, np.int64)
    n_cand = np.zeros(I, np.int64)
    ends_of_col = {}
    for start in range(I):
        heads = ([start] if cls[start] == 2 else []) + rnn[start]
        if heads:
            heads_of[start] = heads
        ends = set()
        if flags[start] & FLAG_T:             # role T: the non-joint paths from t = start
            for s, _ in src[start]:
                P_adds[start] += tail[s]
                ends.add(s)
                for x in attach[s]:
                    ends.update(_col_ends(ends_of_col, col, cnt, x))
        for xp in heads:
            P_adds[start] += head_s[xp]
            if head_s[xp]:
                for t in col[xp, 0, :cnt[xp, 0]]:
                    if flags[t] & FLAG_T:
                        ends.update(s for s, joint in src[t] if joint)
        for b in range(0, len(heads), 64):
            batch = heads[b:b + 64]
            cols = {}
            first = {}
            for lane, xp in enumerate(batch):
                xs, cs = tiles[xp]
                for x, c in zip(xs, cs):
                    cols.setdefault(x, []).append(c)
                    first.setdefault(x, lane)
            for x in sorted(cols):
                cs = cols[x]
                R, pos, straddle = sum(cs), 0, 0
                for c in cs:
                    if pos // 16 != (pos + c - 1) // 16:
                        straddle = 1
                    pos += c
                ne = int(ne_of[x])
                visits.append((start, b // 64, x, len(batch), ne, R, len(cs), max(cs), straddle, first[x]))
                P_tiles[start] += R * ne
                upd_tiles[start] += ne * ((R + 63) // 64)
                ends.update(_col_ends(ends_of_col, col, cnt, x))
        n_cand[start] = len(ends)
    St.visits = np.array(visits, np.int64).reshape(-1, 10)
    St.heads = heads_of
    St.P_tiles, St.P_adds, St.P = P_tiles, P_adds, P_tiles + P_adds
    St.upd = upd_tiles + P_adds
    sel = np.ones(I, bool)
    if starts is not None:
        sel[:] = False
        sel[np.asarray(starts, np.int64)] = True
    St.sel = sel
    St.n_paths, St.n_updates = int(St.P[sel].sum()), int(St.upd[sel].sum())
    St.n_cand = np.where(sel, n_cand, 0)
    St.ne_of = ne_of
    # home column of every end: the lowest column whose end list holds it (k_col_home); -1: in no column
    home = np.full(I, -1, np.int64)
    for x in nb[::-1]:
        home[list(_col_ends(ends_of_col, col, cnt, int(x)))] = x
    St.home = home
    St.col_ends = lambda x: _col_ends(ends_of_col, col, cnt, x)
    return St


def _col_ends(cache, col, cnt, x):
    e = cache.get(x)
    if e is None:
        e = cache[x] = frozenset([int(x)] + col[x, 1, :cnt[x, 1]].tolist())
    return e


NE_EXACT = (16, 17, 32, 33, 64, 65)
R_EXACT = (16, 17, 64, 65, 128, 129)
NH_EXACT = (1, 4, 5, 16, 17, 64, 65, 128, 129)


def column_census(St):
    """Named counts of the classes of code the visits of St reach (visits of the selected starts only).  Keys:
      visits; nloc<=4, nloc5-16, nloc17-64 (the three head-count classes of the column-minimum step); batch>0
      ne<=16, ne17-32, ne33-64, ne>64 (S = 4 / 2 / 1 slices; the second chunk of ends); ne=16 ... ne=65, ne=k+1; max_ne
      R=16 ... R=129, R>128 (groups of 16, rounds of 64); max_R
      head>16, head>64 (one head alone brings more than a group / a round); straddle; p>=17
      R>64&ne<=16, R>64&ne17-32, R>64&ne33-64, R>64&ne>64 (a second round on every slice class)
      late_home      visits in a batch > 0 of a column that holds an end whose home column an earlier batch of the same start
                     visited; late_home_own: that home column is the visited column itself -- the entry the first batch may
                     store without a load and a later one may not (the `fresh` argument of heads_Q)
      later_batches, later_empty (a batch > 0 without a column), later_one_head (a batch > 0 of one head: of those with a column)
      nH=1 ... nH=129 (starts with paths and exactly that many heads); max_nH
      last_lane@4 ... last_lane@64: visits of a batch of exactly that many heads in which the batch's last lane alone takes part"""
    V = St.visits[St.sel[St.visits[:, 0]]] if len(St.visits) else St.visits
    start, batch, x, nloc, ne, R, p, big, strad, first = (V[:, i] for i in range(10))
    c = {"visits": len(V)}
    n = lambda m: int(np.count_nonzero(m))
    c["nloc<=4"], c["nloc5-16"], c["nloc17-64"] = n(nloc <= 4), n((nloc > 4) & (nloc <= 16)), n(nloc > 16)
    c["batch>0"] = n(batch > 0)
    cls_ne = {"ne<=16": ne <= 16, "ne17-32": (ne > 16) & (ne <= 32), "ne33-64": (ne > 32) & (ne <= 64), "ne>64": ne > 64}
    for name, m in cls_ne.items():
        c[name] = n(m)
        c["R>64&" + name] = n(m & (R > 64))
    for v in NE_EXACT:
        c["ne=%d" % v] = n(ne == v)
    c["ne=k+1"] = n(ne == St.k + 1)
    for v in R_EXACT:
        c["R=%d" % v] = n(R == v)
    c["R>128"] = n(R > 128)
    c["head>16"], c["head>64"], c["straddle"], c["p>=17"] = n(big > 16), n(big > 64), n(strad > 0), n(p >= 17)
    for v in (4, 5, 16, 17, 64):
        c["last_lane@%d" % v] = n((nloc == v) & (p == 1) & (first == v - 1))
    c["max_ne"], c["max_R"] = (int(ne.max()), int(R.max())) if len(V) else (0, 0)
    # late_home: the columns of the earlier batches of a start, batch by batch (visits come in start, batch, column order)
    late = own = 0
    seen, cur, key = set(), set(), None
    for i in range(len(V)):
        s, b, xx = int(start[i]), int(batch[i]), int(x[i])
        if key is None or key[0] != s:
            seen, cur = set(), set()
        elif key[1] != b:
            seen |= cur
            cur = set()
        key = (s, b)
        cur.add(xx)
        if b > 0:
            homes = {int(St.home[e]) for e in St.col_ends(xx)}
            late += bool(homes & seen)
            own += xx in homes and xx in seen
    c["late_home"], c["late_home_own"] = late, own
    with_col = {(int(s), int(b)) for s, b in zip(start, batch)}
    later = empty = one = 0
    nh = {v: 0 for v in NH_EXACT}
    max_nh = 0
    for s, heads in St.heads.items():
        if not St.sel[s] or St.P[s] == 0:
            continue
        max_nh = max(max_nh, len(heads))
        if len(heads) in nh:
            nh[len(heads)] += 1
        for b in range(1, (len(heads) + 63) // 64):
            later += 1
            if (s, b) not in with_col:
                empty += 1
            elif len(heads) - 64 * b == 1:
                one += 1
    c["later_batches"], c["later_empty"], c["later_one_head"], c["max_nH"] = later, empty, one, max_nh
    for v in NH_EXACT:
        c["nH=%d" % v] = nh[v]
    return c


def plan_statement(P, lo, hi, chunk, chunk_div, max_rows):
    """xmap_path_plan (csrc/plan.hip) on the per-start path counts P: starts outside [lo, hi) count as zero; with chunk_div > 0
    the chunk is max(2^22, paths in the range // chunk_div); the chunk doubles until the rows of the heavy starts (those with
    more than `chunk` paths: G = ceil(P / chunk) rows each) are at most max_rows or the chunk exceeds the total; starts in the
    order of P // G descending (capped at 2^44 - 1), equal costs in start order; a start's G units follow each other, a heavy
    start's rows too.  -> dict(unit_start, unit_c, unit_G, unit_row, heavy_unit0, G, h_out = [units, heavy starts, rows,
    paths in the range, chunk])"""
    P = np.asarray(P, np.int64)
    I = len(P)
    if I == 0:
        z = np.zeros(0, np.int64)
        return dict(unit_start=z, unit_c=z, unit_G=z, unit_row=z, heavy_unit0=z, G=z, h_out=[0, 0, 0, 0, int(chunk)])
    idx = np.arange(I)
    p = np.where((idx >= lo) & (idx < hi), P, 0)
    total = int(p[p > 0].sum())
    chunk = int(chunk)
    if chunk_div > 0:
        chunk = max(total // int(chunk_div), 1 << 22)
    while True:
        G = np.where(p > chunk, -(-p // chunk), (p > 0).astype(np.int64))
        rows = int(G[G > 1].sum())
        if rows <= max_rows or chunk > total:
            break
        chunk *= 2
    starts = np.nonzero(G > 0)[0]
    cost = np.minimum(P[starts] // G[starts], COST_CAP)
    order = starts[np.argsort(-cost, kind="stable")]
    us, uc, ug, ur, h0 = [], [], [], [], []
    row = 0
    for s in order:
        g = int(G[s])
        if g > 1:
            h0.append(len(us))
        for c in range(g):
            us.append(int(s)); uc.append(c); ug.append(g); ur.append(row + c if g > 1 else -1)
        if g > 1:
            row += g
    a = lambda v: np.array(v, np.int64)
    return dict(unit_start=a(us), unit_c=a(uc), unit_G=a(ug), unit_row=a(ur), heavy_unit0=a(h0), G=G,
                h_out=[len(us), len(h0), row, total, chunk])


def unit_work(St, start, G):
    """the units c of a start cut into G that receive work, as k_paths4 deals its entries: numbered, role T first, then one per
    head (its paths x' - t - s), then one per (batch, column range); entry number % G is the unit"""
    heads = St.heads.get(int(start), [])
    role = 1 if (St.flags[start] & FLAG_T) else 0
    nbatch = (len(heads) + 63) // 64
    RX = -(-G // nbatch) if nbatch else 1
    work = set()
    if role and St.src[start]:
        work.add(0)
    for h, xp in enumerate(heads):
        if St.head_s[xp]:
            work.add((role + h) % G)
    n_nb = len(St.nb)
    cuts = [0 if rx == 0 else int(St.nb[rx * n_nb // RX]) for rx in range(RX)] + [1 << 31]
    V = St.visits[St.visits[:, 0] == start]
    for b, x in zip(V[:, 1], V[:, 2]):
        rx = int(np.searchsorted(cuts, x, side="right")) - 1
        work.add((role + len(heads) + int(b) * RX + rx) % G)
    return work, RX


def range_census(St, G):
    """What the unit plan of per-start chunk counts G (plan_statement) reaches.  A heavy start's batches are cut into RX =
    ceil(G / batches) column ranges at the items nb[rx * n_nb // RX] (k_paths4).  -> dict(G = the chunk counts that occur,
    rx1 = heavy starts with RX == 1, rx>1 = with RX > 1, hi_range = visits of heavy starts that fall into a range > 0 (found
    through the directory bisection), odd_group = heavy starts whose G leaves a merge group of one row, deep_rows = rows
    with work at position >= MERGE_GROUP of their start (what the second merge level has to fold in))"""
    n_nb = len(St.nb)
    out = dict(G=sorted(set(int(g) for g in G if g > 1)), rx1=0, hi_range=0, odd_group=0, deep_rows=0)
    out["rx>1"] = 0
    V = St.visits
    for s in np.nonzero(np.asarray(G) > 1)[0]:
        g = int(G[s])
        work, RX = unit_work(St, s, g)
        out["rx1" if RX == 1 else "rx>1"] += 1
        out["odd_group"] += (g > MERGE_GROUP and g % MERGE_GROUP == 1)
        out["deep_rows"] += sum(1 for c in work if c >= MERGE_GROUP)
        if RX > 1:
            cut1 = St.nb[1 * n_nb // RX]
            out["hi_range"] += int(np.count_nonzero((V[:, 0] == s) & (V[:, 2] >= cut1)))
    return out
