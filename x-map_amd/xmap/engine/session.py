"""Host-side plumbing between the reference's record formats and the device engine.

  trainRDD records   (uid, [(iid, rating, time)*])           -> DeviceRatings (index space, HBM)
  item2item_simRDD   ((iid1, iid2), (sim, mutu, frac, label)) <-> SimResult
  extended_simRDD    (start_iid, [(end_iid, xsim)*])          <-> ExtResult
  alterEgo_profile   (uid, iid, rating, time)                 <-  GenResult

The id dictionary built from a trainRDD is shared by the three stages; engines are
cached per trainRDD object so that generator_pipeline reuses the one stage A uploaded.
"""
import math
import weakref

import numpy as np

from . import ids as xids
from .localrdd import LocalRDD, records_of

_engines = {}   # id(trainRDD) -> (weakref or None, TrainState, fingerprint or None)


def float32_rating_error(uid, iid, value):
    """the ValueError for a caller rating that float32 -- the rating type of the three stages -- cannot hold exactly: the
    AlterEgo means would be taken over a different value than the one the caller passed"""
    return ValueError("rating %r of user %r, item %r is not exactly representable as float32 (the engine's rating type); "
                      "round the ratings to np.float32 first, e.g. float(np.float32(r))" % (value, uid, iid))


def check_float32(ptr, item, rating64, uids, iids):
    """raise float32_rating_error for the first rating of a CSR (trainRDD order) that float32 does not hold exactly
    (NaN passes: it stays NaN)"""
    r64 = np.asarray(rating64, np.float64)
    r32 = r64.astype(np.float32).astype(np.float64)
    bad = np.nonzero((r32 != r64) & ~np.isnan(r64))[0]
    if len(bad):
        e = int(bad[0])
        u = int(np.searchsorted(ptr, e, side="right") - 1)
        raise float32_rating_error(uids[u], iids[int(item[e])], float(r64[e]))


class TrainState(object):
    def __init__(self, records):
        from . import device
        self.idt = xids.IdTable.from_records(records)
        iidx = self.idt.iidx
        n = sum(len(p) for _, p in records)
        ptr = np.zeros(len(records) + 1, np.int64)
        item = np.empty(n, np.int32)
        rating = np.empty(n, np.float32)
        self.times = []          # original time objects, device carries their position
        self.ratings = []        # original rating objects (pass-through rows keep them)
        e = 0
        for u, (_, prof) in enumerate(records):
            for (iid, r, t) in prof:
                item[e] = iidx[iid]
                rating[e] = r
                if float(rating[e]) != float(r) and r == r:          # (NaN stays NaN)
                    raise float32_rating_error(records[u][0], iid, r)
                self.times.append(t)
                self.ratings.append(r)
                e += 1
            ptr[u + 1] = e
        self.R = device.DeviceRatings(ptr, item, rating, np.arange(n, dtype=np.int64), len(self.idt.iids),
                                      self.idt.attrs)
        self.engine = device.Engine(self.R)


def _fingerprint(records):
    """content key of a record list that cannot be weak-referenced: every (uid, iid, rating, time) takes part, so ratings edited
    in place -- or a new list of the same shape behind a recycled id(), such as a CV fold with perturbed ratings -- never
    hit the cache of the previous upload.  O(ratings) of host work per call, paid by plain-list inputs only (an RDD
    object is keyed by identity through a weak reference)."""
    h, n = 1469598103934665603, 0
    for rec in records:
        uid, prof = rec[0], rec[1]
        ph = hash((uid, len(prof), tuple((e[0], float(e[1]), e[2]) for e in prof)))      # (times too: AlterEgo rows and the decay read them)
        h = ((h ^ (ph & 0xFFFFFFFFFFFFFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        n += len(prof)
    return (len(records), n, h)


def train_state(trainRDD):
    """The TrainState (id dictionary + ratings in HBM + engine) of a trainRDD, shared by the three stages.  Cached per
    trainRDD object through a weak reference; inputs that cannot be weak-referenced (plain lists) are keyed on a content
    fingerprint and only the most recent one is kept, so a recycled id() can neither leak the previous engine nor be
    mistaken for it.  release() drops everything."""
    key = id(trainRDD)
    hit = _engines.get(key)
    if hit is not None:
        ref, st, fp = hit
        if ref is not None and ref() is trainRDD:
            return st
        if ref is None and fp == _fingerprint(records_of(trainRDD)):
            return st
        _engines.pop(key, None)
    feed = getattr(trainRDD, "feed", None)
    if feed is not None and getattr(trainRDD, "_items", None) is None:
        from . import feeder                       # native records (xmap.engine.feeder.FeedRDD): no Python loop over them
        recs = None
        st = feeder.train_state_from_feed(feed)
    else:
        recs = records_of(trainRDD)
        st = TrainState(recs)
    try:
        ref = weakref.ref(trainRDD, lambda _r, k=key: _engines.pop(k, None))
        fp = None
    except TypeError:
        ref, fp = None, _fingerprint(recs)
        for k in [k for k, v in _engines.items() if v[0] is None]:      # one strong entry at most
            _engines.pop(k, None)
    _engines[key] = (ref, st, fp)
    return st


def release(trainRDD=None):
    """drop the cached engine of one trainRDD (or of all): frees its HBM buffers and accumulator scratch"""
    if trainRDD is None:
        _engines.clear()
    else:
        _engines.pop(id(trainRDD), None)


# ---------------------------------------------------------------------------------------------
class SimPairsRDD(LocalRDD):
    """item2item_simRDD: ((iid1, iid2), (sim, mutu, frac_mutu, label)) -- rows live in HBM."""

    def __init__(self, state, S, ctx=None):
        LocalRDD.__init__(self, None, ctx)
        self.state, self.S = state, S

    def _rows(self):
        S, idt = self.S, self.state.idt
        row_ptr = S.row_ptr.cpu().numpy()
        rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
        col = S.col.cpu().numpy()
        o = np.lexsort((col, rows))        # canonical order: (iid1, iid2) ascending
        rows, col = rows[o], col[o]
        sim = S.sim.cpu().numpy()[o]
        mutu = S.mutu.cpu().numpy()[o].astype(np.float64)
        info = S.info.cpu().numpy()
        frac = mutu / (info[rows, 3] + info[col, 3] - S.nij.cpu().numpy()[o])
        pre = self.state.idt.attrs[0]
        label = (pre[rows] != pre[col]).astype(int)
        iids = idt.iids
        return [((iids[a], iids[b]), (float(s), float(m), float(f), int(lab)))
                for a, b, s, m, f, lab in zip(rows, col, sim, mutu, frac, label)]


class RecSimRDD(LocalRDD):
    """alterEgo_sim of recommender_calculate_sim_pipeline: ((iid1, iid2), [sim, local sensitivity]) -- rows live in
    HBM (Engine.rec_sim); both directions of every pair, an item paired with itself once."""

    def __init__(self, S, iids, ctx=None, engine=None):
        LocalRDD.__init__(self, None, ctx)
        self.S, self.iids, self.engine = S, iids, engine

    def select_neighbors(self, keep):
        """nonprivate_neighbor_selection on the device: [(iid, [(nid, [sim, ls])*])*], items in id order"""
        cnt, col, sim, ls = [x.cpu().numpy() for x in self.engine.rec_select(self.S, int(keep))]
        iids = self.iids
        return [(iids[i], [(iids[col[i, t]], [float(sim[i, t]), float(ls[i, t])]) for t in range(cnt[i])])
                for i in range(len(iids)) if cnt[i]]

    def _rows(self):
        S, iids = self.S, self.iids
        row_ptr = S.row_ptr.cpu().numpy()
        rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
        col = S.col.cpu().numpy()
        o = np.lexsort((col, rows))        # canonical order: (iid1, iid2) ascending
        sim, ls = S.sim.cpu().numpy()[o], S.ls.cpu().numpy()[o]
        return [((iids[a], iids[b]), [float(s), float(l)]) for a, b, s, l in zip(rows[o], col[o], sim, ls)]


def rec_sim_from_profiles(user_profiles, cap, ctx=None):
    """user_profiles: [(uid, [(iid, rating, time)*])*] (the user-based AlterEgo profile).  Builds the index space
    (items in lexicographic id order), uploads the CSR and runs Engine.rec_sim."""
    import torch
    from . import device
    recs = records_of(user_profiles)
    iids = sorted({t[0] for _, prof in recs for t in prof})
    iidx = {s: k for k, s in enumerate(iids)}
    ptr = np.zeros(len(recs) + 1, np.int64)
    item, rating = [], []
    for k, (_, prof) in enumerate(recs):
        ptr[k + 1] = ptr[k] + len(prof)
        item.extend(iidx[t[0]] for t in prof)
        rating.extend(float(t[1]) for t in prof)
    dev = "cuda:%d" % torch.cuda.current_device()
    # fp64 all the way: AlterEgo ratings are np.float64 means (reference core/generator.py:123-138), and that is what
    # RecommenderSim multiplies (core/recommenderSim.py:64-133)
    R = device.DeviceRatings(ptr, np.asarray(item, np.int32), np.asarray(rating, np.float64),
                             np.zeros(len(item), np.int64), len(iids), xids.item_attrs(iids), dev, rating64=True)
    eng = device.Engine(R)
    S = eng.rec_sim(cap)
    return RecSimRDD(S, iids, ctx, eng)


class ExtendedSimRDD(LocalRDD):
    """extended_simRDD: (start_iid, [(end_iid, xsim)*]) -- a LAZY handle.  The pass behind it keeps, per start item, the
    number of candidates and the XMAP_TOPC best by |xsim| (all a Generator reads: generator.py:85,109) in HBM.  The full
    lists (4.6e9 pairs at BASELINE configs[1]) are only produced when somebody iterates / collects this RDD: the
    enumeration then runs once more with list buffers sized exactly from the candidate counts."""

    def __init__(self, state, E, ctx=None):
        LocalRDD.__init__(self, None, ctx)
        self.state, self.E = state, E

    @property
    def materialised(self):
        return getattr(self.E, "xs_end", None) is not None

    def _rows(self):
        self.state.engine.extend_lists(self.E)
        E, iids = self.E, self.state.idt.iids
        I = len(iids)
        n_cand = E.n_cand.cpu().numpy()[:I]
        off = E.xs_off.cpu().numpy()[:I]
        xe, xv = E.xs_end.cpu().numpy(), E.xs_val.cpu().numpy()
        out = []
        for s in np.nonzero(n_cand)[0]:
            e = xe[off[s]:off[s] + n_cand[s]]
            v = xv[off[s]:off[s] + n_cand[s]]
            o = np.argsort(e)               # canonical order: end id ascending
            out.append((iids[s], [(iids[j], float(x)) for j, x in zip(e[o], v[o])]))
        return out


class AlterEgoRDD(LocalRDD):
    """alterEgo_profile: (uid, iid, rating, time) rows -- generator.py:140-157."""

    def __init__(self, state, G, ctx=None):
        LocalRDD.__init__(self, None, ctx)
        self.state, self.G = state, G

    def _rows(self):
        G, st = self.G, self.state
        u = G.user.cpu().numpy()
        it = G.item.cpu().numpy()
        r = G.rating.cpu().numpy()
        pos = G.time.cpu().numpy()          # position of the source row in trainRDD order
        nt = G.n_target_rows
        uids, iids = st.idt.uids, st.idt.iids
        out = []
        for q in range(len(u)):
            # pass-through rows keep the caller's rating object; AlterEgo rows carry the mean
            rating = st.ratings[pos[q]] if q < nt else np.float64(r[q])
            out.append((uids[u[q]], iids[it[q]], rating, st.times[pos[q]]))
        return out


def time_rank(state):
    """int64 device tensor over the positions of the train rows: the dense rank of the caller's time objects (their order
    and their ties; the device never sees the objects).  Built once per train state."""
    key = getattr(state, "_time_rank", None)
    if key is None:
        import torch
        when = getattr(state.times, "when", None)
        if when is not None:                        # native feed: numbers already
            rank = np.unique(np.asarray(when), return_inverse=True)[1]
        else:
            order = {t: k for k, t in enumerate(sorted(set(state.times)))}
            rank = np.fromiter((order[t] for t in state.times), np.int64, len(state.times))
        key = state._time_rank = torch.from_numpy(np.ascontiguousarray(rank, np.int64).reshape(-1)).to(state.engine.dev)
    return key


class _UnionState(object):
    """what the tail reads of a train state, over the id tables of a union: .idt (uids, iids, uidx, iidx) and .engine (its
    device and timers: the first part's)"""

    def __init__(self, idt, engine):
        self.idt, self.engine = idt, engine


class AlterEgoUnion(LocalRDD):
    """union_alterego's handle: the AlterEgo rows of several two-domain problems as ONE set of profiles on the device
    (Engine.union_profiles), over joint id tables.  Iterates like handles[0].union(handles[1]) ... [.distinct()]: the same
    tuples in the same order (that order is part-major, so iterating collects the parts' rows on the host; the tail does not).
    .state.idt holds the joint tables, .counts = (rows, duplicates removed, rows dropped, users with a row)."""

    def __init__(self, handles, distinct, state, parts, ctx=None):
        LocalRDD.__init__(self, None, ctx)
        self.handles, self.distinct_rows, self.state, self._parts = list(handles), bool(distinct), state, parts
        self._P = None

    def _rows(self):
        out = [row for h in self.handles for row in h.collect()]
        return LocalRDD(out).distinct().collect() if self.distinct_rows else out

    def profiles(self):
        """the union's user-major profiles (built once): the view Engine.union_profiles returns"""
        if self._P is None:
            from . import device
            idt = self.state.idt
            self._P = device.Engine.union_profiles(self._parts, len(idt.uids), len(idt.iids), self.distinct_rows,
                                                   timers=self.state.engine.timers)
        return self._P

    @property
    def counts(self):
        return self.profiles().counts


def _common_time_ranks(states):
    """per train state the int64 device tensor time_rank gives, but ranked over the time objects of ALL the states, so that
    the ranks of different domains compare (their order and their ties)"""
    import torch
    whens = [getattr(st.times, "when", None) for st in states]
    if all(w is not None for w in whens):               # native feeds: numbers already
        arrs = [np.asarray(w).reshape(-1) for w in whens]
        inv = np.unique(np.concatenate(arrs), return_inverse=True)[1].reshape(-1)
        cuts = np.cumsum([0] + [len(a) for a in arrs])
        ranks = [inv[cuts[k]:cuts[k + 1]] for k in range(len(arrs))]
    else:
        times = [list(w) if w is not None else st.times for st, w in zip(states, whens)]
        order = {t: k for k, t in enumerate(sorted(set().union(*[set(ts) for ts in times])))}
        ranks = [np.fromiter((order[t] for t in ts), np.int64, len(ts)) for ts in times]
    return [torch.from_numpy(np.ascontiguousarray(r, np.int64)).to(st.engine.dev) for r, st in zip(ranks, states)]


def union_alterego(handles, distinct=True):
    """The union of the AlterEgoRDD handles of several two-domain problems -- the multi-domain pipeline's
    alterEgo_profile1.union(alterEgo_profile2) and, with distinct, .distinct() (reference code/multidomain_demo.py:128) -- kept on
    the device.  The host builds only the tables: the joint uids (sorted) and iids (sorted; the items that occur in AlterEgo rows
    -- every other item of a part maps to -1), each part's user and item map into them, and ONE dense rank of the time objects of
    all parts.  Returns an AlterEgoUnion; recommend, recommend_topn and evaluate_topn take it wherever they take an AlterEgoRDD
    (fold-in does not: it needs one replacement map)."""
    import torch
    handles = list(handles)
    if not handles or not all(isinstance(h, AlterEgoRDD) for h in handles):
        raise TypeError("union_alterego() takes a list of AlterEgoRDD handles of generator_pipeline")
    states = [h.state for h in handles]
    held = []                                           # per part: the local items that occur in its rows
    for h in handles:
        held.append(torch.unique(h.G.item[:h.G.n_rows]).cpu().numpy() if h.G.n_rows else np.zeros(0, np.int64))
    uids = sorted(set().union(*[set(st.idt.uids) for st in states]))
    iids = sorted(set().union(*[{st.idt.iids[i] for i in its.tolist()} for st, its in zip(states, held)]))
    idt = xids.IdTable(uids, iids)
    ranks = _common_time_ranks(states)
    parts = []
    for h, st, its, rank in zip(handles, states, held, ranks):
        user_map = np.fromiter((idt.uidx[u] for u in st.idt.uids), np.int32, len(st.idt.uids))
        item_map = np.full(len(st.idt.iids), -1, np.int32)
        for i in its.tolist():
            item_map[i] = idt.iidx[st.idt.iids[i]]
        parts.append((h.G, user_map, item_map, rank[h.G.time] if h.G.n_rows else h.G.time))
    return AlterEgoUnion(handles, distinct, _UnionState(idt, states[0].engine), parts, getattr(handles[0], "ctx", None))


def _no_fold_in(alterEgoRDD, who):
    if isinstance(alterEgoRDD, AlterEgoUnion):
        raise TypeError("%s(): fold-in needs one replacement map, and a union of AlterEgo rows has one per part; fold the "
                        "profiles in against one part's AlterEgoRDD" % who)


def _tail_profiles(alterEgoRDD, who):
    """the profiles of the AlterEgo rows.  Returns (state, engine over the profiles, P)."""
    from . import device
    if isinstance(alterEgoRDD, AlterEgoUnion):
        st = alterEgoRDD.state
        eng = st.engine
        P = alterEgoRDD.profiles()
    elif isinstance(alterEgoRDD, AlterEgoRDD):
        st, G = alterEgoRDD.state, alterEgoRDD.G
        eng = st.engine
        key = time_rank(st)[G.time] if G.n_rows else G.time
        P = eng.alterego_profiles(G, time_key=key)
    else:
        raise TypeError("%s() takes the AlterEgoRDD handle of generator_pipeline (rows resident on the device) or the "
                        "AlterEgoUnion of union_alterego" % who)
    eng2 = device.Engine(P)
    eng2.timers = eng.timers
    return st, eng2, P


def _tail_matrix(alterEgoRDD, cap, who):
    """the front of every tail call: profiles of the AlterEgo rows -> RecommenderSim.  Returns (state, engine over the profiles, P,
    S); no neighbour list is selected."""
    st, eng2, P = _tail_profiles(alterEgoRDD, who)
    S = eng2.rec_sim(int(cap))
    return st, eng2, P, S


def _tail_setup(alterEgoRDD, cap, keep, neighbors, who):
    """what recommend and recommend_topn share: profiles of the AlterEgo rows -> RecommenderSim -> neighbour lists (selected on
    the device, or the caller's lists as arrays).  Returns (state, engine over the profiles, P, S, (cnt, col, sim), item_avg)."""
    import torch
    st, eng2, P, S = _tail_matrix(alterEgoRDD, cap, who)
    idt = st.idt
    dev = st.engine.dev
    I = len(idt.iids)
    item_avg = S.info[:I, 0].contiguous()
    if neighbors is None:
        nb = eng2.rec_select(S, int(keep))[:3]
    else:
        lists = dict(neighbors) if not isinstance(neighbors, dict) else neighbors
        width = max([len(v) for v in lists.values()] + [1])
        if width > 64:
            raise ValueError("a neighbour list holds %d entries; the device prediction takes up to 64" % width)
        cnt = np.zeros(max(I, 1), np.int32)
        col = np.full((max(I, 1), width), -1, np.int32)
        sim = np.zeros((max(I, 1), width), np.float64)
        for iid, lst in lists.items():
            i = idt.iidx[iid]
            cnt[i] = len(lst)
            for q, (nid, sv) in enumerate(lst):
                col[i, q] = idt.iidx[nid]
                sim[i, q] = sv
        nb = tuple(torch.from_numpy(a).to(dev) for a in (cnt, col, sim))
    return st, eng2, P, S, nb, item_avg


def _decay_table(alpha, n_w, dev):
    import torch
    return torch.from_numpy(np.asarray([np.exp(- alpha * d) for d in range(n_w)], np.float64)).to(dev)     # scalar np.exp, like the reference


def _tail_dicts(res, st, S, nb):
    """.item_info {iid: (avg, norm, n)} and .sim_pairs {iid: [(nid, sim)*]} of a tail result"""
    cnt, col, sim = [x.cpu().numpy() for x in nb]
    info, iids = S.info.cpu().numpy(), st.idt.iids
    I = len(iids)
    res.item_info = {iids[i]: (float(info[i, 0]), float(info[i, 1]), int(info[i, 3])) for i in range(I) if info[i, 3] > 0}
    res.sim_pairs = {iids[i]: [(iids[col[i, t]], float(sim[i, t])) for t in range(cnt[i])] for i in range(I) if cnt[i] > 0}


def recommend(alterEgoRDD, testRDD, cap, keep, alpha, neighbors=None):
    """The recommender tail on the device, from an AlterEgoRDD handle to the records of
    RecommenderPrediction.item_based_recommendation: profiles of the AlterEgo rows (Engine.alterego_profiles), RecommenderSim
    (rec_sim, cap), neighbour selection (rec_select, keep = mapping_range; or `neighbors`: the lists a host-side selection
    made, [(iid, [(nid, sim)*])*] or a dict of them -- the private route), prediction with temporal decay alpha and no limit
    on the evidence of a pair (Engine.predict).  Returns a LocalRDD of (uid, [(iid, real, plain, decayed) | ()]) in testRDD
    order, usable with calculate_mae; it carries .mae (count, sum |real - plain|, sum |real - decayed| from the device, or
    None when a real rating is not a number), .item_info {iid: (avg, norm, n)} and .sim_pairs {iid: [(nid, sim)*]}: the
    dictionaries the Python statement takes.  A user id matches by equality."""
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend")
    idt = st.idt
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    res = _predict_records(st, eng2, P, nb, item_avg, uidx, testRDD, alpha)
    _tail_dicts(res, st, S, nb)
    return res


def _predict_records(st, eng2, P, nb, item_avg, uidx, testRDD, alpha, iidx=None, n_items=None):
    """what recommend, recommend_profiles and recommend_items share: the held-out pairs of testRDD against the profiles P (uidx:
    uid -> user index of P; iidx: iid -> item index of the tables, default the train set's; n_items: the items of the tables
    when they are extended ones) -> the LocalRDD of (uid, [(iid, real, plain, decayed) | ()]) with .mae"""
    import torch
    idt, dev = st.idt, st.engine.dev
    iidx = idt.iidx if iidx is None else iidx
    recs = records_of(testRDD)
    tu = np.fromiter((uidx.get(uid, -1) for uid, pairs in recs for _ in pairs), np.int32)
    ti = np.fromiter((iidx.get(pair[0], -1) for _, pairs in recs for pair in pairs), np.int32)
    try:
        real = np.fromiter((float(pair[1]) for _, pairs in recs for pair in pairs), np.float64)
    except (TypeError, ValueError):
        real = None
    d_tu, d_ti = torch.from_numpy(tu).to(dev), torch.from_numpy(ti).to(dev)
    n_w = 66
    while True:
        wtab = _decay_table(alpha, n_w, dev)
        plain, decay, status, max_now = eng2.predict(P, nb, d_tu, d_ti, item_avg, wtab, n_items=n_items)
        if max_now <= n_w:
            break
        n_w = max_now
    mae = None
    if real is not None and len(tu):
        mae = tuple(eng2.mae(status, torch.from_numpy(real).to(dev), plain, decay).tolist())
    plain, decay, status = plain.cpu().numpy(), decay.cpu().numpy(), status.cpu().numpy()
    out, q = [], 0
    for uid, pairs in recs:
        line = []
        for pair in pairs:
            if status[q] == 0:
                line.append((pair[0], pair[1], float(plain[q]), float(decay[q])))
            elif status[q] == 1:
                line.append(())
            else:
                raise ZeroDivisionError("prediction of (%r, %r): zero weight sum or non-finite value (the reference raises here)"
                                        % (uid, pair[0]))
            q += 1
        out.append((uid, line))
    res = LocalRDD(out, getattr(testRDD, "ctx", None))
    res.mae = mae
    return res


def _eligibility(dev, labels, index, n_ids, allow, exclude, min_score):
    """The eligibility rules of a top-N / audience call as the keyword arguments of Engine.topn / Engine.audience: allow = the ids
    (id strings) that may be returned, exclude = {query label: ids never returned for it}, min_score = floor on the ranking score;
    index = {id string: index below n_ids}, labels = the query labels in query order.  Ids the dictionary does not know are
    ignored.  All three None: {} -- the unfiltered call."""
    if allow is None and exclude is None and min_score is None:
        return {}
    import torch
    from . import filters
    kw = {}
    if allow is not None:
        ids = [index[x] for x in (allow.collect() if hasattr(allow, "collect") else allow) if x in index]
        kw["allow"] = torch.from_numpy(filters.pack_mask(np.asarray(ids, np.int64), n_ids).view(np.int32)).to(dev)
    if exclude is not None:
        ptr, ids = filters.exclusion_csr([[index[x] for x in exclude.get(lab, ()) if x in index] for lab in labels])
        kw["exclude"] = (torch.from_numpy(ptr).to(dev), torch.from_numpy(ids).to(dev))
    if min_score is not None:
        kw["min_score"] = float(min_score)
    return kw


def recommend_topn(alterEgoRDD, users, cap, keep, alpha, n, decay=False, keep_held=False, neighbors=None, explain=None,
                   allow_items=None, exclude=None, min_score=None, diversify=None, pool=None, fill=None):
    """Top-N recommendation on the device from an AlterEgoRDD handle: the set-up of recommend (profiles -> RecommenderSim ->
    neighbour lists, or `neighbors`), then for every uid of `users` the n (1..64) best items its own rows give evidence for,
    ranked by the unrounded prediction -- without temporal decay, or with (decay=True, alpha) -- score descending, item id
    ascending on equal scores; items the user already holds are left out unless keep_held (Engine.topn).  Returns a LocalRDD
    of (uid, [(iid, plain, decayed)*]) in the order of `users`; a uid the train set does not know gives (uid, []).  It carries
    .sim_pairs and .item_info like recommend, and .stats = (candidates scored, candidates dropped, largest `now`, largest
    candidate count of a user).  explain = n_ev or (n_ev, n_src) (n_src defaults to 4): the result also carries .explanations
    = [(uid, [(iid, [entry*])*])*], the explanation of exactly the (user, item) pairs of the returned lists in their order,
    entries as explain() gives them; without it the call returns what it always returned.
    Eligibility (the rules act before scoring: the n best ELIGIBLE items are returned): allow_items = the iids that may be
    returned at all (in stock, a category, the new releases), exclude = {uid: iids never returned for that user} (shown yesterday,
    bought elsewhere), min_score = floor on the ranking score (plain, or decayed with decay=True); iids the train set does not know
    are ignored.  With any of them .stats has six entries: the four above over the eligible candidates, the candidates below the
    floor, the candidate pairs the rules removed before scoring.
    Diversified lists: diversify = a weight w >= 0 re-ranks the `pool` best items (default min(64, 4 n); n <= pool <= 64) of every
    user into the n returned ones by greedy maximal marginal relevance (Engine.diversify): the next item is the one with the largest
    score - w * (its largest |sim| in the RecommenderSim matrix to an item picked so far).  The records are the existing ones in the
    new order, the rules act before the pool is cut, and the result carries .ils = the mean pairwise |sim| of every user's list, in
    the order of `users`, and .div_stats = (lists that differ from the pool's prefix, items returned).  diversify = 0 returns the
    lists of the plain call with their .ils; diversify = None takes the plain path untouched.
    Popularity fill: fill = "count", "mean" or dict(how=, damping=, min_count=) completes every list shorter than n -- a user
    without rows, a uid the train set does not know, a narrow allow_items -- with the most popular items of the resident profiles
    (Engine.pop_index: by holders, or by the damped mean rating) that the list does not contain, the user does not hold (unless
    keep_held), exclude does not name and allow_items admits; min_score is a floor on predictions and does not apply.  A filled
    record is (iid, item average, item average): what the model predicts without evidence.  The stages run rules -> pool ->
    diversify -> fill: fills never enter the re-ranking and .ils stays that of the model's part.  The result carries .sources (per
    user a list of 0 = the model's / 1 = a fill) and .fill_stats = (lists short before the fill, of those filled to n, fill
    entries, lists still short); with explain a filled pair is explained as any pair without evidence is.  fill = None takes the
    path as it is without it.  Every call with fill builds the peer index and the ranking anew (as it builds RecommenderSim anew);
    a caller that fills many batches keeps them with Engine.peer_index / pop_index / fill, or in a coarse context."""
    _diverse(n, diversify, pool)
    spec = _fill_spec(fill)
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_topn")
    idt = st.idt
    uids = list(users.collect()) if hasattr(users, "collect") else list(users)
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    query = [uidx.get(uid, -1) for uid in uids]
    res = _topn_records(st, eng2, P, nb, item_avg, query, uids, alpha, n, decay, keep_held, getattr(users, "ctx", None),
                        _eligibility(st.engine.dev, uids, idt.iidx, len(idt.iids), allow_items, exclude, min_score),
                        _diverse(n, diversify, pool, eng2, S), (spec, P) if spec else None)
    _tail_dicts(res, st, S, nb)
    if explain is not None:
        _explain_lists(res, st, eng2, P, nb, item_avg, query, alpha, decay, explain, (st.ratings, st.times) if hasattr(st, "ratings") else None)
    return res


def _diverse(n, diversify, pool, eng2=None, S=None):
    """the diversify= / pool= keywords of a top-N call, checked (before any device work, without eng2) -> None (the plain path) or
    (weight, pool width, the diversity index of S: built once per RecommenderSim result and kept on it, next to what the neighbour
    lists are selected from)"""
    if diversify is None:
        if pool is not None:
            raise ValueError("pool = %r without diversify" % (pool,))
        return None
    weight = float(diversify)
    if not (0.0 <= weight < float("inf")):
        raise ValueError("diversify = %r: a finite weight >= 0" % (diversify,))
    m = min(64, 4 * int(n)) if pool is None else int(pool)
    if not 1 <= int(n) <= m <= 64:
        raise ValueError("n = %d of a pool of %d: 1 <= n <= pool <= 64" % (int(n), m))
    if eng2 is None:
        return weight, m, None
    if getattr(S, "div_index", None) is None:
        S.div_index = eng2.div_index(S)
    return weight, m, S.div_index


def _topn_lists(eng2, P, nb, d_q, item_avg, alpha, n, decay, keep_held, dev, rules, diverse):
    """Engine.topn with a decay table long enough (and Engine.diversify over its pool): (cnt, item, plain, decayed, stats, ils,
    div_stats), the last two None on the plain path"""
    n_w = 66
    while True:
        wtab = _decay_table(alpha, n_w, dev)
        out = eng2.topn(P, nb, d_q, item_avg, wtab, int(diverse[1] if diverse else n), 1 if decay else 0, keep_held, **(rules or {}))
        if out[4][2] <= n_w:
            break
        n_w = out[4][2]
    if not diverse:
        return out + (None, None)
    cnt, item, plain, decayed, _, _, ils, div_stats = eng2.diversify(out, diverse[2], diverse[0], int(n), 1 if decay else 0)
    return cnt, item, plain, decayed, out[4], ils, div_stats


def _fill_spec(fill):
    """the fill= keyword of a top-N call, checked before any device work -> None (the path as it is without it) or (how, damping,
    min_count): "count" / "mean", or a dict with how / damping / min_count"""
    if fill is None:
        return None
    spec = dict(how=fill) if isinstance(fill, str) else dict(fill)
    if set(spec) - {"how", "damping", "min_count"}:
        raise ValueError("fill = %r: a dict of how / damping / min_count" % (fill,))
    how, damping, min_count = spec.get("how", "count"), float(spec.get("damping", 0.0)), int(spec.get("min_count", 1))
    if how not in ("count", "mean"):
        raise ValueError("fill: how = %r, not \"count\" or \"mean\"" % (how,))
    if not (0.0 <= damping < float("inf")):
        raise ValueError("fill: damping = %r: finite and >= 0" % damping)
    if min_count < 1:
        raise ValueError("fill: min_count = %d: at least 1" % min_count)
    return how, damping, min_count


def _fill_lists(eng2, resident, P, d_q, item_avg, lists, spec, keep_held, rules):
    """Engine.fill of `lists` (cnt, item, plain, decayed of the queries d_q over the profiles P) with the popularity ranking of the
    RESIDENT profiles for spec = _fill_spec(...); of the rules the mask and the exclusion lists apply, the floor is one on
    predictions.  Returns (cnt, item, plain, decayed, src, fill_stats).  Like the rest of the session layer, which rebuilds its
    model per call, this builds the peer index and the ranking on every call (3.4 ms together at BASELINE configs[1], beside the
    0.1 ms of the fill itself); only the coarse context (xmap_ctx_recommend_filled) keeps them between calls."""
    pop = eng2.pop_index(eng2.peer_index(resident), *spec)
    kw = {k: v for k, v in (rules or {}).items() if k in ("allow", "exclude")}
    return eng2.fill(lists, pop, P, d_q, item_avg, keep_held=keep_held, **kw)


def _topn_records(st, eng2, P, nb, item_avg, query, uids, alpha, n, decay, keep_held, ctx, rules=None, diverse=None, fill=None):
    """what recommend_topn and recommend_topn_profiles share: the lists of the user indices `query` of P, labelled `uids` -> the
    LocalRDD of (uid, [(iid, plain, decayed)*]) with .stats; rules = _eligibility(...), diverse = _diverse(...), fill = None or
    (_fill_spec(...), the resident profiles): the stages run rules -> pool -> diversify -> fill"""
    import torch
    idt, dev = st.idt, st.engine.dev
    d_q = torch.from_numpy(np.fromiter(query, np.int32, len(uids))).to(dev)
    cnt, item, plain, decayed, stats, ils, div_stats = _topn_lists(eng2, P, nb, d_q, item_avg, alpha, n, decay, keep_held, dev, rules, diverse)
    src = fill_stats = None
    if fill:
        cnt, item, plain, decayed, src, fill_stats = _fill_lists(eng2, fill[1], P, d_q, item_avg, (cnt, item, plain, decayed), fill[0],
                                                                 keep_held, rules)
    cnt, item, plain, decayed = cnt.cpu().numpy(), item.cpu().numpy(), plain.cpu().numpy(), decayed.cpu().numpy()
    iids = idt.iids
    out = [(uid, [(iids[item[q, t]], float(plain[q, t]), float(decayed[q, t])) for t in range(cnt[q])]) for q, uid in enumerate(uids)]
    res = LocalRDD(out, ctx)
    res.stats = stats
    if diverse:
        res.ils, res.div_stats = [float(x) for x in ils.cpu().numpy()], div_stats
    if fill:
        src = src.cpu().numpy()
        res.sources, res.fill_stats = [[int(x) for x in src[q, :cnt[q]]] for q in range(len(uids))], fill_stats
    return res


def _explain_pairs(st, eng2, P, nb, item_avg, pair_user, pair_item, alpha, n_ev, n_src, decay, raw_host):
    """what explain and the explain= option share: the pairs (user index of P, item index) -> per pair (status, score, [entry*])
    with entry = (neighbour iid, sim, the user's AlterEgo rating of it, share, [(source iid, rating, time)*], src_total).
    raw_host = (ratings, times) by raw position: the caller's objects a source cites.  Profiles without raw profiles (a union)
    or n_src = 0: evidence only, every entry ends with ([], None)."""
    import torch
    idt, dev = st.idt, st.engine.dev
    iids, I = idt.iids, len(idt.iids)
    d_u = torch.from_numpy(np.ascontiguousarray(pair_user, np.int32)).to(dev)
    d_i = torch.from_numpy(np.ascontiguousarray(pair_item, np.int32)).to(dev)
    T = int(d_u.numel())
    if T == 0:
        return []
    n_w = 66
    while True:
        wtab = _decay_table(alpha, n_w, dev)
        status, total, cnt, score, row, slot, share, max_now = eng2.explain(P, nb, d_u, d_i, item_avg, wtab, int(n_ev), 1 if decay else 0)
        if max_now <= n_w:
            break
        n_w = max_now
    with_src = int(n_src) > 0 and getattr(P, "sources", None) is not None and raw_host is not None
    # the neighbour behind a slot and the user's AlterEgo rating of it, gathered on the device
    at_i = d_i.clamp(0, max(I - 1, 0)).long()[:, None].expand_as(slot)
    at_s = slot.clamp(min=0).long()
    e_col, e_sim = nb[1][at_i, at_s].cpu().numpy(), nb[2][at_i, at_s].cpu().numpy()
    e_rating = P.user_rating64[row.clamp(min=0)].cpu().numpy()
    if with_src:
        s_total, s_pos = eng2.explain_sources(P, d_u, cnt, row, int(n_src))
        s_item = P.sources[1][s_pos.clamp(min=0)].cpu().numpy() if int(P.sources[1].numel()) else None
        s_total, s_pos = s_total.cpu().numpy(), s_pos.cpu().numpy()
    status, cnt, score, share = status.cpu().numpy(), cnt.cpu().numpy(), score.cpu().numpy(), share.cpu().numpy()
    out = []
    for t in range(T):
        entries = []
        for e in range(int(cnt[t])):
            srcs, n_all = [], None
            if with_src:
                n_all = int(s_total[t, e])
                for k in range(min(max(n_all, 0), int(n_src))):
                    pos = int(s_pos[t, e, k])
                    srcs.append((iids[int(s_item[t, e, k])], raw_host[0][pos], raw_host[1][pos]))
            entries.append((iids[int(e_col[t, e])], float(e_sim[t, e]), float(e_rating[t, e]), float(share[t, e]), srcs, n_all))
        out.append((int(status[t]), float(score[t]), entries))
    return out


def _explain_lists(res, st, eng2, P, nb, item_avg, query, alpha, decay, explain, raw_host):
    """.explanations of a top-N result: exactly the (user, item) pairs of its lists, in their order"""
    n_ev, n_src = (explain if isinstance(explain, (tuple, list)) else (explain, 4))
    lists = res.collect()
    iidx = st.idt.iidx
    pu = [q for q, (_, lst) in zip(query, lists) for _ in lst]
    pi = [iidx[c[0]] for _, lst in lists for c in lst]
    got = iter(_explain_pairs(st, eng2, P, nb, item_avg, pu, pi, alpha, n_ev, n_src, decay, raw_host))
    res.explanations = [(uid, [(c[0], next(got)[2]) for c in lst]) for uid, lst in lists]


def explain(alterEgoRDD, pairs, cap, keep, alpha, n_ev=3, n_src=4, decay=False, neighbors=None):
    """Why an item is (or would be) recommended to a user, on the device: the set-up of recommend, then for every (uid, iid) of
    `pairs` (an RDD or a list) the n_ev (1..16) strongest evidence entries of the unrounded prediction -- plain, or decayed with
    decay=True -- and for each of them the user's own raw ratings behind it (Engine.explain, Engine.explain_sources).  Returns a
    LocalRDD of (uid, iid, score, [entry*]) in the order of `pairs`: entry = (neighbour iid, its similarity to iid, the user's
    AlterEgo rating of the neighbour, share, [(source iid, rating, time)*], src_total) -- share is what the entry adds to
    score - item average, entries by |share| descending; the sources are the first n_src (0..8) of the src_total train ratings of
    the user that stage C made the AlterEgo row from (the row itself for a target item the user rated; the ratings of the
    source items the replacement map sends to the neighbour otherwise), as the caller passed them.  An item without a neighbour
    list gives (uid, iid, None, []); a uid or iid the train set does not know is a user without ratings / an item without a
    list.  On the AlterEgoUnion of union_alterego: evidence without sources ([] and None) -- a union has one replacement map per
    part.  It carries .sim_pairs and .item_info like recommend."""
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "explain")
    if not 0 <= int(n_src) <= 8:
        raise ValueError("n_src = %d: an explanation reports 0 .. 8 sources per entry" % n_src)
    idt = st.idt
    todo = list(pairs.collect()) if hasattr(pairs, "collect") else list(pairs)
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    raw_host = (st.ratings, st.times) if hasattr(st, "ratings") else None
    got = _explain_pairs(st, eng2, P, nb, item_avg, [uidx.get(p[0], -1) for p in todo], [idt.iidx.get(p[1], -1) for p in todo], alpha,
                         n_ev, n_src, decay, raw_host)
    out = []
    for (uid, iid), (status, score, entries) in zip([(p[0], p[1]) for p in todo], got):
        if status == 2:
            raise ZeroDivisionError("explanation of (%r, %r): zero weight sum or non-finite value (the reference raises here)" % (uid, iid))
        out.append((uid, iid, score if status == 0 else None, entries))
    res = LocalRDD(out, getattr(pairs, "ctx", None))
    _tail_dicts(res, st, S, nb)
    return res


def _fold_in(st, G, profiles):
    """raw profiles [(uid, [(iid, rating, time)*])*] (an RDD or a list) -> (their AlterEgo profiles on the device:
    Engine.foldin_profiles with the map of G, {uid: index in the batch}, entries dropped for an iid the id table does not know).
    The uids are labels (never looked up in the train set); the device gets the dense rank of the times over the batch."""
    idt = st.idt
    if getattr(G, "map", None) is None:
        raise ValueError("fold-in needs the replacement map of the generate pass (Engine.alterego keeps it on its result)")
    recs = records_of(profiles)
    index = {}
    for k, rec in enumerate(recs):
        if rec[0] in index:
            raise ValueError("fold-in profile of user %r occurs more than once" % (rec[0],))
        index[rec[0]] = k
    ptr = np.zeros(len(recs) + 1, np.int64)
    item, rating, times, unknown = [], [], [], 0
    for k, (_, prof) in enumerate(recs):
        for iid, r, t in prof:
            i = idt.iidx.get(iid)
            if i is None:
                unknown += 1
                continue
            item.append(i); rating.append(r); times.append(t)
        ptr[k + 1] = len(item)
    item = np.asarray(item, np.int32)
    rating = np.asarray(rating, np.float64)
    check_float32(ptr, item, rating, [rec[0] for rec in recs], idt.iids)
    order = {t: k for k, t in enumerate(sorted(set(times)))}
    rank = np.fromiter((order[t] for t in times), np.int64, len(times))
    F = st.engine.foldin_profiles(ptr, item, rating.astype(np.float32), rank, G.map)
    F.raw_host = (rating, times)            # the caller's ratings and time objects by batch position (explanations cite them)
    return F, index, unknown


def recommend_topn_profiles(alterEgoRDD, profiles, cap, keep, alpha, n, decay=False, keep_held=False, neighbors=None, explain=None,
                            allow_items=None, exclude=None, min_score=None, diversify=None, pool=None, fill=None):
    """recommend_topn for users that are not rows of the train set -- a user who arrived after training, a trained user whose
    profile changed: `profiles` is an RDD or list of (uid, [(iid, rating, time)*]) raw profiles, source and target items mixed.
    Each gets its AlterEgo profile with the replacement map behind alterEgoRDD (fold-in: Engine.foldin_profiles) and then the
    lists of recommend_topn from the model trained on alterEgoRDD's rows, which stays as it is.  The uids are labels only, a
    repeated one raises ValueError; an entry whose iid the train set does not know is dropped and counted in .unknown_items; a
    rating float32 does not hold raises as the train set's does; times are any mutually comparable objects.  Returns the LocalRDD of
    recommend_topn in the order of `profiles`, with .stats, .sim_pairs, .item_info, .unknown_items and .counts = (AlterEgo rows,
    pass-through rows, profiles with a row).  explain as recommend_topn takes it: the sources are then entries of the profile
    passed in (its iid, rating and time objects).  allow_items, exclude = {uid of a profile: iids}, min_score: the eligibility
    rules of recommend_topn.  diversify, pool: the diversified lists of recommend_topn, with .ils and .div_stats.  fill: the
    popularity fill of recommend_topn, with .sources and .fill_stats: what a profile holds is its own (folded-in) rows, what is
    popular is taken over the resident users."""
    _no_fold_in(alterEgoRDD, "recommend_topn_profiles")
    _diverse(n, diversify, pool)
    spec = _fill_spec(fill)
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_topn_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    uids = sorted(index, key=index.get)
    res = _topn_records(st, eng2, F, nb, item_avg, range(len(uids)), uids, alpha, n, decay, keep_held, getattr(profiles, "ctx", None),
                        _eligibility(st.engine.dev, uids, st.idt.iidx, len(st.idt.iids), allow_items, exclude, min_score),
                        _diverse(n, diversify, pool, eng2, S), (spec, P) if spec else None)
    res.unknown_items, res.counts = unknown, F.counts
    _tail_dicts(res, st, S, nb)
    if explain is not None:
        _explain_lists(res, st, eng2, F, nb, item_avg, range(len(uids)), alpha, decay, explain, F.raw_host)
    return res


def _shelf_labels(st, eng2, labels):
    """the labels= keyword of a shelf call: {iid: [label names]} or an RDD / list of (iid, [names]) -> an Engine.set_labels handle
    over the train set's items; an iid the model does not know is ignored"""
    from .labels import label_csr
    idt = st.idt
    pairs = labels.items() if isinstance(labels, dict) else (labels.collect() if hasattr(labels, "collect") else labels)
    per = {}
    for iid, names in pairs:
        i = idt.iidx.get(iid)
        if i is not None:
            per[i] = list(per.get(i, ())) + list(names)
    n_labels, lab_ptr, lab_id, names = label_csr(per, len(idt.iids))
    if n_labels == 0:
        raise ValueError("shelves: no item of the model carries a label")
    return eng2.set_labels(len(idt.iids), n_labels, lab_ptr, lab_id, names)


def _shelf_records(st, eng2, P, nb, item_avg, query, uids, alpha, labels, n_shelf, n, shelf_by, min_fill, allow_labels, decay, keep_held, ctx,
                   rules):
    """what recommend_shelves and recommend_shelves_profiles share: the pages of the user indices `query` of P, labelled `uids` ->
    the LocalRDD of (uid, [(label name, shelf score, size, [(iid, score)*])*]) with .stats"""
    import torch
    from .labels import label_mask
    idt, dev = st.idt, st.engine.dev
    T = _shelf_labels(st, eng2, labels)
    words = None
    if allow_labels is not None:
        chosen = allow_labels.collect() if hasattr(allow_labels, "collect") else allow_labels
        words = label_mask(T.names, [x for x in chosen if x in set(T.names)])
    d_q = torch.from_numpy(np.fromiter(query, np.int32, len(uids))).to(dev)
    rank_by = 1 if decay else 0
    n_w = 66
    while True:
        wtab = _decay_table(alpha, n_w, dev)
        out = eng2.shelves(P, nb, d_q, item_avg, wtab, T, n_shelf, n, shelf_by, min_fill, rank_by, keep_held, lab_allow=words, **(rules or {}))
        if out[8][2] <= n_w:
            break
        n_w = out[8][2]
    nshelf, label, sscore, size, cnt, item, plain, decayed = [x.cpu().numpy() for x in out[:8]]
    score = decayed if decay else plain
    iids = idt.iids
    recs = [(uid, [(T.names[label[q, s]], float(sscore[q, s]), int(size[q, s]),
                    [(iids[item[q, s, t]], float(score[q, s, t])) for t in range(cnt[q, s])]) for s in range(nshelf[q])])
            for q, uid in enumerate(uids)]
    res = LocalRDD(recs, ctx)
    res.stats, res.label_names = out[8], list(T.names)
    return res


def recommend_shelves(alterEgoRDD, users, cap, keep, alpha, labels, n_shelf, n, shelf_by="best", min_fill=1, decay=False, keep_held=False,
                      neighbors=None, allow_labels=None, allow_items=None, exclude=None, min_score=None):
    """A page of shelves per user on the device from an AlterEgoRDD handle: the set-up of recommend_topn, then for every uid of
    `users` a top-n (1..64) per label of the items -- "Top picks in Cookery" -- over the eligible candidates of recommend_topn
    (allow_items, exclude, min_score as it takes them), and the n_shelf (1..64) best shelves of the page (Engine.shelves).  labels =
    {iid: [label names]} or an RDD / list of (iid, [names]): an item may carry several labels, a repeated name counts once, an iid
    the model does not know is ignored, an item without labels is on no shelf.  shelf_by: "best" (a shelf's first score), "mean"
    (the mean of its returned scores) or "label" (label name ascending, a fixed layout); a shelf with fewer than min_fill members is
    not shown; allow_labels = the label names that may form a shelf (None: all; a name no item carries is ignored).  Returns a
    LocalRDD of (uid, [(label name, shelf score, size, [(iid, score)*])*]) in the order of `users` -- size is the whole shelf's
    ("see all 212"), score the plain prediction, or the decayed one with decay=True -- with .stats (the ten of Engine.shelves) and
    .label_names.  A uid the train set does not know gives (uid, [])."""
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_shelves")
    idt = st.idt
    uids = list(users.collect()) if hasattr(users, "collect") else list(users)
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    query = [uidx.get(uid, -1) for uid in uids]
    return _shelf_records(st, eng2, P, nb, item_avg, query, uids, alpha, labels, n_shelf, n, shelf_by, min_fill, allow_labels, decay, keep_held,
                          getattr(users, "ctx", None),
                          _eligibility(st.engine.dev, uids, idt.iidx, len(idt.iids), allow_items, exclude, min_score))


def recommend_shelves_profiles(alterEgoRDD, profiles, cap, keep, alpha, labels, n_shelf, n, shelf_by="best", min_fill=1, decay=False,
                               keep_held=False, neighbors=None, allow_labels=None, allow_items=None, exclude=None, min_score=None):
    """recommend_shelves for users that are not rows of the train set: `profiles` as recommend_topn_profiles takes them (fold-in).
    Returns the LocalRDD of recommend_shelves in the order of `profiles`, with .stats, .label_names, .unknown_items and .counts."""
    _no_fold_in(alterEgoRDD, "recommend_shelves_profiles")
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_shelves_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    uids = sorted(index, key=index.get)
    res = _shelf_records(st, eng2, F, nb, item_avg, range(len(uids)), uids, alpha, labels, n_shelf, n, shelf_by, min_fill, allow_labels, decay,
                         keep_held, getattr(profiles, "ctx", None),
                         _eligibility(st.engine.dev, uids, st.idt.iidx, len(st.idt.iids), allow_items, exclude, min_score))
    res.unknown_items, res.counts = unknown, F.counts
    return res


def _quota_records(st, eng2, P, nb, item_avg, query, uids, alpha, labels, n, pool, mode, at_most, per_label, weights, allow_labels, decay,
                   keep_held, ctx, rules):
    """what recommend_quota and recommend_quota_profiles share: the lists of the user indices `query` of P, labelled `uids` -> the
    LocalRDD of (uid, [(iid, plain, decayed, label name or None)*]) with .stats, .cut_short and .label_names"""
    import torch
    from .labels import label_mask, label_values
    idt, dev = st.idt, st.engine.dev
    T = _shelf_labels(st, eng2, labels)
    words = None
    if allow_labels is not None:
        words = label_mask(T.names, allow_labels.collect() if hasattr(allow_labels, "collect") else allow_labels)
    caps = None if per_label is None else label_values(T.names, per_label, at_most, np.int32)
    w = None if weights is None else label_values(T.names, weights, 0, np.uint32)
    if w is not None and int(w.max(initial=0)) >= 1 << 31:
        raise ValueError("recommend_quota: a weight is 2^31 or more")
    d_q = torch.from_numpy(np.fromiter(query, np.int32, len(uids))).to(dev)
    rank_by = 1 if decay else 0
    n_w = 66
    while True:
        wtab = _decay_table(alpha, n_w, dev)
        out = eng2.quota_topn(P, nb, d_q, item_avg, wtab, T, pool, n, mode, at_most, caps, w, lab_allow=words, rank_by=rank_by,
                              keep_held=keep_held, **(rules or {}))
        if out[6][2] <= n_w:
            break
        n_w = out[6][2]
    cnt, item, plain, decayed, pos, label = [x.cpu().numpy() for x in out[:6]]
    iids = idt.iids
    recs = [(uid, [(iids[item[q, t]], float(plain[q, t]), float(decayed[q, t]), T.names[label[q, t]] if label[q, t] >= 0 else None)
                   for t in range(cnt[q])]) for q, uid in enumerate(uids)]
    res = LocalRDD(recs, ctx)
    res.stats, res.cut_short, res.label_names = out[6], out[6][9], list(T.names)
    return res


def recommend_quota(alterEgoRDD, users, cap, keep, alpha, labels, n, pool, mode="cap", per_label=None, weights=None, allow_labels=None,
                    at_most=1, decay=False, keep_held=False, neighbors=None, allow_items=None, exclude=None, min_score=None):
    """ONE list per user with a guaranteed mix of labels, on the device from an AlterEgoRDD handle: the set-up of recommend_topn,
    then for every uid of `users` the eligible candidates of recommend_topn (allow_items, exclude, min_score as it takes them)
    ranked into a pool of `pool` (n <= pool <= 1 024) that never leaves the device, and a list of n cut from it (Engine.quota_topn).
    labels as recommend_shelves takes them.  mode "cap": at most at_most entries of one label, or per_label = {label name: cap}
    (0 bars a label; a label it does not name: at_most), greedy in rank order.  mode "share": calibrated -- the seats of the list
    go to the labels in proportion (Sainte-Lague) to weights = {label name: weight}, or, without it, to the user's own history:
    the rows of the AlterEgo profile per label, so a user who only rated the other domain gets a list whose mix follows the mapped
    taste.  allow_labels = the label names the quota governs (None: all).  A name that is no label raises.  Returns a LocalRDD of
    (uid, [(iid, plain, decayed, label name or None)*]) in the order of `users` -- the name is the claiming label ("share"; None:
    filled off-profile) or the item's first governed label ("cap") -- with .stats (the ten of Engine.quota_topn), .cut_short (the
    "cap" lists a full pool cut short: widen `pool`) and .label_names.  A uid the train set does not know gives (uid, [])."""
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_quota")
    idt = st.idt
    uids = list(users.collect()) if hasattr(users, "collect") else list(users)
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    query = [uidx.get(uid, -1) for uid in uids]
    return _quota_records(st, eng2, P, nb, item_avg, query, uids, alpha, labels, n, pool, mode, at_most, per_label, weights, allow_labels,
                          decay, keep_held, getattr(users, "ctx", None),
                          _eligibility(st.engine.dev, uids, idt.iidx, len(idt.iids), allow_items, exclude, min_score))


def recommend_quota_profiles(alterEgoRDD, profiles, cap, keep, alpha, labels, n, pool, mode="cap", per_label=None, weights=None,
                             allow_labels=None, at_most=1, decay=False, keep_held=False, neighbors=None, allow_items=None, exclude=None,
                             min_score=None):
    """recommend_quota for users that are not rows of the train set: `profiles` as recommend_topn_profiles takes them (fold-in);
    the history of mode "share" is the folded-in profile.  Returns the LocalRDD of recommend_quota in the order of `profiles`, with
    .stats, .cut_short, .label_names, .unknown_items and .counts."""
    _no_fold_in(alterEgoRDD, "recommend_quota_profiles")
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_quota_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    uids = sorted(index, key=index.get)
    res = _quota_records(st, eng2, F, nb, item_avg, range(len(uids)), uids, alpha, labels, n, pool, mode, at_most, per_label, weights,
                         allow_labels, decay, keep_held, getattr(profiles, "ctx", None),
                         _eligibility(st.engine.dev, uids, st.idt.iidx, len(st.idt.iids), allow_items, exclude, min_score))
    res.unknown_items, res.counts = unknown, F.counts
    return res


def _allot_records(st, eng2, P, nb, item_avg, query, uids, alpha, n, pool, stock, per_item, decay, keep_held, ctx, rules):
    """what recommend_allotted and recommend_allotted_profiles share: the lists of the user indices `query` of P, labelled `uids` ->
    the LocalRDD of (uid, [(iid, plain, decayed)*]) with .positions, .taken, .stats, .changed, .rounds and .cut_short"""
    import torch
    idt, dev = st.idt, st.engine.dev
    caps = None
    if per_item is not None:
        per_item = dict(per_item.collect() if hasattr(per_item, "collect") else per_item)
        unknown = [i for i in per_item if i not in idt.iidx]
        if unknown:
            raise ValueError("recommend_allotted: per_item names %d items the train set does not know, e.g. %r" % (len(unknown), unknown[0]))
        caps = np.full(len(idt.iids), int(stock), np.int64)
        for iid, c in per_item.items():
            caps[idt.iidx[iid]] = int(c)
        if caps.min(initial=0) < 0 or caps.max(initial=0) > 2 ** 31 - 1:
            raise ValueError("recommend_allotted: a capacity is negative or above 2^31 - 1")
        caps = caps.astype(np.int32)
    d_q = torch.from_numpy(np.fromiter(query, np.int32, len(uids))).to(dev)
    n_w = 66
    while True:
        wtab = _decay_table(alpha, n_w, dev)
        out = eng2.allot_topn(P, nb, d_q, item_avg, wtab, pool, n, cap=stock, item_cap=caps, rank_by=1 if decay else 0, keep_held=keep_held,
                              **(rules or {}))
        if out.stats[2] <= n_w:
            break
        n_w = out.stats[2]
    cnt, item, plain, decayed = [x.cpu().numpy() for x in out]
    pos, taken = out.positions.cpu().numpy(), out.taken.cpu().numpy()
    iids = idt.iids
    res = LocalRDD([(uid, [(iids[item[q, t]], float(plain[q, t]), float(decayed[q, t])) for t in range(cnt[q])]) for q, uid in enumerate(uids)],
                   ctx)
    res.positions = [pos[q, :cnt[q]].tolist() for q in range(len(uids))]
    res.taken = {iids[i]: int(taken[i]) for i in np.nonzero(taken)[0]}
    res.stats, res.changed, res.rounds, res.cut_short = out.stats, out.stats[6], out.stats[10], out.stats[11]
    return res


def recommend_allotted(alterEgoRDD, users, cap, keep, alpha, n, pool, stock=1, per_item=None, decay=False, keep_held=False, neighbors=None,
                       allow_items=None, exclude=None, min_score=None):
    """Top-n under stock limits, on the device from an AlterEgoRDD handle: item i goes to at most stock (or per_item[iid]) of the
    `users`, every user gets at most n items.  The set-up of recommend_topn; the pool of every uid is its recommend_topn list of
    `pool` entries (n <= pool <= 64; allow_items, exclude, min_score as recommend_topn takes them), and the lists are the
    recipient-optimal stable assignment over all the users at once (Engine.allot_topn): an item keeps its best offers by score, a
    user moves down its pool past the items that refused it.  per_item = {iid: capacity} (0 bars an item; an item it does not name:
    stock).  `users` are ONE market: serving them in batches with stock - taken handed on gives another, batch-order-dependent
    outcome.  Returns a LocalRDD of (uid, [(iid, plain, decayed)*]) in the order of `users` with .positions (the pool position of
    each entry), .taken ({iid: offers held}), .stats (the twelve of Engine.allot_topn), .changed (lists that differ from the plain
    top-n), .rounds and .cut_short (lists a full pool cut short: widen `pool`).  A uid the train set does not know gives (uid, [])."""
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_allotted")
    idt = st.idt
    uids = list(users.collect()) if hasattr(users, "collect") else list(users)
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    query = [uidx.get(uid, -1) for uid in uids]
    return _allot_records(st, eng2, P, nb, item_avg, query, uids, alpha, n, pool, stock, per_item, decay, keep_held, getattr(users, "ctx", None),
                          _eligibility(st.engine.dev, uids, idt.iidx, len(idt.iids), allow_items, exclude, min_score))


def recommend_allotted_profiles(alterEgoRDD, profiles, cap, keep, alpha, n, pool, stock=1, per_item=None, decay=False, keep_held=False,
                                neighbors=None, allow_items=None, exclude=None, min_score=None):
    """recommend_allotted for users that are not rows of the train set: `profiles` as recommend_topn_profiles takes them (fold-in); the
    batch is one market.  Returns the LocalRDD of recommend_allotted in the order of `profiles`, with .unknown_items and .counts."""
    _no_fold_in(alterEgoRDD, "recommend_allotted_profiles")
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_allotted_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    uids = sorted(index, key=index.get)
    res = _allot_records(st, eng2, F, nb, item_avg, range(len(uids)), uids, alpha, n, pool, stock, per_item, decay, keep_held,
                         getattr(profiles, "ctx", None),
                         _eligibility(st.engine.dev, uids, st.idt.iidx, len(st.idt.iids), allow_items, exclude, min_score))
    res.unknown_items, res.counts = unknown, F.counts
    return res


def _group_records(st, eng2, P, nb, item_avg, uidx, groups, alpha, n, how, veto, decay, keep_held, ctx, allow_items, exclude, min_score):
    """what recommend_group and recommend_group_profiles share: groups = [(gid, [uid*])*] over the users of P (uidx: uid -> user
    index of P; an unknown uid stays a member without rows) -> the LocalRDD of (gid, [(iid, plain, decayed, low_uid)*]) with .stats;
    the decay table grows by the stats[2] loop of _topn_lists"""
    import torch
    from . import hipabi
    idt, dev = st.idt, st.engine.dev
    groups = [(gid, list(members)) for gid, members in (groups.collect() if hasattr(groups, "collect") else groups)]
    for gid, members in groups:
        if len(members) > hipabi.GROUP_MAX_MEMBERS:
            raise ValueError("group %r has %d members; the device aggregation takes up to %d" % (gid, len(members), hipabi.GROUP_MAX_MEMBERS))
    gids = [gid for gid, _ in groups]
    ptr = np.zeros(len(groups) + 1, np.int64)
    np.cumsum([len(m) for _, m in groups], out=ptr[1:])
    users = np.fromiter((uidx.get(uid, -1) for _, m in groups for uid in m), np.int32, int(ptr[-1]))
    d_ptr, d_user = torch.from_numpy(ptr).to(dev), torch.from_numpy(users).to(dev)
    rules = _eligibility(dev, gids, idt.iidx, len(idt.iids), allow_items, exclude, min_score)
    n_w = 66
    while True:
        wtab = _decay_table(alpha, n_w, dev)
        out = eng2.group_topn(P, nb, d_ptr, d_user, item_avg, wtab, int(n), how, veto, 1 if decay else 0, keep_held, **rules)
        if out[5][2] <= n_w:
            break
        n_w = out[5][2]
    cnt, item, plain, decayed, low = [x.cpu().numpy() for x in out[:5]]
    iids = idt.iids
    res = LocalRDD([(gid, [(iids[item[g, t]], float(plain[g, t]), float(decayed[g, t]), members[low[g, t]]) for t in range(cnt[g])])
                    for g, (gid, members) in enumerate(groups)], ctx)
    res.stats = out[5]
    return res


def recommend_group(alterEgoRDD, groups, cap, keep, alpha, n, how="mean", veto=None, decay=False, keep_held=False, neighbors=None,
                    allow_items=None, exclude=None, min_score=None):
    """ONE list for several users -- a household, a party, a shared account -- on the device (Engine.group_topn): the set-up of
    recommend_topn, then for every (gid, [uid*]) of `groups` the n (1..64) best items by the aggregate of the members' unrounded
    predictions: how = "mean", "min" (least misery) or "max" (most pleasure).  Candidates are the items at least one member's rows
    give evidence for; a member without evidence for one predicts the item average (as the prediction itself does); items ANY member
    holds are left out unless keep_held.  veto: an item leaves if some member's score is below it ("average without misery").  A
    member listed twice counts twice; a uid the train set does not know stays a member without rows; at most 64 members.  Returns a
    LocalRDD of (gid, [(iid, plain, decayed, low_uid)*]) in the order of `groups` -- low_uid = the member who likes the item least,
    the first such in list order -- with .stats (the eight of Engine.group_topn), .sim_pairs and .item_info.  allow_items, exclude =
    {gid: iids}, min_score (on the aggregate): the eligibility rules of recommend_topn."""
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_group")
    idt = st.idt
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    res = _group_records(st, eng2, P, nb, item_avg, uidx, groups, alpha, n, how, veto, decay, keep_held, getattr(groups, "ctx", None),
                         allow_items, exclude, min_score)
    _tail_dicts(res, st, S, nb)
    return res


def recommend_group_profiles(alterEgoRDD, profiles, groups, cap, keep, alpha, n, how="mean", veto=None, decay=False, keep_held=False,
                             neighbors=None, allow_items=None, exclude=None, min_score=None):
    """recommend_group for members that are not rows of the train set -- a party of guests nobody trained on: `profiles` as
    recommend_topn_profiles takes them (folded in with the replacement map behind alterEgoRDD), and the uids of `groups` name
    profiles of that batch; a uid without a profile stays a member without rows.  Returns the LocalRDD of recommend_group, with
    .unknown_items and .counts as recommend_topn_profiles."""
    _no_fold_in(alterEgoRDD, "recommend_group_profiles")
    st, eng2, _, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_group_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    res = _group_records(st, eng2, F, nb, item_avg, index, groups, alpha, n, how, veto, decay, keep_held, getattr(groups, "ctx", None),
                         allow_items, exclude, min_score)
    res.unknown_items, res.counts = unknown, F.counts
    _tail_dicts(res, st, S, nb)
    return res


def recommend_audience(alterEgoRDD, items, cap, keep, alpha, n, decay=False, keep_holders=False, neighbors=None, allow_users=None,
                       exclude=None, min_score=None):
    """The audience of an item on the device from an AlterEgoRDD handle -- recommend_topn the other way round: the set-up of
    recommend_topn, then for every iid of `items` the n (1..1024) best users among those whose own rows give evidence for it,
    ranked by the unrounded prediction -- without temporal decay, or with (decay=True, alpha) -- score descending, user INDEX
    (the order of the train set's users) ascending on equal scores; users who already hold the item are left out unless
    keep_holders (Engine.audience).  Returns a LocalRDD of (iid, [(uid, plain, decayed)*]) in the order of `items`; an iid the
    train set does not know gives (iid, []).  It carries .sim_pairs, .item_info and .stats like recommend_topn (.stats[3]: the
    largest candidate count of an item).  The scores of a (uid, iid) pair are the bits recommend_topn gives it.
    Eligibility, as recommend_topn takes it with users for items: allow_users = the uids that may be returned at all (a segment,
    those who did not opt out), exclude = {iid: uids never returned for that item} (already contacted), min_score = floor; uids
    the train set does not know are ignored; .stats then has six entries.  Only eligible pairs are scored: a campaign over a 1 %
    segment scores 1 % of the pairs."""
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_audience")
    iids = list(items.collect()) if hasattr(items, "collect") else list(items)
    res = _audience_records(st, eng2, P, nb, item_avg, iids, st.idt.uids, alpha, n, decay, keep_holders, getattr(items, "ctx", None),
                            rules=_eligibility(st.engine.dev, iids, _user_index(st.idt), len(st.idt.uids), allow_users, exclude, min_score))
    _tail_dicts(res, st, S, nb)
    return res


def _user_index(idt):
    return getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}


def _audience_records(st, eng2, P, nb, item_avg, iids, uids, alpha, n, decay, keep_holders, ctx, iidx=None, batch=None, rules=None):
    """what recommend_audience, recommend_audience_profiles and recommend_audience_items share: the audiences of the items
    `iids` among the users of P, labelled `uids` by index -> the LocalRDD of (iid, [(uid, plain, decayed)*]) with .stats.
    iidx / batch: the item indices and the rater CSR of an item fold-in, whose extended tables nb and item_avg then are;
    rules = _eligibility(...) over the users of P"""
    import torch
    idt, dev = st.idt, st.engine.dev
    iidx = idt.iidx if iidx is None else iidx
    d_q = torch.from_numpy(np.fromiter((iidx.get(iid, -1) for iid in iids), np.int32, len(iids))).to(dev)
    n_w = 66
    while True:
        wtab = _decay_table(alpha, n_w, dev)
        cnt, user, plain, decayed, stats = eng2.audience(P, nb, d_q, item_avg, wtab, int(n), 1 if decay else 0, keep_holders, batch=batch,
                                                                **(rules or {}))
        if stats[2] <= n_w:
            break
        n_w = stats[2]
    cnt, user, plain, decayed = cnt.cpu().numpy(), user.cpu().numpy(), plain.cpu().numpy(), decayed.cpu().numpy()
    out = [(iid, [(uids[user[q, t]], float(plain[q, t]), float(decayed[q, t])) for t in range(cnt[q])]) for q, iid in enumerate(iids)]
    res = LocalRDD(out, ctx)
    res.stats = stats
    return res


def recommend_audience_profiles(alterEgoRDD, profiles, items, cap, keep, alpha, n, decay=False, keep_holders=False, neighbors=None,
                                allow_users=None, exclude=None, min_score=None):
    """recommend_audience among users that are not rows of the train set ("which of the users who arrived today"): `profiles`
    as recommend_topn_profiles takes them and folds them in; the audiences of `items` are chosen among these profiles only,
    from the model trained on alterEgoRDD's rows, which stays as it is.  Equal scores are ordered by the position in `profiles`.
    Returns the LocalRDD of recommend_audience with .unknown_items and .counts as recommend_topn_profiles.  allow_users (uids of
    `profiles`), exclude = {iid: uids}, min_score: the eligibility rules of recommend_audience."""
    _no_fold_in(alterEgoRDD, "recommend_audience_profiles")
    st, eng2, _, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_audience_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    iids = list(items.collect()) if hasattr(items, "collect") else list(items)
    res = _audience_records(st, eng2, F, nb, item_avg, iids, sorted(index, key=index.get), alpha, n, decay, keep_holders,
                            getattr(items, "ctx", None),
                            rules=_eligibility(st.engine.dev, iids, index, len(index), allow_users, exclude, min_score))
    res.unknown_items, res.counts = unknown, F.counts
    _tail_dicts(res, st, S, nb)
    return res


def _peer_setup(alterEgoRDD, centred, who):
    """what similar_users and similar_users_profiles share: the profiles of the AlterEgo rows and their peer index -> (state,
    engine over the profiles, P, index).  centred: x = rating - the item average of the profiles (Engine.peer_centre over the
    uncentred index: the exact sum rounded once / entries, RecommenderSim's averages without its pair pass).  The set-up -- the
    profiles, one or two index builds (a stable sort of the profile rows each) and the averages -- is kept on the handle per
    centring, so only the first call on a handle pays it; a call then costs Engine.peers alone."""
    from . import device
    if not isinstance(alterEgoRDD, (AlterEgoUnion, AlterEgoRDD)):
        raise TypeError("%s() takes the AlterEgoRDD handle of generator_pipeline (rows resident on the device) or the "
                        "AlterEgoUnion of union_alterego" % who)
    st = alterEgoRDD.state
    kept = alterEgoRDD.__dict__.setdefault("_peer_setup", {})      # {"P": (engine, profiles), False / True: index}; goes with the handle
    if "P" not in kept:
        if isinstance(alterEgoRDD, AlterEgoUnion):
            P = alterEgoRDD.profiles()
        else:
            G = alterEgoRDD.G
            P = st.engine.alterego_profiles(G, time_key=time_rank(st)[G.time] if G.n_rows else G.time)
        eng2 = device.Engine(P)
        eng2.timers = st.engine.timers
        kept["P"] = (eng2, P)
    eng2, P = kept["P"]
    if False not in kept:
        kept[False] = eng2.peer_index(P)
    if centred and True not in kept:
        kept[True] = eng2.peer_index(P, eng2.peer_centre(kept[False]))
    return st, eng2, P, kept[bool(centred)]


def _peer_records(st, eng2, X, Q, query, labels, uids, n, cap, min_common, same, keep_self, ctx, rules):
    """the peers of the users `query` (indices into the profiles Q, labelled `labels`) among the resident users `uids` -> the
    LocalRDD of (label, [(uid, sim, common)*]) with .stats (the six of Engine.peers)"""
    import torch
    d_q = torch.from_numpy(np.fromiter(query, np.int32, len(labels))).to(st.engine.dev)
    rules = dict(rules)
    if "min_score" in rules:
        rules["min_sim"] = rules.pop("min_score")
    cnt, user, sim, common, stats = eng2.peers(X, Q, d_q, int(n), int(cap), int(min_common), same, keep_self, **rules)
    cnt, user, sim, common = cnt.cpu().numpy(), user.cpu().numpy(), sim.cpu().numpy(), common.cpu().numpy()
    res = LocalRDD([(lab, [(uids[user[q, t]], float(sim[q, t]), int(common[q, t])) for t in range(cnt[q])])
                    for q, lab in enumerate(labels)], ctx)
    res.stats = stats
    return res


def similar_users(alterEgoRDD, users, n, cap=1, centred=True, min_common=1, keep_self=False, allow_users=None, exclude=None,
                  min_sim=None):
    """"Who is this user like?" on the device (Engine.peer_index / Engine.peers): for every uid of `users` the n (1..1024) users of
    the train set whose AlterEgo profiles are most alike -- sim = the cosine of the two profiles over the items both hold (centred:
    ratings minus the item average) times min(common, cap) / cap, the significance weighting of RecommenderSim; sim descending, user
    INDEX ascending on equal sim; the user itself is left out unless keep_self.  min_common: peers with fewer common records are
    dropped.  Returns a LocalRDD of (uid, [(uid2, sim, common)*]) in the order of `users`; a uid the train set does not know gives
    (uid, []).  It carries .stats = (candidates, dropped by min_common, dropped as non-finite, dropped below min_sim, largest
    candidate count of a user, records expanded).  Cost: the first call on a handle builds the peer index (and with centred the
    item averages) and keeps it on the handle; later calls run the expansion, sort and selection only.  Eligibility as
    recommend_audience takes it: allow_users = the uids that may be
    returned (a segment: only their records are expanded), exclude = {uid: uids never returned for it}, min_sim = floor."""
    st, eng2, P, X = _peer_setup(alterEgoRDD, centred, "similar_users")
    uids = list(users.collect()) if hasattr(users, "collect") else list(users)
    uidx = _user_index(st.idt)
    return _peer_records(st, eng2, X, P, (uidx.get(u, -1) for u in uids), uids, st.idt.uids, n, cap, min_common, True, keep_self,
                         getattr(users, "ctx", None), _eligibility(st.engine.dev, uids, uidx, len(st.idt.uids), allow_users, exclude, min_sim))


def similar_users_profiles(alterEgoRDD, profiles, n, cap=1, centred=True, min_common=1, allow_users=None, exclude=None, min_sim=None):
    """similar_users for users that are not rows of the train set: `profiles` as recommend_topn_profiles takes them and folds them
    in; their peers are chosen among the users of the train set (no self rule: a profile is nobody's row).  Returns the LocalRDD of
    similar_users in the order of `profiles`, with .unknown_items and .counts as recommend_topn_profiles.  exclude = {uid of a
    profile: uids of the train set}."""
    _no_fold_in(alterEgoRDD, "similar_users_profiles")
    st, eng2, _, X = _peer_setup(alterEgoRDD, centred, "similar_users_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    labels = sorted(index, key=index.get)
    res = _peer_records(st, eng2, X, F, range(len(labels)), labels, st.idt.uids, n, cap, min_common, False, False,
                        getattr(profiles, "ctx", None),
                        _eligibility(st.engine.dev, labels, _user_index(st.idt), len(st.idt.uids), allow_users, exclude, min_sim))
    res.unknown_items, res.counts = unknown, F.counts
    return res


class UserSimRDD(LocalRDD):
    """alterEgo_sim of a user method (cosine_user): ((uid1, uid2), [sim, local sensitivity]) for both directions of every pair
    of users with a common item, the user itself left out.  Nothing is materialised until the rows are asked for: the handle
    keeps the profiles and their uncentred peer index on the device, and Engine.peers_ls (xmap_peer_rows_ls) gives the lists --
    every user a query, same, uncentred, cap = num_atleast, min_common 1.  Peers orders by sim, the reference's selection by
    |sim|; they agree when no rating is negative, which is checked once at upload (by_abs: the host sorts the full rows)."""

    max_keep = 1024             # the widest list the device selection returns
    GROUP = 2048                # queries per Engine.peers_ls call: the outputs stay at 48 MB

    def __init__(self, engine, P, X, uids, cap, by_abs, ctx=None):
        LocalRDD.__init__(self, None, ctx)
        self.engine, self.P, self.X, self.uids, self.cap, self.by_abs = engine, P, X, uids, int(cap), bool(by_abs)

    def _lists(self, n_top):
        """-> ([(user index, neighbour indices, sims, sensitivities)*] for every user with a neighbour, in rank order; the
        largest candidate count of a user)"""
        import torch
        U, out, widest = len(self.uids), [], 0
        for a in range(0, U, self.GROUP):
            d_q = torch.arange(a, min(a + self.GROUP, U), dtype=torch.int32, device=self.engine.dev)
            cnt, user, sim, _, ls, stats = self.engine.peers_ls(self.X, self.P, d_q, n_top, self.cap, 1, True, False)
            widest = max(widest, stats[4])
            cnt, user, sim, ls = cnt.cpu().numpy(), user.cpu().numpy(), sim.cpu().numpy(), ls.cpu().numpy()
            out.extend((a + k, user[k, :cnt[k]], sim[k, :cnt[k]], ls[k, :cnt[k]]) for k in range(len(cnt)) if cnt[k])
        return out, widest

    def select_neighbors(self, keep):
        """nonprivate_neighbor_selection on the device: [(uid, [(uid2, [sim, ls])*])*] for every user with a neighbour, in uid
        order; per user the `keep` largest |sim|, user index ascending on equal sim"""
        keep = int(keep)
        if not 1 <= keep <= self.max_keep:
            raise ValueError("select_neighbors(%d): the device selection takes 1 .. %d" % (keep, self.max_keep))
        uids = self.uids
        if self.by_abs:
            pos = {u: k for k, u in enumerate(uids)}
            by = {}
            for (u1, u2), info in self._data:
                by.setdefault(u1, []).append((u2, info))
            res = [(u, sorted(lst, key=lambda e: (-abs(e[1][0]), pos[e[0]]))[:keep]) for u, lst in by.items()]
        else:
            res = [(uids[q], [(uids[v], [float(s), float(l)]) for v, s, l in zip(user, sim, ls)])
                   for q, user, sim, ls in self._lists(keep)[0]]
        res.sort(key=lambda e: e[0])
        return res

    def _rows(self):
        lists, widest = self._lists(self.max_keep)
        if widest > self.max_keep:
            raise ValueError("a user has %d neighbours, the rows are materialised through lists of %d: take the neighbours with "
                             "select_neighbors(keep) instead of the full rows" % (widest, self.max_keep))
        uids = self.uids
        rows = []
        for q, user, sim, ls in lists:
            o = np.argsort(user, kind="stable")         # canonical order: (uid1, uid2) by index
            rows.extend(((uids[q], uids[v]), [float(s), float(l)]) for v, s, l in zip(user[o], sim[o], ls[o]))
        return rows


def user_sim_from_profiles(user_profiles, cap, ctx=None):
    """user_profiles: [(uid, [(iid, rating, time)*])*] (the user-based AlterEgo profile) -> the UserSimRDD of the cosine_user
    similarity.  uids and iids go in lexicographic order, so "index ascending on equal sim" is "uid ascending".  A profile that
    holds an item twice is refused: the peer index gives such a user a bilinear norm, the reference sqrt(sum r^2)."""
    import torch
    from types import SimpleNamespace
    from . import device
    recs = sorted(records_of(user_profiles), key=lambda r: r[0])
    uids = [u for u, _ in recs]
    if len(set(uids)) != len(uids):
        raise ValueError("user_sim_from_profiles: a uid appears in two profiles")
    iids = sorted({t[0] for _, prof in recs for t in prof})
    iidx = {s: k for k, s in enumerate(iids)}
    ptr = np.zeros(len(recs) + 1, np.int64)
    item, rating = [], []
    for k, (uid, prof) in enumerate(recs):
        held = [iidx[t[0]] for t in prof]
        if len(set(held)) != len(held):
            raise ValueError("user_sim_from_profiles: the profile of %r holds an item twice; cosine_user on the device takes "
                             "profiles without repeated items (the reference pipeline removes them: avoid_duplicate_ratings)" % (uid,))
        ptr[k + 1] = ptr[k] + len(prof)
        item.extend(held)
        rating.extend(float(t[1]) for t in prof)
    dev = torch.device("cuda:%d" % torch.cuda.current_device())
    rating = np.asarray(rating, np.float64)
    to = lambda a: torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(dev)
    P = SimpleNamespace(device=dev, n_users=len(uids), n_items=len(iids), user_ptr=to(ptr), user_item=to(np.asarray(item, np.int32)),
                        user_rating64=to(rating))
    eng = device.Engine(P)
    return UserSimRDD(eng, P, eng.peer_index(P), uids, cap, bool((rating < 0).any()), ctx)


def user_sim(alterEgoRDD, cap):
    """user_sim_from_profiles over the handle's resident profiles (_peer_setup: no host round trip) -> UserSimRDD; the users
    are indexed as the train set has them"""
    st, eng2, P, X = _peer_setup(alterEgoRDD, False, "user_sim")
    n = int(P.user_ptr[-1].item())
    return UserSimRDD(eng2, P, X, st.idt.uids, cap, bool((P.user_rating64[:n] < 0).any().item()) if n else False,
                      getattr(alterEgoRDD, "ctx", None))


def _uknn_setup(alterEgoRDD, centred, who):
    """_peer_setup + the resident users' means (Engine.user_means), kept on the handle like the index"""
    st, eng2, P, X = _peer_setup(alterEgoRDD, centred, who)
    kept = alterEgoRDD.__dict__["_peer_setup"]
    if "means" not in kept:
        kept["means"] = eng2.user_means(P)[0]
    return st, eng2, P, X, kept["means"]


def _uknn_lists(st, eng2, X, Q, means, query, n_nb, cap, min_common, same):
    """the peer lists of the users `query` (indices into the profiles Q whose means are `means`) and their own means (0.0 for an
    index outside Q: such a query has no list either) -> (query tensor, lists, query_avg)"""
    import torch
    d_q = torch.from_numpy(np.asarray(list(query), np.int32).reshape(-1)).to(st.engine.dev)
    lists = eng2.peers(X, Q, d_q, int(n_nb), int(cap), int(min_common), same, False)
    if int(means.numel()):
        inside = (d_q >= 0) & (d_q < int(means.numel()))
        q_avg = torch.where(inside, means[d_q.clamp(0, int(means.numel()) - 1).long()], torch.zeros((), dtype=means.dtype, device=means.device))
    else:
        q_avg = torch.zeros(int(d_q.numel()), dtype=torch.float64, device=st.engine.dev)
    return d_q, lists, q_avg


def predict_user_knn(alterEgoRDD, testRDD, n_nb, cap=1, centred=True, min_common=1, own_mean=False):
    """User-based kNN prediction on the device, the reference's user_based_prediction over the AlterEgo profiles: for every uid of
    testRDD its n_nb (1..1024) nearest users (similar_users: cap, centred, min_common; the user itself left out), then for every
    held-out (iid, real) pred = the user's mean + sum(sim * (rating - the user's mean)) / sum(|sim|) over the neighbours' ratings
    of the item, in list order -- the QUERY user's mean is subtracted, as the reference does; own_mean=True subtracts each
    neighbour's own mean (Resnick's formula) -- bounded by bound_rating; without evidence the user's mean; no temporal decay.
    Returns (records, mae): records = a LocalRDD of (uid, [(iid, real, predicted) | ()]) in testRDD order, () for a user without
    neighbours (or unknown to the train set) and for an iid the train set does not know; mae = the single string calculate_mae
    gives for a "user" method (None without a predicted pair or when a real rating is not a number).  records.mae = (count, sum
    |real - predicted|) from the device (Engine.mae)."""
    import torch
    st, eng2, P, X, means = _uknn_setup(alterEgoRDD, centred, "predict_user_knn")
    idt, dev = st.idt, st.engine.dev
    uidx = _user_index(idt)
    recs = records_of(testRDD)
    order = {}
    for uid, _ in recs:
        order.setdefault(uid, len(order))
    _, lists, q_avg = _uknn_lists(st, eng2, X, P, means, (uidx.get(u, -1) for u in sorted(order, key=order.get)), n_nb, cap, min_common, True)
    tq = np.fromiter((order[uid] for uid, pairs in recs for _ in pairs), np.int32)
    ti = np.fromiter((idt.iidx.get(pair[0], -1) for _, pairs in recs for pair in pairs), np.int32)
    try:
        real = np.fromiter((float(pair[1]) for _, pairs in recs for pair in pairs), np.float64)
    except (TypeError, ValueError):
        real = None
    score, bound, n, status = eng2.uknn_predict(P, lists, q_avg, torch.from_numpy(tq).to(dev), torch.from_numpy(ti).to(dev), means, own_mean)
    mae = None
    if real is not None and len(tq):
        mae = tuple(eng2.mae(status, torch.from_numpy(real).to(dev), bound, bound).tolist()[:2])
    bound, status = bound.cpu().numpy(), status.cpu().numpy()
    out, q = [], 0
    for uid, pairs in recs:
        line = []
        for pair in pairs:
            if status[q] == 0:
                line.append((pair[0], pair[1], float(bound[q])))
            elif status[q] == 2:
                raise ZeroDivisionError("prediction of (%r, %r): zero weight sum or non-finite value (the reference raises here)"
                                        % (uid, pair[0]))
            else:
                line.append(())
            q += 1
        out.append((uid, line))
    res = LocalRDD(out, getattr(testRDD, "ctx", None))
    res.mae = mae
    return res, (str(np.float64(mae[1]) / np.float64(mae[0])) if mae and mae[0] > 0 else None)


def _uknn_records(st, eng2, P, Q, d_q, lists, q_avg, means, labels, n, own_mean, keep_held, min_support, ctx, rules):
    cnt, item, score, support, stats = eng2.uknn_topn(P, Q, d_q, lists, q_avg, int(n), means, own_mean, keep_held, int(min_support), **rules)
    cnt, item, score, support = cnt.cpu().numpy(), item.cpu().numpy(), score.cpu().numpy(), support.cpu().numpy()
    iids = st.idt.iids
    res = LocalRDD([(lab, [(iids[item[q, t]], float(score[q, t]), int(support[q, t])) for t in range(cnt[q])])
                    for q, lab in enumerate(labels)], ctx)
    res.stats = stats
    return res


def recommend_user_knn(alterEgoRDD, users, n_nb, n, cap=1, centred=True, min_common=1, own_mean=False, keep_held=False, min_support=1,
                       allow_items=None, exclude=None, min_score=None):
    """User-based top-N on the device ("people like you rated this highly"): for every uid of `users` its n_nb nearest users as
    predict_user_knn takes them, then the n (1..1024) items those neighbours hold with the largest unrounded prediction of
    predict_user_knn; score descending, item INDEX ascending on equal scores.  Items the user holds are left out unless keep_held;
    an item fewer than min_support neighbour ratings speak for is dropped.  Returns a LocalRDD of (uid, [(iid, score, support)*])
    in the order of `users`; a uid the train set does not know gives (uid, []).  .stats = (candidates, dropped by min_support,
    dropped as non-finite, dropped below min_score, largest candidate count of a user, records expanded).  Eligibility as
    recommend_topn takes it: allow_items, exclude = {uid: iids}, min_score."""
    st, eng2, P, X, means = _uknn_setup(alterEgoRDD, centred, "recommend_user_knn")
    uids = list(users.collect()) if hasattr(users, "collect") else list(users)
    uidx = _user_index(st.idt)
    d_q, lists, q_avg = _uknn_lists(st, eng2, X, P, means, (uidx.get(u, -1) for u in uids), n_nb, cap, min_common, True)
    return _uknn_records(st, eng2, P, P, d_q, lists, q_avg, means, uids, n, own_mean, keep_held, min_support, getattr(users, "ctx", None),
                         _eligibility(st.engine.dev, uids, st.idt.iidx, len(st.idt.iids), allow_items, exclude, min_score))


def recommend_user_knn_profiles(alterEgoRDD, profiles, n_nb, n, cap=1, centred=True, min_common=1, own_mean=False, keep_held=False,
                                min_support=1, allow_items=None, exclude=None, min_score=None):
    """recommend_user_knn for users that are not rows of the train set: `profiles` as recommend_topn_profiles takes them and
    folds them in; their neighbours are users of the train set, their mean and their held items come from the folded-in profile.
    Returns the LocalRDD of recommend_user_knn in the order of `profiles`, with .unknown_items and .counts as
    recommend_topn_profiles.  exclude = {uid of a profile: iids}."""
    _no_fold_in(alterEgoRDD, "recommend_user_knn_profiles")
    st, eng2, P, X, means = _uknn_setup(alterEgoRDD, centred, "recommend_user_knn_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    labels = sorted(index, key=index.get)
    d_q, lists, q_avg = _uknn_lists(st, eng2, X, F, eng2.user_means(F)[0], range(len(labels)), n_nb, cap, min_common, False)
    res = _uknn_records(st, eng2, P, F, d_q, lists, q_avg, means, labels, n, own_mean, keep_held, min_support, getattr(profiles, "ctx", None),
                        _eligibility(st.engine.dev, labels, st.idt.iidx, len(st.idt.iids), allow_items, exclude, min_score))
    res.unknown_items, res.counts = unknown, F.counts
    return res


HYBRID_KEYS = ("n_nb", "peer_cap", "centred", "min_common", "own_mean", "min_support", "how", "weights", "rrf_c", "pool_items", "pool_users",
               "min_lists")


def _hybrid_spec(n, n_nb, peer_cap=1, centred=True, min_common=1, own_mean=False, min_support=1, how="rrf", weights=(1.0, 1.0), rrf_c=60.0,
                 pool_items=64, pool_users=64, min_lists=1):
    """the hybrid arguments of recommend_hybrid / evaluate_topn(hybrid=...), checked before any device work -> a dict of them"""
    from . import device
    device.Engine._fuse_args(2, n, how, weights, rrf_c, min_lists)
    if not 1 <= int(pool_items) <= 64:
        raise ValueError("pool_items = %r: the item-based list holds 1 .. 64" % (pool_items,))
    if not 1 <= int(pool_users) <= 1024:
        raise ValueError("pool_users = %r: the user-based list holds 1 .. 1024" % (pool_users,))
    if not 1 <= int(n_nb) <= 1024:
        raise ValueError("n_nb = %r: 1 .. 1024 neighbours" % (n_nb,))
    if int(peer_cap) < 1 or int(min_common) < 1 or int(min_support) < 1:
        raise ValueError("peer_cap = %r, min_common = %r, min_support = %r: >= 1" % (peer_cap, min_common, min_support))
    return dict(n_nb=int(n_nb), peer_cap=int(peer_cap), centred=bool(centred), min_common=int(min_common), own_mean=bool(own_mean),
                min_support=int(min_support), how=how, weights=tuple(float(w) for w in weights), rrf_c=float(rrf_c),
                pool_items=int(pool_items), pool_users=int(pool_users), min_lists=int(min_lists))


def _hybrid_lists(alterEgoRDD, who, st, eng2, Q, nb, item_avg, query, fold, alpha, n, decay, keep_held, rules, h):
    """The item-based and the user-based list of the same queries, fused on the device: Engine.topn (pool_items) over the profiles Q
    (the resident ones, or a folded-in batch with fold=True), Engine.uknn_topn (pool_users) over the peers of the same users,
    Engine.fuse of (count, item, ranking score) of both.  query: a device tensor of indices into Q.  Returns (cnt, item, score,
    mask, (top-N stats, user-kNN stats, fuse stats)); nothing is copied to the host."""
    dev = st.engine.dev
    it = _topn_lists(eng2, Q, nb, query, item_avg, alpha, h["pool_items"], decay, keep_held, dev, rules, None)
    _, eng_u, Pu, X, means = _uknn_setup(alterEgoRDD, h["centred"], who)
    q_host = query.cpu().tolist()
    if fold:
        d_q, peers, q_avg = _uknn_lists(st, eng_u, X, Q, eng_u.user_means(Q)[0], q_host, h["n_nb"], h["peer_cap"], h["min_common"], False)
    else:
        d_q, peers, q_avg = _uknn_lists(st, eng_u, X, Pu, means, q_host, h["n_nb"], h["peer_cap"], h["min_common"], True)
    us = eng_u.uknn_topn(Pu, Q if fold else Pu, d_q, peers, q_avg, h["pool_users"], means, h["own_mean"], keep_held, h["min_support"],
                         **(rules or {}))
    cnt, item, score, mask, stats = eng2.fuse([(it[0], it[1], it[3] if decay else it[2]), us[:3]], int(n), h["how"], h["weights"], h["rrf_c"],
                                              h["min_lists"], n_ids=len(st.idt.iids))
    return cnt, item, score, mask, (tuple(it[4]), tuple(us[4]), stats)


_WHICH = ((), ("item",), ("user",), ("item", "user"))


def _hybrid_records(st, fused, labels, ctx):
    cnt, item, score, mask = [x.cpu().numpy() for x in fused[:4]]
    iids = st.idt.iids
    res = LocalRDD([(lab, [(iids[item[q, t]], float(score[q, t]), _WHICH[mask[q, t] & 3]) for t in range(cnt[q])])
                    for q, lab in enumerate(labels)], ctx)
    res.stats = fused[4]
    return res


def recommend_hybrid(alterEgoRDD, users, cap, keep, alpha, n, n_nb, decay=False, keep_held=False, neighbors=None, allow_items=None,
                     exclude=None, min_score=None, peer_cap=1, centred=True, min_common=1, own_mean=False, min_support=1, how="rrf",
                     weights=(1.0, 1.0), rrf_c=60.0, pool_items=64, pool_users=64, min_lists=1):
    """The usual hybrid on the device ("items my own ratings point to AND people like me rated highly"): for every uid of `users`
    the pool_items (1..64) best items of recommend_topn (cap, keep, alpha, decay, keep_held, neighbors) and the pool_users (1..1024)
    best items of recommend_user_knn (n_nb, peer_cap as its cap, centred, min_common, own_mean, min_support), fused into one list
    of n (1..1024) by Engine.fuse: how = "rrf" (by rank: weight / (rrf_c + rank) summed), "sum" or "mean" (by score: the item-based
    score is the plain prediction, or the decayed one with decay=True; the user-based score is its prediction), weights = (item
    weight, user weight), min_lists = 2 keeps only the items both halves name.  allow_items, exclude, min_score act on both
    halves.  Neither list leaves the device.  Returns a LocalRDD of (uid, [(iid, score, which)*]) in the order of `users`, which
    = the halves that named the item, a subset of ("item", "user"); .stats = (the stats of recommend_topn, of recommend_user_knn,
    of Engine.fuse)."""
    import torch
    h = _hybrid_spec(n, n_nb, peer_cap, centred, min_common, own_mean, min_support, how, weights, rrf_c, pool_items, pool_users, min_lists)
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_hybrid")
    uids = list(users.collect()) if hasattr(users, "collect") else list(users)
    uidx = _user_index(st.idt)
    d_q = torch.from_numpy(np.fromiter((uidx.get(u, -1) for u in uids), np.int32, len(uids))).to(st.engine.dev)
    rules = _eligibility(st.engine.dev, uids, st.idt.iidx, len(st.idt.iids), allow_items, exclude, min_score)
    fused = _hybrid_lists(alterEgoRDD, "recommend_hybrid", st, eng2, P, nb, item_avg, d_q, False, alpha, n, decay, keep_held, rules, h)
    return _hybrid_records(st, fused, uids, getattr(users, "ctx", None))


def recommend_hybrid_profiles(alterEgoRDD, profiles, cap, keep, alpha, n, n_nb, decay=False, keep_held=False, neighbors=None,
                              allow_items=None, exclude=None, min_score=None, peer_cap=1, centred=True, min_common=1, own_mean=False,
                              min_support=1, how="rrf", weights=(1.0, 1.0), rrf_c=60.0, pool_items=64, pool_users=64, min_lists=1):
    """recommend_hybrid for users that are not rows of the train set: `profiles` as recommend_topn_profiles takes them and folds them
    in; both halves run over the folded-in profiles (recommend_topn_profiles and recommend_user_knn_profiles).  Returns the LocalRDD
    of recommend_hybrid in the order of `profiles`, with .unknown_items and .counts.  exclude = {uid of a profile: iids}."""
    import torch
    _no_fold_in(alterEgoRDD, "recommend_hybrid_profiles")
    h = _hybrid_spec(n, n_nb, peer_cap, centred, min_common, own_mean, min_support, how, weights, rrf_c, pool_items, pool_users, min_lists)
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_hybrid_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    labels = sorted(index, key=index.get)
    d_q = torch.arange(len(labels), dtype=torch.int32, device=st.engine.dev)
    rules = _eligibility(st.engine.dev, labels, st.idt.iidx, len(st.idt.iids), allow_items, exclude, min_score)
    fused = _hybrid_lists(alterEgoRDD, "recommend_hybrid_profiles", st, eng2, F, nb, item_avg, d_q, True, alpha, n, decay, keep_held, rules, h)
    res = _hybrid_records(st, fused, labels, getattr(profiles, "ctx", None))
    res.unknown_items, res.counts = unknown, F.counts
    return res


def fuse_lists(results, n, how="rrf", weights=None, rrf_c=60.0, min_lists=1, score_index=1, dev="cuda:0"):
    """Late fusion of the lists of different calls -- recommend_topn, recommend_user_knn, related_items -- or of different AlterEgoRDD
    handles over the same target items: one list per source domain, one weight each (the late counterpart of union_alterego, which
    merges the rows before the model is built).  results: 1 .. 16 collected results [(label, [(iid, score, ...)*])*] (LocalRDDs or
    lists) with the same labels in the same order; a list longer than 1 024 entries is cut there.  score_index: where an entry
    holds its score (an int, or one per result; recommend_topn's decayed score is 2).  The iids of all results are numbered in
    sorted order for the call, so equal scores come out in that order.  Engine.fuse does the rest on the device.  Returns a
    LocalRDD of (label, [(iid, score, which)*]) with which = the indices of the results that named the iid, and .stats."""
    import torch
    from types import SimpleNamespace
    from . import device
    recs = [records_of(r) for r in results]
    w = device.Engine._fuse_args(len(recs), n, how, weights, rrf_c, min_lists)
    sidx = [int(score_index)] * len(recs) if isinstance(score_index, int) else [int(k) for k in score_index]
    labels = [rec[0] for rec in recs[0]]
    if len(sidx) != len(recs) or any([rec[0] for rec in r] != labels for r in recs):
        raise ValueError("fuse_lists: one score_index per result, and every result lists the same labels in the same order")
    ids = sorted({e[0] for r in recs for _, lst in r for e in lst})
    index = {x: k for k, x in enumerate(ids)}
    Q = len(labels)
    lists = []
    for r, k in zip(recs, sidx):
        width = min(max([len(lst) for _, lst in r] + [1]), 1024)
        cnt, item, score = np.zeros(max(Q, 1), np.int32), np.full((max(Q, 1), width), -1, np.int32), np.zeros((max(Q, 1), width), np.float64)
        for q, (_, lst) in enumerate(r):
            cnt[q] = min(len(lst), width)
            for t, e in enumerate(lst[:width]):
                item[q, t], score[q, t] = index[e[0]], e[k]
        lists.append(tuple(torch.from_numpy(a).to(dev)[:Q] for a in (cnt, item, score)))
    eng = device.Engine(SimpleNamespace(device=torch.device(dev), n_items=len(ids)))
    cnt, item, score, mask, stats = eng.fuse(lists, int(n), how, w, rrf_c, min_lists, n_ids=len(ids))
    cnt, item, score, mask = cnt.cpu().numpy(), item.cpu().numpy(), score.cpu().numpy(), mask.cpu().numpy()
    res = LocalRDD([(lab, [(ids[item[q, t]], float(score[q, t]), tuple(l for l in range(len(recs)) if (mask[q, t] >> l) & 1))
                           for t in range(cnt[q])]) for q, lab in enumerate(labels)], getattr(results[0], "ctx", None))
    res.stats = stats
    return res


def related_items(alterEgoRDD, baskets, cap, n, how="sum", keep_members=False, min_support=1, allow_items=None, exclude=None,
                  min_score=None, map_sources=False):
    """Related items for a basket, on the device: "what goes with these items" -- the product page, the cart, an anonymous
    session; no user and no rating takes part.  The front of recommend (profiles of the AlterEgo rows -> RecommenderSim, cap; no
    neighbour list is selected), then for every basket the n (1..1024) items most related to its members over the rows of the
    RecommenderSim matrix (Engine.related): an item's records are the entries that name it in the members' rows, its score their
    sum (how="sum"), mean ("mean") or largest ("max"); score descending, item index ascending on equal scores.  `baskets` is an
    RDD or list of (label, [iid*]) or (label, [(iid, weight)*]) -- weights multiply the member's similarities; a repeated member
    counts once per occurrence; a repeated label raises ValueError.  The members themselves are left out unless keep_members; an
    item with fewer than min_support records is dropped.  allow_items, exclude = {label: iids}, min_score: the eligibility rules of
    recommend_topn, applied before the cut.  Takes an AlterEgoRDD or an AlterEgoUnion.
    map_sources=True (an AlterEgoRDD only) is the cross-domain query -- a basket of movies gives related books: a member that is
    a source item is replaced by its target under the handle's replacement map before the call (looked up on the host; the map is
    downloaded once per call), and a source member without a replacement counts as unknown.  A union has one map per part: TypeError.
    Returns a LocalRDD of (label, [(iid, score, support)*]) in basket order with .stats = (candidates, dropped by min_support,
    dropped as non-finite, dropped below the floor, largest candidate count of a basket, records expanded) and .unknown_items =
    the members dropped because the id table does not know their iid (or, with map_sources, the map has no target for them)."""
    import torch
    if map_sources and isinstance(alterEgoRDD, AlterEgoUnion):
        raise TypeError("related_items(map_sources=True): a union of AlterEgo rows has one replacement map per part; map the "
                        "basket against one part's AlterEgoRDD")
    st, eng2, _, S = _tail_matrix(alterEgoRDD, cap, "related_items")
    idt, dev = st.idt, st.engine.dev
    recs = [(rec[0], list(rec[1])) for rec in (baskets.collect() if hasattr(baskets, "collect") else baskets)]
    labels = [lab for lab, _ in recs]
    if len(set(labels)) != len(labels):
        seen = set()
        raise ValueError("related_items(): basket label %r occurs more than once" % ([x for x in labels if x in seen or seen.add(x)][0],))
    mp = flags = None
    if map_sources:
        G = alterEgoRDD.G
        if getattr(G, "map", None) is None:
            raise ValueError("map_sources needs the replacement map of the generate pass (Engine.alterego keeps it on its result)")
        mp, flags = G.map.cpu().numpy(), st.engine.R.flags.cpu().numpy()
    ptr = np.zeros(len(recs) + 1, np.int64)
    item, weight, weighted, unknown = [], [], False, 0
    for k, (_, members) in enumerate(recs):
        for m in members:
            iid, w = (m[0], float(m[1])) if isinstance(m, (tuple, list)) else (m, 1.0)
            weighted = weighted or isinstance(m, (tuple, list))
            i = idt.iidx.get(iid)
            if i is not None and mp is not None and not (int(flags[i]) & 2):      # a source item: its target, if it has one
                i = int(mp[i]) if int(mp[i]) >= 0 else None
            if i is None:
                unknown += 1
                continue
            item.append(i); weight.append(w)
        ptr[k + 1] = len(item)
    d_ptr = torch.from_numpy(ptr).to(dev)
    d_item = torch.from_numpy(np.asarray(item, np.int32)).to(dev)
    d_w = torch.from_numpy(np.asarray(weight, np.float64)).to(dev) if weighted else None
    rules = _eligibility(dev, labels, idt.iidx, len(idt.iids), allow_items, exclude, min_score)
    cnt, it, score, support, stats = eng2.related(S, d_ptr, d_item, int(n), how=how, weights=d_w, keep_members=keep_members,
                                                  min_support=min_support, **rules)
    cnt, it, score, support = cnt.cpu().numpy(), it.cpu().numpy(), score.cpu().numpy(), support.cpu().numpy()
    iids = idt.iids
    out = [(lab, [(iids[it[q, t]], float(score[q, t]), int(support[q, t])) for t in range(cnt[q])]) for q, lab in enumerate(labels)]
    res = LocalRDD(out, getattr(baskets, "ctx", None))
    res.stats, res.unknown_items = stats, unknown
    return res


def popular_items(alterEgoRDD, cap, n, how="count", damping=0.0, min_count=1):
    """The most popular / best rated items of the resident profiles, on the device: the shelf an anonymous visitor sees, with no
    user, no evidence and no model.  The profiles of the AlterEgo rows, their item-major transposition (Engine.peer_index) and the
    ranking over it (Engine.pop_index): how="count" ranks by the profiles that hold an item, "mean" by (sum of its ratings +
    damping * the mean of all ratings) / (holders + damping); an item with fewer than min_count holders is not ranked; score
    descending, item index ascending on equal scores.  Returns [(iid, score)*], the first n of the ranking (fewer when it is
    shorter).  cap is taken for the symmetry of the tail calls; the ranking needs no RecommenderSim and does not depend on it.
    Takes an AlterEgoRDD or an AlterEgoUnion."""
    spec = _fill_spec(dict(how=how, damping=damping, min_count=min_count))
    if int(n) < 0:
        raise ValueError("n = %d: at least 0" % int(n))
    st, eng2, P = _tail_profiles(alterEgoRDD, "popular_items")
    pop = eng2.pop_index(eng2.peer_index(P), *spec)
    m = min(int(n), pop.n_ranked)
    item, score = pop.item[:m].cpu().numpy(), pop.score[:m].cpu().numpy()
    return [(st.idt.iids[int(i)], float(v)) for i, v in zip(item, score)]


def _item_fold_in(st, eng2, P, S, nb, item_avg, new_items):
    """new items [(iid, [(uid, rating)*])*] (an RDD or a list) -> (their RecommenderSim rows: Engine.item_foldin against the
    profiles P with the norms and the cap of S, the extended tables of Engine.item_foldin_tables, {iid: index in the batch},
    entries dropped for a uid the train set does not know).  The iids are labels; one the train set knows, or a repeated one,
    raises ValueError: a resident item has its row already."""
    idt = st.idt
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    recs = records_of(new_items)
    index = {}
    for k, rec in enumerate(recs):
        if rec[0] in index:
            raise ValueError("fold-in item %r occurs more than once" % (rec[0],))
        if rec[0] in idt.iidx:
            raise ValueError("fold-in item %r is an item of the train set" % (rec[0],))
        index[rec[0]] = k
    ptr = np.zeros(len(recs) + 1, np.int64)
    user, rating, unknown = [], [], 0
    for k, (_, raters) in enumerate(recs):
        for entry in raters:
            u = uidx.get(entry[0])
            if u is None:
                unknown += 1
                continue
            user.append(u); rating.append(float(entry[1]))
        ptr[k + 1] = len(user)
    rows, _, _ = eng2.item_foldin(P, ptr, np.asarray(user, np.int32), np.asarray(rating, np.float64), S.norm, S.cap)
    x_nb, x_avg = eng2.item_foldin_tables(nb, item_avg, rows)
    return rows, x_nb, x_avg, index, unknown


def _item_dicts(res, st, rows, x_nb, index):
    """.new_sim_pairs {iid: [(nid, sim)*]} and .new_item_info {iid: (avg, norm, raters)} of the batch of an item fold-in"""
    I, iids = len(st.idt.iids), st.idt.iids
    cnt, col, sim = [x[I:].cpu().numpy() for x in x_nb[:3]]
    avg, norm, n = rows.avg.cpu().numpy(), rows.norm.cpu().numpy(), np.diff(rows.ptr.cpu().numpy())
    res.new_sim_pairs = {iid: [(iids[col[q, t]], float(sim[q, t])) for t in range(cnt[q])] for iid, q in index.items() if cnt[q] > 0}
    res.new_item_info = {iid: (float(avg[q]), float(norm[q]), int(n[q])) for iid, q in index.items()}


def recommend_audience_items(alterEgoRDD, new_items, cap, keep, alpha, n, decay=False, keep_holders=False, neighbors=None,
                             allow_users=None, exclude=None, min_score=None):
    """recommend_audience for items that are not items of the train set -- a book that enters the catalogue: `new_items` is an
    RDD or list of (iid, [(uid, rating)*]), the ratings the item has collected so far from users of the train set.  Each item
    gets one row of RecommenderSim against the frozen AlterEgo profiles (item fold-in: Engine.item_foldin), its neighbour list
    by the rule of the resident lists, and then the audience of recommend_audience from the model trained on alterEgoRDD's rows,
    which stays as it is; the item's raters are its holders (left out unless keep_holders).  The iids are labels only: a
    repeated one, or one the train set knows, raises ValueError; an entry whose uid the train set does not know is dropped and
    counted in .unknown_users.  Works on a union of AlterEgo rows as well (it reads the tail only).  Returns the LocalRDD of
    (iid, [(uid, plain, decayed)*]) in the order of `new_items`, with .stats, .sim_pairs, .item_info, .unknown_users, .counts =
    (pairs, records, items with a pair), .new_sim_pairs {iid: [(nid, sim)*]} and .new_item_info {iid: (avg, norm, raters)}.
    allow_users, exclude = {iid of a new item: uids}, min_score: the eligibility rules of recommend_audience."""
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_audience_items")
    rows, x_nb, x_avg, index, unknown = _item_fold_in(st, eng2, P, S, nb, item_avg, new_items)
    I = len(st.idt.iids)
    iids = sorted(index, key=index.get)
    res = _audience_records(st, eng2, P, x_nb, x_avg, iids, st.idt.uids, alpha, n, decay, keep_holders, getattr(new_items, "ctx", None),
                            iidx={iid: I + q for iid, q in index.items()}, batch=(rows.ptr, rows.user),
                            rules=_eligibility(st.engine.dev, iids, _user_index(st.idt), len(st.idt.uids), allow_users, exclude, min_score))
    res.unknown_users, res.counts = unknown, rows.counts
    _tail_dicts(res, st, S, nb)
    _item_dicts(res, st, rows, x_nb, index)
    return res


def recommend_items(alterEgoRDD, new_items, testRDD, cap, keep, alpha, neighbors=None):
    """recommend for items that are not items of the train set: `new_items` as recommend_audience_items takes them and folds
    them in, testRDD the held-out (uid, [(iid, rating, ...)*]) records whose iids are looked up among the new items' labels
    first, then in the train set -- one that is neither is an item without a list.  Returns the LocalRDD of recommend (with
    .mae, .sim_pairs, .item_info) and .unknown_users, .counts, .new_sim_pairs, .new_item_info."""
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_items")
    rows, x_nb, x_avg, index, unknown = _item_fold_in(st, eng2, P, S, nb, item_avg, new_items)
    idt, I = st.idt, len(st.idt.iids)
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    iidx = dict(idt.iidx)
    iidx.update({iid: I + q for iid, q in index.items()})
    res = _predict_records(st, eng2, P, x_nb, x_avg, uidx, testRDD, alpha, iidx=iidx, n_items=I + len(index))
    res.unknown_users, res.counts = unknown, rows.counts
    _tail_dicts(res, st, S, nb)
    _item_dicts(res, st, rows, x_nb, index)
    return res


def recommend_profiles(alterEgoRDD, profiles, testRDD, cap, keep, alpha, neighbors=None):
    """recommend for users that are not rows of the train set: `profiles` as recommend_topn_profiles takes them, testRDD the
    held-out (uid, [(iid, rating, ...)*]) records of those users -- a uid is looked up among the profiles' labels, one without a
    profile is a user without ratings.  Returns the LocalRDD of recommend (with .mae, .sim_pairs, .item_info) and .unknown_items,
    .counts."""
    _no_fold_in(alterEgoRDD, "recommend_profiles")
    st, eng2, _, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "recommend_profiles")
    F, index, unknown = _fold_in(st, alterEgoRDD.G, profiles)
    res = _predict_records(st, eng2, F, nb, item_avg, index, testRDD, alpha)
    res.unknown_items, res.counts = unknown, F.counts
    _tail_dicts(res, st, S, nb)
    return res


class TopnEvaluation(object):
    """what evaluate_topn returns: .at {cutoff: dict(users, hit_rate, precision, recall, ndcg, map, mrr, coverage)}, .stats,
    .masks {uid: hit mask}, .sim_pairs, .item_info, .ils (mean intra-list similarity over the evaluated users; None unless the lists
    were diversified)"""

    def __init__(self):
        self.at, self.stats, self.masks, self.ils = {}, (0,) * 8, {}, None


def evaluate_topn(alterEgoRDD, testRDD, cap, keep, alpha, n, cutoffs=(5, 10, 20), rel_min=4.0, decay=False, keep_held=False,
                  neighbors=None, diversify=None, pool=None, fill=None, hybrid=None):
    """Hold-out evaluation of the top-N recommendation on the device: the set-up of recommend, then the held-out pairs of
    testRDD ((uid, [(iid, rating, ...)*]) records as recommend takes them, every (uid, iid) once) pick the users with a rating
    >= rel_min (Engine.eval_users), those users get their n best items (Engine.topn: recommend_topn's lists), and the lists
    are scored against the relevant pairs where they lie (Engine.topn_eval); no list is copied to the host.  A pair whose uid
    or iid the train set does not know is ignored.  Returns a TopnEvaluation: .at[c] for every cutoff c (ascending, 1 .. n, at
    most 8) = dict(users = evaluated users, hit_rate, precision, recall, ndcg, map, mrr = the means over them, coverage =
    distinct items within c over their lists); .stats = (evaluated users, relevant pairs, ignored pairs, pairs below rel_min,
    candidates scored, candidates dropped, largest `now`, largest candidate count); .masks {uid: int} for the evaluated users
    (bit r = the item at rank r is a relevant held-out item); .sim_pairs / .item_info like recommend.  ValueError on a
    repeated (uid, iid) or a rating that is not a number.
    diversify, pool as recommend_topn takes them: the lists that are scored are the re-ranked ones, and .ils is the mean intra-list
    similarity over the evaluated users (summed on the host from the per-user values; 0.0 without users), so one call per weight
    gives the accuracy / redundancy curve -- diversify = 0 the redundancy of the plain lists.
    fill as recommend_topn takes it: the lists that are scored are the completed ones (the same lists, filled in place on the
    device, go to Engine.topn_eval), and the result carries .fill_stats -- one call with and one without shows what the fill buys
    in recall and coverage.
    hybrid = a dict of recommend_hybrid's extra arguments (n_nb, and any of peer_cap, centred, min_common, own_mean, min_support,
    how, weights, rrf_c, pool_items, pool_users, min_lists): the lists that are scored are the fused ones of recommend_hybrid (n <=
    64), and .stats carries the item-based half's counters; .hybrid_stats = (top-N, user-kNN, fuse).  Together with diversify or
    fill it raises ValueError; None takes the path as it is without it."""
    import torch
    if hybrid is not None:
        if diversify is not None or pool is not None or fill is not None:
            raise ValueError("evaluate_topn: hybrid together with diversify or fill")
        if set(hybrid) - set(HYBRID_KEYS) or "n_nb" not in hybrid:
            raise ValueError("hybrid = %r: a dict of n_nb and any of %s" % (hybrid, ", ".join(HYBRID_KEYS[1:])))
        if not 1 <= int(n) <= 64:
            raise ValueError("n = %d: the evaluation takes lists of 1 .. 64" % int(n))
        hybrid = _hybrid_spec(n, **hybrid)
    if not isinstance(alterEgoRDD, (AlterEgoRDD, AlterEgoUnion)):
        raise TypeError("evaluate_topn() takes the AlterEgoRDD handle of generator_pipeline (rows resident on the device) or the "
                        "AlterEgoUnion of union_alterego")
    _diverse(n, diversify, pool)
    spec = _fill_spec(fill)
    recs = records_of(testRDD)
    seen = set()
    for uid, pairs in recs:
        for pair in pairs:
            if (uid, pair[0]) in seen:
                raise ValueError("held-out pair (%r, %r) occurs more than once" % (uid, pair[0]))
            seen.add((uid, pair[0]))
    try:
        real = np.fromiter((float(pair[1]) for _, pairs in recs for pair in pairs), np.float64)
    except (TypeError, ValueError):
        real = None
    if real is None or np.isnan(real).any():
        raise ValueError("a held-out rating is not a number")
    st, eng2, P, S, nb, item_avg = _tail_setup(alterEgoRDD, cap, keep, neighbors, "evaluate_topn")
    idt, dev = st.idt, st.engine.dev
    uidx = getattr(idt, "uidx", None) or {u: k for k, u in enumerate(idt.uids)}
    tu = np.fromiter((uidx.get(uid, -1) for uid, pairs in recs for _ in pairs), np.int32)
    ti = np.fromiter((idt.iidx.get(pair[0], -1) for _, pairs in recs for pair in pairs), np.int32)
    cuts = [int(c) for c in cutoffs]
    d_tu, d_ti, d_tr = torch.from_numpy(tu).to(dev), torch.from_numpy(ti).to(dev), torch.from_numpy(real).to(dev)
    U, I = len(idt.uids), len(idt.iids)
    n_rel, users, counts = eng2.eval_users(d_tu, d_ti, d_tr, float(rel_min), U, I)
    hybrid_stats = None
    if hybrid is not None:
        cnt, item, _, _, hybrid_stats = _hybrid_lists(alterEgoRDD, "evaluate_topn", st, eng2, P, nb, item_avg, users, False, alpha, n, decay,
                                                      keep_held, None, hybrid)
        stats, ils = hybrid_stats[0], None
    else:
        cnt, item, plain, decayed, stats, ils, _ = _topn_lists(eng2, P, nb, users, item_avg, alpha, n, decay, keep_held, dev, None,
                                                               _diverse(n, diversify, pool, eng2, S))
    fill_stats = None
    if spec:
        cnt, item, _, _, _, fill_stats = _fill_lists(eng2, P, P, users, item_avg, (cnt, item, plain, decayed), spec, keep_held, None)
    mask, _, agg, cover = eng2.topn_eval(d_tu, d_ti, d_tr, float(rel_min), n_rel, users, cnt, item, cuts, I)
    res = TopnEvaluation()
    agg, cover = agg.cpu().numpy(), cover.cpu().numpy()
    for k, c in enumerate(cuts):
        m = float(agg[k, 0])
        mean = (lambda x: x / m) if m else (lambda x: 0.0)
        res.at[c] = dict(users=int(agg[k, 0]), hit_rate=mean(float(agg[k, 1])), precision=mean(float(agg[k, 3])),
                         recall=mean(float(agg[k, 4])), ndcg=mean(float(agg[k, 5])), map=mean(float(agg[k, 6])),
                         mrr=mean(float(agg[k, 7])), coverage=int(cover[k]))
    res.stats = tuple(counts) + tuple(stats)
    if spec:
        res.fill_stats = fill_stats
    if hybrid_stats is not None:
        res.hybrid_stats = hybrid_stats
    if ils is not None:
        v = ils.cpu().numpy()
        res.ils = math.fsum(v.tolist()) / len(v) if len(v) else 0.0
    res.masks = {idt.uids[u]: int(b) & 0xffffffffffffffff for u, b in zip(users.cpu().tolist(), mask.cpu().tolist())}
    _tail_dicts(res, st, S, nb)
    return res


# ---------------------------------------------------------------------------------------------
def sim_from_records(state, records):
    """Device SimResult from generic ((iid1,iid2),(sim,mutu,frac,label)) records (any order)."""
    iidx = state.idt.iidx
    I = len(state.idt.iids)
    n = len(records)
    a = np.fromiter((iidx[k[0]] for k, _ in records), np.int64, n)
    b = np.fromiter((iidx[k[1]] for k, _ in records), np.int32, n)
    sim = np.fromiter((v[0] for _, v in records), np.float64, n)
    mutu = np.fromiter((v[1] for _, v in records), np.float64, n)
    frac = np.fromiter((v[2] for _, v in records), np.float64, n)
    o = np.lexsort((b, a))
    row_ptr = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(a, minlength=I), out=row_ptr[1:])
    info = np.zeros((I, 4))
    return state.engine.sim_from_host(row_ptr, b[o], sim[o], mutu[o].astype(np.int32), None, info, frac=frac[o])


def ext_from_records(state, records):
    """Device candidate arrays from generic (start, [(end, xsim)*]) records."""
    import torch
    from . import device, hipabi as abi
    eng = state.engine
    iidx = state.idt.iidx
    I = len(state.idt.iids)
    st = np.fromiter((iidx[s] for s, lst in records for _ in lst), np.int64)
    en = np.fromiter((iidx[e] for _, lst in records for (e, _) in lst), np.int32)
    va = np.fromiter((v for _, lst in records for (_, v) in lst), np.float64)
    o = np.lexsort((en, st))
    xs_ptr = np.zeros(I + 1, np.int64)
    np.cumsum(np.bincount(st, minlength=I), out=xs_ptr[1:])
    d = eng.dev
    E = device.ExtResult()
    pad = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros(1), dt)).to(d)
    E.xs_ptr = torch.from_numpy(xs_ptr).to(d)
    E.xs_off = E.xs_ptr[:-1].contiguous()
    E.xs_end, E.xs_val = pad(en[o], np.int32), pad(va[o], np.float64)
    E.n_cand = torch.zeros(max(I, 1), dtype=torch.int32, device=d)
    E.top_end = torch.full((max(I, 1), abi.TOPC), -1, dtype=torch.int32, device=d)
    E.top_val = torch.zeros((max(I, 1), abi.TOPC), dtype=torch.float64, device=d)
    abi.check(abi.lib.xmap_topc_from_lists(device._stream(d), abi.i32(I), abi.vp(E.xs_ptr), abi.vp(E.xs_end),
                                           abi.vp(E.xs_val), abi.vp(E.n_cand), abi.vp(E.top_end), abi.vp(E.top_val)))
    return E
