"""The brute-force statement of the eligibility rules of top-N and audience (xmap_rec_filter, include/xmap_hip.h), applied to
what the existing statements give: test_gpu_topn.score_users' {user: [(item, plain, decayed, now, held)*]} for top-N, and
test_gpu_audience.statement's {item: [(user, plain, decayed, now, held)*]} for audience -- the same shape, {query key: [(id,
plain, decayed, now, held)*]}, so one function serves both.  NumPy only, no device.

Order of the rules: the candidates as today -> the held items / the holders leave unless `keep` -> the ids of the QUERY's
exclusion list leave -> what remains meets `allow` -> scores -> the status-2 candidates are dropped and counted -> the
candidates below the floor are dropped and counted -> selection (score descending, id ascending; as the unfiltered calls)."""
import numpy as np


def allowed(allow, n):
    """allow as a bool array [n]: None (every id), a bool array, or uint32 words in the bit order of the header (garbage at or
    beyond n is cut off)"""
    if allow is None:
        return np.ones(n, bool)
    a = np.asarray(allow)
    if a.dtype == np.bool_:
        assert a.shape == (n,)
        return a
    assert a.dtype == np.uint32 and len(a) == (n + 31) // 32
    return np.unpackbits(a.astype("<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def expected_filtered(scored, queries, n, rank_by, keep, n_w, n_ids, allow=None, exclude=None, min_score=None):
    """(lists [[(id, plain, decayed)*]*], stats [6]) of the queries.  exclude: one sequence of ids per QUERY (or None); allow:
    see allowed(); min_score None = no floor.  stats = (scored, dropped, largest now, widest) over the eligible candidates,
    then the candidates below the floor and the candidate pairs the mask or the lists removed."""
    ok_id = allowed(allow, n_ids)
    floor = -np.inf if min_score is None else float(min_score)
    assert floor == floor
    lists, n_scored, dropped, max_now, widest, floored, removed = [], 0, 0, 0, 0, 0, 0
    for q, key in enumerate(queries):
        cand = [c for c in scored.get(int(key), []) if keep or not c[4]]
        ex = set() if exclude is None or exclude[q] is None else {int(x) for x in exclude[q]}
        elig = [c for c in cand if c[0] not in ex and ok_id[c[0]]]
        removed += len(cand) - len(elig)
        n_scored += len(elig)
        widest = max(widest, len(elig))
        max_now = max([max_now] + [c[3] for c in elig])
        kept = [c for c in elig if c[1] is not None and c[3] <= n_w]
        dropped += len(elig) - len(kept)
        above = [c for c in kept if c[1 + rank_by] >= floor]
        floored += len(kept) - len(above)
        above.sort(key=lambda c: (- c[1 + rank_by], c[0]))
        lists.append([(c[0], c[1], c[2]) for c in above[:n]])
    return lists, (n_scored, dropped, max_now, widest, floored, removed)
