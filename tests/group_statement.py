"""The statement of the group lists (xmap_group_topn_rows, include/xmap_hip.h) in NumPy and Python, applied to what the
existing statement of top-N gives per member: test_gpu_topn.score_users' {user: [(item, plain, decayed, now, held)*]} -- the items a
user's own rows give evidence for -- plus the set of items every user holds.  No device.

A group is a list of member indices in order (repeats count as often as listed; an index outside the users, or a user without
rows, is a member that holds nothing and has no evidence).  Candidates: the union of the members' evidence items -> without
`keep_held` every item ANY member holds leaves -> the ids of the GROUP's exclusion list leave -> what remains meets `allow`.  Per
candidate and member the score is the member's own (plain, decayed), or the item average where the member has no evidence.
Dropped, in this order: a member pair with status 2 (or a non-finite average for a member without evidence), the veto (some
member's rank_by score < veto), the floor (aggregate rank_by score < min_score).  Aggregates: the mean by a left-to-right loop
starting from the first member's score and one division; min / max as numbers, the earliest member's bits on equal values.
Ranking: aggregate rank_by score descending, item ascending."""
import math

import numpy as np

from filter_statement import allowed

MEAN, MIN, MAX = 0, 1, 2
MAX_MEMBERS = 64


def held_sets(ptr, pit, n_items):
    """[set of the items in [0, n_items) user u holds]"""
    pit = np.asarray(pit).tolist()
    return [{i for i in pit[int(ptr[u]):int(ptr[u + 1])] if 0 <= i < n_items} for u in range(len(ptr) - 1)]


def aggregate(scores, how):
    """(aggregate, index of the least) of one candidate's member scores in list order"""
    if how == MEAN:
        acc = scores[0]
        for s in scores[1:]:
            acc = acc + s
        agg = acc / float(len(scores))
    else:
        agg = scores[0]
        for s in scores[1:]:
            if (s < agg) if how == MIN else (s > agg):
                agg = s
    return agg


def least(scores):
    low = 0
    for j, s in enumerate(scores):
        if s < scores[low]:
            low = j
    return low


def member_pairs(scored, held, u, keep_held, ok_id):
    """the pairs the member pass scores for user u: evidence, the mask, and -- without keep_held -- not held by u itself (such an
    item leaves the group whoever has evidence for it)"""
    return [c for c in scored.get(int(u), []) if ok_id[c[0]] and (keep_held or c[0] not in held[int(u)])] if 0 <= u < len(held) else []


def expected_group(scored, held, groups, avg, n, rank_by, keep_held, n_w, how, n_ids, veto=None, allow=None, exclude=None,
                   min_score=None, census=None):
    """(lists [[(item, plain, decayed, low)*]*], stats [8]) of the groups.  exclude: one sequence of ids per GROUP (or None).
    census (a dict, optional) takes counts of what the input shows."""
    assert how in (MEAN, MIN, MAX) and all(len(g) <= MAX_MEMBERS for g in groups)
    ok_id = allowed(allow, n_ids)
    floor = -math.inf if min_score is None else float(min_score)
    veto = -math.inf if veto is None else float(veto)
    assert floor == floor and veto == veto
    U = len(held)
    lists, stats = [], [0] * 8
    cz = dict(candidates=0, held_by_another=0, two_or_more=0, lacking=0, empty=0, widest=0, ghosts=0)
    for g, members in enumerate(groups):
        members = [int(u) for u in members]
        cz["ghosts"] += sum(not 0 <= u < U for u in members)
        by_member = []
        for u in members:
            pairs = member_pairs(scored, held, u, keep_held, ok_id)
            stats[0] += len(pairs)
            stats[2] = max([stats[2]] + [c[3] for c in pairs])
            by_member.append({c[0]: c for c in pairs})
        union = set()
        for d in by_member:
            union |= set(d)
        if not keep_held:
            gone = set()
            for u in members:
                if 0 <= u < U:
                    gone |= held[u]
            cz["held_by_another"] += len(union & gone)
            union -= gone
        ex = set() if exclude is None or exclude[g] is None else {int(x) for x in exclude[g]}
        stats[5] += len(union & ex)
        union -= ex
        cand = sorted(union)
        stats[7] += len(cand)
        stats[3] = max(stats[3], len(cand))
        cz["candidates"] += len(cand)
        cz["widest"] = max(cz["widest"], len(cand))
        cz["empty"] += not cand
        kept = []
        for i in cand:
            base = float(avg[i])
            sp, sd, bad = [], [], False
            with_ev = 0
            for d in by_member:
                c = d.get(i)
                if c is None:
                    sp.append(base)
                    sd.append(base)
                    bad |= not math.isfinite(base)
                else:
                    with_ev += 1
                    if c[1] is None or c[3] > n_w:
                        bad = True
                        sp.append(0.0)
                        sd.append(0.0)
                    else:
                        sp.append(c[1])
                        sd.append(c[2])
            cz["two_or_more"] += with_ev >= 2
            cz["lacking"] += with_ev < len(members)
            if bad:
                stats[1] += 1
                continue
            rs = sd if rank_by else sp
            if any(s < veto for s in rs):
                stats[6] += 1
                continue
            ap, ad = aggregate(sp, how), aggregate(sd, how)
            if (ad if rank_by else ap) < floor:
                stats[4] += 1
                continue
            kept.append((i, ap, ad, least(rs)))
        kept.sort(key=lambda c: (- c[1 + rank_by], c[0]))
        lists.append(kept[:n])
    if census is not None:
        census.update(cz)
    return lists, stats


def check_group_output(out, want, n):
    """out = (cnt [G], item, plain, decayed, low [G][n], stats) as NumPy arrays; items and low exactly, scores as uint64 views,
    the padding behind the count, all eight stats"""
    cnt, item, plain, decay, low = out[:5]
    lists, stats = want
    assert cnt.tolist() == [len(l) for l in lists]
    for q, l in enumerate(lists):
        k = len(l)
        assert item[q, :k].tolist() == [c[0] for c in l], q
        assert np.array_equal(plain[q, :k].view(np.uint64), np.asarray([c[1] for c in l], np.float64).view(np.uint64)), q
        assert np.array_equal(decay[q, :k].view(np.uint64), np.asarray([c[2] for c in l], np.float64).view(np.uint64)), q
        assert low[q, :k].tolist() == [c[3] for c in l], q
        assert (item[q, k:] == -1).all() and (low[q, k:] == -1).all()
        assert not plain[q, k:].view(np.uint64).any() and not decay[q, k:].view(np.uint64).any()
    if len(out) > 5 and out[5] is not None:
        assert [int(x) for x in out[5]] == [int(x) for x in stats]
