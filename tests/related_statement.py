"""The statement of the related-items call (include/xmap_hip.h, "related items"; csrc/stage_e_related.hip) in plain Python, written
from the rules and not from the kernel: records in basket-position order and storage order, Python floats for the sums, one
np.float64 product per weighted record.  Also the builders of the designed inputs the GPU test runs (tests/test_gpu_related.py),
built directly as CSRs -- no training run -- whose census tests/test_cpu_related_statement.py takes on the CPU.  Every layer must
reproduce these bit for bit."""
import math

import numpy as np

SUM, MEAN, MAX = 0, 1, 2
KEEP_MEMBERS = 1
HOWS = {"sum": SUM, "mean": MEAN, "max": MAX}
FAMILIES = ["dyadic", "generic", "ties", "special"]


class Matrix(object):
    """a RecommenderSim CSR: rows in storage order, not sorted; a row may hold a column twice and its own index"""

    def __init__(self, row_ptr, col, sim, n_items=None):
        self.row_ptr = np.ascontiguousarray(row_ptr, np.int64)
        self.col = np.ascontiguousarray(col, np.int32)
        self.sim = np.ascontiguousarray(sim, np.float64)
        self.n_items = len(self.row_ptr) - 1 if n_items is None else int(n_items)


def _mul(w, s):
    with np.errstate(all="ignore"):
        return float(np.float64(w) * np.float64(s))


def raw_records(M, b_ptr, b_item, weights=None):
    """per query (the set of its valid members, {item: [v*] in record order}) before any rule: for each basket position in order
    whose member is an item of the matrix, each entry of the member's row in storage order whose column is an item"""
    I = M.n_items
    rp, col, sim = M.row_ptr.tolist(), M.col.tolist(), M.sim.tolist()
    b_ptr, b_item = [int(x) for x in b_ptr], [int(x) for x in b_item]
    w = None if weights is None else [float(x) for x in weights]
    out = []
    for q in range(len(b_ptr) - 1):
        members, rec = set(), {}
        for p in range(b_ptr[q], b_ptr[q + 1]):
            b = b_item[p]
            if not 0 <= b < I:
                continue                        # a member without a row
            members.add(b)
            for e in range(rp[b], rp[b + 1]):
                if 0 <= col[e] < I:
                    rec.setdefault(col[e], []).append(sim[e] if w is None else _mul(w[p], sim[e]))
        out.append((members, rec))
    return out


def score_of(vs, how):
    """the score of an item over its records in record order"""
    if how == MAX:
        if any(v != v for v in vs):
            return float("nan")
        best = vs[0]
        for v in vs[1:]:
            if v > best:                        # the first occurrence's bits among equals
                best = v
        return best
    s = 0.0
    with np.errstate(all="ignore"):
        for v in vs:
            s = float(np.float64(s) + np.float64(v))
        return s if how == SUM else float(np.float64(s) / np.float64(float(len(vs))))


def related_statement(M, b_ptr, b_item, n_top, how=SUM, flags=0, min_support=1, weights=None, allow=None, exclude=None, min_score=None,
                      raw=None):
    """-> (cnt [Q], item [Q][n_top], score [Q][n_top], support [Q][n_top], stats [6], detail).  allow: bool [I] or None; exclude:
    one list of ids per query or None; min_score: the floor or None.  detail: rule2 / mask / excluded = candidates the rules 2,
    3 (exclusion list) and 3 (mask) removed, in that order of the rules (an item counts for the first that removes it);
    scored = per query {item: (score, support)} of every candidate that reached rule 5; nonfinite = the scores rule 6 dropped"""
    I = M.n_items
    raw = raw_records(M, b_ptr, b_item, weights) if raw is None else raw
    n_q = len(raw)
    cnt = np.zeros(n_q, np.int32)
    item = np.full((n_q, n_top), -1, np.int32)
    score = np.zeros((n_q, n_top))
    support = np.zeros((n_q, n_top), np.int32)
    stats = [0] * 6
    detail = dict(rule2=0, excluded=0, mask=0, scored=[], nonfinite=[])
    floor = -math.inf if min_score is None else float(min_score)
    for q, (members, rec) in enumerate(raw):
        ex = set() if exclude is None else {int(x) for x in exclude[q]}
        kept, scored = [], {}
        n_cand = 0
        for it in sorted(rec):
            vs = rec[it]
            eligible = it not in ex and (allow is None or bool(allow[it]))
            if eligible:
                stats[5] += len(vs)             # the records the expansion writes
            if not (flags & KEEP_MEMBERS) and it in members:
                detail["rule2"] += 1
                continue
            if it in ex:
                detail["excluded"] += 1
                continue
            if not eligible:
                detail["mask"] += 1
                continue
            n_cand += 1
            if len(vs) < min_support:
                stats[1] += 1
                continue
            s = score_of(vs, how)
            scored[it] = (s, len(vs))
            if not math.isfinite(s):
                stats[2] += 1
                detail["nonfinite"].append(s)
                continue
            if s < floor:
                stats[3] += 1
                continue
            kept.append((it, s, len(vs)))
        stats[0] += n_cand
        stats[4] = max(stats[4], n_cand)
        kept.sort(key=lambda t: (-t[1], t[0]))  # score descending as numbers (-0.0 == 0.0), item index ascending
        detail["scored"].append(scored)
        detail.setdefault("kept", []).append(kept)
        cnt[q] = min(len(kept), n_top)
        for t, (it, s, sup) in enumerate(kept[:n_top]):
            item[q, t], score[q, t], support[q, t] = it, s, sup
    return cnt, item, score, support, stats, detail


# ---------------------------------------------------------------------------------------------------- the designed inputs
N_ROWS, N_ITEMS, BIG, BIG_LEN = 600, 3600, 599, 3000       # rows 0 .. 599 hold entries; row BIG holds 3000 over the whole item space
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257]                # row i < BIG has LENGTHS[i % 8] entries, except the overlap group
GROUP = list(range(520, 585))                              # 65 items whose rows share most of 64 columns, and 8 of them all
WEIGHTS = [1.0, 0.0, -1.0, 0.3, 2.5, -0.7, 1e-3, 3.0]


def _values(family, rng, n):
    if family == "dyadic":
        return rng.randint(-4096, 4097, n) / 1024.0
    if family == "generic":
        return np.where(rng.rand(n) < 0.5, -1.0, 1.0) * np.ldexp(1.0 + rng.rand(n), rng.randint(-40, 41, n))
    if family == "ties":                        # non-negative, a handful of values: hundreds of equal scores in a long row
        return rng.randint(1, 4, n) / 4.0
    v = rng.randint(-4096, 4097, n) / 1024.0    # special: NaN, the infinities, the zeros and subnormals among dyadic values
    special = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1060]
    at = rng.rand(n) < 0.04
    v[at] = np.asarray(special)[rng.randint(0, len(special), int(at.sum()))]
    return v


def design(family):
    """the matrix of a family: the same structure (lengths, repeated columns, self entries), the family's values"""
    rng = np.random.RandomState(20 + FAMILIES.index(family))
    srng = np.random.RandomState(7)             # the structure is the same for every family
    base = srng.choice([i for i in range(N_ROWS) if i not in GROUP], 64, replace=False)   # the first 8: in every row of the group
    rows = []
    for i in range(N_ROWS):
        if i == BIG:
            c = srng.choice(N_ITEMS, BIG_LEN, replace=False)
        elif i in GROUP:
            c = srng.permutation(np.concatenate([base[:8], srng.choice(base[8:], 53, replace=False), srng.randint(0, N_ROWS, 3)]))
        else:
            c = srng.choice(N_ROWS, LENGTHS[i % 8], replace=False)
        c = c.astype(np.int32)
        if len(c) >= 63 and i % 3 == 0:
            c[len(c) // 2] = c[0]               # a column twice
        if len(c) >= 1 and i % 5 == 0:
            c[len(c) - 1] = i                   # its own index
        rows.append(c)
    row_ptr = np.zeros(N_ITEMS + 1, np.int64)
    row_ptr[1:N_ROWS + 1] = np.cumsum([len(c) for c in rows])
    row_ptr[N_ROWS + 1:] = row_ptr[N_ROWS]
    col = np.concatenate(rows)
    return Matrix(row_ptr, col, _values(family, rng, len(col)), N_ITEMS)


def plain_rows(M):
    """the items whose row holds neither its own index nor a column twice, and at least one entry"""
    out = []
    for i in range(M.n_items):
        c = M.col[M.row_ptr[i]:M.row_ptr[i + 1]].tolist()
        if c and i not in c and len(set(c)) == len(c):
            out.append(i)
    return out


def baskets():
    """-> (b_ptr, b_item, weights): the designed baskets, the same for every family"""
    rng = np.random.RandomState(11)
    B = [[],                                    # empty
         [3],                                   # one member
         [8],                                   # one member whose row is empty
         [N_ITEMS + 5],                         # one member without a row
         [-1, N_ITEMS, 12, N_ITEMS + 7, -2147483648, 2147483647],       # members out of range around a valid one
         [13, 13, 21],                          # a repeated member
         [5, 6],
         [int(x) for x in rng.choice(N_ROWS, 64, replace=False)],
         [int(x) for x in rng.choice(N_ROWS, 65, replace=False)],
         list(GROUP),                           # rows that overlap in most columns: support up to 65
         [BIG],                                 # more than 2 048 candidates
         [BIG, 5, 6, BIG],
         []]
    B.append(list(B[7]))                        # repeated queries
    B.append(list(B[10]))
    B += [[i] for i in range(N_ROWS) if LENGTHS[i % 8] >= 63 and i not in GROUP and i != BIG][:28]      # long single rows: ties at the cut
    B += [[int(x) for x in rng.randint(0, N_ROWS, rng.randint(1, 7))] for _ in range(12)]
    B += [[BIG, i] for i in range(1, 21)]      # twenty more baskets of thousands of candidates: ties at the 256th and the 1024th place
    b_ptr = np.concatenate([[0], np.cumsum([len(b) for b in B])]).astype(np.int64)
    b_item = np.asarray([x for b in B for x in b], np.int64).astype(np.int32)
    weights = np.asarray([WEIGHTS[p % len(WEIGHTS)] for p in range(len(b_item))], np.float64)
    return b_ptr, b_item, weights


def rules(b_ptr):
    """-> (allow bool [I], exclude: one list per query with repeats and ids out of range, floor) of the designed rules case"""
    rng = np.random.RandomState(13)
    allow = np.arange(N_ITEMS) % 3 != 0
    exclude = []
    for q in range(len(b_ptr) - 1):
        ids = [int(x) for x in rng.randint(0, N_ROWS, rng.randint(0, 9))]
        exclude.append(ids + ids[:2] + ([-1, N_ITEMS, N_ITEMS + 9] if q % 2 else []))
    return allow, exclude, 0.5
