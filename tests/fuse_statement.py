"""The statement of xmap_fuse_rows (include/xmap_hip.h, "fused lists") in plain loops over NumPy scalars, and the builders of
the designed inputs that tests/test_cpu_fuse_statement.py takes a census of and tests/test_gpu_fuse.py runs on the device.

A list is a FuseIn(cnt int32 [Q], item int32 [Q][width], score float64 [Q][width] or None, weight).  Every float operation below
is one np.float64 operation: one rounding per step, no fused multiply-add, IEEE division."""
import collections

import numpy as np

RRF, SUM, MEAN = 0, 1, 2
MAX_LISTS, BLOCK_RECORDS = 16, 2048
FuseIn = collections.namedtuple("FuseIn", "cnt item score weight")
Case = collections.namedtuple("Case", "lists n_ids how rrf_c")


def width(L):
    return int(L.item.shape[1])


def total_width(lists):
    return sum(width(L) for L in lists)


def records(lists, n_ids, q):
    """the records (id, l, r) of query q in record order"""
    out = []
    for l, L in enumerate(lists):
        m = min(max(int(L.cnt[q]), 0), width(L))
        for r in range(m):
            i = int(L.item[q, r])
            if 0 <= i < n_ids:
                out.append((i, l, r))
    return out


def scores(lists, n_ids, q, how, rrf_c, reverse=False):
    """{id: (score, mask)} of query q over its records in record order (reverse: in the opposite order -- what an unstable sort
    could do; the census measures how many scores that changes)"""
    by_id = collections.OrderedDict()
    for rec in records(lists, n_ids, q):
        by_id.setdefault(rec[0], []).append(rec)
    out = {}
    c = np.float64(rrf_c)
    for i, recs in by_id.items():
        num, den, mask = np.float64(0.0), np.float64(0.0), 0
        for (_, l, r) in (recs[::-1] if reverse else recs):
            w = np.float64(lists[l].weight)
            with np.errstate(all="ignore"):
                t = w / (c + np.float64(r + 1)) if how == RRF else w * np.float64(lists[l].score[q, r])
                num = num + t
                den = den + w
            mask |= 1 << l
        with np.errstate(all="ignore"):
            out[i] = (num / den if how == MEAN else num, mask)
    return out


def fuse_statement(lists, n_ids, how, rrf_c, min_lists, n_top):
    """-> (cnt [Q], id [Q][n_top], score [Q][n_top], lists [Q][n_top], stats [5])"""
    Q = len(lists[0].cnt)
    o_cnt = np.zeros(Q, np.int32)
    o_id = np.full((Q, n_top), -1, np.int32)
    o_score = np.zeros((Q, n_top), np.float64)
    o_mask = np.zeros((Q, n_top), np.int32)
    st = [0, 0, 0, 0, 0]
    for q in range(Q):
        st[4] += len(records(lists, n_ids, q))
        sc = scores(lists, n_ids, q, how, rrf_c)
        st[0] += len(sc)
        st[3] = max(st[3], len(sc))
        kept = []
        for i, (s, mask) in sc.items():
            if bin(mask).count("1") < min_lists:
                st[1] += 1
            elif not np.isfinite(s):
                st[2] += 1
            else:
                kept.append((-float(s), i, s, mask))        # -0.0 and 0.0 compare equal: the id decides
        kept.sort(key=lambda k: (k[0], k[1]))
        o_cnt[q] = min(len(kept), n_top)
        for j, (_, i, s, mask) in enumerate(kept[:n_top]):
            o_id[q, j], o_score[q, j], o_mask[q, j] = i, s, mask
    return o_cnt, o_id, o_score, o_mask, st


def candidate_counts(lists, n_ids):
    return [len({i for i, _, _ in records(lists, n_ids, q)}) for q in range(len(lists[0].cnt))]


# ------------------------------------------------------------------------------------------------------- shaping a call
def pad_width(L, w):
    """the same list at a larger row stride"""
    Q, w0 = L.item.shape
    item = np.full((Q, w), -1, np.int32)
    item[:, :w0] = L.item
    score = None
    if L.score is not None:
        score = np.zeros((Q, w), np.float64)
        score[:, :w0] = L.score
    return FuseIn(L.cnt, item, score, L.weight)


def empty_list(Q, w=1024, scored=True, weight=1.0):
    return FuseIn(np.zeros(Q, np.int32), np.full((Q, w), -1, np.int32), np.zeros((Q, w), np.float64) if scored else None, weight)


def on_sorted_route(lists):
    """the same records with the sum of the widths above BLOCK_RECORDS: an all-empty list of width 1 024 appended, or -- with 16
    lists already -- the first list's stride padded"""
    lists = list(lists)
    if total_width(lists) > BLOCK_RECORDS:
        return lists
    if len(lists) < MAX_LISTS:
        while total_width(lists) <= BLOCK_RECORDS and len(lists) < MAX_LISTS:
            lists.append(empty_list(len(lists[0].cnt), scored=lists[0].score is not None))
    if total_width(lists) <= BLOCK_RECORDS:
        lists[0] = pad_width(lists[0], width(lists[0]) + BLOCK_RECORDS + 1 - total_width(lists))
    assert total_width(lists) > BLOCK_RECORDS and all(width(L) <= 1024 for L in lists)
    return lists


# ------------------------------------------------------------------------------------------------------- the designed inputs
def _perm_lists(rng, Q, n_ids, widths, scored=True, weights=None):
    lists = []
    for l, w in enumerate(widths):
        item = np.stack([rng.permutation(n_ids)[:w] if n_ids >= w else rng.randint(0, n_ids, w) for _ in range(Q)]).astype(np.int32)
        score = rng.uniform(-2.0, 5.0, (Q, w)) if scored else None
        lists.append(FuseIn(np.full(Q, w, np.int32), item, score, 1.0 if weights is None else weights[l]))
    return lists


def ties():
    """two RRF lists, the second the reverse of the first (width 64, c = 60, equal weights): rank r and rank 63 - r get the same
    two terms in opposite order -- an addition of two terms commutes, so 32 pairs of bit-equal scores per query"""
    rng = np.random.RandomState(11)
    Q, n_ids = 6, 500
    a = _perm_lists(rng, Q, n_ids, [64], scored=False)[0]
    b = FuseIn(a.cnt, np.ascontiguousarray(a.item[:, ::-1]), None, 1.0)
    return Case([a, b], n_ids, RRF, 60.0)


def order():
    """SUM over three lists in which one id scores 1e300, -1e300, 1.0: 1.0 in record order, 0.0 in any order that adds the 1.0
    before the last large term; the other queries permute the three and hold generic ids beside them"""
    rng = np.random.RandomState(12)
    Q, n_ids, w = 6, 40, 5
    vals = [(1e300, -1e300, 1.0), (1.0, 1e300, -1e300), (1e300, 1.0, -1e300), (-1e300, 1e300, 1.0), (1.0, -1e300, 1e300), (-1e300, 1.0, 1e300)]
    lists = _perm_lists(rng, Q, n_ids - 1, [w, w, w])
    for q in range(Q):
        for l in range(3):
            r = (q + l) % w
            lists[l].item[q, r] = n_ids - 1     # the designed id: in no list otherwise (the generic ids stay below it)
            lists[l].score[q, r] = vals[q][l]
    return Case(lists, n_ids, SUM, 0.0)


def generic():
    """three to five RRF lists with unequal weights over random ranks: lists 3 and 4 are empty for a third of the queries each"""
    rng = np.random.RandomState(13)
    Q, n_ids = 24, 90
    lists = _perm_lists(rng, Q, n_ids, [63, 64, 65, 64, 33], weights=[1.0, 0.7, 1.3, 0.45, 2.1])
    for q in range(Q):
        if q % 3 == 1:
            lists[3].cnt[q] = 0
        if q % 3 == 2:
            lists[3].cnt[q] = 0
            lists[4].cnt[q] = 0
    return Case(lists, n_ids, RRF, 60.0)


def special():
    """+-0.0, subnormals, inf and NaN scores, a negative weight and weights that sum to 0.0 (MEAN: den == 0.0 for an id of both
    lists): run under SUM and MEAN"""
    rng = np.random.RandomState(14)
    Q, n_ids, w = 8, 30, 12
    lists = _perm_lists(rng, Q, n_ids, [w, w, w], weights=[1.0, -1.0, 0.5])
    sp = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, np.inf, -np.inf, np.nan, 1e308, -1e308]
    for q in range(Q):
        for l in range(3):
            for k in range(4):
                lists[l].score[q, (3 * q + 5 * l + k) % w] = sp[(q + 3 * l + 2 * k) % len(sp)]
    # query 0: every id scores +-0.0 -- the selection is by id, and the sign bit comes back
    for l in range(3):
        lists[l].score[0, :] = [(-0.0 if (r + l) % 2 else 0.0) for r in range(w)]
    return Case(lists, n_ids, SUM, 0.0)


def shapes():
    """widths 1, 63, 64, 65, 1 024; counts negative, 0, equal to the width, above it; ids -1 and n_ids; an id twice in one list;
    queries without records between queries with records"""
    rng = np.random.RandomState(15)
    Q, n_ids = 9, 1500
    lists = _perm_lists(rng, Q, n_ids, [1, 63, 64, 65, 1024], weights=[2.0, 1.0, 1.5, 0.25, 1.0])
    for q in range(Q):
        for l, L in enumerate(lists):
            w = width(L)
            L.cnt[q] = [w, w + 7, w // 2, w, -3, w, 0, w, w][(q + l) % 9]
            if q in (2, 5):                     # the queries without records
                L.cnt[q] = 0 if l % 2 else -1
    for q in (0, 3, 7):
        lists[1].item[q, 5] = -1
        lists[2].item[q, 9] = n_ids
        lists[3].item[q, 11] = lists[3].item[q, 2]          # twice in one list
        lists[4].item[q, 1000] = lists[4].item[q, 0]
        lists[4].item[q, 17] = 2 ** 31 - 1
    return Case(lists, n_ids, RRF, 1.0)


def sixteen():
    """16 lists of width 128: the sum of the widths is exactly BLOCK_RECORDS; few ids, so an id is in most lists"""
    rng = np.random.RandomState(16)
    Q, n_ids = 4, 200
    lists = _perm_lists(rng, Q, n_ids, [128] * 16, weights=[1.0 + 0.125 * l for l in range(16)])
    lists[7].cnt[1] = 0
    return Case(lists, n_ids, MEAN, 0.0)


CAND_COUNTS = [0, 1, 9, 10, 11, 255, 256, 257, 258, 1023, 1024]


def one():
    """one list of width 1 024 whose counts put the candidates below, at and above every n_top of N_TOPS"""
    rng = np.random.RandomState(17)
    Q, n_ids = len(CAND_COUNTS), 3000
    lists = _perm_lists(rng, Q, n_ids, [1024])
    lists[0].cnt[:] = CAND_COUNTS
    return Case(lists, n_ids, SUM, 0.0)


FAMILIES = {"ties": ties, "order": order, "generic": generic, "special": special, "shapes": shapes, "sixteen": sixteen, "one": one}
N_TOPS = [1, 10, 256, 257, 1024]
# the calls of a family: (how, min_lists, n_top)
CALLS = {
    "ties": [(RRF, 1, 63), (RRF, 2, 1), (RRF, 1, 257)],
    "order": [(SUM, 1, 10), (SUM, 3, 1), (MEAN, 2, 256)],
    "generic": [(RRF, 1, 10), (RRF, 2, 257), (RRF, 5, 1024), (SUM, 3, 1), (MEAN, 1, 256)],
    "special": [(SUM, 1, 10), (MEAN, 1, 256), (MEAN, 2, 1), (SUM, 3, 1024), (RRF, 1, 257)],
    "shapes": [(RRF, 1, 1024), (RRF, 2, 10), (SUM, 1, 257), (MEAN, 5, 1), (RRF, 1, 256)],
    "sixteen": [(MEAN, 1, 256), (RRF, 16, 10), (SUM, 2, 1024), (RRF, 1, 1), (MEAN, 16, 257)],
    "one": [(SUM, 1, n) for n in N_TOPS] + [(RRF, 1, 256), (MEAN, 1, 257)],
}
