"""The brute-force statement of the shelves (xmap_shelf_segments / xmap_shelf_rows, include/xmap_hip.h): per query a top-N per
label of the items and the best shelves of the page.  NumPy / Python only, no device.

  expected_shelf_segments : over scored segments [[(item, plain, decayed, status)*]*]
  expected_shelves        : over test_gpu_topn.score_users' {user: [(item, plain, decayed, now, held)*]}: the kept candidates are what
                            filter_statement.expected_filtered keeps (its rule order, its stats; the scoring is not restated here)
  check_tables            : the rules of a label table
  designed()              : the designed segments of the device tests, census() what they are meant to hold

A page is [(label, shelf score, size, [(item, plain, decayed)*])*]; to_arrays() lays pages out as the eight output arrays."""
import numpy as np

from filter_statement import allowed, expected_filtered

BEST, MEAN, LABEL = 0, 1, 2
SHELF_BY = {"best": BEST, "mean": MEAN, "label": LABEL}
MAX_LABELS = 1 << 24


class Labels(object):
    """a label table: CSR over n_items items, ids in [0, n_labels)"""

    def __init__(self, n_items, n_labels, lab_ptr, lab_id):
        self.n_items, self.n_labels = int(n_items), int(n_labels)
        self.ptr, self.id = np.asarray(lab_ptr, np.int64), np.asarray(lab_id, np.int32)

    @classmethod
    def of(cls, per_item, n_labels):
        """per_item: one sequence of label ids per item, taken as it stands (no sorting: check_tables is the judge)"""
        ptr = np.concatenate([[0], np.cumsum([len(l) for l in per_item])]).astype(np.int64)
        return cls(len(per_item), n_labels, ptr, np.asarray([x for l in per_item for x in l], np.int32))

    def carried(self, item):
        if not 0 <= item < self.n_items:
            return []
        return self.id[self.ptr[item]:self.ptr[item + 1]].tolist()

    def carries(self, label):
        """bool [n_items]: the items that carry `label`"""
        out = np.zeros(self.n_items, bool)
        for i in range(self.n_items):
            out[i] = label in self.carried(i)
        return out


def check_tables(n_items, n_labels, lab_ptr, lab_id):
    """None for a good table, else (rule, first offending index) in the order the library reports: 'lab_ptr' (lab_ptr[0] != 0 or a
    decrease; index into lab_ptr), 'range' (an id outside [0, n_labels); index into lab_id), 'ascending' (an id not above the one
    in front of it inside one item)"""
    ptr = [int(x) for x in lab_ptr]
    assert len(ptr) == n_items + 1
    bad = [k for k in range(n_items + 1) if (ptr[0] != 0 if k == 0 else ptr[k] < ptr[k - 1])]
    if bad:
        return "lab_ptr", bad[0]
    ids = [int(x) for x in lab_id[:ptr[-1]]]
    out = [k for k, l in enumerate(ids) if not 0 <= l < n_labels]
    if out:
        return "range", out[0]
    for i in range(n_items):
        for k in range(ptr[i] + 1, ptr[i + 1]):
            if ids[k] <= ids[k - 1]:
                return "ascending", k
    return None


def shelf_score(entries, rank_by, shelf_by):
    s = [e[1 + rank_by] for e in entries]
    if shelf_by != MEAN:
        return s[0]
    acc = s[0]
    for x in s[1:]:
        acc = acc + x
    return acc / float(len(s))


def page_of(kept, labels, n_shelf, n_top, rank_by, shelf_by, min_fill, lab_ok):
    """kept: the kept candidates of one query [(item, plain, decayed)*] -> (page, all formed shelves in page order, records, shelves,
    shelves below min_fill)"""
    members = {}
    records = 0
    for c in kept:
        for l in labels.carried(c[0]):
            if lab_ok[l]:
                members.setdefault(l, []).append(c)
                records += 1
    formed, small = [], 0
    for l, m in members.items():
        if len(m) < min_fill:
            small += 1
            continue
        m = sorted(m, key=lambda c: (- c[1 + rank_by], c[0]))
        entries = [(c[0], c[1], c[2]) for c in m[:n_top]]
        formed.append((l, shelf_score(entries, rank_by, shelf_by), len(m), entries))
    formed.sort(key=(lambda s: s[0]) if shelf_by == LABEL else (lambda s: (- s[1], s[0])))
    return formed[:n_shelf], formed, records, len(members), small


def expected_shelf_segments(segments, labels, n_shelf, n_top, rank_by, shelf_by, min_fill, min_score=None, lab_allow=None, full=None):
    """(pages, stats [4]) of the segments [[(item, plain, decayed, status)*]*]; full (a list, or None) takes every query's formed
    shelves in page order, uncut"""
    assert 1 <= n_shelf <= 64 and 1 <= n_top <= 64 and rank_by in (0, 1) and shelf_by in (BEST, MEAN, LABEL) and min_fill >= 1
    assert check_tables(labels.n_items, labels.n_labels, labels.ptr, labels.id) is None
    lab_ok = allowed(lab_allow, labels.n_labels)
    floor = -np.inf if min_score is None else float(min_score)
    pages, tot = [], [0, 0, 0, 0]
    for seg in segments:
        assert [c[0] for c in seg] == sorted({c[0] for c in seg})      # ascending, each once
        kept = [(c[0], c[1], c[2]) for c in seg if c[3] == 0 and c[1 + rank_by] >= floor]
        page, formed, records, shelves, small = page_of(kept, labels, n_shelf, n_top, rank_by, shelf_by, min_fill, lab_ok)
        pages.append(page)
        if full is not None:
            full.append(formed)
        tot = [tot[0] + records, tot[1] + shelves, tot[2] + small, max(tot[3], len(formed))]
    return pages, tuple(tot)


def expected_shelves(scored, queries, labels, n_shelf, n_top, rank_by, shelf_by, min_fill, keep, n_w, lab_allow=None, allow=None,
                     exclude=None, min_score=None):
    """(pages, stats [10]) of the query users: the kept candidates are expected_filtered's with no cut"""
    n_ids = labels.n_items
    lists, stats6 = expected_filtered(scored, queries, max(n_ids, 1), rank_by, keep, n_w, n_ids, allow=allow, exclude=exclude,
                                      min_score=min_score)
    segments = [sorted((c[0], c[1], c[2], 0) for c in l) for l in lists]
    pages, stats4 = expected_shelf_segments(segments, labels, n_shelf, n_top, rank_by, shelf_by, min_fill, lab_allow=lab_allow)
    return pages, tuple(stats6) + tuple(stats4)


def to_arrays(pages, n_shelf, n_top):
    """(nshelf [Q], label, sscore, size, cnt [Q][n_shelf], item, plain, decayed [Q][n_shelf][n_top]) with the padding of the header"""
    Q = len(pages)
    nshelf = np.zeros(Q, np.int32)
    label = np.full((Q, n_shelf), -1, np.int32)
    sscore = np.zeros((Q, n_shelf))
    size, cnt = np.zeros((Q, n_shelf), np.int32), np.zeros((Q, n_shelf), np.int32)
    item = np.full((Q, n_shelf, n_top), -1, np.int32)
    plain, decay = np.zeros((Q, n_shelf, n_top)), np.zeros((Q, n_shelf, n_top))
    for q, page in enumerate(pages):
        nshelf[q] = len(page)
        for s, (l, sc, sz, entries) in enumerate(page):
            label[q, s], sscore[q, s], size[q, s], cnt[q, s] = l, sc, sz, len(entries)
            for j, e in enumerate(entries):
                item[q, s, j], plain[q, s, j], decay[q, s, j] = e
    return nshelf, label, sscore, size, cnt, item, plain, decay


NAMES = ("nshelf", "label", "sscore", "size", "cnt", "item", "plain", "decay")


def check_shelf_output(got, pages, n_shelf, n_top):
    """the eight arrays byte for byte (integers with array_equal, doubles through uint64 views)"""
    want = to_arrays(pages, n_shelf, n_top)
    for name, g, w in zip(NAMES, got, want):
        g = np.asarray(g).reshape(w.shape)
        if w.dtype == np.float64:
            g, w = np.ascontiguousarray(g, np.float64).view(np.uint64), w.view(np.uint64)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0].tolist()
            raise AssertionError("%s differs first at %s: got %r, statement %r" % (name, at, g[tuple(at)], w[tuple(at)]))


# ------------------------------------------------------------------------------------------------- the designed segments
N_LABELS = 80           # 0 .. 9 the size labels, 10 .. 22 the multi-label region, 0 .. 78 one item each (700 + k), 79: no item
SIZES = ((0, 1), (1, 9), (2, 10), (3, 11), (4, 62), (5, 63), (6, 64), (7, 65), (8, 129), (9, 2))
N_SIZED = sum(n for _, n in SIZES)      # 416
TRIPLE = range(516, 541)                # items on four labels
LONE = 700                              # item LONE + k carries label k alone, k < 79
N_ITEMS = LONE + 79
LAB_DENIED = (0, 8, 11, 31, 50)         # the labels the designed lab_allow takes out


def designed_labels(seed=11):
    rng = np.random.default_rng(seed)
    sized = rng.permutation(np.repeat([l for l, _ in SIZES], [n for _, n in SIZES])).tolist()
    per = [[l] for l in sized]
    for i in range(N_SIZED, 516):       # 0 .. 4 labels of 10 .. 22
        per.append(sorted(rng.choice(np.arange(10, 23), size=int(rng.integers(0, 5)), replace=False).tolist()))
    per += [[10, 11, 12, 13] for _ in TRIPLE]
    for i in range(541, LONE):          # one label of 0 .. 77, every third item the next label too
        l = int(rng.integers(0, 78))
        per.append([l, l + 1] if i % 3 == 0 else [l])
    per += [[k] for k in range(79)]
    assert len(per) == N_ITEMS
    return Labels.of(per, N_LABELS)


def designed_allow():
    on = np.ones(N_LABELS, bool)
    on[list(LAB_DENIED)] = False
    return on


def designed(seed=11):
    """(segments, labels): 60 queries, fewer than 2 000 candidates; what each is for stands beside it, census() counts it"""
    rng = np.random.default_rng(seed + 1)
    labels = designed_labels(seed)
    with_label = {l: [i for i in range(N_SIZED) if labels.carried(i) == [l]] for l, _ in SIZES}
    tie_prone = lambda n: np.round(rng.normal(size=n), 1) + 0.0

    def seg(items, plain, decay=None, status=None):
        items = list(items)
        decay = tie_prone(len(items)) if decay is None else decay
        status = [0] * len(items) if status is None else status
        o = np.argsort(items, kind="stable")
        return [(int(items[k]), float(plain[k]), float(decay[k]), int(status[k])) for k in o]

    segments = []
    # 0: every sized shelf (1, 9, 10, 11, 62, 63, 64, 65, 129, 2 members), the two last places of the shelves of 11, 64, 65 and 2
    #    members tied (a cut at n_top = 10, 63, 64, 1 falls between them): -0.0 / 0.0 in both orders, and ordinary numbers
    score = {}
    for l, n in SIZES:
        its = with_label[l]
        vals = 1.0 + rng.permutation(n) / 4.0           # distinct, above every tie value
        for i, v in zip(its, vals):
            score[i] = float(v)
        low = sorted(its, key=lambda i: score[i])[:2]
        pair = {3: (-0.0, 0.0), 6: (0.0, -0.0), 7: (0.5, 0.5), 9: (0.25, 0.25)}.get(l)
        if pair:
            score[min(low)], score[max(low)] = pair
    items = list(range(N_SIZED))
    segments.append(seg(items, [score[i] for i in items]))
    # 1: the same items with status 1 / 2 inside every run and tie-prone scores on both sides of a floor
    segments.append(seg(items, tie_prone(N_SIZED), status=rng.choice([0, 0, 0, 1, 2], N_SIZED).tolist()))
    # 2: no candidates
    segments.append([])
    # 3: the items on four labels: one item on several returned shelves
    its = list(TRIPLE)[:6]
    segments.append(seg(its, tie_prone(len(its))))
    # 4: one item per label, 79 shelves of one member: more formed shelves than any n_shelf
    its = [LONE + k for k in range(79)]
    segments.append(seg(its, tie_prone(79)))
    # 5: equal shelf scores at the third place (labels 31, 32, 33 behind 30), 6: at the first (labels 40, 41)
    segments.append(seg([LONE + 30, LONE + 31, LONE + 32, LONE + 33], [9.0, 7.0, 7.0, 7.0]))
    segments.append(seg([LONE + 40, LONE + 41], [5.0, 5.0]))
    a, b, c = with_label[1][:3], with_label[2][:3], with_label[4][:3]
    # 7: BEST puts label 1 first (10 > 5), MEAN label 2 (5 > 10 / 3); label 4 ties label 2 under MEAN ((6 + 5) + 4) / 3 = 5
    segments.append(seg(a + b + c, [10.0, 0.0, 0.0, 5.0, 5.0, 5.0, 6.0, 5.0, 4.0]))
    # 8: a shelf of one member whose score ranks first: not formed under min_fill = 2
    segments.append(seg([LONE + 50] + b, [100.0, 1.0, 2.0, 3.0]))
    # 9: candidates without a label; 10: candidates whose labels the designed lab_allow denies
    bare = [i for i in range(N_SIZED, 516) if not labels.carried(i)]
    assert len(bare) >= 3
    segments.append(seg(bare, tie_prone(len(bare))))
    segments.append(seg([LONE + l for l in LAB_DENIED], tie_prone(len(LAB_DENIED))))
    # 11: the best shelf carries a denied label (31)
    segments.append(seg([LONE + 31, LONE + 32, LONE + 33], [8.0, 2.0, 1.0]))
    # 12 .. 19: the multi-label region with scores at the ends of the range
    ends = [1e300, -1e300, 5e-324, -5e-324, 1e-310, -1e-310, 2.5e-308, 0.0, -0.0, 1.0]
    for k in range(8):
        its = rng.choice(np.arange(N_SIZED, LONE), size=22, replace=False)
        segments.append(seg(its, rng.choice(ends, 22), decay=rng.choice(ends, 22), status=rng.choice([0, 0, 0, 0, 2], 22).tolist()))
    # 20 .. 59: random queries of 0 .. 30 candidates over the whole item space, tie-prone scores
    while len(segments) < 60:
        n = int(rng.integers(0, 31))
        its = rng.choice(N_ITEMS + 5, size=n, replace=False)       # (a few items beyond the table: no label)
        segments.append(seg(its, tie_prone(n), status=rng.choice([0, 0, 0, 0, 1, 2], n).tolist()))
    assert sum(len(s) for s in segments) <= 2000
    return segments, labels


def chunks(records, max_records):
    """the chunks [q0, q1) of consecutive queries with at most max_records records, or one query"""
    out, q0, Q = [], 0, len(records)
    while q0 < Q:
        q1 = q0 + 1
        while q1 < Q and sum(records[q0:q1 + 1]) <= max_records:
            q1 += 1
        out.append((q0, q1))
        q0 = q1
    return out


def census(segments, labels, n_top=10, n_shelf=3, min_fill=2, floor=-0.5, lab_allow=None):
    """counts of what the designed segments are meant to hold, at the nominal parameters"""
    cz = {}
    full = []
    expected_shelf_segments(segments, labels, 64, 64, 0, BEST, 1, full=full)
    sizes = {s[2] for f in full for s in f}
    cz["sizes"] = sorted(sizes & {1, 2, n_top - 1, n_top, n_top + 1, 62, 63, 64, 65, 129})
    # ties at the cut: the n-th and the (n + 1)-th member of a shelf have equal scores, for the n_top the device tests use
    lab_ok = np.ones(labels.n_labels, bool)
    cz["cut_ties"], cz["zero_ties"] = {}, 0
    for n in (1, 10, 63, 64):
        k = 0
        for seg in segments:
            kept = [(c[0], c[1], c[2]) for c in seg if c[3] == 0]
            for s in page_of(kept, labels, 64, 64, 0, BEST, n + 1, lab_ok)[1]:
                m = sorted((c for c in kept if s[0] in labels.carried(c[0])), key=lambda c: (- c[1], c[0]))
                if m[n - 1][1] == m[n][1]:
                    k += 1
                    cz["zero_ties"] += np.signbit(m[n - 1][1]) != np.signbit(m[n][1])
        cz["cut_ties"][n] = k
    # shelves tied at the n_shelf-th place
    for name, by in (("best", BEST), ("mean", MEAN)):
        f = []
        expected_shelf_segments(segments, labels, 64, n_top, 0, by, 1, full=f)
        cz["shelf_ties_" + name] = sum(len(p) > ns and p[ns - 1][1] == p[ns][1] for p in f for ns in (1, n_shelf))
    fb, fm = [], []
    expected_shelf_segments(segments, labels, 64, n_top, 0, BEST, 1, full=fb)
    expected_shelf_segments(segments, labels, 64, n_top, 0, MEAN, 1, full=fm)
    cz["best_mean_differ"] = sum([s[0] for s in a] != [s[0] for s in b] for a, b in zip(fb, fm))
    # a shelf below min_fill that would have ranked first
    cz["small_first"] = sum(bool(a) and a[0][2] < min_fill for a in fb)
    # an item on three returned shelves of one page
    pages = expected_shelf_segments(segments, labels, n_shelf, n_top, 0, BEST, 1)[0]
    cz["item_on_3"] = sum(any(sum(i in [e[0] for e in s[3]] for s in p) >= 3 for i in {e[0] for s in p for e in s[3]}) for p in pages)
    cz["more_than_n_shelf"] = {ns: sum(len(f) > ns for f in fb) for ns in (1, 3, 64)}
    cz["fewer_than_n_shelf"] = sum(0 < len(f) < n_shelf for f in fb)
    cz["no_shelf_with_candidates"] = sum(not f and bool(seg) for f, seg in zip(fb, segments))
    cz["no_candidates"] = sum(not seg for seg in segments)
    carried = set(labels.id.tolist())
    cz["labels_without_item"] = labels.n_labels - len(carried)
    if lab_allow is not None:
        fa = []
        expected_shelf_segments(segments, labels, 64, n_top, 0, BEST, 1, lab_allow=lab_allow, full=fa)
        cz["allow_takes_best"] = sum(bool(a) and not lab_allow[a[0][0]] for a in fb)
        cz["allow_leaves_none"] = sum(bool(a) and not b for a, b in zip(fb, fa))
    vals = [abs(c[1]) for seg in segments for c in seg if c[3] == 0]
    cz["huge"], cz["subnormal"] = sum(v >= 1e300 for v in vals), sum(0 < v < 2.2250738585072014e-308 for v in vals)
    # status 1 / 2 and below-floor candidates INSIDE a run: between two kept members of one shelf
    inside = dict(status1=0, status2=0, floored=0)
    for seg in segments:
        for l in {x for c in seg for x in labels.carried(c[0])}:
            m = [c for c in seg if l in labels.carried(c[0])]
            keep = [c[3] == 0 and c[1] >= floor for c in m]
            if sum(keep) < 2:
                continue
            lo, hi = keep.index(True), len(keep) - 1 - keep[::-1].index(True)
            for c in m[lo:hi + 1]:
                inside["status1"] += c[3] == 1
                inside["status2"] += c[3] == 2
                inside["floored"] += c[3] == 0 and c[1] < floor
    cz["inside_runs"] = inside
    # chunking
    per_q = []
    for seg in segments:
        kept = [(c[0], c[1], c[2]) for c in seg if c[3] == 0]
        per_q.append(page_of(kept, labels, 64, 64, 0, BEST, 1, lab_ok)[2])
    cz["records"] = sum(per_q)
    cz["chunks"] = {}
    for mr in (1, 7, 64):
        ch = chunks(per_q, mr)
        cz["chunks"][mr] = dict(chunks=len(ch), shared=sum(sum(per_q[q] > 0 for q in range(a, b)) >= 2 for a, b in ch),
                                boundaries=sum(1 for (a, b), (c, d) in zip(ch, ch[1:]) if sum(per_q[a:b]) and sum(per_q[c:d])),
                                above=sum(b - a == 1 and per_q[a] > mr for a, b in ch))
    cz["queries"], cz["candidates"] = len(segments), sum(len(s) for s in segments)
    return cz
