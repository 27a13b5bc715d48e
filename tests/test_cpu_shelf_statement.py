"""The statement of the shelves (tests/shelf_statement.py) against the statement of the filtered top-N it is defined by
(tests/filter_statement.py), and the census of the designed segments the device tests drive.  NumPy only, no device."""
import numpy as np

import shelf_statement as ss
from filter_statement import expected_filtered
from shelf_statement import BEST, LABEL, MEAN, Labels, check_tables, expected_shelf_segments, expected_shelves


def _random_scored(seed, U, I):
    """{user: [(item, plain, decayed, now, held)*]} in ascending item, tie-prone scores, a few status-2 candidates (plain None,
    or now beyond the table)"""
    rng = np.random.default_rng(seed)
    scored = {}
    for u in range(U):
        items = np.sort(rng.choice(I, size=int(rng.integers(0, 60)), replace=False))
        rows = []
        for i in items.tolist():
            p, d = float(np.round(rng.normal(), 1) + 0.0), float(np.round(rng.normal(), 1) + 0.0)
            kind = rng.integers(0, 20)
            rows.append((i, None if kind == 0 else p, None if kind == 0 else d, 80 if kind == 1 else int(rng.integers(2, 9)),
                         bool(rng.integers(0, 4) == 0)))
        scored[u] = rows
    return scored


def _random_labels(seed, I, n_labels):
    rng = np.random.default_rng(seed)
    return Labels.of([sorted(rng.choice(n_labels, size=int(rng.integers(0, 4)), replace=False).tolist()) for _ in range(I)], n_labels)


def test_a_shelf_is_the_filtered_list_under_the_labels_mask():
    U, I, n_labels, n_w = 25, 120, 9, 66
    scored, labels = _random_scored(3, U, I), _random_labels(4, I, n_labels)
    rng = np.random.default_rng(5)
    queries = list(range(U)) + [3, 3, -1, U + 2]
    allow = rng.integers(0, 5, I) > 0
    exclude = [rng.integers(-1, I + 1, int(rng.integers(0, 6))).tolist() for _ in queries]
    seen = 0
    for keep in (False, True):
        for rank_by in (0, 1):
            for n_top in (1, 5, 64):
                for min_score in (None, -0.4):
                    kw = dict(allow=allow, exclude=exclude, min_score=min_score)
                    pages, stats = expected_shelves(scored, queries, labels, n_labels, n_top, rank_by, LABEL, 1, keep, n_w, **kw)
                    ref6 = expected_filtered(scored, queries, n_top, rank_by, keep, n_w, I, **kw)[1]
                    assert stats[:6] == tuple(ref6)
                    by_label = [{s[0]: s for s in p} for p in pages]
                    for l in range(n_labels):
                        mask = allow & labels.carries(l)
                        lists = expected_filtered(scored, queries, n_top, rank_by, keep, n_w, I, allow=mask, exclude=exclude,
                                                  min_score=min_score)[0]
                        whole = expected_filtered(scored, queries, I, rank_by, keep, n_w, I, allow=mask, exclude=exclude,
                                                  min_score=min_score)[0]
                        for q in range(len(queries)):
                            if not lists[q]:
                                assert l not in by_label[q]
                                continue
                            s = by_label[q][l]
                            assert s[3] == lists[q] and s[2] == len(whole[q]) and s[1] == lists[q][0][1 + rank_by]
                            seen += 1
    assert seen > 1000          # (shelves compared: the loop is not vacuous)


def test_one_label_on_every_item_and_one_shelf_is_the_filtered_list():
    U, I, n_w = 25, 120, 66
    scored = _random_scored(7, U, I)
    labels = Labels.of([[0]] * I, 1)
    queries = list(range(U)) + [0, -5]
    rng = np.random.default_rng(8)
    allow = rng.integers(0, 3, I) > 0
    exclude = [rng.integers(0, I, 4).tolist() for _ in queries]
    for keep in (False, True):
        for rank_by in (0, 1):
            for n_top in (1, 10, 64):
                for shelf_by in (BEST, MEAN, LABEL):
                    kw = dict(allow=allow, exclude=exclude, min_score=-0.3)
                    pages, stats = expected_shelves(scored, queries, labels, 1, n_top, rank_by, shelf_by, 1, keep, n_w, **kw)
                    lists, ref6 = expected_filtered(scored, queries, n_top, rank_by, keep, n_w, I, **kw)
                    whole = expected_filtered(scored, queries, I, rank_by, keep, n_w, I, **kw)[0]
                    assert stats[:6] == tuple(ref6)
                    assert [([] if not p else p[0][3]) for p in pages] == lists
                    assert [(0 if not p else p[0][2]) for p in pages] == [len(w) for w in whole]
                    assert stats[6] == sum(len(w) for w in whole) and stats[7] == sum(bool(w) for w in whole) and stats[8] == 0
                    assert stats[9] == 1


def test_the_mean_is_summed_in_rank_order_from_the_first_entry():
    labels = Labels.of([[0]] * 3, 1)
    seg = [[(0, 1e300, 0.0, 0), (1, 1.0, 0.0, 0), (2, -1e300, 0.0, 0)]]
    page = expected_shelf_segments(seg, labels, 1, 3, 0, MEAN, 1)[0][0]
    assert page[0][1] == ((1e300 + 1.0) + -1e300) / 3.0 == 0.0 and page[0][2] == 3
    assert expected_shelf_segments(seg, labels, 1, 2, 0, MEAN, 1)[0][0][0][1] == (1e300 + 1.0) / 2.0


def test_the_rules_of_a_label_table():
    assert check_tables(3, 4, [0, 2, 2, 3], [1, 3, 0]) is None
    assert check_tables(3, 4, [1, 2, 2, 3], [1, 3, 0]) == ("lab_ptr", 0)
    assert check_tables(3, 4, [0, 2, 1, 3], [1, 3, 0]) == ("lab_ptr", 2)
    assert check_tables(3, 4, [0, 2, 2, 3], [1, 4, 0]) == ("range", 1)
    assert check_tables(3, 4, [0, 2, 2, 3], [1, 3, -1]) == ("range", 2)
    assert check_tables(3, 4, [0, 2, 2, 3], [1, 1, 0]) == ("ascending", 1)
    assert check_tables(3, 4, [0, 2, 2, 3], [3, 1, 0]) == ("ascending", 1)
    assert check_tables(3, 4, [0, 1, 2, 3], [3, 1, 0]) is None       # descending across items is no fault


def test_the_census_of_the_designed_segments():
    """conditions, asserted so that a later edit of a builder cannot empty a class"""
    segments, labels = ss.designed()
    allow = ss.designed_allow()
    cz = ss.census(segments, labels, n_top=10, n_shelf=3, min_fill=2, floor=-0.5, lab_allow=allow)
    print(cz)
    assert 40 <= cz["queries"] <= 200 and cz["candidates"] <= 2000
    assert cz["sizes"] == [1, 2, 9, 10, 11, 62, 63, 64, 65, 129]
    assert all(cz["cut_ties"][n] >= 1 for n in (1, 10, 63, 64)) and cz["zero_ties"] >= 2
    assert cz["shelf_ties_best"] >= 2 and cz["shelf_ties_mean"] >= 2 and cz["best_mean_differ"] >= 1
    assert cz["small_first"] >= 1 and cz["item_on_3"] >= 1
    assert all(cz["more_than_n_shelf"][ns] >= 1 for ns in (1, 3, 64)) and cz["fewer_than_n_shelf"] >= 1
    assert cz["no_shelf_with_candidates"] >= 1 and cz["no_candidates"] >= 1 and cz["labels_without_item"] >= 1
    assert cz["allow_takes_best"] >= 1 and cz["allow_leaves_none"] >= 1
    assert cz["huge"] >= 2 and cz["subnormal"] >= 2
    assert all(v >= 1 for v in cz["inside_runs"].values())
    for mr in (1, 7, 64):
        assert cz["chunks"][mr]["boundaries"] >= 1 and cz["chunks"][mr]["above"] >= 1
    assert cz["chunks"][7]["shared"] >= 1 and cz["chunks"][64]["shared"] >= 1
    # the planted pages, by hand
    pages = expected_shelf_segments(segments, labels, 3, 10, 0, BEST, 1)[0]
    assert [s[0] for s in pages[5]] == [30, 31, 32] and [s[0] for s in pages[6]] == [40, 41]
    assert [s[0] for s in pages[7]] == [1, 4, 2]
    assert [s[0] for s in expected_shelf_segments(segments, labels, 3, 10, 0, MEAN, 1)[0][7]] == [2, 4, 1]
    assert pages[8][0][0] == 50 and expected_shelf_segments(segments, labels, 3, 10, 0, BEST, 2)[0][8][0][0] == 2
    assert pages[11][0][0] == 31 and expected_shelf_segments(segments, labels, 3, 10, 0, BEST, 1, lab_allow=allow)[0][11][0][0] == 32
    # the -0.0 / 0.0 pair at the tenth place of the shelf of 11: the lower item index wins, whatever its sign
    shelf = [s for s in expected_shelf_segments(segments, labels, 64, 10, 0, LABEL, 1)[0][0] if s[0] == 3][0]
    last = shelf[3][-1]
    assert shelf[2] == 11 and last[1] == 0.0 and np.signbit(last[1])
    both = sorted(c[0] for c in segments[0] if c[1] == 0.0 and 3 in labels.carried(c[0]))
    assert len(both) == 2 and last[0] == both[0]
