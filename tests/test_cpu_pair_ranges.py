"""The conditions the tests at the launch limit (test_gpu_pair_ranges.py) put on their input, checked without a GPU: the sizes
cross the limit, the closed form of pair_range_statement.py is exact and free of ties, and on a shrunk model it equals the
project's brute-force statements of the prediction, the top-N lists and the audiences."""
from fractions import Fraction

import numpy as np

import pair_range_statement as prs
from test_gpu_audience import statement as audience_statement
from test_gpu_explain import explain_pair
from test_gpu_topn import _tool, expected, score_users


def test_the_sizes_cross_the_limit():
    assert (prs.THREADS_LIMIT_PAIRS + 3) // 4 * 256 >= 2 ** 32 > (prs.THREADS_LIMIT_PAIRS - 1 + 3) // 4 * 256
    assert prs.Q * prs.U >= prs.THREADS_LIMIT_PAIRS
    assert prs.N_PAIRS_A >= prs.THREADS_LIMIT_PAIRS + 4099 and prs.N_PAIRS_A % 4 != 0
    assert (prs.EXPLAIN_LIMIT_PAIRS * 16 + 3) // 4 * 256 >= 2 ** 32 > ((prs.EXPLAIN_LIMIT_PAIRS - 1) * 16 + 3) // 4 * 256
    assert prs.N_PAIRS_D > prs.EXPLAIN_LIMIT_PAIRS and prs.N_W >= 301 == max(prs.LONG) + 1


def test_the_model_is_what_the_closed_form_assumes():
    M = prs.model()
    ptr, item, rating, time, cnt, col, sim, avg = M["arrays"]
    U, Q, I = prs.U, prs.Q, M["n_items"]
    assert M["n_users"] == U + 3 and I == Q + 2 and np.diff(ptr).tolist() == [1] * U + list(prs.LONG)
    assert not item.any() and cnt[0] == 0 and cnt[I - 1] == 0 and (cnt[1:Q + 1] == 1).all() and not col[1:Q + 1].any()
    assert sorted(prs.permutation(U).tolist()) == list(range(U))
    assert set(np.abs(sim[1:Q + 1, 0]).tolist()) == {0.5} and 0.3 < (sim[1:Q + 1, 0] > 0).mean() < 0.8
    assert avg[0] == 0 and len(set(avg[1:Q + 1].tolist())) == Q and not (avg[1:Q + 1] % 8).any() and (avg[1:Q + 1] == 0).sum() == 1
    assert (np.diff(avg[1:Q + 1]) < 0).any() and (np.diff(avg[1:Q + 1]) > 0).any()
    for k, (c, m) in enumerate(zip(prs.LONG, prs.LONG_MEAN)):
        a, b = int(ptr[U + k]), int(ptr[U + k + 1])
        assert b - a == c and len(set(time[a:b].tolist())) == c and (np.diff(time[a:b]) < 0).any()      # distinct times, not in row order
        assert not ((rating[a:b] * 16) % 1).any() and rating[a:b].min() >= 1.0 and len(set(rating[a:b].tolist())) > 8
        assert sum(Fraction(x) for x in rating[a:b].tolist()) / c == Fraction(m)


def test_every_score_is_exact_and_strictly_ordered():
    M = prs.model()
    avg, sign, R = M["arrays"][7], M["sign"], M["R"]
    Q = prs.Q
    # exactly representable: the fp64 closed form equals the rational one -- every R, and every average against the extreme R
    for u in list(range(0, prs.U, 997)) + [prs.U - 1, prs.U, prs.U + 1, prs.U + 2]:
        for q in (1, 2, 3, Q // 2, Q - 1, Q, int(np.argmax(avg)), int(np.argmin(avg[1:Q + 1])) + 1):
            exact = Fraction(float(avg[q])) + Fraction(float(sign[q])) * Fraction(float(R[u]))
            assert Fraction(float(avg[q] + sign[q] * R[u])) == exact
    assert not ((R * 2.0 ** 17) % 1).any() and R.min() >= 1.0 and R.max() < 4.0 and np.abs(avg).max() < 2.0 ** 12     # 30 bits at the most
    # the long users: the left-to-right sums of the kernel give avg + sign * mean, and nothing was rounded on the way
    ptr, _, rating, _, _, _, sim, _ = M["arrays"]
    for k in range(3):
        u = prs.U + k
        for q in (1, 2, 3, 4, 5, Q):
            plain, decayed, n = prs.loop_score(M, u, q)
            assert n == prs.LONG[k] and plain == decayed == avg[q] + sign[q] * R[u]
            e0 = [Fraction(float(sim[q, 0])) * Fraction(float(x)) for x in rating[ptr[u]:ptr[u + 1]].tolist()]
            assert Fraction(plain) == Fraction(float(avg[q])) + sum(e0) / (Fraction(1, 2) * n)
    for u in (0, 1, prs.U - 1):
        assert prs.loop_score(M, u, 7)[:2] == (avg[7] + sign[7] * R[u],) * 2
    # strictly ordered within a user (the averages are 8 apart, R below 4) and within an item (R is distinct)
    assert len(set(R.tolist())) == len(R)
    assert np.diff(np.sort(avg[1:Q + 1])).min() == 8.0 and 2 * R.max() < 8.0
    S = prs.closed_scores(M)[[0, 1, prs.U // 2, prs.U, prs.U + 2]][:, 1:Q + 1]
    assert (np.diff(np.sort(S, axis=1), axis=1) > 0).all()
    # the bounded predictions are mostly 0 and 5 (averages 8 apart); the item with the average 0 tells the users apart
    zero = int(np.nonzero(avg[1:Q + 1] == 0)[0][0]) + 1
    assert sign[zero] > 0 and sorted(set(prs.bound_rating(prs.closed_scores(M)[:, zero]).tolist())) == [1.0, 2.0, 3.0, 4.0]


def test_the_closed_form_equals_the_brute_force_statements_on_a_shrunk_model():
    M = prs.model(n_users=50, n_lists=7)
    arrays, n_all, I, keep = M["arrays"], M["n_users"], M["n_items"], 1
    ptr, pit, pra, pti, cnt, col, sim, avg = arrays
    S = prs.closed_scores(M)
    w = M["wtab"]
    # the prediction: every user against every item, + a user and an item out of range
    tool = _tool(0.0)
    for u in list(range(n_all)) + [-1, n_all]:
        for i in list(range(I)) + [-1, I]:
            st, n, score, _, now = explain_pair(u, i, ptr, pit.tolist(), pra.tolist(), pti.tolist(), cnt, col, sim, avg, keep, w, 1, 0)
            decayed = explain_pair(u, i, ptr, pit.tolist(), pra.tolist(), pti.tolist(), cnt, col, sim, avg, keep, w, 1, 1)[2]
            if not 1 <= i <= 7:
                assert (st, score) == (1, 0.0)
            elif not 0 <= u < n_all:
                assert (st, n, score, decayed) == (0, 0, avg[i], avg[i])
            else:
                assert (st, score, decayed) == (0, S[u, i], S[u, i]) and n == ptr[u + 1] - ptr[u] and now == n + 1
                assert prs.bound_rating(score) == tool.bound_rating(score)
    # top-N: the statement of test_gpu_topn.py
    users = list(range(n_all))
    scored = score_users(0.0, users, *arrays, keep)
    for n in (3, 10):
        lists, stats = expected(scored, users, n, 0, False, prs.N_W)
        items, scores = prs.closed_topn(M, users, n)
        assert stats[:3] == (7 * n_all, 0, 301)
        for q, l in enumerate(lists):
            k = min(n, 7)
            assert [c[0] for c in l] == items[q, :k].tolist() and [c[1] for c in l] == scores[q, :k].tolist()
            assert [c[2] for c in l] == scores[q, :k].tolist()
    # audiences: the statement of test_gpu_audience.py
    inv = audience_statement(arrays, keep, alpha=0.0)
    queries = list(range(1, 8))
    for n in (1, 10, 1000):
        lists, stats = expected(inv, queries, n, 1, False, prs.N_W)
        who, scores = prs.closed_audience(M, queries, n)
        assert stats[:3] == (7 * n_all, 0, 301)
        for q, l in enumerate(lists):
            k = min(n, n_all)
            assert [c[0] for c in l] == who[q, :k].tolist() and [c[2] for c in l] == scores[q, :k].tolist()
            best = np.argmax(M["R"]) if M["sign"][queries[q]] > 0 else np.argmin(M["R"])
            assert l[0][0] == best


def test_the_raw_profile_model_has_every_kind_of_row():
    ptr, pit, cnt_t, raw_ptr, raw_item, flags, m = prs.raw_profile_model(1000, 5)
    n, raw_n = np.diff(ptr), np.diff(raw_ptr)
    assert len(n) == 1000 and n.min() >= 0 and raw_n.max() > 64 and (raw_n <= 3).any()
    assert (cnt_t > 0).any() and (n > cnt_t).any() and (n == cnt_t).any() and (cnt_t > 64).sum() == 0
    for u in (0, 1, 2, 500, 999):                       # pass-through rows first, then one mapped row per target
        rows = pit[ptr[u]:ptr[u + 1]].tolist()
        raw = raw_item[raw_ptr[u]:raw_ptr[u + 1]].tolist()
        assert rows[:cnt_t[u]] == [x for x in raw if flags[x] & 2]
        assert sorted(rows[cnt_t[u]:]) == sorted({int(m[x]) for x in raw if m[x] >= 0})
