"""The statement of diversified top-N (tests/diversify_statement.py) against itself, and the condition that keeps
tests/test_gpu_diversify.py from being vacuous: on the random family the re-ranking changes most lists and lowers the intra-list
similarity, by the statement alone.  No device."""
import numpy as np

import diversify_statement as ds


def _family():
    f = getattr(_family, "f", None)
    if f is None:
        row_ptr, col, sim, dense, cnt, item, plain, decay = ds.random_family()
        dv_col, dv_abs, dups = ds.div_index(row_ptr, col, sim)
        assert dups == 0
        f = _family.f = dict(I=400, row_ptr=row_ptr, col=col, sim=sim, dense=dense, pool=(cnt, item, plain, decay), dv=(dv_col, dv_abs),
                             by_w={w: ds.rerank(cnt, item, plain, decay, 0, w, 10, 400, row_ptr, dv_col, dv_abs) for w in (0.0, 0.5, 2.0)})
    return f


def test_weight_zero_gives_the_pool_prefix():
    f = _family()
    cnt, item, plain, decay = f["pool"]
    o_cnt, o_item, o_plain, o_decay, o_pos, o_pen, o_ils, stats = f["by_w"][0.0]
    assert np.array_equal(o_cnt, np.minimum(cnt, 10)) and stats == (0, int(o_cnt.sum()))
    for q in range(len(cnt)):
        n = o_cnt[q]
        assert np.array_equal(o_item[q, :n], item[q, :n]) and np.array_equal(o_pos[q, :n], np.arange(n))
        assert np.array_equal(ds.bits(o_plain[q, :n]), ds.bits(plain[q, :n])) and np.array_equal(ds.bits(o_decay[q, :n]), ds.bits(decay[q, :n]))
        assert np.all(o_item[q, n:] == -1) and np.all(o_pos[q, n:] == -1) and not o_plain[q, n:].any() and not o_pen[q, n:].any()


def test_the_index_is_invariant_under_the_order_inside_the_rows():
    f = _family()
    rng = np.random.default_rng(3)
    for how in ("shuffle", "asc", "desc"):
        col, sim = ds.shuffle_rows(rng, f["row_ptr"], f["col"], f["sim"], how)
        dv_col, dv_abs, dups = ds.div_index(f["row_ptr"], col, sim)
        assert dups == 0 and np.array_equal(dv_col, f["dv"][0]) and np.array_equal(ds.bits(dv_abs), ds.bits(f["dv"][1]))
    rp, c, s = ds.csr_of({0: [(2, 0.5), (1, -0.25), (2, 0.125)], 2: [(0, 1.0)]}, 3)
    assert ds.div_index(rp, c, s)[2] == 1           # a repeated (row, column) is counted


def test_ils_is_the_mean_pairwise_similarity_of_the_returned_items():
    f = _family()
    for w in (0.0, 0.5, 2.0):
        o_cnt, o_item, _, _, _, o_pen, o_ils, _ = f["by_w"][w]
        for q in range(len(o_cnt)):
            ids = o_item[q, :o_cnt[q]]
            sub = f["dense"][np.ix_(ids, ids)]
            want = np.triu(sub, 1).sum() / (len(ids) * (len(ids) - 1) / 2) if len(ids) >= 2 else 0.0
            assert np.isclose(o_ils[q], want, rtol=1e-12, atol=0.0)
            for r in range(o_cnt[q]):           # the penalty of a pick is its largest |sim| to the picks before it
                assert o_pen[q, r] == (sub[r, :r].max() if r else 0.0)


def test_the_random_family_is_not_vacuous():
    f = _family()
    n_query = len(f["pool"][0])
    for w in (0.5, 2.0):
        assert f["by_w"][w][7][0] * 2 >= n_query, (w, f["by_w"][w][7])
    ils = {w: float(f["by_w"][w][6].mean()) for w in (0.0, 2.0)}
    assert ils[2.0] < ils[0.0], ils
