"""tests/related_statement.py against a second, independent formulation, and the census of the designed inputs -- asserted here, on
the CPU, so that tests/test_gpu_related.py cannot pass vacuously: an input that never ties at the cut, never re-sorts the
selection or never drops anything would prove nothing about the kernels."""
import math

import numpy as np
import pytest

import related_statement as rs
from related_statement import KEEP_MEMBERS, MAX, MEAN, SUM


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def designed():
    b_ptr, b_item, weights = rs.baskets()
    out = {}
    for f in rs.FAMILIES:
        M = rs.design(f)
        out[f] = (M, rs.raw_records(M, b_ptr, b_item), rs.raw_records(M, b_ptr, b_item, weights))
    return b_ptr, b_item, weights, out


def test_the_sum_equals_the_dense_product_on_dyadic_values(designed):
    """sums of k / 2^10 are exact, hence independent of order: the SUM score of every (basket, item) is, bit for bit, the product
    of the basket's indicator (a repeated member counts twice) with the dense matrix"""
    b_ptr, b_item, _, fam = designed
    M, raw, _ = fam["dyadic"]
    D = np.zeros((rs.N_ROWS, M.n_items))
    rows = np.repeat(np.arange(M.n_items), np.diff(M.row_ptr))
    np.add.at(D, (rows, M.col), M.sim)
    H = np.zeros((rs.N_ROWS, M.n_items), np.int64)
    np.add.at(H, (rows, M.col), 1)
    w = rs.related_statement(M, b_ptr, b_item, 16, SUM, KEEP_MEMBERS, raw=raw)
    seen = 0
    for q in range(len(b_ptr) - 1):
        x = np.zeros(rs.N_ROWS)
        for b in b_item[b_ptr[q]:b_ptr[q + 1]]:
            if 0 <= b < M.n_items:
                x[b] += 1.0
        dense, sup = x @ D, x.astype(np.int64) @ H
        scored = w[5]["scored"][q]
        assert sorted(scored) == np.nonzero(sup)[0].tolist()
        for it, (s, n) in scored.items():
            assert n == sup[it] and bits(s + 0.0) == bits(dense[it] + 0.0), (q, it)
        seen += len(scored)
    assert seen > 10000


def test_one_member_lists_the_row_in_selection_order(designed):
    """a single-member, unweighted basket over non-negative similarities: the list is the member's row sorted by (sim descending,
    column ascending) -- the order xmap_rec_select defines -- for a row without a self entry or a repeated column"""
    _, _, _, fam = designed
    M = fam["ties"][0]
    plain = rs.plain_rows(M)
    assert len(plain) > 200
    b_ptr = np.arange(len(plain) + 1, dtype=np.int64)
    w = rs.related_statement(M, b_ptr, np.asarray(plain, np.int32), 64)
    for q, i in enumerate(plain):
        c, s = M.col[M.row_ptr[i]:M.row_ptr[i + 1]], M.sim[M.row_ptr[i]:M.row_ptr[i + 1]]
        o = np.lexsort((c, -s))[:64]
        assert w[0][q] == len(o) and np.array_equal(w[1][q, :len(o)], c[o]) and np.array_equal(bits(w[2][q, :len(o)]), bits(s[o]))
        assert (w[3][q, :len(o)] == 1).all()


def test_the_census_of_the_designed_inputs(designed):
    b_ptr, b_item, weights, fam = designed
    allow, exclude, floor = rs.rules(b_ptr)
    n_q = len(b_ptr) - 1
    sizes = np.diff(b_ptr)
    assert {0, 1, 2, 64, 65} <= set(sizes.tolist())
    assert any(len(set(b_item[b_ptr[q]:b_ptr[q + 1]].tolist())) < sizes[q] for q in range(n_q))       # a repeated member
    assert ((b_item < 0) | (b_item >= rs.N_ITEMS)).sum() >= 5
    assert {0.0} < set(weights.tolist()) and (weights < 0).any() and any(w * 1024 != int(w * 1024) for w in weights.tolist())
    # the matrix: every length, a repeated column, a self entry
    M = fam["dyadic"][0]
    lens = set(np.diff(M.row_ptr).tolist())
    assert set(rs.LENGTHS) | {rs.BIG_LEN} <= lens
    dup = own = 0
    for i in range(rs.N_ROWS):
        c = M.col[M.row_ptr[i]:M.row_ptr[i + 1]].tolist()
        dup += len(set(c)) < len(c)
        own += i in c
    assert dup >= 50 and own >= 50
    # more candidates than the selection holds: it re-sorts
    w = rs.related_statement(M, b_ptr, b_item, 7, raw=fam["dyadic"][1])
    assert w[4][4] > 2048
    # the basket whose rows overlap: support up to the basket size
    assert max(n for _, n in w[5]["scored"][9].values()) >= 65
    big = rs.related_statement(M, b_ptr, b_item, 7, min_support=65, raw=fam["dyadic"][1])        # min_support = the basket's size
    assert sizes[9] == 65 and big[0][9] >= 3 and big[0].sum() == big[0][9] and big[4][1] > 10000
    # ties across the cut
    for n_top, need in ((1, 20), (7, 20), (256, 20), (1024, 20)):
        wt = rs.related_statement(fam["ties"][0], b_ptr, b_item, n_top, raw=fam["ties"][1])
        tied = sum(1 for kept in wt[5]["kept"] if len(kept) > n_top and kept[n_top - 1][1] == kept[n_top][1])
        assert tied >= need, (n_top, tied)
    # NaN and infinite scores, per how
    for how in (SUM, MEAN, MAX):
        ws = rs.related_statement(fam["special"][0], b_ptr, b_item, 7, how, raw=fam["special"][1])
        bad = ws[5]["nonfinite"]
        assert any(s != s for s in bad) and any(math.isinf(s) for s in bad) and ws[4][2] == len(bad), how
        zeros = [s for sc in ws[5]["scored"] for s, _ in sc.values() if s == 0.0]
        assert any(math.copysign(1.0, s) > 0 for s in zeros), how
        assert any(math.copysign(1.0, s) < 0 for s in zeros) == (how == MAX), how       # a sum from 0.0 is never -0.0; a maximum may be
    # every rule drops something
    wr = rs.related_statement(M, b_ptr, b_item, 7, min_support=2, allow=allow, exclude=exclude, min_score=floor, raw=fam["dyadic"][1])
    d = wr[5]
    assert d["rule2"] > 0 and d["mask"] > 0 and d["excluded"] > 0 and wr[4][1] > 0 and wr[4][3] > 0 and wr[4][0] > 0
    plain = rs.related_statement(M, b_ptr, b_item, 7, min_support=2, raw=fam["dyadic"][1])
    assert plain[4][0] - wr[4][0] == d["mask"] + d["excluded"] and plain[5]["rule2"] == d["rule2"]
    # the order of the records matters on the generic family
    differ = 0
    for _, rec in fam["generic"][2]:
        for vs in rec.values():
            differ += len(vs) > 1 and bits(rs.score_of(vs, SUM)) != bits(rs.score_of(vs[::-1], SUM))
    assert differ >= 100


def test_how_and_weights_and_members():
    """a hand-made case, every number checked by eye"""
    M = rs.Matrix([0, 3, 5, 5, 6], [1, 2, 1, 0, 3, 1], [0.5, 0.25, 1.0, 2.0, -0.0, 4.0])
    b_ptr, b_item = [0, 2, 2, 5], [0, 1, 3, 9, 0]
    w = rs.related_statement(M, b_ptr, b_item, 3)
    # query 0: members 0, 1; records 1: [0.5, 1.0], 2: [0.25], 0: [2.0], 3: [-0.0]; the members leave
    assert w[0].tolist() == [2, 0, 2] and w[1][0].tolist() == [2, 3, -1] and w[2][0].tolist() == [0.25, 0.0, 0.0]
    assert math.copysign(1.0, w[2][0, 1]) > 0           # 0.0 + -0.0: the sum starts from 0.0
    # query 2: members 3, 0 (9 has no row); records 1: [4.0, 0.5, 1.0], 2: [0.25]
    assert w[1][2].tolist() == [1, 2, -1] and w[2][2].tolist() == [5.5, 0.25, 0.0] and w[3][2].tolist() == [3, 1, 0]
    assert w[4] == [4, 0, 0, 0, 2, 9]
    k = rs.related_statement(M, b_ptr, b_item, 3, MEAN, KEEP_MEMBERS, weights=[1.0, 2.0, 1.0, 1.0, -1.0])
    assert k[1][0].tolist() == [0, 1, 2] and k[2][0].tolist() == [4.0, 0.75, 0.25] and k[3][0].tolist() == [1, 2, 1]
    assert k[1][2].tolist() == [1, 2, -1] and k[2][2].tolist() == [(4.0 - 0.5 - 1.0) / 3, -0.25, 0.0]
    m = rs.related_statement(M, b_ptr, b_item, 3, MAX, KEEP_MEMBERS, min_support=2)
    assert m[0].tolist() == [1, 0, 1] and m[2][0, 0] == 1.0 and m[2][2, 0] == 4.0 and m[4][1] == 4
    z = rs.related_statement(M, b_ptr, b_item, 4, MAX)
    assert z[1][0].tolist() == [2, 3, -1, -1] and math.copysign(1.0, z[2][0, 1]) < 0     # the -0.0 of the matrix
