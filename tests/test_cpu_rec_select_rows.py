"""The designed rows of tests/rec_select_rows.py before a GPU sees them (tests/test_gpu_rec_select_rows.py): the CPU oracle's
xo_rec_select equals the NumPy statement on every family x storage order x keep, the rows meet the census the comparison needs
(lengths, 4 n + 1 rows, a tie at the cut at every keep, -0.0 and both signs among the chosen entries), and the inputs tell the
two wrong variants of the statement -- ties by arrival order, the key sim without abs -- from the right one.  Everything is
compared exactly: integers as integers, doubles through their uint64 views."""
import numpy as np
import pytest

import rec_select_rows as rr
from rec_select_rows import FAMILIES, KEEPS, LENS, ORDERS, TIED


def test_rows_as_designed():
    n = rr.row_lengths()
    assert len(n) % 4 == 1 and n[0] == 0 and n[-1] == 0
    assert set(LENS) <= set(n.tolist())
    two = np.argsort(n)[-2:]
    assert two[1] - two[0] == 2 and n[two[0] + 1] == 0             # an empty row between the two longest
    assert int(n.sum()) == sum(LENS) + sum(rr.SHORT) and 3800 < int(n.sum()) < 4000
    seen = set()
    for order in ORDERS:
        R = rr.design("levels4", order)
        assert np.array_equal(np.diff(R.row_ptr), n)
        assert R.col.min() == 0 and R.col.max() == 2 ** 31 - 2
        long_row = int(np.argmax(n))
        c = R.col[R.row_ptr[long_row]:R.row_ptr[long_row + 1]]
        assert c.min() == 0 and c.max() == 2 ** 31 - 2
        for i in range(R.I):
            lo, hi = R.row_ptr[i], R.row_ptr[i + 1]
            assert len(np.unique(R.col[lo:hi])) == hi - lo           # distinct columns inside a row
            assert np.array_equal(R.ls[lo:hi], 0.5 * np.arange(hi - lo) + 0.25)
        seen.add(R.col.tobytes())
        # the same entries in every order
        first = rr.design("levels4", "col_asc")
        o = np.lexsort((R.col, R.rows))
        assert np.array_equal(R.col[o], first.col) and np.array_equal(rr.bits(R.sim[o]), rr.bits(first.sim))
        i = long_row
        lo, hi = R.row_ptr[i], R.row_ptr[i + 1]
        rank = np.lexsort((R.col[lo:hi], -np.abs(R.sim[lo:hi])))
        if order == "abs_asc":
            assert np.array_equal(rank, np.arange(hi - lo)[::-1])    # every entry sorts before all the earlier ones
        if order == "abs_desc":
            assert np.array_equal(rank, np.arange(hi - lo))
    assert len(seen) == 5


@pytest.mark.parametrize("family", FAMILIES)
def test_family_values(family):
    s = rr.design(family, "col_asc").sim
    a = np.abs(s)
    assert not np.isnan(s).any() and np.signbit(s).any() and not np.signbit(s).all()
    if family == "one":
        assert len(np.unique(a)) == 1
    elif family == "levels4":
        assert len(np.unique(a)) == 4
    elif family == "zeros":
        z = s[a == 0.0]
        assert 0.65 < len(z) / len(s) < 0.75 and np.signbit(z).any() and not np.signbit(z).all()
    elif family == "distinct":
        assert len(np.unique(a)) == len(s)
    else:
        assert sorted(np.unique(a).tolist()) == sorted(rr.EXTREMES)


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_is_the_statement_and_census(family):
    from oracle import xmap_oracle as xo
    for order in ORDERS:
        R = rr.design(family, order)
        chosen = []
        for keep in KEEPS:
            want = rr.statement(R, keep)
            got = xo.rec_select_rows(R.row_ptr, R.col, R.sim, R.ls, keep)
            assert rr.same(got, want), (family, order, keep, rr.rows_that_differ(got, want))
            n = np.diff(R.row_ptr)
            assert np.array_equal(want[0], np.minimum(n, keep))
            held = np.arange(keep)[None, :] < want[0][:, None]
            assert np.all(want[1][~held] == -1) and not rr.bits(want[2][~held]).any() and not rr.bits(want[3][~held]).any()
            chosen.append(want[2][held])
            # a tie at the cut: the first entry left out has the |sim| of the last one taken
            full = rr.statement(R, int(n.max()))
            rows = np.nonzero(n > keep)[0]
            cut = int((np.abs(full[2][rows, keep - 1]) == np.abs(full[2][rows, keep])).sum())
            print("%s %s keep=%d: %d of %d longer rows are cut inside a tie" % (family, order, keep, cut, len(rows)))
            if family in TIED:
                assert cut >= 1
            else:
                assert cut == 0
        chosen = np.concatenate(chosen)
        assert (chosen > 0).any() and (chosen < 0).any()             # both signs among the chosen entries
        if family in ("zeros", "extremes"):
            z = chosen[chosen == 0.0]
            assert np.signbit(z).any() and not np.signbit(z).all()       # -0.0 and 0.0 among them


@pytest.mark.parametrize("family", FAMILIES)
def test_inputs_discriminate(family):
    """a selection that breaks ties by arrival order, or ranks by sim instead of |sim|, gives other lists on these rows"""
    for order in ORDERS:
        R = rr.design(family, order)
        by_pos = by_sign = 0
        for keep in KEEPS:
            want = rr.statement(R, keep)
            by_pos += len(rr.rows_that_differ(rr.statement(R, keep, tie_by_position=True), want))
            by_sign += len(rr.rows_that_differ(rr.statement(R, keep, signed_key=True), want))
        print("%s %s: (row, keep) results that differ: %d with ties by position, %d with the signed key" % (family, order, by_pos, by_sign))
        if family in TIED and order in ("col_desc", "abs_asc", "shuffle"):
            assert by_pos >= 1
        if family == "distinct" or order == "col_asc":
            assert by_pos == 0                                      # (no tie, or arrival order = column order: nothing to tell)
        assert by_sign >= 1
