"""The designed pairs of tests/predict_pairs.py before a GPU sees them (tests/test_gpu_predict_pairs.py): the census of the
statement's results -- every status at every n_w, the evidence counts 63 / 64 / 65 in all three constructions, the edges of n_w
as worked out by hand, a pair whose bounded values differ, every time pattern -- and the proof that the order inside a tie of
times reaches the bits of the decayed sum."""
import numpy as np
import pytest

import predict_pairs as pp
from predict_pairs import ALPHAS, COUNTS, HOWS, N_WS, PATTERNS


def _pairs(**tag):
    c = pp.case()
    return [p for p, t in enumerate(c.tags) if all(t.get(k) == v for k, v in tag.items())]


def _b64(x):
    return int(np.float64(x).view(np.uint64))


def test_arrays_as_designed():
    A = pp.arrays()
    c = pp.case()
    assert len(A.tu) == pp.N_TEST == 129 and set(A.pair_of.tolist()) == set(range(len(c.pairs)))
    assert (A.tu == -1).any() and (A.ti == -1).any()
    assert int(np.diff(A.nb_ptr).min()) == 0 and int(np.diff(A.rt_ptr).min()) == 0
    for n in COUNTS:
        for how in HOWS:
            (p,) = _pairs(kind="count", n=n, how=how)
            assert len(pp.evidence_of(p)) == n
            assert sum(pp.groups_of(n, how)) == n
    assert pp.groups_of(64, "mix") == [8] * 8 and len(pp.groups_of(65, "mix")) == 9
    for pattern in PATTERNS:
        assert len(_pairs(kind="time", pattern=pattern)) == 2
        for p in _pairs(kind="time", pattern=pattern):
            t = np.asarray([e[2] for e in pp.evidence_of(p)])
            assert len(t) == 64
            d = np.diff(t)
            assert {"equal": np.all(d == 0), "ascending": np.all(d > 0), "descending": np.all(d < 0),
                    "alternating": len(set(t.tolist())) == 2 and np.all(d != 0),
                    "blocks": np.all(np.bincount(t.astype(int)) == 8) and np.all(d != 0)}[pattern]
    # the rater search: where the user stands in the raters of neighbour x
    want = {"first": 4, "last": 4, "between": 0, "below": 0, "above": 0, "only": 1, "no user": 0, "no item": 0, "neither": 0}
    assert {c.tags[p]["where"]: len(pp.evidence_of(p)) for p in _pairs(kind="rater")} == want


@pytest.mark.parametrize("alpha", ALPHAS)
def test_census_of_the_statement(alpha):
    A = pp.arrays()
    c = pp.case()
    rows = pp.designed_statement(alpha)
    for n_w in N_WS:
        status, plain, decay = pp.expected(alpha, n_w)
        print("alpha=%g n_w=%d: status counts %s, %d pairs with plain != decay" % (alpha, n_w, np.bincount(status, minlength=3).tolist(),
                                                                                 int((plain != decay).sum())))
        assert set(status.tolist()) == {0, 1, 2}
        assert not plain[status != 0].any() and not decay[status != 0].any()
        ok = status == 0
        assert np.all(np.isin(plain[ok], np.arange(6.0))) and np.all(np.isin(decay[ok], np.arange(6.0)))
        for n in COUNTS:
            for how in HOWS:
                (p,) = _pairs(kind="count", n=n, how=how)
                if alpha == 800.0 and n > 0:
                    want = 2                    # every weight the evidence meets is 0.0
                else:
                    want = 0 if (n <= 64 and n + 1 <= n_w) else 2
                assert status[p] == want, (n, how, n_w)
    # by hand: at n_w = 65, n = 64 is computed; at 64 it is handed back and 63 is computed; at 2 only n <= 1
    if alpha != 800.0:
        s = {n_w: {n: pp.expected(alpha, n_w)[0][_pairs(kind="count", n=n, how="mix")[0]] for n in COUNTS} for n_w in N_WS}
        assert s[65][64] == 0 and s[65][65] == 2 and s[66][64] == 0 and s[66][65] == 2
        assert s[64][64] == 2 and s[64][63] == 0
        assert [s[2][n] for n in COUNTS] == [0, 0, 2, 2, 2, 2, 2, 2]
    status, plain, decay = pp.expected(alpha, 66)
    value = lambda what: (int(status[_pairs(kind="value", what=what)[0]]), float(plain[_pairs(kind="value", what=what)[0]]))
    assert value("average 2.5 alone") == (0, 3.0) and value("average 4.5 alone") == (0, 5.0)
    assert value("average %r alone" % np.nextafter(2.5, 0.0)) == (0, 2.0)
    assert value("average -3.0 alone") == (0, 0.0) and value("average -0.5 alone") == (0, 0.0) and value("average 7.2 alone") == (0, 5.0)
    assert value("average 1e+300 alone") == (0, 5.0) and value("average -1e+300 alone") == (0, 0.0)
    assert value("average nan alone")[0] == 2 and value("average inf alone")[0] == 2
    assert value("neighbour average inf, not held") == (0, 3.0)
    for what in ("all sims zero", "neighbour average inf", "rating nan", "average nan with evidence"):
        assert value(what)[0] == 2, what
    if alpha != 800.0:
        assert value("above 5 with evidence") == (0, 5.0) and value("below 0 with evidence") == (0, 0.0)
        assert value("rating 1e300") == (0, 5.0) and value("rating -1e300") == (0, 0.0)
        assert value("one sim zero")[0] == 0
    if alpha == 1.5:
        differ = [p for p in range(len(c.pairs)) if rows[p][0] == 0 and rows[p][1] != rows[p][2]]
        print("alpha=1.5: designed pairs with plain != decay after bounding: %s" % [c.tags[p] for p in differ])
        assert len(differ) >= 1
        assert any(c.tags[p]["kind"] == "time" for p in differ)
    assert len(A.pair_of) == len(status)


def test_the_order_inside_a_tie_reaches_the_bits():
    """_decayed_ratio on the evidence with every tie of times reversed (the list reversed before the stable sort) gives
    other bits before bounding: an unstable sort in the kernel is not the same arithmetic"""
    from xmap.core.recommenderPrediction import RecommenderPrediction
    for alpha in (0.05, 1.5):
        tool = RecommenderPrediction(alpha, "cosine")
        changed = {}
        for pattern in ("blocks", "equal", "alternating"):
            for p in _pairs(kind="time", pattern=pattern):
                ev = pp.evidence_of(p)
                a, b = tool._decayed_ratio(ev), tool._decayed_ratio(ev[::-1])
                assert abs(a - b) < 1e-12          # the same sum in exact arithmetic
                changed[pattern] = changed.get(pattern, 0) + int(_b64(a) != _b64(b))
        print("alpha=%g: pairs (of 2 per pattern) whose decayed bits change when the ties are reversed: %s" % (alpha, changed))
        assert changed["blocks"] >= 1
        # ascending times have no tie: the reversed list sorts to the same order
        (p, _) = _pairs(kind="time", pattern="ascending")
        ev = pp.evidence_of(p)
        assert _b64(tool._decayed_ratio(ev)) == _b64(tool._decayed_ratio(ev[::-1]))
