"""The cosine_user drop-in on the CPU: the statement of xmap_peer_rows_ls (tests/user_sim_statement.py) and the per-pair Python
statement (RecommenderSim.calculate_user_sim_host) against what the reference's egg computed (tests/golden/
cosine_user_small.json.gz, profiles/tools/record_cosine_user_golden.py), and the user-based prediction against the egg's tuples.

The bound on the local sensitivity: every leave-one-out variant and sim itself are at most 1 in magnitude, and about ten
correctly rounded fp64 operations separate the reference's formulation (norm ** 2, a plain sum) from the device's (nx * nx, the
double-double dot), each off by at most 2^-53 relative: 2^-48 absolute.  Observed on this fixture: at most 2^-54.  sim itself is
the same operations on the same numbers -- halves sum exactly -- and must be equal as bits."""
import gzip
import json
import os

import numpy as np
import pytest

import peers_statement as ps
import user_sim_statement as us

HERE = os.path.dirname(os.path.abspath(__file__))
LS_BOUND = 2.0 ** -48


def golden():
    return json.loads(gzip.open(os.path.join(HERE, "golden", "cosine_user_small.json.gz")).read().decode())


def golden_rows(g):
    """the (uid, iid, rating, time) rows of the fixture"""
    return [(g["uid"][u], g["iid"][i], r, 0) for u, prof in enumerate(g["profiles"]) for i, r in prof]


def golden_rdds(g, sc):
    return sc.parallelize(golden_rows(g)), sc.parallelize([(u, [tuple(p) for p in pairs]) for u, pairs in g["test"]])


def golden_tuples(g):
    return [(u, [tuple(p) for p in pairs]) for u, pairs in g["predicted"]]


def b64(x):
    return int(np.float64(x).view(np.uint64))


@pytest.fixture(scope="module")
def g():
    return golden()


def held_to_golden(g, rows):
    """rows: {(u1 index, u2 index): (sim, ls)} -> the largest LS difference; sims equal as bits, the same pairs"""
    assert len(rows) == len(g["pairs"]) > 2000
    worst = 0.0
    for u1, u2, s, l in g["pairs"]:
        sim, ls = rows[u1, u2]
        assert b64(sim) == b64(s), (u1, u2, sim, s)
        worst = max(worst, abs(ls - l))
        assert abs(ls - l) <= LS_BOUND, (u1, u2, ls, l)
    print("largest |ls - golden| = %r = 2^%s" % (worst, np.log2(worst) if worst else "-inf"))
    return worst


def test_the_statement_against_the_golden(g):
    P = ps.Profiles.from_lists([[(i, r) for i, r in prof] for prof in g["profiles"]], g["n_items"])
    held_to_golden(g, us.all_pairs_statement(P, g["cap"]))


def test_the_conditions_of_the_fixture(g):
    assert all(len({i for i, _ in prof}) == len(prof) for prof in g["profiles"])                    # no item twice
    assert len({len(x) for x in g["uid"]}) == 1 and len({len(x) for x in g["iid"]}) == 1            # one id width
    assert g["uid"] == sorted(g["uid"]) and g["iid"] == sorted(g["iid"])                             # index order = id order
    assert all(r >= 0 and r * 2 == int(r * 2) for prof in g["profiles"] for _, r in prof)          # halves, none negative
    by = {}
    for u1, _, s, _ in g["pairs"]:
        by.setdefault(u1, []).append(abs(s))
    k = g["mapping_range"]
    for sims in by.values():
        head = sorted(sims, reverse=True)[:k + 1]
        assert len(set(head)) == len(head)                                                          # no tie at the cut
    assert sum(1 for s in by.values() if len(s) > k) > 40 and len(g["lists"]) == len(by)


def _tools(g):
    from pyspark import SparkContext, SparkConf
    from xmap.core.recommenderSim import RecommenderSim
    from xmap.utils import assist
    sc = SparkContext(conf=SparkConf())
    train, test = golden_rdds(g, sc)
    tool = RecommenderSim("cosine_user", g["cap"])
    return sc, tool, assist, train, test


def test_the_host_statement_against_the_golden(g):
    sc, tool, assist, train, _ = _tools(g)
    user_based = tool.build_sthbased_profile(train, "user")
    item_based = tool.build_sthbased_profile(train, "item")
    user_info = sc.broadcast(tool.get_info(user_based).collectAsMap())
    item_info = sc.broadcast(tool.get_info(item_based).collectAsMap())
    uidx = {u: k for k, u in enumerate(g["uid"])}
    rows = {(uidx[u1], uidx[u2]): (s, l) for (u1, u2), (s, l) in
            tool.calculate_user_sim_host(item_based, user_based, item_info, user_info).collect()}
    held_to_golden(g, rows)


def test_the_prediction_against_the_golden(g):
    """fails on the parent commit with AttributeError: user_based_recommendation raised"""
    from xmap.core.recommenderPrediction import RecommenderPrediction
    sc, tool, assist, train, test = _tools(g)
    user_based = tool.build_sthbased_profile(train, "user")
    user_dict = sc.broadcast(user_based.collectAsMap())
    user_info = sc.broadcast(tool.get_info(user_based).collectAsMap())
    sims = sc.broadcast({u: [tuple(e) for e in lst] for u, lst in g["lists"]})
    pred = RecommenderPrediction(0.0, "cosine_user")
    got = pred.user_based_recommendation(test, user_dict, sims, user_info).collect()
    assert got == golden_tuples(g)
    assert sum(1 for _, p in got if p == [()]) == 1 and sum(len(p) for _, p in got) > 100
    assert [pred.user_based_prediction(line, user_dict, sims, user_info) for line in test.collect()] == golden_tuples(g)
    mae = assist.recommender_prediction_pipeline(pred, tool, test, sims, user_dict, None, user_info, None)
    assert mae == g["mae"] and ";" not in mae


class _Bd(object):
    def __init__(self, value):
        self.value = value


def test_no_list_and_zero_weights_on_the_uknn_golden():
    """the existing fixture of the user-kNN kernels: its last query has no list ([()]), and some line's only evidence for a pair
    has sim 0.0 (ZeroDivisionError) -- where the egg raised, the statement raises"""
    from xmap.core.recommenderPrediction import RecommenderPrediction
    d = json.loads(gzip.open(os.path.join(HERE, "golden", "uknn_small.json.gz")).read().decode())
    uid, iid = d["uid"], d["iid"]
    rating_bd = _Bd({uid[u]: [(iid[i], r, 0) for i, r in rows] for u, rows in enumerate(d["profiles"])})
    sim_bd = _Bd({uid[a]: [(uid[v], s) for v, s in zip(d["nb_user"][q][:d["nb_cnt"][q]], d["nb_sim"][q][:d["nb_cnt"][q]])]
                  for q, a in enumerate(d["query"]) if d["nb_cnt"][q] > 0})
    user_bd = _Bd({uid[u]: (a, 0.0, len(d["profiles"][u])) for u, a in enumerate(d["user_avg"])})
    tool = RecommenderPrediction(0.0, "user_based")
    seen = set()
    for (u, pairs), (u2, want) in zip(d["test"], d["predicted"]):
        line = (u, [tuple(p) for p in pairs])
        if want == "ZeroDivisionError":
            with pytest.raises(ZeroDivisionError):
                tool.user_based_prediction(line, rating_bd, sim_bd, user_bd)
            seen.add("raise")
        else:
            got = tool.user_based_prediction(line, rating_bd, sim_bd, user_bd)
            assert got == (u2, [tuple(p) for p in want])
            seen.add("none" if got[1] == [()] else "some")
    assert seen == {"raise", "none", "some"}
    with pytest.raises(KeyError):                                       # a neighbour without ratings, as in the egg
        tool.user_based_prediction((uid[0], []), rating_bd, _Bd({uid[0]: [("nobody", 1.0)]}), user_bd)
