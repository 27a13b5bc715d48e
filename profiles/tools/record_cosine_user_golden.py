"""Record tests/golden/cosine_user_small.json.gz: the reference's own user-based pipeline (cosine_user similarity with local
sensitivity, non-private neighbour selection, user_based_recommendation, MAE -- the code ships in the reference's egg only) run
once on a small designed input, inputs and outputs side by side.  Data only; the tests read the fixture, never this script.

    python profiles/tools/record_cosine_user_golden.py PATH/TO/xmap-0.1.0-py3.5.egg

The input: the `halves` family of tests/peers_statement.py at 60 users and 25 items, no invalid row and no item twice in a
profile (the reference's norm is sqrt(sum r^2), the peer index's a bilinear form: they agree without repeats), under fixed-width
ids -- the egg tests `iid in rating[0]`, a substring test, which is equality between ids of one width --, ratings in halves so
that every sum is exact, cap 5, mapping_range 10, and for every third user six held-out pairs.  The seed is one for which no user
has two equal |sim| among its first mapping_range + 1 neighbours: the selection then does not depend on the order of the rows.
oracle/ref_harness/minirdd.py stands in for Spark."""
import gzip
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SEED, U, I, CAP, RANGE = 3, 60, 25, 5, 10


def main(egg):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_harness"))
    import minirdd
    import peers_statement as ps
    minirdd.install_pyspark_stub()
    sys.path.insert(0, egg)
    warnings.simplefilter("ignore", SyntaxWarning)                     # the egg's `pair is not ()`
    from xmap.core.recommenderPrediction import RecommenderPrediction
    from xmap.core.recommenderPrivacy import RecommenderPrivacy
    from xmap.core.recommenderSim import RecommenderSim
    from xmap.utils import assist
    assert os.path.abspath(sys.modules["xmap"].__file__).startswith(os.path.abspath(egg)), "the egg's package, not the project's"
    P = ps.random_profiles(SEED, "halves", U=U, I=I, dup=0.0, invalid=0.0)
    uid, iid = ["u%03d" % u for u in range(U)], ["i%03d" % i for i in range(I)]
    profiles = []
    for u in range(U):                              # the first row of every item: the draw may repeat one
        prof = {}
        for p in range(P.ptr[u], P.ptr[u + 1]):
            prof.setdefault(int(P.item[p]), float(P.rating[p]))
        profiles.append(list(prof.items()))
    assert all(len({i for i, _ in prof}) == len(prof) for prof in profiles), "an item twice in a profile"
    sc = minirdd.MiniSC()
    train = sc.parallelize([(uid[u], iid[i], r, 0) for u in range(U) for i, r in profiles[u]])
    sim_tool = RecommenderSim("cosine_user", CAP)
    user_based, item_based, user_dict_bd, item_dict_bd, user_info_bd, item_info_bd, alterEgo_sim = \
        assist.recommender_calculate_sim_pipeline(sc, sim_tool, train)
    pairs = sorted(alterEgo_sim.collect())
    by = {}
    for (u1, u2), (s, _) in pairs:
        by.setdefault(u1, []).append(abs(s))
    for u1, sims in by.items():
        head = sorted(sims, reverse=True)[:RANGE + 1]
        assert len(set(head)) == len(head), "seed %d: %s has equal |sim| among its first %d neighbours" % (SEED, u1, RANGE + 1)
    lists = assist.recommender_privacy_pipeline(RecommenderPrivacy(RANGE, 0.6, 0.1), alterEgo_sim, False)
    simpair_bd = sc.broadcast(lists.collectAsMap())
    rng = np.random.RandomState(17)
    test = [(uid[a], [(iid[int(i)], float(rng.randint(1, 11)) / 2.0, 0) for i in rng.randint(0, I, 6)]) for a in range(0, U, 3)]
    testRDD = sc.parallelize(test)
    tool = RecommenderPrediction(0.0, "cosine_user")
    predicted = tool.user_based_recommendation(testRDD, user_dict_bd, simpair_bd, user_info_bd).collect()
    mae = assist.recommender_prediction_pipeline(tool, sim_tool, testRDD, simpair_bd, user_dict_bd, item_dict_bd, user_info_bd,
                                                 item_info_bd)
    assert isinstance(mae, str) and ";" not in mae
    uidx = {u: k for k, u in enumerate(uid)}
    doc = dict(n_users=U, n_items=I, cap=CAP, mapping_range=RANGE, seed=SEED, uid=uid, iid=iid,
               profiles=[[[i, r] for i, r in prof] for prof in profiles],
               pairs=[[uidx[u1], uidx[u2], float(s), float(l)] for (u1, u2), (s, l) in pairs],
               lists=[[u, [[v, float(s)] for v, s in lst]] for u, lst in sorted(lists.collect())],
               test=[[u, [list(p) for p in pr]] for u, pr in test],
               predicted=[[u, [list(p) for p in pr]] for u, pr in predicted], mae=mae)
    path = os.path.join(ROOT, "tests", "golden", "cosine_user_small.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(doc, sort_keys=True).encode())
    print("%s: %d bytes, %d pairs, %d lists, %d test users (%d without a list), MAE %s"
          % (path, os.path.getsize(path), len(pairs), len(doc["lists"]), len(test), sum(1 for _, p in predicted if p == [()]), mae))


if __name__ == "__main__":
    main(sys.argv[1])
