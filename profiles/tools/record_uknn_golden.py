"""Record tests/golden/uknn_small.json.gz: the reference's own user_based_prediction (it ships in the reference's egg only) run
once on a small designed input, inputs and outputs side by side.  Data only; the tests read the fixture, never this script.

    python profiles/tools/record_uknn_golden.py PATH/TO/xmap-0.1.0-py3.5.egg

The input: the `halves` family of tests/peers_statement.py at 60 users and 25 items without invalid rows (repeated items stay),
under fixed-width ids -- the egg tests `iid in rating[0]`, a substring test, which is equality between ids of one width --, ratings
in halves so that every mean is exact, the neighbour lists of the peers statement (10 neighbours, cap 5, centred), and for every
third user six held-out pairs.  A stub with .value stands in for the broadcasts."""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Stub(object):
    def __init__(self, value):
        self.value = value


def main(egg):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import peers_statement as ps
    import uknn_statement as us
    sys.path.insert(0, egg)
    from xmap.core.recommenderPrediction import RecommenderPrediction
    assert os.path.abspath(sys.modules["xmap"].__file__).startswith(os.path.abspath(egg)), "the egg's package, not the project's"
    U, I, n_nb = 60, 25, 10
    P = ps.random_profiles(3, "halves", U=U, I=I, invalid=0.0)
    uid, iid = ["u%03d" % u for u in range(U)], ["i%03d" % i for i in range(I)]
    rows = us._rows_of(P)
    query = list(range(0, U, 3))
    lists = us.lists_from_peers(P, P, query, (n_nb,), centre=ps.item_means(P))[n_nb]
    lists[0][-1] = 0                                # the last query has no list: the egg skips its pairs, [()]
    avg, cnt = us.means_statement(P)
    for u in range(U):                              # halves: the plain mean is the exact one
        assert cnt[u] == len(rows[u]) and (not rows[u] or avg[u] == sum(r for _, r in rows[u]) / len(rows[u]))
    rng = np.random.RandomState(17)
    test = [(uid[a], [(iid[int(i)], float(rng.randint(1, 11)) / 2.0, 0) for i in rng.randint(0, I, 6)]) for a in query]
    rating_bd = Stub({uid[u]: [(iid[i], r, 0) for i, r in rows[u]] for u in range(U)})
    sim_bd = Stub({uid[a]: [(uid[v], s) for v, s in us._list_of(lists, q)] for q, a in enumerate(query) if lists[0][q] > 0})
    user_bd = Stub({uid[u]: (float(avg[u]), 0.0, int(cnt[u])) for u in range(U)})
    tool = RecommenderPrediction(0.0, "user_based")
    out = []
    for line in test:                               # a line whose only evidence for some pair has sim 0.0 raises: recorded as such
        try:
            out.append(tool.user_based_prediction(line, rating_bd, sim_bd, user_bd))
        except ZeroDivisionError:
            out.append((line[0], "ZeroDivisionError"))
    doc = dict(n_users=U, n_items=I, n_nb=n_nb, uid=uid, iid=iid,
               profiles=[[[int(i), r] for i, r in rows[u]] for u in range(U)], query=query,
               nb_cnt=lists[0].tolist(), nb_user=lists[1].tolist(), nb_sim=lists[2].tolist(), user_avg=avg.tolist(),
               test=[[u, [list(p) for p in pairs]] for u, pairs in test],
               predicted=[[u, pairs if isinstance(pairs, str) else [list(p) for p in pairs]] for u, pairs in out])
    path = os.path.join(ROOT, "tests", "golden", "uknn_small.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(doc, sort_keys=True).encode())
    print("%s: %d users, %d without a list, %d raise" % (path, len(out), sum(1 for _, p in out if p == [()]),
                                                         sum(1 for _, p in out if isinstance(p, str))))


if __name__ == "__main__":
    main(sys.argv[1])
