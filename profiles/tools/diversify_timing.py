"""Timing of diversified top-N (Engine.div_index, Engine.diversify) on the AlterEgo rows of a synthetic workload, with the protocol
of filter_timing.py: HIP events, warm, median of --reps, the calls alternated rep by rep.  The first --users users with rows are
the queries; their pools are the unfiltered xmap_topn_rows lists with n_top = --pool, and that call is timed too: it is what the
re-ranking is an addition to.  One top-N call stays below MAX_PAIRS scored pairs (as in filter_timing.py: once the limit of a single
scoring grid, kept so that the numbers compare), so the queries are cut into equal chunks, halved until the first chunk's call scores
at most MAX_PAIRS pairs; top-N runs chunk by chunk and its time is the sum over the chunks, the re-ranking runs over all pools at
once.

    index           xmap_div_index over the resident RecommenderSim CSR
    topn_pool       xmap_topn_rows, n_top = --pool (unfiltered), all chunks
    topn_n          xmap_topn_rows, n_top = --n: the call without diversification
    rerank_w0       xmap_diversify_rows, pool -> n at weight 0 (the pool's prefix and its ILS)
    rerank_w        xmap_diversify_rows, pool -> n at --weight

and records the sizes (entries of the matrix, its longest row, mean pool count), the share of lists the weight changed and the
mean ILS at both weights.  Weight 0 must return the lists of topn_n (asserted).

    python profiles/tools/diversify_timing.py --workload c2 --out profiles/diversify_timing_c2.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))

MAX_PAIRS = 60000000            # pairs of one call: what the recorded runs used (once the limit of a single scoring grid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c1", "c2"])
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--weight", type=float, default=1.0)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--alpha", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from xmap.engine import device, hipabi as abi, synth

    def say(what):                  # progress on stderr
        sys.stderr.write(what + "\n")
        sys.stderr.flush()

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    dev = "cuda:0"
    say("making the workload")
    r = synth.config_c2() if args.workload == "c2" else synth.config_c1()
    k = args.k or (50 if args.workload == "c2" else 10)
    U, I, keep = r.n_users, r.n_items, args.keep
    say("stages A-C")
    eng = device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, I, r.item_attrs(), dev))
    S = eng.item_sim("cosine", 50)
    E = eng.extend(S, k)
    _, _, mp = eng.select(E, True)
    G = eng.alterego(mp)
    del S, E
    say("RecommenderSim and selection over %d AlterEgo rows" % G.n_rows)
    P = eng.alterego_profiles(G)
    e2 = device.Engine(P)
    Sr = e2.rec_sim(50)
    nb = e2.rec_select(Sr, keep)[:3]
    avg = Sr.info[:I, 0].contiguous()
    wtab = torch.from_numpy(np.asarray([np.exp(- args.alpha * d) for d in range(66)], np.float64)).to(dev)
    deg = P.user_ptr[1:] - P.user_ptr[:-1]
    query = torch.nonzero(deg > 0).flatten()[:args.users].int().contiguous()
    say("pools")
    Q = int(query.numel())
    chunk = Q
    while e2.topn(P, nb, query[:chunk].contiguous(), avg, wtab, args.pool)[4][0] > MAX_PAIRS:
        chunk = (chunk + 1) // 2
    chunks = [query[a:a + chunk].contiguous() for a in range(0, Q, chunk)]

    def topn_all(n_top):            # chunk by chunk: (cnt, item, plain, decayed) of all queries, the pairs scored per chunk
        outs = [e2.topn(P, nb, c, avg, wtab, n_top) for c in chunks]
        return tuple(torch.cat([o[t] for o in outs]) for t in range(4)) + ([o[4][0] for o in outs],)
    pool = topn_all(args.pool)
    assert max(pool[4]) <= MAX_PAIRS, pool[4]
    X = e2.div_index(Sr)
    plain = topn_all(args.n)
    zero = e2.diversify(pool, X, 0.0, args.n)
    assert all(torch.equal(a, b) for a, b in zip(zero[:4], plain[:4])) and zero[7][0] == 0, "weight 0 is the plain call"
    some = e2.diversify(pool, X, args.weight, args.n)
    rows = (Sr.row_ptr[1:] - Sr.row_ptr[:-1])
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": keep, "alterego_rows": int(G.n_rows), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()), "queries": Q, "pool": args.pool, "n": args.n,
           "weight": args.weight, "matrix_entries": int(X.nnz), "longest_row": int(rows.max()) if I else 0,
           "mean_row": float(rows.double().mean()) if I else 0.0, "topn_chunks": len(chunks), "queries_per_chunk": chunk,
           "pairs_scored_pool": int(sum(pool[4])), "pairs_scored_largest_chunk": int(max(pool[4])),
           "mean_pool_count": float(pool[0].double().mean()), "lists_changed": int(some[7][0]), "items_returned": int(some[7][1]),
           "mean_ils_w0": float(zero[6].mean()), "mean_ils_w": float(some[6].mean())}
    variants = [("index", lambda: e2.div_index(Sr)),
                ("topn_pool", lambda: topn_all(args.pool)),
                ("topn_n", lambda: topn_all(args.n)),
                ("rerank_w0", lambda: e2.diversify(pool, X, 0.0, args.n)),
                ("rerank_w", lambda: e2.diversify(pool, X, args.weight, args.n))]
    times = {v: [] for v, _ in variants}
    for rep in range(args.reps):    # alternated, and every rep starts one variant further on: no variant keeps one neighbour
        for v, fn in variants[rep % len(variants):] + variants[:rep % len(variants)]:
            times[v].append(once(fn))
    res["ms"] = {v: float(np.median(t)) for v, t in times.items()}
    res["ms_min_max"] = {v: [float(min(t)), float(max(t))] for v, t in times.items()}
    res["rerank_w_over_topn_pool"] = res["ms"]["rerank_w"] / res["ms"]["topn_pool"]
    say(json.dumps(res["ms"]))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
