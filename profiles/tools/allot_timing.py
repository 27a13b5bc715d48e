"""Timing of the allotment (Engine.allot_topn / allot_pool) beside the plain filtered top-N over the same users, on a synthetic
workload, with the model construction and the protocol of quota_timing.py: HIP events, a warm-up of every variant, the median of
--reps.

    allot_<x>     (a) Engine.allot_topn for --queries random users with rows, pool --pool, n_top --n-top, the scalar cap chosen so
                  that the seats of all items together come closest to x times --queries * --n-top (x of --seats: 4, 1, 0.25;
                  an integer cap >= 1 over all items: the result names the ratio it reached)
    topn          (b) one filtered Engine.topn (xmap_topn_rows_filtered, no rule set) over the same queries with n_top = --pool: the
                  pool of every variant of (a)
    pool_<x>      (c) Engine.allot_pool alone on (b)'s output, at the caps of (a)

(a) - (b) and (c) are the allotment's own cost.  --only-allot runs (c) alone, --reps times after a warm-up: the process a kernel
trace is taken of.
A number, not a gate: the process exits with status 0 whatever it measures.  Run it under a time limit of its own:

    timeout -k 10 540 python profiles/tools/allot_timing.py --workload c2 --out profiles/allot_timing_c2.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c1", "c2"])
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--n-top", type=int, default=10)
    ap.add_argument("--pool", type=int, default=64)
    ap.add_argument("--seats", default="4,1,0.25")
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-allot", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from xmap.engine import device, hipabi as abi, synth

    def say(what):                  # progress on stderr: the workload takes minutes to make and to train
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
    U, I = r.n_users, r.n_items
    say("stages A-C")
    eng = device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, I, r.item_attrs(), dev))
    S = eng.item_sim("cosine", 50)
    E = eng.extend(S, k)
    _, _, mp = eng.select(E, True)
    G = eng.alterego(mp)
    del S, E
    P = eng.alterego_profiles(G)
    e2 = device.Engine(P)
    say("RecommenderSim and neighbour lists over %d AlterEgo rows" % G.n_rows)
    S = e2.rec_sim(50)
    nb = e2.rec_select(S, args.keep)[:3]
    item_avg = S.info[:I, 0].contiguous()
    wtab = torch.from_numpy(np.asarray([np.exp(-0.1 * d) for d in range(4096)], np.float64)).to(dev)
    rng = np.random.default_rng(1)
    with_rows = torch.nonzero(P.user_ptr[1:] > P.user_ptr[:-1]).flatten().cpu().numpy()
    q = torch.from_numpy(with_rows[rng.integers(0, len(with_rows), args.queries)].astype(np.int32)).to(dev)
    seats = [float(x) for x in args.seats.split(",")]
    caps = {("%g" % x): max(1, int(round(x * args.queries * args.n_top / float(I)))) for x in seats}
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": args.keep, "alterego_rows": int(G.n_rows), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()), "queries": args.queries, "n_pool": args.pool,
           "n_top": args.n_top, "caps": caps, "seats_over_demand": {x: c * I / float(args.queries * args.n_top) for x, c in caps.items()},
           "stats": {}, "ms": {}, "ms_all": {}}

    def topn():
        return e2.topn(P, nb, q, item_avg, wtab, args.pool, min_score=float("-inf"))
    say("the pools")
    pools = topn()
    res["pool_entries"] = int(pools[0].sum())
    variants = [("pool_" + x, (lambda c=c: e2.allot_pool(pools, args.n_top, cap=c, n_items=I))) for x, c in caps.items()]
    if not args.only_allot:
        variants += [("allot_" + x, (lambda c=c: e2.allot_topn(P, nb, q, item_avg, wtab, args.pool, args.n_top, cap=c))) for x, c in caps.items()]
        variants.append(("topn", topn))
    for v, fn in variants:
        if v != "topn":
            # [lists changed, entries, |R|, void positions, rounds, lists cut short]
            res["stats"][v] = [int(x) for x in fn().stats[-6:]]
    times = {v: [] for v, _ in variants}
    for v, fn in variants:
        say("warm-up: " + v)
        once(fn)
    for rep in range(args.reps):
        for v, fn in variants:
            times[v].append(once(fn))
    res["ms"] = {v: float(np.median(t)) for v, t in times.items()}
    res["ms_all"] = {v: [float(x) for x in t] for v, t in times.items()}
    res["ms_per_round"] = {v: res["ms"][v] / max(res["stats"][v][4], 1) for v in res["ms"] if v.startswith("pool_")}
    if not args.only_allot:
        b = res["ms"]["topn"]
        res["a_minus_b_ms"] = {v: res["ms"][v] - b for v in res["ms"] if v.startswith("allot_")}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
