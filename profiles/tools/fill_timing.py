"""Timing of the popularity fill (Engine.pop_index, Engine.fill) on a synthetic workload, with the model construction and the
protocol of related_timing.py: HIP events, a warm-up of every variant, the median of --reps, one process.

    index_count / index_mean   Engine.pop_index over the peer index of the resident profiles (the transposition itself,
                               Engine.peer_index, is timed beside them as peer_index)
    topn_<who>_<n>[_mask]      Engine.topn (xmap_topn_rows_filtered when masked) for --queries queries: who = random resident users,
                               or norows = user indices outside the profiles (the anonymous visitor: no evidence, every list empty)
    fill_<who>_<n>[_mask]      Engine.fill of exactly those lists (the copy of the lists it works on included)

at n_top = 10 and 64, without a mask and with a 1 % mask, and records the medians, the fill's stats and fill / topn per case.  A
number, not a gate: the process exits with status 0 whatever it measures.  Run it under a time limit of its own:

    timeout -k 10 1080 python profiles/tools/fill_timing.py --workload c2 --out profiles/fill_timing_c2.json"""
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
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
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
    say("RecommenderSim over %d AlterEgo rows" % G.n_rows)
    P = eng.alterego_profiles(G)
    e2 = device.Engine(P)
    S = e2.rec_sim(50)
    nb = e2.rec_select(S, args.keep)[:3]
    item_avg = S.info[:I, 0].contiguous()
    wtab = torch.from_numpy(np.asarray([np.exp(-0.1 * d) for d in range(4096)], np.float64)).to(dev)
    X = e2.peer_index(P)
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": args.keep, "alterego_rows": int(G.n_rows),
           "indexed_rows": int(X.n_rows), "reps": args.reps, "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()),
           "queries": args.queries, "fill_window": int(abi.FILL_WINDOW), "ranked": {}, "fill_stats": {}, "topn_stats": {}, "ms": {},
           "ms_all": {}, "fill_over_topn": {}}
    rng = np.random.default_rng(1)
    pops = {how: e2.pop_index(X, how, 25.0 if how == "mean" else 0.0, 1) for how in ("count", "mean")}
    res["ranked"] = {how: list(p.counts) for how, p in pops.items()}
    pop = pops["count"]
    mask = torch.from_numpy(rng.random(I) < 0.01).to(dev)
    res["mask_items"] = int(mask.sum().item())
    who = {"random": torch.from_numpy(rng.integers(0, U, args.queries).astype(np.int32)).to(dev),
           "norows": torch.arange(U, U + args.queries, dtype=torch.int32, device=dev)}
    variants = [("peer_index", lambda: e2.peer_index(P)),
                ("index_count", lambda: e2.pop_index(X, "count", 0.0, 1)), ("index_mean", lambda: e2.pop_index(X, "mean", 25.0, 1))]
    for name, d_q in who.items():
        for n_top in (10, 64):
            for masked in (False, True):
                case = "%s_%d%s" % (name, n_top, "_mask" if masked else "")
                kw = {"allow": mask} if masked else {}
                lists = e2.topn(P, nb, d_q, item_avg, wtab, n_top, **kw)
                res["topn_stats"][case] = [int(x) for x in lists[4]]
                res["fill_stats"][case] = [int(x) for x in e2.fill(lists, pop, P, d_q, item_avg, **kw)[5]]
                variants.append(("topn_" + case, lambda d_q=d_q, n_top=n_top, kw=kw: e2.topn(P, nb, d_q, item_avg, wtab, n_top, **kw)))
                variants.append(("fill_" + case, lambda lists=lists, d_q=d_q, kw=kw: e2.fill(lists, pop, P, d_q, item_avg, **kw)))
    times = {v: [] for v, _ in variants}
    for v, fn in variants:
        say("warm-up: " + v)
        once(fn)
    for rep in range(args.reps):
        for v, fn in variants:
            times[v].append(once(fn))
    res["ms"] = {v: float(np.median(t)) for v, t in times.items()}
    res["ms_all"] = {v: [float(x) for x in t] for v, t in times.items()}
    for v in res["ms"]:
        if v.startswith("fill_"):
            res["fill_over_topn"][v[5:]] = res["ms"][v] / max(res["ms"]["topn_" + v[5:]], 1e-9)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
