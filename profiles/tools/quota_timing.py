"""Timing of the quota lists (Engine.quota_topn) beside the plain top-N over the same users, on a synthetic workload, with the model
construction and the protocol of shelf_timing.py: HIP events, a warm-up of every variant, the median of --reps.

    cap_<p>_<t> / share_<p>_<t>   (a) Engine.quota_topn for --queries random users with rows: pool p of --pools, label table t (1: one
                                  label per item, 2: two), --labels labels, n_top --n-top; "cap": at most --cap of a label, "share": the
                                  seats by the user's own history
    topn                          (b) one Engine.topn over the same queries (n_top --n-top): the yardstick -- its scoring pass is the
                                  front half of every variant of (a)

(a) - (b) is what the back half costs beyond the wave-per-query selection it replaces.  --only-quota runs (a) alone, --reps times
after a warm-up: the process a kernel trace is taken of.
A number, not a gate: the process exits with status 0 whatever it measures.  Run it under a time limit of its own:

    timeout -k 10 540 python profiles/tools/quota_timing.py --workload c2 --out profiles/quota_timing_c2.json"""
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
    ap.add_argument("--cap", type=int, default=2)
    ap.add_argument("--pools", default="64,256,1024")
    ap.add_argument("--labels", type=int, default=20)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-quota", action="store_true")
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
    # the labels of shelf_timing.py: pseudo-categories by a hash of the item index; the second table adds another label to every item
    L = args.labels
    first = (np.arange(I, dtype=np.int64) * 2654435761 % (1 << 32)) % L
    second = (first + 1 + (np.arange(I, dtype=np.int64) * 40503 % (L - 1))) % L
    tables = {}
    for name, per in (("1", first[:, None]), ("2", np.sort(np.stack([first, second], axis=1), axis=1))):
        lab_ptr = np.arange(I + 1, dtype=np.int64) * per.shape[1]
        tables[name] = e2.set_labels(I, L, lab_ptr, per.reshape(-1).astype(np.int32))
    pools = [int(x) for x in args.pools.split(",")]
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": args.keep, "alterego_rows": int(G.n_rows), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()), "queries": args.queries, "labels": L,
           "n_top": args.n_top, "cap": args.cap, "pools": pools, "stats": {}, "ms": {}, "ms_all": {}}

    def quota(mode, pool, name):
        return e2.quota_topn(P, nb, q, item_avg, wtab, tables[name], pool, args.n_top, mode, cap=args.cap)
    variants = [("%s_%d_%s" % (mode, pool, name), (lambda m=mode, p=pool, n=name: quota(m, p, n)))
                for mode in ("cap", "share") for pool in pools for name in ("1", "2")]
    if not args.only_quota:
        variants.append(("topn", lambda: e2.topn(P, nb, q, item_avg, wtab, args.n_top)))
    for v, fn in variants:
        if v != "topn":
            res["stats"][v] = [int(x) for x in fn()[6]]
    times = {v: [] for v, _ in variants}
    for v, fn in variants:
        say("warm-up: " + v)
        once(fn)
    for rep in range(args.reps):
        for v, fn in variants:
            times[v].append(once(fn))
    res["ms"] = {v: float(np.median(t)) for v, t in times.items()}
    res["ms_all"] = {v: [float(x) for x in t] for v, t in times.items()}
    if not args.only_quota:
        b = res["ms"]["topn"]
        res["a_minus_b_ms"] = {v: res["ms"][v] - b for v in res["ms"] if v != "topn"}
        res["a_over_b"] = {v: res["ms"][v] / max(b, 1e-9) for v in res["ms"] if v != "topn"}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
