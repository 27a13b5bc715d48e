"""Timing of the fused lists (Engine.fuse) beside the calls that feed them, on a synthetic workload, with the model construction and
the protocol of related_timing.py: HIP events, a warm-up of every variant, the median of --reps.

    topn_64          Engine.topn (item-kNN, n_top 64) for --queries random users with rows
    uknn_64 / _1024  Engine.uknn_topn (n_top 64 and 1 024) over the --n-nb peers of the same users
    fuse_64 / _1024  Engine.fuse of the item-kNN list with the user-kNN list of that depth (RRF, n_top --n-top): W = 128 is the block
                     route, W = 1 088 the block route at N = 2 048
    ab_block / ab_wide / ab_sorted  the A/B of the two routes on the same records: the two 64-wide lists as they are (block route, W =
                     128), with ONE list of width 1 024 whose counts are all 0 appended (W = 1 152: still the block route, its
                     widest kernel) and with TWO of them (W = 2 176, above XMAP_FUSE_BLOCK_RECORDS: the sorted-runs route); the
                     same output bytes, asserted.  The three are alternated in this process --ab-reps times in a rotating order,
                     so the spread is known: the medians, the quartiles and every sample are recorded.

A number, not a gate: the process exits with status 0 whatever it measures.  Run it under a time limit of its own:

    timeout -k 10 1080 python profiles/tools/fuse_timing.py --workload c2 --out profiles/fuse_timing_c2.json"""
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
    ap.add_argument("--n-nb", type=int, default=50)
    ap.add_argument("--cap", type=int, default=5)
    ap.add_argument("--n-top", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ab-reps", type=int, default=31)
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
    say("RecommenderSim, neighbour lists and the peer index over %d AlterEgo rows" % G.n_rows)
    S = e2.rec_sim(50)
    nb = e2.rec_select(S, args.keep)[:3]
    item_avg = S.info[:I, 0].contiguous()
    wtab = torch.from_numpy(np.asarray([np.exp(-0.1 * d) for d in range(4096)], np.float64)).to(dev)
    X = e2.peer_index(P, e2.peer_centre(e2.peer_index(P)))
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": args.keep, "alterego_rows": int(G.n_rows), "reps": args.reps,
           "ab_reps": args.ab_reps, "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()), "queries": args.queries,
           "n_nb": args.n_nb, "cap": args.cap, "n_top": args.n_top, "how": "rrf", "block_records": int(abi.FUSE_BLOCK_RECORDS), "stats": {},
           "ms": {}, "ms_all": {}}
    rng = np.random.default_rng(1)
    with_rows = torch.nonzero(P.user_ptr[1:] > P.user_ptr[:-1]).flatten().cpu().numpy()
    q = torch.from_numpy(with_rows[rng.integers(0, len(with_rows), args.queries)].astype(np.int32)).to(dev)
    say("warm-up: the lists")
    peers = e2.peers(X, P, q, args.n_nb, cap=args.cap, same=True)
    means = e2.user_means(P)[0]
    q_avg = means[q.long()]
    it = e2.topn(P, nb, q, item_avg, wtab, 64)
    us = {d: e2.uknn_topn(P, P, q, peers, q_avg, d, means, own_mean=True) for d in (64, 1024)}
    res["stats"]["topn_64"] = [int(x) for x in it[4]]
    res["list_entries"] = {"topn_64": int(it[0].sum().item())}
    for d in us:
        res["stats"]["uknn_%d" % d] = [int(x) for x in us[d][4]]
        res["list_entries"]["uknn_%d" % d] = int(us[d][0].sum().item())
    pair = {d: [it[:3], us[d][:3]] for d in us}
    empty = (torch.zeros(args.queries, dtype=torch.int32, device=dev), torch.full((args.queries, 1024), -1, dtype=torch.int32, device=dev),
             torch.zeros((args.queries, 1024), dtype=torch.float64, device=dev))
    ab = {"ab_block": pair[64], "ab_wide": pair[64] + [empty], "ab_sorted": pair[64] + [empty, empty]}
    res["ab_widths"] = {name: sum(int(l[1].shape[1]) for l in lists) for name, lists in ab.items()}
    assert res["ab_widths"]["ab_block"] <= res["ab_widths"]["ab_wide"] <= abi.FUSE_BLOCK_RECORDS < res["ab_widths"]["ab_sorted"]
    outs = {name: e2.fuse(lists, args.n_top) for name, lists in ab.items()}
    for d in us:
        res["stats"]["fuse_%d" % d] = [int(x) for x in e2.fuse(pair[d], args.n_top)[4]]
    for name in ab:
        res["stats"][name] = [int(x) for x in outs[name][4]]
    res["ab_same_bytes"] = bool(all(all(torch.equal(a.view(torch.int32) if a.dtype == torch.float64 else a,
                                                    b.view(torch.int32) if b.dtype == torch.float64 else b)
                                        for a, b in zip(outs["ab_block"][:4], outs[name][:4])) and outs["ab_block"][4] == outs[name][4]
                                    for name in ab))
    variants = [("topn_64", lambda: e2.topn(P, nb, q, item_avg, wtab, 64))]
    for d in us:
        variants.append(("uknn_%d" % d, lambda d=d: e2.uknn_topn(P, P, q, peers, q_avg, d, means, own_mean=True)))
        variants.append(("fuse_%d" % d, lambda d=d: e2.fuse(pair[d], args.n_top)))
    times = {v: [] for v, _ in variants}
    for v, fn in variants:
        say("warm-up: " + v)
        once(fn)
    for rep in range(args.reps):
        for v, fn in variants:
            times[v].append(once(fn))
    # the A/B: alternated in one process, the order rotated every repetition
    ab_fn = {name: (lambda lists=lists: e2.fuse(lists, args.n_top)) for name, lists in ab.items()}
    for name in ab_fn:
        say("warm-up: " + name)
        once(ab_fn[name])
        times[name] = []
    for rep in range(args.ab_reps):
        names = list(ab_fn)
        for name in names[rep % 3:] + names[:rep % 3]:
            times[name].append(once(ab_fn[name]))
    res["ms"] = {v: float(np.median(t)) for v, t in times.items()}
    res["ms_all"] = {v: [float(x) for x in t] for v, t in times.items()}
    res["ab_quartiles_ms"] = {v: [float(x) for x in np.percentile(times[v], [25, 50, 75])] for v in ab_fn}
    res["ab_range_ms"] = {v: [float(min(times[v])), float(max(times[v]))] for v in ab_fn}
    res["ab_sorted_over_block"] = res["ms"]["ab_sorted"] / max(res["ms"]["ab_block"], 1e-9)
    res["ab_block_faster_beyond_spread"] = bool(max(times["ab_block"]) < min(times["ab_sorted"]))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
