"""Timing of the union of AlterEgo rows at BASELINE configs[3] (synth.config_c4: 4 source domains x 1.25 M users, k = 100, private
mapping), the rows as run_multidomain produces them:

 (a) Engine.union_profiles (xmap_union_count + xmap_union_fill), HIP-event brackets (Engine.timed), median of --reps after a
     warm-up, next to the bytes it must move -- every input row read twice (24 B: item, rating, time; + the 4 B gather of its
     item_map entry), every output row written once (20 B), the offsets and inverse maps once per pass -- so the achieved
     fraction of the HBM bandwidth is on file;
 (b) the host route the driver took before: .cpu() of every domain's columns, concatenation, the example's tuples and
     LocalRDD.distinct() -- wall clock, once (--host-rows bounds the rows the Python part takes; the result is scaled);
 (c) the RecommenderSim pass that follows the union (Engine(P).rec_sim), once after a warm-up, for the ranking of what is left;
 and the histogram of the union users' row counts by class (short / medium / large).

    python profiles/tools/union_timing.py --out profiles/union_c4.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))
HBM_GBS = 8000.0            # MI355X peak HBM3E bandwidth, GB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--users", type=int, default=0, help="0: the configs[3] shape; else a smaller shape of the same generator")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-rows", type=int, default=0, help="rows the Python part of the host route takes (0: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from xmap.engine import device, sharded, synth
    t0 = time.perf_counter()

    def note(what):
        print("[%7.1f s] %s" % (time.perf_counter() - t0, what), file=sys.stderr, flush=True)
    doms = synth.config_c4(n_sources=args.sources) if not args.users else \
        synth.make_multi_domain(4, args.users, max(args.users // 6, 50), max(args.users // 6, 50), args.sources)
    note("workload made")
    parts, n_users, n_target = [], 0, 0
    for d, r in enumerate(doms):
        eng = device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
        G = sharded.run_step(eng, "adjust_cosine", 50, args.k, True)["G"]
        item_map = torch.arange(r.n_items, dtype=torch.int32, device=eng.dev) - r.n_src_items
        item_map[:r.n_src_items] = -1
        parts.append((G, torch.arange(r.n_users, dtype=torch.int32, device=eng.dev), item_map, None))
        n_users, n_target = max(n_users, r.n_users), max(n_target, r.n_items - r.n_src_items)
        del eng
        torch.cuda.empty_cache()
        note("domain %d: %d AlterEgo rows" % (d, G.n_rows))
    rows_in = sum(int(p[0].n_rows) for p in parts)
    res = {"shape": "configs[3]" if not args.users else "make_multi_domain(%d users)" % args.users, "sources": args.sources, "k": args.k,
           "users": n_users, "target_items": n_target, "rows_in": rows_in, "device": torch.cuda.get_device_name(0), "reps": args.reps}
    # ---- (a)
    for distinct in (True, False):
        timers = {}
        for _ in range(3 + args.reps):
            P = device.Engine.union_profiles(parts, n_users, n_target, distinct=distinct, timers=timers)
        torch.cuda.synchronize()
        ms = {k: [a.elapsed_time(b) for a, b in v][3:] for k, v in timers.items()}
        both = [x + y for x, y in zip(ms["union_count"], ms["union_fill"])]
        n_out = P.counts[0]
        small = 8 * 2 * sum(int(p[0].off_t.numel()) for p in parts) + 4 * 3 * len(parts) * n_users + 8 * n_users
        bytes_count = rows_in * 28 + small + 4 * sum(int(p[1].numel()) + int(p[2].numel()) for p in parts)     # + the check's pass over the maps
        bytes_fill = rows_in * 28 + n_out * 20 + small
        key = "distinct" if distinct else "plain"
        res[key] = {"counts": list(P.counts), "count_ms": float(np.median(ms["union_count"])), "fill_ms": float(np.median(ms["union_fill"])),
                    "count_plus_fill_ms": float(np.median(both)), "p10_ms": float(np.percentile(both, 10)), "p90_ms": float(np.percentile(both, 90)),
                    "bytes_moved": bytes_count + bytes_fill,
                    "achieved_GBs": (bytes_count + bytes_fill) / (float(np.median(both)) * 1e-3) / 1e9}
        res[key]["fraction_of_hbm_peak"] = res[key]["achieved_GBs"] / HBM_GBS
        note("union (%s): %.3f ms" % (key, res[key]["count_plus_fill_ms"]))
    P = device.Engine.union_profiles(parts, n_users, n_target, distinct=True)
    L = np.zeros(n_users, np.int64)
    for G, um, _, _ in parts:
        L[um.cpu().numpy()] += (torch.diff(G.off_t) + torch.diff(G.off_m)).cpu().numpy()
    res["users_by_class"] = {"none": int((L == 0).sum()), "short_1_32": int(((L > 0) & (L <= 32)).sum()),
                             "medium_33_2048": int(((L > 32) & (L <= 2048)).sum()), "large": int((L > 2048).sum()),
                             "rows_short": int(L[L <= 32].sum()), "rows_medium": int(L[(L > 32) & (L <= 2048)].sum()),
                             "rows_large": int(L[L > 2048].sum()), "mean_rows": float(L.mean()), "max_rows": int(L.max())}
    # ---- (c)
    e2 = device.Engine(P)
    e2.rec_sim(50)
    torch.cuda.synchronize()
    t = time.perf_counter()
    S = e2.rec_sim(50)
    torch.cuda.synchronize()
    res["rec_sim_after_union_ms"] = (time.perf_counter() - t) * 1e3
    res["rec_sim_pairs"] = int(S.row_ptr[-1].item())
    del S, e2
    note("rec_sim over the union: %.1f ms" % res["rec_sim_after_union_ms"])
    # ---- (b)
    t = time.perf_counter()
    cols = {"user": [], "item": [], "rating": [], "time": []}
    for d, (G, _, _, _) in enumerate(parts):
        cols["user"].append(G.user.cpu())
        cols["item"].append(G.item.cpu() - int(doms[d].n_src_items))
        cols["rating"].append(G.rating.cpu())
        cols["time"].append(G.time.cpu())
    host = {k: torch.cat(v).numpy() for k, v in cols.items()}
    t_copy = time.perf_counter() - t
    n_py = min(args.host_rows, rows_in) if args.host_rows else rows_in
    t = time.perf_counter()
    tuples = list(zip(host["user"][:n_py].tolist(), host["item"][:n_py].tolist(), host["rating"][:n_py].tolist(), host["time"][:n_py].tolist()))
    seen, out = set(), []
    for x in tuples:
        if x not in seen:
            seen.add(x)
            out.append(x)
    t_py = time.perf_counter() - t
    res["host_route"] = {"copy_and_concatenate_ms": t_copy * 1e3, "python_rows": n_py, "python_distinct_ms": t_py * 1e3,
                         "python_distinct_scaled_ms": t_py * 1e3 * rows_in / max(n_py, 1), "rows_out_of_python_rows": len(out),
                         "total_ms": t_copy * 1e3 + t_py * 1e3 * rows_in / max(n_py, 1)}
    note("host route: %.0f ms" % res["host_route"]["total_ms"])
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
