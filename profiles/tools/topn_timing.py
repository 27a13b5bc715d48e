"""Timing of the top-N recommendation (Engine.topn: reverse lists -> candidates -> scores -> selection) for all users with
rows on the AlterEgo rows of a synthetic workload, HIP events, warm, median of --reps; beside it Engine.predict (the unchanged
wave-per-pair kernel) on the identical candidate pair list, made here with torch from the profiles and the neighbour lists.

    python profiles/tools/topn_timing.py --workload c2 --out profiles/topn_timing_c2.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/tools/topn_timing.py --workload c2 --reps 3
    python profiles/tools/topn_timing.py --merge profiles/topn_timing_c2.json DIR/.../*kernel_stats.csv

The second command is a run of its own (tracing slows the host); --merge (no GPU) adds the kernels' average times per
Engine.topn call from its statistics, grouped into reverse lists / candidates / scoring / selection."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))

GROUPS = (("reverse_lists", "k_tn_rev<"), ("candidates", "k_tn_candidates<"), ("scoring", "k_predict_rows<false, true>"),
          ("scoring_arena", "k_predict_rows<true, true>"), ("selection", "k_tn_select"), ("predict_same_pairs", "k_predict_rows<false, false>"))


def merge(path, stats_csv):
    with open(path) as f:
        res = json.load(f)
    calls = {}
    with open(stats_csv) as f:
        rows = list(csv.DictReader(f))
    split = {}
    for row in rows:
        name = row.get("Name") or row.get("KernelName") or ""
        for group, key in GROUPS:
            if key in name:
                n, total = int(row["Calls"]), float(row["TotalDurationNs"])
                split.setdefault(group, [0, 0.0])
                split[group][0] += n
                split[group][1] += total
                if group == "selection":
                    calls["topn"] = n
                break
    n_topn = max(calls.get("topn", 1), 1)
    # the k_tn_* kernels and k_predict_rows<., true> run only inside Engine.topn, k_predict_rows<false, false> only inside Engine.predict
    res["kernel_ms_per_topn_call"] = {g: v[1] / 1e6 / (v[0] if g == "predict_same_pairs" else n_topn) for g, v in split.items()}
    res["kernel_launches"] = {g: v[0] for g, v in split.items()}
    with open(path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res["kernel_ms_per_topn_call"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c1", "c2"])
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", nargs=2, default=None, metavar=("JSON", "KERNEL_STATS_CSV"))
    args = ap.parse_args()
    if args.merge:
        return merge(*args.merge)
    import numpy as np
    import torch
    from xmap.engine import device, synth

    def events(fn, reps):
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return out
    dev = "cuda:0"
    r = synth.config_c2() if args.workload == "c2" else synth.config_c1()
    k = args.k or (50 if args.workload == "c2" else 10)
    U, I, keep = r.n_users, r.n_items, args.keep
    eng = device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, I, r.item_attrs(), dev))
    S = eng.item_sim("cosine", 50)
    E = eng.extend(S, k)
    _, _, mp = eng.select(E, True)
    G = eng.alterego(mp)
    del S, E
    P = eng.alterego_profiles(G)
    e2 = device.Engine(P)
    Sr = e2.rec_sim(50)
    nb = e2.rec_select(Sr, keep)[:3]
    avg = Sr.info[:I, 0].contiguous()
    wtab = torch.from_numpy(np.asarray([np.exp(- args.alpha * d) for d in range(66)], np.float64)).to(dev)
    deg = P.user_ptr[1:] - P.user_ptr[:-1]
    query = torch.nonzero(deg > 0).flatten().int().contiguous()                     # all users with rows
    out = e2.topn(P, nb, query, avg, wtab, args.n)                                  # warm-up
    stats = out[4]
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": keep, "n_top": args.n, "alterego_rows": int(G.n_rows),
           "query_users": int(query.numel()), "device": torch.cuda.get_device_name(0), "candidate_pairs": stats[0],
           "dropped": stats[1], "max_now": stats[2], "largest_candidate_count": stats[3], "lists_filled": int((out[0] == args.n).sum())}
    res["topn_ms"] = float(np.median(events(lambda: e2.topn(P, nb, query, avg, wtab, args.n), args.reps)))
    # ---- the identical pair list for the unchanged prediction kernel: (row of a profile) x (reverse row of its item), distinct,
    # without the held pairs; in chunks of users (the join is about keep entries per profile row)
    cnt, col, _ = nb
    pos = torch.arange(keep, device=dev)[None, :] < torch.clamp(cnt, max=keep)[:, None]
    owner = torch.arange(I, device=dev)[:, None].expand(I, keep)[pos]
    neigh = col[pos].long()
    o = torch.argsort(neigh)
    rev_item, rev_cnt = owner[o], torch.bincount(neigh, minlength=I)
    rev_ptr = torch.zeros(I + 1, dtype=torch.int64, device=dev)
    rev_ptr[1:] = torch.cumsum(rev_cnt, 0)
    user_of = torch.repeat_interleave(torch.arange(U, device=dev), deg)
    pu = []
    step = 1 << 22
    for lo in range(0, int(P.nnz), step):
        it = P.user_item[lo:lo + step].long()
        n_each = rev_cnt[it]
        start = torch.repeat_interleave(rev_ptr[it], n_each)
        within = torch.arange(int(n_each.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(n_each, 0) - n_each, n_each)
        key = torch.repeat_interleave(user_of[lo:lo + step], n_each) * I + rev_item[start + within]
        pu.append(key)
    key = torch.unique(torch.cat(pu))
    del pu
    held = user_of * I + P.user_item.long()
    key = key[~torch.isin(key, held)]
    tu, ti = (key // I).int().contiguous(), (key % I).int().contiguous()
    res["predict_pairs"] = int(key.numel())
    assert res["predict_pairs"] == stats[0], (res["predict_pairs"], stats[0])
    e2.predict(P, nb, tu, ti, avg, wtab)
    res["predict_same_pairs_ms"] = float(np.median(events(lambda: e2.predict(P, nb, tu, ti, avg, wtab), args.reps)))
    res["topn_over_predict"] = res["topn_ms"] / res["predict_same_pairs_ms"]
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
