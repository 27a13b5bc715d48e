"""Timing of the audience of an item (Engine.audience: holders -> candidates -> scores -> selection) on the AlterEgo rows of a
synthetic workload, for two sets of target items that have a neighbour list -- the --items most-held ones and --items random
ones -- HIP events, warm, median of --reps; beside each Engine.predict (the unchanged wave-per-pair kernel) on the identical
candidate pair list, made here with torch from the profiles and the neighbour lists.

    python profiles/tools/audience_timing.py --workload c2 --out profiles/audience_timing_c2.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/tools/audience_timing.py --workload c2 --reps 3
    python profiles/tools/audience_timing.py --merge profiles/audience_timing_c2.json DIR/.../*kernel_stats.csv

The second command is a run of its own (tracing slows the host); --merge (no GPU) adds the kernels' average times per
Engine.audience call from its statistics (both item sets together), grouped into holders / candidates / scoring / selection."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))

GROUPS = (("holders", "k_au_holders<"), ("candidates", "k_au_candidates<"), ("scoring", "k_predict_rows<false, true>"),
          ("scoring_arena", "k_predict_rows<true, true>"), ("selection", "k_au_select<"), ("predict_same_pairs", "k_predict_rows<false, false>"))


def merge(path, stats_csv):
    with open(path) as f:
        res = json.load(f)
    with open(stats_csv) as f:
        rows = list(csv.DictReader(f))
    split = {}
    for row in rows:
        name = row.get("Name") or row.get("KernelName") or ""
        for group, key in GROUPS:
            if key in name:
                split.setdefault(group, [0, 0.0])
                split[group][0] += int(row["Calls"])
                split[group][1] += float(row["TotalDurationNs"])
                break
    n_calls = max(split.get("selection", [1])[0], 1)         # one selection launch per Engine.audience call
    # the k_au_* kernels and k_predict_rows<., true> run only inside Engine.audience, k_predict_rows<false, false> only inside Engine.predict
    res["kernel_ms_per_audience_call"] = {g: v[1] / 1e6 / (v[0] if g == "predict_same_pairs" else n_calls) for g, v in split.items()}
    res["kernel_launches"] = {g: v[0] for g, v in split.items()}
    with open(path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res["kernel_ms_per_audience_call"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c1", "c2"])
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--items", type=int, default=1000)
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

    def say(what):                  # progress on stderr: the workload takes minutes to make and to train
        sys.stderr.write(what + "\n")
        sys.stderr.flush()
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
    cnt, col, _ = nb
    # ---- the profiles by item, with torch (what k_au_holders builds inside every call)
    deg = P.user_ptr[1:] - P.user_ptr[:-1]
    user_of = torch.repeat_interleave(torch.arange(U, device=dev), deg)
    items = P.user_item[:P.nnz].long()
    o = torch.argsort(items)
    hold_user, hold_cnt = user_of[o], torch.bincount(items, minlength=I)
    hold_ptr = torch.zeros(I + 1, dtype=torch.int64, device=dev)
    hold_ptr[1:] = torch.cumsum(hold_cnt, 0)
    listed = torch.nonzero(cnt > 0).flatten()
    n_q = min(args.items, int(listed.numel()))
    sets = {"most_held": listed[torch.argsort(hold_cnt[listed], descending=True, stable=True)[:n_q]],
            "random": listed[torch.from_numpy(np.random.default_rng(1).permutation(int(listed.numel()))[:n_q]).to(dev)]}
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": keep, "n_top": args.n, "alterego_rows": int(G.n_rows),
           "items_with_a_list": int(listed.numel()), "device": torch.cuda.get_device_name(0), "reps": args.reps, "sets": {}}
    for name, q_items in sets.items():
        say("audience of the %s items" % name)
        query = q_items.int().contiguous()
        out = e2.audience(P, nb, query, avg, wtab, args.n)                          # warm-up
        stats = out[4]
        one = {"query_items": int(query.numel()), "holders_of_the_most_held": int(hold_cnt[q_items].max()), "candidate_pairs": stats[0],
               "dropped": stats[1], "max_now": stats[2], "largest_candidate_count": stats[3], "lists_filled": int((out[0] == args.n).sum())}
        one["audience_ms"] = float(np.median(events(lambda: e2.audience(P, nb, query, avg, wtab, args.n), args.reps)))
        # ---- the identical pair list for the unchanged prediction kernel: (list position of a query item) x (holders of that
        # neighbour), distinct, without the pairs whose user holds the item
        pos = torch.arange(keep, device=dev)[None, :] < torch.clamp(cnt[q_items], max=keep)[:, None]
        owner = q_items[:, None].expand(-1, keep)[pos]
        neigh = col[q_items][pos].long()
        ok = (neigh >= 0) & (neigh < I)
        owner, neigh = owner[ok], neigh[ok]
        n_each = hold_cnt[neigh]
        start = torch.repeat_interleave(hold_ptr[neigh], n_each)
        within = torch.arange(int(n_each.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(n_each, 0) - n_each, n_each)
        key = torch.unique(torch.repeat_interleave(owner, n_each) * U + hold_user[start + within])      # item-major, users ascending
        n_own = hold_cnt[q_items]
        own_start = torch.repeat_interleave(hold_ptr[q_items], n_own)
        own_within = torch.arange(int(n_own.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(n_own, 0) - n_own, n_own)
        held = torch.repeat_interleave(q_items, n_own) * U + hold_user[own_start + own_within]
        key = key[~torch.isin(key, held)]
        ti, tu = (key // U).int().contiguous(), (key % U).int().contiguous()
        one["predict_pairs"] = int(key.numel())
        say("%d pairs: audience %.3f ms; the prediction on the same pairs" % (stats[0], one["audience_ms"]))
        assert one["predict_pairs"] == stats[0], (one["predict_pairs"], stats[0])
        e2.predict(P, nb, tu, ti, avg, wtab)
        one["predict_same_pairs_ms"] = float(np.median(events(lambda: e2.predict(P, nb, tu, ti, avg, wtab), args.reps)))
        one["audience_over_predict"] = one["audience_ms"] / one["predict_same_pairs_ms"]
        del key, held, tu, ti, start, within
        res["sets"][name] = one
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
