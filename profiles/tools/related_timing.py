"""Timing of the related-items call (Engine.related) on the RecommenderSim matrix of a synthetic workload, with the model
construction and the protocol of peers_timing.py: HIP events, a warm-up of every variant, the median of --reps.

    random      Engine.related for --queries baskets of --members random items with a row (how = sum, n_top = --n-top)
    held        Engine.related for --queries baskets of the --members most-held items (the same basket every time: the longest
                rows the model has, and every query with the same candidates)
    sort_*      the library's radix sort alone (xmap_debug_sort_pairs), chunk by chunk as the call cuts its queries (the same
                record count -- markers included -- and key width per chunk, random keys), the keys laid out before the clock
                starts: the yardstick -- the call cannot be faster than its sort

and records the medians, the records per call, the chunks, the key widths and the stats of both calls.  A number, not a gate: the
process exits with status 0 whatever it measures.  Run it under a time limit of its own:

    timeout -k 10 1080 python profiles/tools/related_timing.py --workload c2 --out profiles/related_timing_c2.json"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))


def bits_for(v):
    b = 1
    while (1 << b) < v:
        b += 1
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c1", "c2"])
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--n-top", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--members", type=int, default=5)
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
        if getattr(fn, "prepare", None):
            fn.prepare()                # outside the clock
            torch.cuda.synchronize()
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
    row_len = (S.row_ptr[1:] - S.row_ptr[:-1])[:I]
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "alterego_rows": int(G.n_rows), "matrix_entries": int(S.row_ptr[I].item()),
           "reps": args.reps, "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()), "queries": args.queries,
           "members": args.members, "n_top": args.n_top, "how": "sum", "stats": {}, "ms": {}, "ms_all": {}, "records": {}, "key_bits": {}}
    rng = np.random.default_rng(1)
    with_row = torch.nonzero(row_len > 0).flatten().cpu().numpy()
    n = int(P.user_ptr[-1].item())
    holders = torch.bincount(P.user_item[:n].long().clamp(0, I - 1), minlength=I)
    most_held = torch.topk(holders, args.members).indices.to(torch.int32)
    res["most_held"] = {"items": most_held.tolist(), "holders": holders[most_held.long()].tolist(), "row_entries": row_len[most_held.long()].tolist()}
    b_ptr = torch.arange(args.queries + 1, dtype=torch.int64, device=dev) * args.members
    baskets = {"random": torch.from_numpy(with_row[rng.integers(0, len(with_row), args.queries * args.members)].astype(np.int32)).to(dev),
               "held": most_held.repeat(args.queries).contiguous()}
    variants = []
    for name, b_item in baskets.items():
        say("warm-up: " + name)
        out = e2.related(S, b_ptr, b_item, args.n_top)
        res["stats"][name] = [int(x) for x in out[4]]
        res["records"][name] = int(out[4][5])
        variants.append((name, lambda b_item=b_item: e2.related(S, b_ptr, b_item, args.n_top)))
        # the sort alone, chunk by chunk as the call cuts the queries: consecutive queries with at most 2^22 records (one marker
        # per member included), or one query
        recs = (row_len[b_item.long()] + 1).view(args.queries, args.members).sum(dim=1).cpu().numpy().tolist()
        chunks, k0 = [], 0
        while k0 < len(recs):
            k1, tot = k0 + 1, recs[k0]
            while k1 < len(recs) and tot + recs[k1] <= (1 << 22):
                tot += recs[k1]
                k1 += 1
            chunks.append((tot, bits_for(I) + bits_for(k1 - k0)))
            k0 = k1
        res["key_bits"][name] = sorted(set(c[1] for c in chunks))
        res.setdefault("sort_chunks", {})[name] = [len(chunks), max(c[0] for c in chunks)]
        res.setdefault("records_sorted", {})[name] = int(sum(c[0] for c in chunks))
        src = [torch.from_numpy(rng.integers(0, 1 << w, m, dtype=np.int64)).to(dev) for m, w in chunks]
        bufs = [(torch.empty_like(x), torch.empty(int(x.numel()), dtype=torch.int32, device=dev)) for x in src]

        def sort_alone(chunks=chunks, bufs=bufs):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for (m, w), (keys, vals) in zip(chunks, bufs):
                abi.check(abi.lib.xmap_debug_sort_pairs(st, abi.vp(keys), abi.vp(vals), abi.i64(m), abi.i32(w)))

        def lay_out(src=src, bufs=bufs):
            for k0_, (keys, vals) in zip(src, bufs):
                keys.copy_(k0_)
                vals.copy_(torch.arange(int(keys.numel()), dtype=torch.int32, device=dev))
        sort_alone.prepare = lay_out
        variants.append(("sort_" + name, sort_alone))
    times = {v: [] for v, _ in variants}
    for v, fn in variants:
        say("warm-up: " + v)
        once(fn)
    for rep in range(args.reps):
        for v, fn in variants:
            times[v].append(once(fn))
    res["ms"] = {v: float(np.median(t)) for v, t in times.items()}
    res["ms_all"] = {v: [float(x) for x in t] for v, t in times.items()}
    for name in baskets:
        res[name + "_over_sort"] = res["ms"][name] / max(res["ms"]["sort_" + name], 1e-9)
        res.setdefault("records_per_s", {})[name] = res["records"][name] / max(res["ms"][name] * 1e-3, 1e-12)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
