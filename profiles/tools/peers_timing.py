"""Timing of the peers call (Engine.peer_index / Engine.peers) on the AlterEgo rows of a synthetic workload, with the model
construction and the protocol of group_timing.py: HIP events, a warm-up of every variant, the median of --reps.

    index       Engine.peer_index over the AlterEgo profiles, centred by the item averages of RecommenderSim
    random      Engine.peers for --queries random users with rows (same = True, n_top = --n-top, cap = --cap)
    heavy       Engine.peers for the --queries users with the most records (records of a user = the sum over its rows of the
                holders of the row's item); either list is cut where its records pass --max-records
    sort_*      the library's radix sort alone (xmap_debug_sort_pairs), chunk by chunk as the call cuts its queries (the same
                record count and key width per chunk, random keys), the keys laid out before the clock starts: the yardstick --
                the call cannot be faster than its sort.  What stays inside the clock beyond the call's own sort: the hook's two
                arena temporaries per chunk (the call takes its sort buffers once)

    <list>_rows, <list>_ls, <list>_parent    with --ls / --parent-lib: xmap_peer_rows and xmap_peer_rows_ls of this build and
                xmap_peer_rows of ANOTHER build of the library (the parent commit's libxmap_hip.so), all three through one path
                -- ctypes on output tensors made once -- and in turn within every repetition, so that a pair of medians is a pair of
                alternating runs on one box.  Reported: <list>_ls_over_rows and <list>_rows_over_parent

and records the medians, the records per call, the chunks, the key widths and the stats of both calls.  --no-sort leaves the
sort_* variants out and --lists picks the calls: for a kernel trace of the calls alone
(rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/tools/peers_timing.py --no-sort --reps 2).
A number, not a gate: the process exits with status 0 whatever it measures.  Run it under a time limit of its own:

    timeout -k 10 1080 python profiles/tools/peers_timing.py --workload c2 --out profiles/peers_timing_c2.json"""
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
    ap.add_argument("--cap", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--max-records", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-sort", action="store_true")
    ap.add_argument("--lists", default="random,heavy")
    ap.add_argument("--ls", action="store_true")
    ap.add_argument("--parent-lib", default=None)
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
    say("RecommenderSim over %d AlterEgo rows (the item averages)" % G.n_rows)
    P = eng.alterego_profiles(G)
    e2 = device.Engine(P)
    avg = e2.rec_sim(50).info[:I, 0].contiguous()
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "alterego_rows": int(G.n_rows), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()), "queries": args.queries, "n_top": args.n_top,
           "cap": args.cap, "centred": True, "stats": {}, "ms": {}, "ms_all": {}, "records": {}, "key_bits": {}}
    say("index")
    X = e2.peer_index(P, avg)
    res["rows_indexed"] = X.n_rows
    # records per user: the holders of the items of its rows
    n = int(P.user_ptr[-1].item())
    item = P.user_item[:n].long()
    held = (X.hd_ptr[1:] - X.hd_ptr[:-1])[item.clamp(0, I - 1)] * ((item >= 0) & (item < I))
    deg = P.user_ptr[1:] - P.user_ptr[:-1]
    per_user = torch.zeros(U, dtype=torch.int64, device=dev).index_add_(0, torch.repeat_interleave(torch.arange(U, device=dev), deg), held)
    rng = np.random.default_rng(1)
    with_rows = torch.nonzero(P.user_ptr[1:] > P.user_ptr[:-1]).flatten().cpu().numpy()
    q_random = torch.from_numpy(with_rows[rng.integers(0, len(with_rows), args.queries)].astype(np.int32)).to(dev)
    q_heavy = torch.topk(per_user, args.queries).indices.to(torch.int32)
    parent = C.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None
    if parent:
        res["parent_version"] = int(parent.xmap_version())

    def raw(L, q, ls):
        """xmap_peer_rows (ls: xmap_peer_rows_ls) of the library L on outputs made once"""
        n_q = int(q.numel())
        o_cnt = torch.empty(n_q, dtype=torch.int32, device=dev)
        o_user, o_common = [torch.empty((n_q, args.n_top), dtype=torch.int32, device=dev) for _ in range(2)]
        o_sim, o_ls = [torch.empty((n_q, args.n_top), dtype=torch.float64, device=dev) for _ in range(2)]
        f = L.xmap_peer_rows_ls if ls else L.xmap_peer_rows

        def call():
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            a = [st, abi.i64(n_q), abi.vp(q), abi.i64(P.n_users), abi.vp(P.user_ptr), abi.vp(P.user_item), abi.vp(P.user_rating64),
                 abi.i32(abi.PEERS_SAME), abi.i32(args.n_top), abi.i32(args.cap), abi.i32(1), abi.i64(X.n_users), abi.i32(X.n_items),
                 abi.vp(X.centre), abi.vp(X.hd_ptr), abi.vp(X.hd_user), abi.vp(X.hd_x), abi.vp(X.nrm), abi.i64(0), abi.vp(o_cnt),
                 abi.vp(o_user), abi.vp(o_sim), abi.vp(o_common)] + ([abi.vp(o_ls)] if ls else []) + [None, None]
            rc = f(*a)
            assert rc == 0, rc
        return call
    calls = []
    for name, q in [c for c in (("random", q_random), ("heavy", q_heavy)) if c[0] in args.lists.split(",")]:      # at most --max-records records per call: fewer queries if need be
        fits = int((torch.cumsum(per_user[q.long()], 0) <= args.max_records).sum().item())
        calls.append((name, q[:max(fits, 1)].contiguous()))
        res.setdefault("queries_run", {})[name] = max(fits, 1)
    variants = [("index", lambda: e2.peer_index(P, avg))]
    for name, q in calls:
        say("warm-up: " + name)
        out = e2.peers(X, P, q, args.n_top, cap=args.cap, same=True)
        res["stats"][name] = [int(x) for x in out[4]]
        n_rec = int(out[4][5])
        res["records"][name] = n_rec
        variants.append((name, lambda q=q: e2.peers(X, P, q, args.n_top, cap=args.cap, same=True)))
        if args.ls or parent:
            variants.append((name + "_rows", raw(abi.lib, q, False)))
        if args.ls:
            variants.append((name + "_ls", raw(abi.lib, q, True)))
        if parent:
            variants.append((name + "_parent", raw(parent, q, False)))
        if args.no_sort:
            continue
        # the sort alone, chunk by chunk as the call cuts the queries: consecutive queries with at most 2^22 records, or one query
        recs = per_user[q.long()].cpu().numpy().tolist()
        chunks, k0 = [], 0
        while k0 < len(recs):
            k1, tot = k0 + 1, recs[k0]
            while k1 < len(recs) and tot + recs[k1] <= (1 << 22):
                tot += recs[k1]
                k1 += 1
            if tot > 0:
                chunks.append((tot, bits_for(U) + bits_for(k1 - k0)))
            k0 = k1
        assert sum(c[0] for c in chunks) == n_rec, (sum(c[0] for c in chunks), n_rec)
        res["key_bits"][name] = sorted(set(c[1] for c in chunks))
        res.setdefault("sort_chunks", {})[name] = [len(chunks), max(c[0] for c in chunks)]
        src = [torch.from_numpy(rng.integers(0, 1 << w, m, dtype=np.int64)).to(dev) for m, w in chunks]
        bufs = [(torch.empty_like(k), torch.empty(int(k.numel()), dtype=torch.int32, device=dev)) for k in src]

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
    for name, _ in ([] if args.no_sort else calls):
        res[name + "_over_sort"] = res["ms"][name] / max(res["ms"]["sort_" + name], 1e-9)
    for name, _ in calls:
        if args.ls:
            res[name + "_ls_over_rows"] = res["ms"][name + "_ls"] / max(res["ms"][name + "_rows"], 1e-9)
        if parent:
            res[name + "_rows_over_parent"] = res["ms"][name + "_rows"] / max(res["ms"][name + "_parent"], 1e-9)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
