"""Timing of the user-kNN calls (Engine.uknn_topn / Engine.uknn_predict) on the AlterEgo rows of a synthetic workload, with the
model construction and the protocol of peers_timing.py: HIP events, a warm-up of every variant, the median of --reps.

    peers       Engine.peers for --queries random users with rows (same = True, n_top = --n-nb, cap = --cap): the call that feeds
                the two below
    means       Engine.user_means over the AlterEgo profiles
    topn        Engine.uknn_topn over those lists (n_top = --n-top, Resnick's formula)
    predict     Engine.uknn_predict for the pairs (query, item) of the lists topn returned: --n-top pairs per user, all with evidence
    sort_topn   the library's radix sort alone (xmap_debug_sort_pairs), chunk by chunk as the call cuts its queries (the same
                record count and key width per chunk, random keys), the keys laid out before the clock starts: the yardstick --
                the call cannot be faster than its sort

and records the medians, the records, the chunks, the key widths and the stats.  A number, not a gate: the process exits with
status 0 whatever it measures.  Run it under a time limit of its own:

    timeout -k 10 1080 python profiles/tools/uknn_timing.py --workload c2 --out profiles/uknn_timing_c2.json"""
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
    ap.add_argument("--n-nb", type=int, default=50)
    ap.add_argument("--n-top", type=int, default=10)
    ap.add_argument("--cap", type=int, default=5)
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
    P = eng.alterego_profiles(G)
    e2 = device.Engine(P)
    say("the peer index over %d AlterEgo rows, centred by the item averages" % G.n_rows)
    X = e2.peer_index(P, e2.peer_centre(e2.peer_index(P)))
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "alterego_rows": int(G.n_rows), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()), "queries": args.queries, "n_nb": args.n_nb,
           "n_top": args.n_top, "cap": args.cap, "centred": True, "own_mean": True, "stats": {}, "ms": {}, "ms_all": {}}
    rng = np.random.default_rng(1)
    with_rows = torch.nonzero(P.user_ptr[1:] > P.user_ptr[:-1]).flatten().cpu().numpy()
    q = torch.from_numpy(with_rows[rng.integers(0, len(with_rows), args.queries)].astype(np.int32)).to(dev)
    say("warm-up: peers, means, topn, predict")
    lists = e2.peers(X, P, q, args.n_nb, cap=args.cap, same=True)
    res["stats"]["peers"] = [int(x) for x in lists[4]]
    means = e2.user_means(P)[0]
    q_avg = means[q.long()]
    top = e2.uknn_topn(P, P, q, lists, q_avg, args.n_top, means, own_mean=True)
    res["stats"]["topn"] = [int(x) for x in top[4]]
    n_rec = int(top[4][5])
    res["records"] = n_rec
    ok = top[1] >= 0
    tq = torch.arange(args.queries, dtype=torch.int32, device=dev)[:, None].expand_as(top[1])[ok].contiguous()
    ti = top[1][ok].contiguous()
    pred = e2.uknn_predict(P, lists, q_avg, tq, ti, means, True)
    res["pairs"] = int(tq.numel())
    res["pair_status"] = [int(x) for x in torch.bincount(pred[3], minlength=4).cpu().numpy()]
    res["pair_evidence_mean"] = float(pred[2].double().mean().item()) if int(tq.numel()) else 0.0
    # the sort alone, chunk by chunk as the call cuts the queries: consecutive queries with at most 2^22 records, or one query
    deg = (P.user_ptr[1:] - P.user_ptr[:-1])
    inside = torch.arange(args.n_nb, device=dev)[None, :] < lists[0][:, None]
    recs = (deg[lists[1].clamp(0, U - 1).long()] * inside).sum(dim=1).cpu().numpy().tolist()
    chunks, k0 = [], 0
    while k0 < len(recs):
        k1, tot = k0 + 1, recs[k0]
        while k1 < len(recs) and tot + recs[k1] <= (1 << 22):
            tot += recs[k1]
            k1 += 1
        if tot > 0:
            chunks.append((tot, bits_for(I) + bits_for(k1 - k0)))
        k0 = k1
    res["records_by_degree"] = int(sum(c[0] for c in chunks))       # = records when every row is valid, as AlterEgo rows are
    res["key_bits"] = sorted(set(c[1] for c in chunks))
    res["sort_chunks"] = [len(chunks), max([c[0] for c in chunks] or [0])]
    src = [torch.from_numpy(rng.integers(0, 1 << w, m, dtype=np.int64)).to(dev) for m, w in chunks]
    bufs = [(torch.empty_like(x), torch.empty(int(x.numel()), dtype=torch.int32, device=dev)) for x in src]

    def sort_alone():
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for (m, w), (keys, vals) in zip(chunks, bufs):
            abi.check(abi.lib.xmap_debug_sort_pairs(st, abi.vp(keys), abi.vp(vals), abi.i64(m), abi.i32(w)))

    def lay_out():
        for x, (keys, vals) in zip(src, bufs):
            keys.copy_(x)
            vals.copy_(torch.arange(int(keys.numel()), dtype=torch.int32, device=dev))
    sort_alone.prepare = lay_out
    variants = [("peers", lambda: e2.peers(X, P, q, args.n_nb, cap=args.cap, same=True)),
                ("means", lambda: e2.user_means(P)),
                ("topn", lambda: e2.uknn_topn(P, P, q, lists, q_avg, args.n_top, means, own_mean=True)),
                ("predict", lambda: e2.uknn_predict(P, lists, q_avg, tq, ti, means, True)),
                ("sort_topn", sort_alone)]
    times = {v: [] for v, _ in variants}
    for v, fn in variants:
        say("warm-up: " + v)
        once(fn)
    for rep in range(args.reps):
        for v, fn in variants:
            times[v].append(once(fn))
    res["ms"] = {v: float(np.median(t)) for v, t in times.items()}
    res["ms_all"] = {v: [float(x) for x in t] for v, t in times.items()}
    res["topn_over_sort"] = res["ms"]["topn"] / max(res["ms"]["sort_topn"], 1e-9)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
