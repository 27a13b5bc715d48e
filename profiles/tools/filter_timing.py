"""Timing of top-N and audience under eligibility rules (Engine.topn / Engine.audience with allow= / exclude= / min_score=) on the
AlterEgo rows of a synthetic workload, with the protocol of audience_timing.py: HIP events, warm, median of --reps; the --items
most-held listed items for audience, the first --users users with rows for top-N.  The query sets are halved until the
unfiltered call scores at most MAX_PAIRS pairs: when the tool was written the scoring pass was one grid, which from 6.7e7
pairs on has 2^32 threads; the pass is launched in ranges since and the bound stays so that the numbers
compare with the recorded ones.  One call times, alternated rep by rep (each rep starts one variant further on):

    unfiltered      the unfiltered entry (xmap_topn_rows / xmap_audience_rows)
    empty           the _filtered entry with an empty filter {NULL, NULL, NULL, -inf}
                    (both, and the parent's, through one path: ctypes on output tensors made once -- the Engine methods
                    allocate their outputs per call, which the comparison with the parent must not carry)
    mask_1pct       a random 1 % mask
    mask_50pct_ex20_floor   a 50 % mask + 20 exclusions per query + a floor at the median returned score
    parent_1, parent_2      with --parent-lib: the unfiltered entry of ANOTHER build of the library (the parent commit's
                    libxmap_hip.so) on the same device tensors, from two separate loads of it -- their difference is the
                    same-box spread the comparison `unfiltered / empty no slower than the parent` is read against

and records stats[0] (pairs scored) of each variant.  Two conditions are written to the JSON as "conditions" (true / false):
    pairs_1pct      under the 1 % mask the pairs scored are 0.5 % .. 2 % of the unfiltered count (a count, not a time; the share
                    is the mask weighted by how often an id is a candidate, so it is near 1 %, not equal to it)
    unfiltered_no_slower, empty_no_slower   (with --parent-lib) the call's median is at most the mean of the two parent medians
                    times (1 + their relative difference)
and the process exits with status 1 when one of them is false.

    python profiles/tools/filter_timing.py --workload c2 --parent-lib PARENT/libxmap_hip.so --out profiles/filter_timing_c2.json"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))


MAX_PAIRS = 60000000            # pairs of one call: what the recorded runs used (once the limit of a single scoring grid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c1", "c2"])
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--n-topn", type=int, default=10)
    ap.add_argument("--n-audience", type=int, default=100)
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--users", type=int, default=40000)
    ap.add_argument("--alpha", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=12)
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
    cnt, col, sim = [x.contiguous() for x in nb]
    deg = P.user_ptr[1:] - P.user_ptr[:-1]
    hold_cnt = torch.bincount(P.user_item[:P.nnz].long(), minlength=I)
    listed = torch.nonzero(cnt > 0).flatten()
    q_items = listed[torch.argsort(hold_cnt[listed], descending=True, stable=True)[:min(args.items, int(listed.numel()))]].int().contiguous()
    q_users = torch.nonzero(deg > 0).flatten()[:args.users].int().contiguous()
    parent = parent2 = None
    if args.parent_lib:
        # two repeats of the parent = two loads of its library (the second from a copy of the file: a load of its own, with its own
        # arena of temporaries), as two runs of the parent's tools would be; two calls into one load differ by far less
        import shutil
        import tempfile
        copy = os.path.join(tempfile.mkdtemp(), "libxmap_hip_parent2.so")
        shutil.copy(os.path.abspath(args.parent_lib), copy)
        parent, parent2 = C.CDLL(os.path.abspath(args.parent_lib)), C.CDLL(copy)
        for L in (parent, parent2):
            for name in ("xmap_topn_rows", "xmap_audience_rows"):
                getattr(L, name).argtypes = abi.PROTOTYPES[name]
                getattr(L, name).restype = C.c_int
    rng = np.random.default_rng(1)
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": keep, "alterego_rows": int(G.n_rows), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "parent_version": int(parent.xmap_version()) if parent else None,
           "version": int(abi.lib.xmap_version()), "calls": {}}
    ok = True
    for what, call, name, query, n_ids, n_top in (("topn", e2.topn, "xmap_topn_rows", q_users, int(P.n_items), args.n_topn),
                                                   ("audience", e2.audience, "xmap_audience_rows", q_items, int(P.n_users), args.n_audience)):
        say(what)
        base = call(P, nb, query, avg, wtab, n_top)                                   # warm-up
        while base[4][0] > MAX_PAIRS:
            query = query[:int(query.numel()) // 2].contiguous()
            base = call(P, nb, query, avg, wtab, n_top)
        Q = int(query.numel())
        scores = base[2][base[1] >= 0]
        floor = float(scores.median()) if scores.numel() else 0.0
        one_pct = torch.from_numpy(rng.random(n_ids) < 0.01).to(dev)
        half = torch.from_numpy(rng.random(n_ids) < 0.5).to(dev)
        ex = (torch.arange(Q + 1, dtype=torch.int64, device=dev) * 20, torch.from_numpy(rng.integers(0, n_ids, 20 * Q).astype(np.int32)).to(dev))
        o = [torch.empty(Q, dtype=torch.int32, device=dev)] + [torch.empty((Q, n_top), dtype=t, device=dev)
                                                                 for t in (torch.int32, torch.float64, torch.float64)]
        h, h6 = (C.c_int64 * 4)(), (C.c_int64 * 6)()
        no_rules = abi.rec_filter()

        def old(L, filtered=False):     # an entry of a library on the tensors of this process: the unfiltered one, or the filtered one with an empty filter
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            head = [st, Q, abi.vp(query), n_top, 0, 0, int(P.n_users), int(P.n_items), keep, abi.vp(cnt), abi.vp(col), abi.vp(sim),
                    abi.vp(P.user_ptr), abi.vp(P.user_item), abi.vp(P.user_rating64), abi.vp(P.user_time), abi.vp(avg),
                    abi.vp(wtab), int(wtab.numel()), abi.vp(o[0]), abi.vp(o[1]), abi.vp(o[2]), abi.vp(o[3])]
            if filtered:
                tail = ([0, None, None] if what == "audience" else []) + [C.byref(no_rules), h6]
                rc = getattr(L, name + "_filtered")(*(head + tail))
            else:
                rc = getattr(L, name)(*(head + [h]))
            assert rc == 0, rc
            return o[0], o[1], o[2], o[3], tuple(int(x) for x in (h6 if filtered else h))
        variants = [("unfiltered", lambda: old(abi.lib)),
                    ("empty", lambda: old(abi.lib, True)),
                    ("mask_1pct", lambda: call(P, nb, query, avg, wtab, n_top, allow=one_pct)),
                    ("mask_50pct_ex20_floor", lambda: call(P, nb, query, avg, wtab, n_top, allow=half, exclude=ex, min_score=floor))]
        if parent:
            variants += [("parent_1", lambda: old(parent)), ("parent_2", lambda: old(parent2))]
        one = {"queries": Q, "n_top": n_top, "floor": floor, "stats": {}, "ms": {}}
        for v, fn in variants:      # warm-up of every variant, and its counts
            out = fn()
            one["stats"][v] = list(out[4])
            if v in ("unfiltered", "empty", "parent_1"):
                assert all(torch.equal(a, b) for a, b in zip(out[:4], base[:4])) and tuple(out[4][:4]) == tuple(base[4]), v
        # at this size a block of the candidate pass serves many queries: rules that remove nothing (a mask of ones, lists that
        # name only ids outside the id space) must give the unfiltered answer
        nothing = (torch.arange(Q + 1, dtype=torch.int64, device=dev) * 2, torch.tensor([-1, n_ids], dtype=torch.int32, device=dev).repeat(Q))
        out = call(P, nb, query, avg, wtab, n_top, allow=torch.ones(n_ids, dtype=torch.bool, device=dev), exclude=nothing)
        one["stats"]["rules_that_remove_nothing"] = list(out[4])
        assert all(torch.equal(a, b) for a, b in zip(out[:4], base[:4])) and tuple(out[4]) == tuple(base[4]) + (0, 0), out[4]
        times = {v: [] for v, _ in variants}
        for rep in range(args.reps):   # alternated, and every rep starts one variant further on: no variant keeps one neighbour
            for v, fn in variants[rep % len(variants):] + variants[:rep % len(variants)]:
                times[v].append(once(fn))
        one["ms"] = {v: float(np.median(t)) for v, t in times.items()}
        one["pairs_1pct_over_unfiltered"] = one["stats"]["mask_1pct"][0] / max(one["stats"]["unfiltered"][0], 1)
        one["conditions"] = {"pairs_1pct": bool(0.005 <= one["pairs_1pct_over_unfiltered"] <= 0.02)}
        if parent:
            p1, p2 = one["ms"]["parent_1"], one["ms"]["parent_2"]
            one["parent_spread"] = abs(p1 - p2) / min(p1, p2)
            one["parent_ms"] = (p1 + p2) / 2.0
            for v in ("unfiltered", "empty"):
                one[v + "_over_parent"] = one["ms"][v] / one["parent_ms"]
                one["conditions"][v + "_no_slower"] = bool(one[v + "_over_parent"] <= 1.0 + one["parent_spread"])
        ok = ok and all(one["conditions"].values())
        say(json.dumps(one["ms"]))
        res["calls"][what] = one
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
