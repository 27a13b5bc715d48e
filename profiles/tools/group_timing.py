"""Timing of the group lists (Engine.group_topn) on the AlterEgo rows of a synthetic workload, with the model construction and the
protocol of filter_timing.py: HIP events, a warm-up of every variant, the median of --reps, the variants alternated rep by rep.

    group       --groups groups of --members random users with rows, how = mean, n_top = --n-top
    members     Engine.topn(..., keep_held=True) over the same flattened members (groups * members queries): the work the
                parent commit does for the same scored pairs -- the member pass of the group call plus top-N's own selection

and records both medians, their ratio, the difference (what the two group-only passes -- the groups' candidates through the
bitmap, aggregate-and-select -- cost beyond the member pass, less top-N's selection) and the stats of both calls.  A number, not
a gate: the process exits with status 0 whatever it measures.  Run it under a time limit of its own:

    timeout -k 10 900 python profiles/tools/group_timing.py --workload c2 --out profiles/group_timing_c2.json

With --parent-lib (the protocol of filter_timing.py): three more variants -- xmap_group_topn_rows of this build (group_abi) and of
ANOTHER build of the library (parent_1, parent_2: the parent commit's libxmap_hip.so, from two separate loads of it) on the same
device tensors, through ctypes on output tensors made once -- and the condition
    group_no_slower     the median of group_abi is at most the mean of the two parent medians times (1 + their relative difference)
is written to the JSON under "conditions"; the process exits with status 1 when it is false."""
import argparse
import ctypes as C
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
    ap.add_argument("--groups", type=int, default=100000)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--alpha", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=7)
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
    deg = P.user_ptr[1:] - P.user_ptr[:-1]
    with_rows = torch.nonzero(deg > 0).flatten().cpu().numpy()
    rng = np.random.default_rng(1)
    n_groups, m = args.groups, args.members
    members = torch.from_numpy(with_rows[rng.integers(0, len(with_rows), n_groups * m)].astype(np.int32)).to(dev)
    grp_ptr = (torch.arange(n_groups + 1, dtype=torch.int64, device=dev) * m).contiguous()
    variants = [("group", lambda: e2.group_topn(P, nb, grp_ptr, members, avg, wtab, args.n_top, how="mean")),
                ("members", lambda: e2.topn(P, nb, members, avg, wtab, args.n_top, keep_held=True))]
    parents = []
    if args.parent_lib:
        # two repeats of the parent = two loads of its library (the second from a copy of the file: a load of its own, with its own
        # arena of temporaries); two calls into one load differ by far less
        import shutil
        import tempfile
        copy = os.path.join(tempfile.mkdtemp(), "libxmap_hip_parent2.so")
        shutil.copy(os.path.abspath(args.parent_lib), copy)
        parents = [C.CDLL(os.path.abspath(args.parent_lib)), C.CDLL(copy)]
        for L in parents:
            L.xmap_group_topn_rows.argtypes = abi.PROTOTYPES["xmap_group_topn_rows"]
            L.xmap_group_topn_rows.restype = C.c_int
        cnt, col, sim = [x.contiguous() for x in nb]
        o = [torch.empty(n_groups, dtype=torch.int32, device=dev)] + [torch.empty((n_groups, args.n_top), dtype=t, device=dev)
                                                                        for t in (torch.int32, torch.float64, torch.float64, torch.int32)]
        h8, no_rules = (C.c_int64 * 8)(), abi.rec_filter()

        def rows(L):                # the entry of a library on the tensors of this process: how = mean, no veto, no rules
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            rc = L.xmap_group_topn_rows(st, n_groups, abi.vp(grp_ptr), abi.vp(members), args.n_top, 0, 0, abi.GROUP_MEAN, float("-inf"),
                                        int(P.n_users), int(P.n_items), keep, abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(P.user_ptr),
                                        abi.vp(P.user_item), abi.vp(P.user_rating64), abi.vp(P.user_time), abi.vp(avg), abi.vp(wtab),
                                        int(wtab.numel()), abi.vp(o[0]), abi.vp(o[1]), abi.vp(o[2]), abi.vp(o[3]), abi.vp(o[4]),
                                        C.byref(no_rules), h8)
            assert rc == 0, rc
            return o[0], o[1], o[2], o[3], o[4], [int(x) for x in h8]
        variants += [("group_abi", lambda: rows(abi.lib)), ("parent_1", lambda: rows(parents[0])), ("parent_2", lambda: rows(parents[1]))]
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": keep, "alterego_rows": int(G.n_rows), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()),
           "parent_version": int(parents[0].xmap_version()) if parents else None, "groups": n_groups, "members": m,
           "n_top": args.n_top, "how": "mean", "stats": {}, "ms": {}}
    for v, fn in variants:          # warm-up of every variant, and its counts
        say("warm-up: " + v)
        out = fn()
        res["stats"][v] = [int(x) for x in out[-1]]
        if v == "group":
            base = [x.clone() for x in out[:5]]
        elif v != "members":        # the three calls through ctypes give the Engine's answer
            assert all(torch.equal(a, b) for a, b in zip(out[:5], base)) and res["stats"][v] == res["stats"]["group"], v
    times = {v: [] for v, _ in variants}
    for rep in range(args.reps):    # alternated: every rep starts one variant further on
        for v, fn in variants[rep % len(variants):] + variants[:rep % len(variants)]:
            times[v].append(once(fn))
    res["ms"] = {v: float(np.median(t)) for v, t in times.items()}
    res["ms_all"] = {v: [float(x) for x in t] for v, t in times.items()}
    res["group_over_members"] = res["ms"]["group"] / res["ms"]["members"]
    res["group_minus_members_ms"] = res["ms"]["group"] - res["ms"]["members"]
    ok = True
    if parents:
        p1, p2 = res["ms"]["parent_1"], res["ms"]["parent_2"]
        res["parent_spread"] = abs(p1 - p2) / min(p1, p2)
        res["parent_ms"] = (p1 + p2) / 2.0
        res["group_abi_over_parent"] = res["ms"]["group_abi"] / res["parent_ms"]
        ok = bool(res["group_abi_over_parent"] <= 1.0 + res["parent_spread"])
        res["conditions"] = {"group_no_slower": ok}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
