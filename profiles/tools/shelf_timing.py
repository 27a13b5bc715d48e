"""Timing of the shelves (Engine.shelves) beside the calls a host would use in their place, on a synthetic workload, with the model
construction and the protocol of related_timing.py: HIP events, a warm-up of every variant, the median of --reps.

    shelves_1 / shelves_2   (a) Engine.shelves for --queries random users with rows: --labels labels, one per item / two per item,
                            n_top --n-top, n_shelf --n-shelf, shelf_by "best"
    topn                    (b) one Engine.topn over the same queries (n_top --n-top): the call the library had before
    masks_1 / masks_2       (c) --labels Engine.topn calls with allow = the items of one label each: the page by the mask route,
                            without the host's ranking of the shelves

--only-shelves runs (a) alone, --reps times after a warm-up: the process a kernel trace is taken of.
A number, not a gate: the process exits with status 0 whatever it measures.  Run it under a time limit of its own:

    timeout -k 10 540 python profiles/tools/shelf_timing.py --workload c2 --out profiles/shelf_timing_c2.json"""
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
    ap.add_argument("--n-shelf", type=int, default=10)
    ap.add_argument("--labels", type=int, default=20)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only-shelves", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from xmap.engine import device, filters, hipabi as abi, synth

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
    # the labels: pseudo-categories by a hash of the item index; the second table adds another label to every item
    L = args.labels
    first = (np.arange(I, dtype=np.int64) * 2654435761 % (1 << 32)) % L
    second = (first + 1 + (np.arange(I, dtype=np.int64) * 40503 % (L - 1))) % L
    tables, masks = {}, {}
    for name, per in (("1", first[:, None]), ("2", np.sort(np.stack([first, second], axis=1), axis=1))):
        lab_ptr = np.arange(I + 1, dtype=np.int64) * per.shape[1]
        tables[name] = e2.set_labels(I, L, lab_ptr, per.reshape(-1).astype(np.int32))
        masks[name] = [torch.from_numpy(filters.pack_mask((per == l).any(axis=1), I).view(np.int32)).to(dev) for l in range(L)]
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": args.keep, "alterego_rows": int(G.n_rows), "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "version": int(abi.lib.xmap_version()), "queries": args.queries, "labels": L,
           "n_top": args.n_top, "n_shelf": args.n_shelf, "shelf_by": "best", "stats": {}, "ms": {}, "ms_all": {}}

    def shelves(name):
        return e2.shelves(P, nb, q, item_avg, wtab, tables[name], args.n_shelf, args.n_top)

    def by_masks(name):
        return [e2.topn(P, nb, q, item_avg, wtab, args.n_top, allow=m) for m in masks[name]]
    variants = [("shelves_1", lambda: shelves("1")), ("shelves_2", lambda: shelves("2"))]
    if not args.only_shelves:
        variants += [("topn", lambda: e2.topn(P, nb, q, item_avg, wtab, args.n_top)), ("masks_1", lambda: by_masks("1")),
                     ("masks_2", lambda: by_masks("2"))]
    for name in ("1", "2"):
        out = shelves(name)
        res["stats"]["shelves_" + name] = [int(x) for x in out[8]]
        res["shelves_returned_" + name] = int(out[0].sum().item())
        if not args.only_shelves:       # the page by the mask route holds the same shelves: every returned shelf is its label's list
            lists = by_masks(name)
            same = True
            nshelf, label, cnt, item = out[0].cpu().numpy(), out[1].cpu().numpy(), out[4].cpu().numpy(), out[5].cpu().numpy()
            ref_cnt = np.stack([l[0].cpu().numpy() for l in lists], axis=1)
            ref_item = np.stack([l[1].cpu().numpy() for l in lists], axis=1)
            for qq in range(args.queries):
                for s in range(int(nshelf[qq])):
                    l = label[qq, s]
                    same &= cnt[qq, s] == ref_cnt[qq, l] and np.array_equal(item[qq, s], ref_item[qq, l])
            res["same_as_masks_" + name] = bool(same)
    times = {v: [] for v, _ in variants}
    for v, fn in variants:
        say("warm-up: " + v)
        once(fn)
    for rep in range(args.reps):
        for v, fn in variants:
            times[v].append(once(fn))
    res["ms"] = {v: float(np.median(t)) for v, t in times.items()}
    res["ms_all"] = {v: [float(x) for x in t] for v, t in times.items()}
    if not args.only_shelves:
        for name in ("1", "2"):
            a, b, c = res["ms"]["shelves_" + name], res["ms"]["topn"], res["ms"]["masks_" + name]
            res["a_minus_b_ms_" + name], res["a_over_b_" + name], res["c_over_a_" + name] = a - b, a / max(b, 1e-9), c / max(a, 1e-9)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
