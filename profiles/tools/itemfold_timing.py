"""Timing of the item fold-in on the AlterEgo rows of a synthetic workload, with the tail resident in a coarse context: for two
batches of new items -- --items copies of random target items that have a list, and copies of the --heavy most-held items --
the milliseconds of xmap_itemfold_count, xmap_itemfold_fill and xmap_rec_select over the batch's rows (HIP events around the
fine-grained calls on device copies of the context's profiles and norms), of the coarse call xmap_ctx_item_foldin (host
clock: it takes host arrays and syncs), and beside them xmap_ctx_rec_sim + xmap_ctx_rec_select on the same context -- the
cheapest resident pass that could otherwise give an item a list.  Warm, median of --reps.

    python profiles/tools/itemfold_timing.py --workload c2 --out profiles/itemfold_timing_c2.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/tools/itemfold_timing.py --workload c2 --reps 3

The second command is a run of its own (tracing slows the host): its kernel statistics split the time into expand (k_if_expand),
sort passes (k_rs_hist, k_rs_scatter and the scans) and reduce (k_if_reduce)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c1", "c2"])
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--cap", type=int, default=50)
    ap.add_argument("--items", type=int, default=1000)
    ap.add_argument("--heavy", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from xmap.engine import hipabi as abi, synth
    lib, check, vp, i32, i64 = abi.lib, abi.check, abi.vp, abi.i32, abi.i64

    def P(a, t):
        return a.ctypes.data_as(C.POINTER(t)) if a is not None else None

    def say(what):                  # progress on stderr: the workload takes minutes to make and to train
        sys.stderr.write(what + "\n")
        sys.stderr.flush()

    def clock_ms(fn, reps):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(out))

    def events_ms(fn, reps):
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return float(np.median(out))
    dev = "cuda:0"
    torch.zeros(1, device=dev)
    say("making the workload")
    r = synth.config_c2() if args.workload == "c2" else synth.config_c1()
    k = args.k or (50 if args.workload == "c2" else 10)
    U, I, keep, cap = r.n_users, r.n_items, args.keep, args.cap
    ctx = C.c_void_p()
    check(lib.xmap_ctx_create(0, C.byref(ctx)))
    say("upload and stages A-C")
    pre, suf, mask, flags = [np.ascontiguousarray(a, t) for a, t in zip(r.item_attrs(), (np.int32, np.int32, np.uint32, np.uint8))]
    ptr, item = np.ascontiguousarray(r.user_ptr, np.int64), np.ascontiguousarray(r.item, np.int32)
    rating, tm = np.ascontiguousarray(r.rating, np.float32), np.ascontiguousarray(r.time, np.int64)
    check(lib.xmap_ctx_upload_ratings(ctx, U, I, P(ptr, C.c_int64), P(item, C.c_int32), P(rating, C.c_float), P(tm, C.c_int64),
                                      P(pre, C.c_int32), P(suf, C.c_int32), P(mask, C.c_uint32), P(flags, C.c_uint8)))
    check(lib.xmap_ctx_item_sim(ctx, 0, 50, None, None))
    check(lib.xmap_ctx_extend(ctx, k, None, None))
    n_rows = C.c_int64(0)
    check(lib.xmap_ctx_generate(ctx, 1, None, P(np.zeros(I, np.int32), C.c_int32), C.byref(n_rows), None))
    n_rows = n_rows.value
    say("the resident pass over %d AlterEgo rows" % n_rows)

    def resident():
        check(lib.xmap_ctx_rec_sim(ctx, cap, None))
        check(lib.xmap_ctx_rec_select(ctx, keep))
    resident()
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": keep, "cap": cap, "alterego_rows": n_rows,
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "batches": {}}
    res["ctx_rec_sim_ms"] = clock_ms(lambda: check(lib.xmap_ctx_rec_sim(ctx, cap, None)), args.reps)
    res["ctx_rec_select_ms"] = clock_ms(lambda: check(lib.xmap_ctx_rec_select(ctx, keep)), args.reps)
    pptr, pitem, prating = np.zeros(U + 1, np.int64), np.zeros(n_rows, np.int32), np.zeros(n_rows)
    check(lib.xmap_ctx_rec_profiles_download(ctx, P(pptr, C.c_int64), P(pitem, C.c_int32), P(prating, C.c_double), None))
    norm, cnt = np.zeros(I), np.zeros(I, np.int32)
    check(lib.xmap_ctx_rec_download(ctx, None, None, None, None, None, None, P(norm, C.c_double)))
    check(lib.xmap_ctx_rec_neighbors_download(ctx, P(cnt, C.c_int32), None, None, None))
    # the holders of every item: users ascending, profile order (a stable sort of the rows by item)
    order = np.argsort(pitem, kind="stable")
    hold_cnt = np.bincount(pitem, minlength=I)
    hold_ptr = np.concatenate([[0], np.cumsum(hold_cnt)])
    owner = np.repeat(np.arange(U, dtype=np.int32), np.diff(pptr))[order]
    hrating = prating[order]
    listed = np.nonzero(cnt > 0)[0]
    sets = {"random": listed[np.random.default_rng(1).permutation(len(listed))[:args.items]],
            "most_held": listed[np.argsort(- hold_cnt[listed], kind="stable")[:args.heavy]]}
    d_pptr, d_pitem, d_prating, d_norm = [torch.from_numpy(a).to(dev) for a in (pptr, pitem, prating, norm)]
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for name, items in sets.items():
        say("a batch of copies of the %s items" % name)
        B = len(items)
        bptr = np.concatenate([[0], np.cumsum(hold_cnt[items])]).astype(np.int64)
        pick = np.concatenate([np.arange(hold_ptr[i], hold_ptr[i + 1]) for i in items])
        buser, brating = np.ascontiguousarray(owner[pick]), np.ascontiguousarray(hrating[pick])
        d_bptr, d_buser, d_brating = [torch.from_numpy(a).to(dev) for a in (bptr, buser, brating)]
        nnz = len(buser)
        d_cnt = torch.zeros(max(B, 1), dtype=torch.int32, device=dev)
        d_row = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        h = (C.c_int64 * 3)(0, 0, 0)

        def count():
            check(lib.xmap_itemfold_count(st, i64(B), i64(nnz), vp(d_bptr), vp(d_buser), i64(U), i32(I), vp(d_pptr), vp(d_pitem), i64(0),
                                          vp(d_cnt), vp(d_row), h))
        count()
        n = int(h[0])
        d_col, d_nij = [torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for _ in range(2)]
        d_sim, d_ls = [torch.zeros(max(n, 1), dtype=torch.float64, device=dev) for _ in range(2)]
        d_avg, d_nrm = [torch.zeros(max(B, 1), dtype=torch.float64, device=dev) for _ in range(2)]
        o_cnt = torch.zeros(max(B, 1), dtype=torch.int32, device=dev)
        o_col = torch.zeros((max(B, 1), keep), dtype=torch.int32, device=dev)
        o_sim, o_ls = [torch.zeros((max(B, 1), keep), dtype=torch.float64, device=dev) for _ in range(2)]

        def fill():
            check(lib.xmap_itemfold_fill(st, i64(B), i64(nnz), vp(d_bptr), vp(d_buser), vp(d_brating), i64(U), i32(I), vp(d_pptr), vp(d_pitem),
                                         vp(d_prating), vp(d_norm), i32(cap), i64(0), vp(d_row), vp(d_col), vp(d_sim), vp(d_ls), vp(d_nij),
                                         vp(d_avg), vp(d_nrm)))

        def select():
            check(lib.xmap_rec_select(st, i32(B), vp(d_row), vp(d_col), vp(d_sim), vp(d_ls), i32(keep), vp(o_cnt), vp(o_col), vp(o_sim),
                                      vp(o_ls)))
        fill()
        select()
        one = {"items": B, "ratings": nnz, "records": int(h[1]), "pairs": n, "items_with_a_pair": int(h[2]),
               "largest_run": int(d_nij.max().item()) if n else 0, "holders_of_the_most_held": int(hold_cnt[items].max())}
        one["count_ms"] = events_ms(count, args.reps)
        one["fill_ms"] = events_ms(fill, args.reps)
        one["select_ms"] = events_ms(select, args.reps)
        counts = np.zeros(3, np.int64)

        def coarse():
            check(lib.xmap_ctx_item_foldin(ctx, B, P(bptr, C.c_int64), P(buser, C.c_int32), P(brating, C.c_double), P(counts, C.c_int64)))
        coarse()
        assert counts.tolist() == [n, int(h[1]), int(h[2])], (counts.tolist(), list(h))
        one["ctx_item_foldin_ms"] = clock_ms(coarse, args.reps)
        one["ctx_item_foldin_over_resident_pass"] = one["ctx_item_foldin_ms"] / (res["ctx_rec_sim_ms"] + res["ctx_rec_select_ms"])
        say(json.dumps(one))
        res["batches"][name] = one
    lib.xmap_ctx_destroy(ctx)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
