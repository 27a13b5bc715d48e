"""Timing of fold-in through the coarse ABI at BASELINE configs[1]: xmap_ctx_foldin for batches of 1, 1 000 and 100 000 of the
upload's own profiles (users [s, s + B), s the first user with a list, so that the batch of one is scored),
xmap_ctx_foldin_recommend (n = 10) on them, and xmap_ctx_recommend for the same users --
the yardstick: its code is what it was before fold-in existed, and fold-in ranking runs the same kernels on the same rows.  One
context, trained once; after a warm-up the three calls alternate in one process, --reps times each per batch size.  Wall-clock
times of the blocking calls (each ends with a stream synchronisation): median, and the spread as the 10th / 90th percentile.

    python profiles/tools/foldin_time.py --out profiles/foldin_bench.json"""
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
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.03)
    ap.add_argument("--batches", default="1,1000,100000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from xmap.engine import hipabi as abi, synth
    lib = abi.lib

    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    torch.zeros(1, device="cuda:0")         # (torch opens the device first, as in the tests)
    t0 = time.perf_counter()

    def note(what):
        print("[%7.1f s] %s" % (time.perf_counter() - t0, what), file=sys.stderr, flush=True)
    r = synth.config_c2() if args.workload == "c2" else synth.config_c1()
    k = args.k or (50 if args.workload == "c2" else 10)
    U, I, keep, n = len(r.user_ptr) - 1, r.n_items, args.keep, args.n
    h = C.c_void_p()
    abi.check(lib.xmap_ctx_create(0, C.byref(h)))

    def call(name, *a):
        abi.check(getattr(lib, name)(h, *a))
    pre, suf, msk, flg = [np.ascontiguousarray(a, t) for a, t in zip(r.item_attrs(), (np.int32, np.int32, np.uint32, np.uint8))]
    ptr, item = np.ascontiguousarray(r.user_ptr, np.int64), np.ascontiguousarray(r.item, np.int32)
    rating, when = np.ascontiguousarray(r.rating, np.float32), np.ascontiguousarray(r.time, np.int64)
    call("xmap_ctx_upload_ratings", U, I, p(ptr, C.c_int64), p(item, C.c_int32), p(rating, C.c_float), p(when, C.c_int64),
         p(pre, C.c_int32), p(suf, C.c_int32), p(msk, C.c_uint32), p(flg, C.c_uint8))
    note("workload made and uploaded")
    t_train = time.perf_counter()
    call("xmap_ctx_item_sim", 0, 50, None, None)
    call("xmap_ctx_extend", k, None, None)
    n_rows = C.c_int64(0)
    call("xmap_ctx_generate", 1, None, None, C.byref(n_rows), None)
    call("xmap_ctx_rec_sim", 50, None)
    call("xmap_ctx_rec_select", keep)
    train_ms = (time.perf_counter() - t_train) * 1e3
    note("stages A-C and the tail's set-up done")
    n_w = 66
    wtab = np.asarray([np.exp(- args.alpha * d) for d in range(n_w)], np.float64)

    def lists(name, users):
        Q = len(users)
        cnt, it = np.zeros(Q, np.int32), np.zeros((Q, n), np.int32)
        pl, de, st = np.zeros((Q, n)), np.zeros((Q, n)), np.zeros(4, np.int64)
        call(name, Q, p(users, C.c_int32), n, 0, 0, p(wtab, C.c_double), n_w, p(cnt, C.c_int32), p(it, C.c_int32), p(pl, C.c_double),
             p(de, C.c_double), p(st, C.c_int64))
        return cnt, it, pl, de, st

    def spread(ms):
        return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
                "min_ms": float(np.min(ms))}
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": keep, "n_top": n, "alterego_rows": int(n_rows.value),
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "train_after_upload_ms": train_ms, "batches": {}}
    start = int(np.nonzero(lists("xmap_ctx_recommend", np.arange(min(U, 1000), dtype=np.int32))[0])[0][0])
    res["first_user"] = start
    for B in [min(int(b), U - start) for b in args.batches.split(",")]:
        users = np.arange(B, dtype=np.int32)                    # indices into the batch
        resident = users + np.int32(start)                      # the same users in the upload
        lo = int(ptr[start])
        bptr = np.ascontiguousarray(ptr[start:start + B + 1] - lo)
        nnz = int(bptr[-1])
        bitem, brating, bwhen = item[lo:lo + nnz], rating[lo:lo + nnz], when[lo:lo + nnz]
        counts = np.zeros(3, np.int64)

        def fold():
            call("xmap_ctx_foldin", B, p(bptr, C.c_int64), p(bitem, C.c_int32), p(brating, C.c_float), p(bwhen, C.c_int64), p(counts, C.c_int64))
        for _ in range(3):                  # warm-up; the batch's lists are the resident ones of the same users
            fold()
            a, b = lists("xmap_ctx_foldin_recommend", users), lists("xmap_ctx_recommend", resident)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        ms = {"foldin": [], "foldin_recommend": [], "recommend": []}
        for _ in range(args.reps):
            for what, fn in (("foldin", fold), ("foldin_recommend", lambda: lists("xmap_ctx_foldin_recommend", users)),
                             ("recommend", lambda: lists("xmap_ctx_recommend", resident))):
                t = time.perf_counter()
                fn()
                ms[what].append((time.perf_counter() - t) * 1e3)
        out = {what: spread(v) for what, v in ms.items()}
        out.update(raw_entries=nnz, alterego_rows=int(counts[0]), candidates_scored=int(a[4][0]),
                   foldin_recommend_over_recommend=out["foldin_recommend"]["median_ms"] / out["recommend"]["median_ms"])
        res["batches"][str(B)] = out
        note("batch of %d timed" % B)
    lib.xmap_ctx_destroy(h)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
