"""Timing of the hold-out evaluation of the top-N lists through the coarse ABI (xmap_ctx_evaluate_topn) on a synthetic
workload, beside the host route it replaces: xmap_ctx_recommend for the same users (the [users][n_top] arrays come to the host)
followed by a vectorised NumPy statement of the metrics.  One held-out pair per user with a list, taken from a first
recommendation (positions 0 / 3 / last of the list rated 5 / 4 / 3 by user index % 3).  Wall-clock times of the blocking calls
(each ends with a stream synchronisation), warm, median of --reps.  The split of the device route comes from the same arrays as
device tensors: Engine.eval_users / Engine.topn / Engine.topn_eval under HIP events.

    python profiles/tools/topn_eval_timing.py --workload c2 --out profiles/topn_eval_timing_c2.json"""
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
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--cutoffs", default="5,10,20")
    ap.add_argument("--alpha", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from xmap.engine import device, hipabi as abi, synth
    lib = abi.lib

    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t)) if a is not None else None

    def wall(fn, reps):
        out = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t) * 1e3)
        return float(np.median(out))

    def events(fn, reps):
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return float(np.median(out))
    torch.zeros(1, device="cuda:0")
    t0 = time.perf_counter()

    def note(what):
        print("[%7.1f s] %s" % (time.perf_counter() - t0, what), file=sys.stderr, flush=True)
    r = synth.config_c2() if args.workload == "c2" else synth.config_c1()
    k = args.k or (50 if args.workload == "c2" else 10)
    U, I, keep, n = len(r.user_ptr) - 1, r.n_items, args.keep, args.n
    cuts = np.asarray([int(c) for c in args.cutoffs.split(",")], np.int32)
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
    call("xmap_ctx_item_sim", 0, 50, None, None)
    call("xmap_ctx_extend", k, None, None)
    n_rows = C.c_int64(0)
    call("xmap_ctx_generate", 1, None, None, C.byref(n_rows), None)
    call("xmap_ctx_rec_sim", 50, None)
    call("xmap_ctx_rec_select", keep)
    note("stages A-C and the tail's set-up done")
    n_w = 66
    wtab = np.asarray([np.exp(- args.alpha * d) for d in range(n_w)], np.float64)
    dtab = np.asarray([1.0 / np.log2(x + 2) for x in range(n)], np.float64)

    def recommend(users, n_top):
        Q = len(users)
        cnt, it = np.zeros(Q, np.int32), np.zeros((Q, n_top), np.int32)
        pl, de, st = np.zeros((Q, n_top)), np.zeros((Q, n_top)), np.zeros(4, np.int64)
        call("xmap_ctx_recommend", Q, p(users, C.c_int32), n_top, 0, 0, p(wtab, C.c_double), n_w, p(cnt, C.c_int32), p(it, C.c_int32),
             p(pl, C.c_double), p(de, C.c_double), p(st, C.c_int64))
        return cnt, it, st
    # ---- one held-out pair per user with a list
    everyone = np.arange(U, dtype=np.int32)
    cnt, it, st = recommend(everyone, 10)
    assert st[2] <= n_w
    has = np.nonzero(cnt)[0]
    pos = np.where(has % 3 == 0, 0, np.where(has % 3 == 1, 3, cnt[has] - 1))
    pos = np.minimum(pos, cnt[has] - 1)
    tu, ti = has.astype(np.int32), it[has, pos].astype(np.int32)
    tr = np.where(has % 3 == 0, 5.0, np.where(has % 3 == 1, 4.0, 3.0))
    del cnt, it
    T, n_cut = len(tu), len(cuts)
    agg, cover, stats = np.zeros((n_cut, 8)), np.zeros(n_cut, np.int64), np.zeros(8, np.int64)

    def evaluate():
        call("xmap_ctx_evaluate_topn", T, p(tu, C.c_int32), p(ti, C.c_int32), p(tr, C.c_double), C.c_double(4.0), n, 0, 0,
             p(wtab, C.c_double), n_w, n_cut, p(cuts, C.c_int32), p(dtab, C.c_double), p(agg, C.c_double), p(cover, C.c_int64), None, None,
             p(stats, C.c_int64))
    note("held-out pairs made")
    evaluate()
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": keep, "n_top": n, "cutoffs": cuts.tolist(),
           "alterego_rows": int(n_rows.value), "held_out_pairs": T, "device": torch.cuda.get_device_name(0),
           "stats": stats.tolist(), "reps": args.reps}
    res["evaluate_topn_ms"] = wall(evaluate, args.reps)
    dev_agg, dev_cover = agg.copy(), cover.copy()
    note("device route timed")
    # ---- the host route: the lists come to the host, NumPy scores them
    users = tu[tr >= 4.0]

    def host_lists():
        return recommend(users, n)

    def host_metrics(cnt, it):
        key = users.astype(np.int64)[:, None] * I + it
        rel = np.sort(tu[tr >= 4.0].astype(np.int64) * I + ti[tr >= 4.0])
        n_rel = np.bincount(tu[tr >= 4.0], minlength=U)[users]
        hit = np.isin(key, rel) & (np.arange(n)[None, :] < cnt[:, None])
        out = np.zeros((n_cut, 8))
        cov = np.zeros(n_cut, np.int64)
        pre_d = np.concatenate([[0.0], np.cumsum(dtab)])
        for x, c in enumerate(cuts.tolist()):
            hc = hit[:, :c]
            hcount = hc.sum(1)
            rank = np.arange(1, c + 1)[None, :]
            cn = np.minimum(c, n_rel)
            first = np.where(hcount > 0, hc.argmax(1) + 1, 1)
            out[x] = [len(users), (hcount > 0).sum(), hcount.sum(), (hcount / c).sum(), (hcount / n_rel).sum(),
                      ((hc * dtab[None, :c]).sum(1) / pre_d[cn]).sum(), ((np.cumsum(hc, 1) * hc / rank).sum(1) / cn).sum(),
                      np.where(hcount > 0, 1.0 / first, 0.0).sum()]
            listed = it[:, :c][np.arange(c)[None, :] < cnt[:, None]]
            cov[x] = len(np.unique(listed))
        return out, cov
    lists = host_lists()
    h_agg, h_cover = host_metrics(lists[0], lists[1])
    assert np.array_equal(h_agg[:, :3], dev_agg[:, :3]) and np.array_equal(h_cover, dev_cover), (h_agg, dev_agg, h_cover, dev_cover)
    assert np.allclose(h_agg[:, 3:], dev_agg[:, 3:], rtol=1e-9, atol=0.0)
    res["host_recommend_download_ms"] = wall(host_lists, args.reps)
    res["host_numpy_metrics_ms"] = wall(lambda: host_metrics(lists[0], lists[1]), args.reps)
    res["host_route_ms"] = res["host_recommend_download_ms"] + res["host_numpy_metrics_ms"]
    res["list_bytes_to_host"] = int(len(users)) * n * 20
    del lists
    note("host route timed")
    # ---- the split of the device route, on the same arrays as device tensors
    n_prof = int(n_rows.value)
    pp, pi = np.zeros(U + 1, np.int64), np.zeros(n_prof, np.int32)
    pr, pt = np.zeros(n_prof), np.zeros(n_prof, np.int64)
    call("xmap_ctx_rec_profiles_download", p(pp, C.c_int64), p(pi, C.c_int32), p(pr, C.c_double), p(pt, C.c_int64))
    nc, ncol, nsim = np.zeros(I, np.int32), np.zeros((I, keep), np.int32), np.zeros((I, keep))
    call("xmap_ctx_rec_neighbors_download", p(nc, C.c_int32), p(ncol, C.c_int32), p(nsim, C.c_double), None)
    avg = np.zeros(I)
    call("xmap_ctx_rec_download", None, None, None, None, None, p(avg, C.c_double), None)
    lib.xmap_ctx_destroy(h)
    dev = "cuda:0"
    t = lambda a: torch.from_numpy(a).to(dev)
    P = type("Profiles", (), {})()
    P.n_users, P.n_items, P.user_ptr, P.user_item, P.user_rating64, P.user_time = U, I, t(pp), t(pi), t(pr), t(pt)
    P.device = torch.device(dev)
    eng = device.Engine(P)
    nb, d_avg, d_w = (t(nc), t(ncol), t(nsim)), t(avg), t(wtab)
    d_tu, d_ti, d_tr = t(tu), t(ti), t(tr)
    n_rel, d_users, counts = eng.eval_users(d_tu, d_ti, d_tr, 4.0, U, I)
    out = eng.topn(P, nb, d_users, d_avg, d_w, n)
    m = eng.topn_eval(d_tu, d_ti, d_tr, 4.0, n_rel, d_users, out[0], out[1], cuts.tolist(), I)
    assert np.array_equal(m[2].cpu().numpy(), dev_agg) and np.array_equal(m[3].cpu().numpy(), dev_cover)
    res["eval_users_ms"] = events(lambda: eng.eval_users(d_tu, d_ti, d_tr, 4.0, U, I), args.reps)
    res["topn_rows_ms"] = events(lambda: eng.topn(P, nb, d_users, d_avg, d_w, n), args.reps)
    res["topn_eval_ms"] = events(lambda: eng.topn_eval(d_tu, d_ti, d_tr, 4.0, n_rel, d_users, out[0], out[1], cuts.tolist(), I), args.reps)
    res["evaluation_over_ranking"] = (res["eval_users_ms"] + res["topn_eval_ms"]) / res["topn_rows_ms"]
    res["at"] = {int(c): dict(users=int(dev_agg[x, 0]), hit_rate=dev_agg[x, 1] / dev_agg[x, 0], precision=dev_agg[x, 3] / dev_agg[x, 0],
                              recall=dev_agg[x, 4] / dev_agg[x, 0], ndcg=dev_agg[x, 5] / dev_agg[x, 0], map=dev_agg[x, 6] / dev_agg[x, 0],
                              mrr=dev_agg[x, 7] / dev_agg[x, 0], coverage=int(dev_cover[x])) for x, c in enumerate(cuts.tolist())}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
