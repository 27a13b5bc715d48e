"""Timing of the explanation call through the coarse ABI, as a foreign host pays for it: xmap_ctx_explain (n_ev = 3, n_src = 4)
over the pairs of the top-10 lists of 10^5 users, and next to it xmap_ctx_predict over the SAME pairs in the same process -- the
yardstick: the prediction's kernel and host code are untouched by the explanation.  Both calls include their host-to-device and
device-to-host copies (that is what the call costs); wall clock, warm, median and 10th / 90th percentile of --reps repetitions,
interleaved so that neither side gets the quieter half of the run.

The device time of the explanation is then split into evidence (xmap_explain_rows) and sources (xmap_explain_sources) with HIP
events around the two fine-grained calls (Engine.explain / Engine.explain_sources) on device copies of what the context
holds: the downloaded profiles, lists and averages, the upload's own CSR, the map derived from the downloaded choice.

    python profiles/tools/explain_timing.py --workload c2 --out profiles/explain_bench.json"""
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
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--n-ev", type=int, default=3)
    ap.add_argument("--n-src", type=int, default=4)
    ap.add_argument("--alpha", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from xmap.engine import device, hipabi as abi, synth
    lib = abi.lib

    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t)) if a is not None else None

    def call(name, *a):
        abi.check(getattr(lib, name)(h, *a))
    torch.zeros(1, device="cuda:0")
    r = synth.config_c2() if args.workload == "c2" else synth.config_c1()
    k = args.k or (50 if args.workload == "c2" else 10)
    U, I, keep, n_ev, n_src = r.n_users, r.n_items, args.keep, args.n_ev, args.n_src
    pre, suf, mask, flags = [np.ascontiguousarray(a, t) for a, t in zip(r.item_attrs(), (np.int32, np.int32, np.uint32, np.uint8))]
    ptr, item = np.ascontiguousarray(r.user_ptr, np.int64), np.ascontiguousarray(r.item, np.int32)
    rating, when = np.ascontiguousarray(r.rating, np.float32), np.ascontiguousarray(r.time, np.int64)
    h = C.c_void_p()
    abi.check(lib.xmap_ctx_create(0, C.byref(h)))
    call("xmap_ctx_upload_ratings", U, I, p(ptr, C.c_int64), p(item, C.c_int32), p(rating, C.c_float), p(when, C.c_int64),
         p(pre, C.c_int32), p(suf, C.c_int32), p(mask, C.c_uint32), p(flags, C.c_uint8))
    call("xmap_ctx_item_sim", 0, 50, None, None)
    call("xmap_ctx_extend", k, None, None)
    choice, n_rows, n_tgt = np.zeros(I, np.int32), C.c_int64(0), C.c_int64(0)
    call("xmap_ctx_generate", 1, None, p(choice, C.c_int32), C.byref(n_rows), C.byref(n_tgt))
    call("xmap_ctx_rec_sim", 50, None)
    call("xmap_ctx_rec_select", keep)
    n = n_rows.value
    pf_ptr, pf_item, pf_rating, pf_time = np.zeros(U + 1, np.int64), np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int64)
    call("xmap_ctx_rec_profiles_download", p(pf_ptr, C.c_int64), p(pf_item, C.c_int32), p(pf_rating, C.c_double), p(pf_time, C.c_int64))
    # the lists of the first --users users with rows
    query = np.nonzero(np.diff(pf_ptr) > 0)[0][:args.users].astype(np.int32)
    Q = len(query)
    w = np.asarray([np.exp(- args.alpha * d) for d in range(66)], np.float64)
    l_cnt, l_item = np.zeros(Q, np.int32), np.zeros((Q, args.n), np.int32)
    l_plain, l_decay, stats = np.zeros((Q, args.n)), np.zeros((Q, args.n)), np.zeros(4, np.int64)
    call("xmap_ctx_recommend", Q, p(query, C.c_int32), args.n, 0, 0, p(w, C.c_double), 66, p(l_cnt, C.c_int32), p(l_item, C.c_int32),
         p(l_plain, C.c_double), p(l_decay, C.c_double), p(stats, C.c_int64))
    filled = np.arange(args.n)[None, :] < l_cnt[:, None]
    pu = np.ascontiguousarray(np.repeat(query, l_cnt))
    pi = np.ascontiguousarray(l_item[filled])
    T = len(pu)
    o_plain, o_decay, o_status = np.zeros(T), np.zeros(T), np.zeros(T, np.int32)
    x_status, x_total, x_cnt, x_score = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T)
    x_row, x_slot, x_share = np.zeros((T, n_ev), np.int64), np.zeros((T, n_ev), np.int32), np.zeros((T, n_ev))
    s_total, s_pos = np.zeros((T, n_ev), np.int32), np.zeros((T, n_ev, max(n_src, 1)), np.int64)

    def predict():
        call("xmap_ctx_predict", T, p(pu, C.c_int32), p(pi, C.c_int32), None, p(w, C.c_double), 66, p(o_plain, C.c_double),
             p(o_decay, C.c_double), p(o_status, C.c_int32), None, None)

    def explain():
        call("xmap_ctx_explain", T, p(pu, C.c_int32), p(pi, C.c_int32), 0, n_ev, n_src, p(w, C.c_double), 66, p(x_status, C.c_int32),
             p(x_total, C.c_int32), p(x_cnt, C.c_int32), p(x_score, C.c_double), p(x_row, C.c_int64), p(x_slot, C.c_int32),
             p(x_share, C.c_double), p(s_total, C.c_int32), p(s_pos, C.c_int64), None)
    predict(); explain(); predict(); explain()                                          # warm
    assert np.array_equal(o_status, x_status)
    t_pred, t_expl = [], []
    for _ in range(args.reps):
        for fn, out in ((predict, t_pred), (explain, t_expl)):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)

    def summary(ms):
        return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90))}
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": keep, "n_top": args.n, "n_ev": n_ev, "n_src": n_src,
           "alterego_rows": int(n), "mapped_rows": int(n - n_tgt.value), "query_users": Q, "pairs": T, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "mean_evidence_per_pair": float(x_total.mean()) if T else 0.0,
           "largest_evidence": int(x_total.max()) if T else 0, "entries_reported": int(x_cnt.sum()),
           "ctx_predict_wall": summary(t_pred), "ctx_explain_wall": summary(t_expl)}
    res["explain_over_predict"] = res["ctx_explain_wall"]["median_ms"] / res["ctx_predict_wall"]["median_ms"]
    # ---- the device time of the two passes, HIP events around the fine-grained calls on device copies
    cnt, col, sim, avg = np.zeros(I, np.int32), np.zeros((I, keep), np.int32), np.zeros((I, keep)), np.zeros(I)
    call("xmap_ctx_rec_neighbors_download", p(cnt, C.c_int32), p(col, C.c_int32), p(sim, C.c_double), None)
    call("xmap_ctx_rec_download", None, None, None, None, None, p(avg, C.c_double), None)
    m = np.full(I, -1, np.int32)
    for s in range(I):
        if choice[s] >= 0:
            m[choice[s]] = s
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    eng = object.__new__(device.Engine)
    eng.dev, eng.timers, eng._scratch = "cuda:0", {}, {}
    import types
    P = types.SimpleNamespace(n_users=U, n_items=I, user_ptr=to(pf_ptr), user_item=to(pf_item), user_rating64=to(pf_rating), user_time=to(pf_time))
    user_of = np.repeat(np.arange(U), np.diff(ptr))
    cnt_t = np.bincount(user_of[(flags[item] & 2) != 0], minlength=U).astype(np.int32)      # pass-through rows per profile
    res["entries_from_mapped_rows"] = int(((x_row >= 0) & (x_row - pf_ptr[pu][:, None] >= cnt_t[pu][:, None])).sum())
    src = (to(ptr), to(item), to(cnt_t), None, to(flags), to(m))
    nb, d_u, d_i, d_avg, d_w = (to(cnt), to(col), to(sim)), to(pu), to(pi), to(avg), to(w)
    for _ in range(args.reps + 2):
        out = eng.explain(P, nb, d_u, d_i, d_avg, d_w, n_ev, 0)
        if n_src:
            eng.explain_sources(P, d_u, out[2], out[4], n_src, sources=src)
    ms = eng.timer_ms()
    assert np.array_equal(out[4].cpu().numpy(), x_row)
    res["evidence_device"] = summary(ms["explain_rows"][2:])
    if n_src:
        res["sources_device"] = summary(ms["explain_sources"][2:])
    lib.xmap_ctx_destroy(h)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
