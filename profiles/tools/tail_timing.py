"""Timing of the device-resident recommender tail (Engine.alterego_profiles -> rec_sim -> rec_select -> predict -> mae)
per step, HIP-event times, on the AlterEgo rows of a synthetic workload; beside it the wall clock of the host-converting
route for the same inputs (AlterEgoRDD.collect() -> rec_sim_from_profiles -> RecommenderPrediction._device_recommendation)
and the thread-per-pair kernel (xmap_predict) against the wave-per-pair one (xmap_predict_rows) on identical arrays.

    python profiles/tools/tail_timing.py --workload c2 --out profiles/tail_timing_c2.json [--host-route]

--host-route builds Python records for every row: minutes at c2, so it is meant for --workload c1."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "x-map_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from xmap.engine import device, hipabi as abi, synth  # noqa: E402


def med(v):
    return float(np.median(v))


def events(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2", choices=["c1", "c2"])
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--keep", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-route", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    r = synth.config_c2() if args.workload == "c2" else synth.config_c1()
    k = args.k or (50 if args.workload == "c2" else 10)
    U, I = r.n_users, r.n_items
    R = device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, I, r.item_attrs(), "cuda:0")
    eng = device.Engine(R)
    S = eng.item_sim("cosine", 50)
    E = eng.extend(S, k)
    _, _, mp = eng.select(E, True)
    G = eng.alterego(mp)
    del S, E
    res = {"workload": args.workload, "users": U, "items": I, "k": k, "keep": args.keep, "alterego_rows": int(G.n_rows),
           "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(1)
    held = torch.unique(G.item).cpu().numpy()
    tu = torch.arange(U, dtype=torch.int32, device="cuda:0")                       # about one pair per user
    ti = torch.from_numpy(rng.choice(held, U).astype(np.int32)).to("cuda:0")
    real = torch.from_numpy(rng.integers(1, 6, U).astype(np.float64)).to("cuda:0")
    wtab = torch.from_numpy(np.asarray([np.exp(- args.alpha * d) for d in range(66)], np.float64)).to("cuda:0")
    steps = {}
    state = {}

    def tail():
        P = eng.alterego_profiles(G)
        e2 = device.Engine(P)
        e2.timers = eng.timers
        Sr = e2.rec_sim(50)
        nb = e2.rec_select(Sr, args.keep)
        avg = Sr.info[:I, 0].contiguous()
        out = e2.predict(P, nb, tu, ti, avg, wtab)
        m = e2.mae(out[2], real, out[0], out[1])
        state.update(P=P, nb=nb, avg=avg, out=out, mae=m.tolist(), pairs=int(Sr.row_ptr[I].item()))
    tail()                                                                          # warm-up
    for _ in range(args.reps):
        eng.timers = {}
        tail()
        for name, v in eng.timer_ms().items():
            steps.setdefault(name, []).append(sum(v))
    eng.timers = None
    group = {"profiles": ["rec_profiles"], "rec_sim": ["rec_stats", "layout3", "tri_plan", "pair_tri", "mir_count", "scatter"],
             "select": ["rec_select"], "predict": ["predict_rows"], "mae": ["mae"]}
    res["new_route_ms"] = {g: sum(med(steps[n]) for n in names if n in steps and n != "rec_stats") if g == "rec_sim"
                           else sum(med(steps[n]) for n in names if n in steps) for g, names in group.items()}
    res["new_route_events_ms"] = {n: med(v) for n, v in steps.items()}
    res["rec_pairs"] = state["pairs"]
    res["status_counts"] = torch.bincount(state["out"][2], minlength=3).tolist()
    res["max_now"] = state["out"][3]
    res["mae"] = state["mae"]
    # ---- thread per pair (xmap_predict) against wave per pair (xmap_predict_rows), identical arrays
    P, (cnt, col, sim), avg = state["P"], state["nb"][:3], state["avg"]
    keep = args.keep
    user_of = torch.repeat_interleave(torch.arange(U, device="cuda:0"), P.user_ptr[1:] - P.user_ptr[:-1])
    o = torch.sort(P.user_item.long() * U + user_of, stable=True)[1]
    rt_ptr = torch.zeros(I + 1, dtype=torch.int64, device="cuda:0")
    rt_ptr[1:] = torch.cumsum(torch.bincount(P.user_item.long(), minlength=I), 0)
    rt_user, rt_rating = user_of[o].int().contiguous(), P.user_rating64[o].contiguous()
    rt_time = P.user_time[o].double().contiguous()
    nb_ptr = torch.zeros(I + 1, dtype=torch.int64, device="cuda:0")
    nb_ptr[1:] = torch.cumsum(cnt.long(), 0)
    mask = torch.arange(keep, device="cuda:0")[None, :] < cnt[:, None]
    nb_item, nb_sim = col[mask].contiguous(), sim[mask].contiguous()
    ti_old = torch.where(cnt[ti.long()] > 0, ti, torch.full_like(ti, -1))
    T = int(tu.numel())
    plain, decay = torch.zeros(T, dtype=torch.float64, device="cuda:0"), torch.zeros(T, dtype=torch.float64, device="cuda:0")
    status = torch.zeros(T, dtype=torch.int32, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = abi.vp

    def old():
        abi.check(abi.lib.xmap_predict(st, abi.i64(T), vp(tu), vp(ti_old), vp(nb_ptr), vp(nb_item), vp(nb_sim), vp(rt_ptr), vp(rt_user),
                                       vp(rt_rating), vp(rt_time), vp(avg), vp(wtab), abi.i32(66), vp(plain), vp(decay), vp(status)))
    e2 = device.Engine(P)
    old()
    torch.cuda.synchronize()
    same = bool(torch.equal(status, state["out"][2]) and torch.equal(plain, state["out"][0]) and torch.equal(decay, state["out"][1]))
    res["kernel_ms"] = {"xmap_predict (thread per pair)": med(events(old, args.reps)),
                        "xmap_predict_rows (wave per pair)": med(events(lambda: e2.predict(P, (cnt, col, sim), tu, ti, avg, wtab), args.reps)),
                        "same_results": same, "old_status_counts": torch.bincount(status, minlength=3).tolist()}
    # ---- the host-converting route, wall clock
    if args.host_route:
        from xmap.core.recommenderPrediction import RecommenderPrediction
        from xmap.core.recommenderPrivacy import RecommenderPrivacy
        from xmap.core.recommenderSim import RecommenderSim
        from xmap.engine import session
        from xmap.engine.localrdd import LocalRDD

        class B(object):
            def __init__(self, v):
                self.value = v
        stt = session.TrainState(r.train_records())
        _, _, mp2 = stt.engine.select(stt.engine.extend(stt.engine.item_sim("cosine", 50), k), True)
        ae = session.AlterEgoRDD(stt, stt.engine.alterego(mp2))
        uids, iids = stt.idt.uids, stt.idt.iids
        tu_h, ti_h, real_h = tu.cpu().numpy(), ti.cpu().numpy(), real.cpu().numpy()
        test = [(uids[u], [(iids[i], float(x))]) for u, i, x in zip(tu_h, ti_h, real_h)]
        wall = {}

        def clock(name, f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            wall[name] = (time.perf_counter() - t0) * 1e3
            return out
        rows = clock("AlterEgoRDD.collect", ae.collect)
        rs = RecommenderSim("cosine_item", 50)
        user_based = clock("build user profiles", lambda: rs.build_sthbased_profile(LocalRDD(rows), "user").cache())
        item_based = clock("build item profiles + info", lambda: (
            rs.build_sthbased_profile(LocalRDD(rows), "item").collectAsMap(),
            rs.get_info(rs.build_sthbased_profile(LocalRDD(rows), "item")).collectAsMap()))
        simr = clock("rec_sim_from_profiles", lambda: session.rec_sim_from_profiles(user_based, 50))
        pol = RecommenderPrivacy(keep, 0.6, 0.1)
        sel = clock("select + dict", lambda: dict(pol.nonnoise_perturbation(pol.nonprivate_neighbor_selection(simr)).collect()))
        tool = RecommenderPrediction(args.alpha, "cosine_item")
        pred = clock("_device_recommendation", lambda: tool._device_recommendation(LocalRDD(test), B(item_based[0]), B(sel), B(item_based[1])))
        clock("calculate_mae", lambda: tool.calculate_mae(pred))
        res["host_route_wall_ms"] = wall
        res["host_route_total_ms"] = sum(wall.values())
        t0 = time.perf_counter()
        out = session.recommend(ae, LocalRDD(test), 50, keep, args.alpha)
        torch.cuda.synchronize()
        res["session_recommend_wall_ms"] = (time.perf_counter() - t0) * 1e3
        res["session_recommend_mae"] = list(out.mae)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
