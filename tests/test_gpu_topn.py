"""Top-N recommendation on the device (csrc/stage_e_topn.hip; xmap_topn_rows, xmap_ctx_recommend, Engine.topn,
session.recommend_topn): per query user the N best items its own rows give evidence for, ranked by the unrounded prediction.

The expected lists are a brute-force Python statement fed only with downloaded arrays (profiles, neighbour lists, averages):
for each query user and every item with a list the evidence is gathered as RecommenderPrediction._predict_pair gathers it,
plain = base + sum(e0) / sum(e1) with Python's sum, decayed = base + RecommenderPrediction._decayed_ratio(evidence) (pinned to the
reference in test_cpu_downstream.py), then sorted(key=(-score, item))[:n].  Items are compared exactly, scores as uint64
views, and bound_rating of the returned scores must be what xmap_ctx_predict / xmap_predict_rows return for the same pair."""
import ctypes as C
import datetime
import math
import os
import re
import warnings

import numpy as np
import pytest

from golden_util import CAP
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_coarse_oracle import stage_c
from test_gpu_recsim import _B, _prediction_case
from test_gpu_tail import _case_arrays, _few_times, _predict_rows, generate, predict, rec_sim, select, wtab

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TN_WINDOW = 1 << 19         # items per bitmap pass of the candidate kernel (csrc/stage_e_topn.hip)
KEEP_HELD = 1


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


# ---------------------------------------------------------------------------------------------- the brute-force statement
def _tool(alpha):
    from xmap.core.recommenderPrediction import RecommenderPrediction
    return RecommenderPrediction(alpha, "cosine_item")


def score_user(tool, rows, cnt, col, sim, avg, keep):
    """every item with a list against one user's profile rows [(item, rating, time)*]: [(item, plain, decayed, now, held)*] in
    ascending item order for the items with evidence; plain is None where the Python statement raises or leaves the numbers.
    (The vectorised test only skips items whose evidence list would be empty.)"""
    I = len(cnt)
    by_item = {}
    for it, ra, tm in rows:
        by_item.setdefault(it, []).append((ra, tm))
    if not by_item:
        return []
    held = np.zeros(I, bool)
    held[[it for it in by_item if 0 <= it < I]] = True
    width = np.minimum(np.maximum(cnt, 0), keep)
    valid = (np.arange(col.shape[1])[None, :] < width[:, None]) & (col >= 0) & (col < I)
    has = (valid & held[np.where(valid, col, 0)]).any(axis=1)
    out = []
    for i in np.nonzero(has)[0].tolist():
        base = float(avg[i])
        ev = []
        for t in range(int(width[i])):
            nb = int(col[i, t])
            if not 0 <= nb < I:
                continue
            s, navg = float(sim[i, t]), float(avg[nb])
            for ra, tm in by_item.get(nb, ()):
                ev.append((s * (ra - navg), abs(s), tm))
        assert ev
        now = len({e[2] for e in ev}) + 1
        try:
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                plain = base + sum(e[0] for e in ev) / sum(e[1] for e in ev)
                decayed = float(base + tool._decayed_ratio(ev))
            if not (math.isfinite(plain) and math.isfinite(decayed)):
                plain = decayed = None
        except ZeroDivisionError:
            plain = decayed = None
        out.append((i, plain, decayed, now, bool(held[i])))
    return out


def score_users(alpha, users, ptr, pit, pra, pti, cnt, col, sim, avg, keep):
    """{user: score_user(...)} for the distinct users with rows"""
    tool, out = _tool(alpha), {}
    U = len(ptr) - 1
    pit, pra, pti = pit.tolist(), pra.tolist(), pti.tolist()
    for u in sorted({int(u) for u in users if 0 <= u < U}):
        a, b = int(ptr[u]), int(ptr[u + 1])
        out[u] = score_user(tool, list(zip(pit[a:b], pra[a:b], pti[a:b])), cnt, col, sim, avg, keep)
    return out


def expected(scored, queries, n, rank_by, keep_held, n_w):
    """(lists [[(item, plain, decayed)*]*], stats) of the queries"""
    lists, n_scored, dropped, max_now, widest = [], 0, 0, 0, 0
    for u in queries:
        cand = [c for c in scored.get(int(u), []) if keep_held or not c[4]]
        n_scored += len(cand)
        widest = max(widest, len(cand))
        max_now = max([max_now] + [c[3] for c in cand])
        kept = [c for c in cand if c[1] is not None and c[3] <= n_w]
        dropped += len(cand) - len(kept)
        kept.sort(key=lambda c: (- c[1 + rank_by], c[0]))
        lists.append([(c[0], c[1], c[2]) for c in kept[:n]])
    return lists, (n_scored, dropped, max_now, widest)


def check_output(out, want, n):
    cnt, item, plain, decay = out[:4]
    lists, stats = want
    assert cnt.tolist() == [len(l) for l in lists]
    for q, l in enumerate(lists):
        k = len(l)
        assert item[q, :k].tolist() == [c[0] for c in l], q
        assert np.array_equal(plain[q, :k].view(np.uint64), np.asarray([c[1] for c in l], np.float64).view(np.uint64)), q
        assert np.array_equal(decay[q, :k].view(np.uint64), np.asarray([c[2] for c in l], np.float64).view(np.uint64)), q
        assert (item[q, k:] == -1).all() and not plain[q, k:].any() and not decay[q, k:].any()
    if len(out) > 4 and out[4] is not None:
        assert tuple(out[4]) == tuple(stats)


# ------------------------------------------------------------------------------------------------------- the drivers
def recommend(ctx, queries, n, rank_by, flags, alpha, n_w=66):
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    cnt, item = np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32)
    plain, decay, stats = np.full((Q, n), -7.0), np.full((Q, n), -7.0), np.zeros(4, np.int64)
    ctx.call("xmap_ctx_recommend", Q, _p(q, C.c_int32), n, rank_by, flags, _p(w, C.c_double), n_w, _p(cnt, C.c_int32),
             _p(item, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), _p(stats, C.c_int64))
    return cnt, item, plain, decay, stats.tolist()


def topn_rows(arrays, n_users, n_items, keep, alpha, n_w, queries, n, rank_by=0, flags=0):
    """xmap_topn_rows on device copies of (ptr, item, rating, time, cnt, col, sim, avg, ...)"""
    import torch
    from xmap.engine import hipabi as abi
    dev = "cuda:0"
    ptr, pit, pra, pti, cnt, col, sim, avg = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays[:8]]
    q = torch.from_numpy(np.ascontiguousarray(queries, np.int32)).to(dev)
    Q = int(q.numel())
    w = torch.from_numpy(wtab(alpha, n_w)).to(dev)
    o_cnt = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    o_item = torch.full((Q, n), -7, dtype=torch.int32, device=dev)
    o_plain = torch.full((Q, n), -7.0, dtype=torch.float64, device=dev)
    o_decay = torch.full((Q, n), -7.0, dtype=torch.float64, device=dev)
    h = (C.c_int64 * 4)(0, 0, 0, 0)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    abi.check(abi.lib.xmap_topn_rows(st, abi.i64(Q), abi.vp(q), abi.i32(n), abi.i32(rank_by), abi.i32(flags), abi.i64(n_users),
                                     abi.i32(n_items), abi.i32(keep), abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ptr), abi.vp(pit),
                                     abi.vp(pra), abi.vp(pti), abi.vp(avg), abi.vp(w), abi.i32(n_w), abi.vp(o_cnt), abi.vp(o_item),
                                     abi.vp(o_plain), abi.vp(o_decay), h))
    return o_cnt.cpu().numpy(), o_item.cpu().numpy(), o_plain.cpu().numpy(), o_decay.cpu().numpy(), [int(x) for x in h]


def test_the_window_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "x-map_amd", "csrc", "stage_e_topn.hip")).read()
    m = re.search(r"constexpr int TN_WINDOW = 1 << (\d+);", src)
    assert m and 1 << int(m.group(1)) == TN_WINDOW


# ------------------------------------------------------------------------------------------- 1. coarse ABI, NumPy only
@pytest.mark.parametrize("seed,users,src,tgt,overlap", [(5, 1500, 300, 300, 0.4), (7, 3000, 600, 80, 0.5)])
def test_recommend_through_the_coarse_abi(seed, users, src, tgt, overlap):
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(seed, users, src, tgt, overlap=overlap))
    I, U, alpha = r.n_items, users, 1.5
    drawn = np.random.default_rng(seed).integers(0, U, 300)
    queries = np.concatenate([drawn, [-1, U + 5, drawn[0]]]).astype(np.int32)
    tool = _tool(alpha)
    seen = dict(equal=False, few=False)         # what the input shows at one of its settings at least (asserted at the end)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        for keep in (1, 10):
            cnt, col, sim, _ = select(ctx, I, keep)
            scored = score_users(alpha, queries, T["ptr"], T["item"], T["rating"], T["time"], cnt, col, sim, T["avg"], keep)
            assert not any(c[1] is None for l in scored.values() for c in l)     # nothing dropped: the lists leave nothing out
            sizes = [len([c for c in scored.get(int(u), []) if not c[4]]) for u in queries]
            print("keep %d: candidates per query: 0: %d, 1-10: %d, > 10: %d, >= 64: %d, largest %d" % (
                keep, sum(s == 0 for s in sizes), sum(1 <= s <= 10 for s in sizes), sum(s > 10 for s in sizes),
                sum(s >= 64 for s in sizes), max(sizes)))
            seen["equal"] |= any(len({c[1] for c in l}) < len(l) for l in scored.values())  # two equal scores with one user
            assert sum(c[4] for l in scored.values() for c in l) > 0                       # held items with evidence
            pairs = set()
            tops = {}
            for n in (1, 10, 64):
                for rank_by in (0, 1):
                    for flags in (0, KEEP_HELD):
                        want = expected(scored, queries, n, rank_by, bool(flags), 66)
                        lens = [len([c for c in scored.get(int(u), []) if flags or not c[4]]) for u in queries]
                        assert 0 in lens and any(x > n for x in lens)
                        seen["few"] |= any(1 <= x < n for x in lens)
                        got = recommend(ctx, queries, n, rank_by, flags, alpha)
                        check_output(got, want, n)
                        assert want[1][1] == 0 and want[1][2] <= 66
                        holds = any(it in set(T["item"][T["ptr"][u]:T["ptr"][u + 1]].tolist())
                                    for u, l in zip(queries, want[0]) for it, _, _ in l)
                        assert holds == bool(flags)
                        again = recommend(ctx, queries, n, rank_by, flags, alpha)
                        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], again[:4])) and got[4] == again[4]
                        tops[n, rank_by, flags] = want[0]
                        pairs.update((int(u), it, p, d) for u, l in zip(queries, want[0]) for it, p, d in l)
            assert got[0][-3] == 0 and got[0][-2] == 0                                     # users -1 and U + 5
            assert got[1][0].tolist() == got[1][-1].tolist()                               # the user listed twice
            if keep == 10:
                differ = sum([c[0] for c in a] != [c[0] for c in b] for a, b in zip(tops[10, 0, 0], tops[10, 1, 0]))
                print("keep 10: %d top-10 lists differ between the plain and the decayed order" % differ)
                assert differ > 0
            # every returned score, rounded, is the prediction of the existing kernel for that pair
            pairs = sorted(pairs)
            p_plain, p_decay, p_status, _, _ = predict(ctx, [p[0] for p in pairs], [p[1] for p in pairs], None, alpha)
            assert not p_status.any()
            assert p_plain.tolist() == [tool.bound_rating(p[2]) for p in pairs]
            assert p_decay.tolist() == [tool.bound_rating(p[3]) for p in pairs]
        assert seen["equal"] and seen["few"]
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ 2. fine-grained, hand-built
def _hand_case(copies=300):
    """the construction of test_gpu_tail.test_evidence_beyond_64_entries (a user holding one neighbour 300 times with distinct
    times) + two items with identical lists and equal averages + a host-made list with a repeated neighbour, an entry >= I and
    negative similarities"""
    n_users, n_items, keep, dup_user = 80, 60, 10, 7
    ratings, sims, info, test = _prediction_case(3, n_users, n_items, dup_user=dup_user)
    held = "B%04dT:" % 1
    t0 = datetime.datetime(2012, 6, 1)
    ratings[held] = ratings[held] + [("U%05d" % dup_user, float(1 + q % 5), t0 + datetime.timedelta(minutes=7 * q + 1))
                                     for q in range(copies - 70)]
    info[held] = (float(np.mean([x[1] for x in ratings[held]])), 1.0, len(ratings[held]))
    a, b = "B%04dT:" % 10, "B%04dT:" % 20
    sims[b] = list(sims[a])
    info[b] = (info[a][0], 1.0, info[b][2])
    arrays = list(_case_arrays(ratings, sims, info, test, n_users, n_items, keep))
    cnt, col, sim = arrays[4], arrays[5], arrays[6]
    cnt[5] = 6
    col[5, :6] = [3, 3, n_items + 2, 1, -4, 3]
    sim[5, :6] = [-0.75, 0.5, 0.9, -0.125, 0.3, -0.25]
    return arrays, n_users, n_items, keep, dup_user


def test_hand_built_lists_and_evidence_beyond_the_lds_staging():
    arrays, U, I, keep, dup_user = _hand_case()
    ptr, pit, pra, pti, cnt, col, sim, avg = arrays[:8]
    alpha = 1.5
    queries = list(range(U)) + [U + 5]
    scored = score_users(alpha, queries, ptr, pit, pra, pti, cnt, col, sim, avg, keep)
    # the user with 300 rows of one neighbour: evidence beyond PR_CAP = 128 (the arena launch), now > 66
    big = [c for c in scored[dup_user] if c[3] > 66]
    assert big and max(c[3] for c in big) > 129          # now <= evidence entries + 1
    for n, rank_by, flags in ((10, 0, 0), (64, 1, KEEP_HELD), (5, 1, 0)):
        short = topn_rows(arrays, U, I, keep, alpha, 66, queries, n, rank_by, flags)
        want = expected(scored, queries, n, rank_by, bool(flags), 66)
        assert short[4][2] > 66 and short[4][1] == want[1][1] >= len([c for c in big if flags or not c[4]]) > 0
        check_output(short, want, n)
        full = topn_rows(arrays, U, I, keep, alpha, short[4][2], queries, n, rank_by, flags)
        want = expected(scored, queries, n, rank_by, bool(flags), short[4][2])
        check_output(full, want, n)
        assert full[4][2] == short[4][2]
    # the two items with identical lists and equal averages: equal scores, index order
    lists = expected(scored, queries, 64, 0, True, 10 ** 6)[0]
    twins = 0
    for l in lists:
        at = {c[0]: k for k, c in enumerate(l)}
        if 10 in at and 20 in at:
            assert l[at[10]][1] == l[at[20]][1] and at[10] < at[20]
            assert all(c[1] == l[at[10]][1] for c in l[at[10]:at[20]])
            twins += 1
    assert twins > 0
    # the host-made list: a repeated neighbour counts once per position, the entries outside [0, I) are ignored
    assert any(c[0] == 5 for l in lists for c in l)
    # the rounded scores are xmap_predict_rows' on the same arrays
    tool = _tool(alpha)
    pairs = sorted({(u, c[0], c[1], c[2]) for u, l in zip(queries, lists) for c in l})
    arr = arrays[:8] + [np.asarray([p[0] for p in pairs], np.int32), np.asarray([p[1] for p in pairs], np.int32)]
    plain, decay, status, _ = _predict_rows(arr, U, I, keep, alpha, 400)
    assert not status.any()
    assert plain.tolist() == [tool.bound_rating(p[2]) for p in pairs] and decay.tolist() == [tool.bound_rating(p[3]) for p in pairs]


# ------------------------------------------------------------------------------ 3. shapes that break the kernels
def _random_case(seed, U, I, keep, listed, rows_of, fixed_neighbor=None):
    """profiles (user u holds rows_of(u) distinct items, a few of them twice) and lists of `keep` random neighbours for the
    items of `listed`; ratings in thirds, five distinct times"""
    rng = np.random.default_rng(seed)
    per = []
    for u in range(U):
        items = rng.choice(I, size=rows_of(u), replace=False)
        items = np.concatenate([items, items[:len(items) // 50]])
        per.append(rng.permutation(items))
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum([len(p) for p in per], out=ptr[1:])
    pit = np.concatenate(per).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    pra = (rng.integers(1, 6, len(pit)) + rng.integers(0, 3, len(pit)) / 3.0).astype(np.float64)
    pti = rng.integers(0, 5, len(pit)).astype(np.int64)
    cnt, col, sim = np.zeros(I, np.int32), np.full((I, keep), -1, np.int32), np.zeros((I, keep))
    listed = np.asarray(listed)
    cnt[listed] = rng.integers(1, keep + 1, len(listed))
    col[listed] = rng.integers(0, I, (len(listed), keep))
    if fixed_neighbor is not None:
        col[listed, 0] = fixed_neighbor
    sim[listed] = np.round(rng.normal(size=(len(listed), keep)), 2)
    avg = np.round(rng.uniform(1.0, 5.0, I), 1)
    return [ptr, pit, pra, pti, cnt, col, sim, avg]


def _run_case(arrays, U, I, keep, queries, n, rank_by=0, flags=0, alpha=1.5):
    scored = score_users(alpha, queries, *arrays[:8], keep)
    want = expected(scored, queries, n, rank_by, bool(flags), 66)
    got = topn_rows(arrays, U, I, keep, alpha, 66, queries, n, rank_by, flags)
    check_output(got, want, n)
    return want


def test_a_profile_of_1000_distinct_items():
    U, I, keep = 6, 3000, 4
    arrays = _random_case(21, U, I, keep, np.arange(0, I, 2), lambda u: 1000 if u == 2 else 3 + u)
    for rank_by, flags in ((0, 0), (1, KEEP_HELD)):
        want = _run_case(arrays, U, I, keep, [2, 0, 5, 2], 64, rank_by, flags)
        assert want[1][3] > 256 and len(want[0][0]) == 64


def test_an_item_in_every_neighbor_list():
    U, I, keep = 30, 2000, 3
    arrays = _random_case(22, U, I, keep, np.arange(I), lambda u: 4 + u % 5, fixed_neighbor=0)
    arrays[1][arrays[0][3]] = 0             # users 3 and 11 hold item 0: every other item is their candidate
    arrays[1][arrays[0][11] + 1] = 0
    want = _run_case(arrays, U, I, keep, list(range(U)), 10, 1, 0)
    assert want[1][3] >= I - 16


def test_an_item_space_just_above_the_window():
    U, I, keep = 20, TN_WINDOW + 100, 2
    rng = np.random.default_rng(23)
    listed = np.unique(np.concatenate([[0, TN_WINDOW - 1, TN_WINDOW, I - 1], rng.integers(0, I, 100), rng.integers(TN_WINDOW, I, 96)]))
    pool = rng.integers(0, I, 30)           # the neighbours and the held items come from one small pool: evidence exists
    arrays = _random_case(23, U, I, keep, listed, lambda u: 8)
    arrays[5][listed] = pool[rng.integers(0, 30, (len(listed), keep))]
    arrays[4][listed] = keep
    arrays[1][:] = pool[rng.integers(0, 30, len(arrays[1]))]
    arrays[1][arrays[0][4]] = TN_WINDOW     # held items at the window's edges: they leave the lists without the flag
    arrays[1][arrays[0][5]] = TN_WINDOW - 1
    for flags in (0, KEEP_HELD):
        want = _run_case(arrays, U, I, keep, list(range(U)), 64, 0, flags)
        got = {c[0] for l in want[0] for c in l}
        assert {0, TN_WINDOW - 1, TN_WINDOW, I - 1} <= got and want[1][3] > 64


def test_one_query_and_many_queries_of_few_users():
    U, I, keep = 50, 400, 5
    arrays = _random_case(24, U, I, keep, np.arange(0, I, 3), lambda u: 2 + u % 9)
    _run_case(arrays, U, I, keep, [17], 10)
    queries = np.random.default_rng(24).integers(-2, U + 2, 5000).tolist()
    _run_case(arrays, U, I, keep, queries, 3, 1, KEEP_HELD)
    empty = topn_rows(arrays, U, I, keep, 1.5, 66, [], 10)
    assert empty[4] == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- 4. the Python route
def test_session_recommend_topn_equals_the_statement_on_id_strings():
    """the construction of test_gpu_tail.test_session_recommend_equals_the_python_statement; the expected lists from the
    collected dictionaries, on id strings"""
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.core.recommenderSim import RecommenderSim
    from xmap.engine import session, synth
    from xmap.engine.localrdd import LocalRDD
    from xmap.utils.assist import baseliner_calculate_sim_pipeline, extender_pipeline, generator_pipeline
    r = synth.make_two_domain(9, 1200, 300, 300, overlap=0.4)
    t0 = datetime.datetime(2013, 3, 1)
    recs = [(u, [(i, ra, t0 + datetime.timedelta(days=(t * 7919) % 6)) for i, ra, t in prof]) for u, prof in r.train_records()]
    sc = SparkContext(conf=SparkConf())
    trainRDD = sc.parallelize(recs, 8).cache()
    tool = BaselinerSim("cosine", CAP)
    sim = baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
    ae = generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True)
    rng = np.random.default_rng(9)
    uids = [recs[int(x)][0] for x in rng.integers(0, len(recs), 120)] + ["A%013d" % (10 ** 9 + 1)]
    item_based = RecommenderSim("cosine_item", CAP).build_sthbased_profile(ae, "item").collectAsMap()
    alpha = 1.5
    ptool = _tool(alpha)

    mine = {uid: {} for uid in uids}              # per query user: {iid: [(rating, time)*]} in the order of the item's list
    for iid, lst in item_based.items():
        for who, ra, when in lst:
            if who in mine:
                mine[who].setdefault(iid, []).append((ra, when))

    def statement(sim_pairs, item_info, n, decay, keep_held):
        out = []
        for uid in uids:
            cand = []
            for iid in sorted(sim_pairs):
                if not keep_held and iid in mine[uid]:
                    continue
                ev = [(s * (ra - item_info[nid][0]), abs(s), when) for nid, s in sim_pairs[iid] for ra, when in mine[uid].get(nid, ())]
                if ev:
                    base = item_info[iid][0]
                    cand.append((iid, base + sum(e[0] for e in ev) / sum(e[1] for e in ev), float(base + ptool._decayed_ratio(ev))))
            cand.sort(key=lambda c: (- c[2 if decay else 1], c[0]))
            out.append((uid, cand[:n]))
        return out

    first = None
    for n, decay, keep_held in ((10, False, False), (10, True, False), (3, True, True)):
        out = session.recommend_topn(ae, uids, CAP, 10, alpha, n, decay=decay, keep_held=keep_held)
        want = statement(out.sim_pairs, out.item_info, n, decay, keep_held)
        assert out.collect() == want
        assert out.stats[1] == 0 and out.stats[0] > 0
        if first is None:
            first = out
    assert out.collect()[-1] == (uids[-1], []) and any(len(l) == 10 for _, l in first.collect())
    assert any([c[0] for c in a[1]] != [c[0] for c in b[1]]
               for a, b in zip(statement(first.sim_pairs, first.item_info, 10, False, False), statement(first.sim_pairs, first.item_info, 10, True, False)))
    out2 = session.recommend_topn(ae, LocalRDD(uids), CAP, 10, alpha, 10, neighbors=first.sim_pairs)
    assert out2.collect() == first.collect()
    with pytest.raises(TypeError):
        session.recommend_topn(LocalRDD(ae.collect()), uids, CAP, 10, alpha, 10)


# ---------------------------------------------------------------------------------------------------- 5. lifecycle
def test_recommend_lifecycle_and_argument_errors():
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(3, 800, 200, 200, overlap=0.4))
    I, U = r.n_items, 800
    queries = np.random.default_rng(2).integers(0, U, 200).astype(np.int32)
    fresh = Ctx()
    try:
        generate(fresh, r)
        fresh.call("xmap_ctx_rec_sim", CAP, None)
        fresh.call("xmap_ctx_rec_select", 10)
        ref = recommend(fresh, queries, 10, 1, 0, 0.2)
    finally:
        fresh.close()
    assert ref[4][0] > 0 and ref[0].max() == 10
    c = Ctx()
    try:
        ERR = c.abi.ERR_ARG
        q, w = np.zeros(1, np.int32), wtab(0.2, 8)
        oc, oi, op, od = np.zeros(1, np.int32), np.zeros(4, np.int32), np.zeros(4), np.zeros(4)

        def raw(n_query=1, qu=q, n=4, rank_by=0, flags=0, tab=w, n_w=8, out=(oc, oi, op, od)):
            return c.lib.xmap_ctx_recommend(c.h, n_query, _p(qu, C.c_int32), n, rank_by, flags, _p(tab, C.c_double), n_w,
                                            _p(out[0], C.c_int32), _p(out[1], C.c_int32), _p(out[2], C.c_double),
                                            _p(out[3], C.c_double), None)
        assert raw() == ERR                                                 # before upload
        rows = generate(c, r)
        assert raw() == ERR                                                 # before rec_sim
        c.call("xmap_ctx_rec_sim", CAP, None)
        assert raw() == ERR and b"have_nb" in c.lib.xmap_last_error()      # before rec_select
        c.call("xmap_ctx_rec_select", 10)
        assert raw() == 0
        # argument errors leave the context working
        for kw in (dict(n=0), dict(n=65), dict(rank_by=2), dict(rank_by=-1), dict(flags=2), dict(flags=-1), dict(n_w=0),
                   dict(out=(None, oi, op, od)), dict(out=(oc, None, op, od)), dict(out=(oc, oi, None, od)),
                   dict(out=(oc, oi, op, None)), dict(qu=None)):
            assert raw(**kw) == ERR, kw
            assert c.lib.xmap_last_error()
        assert raw(n_query=0, qu=None, out=(None, None, None, None)) == 0   # nothing to do, nothing touched
        got = recommend(c, queries, 10, 1, 0, 0.2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], ref[:4])) and got[4] == ref[4]
        c.call("xmap_ctx_item_sim", 0, CAP, None, None)                     # an earlier stage run again drops the tail
        assert raw() == ERR
        c.call("xmap_ctx_extend", 5, None, None)
        stage_c(c, I, True, None)
        c.call("xmap_ctx_rec_sim", CAP, None)
        assert raw() == ERR
        c.call("xmap_ctx_rec_select", 10)
        got = recommend(c, queries, 10, 1, 0, 0.2)                          # the reused context: the bytes of a fresh one
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], ref[:4])) and got[4] == ref[4]
        assert len(rows["user"]) > 0
    finally:
        c.close()
