"""Non-integer ratings end to end.

With integer ratings every fp64 sum of stage A is exact, so any order of addition gives the same bits and a kernel that
sums in an arbitrary order (LDS atomics, lane-strided partials) cannot be told from one that sums exactly.  Here the
ratings are fractional (float32 values), zero or negative: the canonical value of every sum is the exact sum rounded
once, which the oracle and every HIP formulation must reproduce bit for bit.

CPU tests: an independent restatement of stage A (NumPy + math.fsum) against the oracle, the predicate that keeps the
plain-sum kernels for ratings whose sums are exact (xmap.engine.exactness), the float32 rule of the drop-in.
GPU tests (-m gpu): every stage against the oracle on such ratings, the formulations and partitionings against each
other, the user- and item-sharded steps against one rank, the drop-in boundary.
"""
import math
import os

import numpy as np
import pytest

from golden_util import CAP, METHODS, Golden, csr_to_pairs

# ratings with zeros and negatives (float32 values): negative dot products, zero norms
SIGNED = (-2.5, -1.3, 0.0, 0.7, 1.9, 3.3)


def _with_ratings(r, rating):
    from xmap.engine import synth
    return synth.Ratings(r.user_ptr, r.item, np.ascontiguousarray(rating, np.float32), r.time, r.n_items, r.n_src_items,
                         r.src_numbers, r.tgt_numbers)


def _ulps(a, b):
    """distance of two fp64 arrays in units of the last place of b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sp = np.spacing(np.abs(b))
    return np.where(a == b, 0.0, np.abs(a - b) / np.where(sp > 0, sp, 1.0))


# ------------------------------------------------------------------------------------------------ the fsum reference
def fsum_stage_a(ptr, item, rating, n_items, method, cap):
    """stage A restated with the canonical sums (core/baselinerSim.py:17-216): the user average as the reference's
    python sum() (left to right), every other sum exact (math.fsum, correctly rounded).  Returns (uavg, info [I][4],
    {(i, j): (sim, mutu, nij)} of the kept directed pairs)."""
    rating = np.asarray(rating, np.float32).astype(np.float64)
    U = len(ptr) - 1
    uavg = np.zeros(U)
    for u in range(U):
        rs = [float(x) for x in rating[ptr[u]:ptr[u + 1]]]
        uavg[u] = sum(rs) / len(rs) if rs else 0.0
    raters = [[] for _ in range(n_items)]
    for u in range(U):
        for e in range(ptr[u], ptr[u + 1]):
            raters[item[e]].append((u, float(rating[e])))
    info = np.zeros((n_items, 4))
    for i, rs in enumerate(raters):
        n = len(rs)
        info[i, 0] = 1.0 * math.fsum(r for _, r in rs) / n if n else 0.0
        info[i, 1] = math.sqrt(math.fsum(r ** 2 for _, r in rs))
        info[i, 2] = math.sqrt(math.fsum((r - uavg[u]) * (r - uavg[u]) for u, r in rs))
        info[i, 3] = 1.0 * n
    c1 = 1 if method == "cosine" else 2
    terms, mutu = {}, {}
    for u in range(U):
        a, b = ptr[u], ptr[u + 1]
        if b - a < 2:
            continue
        for e in range(a, b):
            i, ri = int(item[e]), float(rating[e])
            for f in range(a, b):
                j, rj = int(item[f]), float(rating[f])
                if j == i:
                    continue
                t = 1.0 * ri * rj if method == "cosine" else (ri - uavg[u]) * (rj - uavg[u])
                terms.setdefault((i, j), []).append(t)
                mutu[(i, j)] = mutu.get((i, j), 0) + int((ri >= info[i, 0]) == (rj >= info[j, 0]))
    kept = {}
    for (i, j), ts in terms.items():
        n = len(ts)
        dot = math.fsum(ts)
        den = info[i, c1] * info[j, c1]
        cs = 1.0 * dot / den if den else 0.0
        sim = 1.0 * cs * min(n, cap) / cap
        m = mutu[(i, j)]
        frac = 1.0 * m / (info[i, 3] + info[j, 3] - n)
        if sim != 0.0 and m != 0 and frac != 0.0:
            kept[(i, j)] = (sim, m, n)
    return uavg, info, kept


def _small_inputs():
    from xmap.engine import synth
    r = synth.make_two_domain(9, 300, 70, 70, overlap=0.4)
    return [("fractional", synth.fractional(r, seed=3)),
            ("signed", synth.fractional(r, seed=4, values=SIGNED)),
            ("integer", r)]


@pytest.mark.parametrize("method", METHODS)
def test_fsum_reference_vs_oracle(method):
    """the oracle's sums are the exact sums (within 1 ulp: a double-double is not correctly rounded in every case), its
    discrete outputs those of the restatement; on integer ratings everything is bit-identical"""
    from oracle import xmap_oracle as xo
    for name, r in _small_inputs():
        T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
        uavg, info, kept = fsum_stage_a(r.user_ptr, r.item, r.rating, r.n_items, method, CAP)
        ou, _ = xo.user_info(T)
        oi = xo.item_info(T, ou)
        assert np.array_equal(ou, uavg), name
        assert np.array_equal(oi[:, 3], info[:, 3]), name
        assert _ulps(oi[:, :3], info[:, :3]).max() <= 1, name
        S = xo.item_sim(T, method, CAP, nthreads=2)
        rows, cols = csr_to_pairs(S.row_ptr, S.col)
        keys = sorted(kept)
        assert [(int(a), int(b)) for a, b in zip(rows, cols)] == keys, name
        want = np.array([kept[k][0] for k in keys])
        assert np.array_equal(S.mutu, [kept[k][1] for k in keys]) and np.array_equal(S.nij, [kept[k][2] for k in keys])
        # the sim is a quotient of the sums: a 1-ulp difference of a sum is a few ulps of the sim
        assert _ulps(S.sim, want).max() <= 4, name
        if name == "integer":
            assert np.array_equal(S.sim, want) and np.array_equal(oi, info)
        if name == "signed":
            assert (S.sim < 0).any()
        xo.sim_free(S)


def test_plain_sums_predicate_edges(monkeypatch):
    from xmap.engine.exactness import fraction_bits, plain_sums_exact as ok
    monkeypatch.delenv("XMAP_EXACT_COSINE", raising=False)
    two53 = 2 ** 53
    # integers: U M^2 just below / at / above 2^53
    assert ok([5.0, 1.0], two53 // 25) and not ok([5.0, 1.0], two53 // 25 + 1)
    assert ok([2.0 ** 20, 3.0], 2 ** 13) and not ok([2.0 ** 20, 3.0], 2 ** 13 + 1)
    assert ok([1.0, 2.0, 3.0, 4.0, 5.0], 10 ** 6)
    # halves: e = 1, (2 M)^2 = 81
    assert fraction_bits([0.5, 4.5]) == 1
    assert ok([0.5, 4.5], two53 // 81) and not ok([0.5, 4.5], two53 // 81 + 1)
    # float32(3.7): 22 fractional bits, the sums of a handful of users only are exact
    f = float(np.float32(3.7))
    assert fraction_bits([f]) == 22
    m2 = int(np.ldexp(f, 22)) ** 2
    assert ok([f], two53 // m2) and not ok([f], two53 // m2 + 1) and not ok([f], 10 ** 6)
    # the fp64 value 3.7 has more fractional bits than any exact plain sum allows
    assert fraction_bits([3.7]) is None and not ok([3.7], 1)
    # zeros, negatives, nothing at all
    assert ok([0.0, 0.0], 10 ** 9) and ok([], 10)
    assert ok([-5.0, 3.0], two53 // 25) and not ok([-5.0, 3.0], two53 // 25 + 1)
    # non-finite values
    for bad in (np.inf, -np.inf, np.nan):
        assert not ok([1.0, bad], 2)
    # the override
    monkeypatch.setenv("XMAP_EXACT_COSINE", "1")
    assert not ok([1.0, 2.0], 2) and ok([1.0, 2.0], 2, env=False)


def test_float32_rule_names_the_rating():
    from xmap.engine import session
    ptr = np.array([0, 2, 3])
    item = np.array([1, 0, 1])
    session.check_float32(ptr, item, [1.0, float(np.float32(3.7)), np.nan], ["u0", "u1"], ["a", "b"])
    with pytest.raises(ValueError, match=r"3\.7.*'u1'.*'b'.*np\.float32"):
        session.check_float32(ptr, item, [1.0, 2.0, 3.7], ["u0", "u1"], ["a", "b"])


# ------------------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device
    return device


def _parity():
    import test_gpu_parity as P
    return P


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_golden_fractional_vs_oracle(dev, method):
    """the committed fractional case: every stage against the oracle, bit for bit"""
    from xmap.engine import synth
    g = Golden("fractional")
    r = synth.Ratings(g.ptr, g.item, g.rating, g.time, g.I, 0, None, None)
    r.item_attrs = lambda: g.attrs
    _parity()._check_all_stages(dev, r, method, 5)
    assert not dev.DeviceRatings(g.ptr, g.item, g.rating, g.time, g.I, g.attrs).plain_exact


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_c1_fractional_vs_oracle(dev, method):
    from xmap.engine import synth
    _parity()._check_all_stages(dev, synth.fractional(synth.config_c1(), seed=1), method, 5)


@gpu
@pytest.mark.parametrize("sim_kw", [dict(ch_min=64), dict(slot_target=32)], ids=["ch_min64", "slot32"])
@pytest.mark.parametrize("method", METHODS)
def test_fractional_heavy_rows_and_partitions_vs_oracle(dev, method, sim_kw):
    from xmap.engine import synth
    r = synth.fractional(synth.make_two_domain(106, 1200, 250, 250, overlap=0.4, mu=2.0), seed=6)
    _parity()._check_all_stages(dev, r, method, 5, **sim_kw)


def _stage_a_vs_oracle(dev, r, method, sims):
    from oracle import xmap_oracle as xo
    P = _parity()
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
    So = xo.item_sim(T, method, CAP, nthreads=8)
    orow, ocol = csr_to_pairs(So.row_ptr, So.col)
    for name, S in sims:
        assert S.n_eval == So.n_eval and S.n_contrib == So.n_contrib, name
        rows, cols, sim, mutu, nij = P._sorted_sim(S)
        assert np.array_equal(rows, orow) and np.array_equal(cols, ocol), name
        assert np.array_equal(mutu, So.mutu) and np.array_equal(nij, So.nij), name
        assert np.array_equal(S.info.cpu().numpy(), So.info), name
        assert np.array_equal(sim, So.sim), name
    xo.sim_free(So)


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_fractional_long_profiles_vs_oracle(dev, method):
    """profiles over 1024 ratings and popular items (the unrolled item-stats walk): the three formulations"""
    from xmap.engine import synth
    r = synth.fractional(synth.make_two_domain(21, 600, 1500, 1500, overlap=0.5, mu=4.0, sigma=1.6), seed=21)
    assert np.diff(r.user_ptr).max() > 1024
    eng = dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
    _stage_a_vs_oracle(dev, r, method, [("tri", eng.item_sim(method, CAP)),
                                        ("heavy", eng.item_sim_tri(method, CAP, ch_min=64)),
                                        ("rows", eng.item_sim(method, CAP, algo="rows"))])


def _hubs(frac):
    """test_keys_larger_than_a_tile's input: two items rated by all 8000 users next to thousands of light ones"""
    from xmap.engine import synth
    r = synth.make_two_domain(31, 8000, 4000, 4000, overlap=0.4)
    hubs = (7, r.n_src_items + 11)
    rng = np.random.default_rng(5)
    ptr, item, time = [0], [], []
    for u in range(r.n_users):
        a, b = int(r.user_ptr[u]), int(r.user_ptr[u + 1])
        it, ti = list(r.item[a:b]), list(r.time[a:b])
        for h in hubs:
            if h not in it:
                it.append(h); ti.append(int(rng.integers(synth.T0, synth.T1)))
        item += it; time += ti
        ptr.append(len(item))
    out = synth.Ratings(np.asarray(ptr, np.int64), np.asarray(item, np.int32), np.ones(len(item), np.float32),
                        np.asarray(time, np.int64), r.n_items, r.n_src_items, r.src_numbers, r.tgt_numbers)
    return synth.fractional(out, seed=31) if frac else out


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_fractional_hub_items_vs_oracle(dev, method, monkeypatch):
    """8000 raters on one item (heavy rows, chunked item statistics): both stage-A sequences and the partitioned count"""
    r = _hubs(True)
    eng = dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
    sims = []
    for v2 in ("0", "1"):
        monkeypatch.setenv("XMAP_A_V2", v2)
        sims.append(("v2=%s" % v2, eng.item_sim_tri(method, CAP, ch_min=1024)))
        sims.append(("v2=%s ch64" % v2, eng.item_sim_tri(method, CAP, ch_min=64)))
    monkeypatch.delenv("XMAP_A_V2")
    monkeypatch.setenv("XMAP_COUNT_PART_MIN", "1")
    sims.append(("part", eng.item_sim_tri(method, CAP)))
    _stage_a_vs_oracle(dev, r, method, sims)


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_stage_a_vs_fsum_reference(dev, method):
    """the GPU's sums against the exact (fsum) ones, within 1 ulp: catches a wrong oracle too"""
    for name, r in _small_inputs():
        _, info, kept = fsum_stage_a(r.user_ptr, r.item, r.rating, r.n_items, method, CAP)
        eng = dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
        S = eng.item_sim(method, CAP)
        rows, cols, sim, mutu, nij = _parity()._sorted_sim(S)
        keys = sorted(kept)
        assert [(int(a), int(b)) for a, b in zip(rows, cols)] == keys, name
        assert np.array_equal(mutu, [kept[k][1] for k in keys]) and np.array_equal(nij, [kept[k][2] for k in keys])
        gi = S.info.cpu().numpy()
        assert np.array_equal(gi[:, 3], info[:, 3]) and _ulps(gi[:, :3], info[:, :3]).max() <= 1, name
        assert _ulps(sim, [kept[k][0] for k in keys]).max() <= 4, name


@gpu
def test_fractional_determinism_and_partitions(dev):
    """cosine on fractional ratings: two runs, the table partitionings, the heavy rows and the complete-rows formulation
    give identical bytes"""
    from xmap.engine import synth
    r = synth.fractional(synth.make_two_domain(9, 3000, 600, 600), seed=9)
    eng = dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
    P = _parity()
    runs = [eng.item_sim("cosine", CAP), eng.item_sim("cosine", CAP), eng.item_sim("cosine", CAP, slot_target=48),
            eng.item_sim("cosine", CAP, algo="rows"), eng.item_sim("cosine", CAP, algo="rows", slot_target=48),
            eng.item_sim_tri("cosine", CAP, ch_min=64)]
    a = P._sorted_sim(runs[0])
    info = runs[0].info.cpu().numpy()
    for S in runs[1:]:
        for x, y in zip(a, P._sorted_sim(S)):
            assert np.array_equal(x, y)
        assert np.array_equal(S.info.cpu().numpy(), info)


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_exact_route_equals_fast_route_on_integers(dev, method, monkeypatch):
    from xmap.engine import synth
    r = synth.make_two_domain(9, 3000, 600, 600)
    P = _parity()
    fast = dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
    assert fast.R.plain_exact
    monkeypatch.setenv("XMAP_EXACT_COSINE", "1")
    exact = dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
    assert not exact.R.plain_exact
    for kw in (dict(), dict(algo="rows")):
        A, B = fast.item_sim(method, CAP, **kw), exact.item_sim(method, CAP, **kw)
        for x, y in zip(P._sorted_sim(A), P._sorted_sim(B)):
            assert np.array_equal(x, y)
    A, B = fast.item_sim_tri(method, CAP, ch_min=64), exact.item_sim_tri(method, CAP, ch_min=64)
    for x, y in zip(P._sorted_sim(A), P._sorted_sim(B)):
        assert np.array_equal(x, y)


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_rating_edges_vs_oracle(dev, method):
    """an item rated only 0 (zero norm: sim 0.0, every pair filtered), negative ratings (negative similarities through the
    top-k lists and X-Sim), ratings equal to their item's average (the mutuality test is `>=`).  One user in ten rates in
    both domains, so a quarter of the items have no neighbour of the other domain and paths start from them (oracle census,
    cosine | adjusted cosine: 155 455 | 114 456 paths, 189 | 15 220 candidates with a negative X-Sim, 74 | 98 replaced items)"""
    from xmap.engine import synth
    P = _parity()
    base = synth.make_two_domain(12, 1500, 400, 400, overlap=0.1)
    rating = base.rating.astype(np.float32) - np.float32(3.0)          # -2 .. 2
    zero_item = int(np.bincount(base.item).argmax())
    rating[base.item == zero_item] = 0.0
    flat = np.nonzero(np.bincount(base.item, minlength=base.n_items) > 3)[0][:20]
    rating[np.isin(base.item, flat)] = np.float32(1.3)                 # every rating equals the item average
    r = _with_ratings(base, rating)
    eng = dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
    S = eng.item_sim(method, CAP)
    rows, cols, sim, _, _ = P._sorted_sim(S)
    if method == "cosine":          # (adjusted cosine: r - avg_u is not 0, the item has a norm)
        assert zero_item not in set(rows.tolist()) | set(cols.tolist())
        assert (sim < 0).any()
        E = eng.extend(S, 5, full=True)
        assert (E.kval.cpu().numpy()[..., 0] < 0).any()
    assert set(flat.tolist()) & set(rows.tolist())
    P._check_all_stages(dev, r, method, 5, need=dict(paths=10 ** 4, neg=1, mapped=10))


@gpu
@pytest.mark.parametrize("world,method", [(2, "cosine"), (2, "adjust_cosine"), (3, "cosine"), (3, "adjust_cosine")])
def test_user_sharded_fractional_equals_world1(world, method):
    import test_gpu_sharded as SH
    SH._check_user_sharded(world, method, "gloo", frac=True)


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_item_sharded_fractional_equals_world1(method):
    import test_gpu_sharded as SH
    SH._check_world_equals_world1(2, "gloo", method, frac=True)


@gpu
def test_drop_in_refuses_ratings_float32_cannot_hold():
    """a trainRDD rating 3.7 is refused (the engine would compute with 3.700000047683716); float(np.float32(3.7)) is
    accepted and the AlterEgo rows carry the reference's means of those values, bit for bit"""
    import torch
    assert torch.cuda.is_available()
    from pyspark import SparkContext, SparkConf
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.utils.assist import baseliner_calculate_sim_pipeline
    from test_gpu_api import records
    g = Golden("fractional")
    recs = records(g)
    sc = SparkContext(conf=SparkConf().setAppName("float32"))
    uid, prof = recs[3]
    iid, r0, t0 = prof[0]
    bad = [(u, p) for u, p in recs]
    bad[3] = (uid, [(iid, 3.7, t0)] + list(prof[1:]))
    with pytest.raises(ValueError, match=r"3\.7.*%s.*%s.*float32" % (uid, iid.replace(":", r"\:"))):
        baseliner_calculate_sim_pipeline(sc, BaselinerSim("cosine", CAP), sc.parallelize(bad)).collect()
    # float32 values are accepted: the committed case's ratings are float(np.float32(v))
    assert all(float(np.float32(r)) == r for _, p in recs for (_, r, _) in p)


@gpu
@pytest.mark.parametrize("method", ["cosine"])
def test_fullsize_c2_structure_fractional_stage_a(dev, method):
    """BASELINE configs[1] (c2) structure with fractional ratings: cosine stage A against the oracle over the whole matrix
    and the item info"""
    from xmap.engine import synth
    r = synth.fractional(synth.config_c2(), seed=2)
    eng = dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))
    _stage_a_vs_oracle(dev, r, method, [("c2", eng.item_sim(method, CAP))])
    assert not eng.R.plain_exact


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_coarse_abi_fractional_vs_oracle(method, monkeypatch):
    """the coarse C ABI applies the same rule at upload (api.hip): the fractional case, and the integer one with
    XMAP_EXACT_COSINE=1, give the oracle's stage A bit for bit"""
    import ctypes as C
    from oracle import xmap_oracle as xo
    from test_gpu_coarse_abi import Ctx, _p
    for case, force in (("fractional", None), ("small", "1")):
        if force:
            monkeypatch.setenv("XMAP_EXACT_COSINE", force)
        gold = Golden(case)
        I, U = gold.I, len(gold.ptr) - 1
        pre, suf, mask, flags = [np.ascontiguousarray(a, t) for a, t in zip(gold.attrs, (np.int32, np.int32, np.uint32, np.uint8))]
        ptr, item = np.ascontiguousarray(gold.ptr, np.int64), np.ascontiguousarray(gold.item, np.int32)
        rating, pos = np.ascontiguousarray(gold.rating, np.float32), np.ascontiguousarray(gold.time, np.int64)
        T = xo.Train(ptr, item, rating, pos, I, *gold.attrs)
        So = xo.item_sim(T, method, CAP, nthreads=4)
        ctx = Ctx()
        try:
            ctx.call("xmap_ctx_upload_ratings", U, I, _p(ptr, C.c_int64), _p(item, C.c_int32), _p(rating, C.c_float),
                     _p(pos, C.c_int64), _p(pre, C.c_int32), _p(suf, C.c_int32), _p(mask, C.c_uint32), _p(flags, C.c_uint8))
            n_kept, n_eval = C.c_int64(0), C.c_int64(0)
            ctx.call("xmap_ctx_item_sim", 0 if method == "cosine" else 1, CAP, C.byref(n_kept), C.byref(n_eval))
            n = n_kept.value
            rp, col, sim = np.zeros(I + 1, np.int64), np.zeros(n, np.int32), np.zeros(n, np.float64)
            mutu, nij, info, uavg = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((I, 4)), np.zeros(U)
            ctx.call("xmap_ctx_sim_download", _p(rp, C.c_int64), _p(col, C.c_int32), _p(sim, C.c_double), _p(mutu, C.c_int32),
                     _p(nij, C.c_int32), _p(info, C.c_double), _p(uavg, C.c_double))
        finally:
            ctx.close()
        rows = np.repeat(np.arange(I), np.diff(rp))
        o = np.lexsort((col, rows))
        orow, ocol = csr_to_pairs(So.row_ptr, So.col)
        assert np.array_equal(rows[o], orow) and np.array_equal(col[o], ocol), case
        assert np.array_equal(sim[o], So.sim) and np.array_equal(mutu[o], So.mutu) and np.array_equal(nij[o], So.nij), case
        assert np.array_equal(info, So.info), case
        xo.sim_free(So)
