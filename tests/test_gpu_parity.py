"""GPU parity tests (run on the MI355X box: `pytest -m gpu`).  Everything goes through the C ABI of
libxmap_hip.so (xmap.engine.device -> ctypes); results are compared with
  * the golden vectors captured from the reference (tests/golden/*.npz), and
  * the CPU oracle (oracle/xmap_oracle.c) on seeded synthetic inputs (BASELINE configs[0] size),
ids / index sets bit-exact, similarities to the tolerance stated next to each assert.
"""
import os

import numpy as np
import pytest

from golden_util import CASES, METHODS, CAP, FRACTIONAL, FRACTIONAL_RTOL, Golden, census, check_census, csr_to_pairs

pytestmark = pytest.mark.gpu

SIM_RTOL = 1e-11   # adjusted-cosine: exact (error-free) sum of the fp64 terms vs the reference's np.sum rounding
XSIM_RTOL = 1e-9   # sum over paths: exact sum vs the reference's BLAS dot / pairwise rounding


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device  # raises if libxmap_hip.so is missing: no CPU fallback
    return device


def _engine(dev, ptr, item, rating, time, I, attrs):
    R = dev.DeviceRatings(ptr, item, rating, time, I, attrs)
    return dev.Engine(R)


def _sorted_sim(S):
    row_ptr = S.row_ptr.cpu().numpy()
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))
    col = S.col.cpu().numpy().astype(np.int64)
    o = np.lexsort((col, rows))
    return rows[o], col[o], S.sim.cpu().numpy()[o], S.mutu.cpu().numpy()[o], S.nij.cpu().numpy()[o]


def _xsim_lists(E, I):
    n_cand = E.n_cand.cpu().numpy()[:I]
    off = E.xs_off.cpu().numpy()[:I]
    xe = E.xs_end.cpu().numpy()
    xv = E.xs_val.cpu().numpy()
    st, en, va = [], [], []
    for s in np.nonzero(n_cand)[0]:
        e = xe[off[s]:off[s] + n_cand[s]]
        v = xv[off[s]:off[s] + n_cand[s]]
        o = np.argsort(e)
        st.append(np.full(len(e), s)); en.append(e[o]); va.append(v[o])
    if not st:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(st), np.concatenate(en), np.concatenate(va)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", CASES)
def test_golden_all_stages(dev, case, method):
    gold = Golden(case)
    eng = _engine(dev, gold.ptr, gold.item, gold.rating, gold.time, gold.I, gold.attrs)
    frac = case in FRACTIONAL       # the reference's fp64 sums round (bit for bit against the oracle: test_gpu_ratings.py)
    exact = method == "cosine" and not frac
    # ---- stage A
    S = eng.item_sim(method, CAP)
    exp_u = gold[method + ".user_info"]
    assert np.array_equal(S.u_avg.cpu().numpy()[:len(exp_u)], exp_u[:, 0])
    assert np.array_equal(S.u_norm.cpu().numpy()[:len(exp_u)], exp_u[:, 1])
    info = S.info.cpu().numpy()
    exp_i = gold[method + ".item_info"]
    if frac:
        np.testing.assert_allclose(info[:, :2], exp_i[:, :2], rtol=1e-14, atol=0)
        assert np.array_equal(info[:, 3], exp_i[:, 3])
    else:
        assert np.array_equal(info[:, [0, 1, 3]], exp_i[:, [0, 1, 3]])
    np.testing.assert_allclose(info[:, 2], exp_i[:, 2], rtol=1e-14)
    rows, cols, sim, mutu, nij = _sorted_sim(S)
    assert np.array_equal(rows, gold[method + ".sim_i"])
    assert np.array_equal(cols, gold[method + ".sim_j"])
    val = gold[method + ".sim_val"]
    assert np.array_equal(mutu.astype(np.float64), val[:, 1])
    assert np.array_equal(mutu / (info[rows, 3] + info[cols, 3] - nij), val[:, 2])
    if exact:
        assert np.array_equal(sim, val[:, 0])
    elif method == "cosine":
        np.testing.assert_allclose(sim, val[:, 0], rtol=FRACTIONAL_RTOL, atol=0)
    else:
        np.testing.assert_allclose(sim, val[:, 0], rtol=SIM_RTOL, atol=0)
    # symmetric bit for bit
    back = {(int(a), int(b)): s for a, b, s in zip(rows, cols, sim)}
    assert all(back[(b, a)] == s for (a, b), s in back.items())
    # ---- stage B / C
    for k in gold.ks(method):
        tag = "%s.k%d" % (method, k)
        E = eng.extend(S, k, full=True)
        assert np.array_equal(np.nonzero(E.bb.cpu().numpy()[:gold.I])[0], gold[tag + ".bb"])
        ki = gold[tag + ".knn_items"]
        cls = E.cls.cpu().numpy()[:gold.I]
        assert np.array_equal(np.nonzero(cls)[0], np.sort(ki[:, 0]))
        assert np.array_equal(cls[ki[:, 0]], ki[:, 1])
        head, kv = gold[tag + ".knn_head"], gold[tag + ".knn_val"]
        kcnt = E.kcnt.cpu().numpy()[:gold.I]
        assert int(kcnt[cls > 0].sum()) == len(head)
        it, lid, pos, nbr = head.T
        assert np.array_equal(E.kcol.cpu().numpy()[it, lid % 2, pos], nbr)
        got = E.kval.cpu().numpy()[it, lid % 2, pos]
        if exact:
            assert np.array_equal(got, kv)
        elif method == "cosine":
            np.testing.assert_allclose(got, kv, rtol=FRACTIONAL_RTOL, atol=0)
        else:
            np.testing.assert_allclose(got, kv, rtol=SIM_RTOL, atol=0)
        st, en, va = _xsim_lists(E, gold.I)
        xh = gold[tag + ".xsim_head"]
        assert np.array_equal(st, xh[:, 0]) and np.array_equal(en, xh[:, 1])
        np.testing.assert_allclose(va, gold[tag + ".xsim_val"], rtol=XSIM_RTOL, atol=1e-300)
        for gt in gold.gen_tags(method, k):
            gtag = tag + "." + gt
            private = gt == "priv"
            picks = None
            if not private:
                n_top, _, _ = eng.select(E, False, None)
                np.random.seed(int(gt[2:]))
                if gold.has(gtag + ".raises"):
                    with pytest.raises(ValueError):
                        dev.draw_picks(n_top.cpu().numpy()[:gold.I])
                    continue
                picks = dev.draw_picks(n_top.cpu().numpy()[:gold.I])
            n_top, choice, mp = eng.select(E, private, picks)
            exp = gold[gtag + ".choice"]
            n_top = n_top.cpu().numpy()[:gold.I]
            starts = np.nonzero(n_top)[0]
            assert np.array_equal(starts, exp[:, 0])
            assert np.array_equal(choice.cpu().numpy()[starts], exp[:, 1])
            G = eng.alterego(mp)
            eh = gold[gtag + ".ae_head"]
            assert np.array_equal(G.user.cpu().numpy(), eh[:, 0])
            assert np.array_equal(G.item.cpu().numpy(), eh[:, 1])
            assert np.array_equal(G.rating.cpu().numpy(), gold[gtag + ".ae_rating"])      # fp64 means, bit for bit
            assert np.array_equal(G.time.cpu().numpy(), gold[gtag + ".ae_time"])


def _check_all_stages(dev, r, method, k, private=True, picks_seed=None, need=None, ext_kw=None, **sim_kw):
    """every stage of one pass against the CPU oracle, bit for bit (ratings of the AlterEgo rows: fp32, atol 1e-5).
    need: lower bounds on golden_util.census() of the oracle's own results -- how many non-bridge items, paths, candidates,
    replacements and AlterEgo rows of replaced items the input must produce for the comparison to say something about
    stages B and C; checked before anything of the GPU's is compared.  ext_kw: arguments of Engine.extend (chunk, n_slots).
    Returns the engine and its results (stage A, extension, (n_top, choice, map), AlterEgo rows)."""
    from oracle import xmap_oracle as xo
    attrs = r.item_attrs()
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *attrs)
    So = xo.item_sim(T, method, CAP, nthreads=8)
    Xo = xo.extend(T, So, k)
    picks = None
    if not private:
        n_top_probe, _, _ = xo.select(T, Xo, True, None)
        np.random.seed(picks_seed)
        try:
            picks = dev.draw_picks(np.minimum(n_top_probe, 4))
        except ValueError:       # a start with a single candidate: the reference's randint(0, 0) raises (generator.py:109)
            picks = None
            private = True
    n_top_o, choice_o, m_o = xo.select(T, Xo, private, picks)
    ae = xo.alterego(T, m_o)
    if need is not None:
        check_census(census(So, Xo, m_o, ae), need, "%s, k = %d" % (method, k))
    eng = _engine(dev, r.user_ptr, r.item, r.rating, r.time, r.n_items, attrs)
    S = eng.item_sim_tri(method, CAP, **sim_kw) if sim_kw else eng.item_sim(method, CAP)
    assert S.n_eval == So.n_eval and S.n_contrib == So.n_contrib
    rows, cols, sim, mutu, nij = _sorted_sim(S)
    orow, ocol = csr_to_pairs(So.row_ptr, So.col)
    assert np.array_equal(rows, orow) and np.array_equal(cols, ocol)
    assert np.array_equal(mutu, So.mutu) and np.array_equal(nij, So.nij)
    # both sides sum error-free (cosine: integer-exact) -> bit-identical in both modes
    assert np.array_equal(S.info.cpu().numpy(), So.info)
    assert np.array_equal(sim, So.sim)
    E = eng.extend(S, k, full=True, **(ext_kw or {}))
    assert np.array_equal(E.bb.cpu().numpy()[:T.I], Xo.bb)
    assert np.array_equal(E.cls.cpu().numpy()[:T.I], Xo.cls)
    assert np.array_equal(E.kcnt.cpu().numpy()[:T.I], Xo.cnt)
    kc = E.kcol.cpu().numpy()[:T.I]
    msk = np.arange(k)[None, None, :] < Xo.cnt[:, :, None]
    assert np.array_equal(kc[msk], Xo.col[msk])
    assert E.n_paths == Xo.n_paths
    st, en, va = _xsim_lists(E, T.I)
    ost, oen = csr_to_pairs(Xo.xs_ptr, Xo.xs_end)
    assert np.array_equal(st, ost) and np.array_equal(en, oen)
    # path values are bit-identical and both sides sum them error-free (double-double)
    assert np.array_equal(va, Xo.xs_val)
    n_top, choice, mp = eng.select(E, private, picks)
    assert np.array_equal(n_top.cpu().numpy()[:T.I], n_top_o)
    assert np.array_equal(choice.cpu().numpy()[:T.I], choice_o)
    assert np.array_equal(mp.cpu().numpy()[:T.I], m_o)
    G = eng.alterego(mp)
    assert np.array_equal(G.user.cpu().numpy(), ae["user"]) and np.array_equal(G.item.cpu().numpy(), ae["item"])
    assert np.array_equal(G.rating.cpu().numpy(), ae["rating"])
    assert np.array_equal(G.time.cpu().numpy(), ae["time"])
    assert eng.n_profiles(G) == ae["n_profiles"]
    xo.ext_free(Xo)
    xo.sim_free(So)
    return eng, S, E, (n_top, choice, mp), G


@pytest.mark.parametrize("method", METHODS)
def test_c1_vs_oracle(dev, method):
    """BASELINE configs[0] size (10k users / 2x5k items): every stage against the CPU oracle."""
    from xmap.engine import synth
    _check_all_stages(dev, synth.config_c1(), method, 5)


# a sweep over shapes: sparse / dense, skewed, tiny, one domain much larger, heavy rows forced, many partitions
SWEEP = [
    dict(seed=101, users=40, src=15, tgt=15, overlap=0.6, k=2),
    dict(seed=102, users=300, src=40, tgt=200, overlap=0.3, k=3),
    dict(seed=103, users=800, src=300, tgt=60, overlap=0.5, k=7, mu=1.6),
    dict(seed=104, users=1500, src=120, tgt=120, overlap=0.9, k=4, zipf=1.3),
    dict(seed=105, users=2500, src=900, tgt=900, overlap=0.15, k=10),
    dict(seed=106, users=600, src=80, tgt=80, overlap=0.4, k=5, mu=2.4, sigma=0.8, sim_kw=dict(ch_min=64)),
    dict(seed=107, users=1200, src=250, tgt=250, overlap=0.35, k=6, sim_kw=dict(slot_target=32)),
    dict(seed=108, users=200, src=500, tgt=500, overlap=0.5, k=3, mu=3.0),
    dict(seed=109, users=900, src=260, tgt=260, overlap=0.5, k=100, mu=1.4),     # BASELINE configs[3]'s top-k
    dict(seed=110, users=500, src=150, tgt=150, overlap=0.6, k=64),
]


# The same shapes with work for stages B and C.  In SWEEP almost every item has a neighbour of the other domain, paths
# start from the items that have none, and so most entries enumerate no path at all (seeds 101, 102, 104, 106, 109: none in
# either method).  Here few users rate in both domains (overlap 0.03 .. 0.15): each entry carries the lower bounds its
# oracle census (golden_util.census) has to meet -- all but the tiny one 10^5 paths, 50 replaced items, an AlterEgo row of a
# replaced item and a candidate list the fused top-10 cuts; s209 lists of more than 2048 candidates, which one wave's
# selection cuts back more than once.  Behind each entry: the oracle's census (cosine | adjusted cosine; nb, paths, n_out,
# starts, max_cand, neg, mapped, mapped_rows) and the seconds of its one-thread extension.
_WORK = dict(paths=10 ** 5, mapped=50, mapped_rows=1, max_cand=11)
SWEEP_B = [
    # tiny.  44, 1 227, 467, 41, 26, 0, 15, 100 | 43, 410, 195, 19, 33, 52, 13, 94; 0.0 s
    dict(seed=201, users=60, src=60, tgt=60, overlap=0.1, k=2, need=dict(paths=1, mapped=1)),
    # source 14 times the target (1 643 + 120 items).  861, 135 655, 52 119, 118, 1 463, 0, 66, 1 340 |
    # 851, 133 023, 52 080, 119, 1 400, 12 153, 65, 575; 0.3 s
    dict(seed=202, users=2500, src=1800, tgt=120, overlap=0.1, k=6, need=_WORK),
    # target 11 times the source (320 + 3 651 items).  3 023, 5 220 852, 433 912, 3 247, 199, 0, 117, 6 056 |
    # 2 966, 1 178 871, 260 731, 3 274, 212, 84 007, 197, 7 742; 1.5 | 0.8 s
    dict(seed=203, users=2500, src=320, tgt=6000, overlap=0.04, k=5, mu=1.0, need=_WORK),
    # Zipf 1.3.  713, 13 565 319, 237 539, 578, 517, 0, 56, 3 528 | 686, 9 364 396, 225 757, 567, 499, 194 312, 76, 3 867; 2.9 | 1.9 s
    dict(seed=204, users=2500, src=900, tgt=900, overlap=0.1, k=6, zipf=1.3, need=_WORK),
    # k = 100 (BASELINE configs[3]'s top-k; similarity rows of up to 131 entries).  415, 7 288 193, 57 169, 243, 251, 0, 60, 338 |
    # 399, 5 260 779, 50 363, 227, 241, 11 951, 50, 209; 1.3 | 0.9 s
    dict(seed=205, users=500, src=300, tgt=300, overlap=0.03, k=100, d_min=3, mu=0.3, need=_WORK),
    # heavy rows forced in stage A.  326, 3 410 856, 107 593, 503, 374, 0, 54, 4 366 | 329, 824 794, 119 426, 554, 436, 25 965, 111, 5 758;
    # 0.6 | 0.2 s
    dict(seed=206, users=1500, src=600, tgt=600, overlap=0.06, k=5, mu=2.4, sigma=0.8, sim_kw=dict(ch_min=64), need=_WORK),
    # k = 64.  491, 26 857 963, 84 805, 311, 284, 0, 74, 368 | 471, 19 783 497, 76 689, 298, 270, 13 331, 55, 212; 5.6 | 3.9 s
    dict(seed=207, users=600, src=350, tgt=350, overlap=0.03, k=64, d_min=3, mu=0.3, need=_WORK),
    # many partitions.  303, 1 046 668, 162 735, 748, 534, 0, 104, 3 786 | 304, 486 985, 159 382, 748, 540, 45 747, 153, 3 937; 0.3 | 0.2 s
    dict(seed=208, users=2500, src=800, tgt=800, overlap=0.1, k=6, mu=1.2, sim_kw=dict(slot_target=32), need=_WORK),
    # candidate lists of more than 2048 entries.  2 809, 2 947 119, 1 120 204, 3 628, 2 483, 0, 827, 5 362 |
    # 2 819, 3 242 716, 1 324 750, 3 593, 2 546, 503 718, 1 054, 8 456; 1.5 | 1.4 s
    dict(seed=209, users=4000, src=4000, tgt=4000, overlap=0.15, k=5, mu=1.5, need=dict(_WORK, max_cand=2049)),
]


def sweep_ratings(cfg):
    from xmap.engine import synth
    kw = {n: cfg[n] for n in ("overlap", "mu", "sigma", "zipf", "d_min") if n in cfg}
    return synth.make_two_domain(cfg["seed"], cfg["users"], cfg["src"], cfg["tgt"], **kw)


@pytest.mark.parametrize("cfg", SWEEP + SWEEP_B, ids=lambda c: "s%d" % c["seed"])
@pytest.mark.parametrize("method", METHODS)
def test_shape_sweep_vs_oracle(dev, method, cfg):
    _check_all_stages(dev, sweep_ratings(cfg), method, cfg["k"], private=(cfg["seed"] % 2 == 0), picks_seed=cfg["seed"],
                      need=cfg.get("need"), **cfg.get("sim_kw", {}))


def test_edge_cases(dev):
    """empty input, a single user, users with one rating only (no pairs)."""
    attrs1 = (np.zeros(3, np.int32), np.zeros(3, np.int32), np.ones(3, np.uint32), np.ones(3, np.uint8))
    # users with a single rating each -> no pairs at all
    eng = _engine(dev, np.array([0, 1, 2, 3]), np.array([0, 1, 2]), np.array([5., 4., 3.]),
                  np.array([1, 2, 3]), 3, attrs1)
    S = eng.item_sim("cosine", CAP)
    assert S.n_kept == 0 and S.n_eval == 0
    E = eng.extend(S, 3, full=True)
    assert E.n_out == 0 and E.n_paths == 0
    n_top, choice, mp = eng.select(E, True)
    assert int(n_top.sum()) == 0 and (mp.cpu().numpy()[:3] == -1).all()
    G = eng.alterego(mp)
    assert G.n_rows == 0
    # one user, two items of one domain: one symmetric pair, no bridge
    eng = _engine(dev, np.array([0, 2]), np.array([0, 1]), np.array([5., 3.]), np.array([1, 2]), 3, attrs1)
    S = eng.item_sim("cosine", CAP)
    assert S.n_kept == 2 and S.n_eval == 2
    E = eng.extend(S, 3, full=True)
    assert int(E.bb.sum()) == 0 and E.n_out == 0


@pytest.mark.parametrize("method", METHODS)
def test_long_profiles_and_popular_items(dev, method):
    """Profiles of up to 1100 ratings (all three profile-sort paths: packed 16-lane groups, one wave, counted ranks
    through LDS and through the scratch array) and items rated by most users (LDS-privatised CSC build, heavy rows)."""
    from oracle import xmap_oracle as xo
    from xmap.engine import synth
    r = synth.make_two_domain(21, 600, 1500, 1500, overlap=0.5, mu=4.0, sigma=1.6)
    d = np.diff(r.user_ptr)
    assert d.max() > 1024 and (d > 64).sum() > 100 and (d <= 16).sum() > 10
    attrs = r.item_attrs()
    eng = _engine(dev, r.user_ptr, r.item, r.rating, r.time, r.n_items, attrs)
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *attrs)
    So = xo.item_sim(T, method, CAP, nthreads=8)
    orow, ocol = csr_to_pairs(So.row_ptr, So.col)
    from test_cpu_stage_a_layout import check_plan
    for ch_min, S in ((2048, eng.item_sim(method, CAP)), (64, eng.item_sim_tri(method, CAP, ch_min=64)),
                      (None, eng.item_sim(method, CAP, algo="rows"))):
        if ch_min is not None:      # the device's plan against its NumPy statement (test_cpu_stage_a_layout.py); 600 users: at 2048
            check_plan(S, r, ch_min)    # no threshold is searched (test_keys_larger_than_a_tile has the default one), at 64 one is
        assert S.n_eval == So.n_eval and S.n_contrib == So.n_contrib
        rows, cols, sim, mutu, nij = _sorted_sim(S)
        assert np.array_equal(rows, orow) and np.array_equal(cols, ocol)
        assert np.array_equal(mutu, So.mutu) and np.array_equal(nij, So.nij)
        assert np.array_equal(S.info.cpu().numpy(), So.info)
        assert np.array_equal(sim, So.sim)
    # the on-device CSC is a permutation of the ratings grouped by item
    R = eng.R
    ip = R.item_ptr.cpu().numpy()
    assert np.array_equal(np.diff(ip), np.bincount(r.item, minlength=r.n_items))
    iu, ir = R.item_user.cpu().numpy(), R.item_rating.cpu().numpy()
    users = np.repeat(np.arange(r.n_users), d)
    o = np.lexsort((users, r.item))
    for i in (0, int(np.argmax(np.diff(ip))), r.n_items - 1):
        a, b = ip[i], ip[i + 1]
        q = np.argsort(iu[a:b])
        assert np.array_equal(iu[a:b][q], users[o][a:b]) and np.array_equal(ir[a:b][q], r.rating[o][a:b])
    xo.sim_free(So)


# test_keys_larger_than_a_tile's input (also run through the coarse ABI: test_gpu_coarse_oracle.py): 8000 users, and every
# one of them also rates source item 7 and target item n_src + 11 (appended to the profile if absent).  -> (ratings, hubs)
def hub_ratings():
    from xmap.engine import synth
    r = synth.make_two_domain(31, 8000, 4000, 4000, overlap=0.4)
    hubs = (7, r.n_src_items + 11)
    rng = np.random.default_rng(5)
    ptr, item, rating, time = [0], [], [], []
    for u in range(r.n_users):
        a, b = int(r.user_ptr[u]), int(r.user_ptr[u + 1])
        it, ra, ti = list(r.item[a:b]), list(r.rating[a:b]), list(r.time[a:b])
        for h in hubs:
            if h not in it:
                it.append(h); ra.append(float(rng.integers(1, 6))); ti.append(int(rng.integers(synth.T0, synth.T1)))
        item += it; rating += ra; time += ti
        ptr.append(len(item))
    return synth.Ratings(np.asarray(ptr, np.int64), np.asarray(item, np.int32), np.asarray(rating, np.float32),
                         np.asarray(time, np.int64), r.n_items, r.n_src_items, r.src_numbers, r.tgt_numbers), hubs


@pytest.mark.parametrize("method", METHODS)
def test_keys_larger_than_a_tile(dev, method):
    """The two transpositions of stage A (rater records by item, kept pairs by heavier item: csrc/tilesort.h) with keys
    far larger than a tile: two items rated by every user (8000 raters; each is the partner of every lighter row, so its
    mirrored half has thousands of entries too), next to thousands of items with a handful.  Both sequences of the stage
    (round 3: one transposition, tile-sorted mirror; round 2: CSC + cursor-atomic mirror) against the oracle, bit for bit."""
    from oracle import xmap_oracle as xo
    from xmap.engine import synth
    from test_cpu_stage_a_layout import check_plan
    r, hubs = hub_ratings()
    ptr, item, rating, time = r.user_ptr, r.item, r.rating, r.time
    assert np.bincount(item, minlength=r.n_items)[list(hubs)].tolist() == [r.n_users, r.n_users]
    attrs = r.item_attrs()
    eng = _engine(dev, ptr, item, rating, time, r.n_items, attrs)
    T = xo.Train(ptr, item, rating, time, r.n_items, *attrs)
    So = xo.item_sim(T, method, CAP, nthreads=8)
    orow, ocol = csr_to_pairs(So.row_ptr, So.col)
    assert np.diff(So.row_ptr)[list(hubs)].min() > 3000
    old = os.environ.get("XMAP_A_V2")
    try:
        for v2 in ("0", "1"):
            os.environ["XMAP_A_V2"] = v2
            for ch_min in (1024, 64):
                S = eng.item_sim_tri(method, CAP, ch_min=ch_min)
                check_plan(S, r, ch_min)      # the device's plan against its NumPy statement (test_cpu_stage_a_layout.py)
                assert S.n_eval == So.n_eval and S.n_contrib == So.n_contrib
                rows, cols, sim, mutu, nij = _sorted_sim(S)
                assert np.array_equal(rows, orow) and np.array_equal(cols, ocol)
                assert np.array_equal(mutu, So.mutu) and np.array_equal(nij, So.nij)
                assert np.array_equal(S.info.cpu().numpy(), So.info)
                assert np.array_equal(S.u_avg.cpu().numpy()[:r.n_users], xo.user_info(T)[0])
                assert np.array_equal(sim, So.sim)
    finally:
        if old is None:
            os.environ.pop("XMAP_A_V2", None)
        else:
            os.environ["XMAP_A_V2"] = old
    # the rater counts of large inputs come from the partitioned count (k_cb_*: bucket histogram, scatter, LDS windows),
    # forced here on this input: the hub items are 8000 same-word increments of one window
    os.environ["XMAP_COUNT_PART_MIN"] = "1"
    try:
        S = eng.item_sim_tri(method, CAP)
        assert check_plan(S, r, 2048).n_heavy == 2      # the default threshold, found among 8000 users: the two hubs are heavy
        rows, cols, sim, mutu, nij = _sorted_sim(S)
        assert np.array_equal(rows, orow) and np.array_equal(cols, ocol) and np.array_equal(sim, So.sim)
        assert np.array_equal(S.info.cpu().numpy(), So.info)
    finally:
        os.environ.pop("XMAP_COUNT_PART_MIN", None)
    xo.sim_free(So)


def test_partitioned_count_on_random_shapes(dev):
    """xmap_sim3_layout's partitioned rater count (large inputs) forced on small random shapes, incl. fewer items than
    buckets and items beyond a bucket boundary: stage A against the oracle, bit for bit."""
    from oracle import xmap_oracle as xo
    from xmap.engine import synth
    os.environ["XMAP_COUNT_PART_MIN"] = "1"
    try:
        for seed, (U, Is, It) in enumerate(((300, 40, 50), (2500, 900, 700), (6000, 2100, 1900))):
            r = synth.make_two_domain(100 + seed, U, Is, It, overlap=0.3)
            attrs = r.item_attrs()
            eng = _engine(dev, r.user_ptr, r.item, r.rating, r.time, r.n_items, attrs)
            T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *attrs)
            So = xo.item_sim(T, "adjust_cosine", CAP, nthreads=8)
            S = eng.item_sim_tri("adjust_cosine", CAP)
            rows, cols, sim, mutu, nij = _sorted_sim(S)
            orow, ocol = csr_to_pairs(So.row_ptr, So.col)
            assert np.array_equal(rows, orow) and np.array_equal(cols, ocol) and np.array_equal(sim, So.sim)
            assert np.array_equal(S.info.cpu().numpy(), So.info)
            xo.sim_free(So)
    finally:
        os.environ.pop("XMAP_COUNT_PART_MIN", None)


def test_reverse_lists_fused_count_equals_separate_passes(dev, monkeypatch):
    """attach and rnn lists are counted in ONE pass over the matrix (xmap_reverse_count_att_rnn; its byte per entry serves both
    fill passes); XMAP_REV_SEPARATE=1 counts them in a pass each as rounds 1-4a did (mode 2 then writes its own bit): the
    three reverse adjacencies come out identical, also with every row walked by the 16-wave kernel of the long rows"""
    from xmap.engine import synth
    r = synth.make_two_domain(23, 3000, 700, 700, overlap=0.15)
    eng = _engine(dev, r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs())
    S = eng.item_sim("adjust_cosine", CAP)

    def lists():
        E = eng.ext_tables(S, 10)
        return [t.cpu().numpy() for name in ("att", "src", "rnn") for t in getattr(E, name)[:4]]
    fused = lists()
    monkeypatch.setenv("XMAP_REV_SEPARATE", "1")
    separate = lists()
    monkeypatch.setenv("XMAP_REV_LONG", "8")           # (rows of more than 8 entries: k_reverse_long)
    separate_long = lists()
    monkeypatch.delenv("XMAP_REV_SEPARATE")
    fused_long = lists()
    assert sum(len(x) for x in fused) > 1000
    for other in (separate, separate_long, fused_long):
        for x, y in zip(fused, other):
            assert np.array_equal(x, y)


def test_middle_lists_in_column_ranges(dev, monkeypatch):
    """k_mid_rows keeps the tile counters of XMAP_MID_ROWS_SPAN columns in LDS and builds wider rows range by range: with a
    span of 37 columns (several ranges per row here) the extension equals the one-range build and the oracle, bit for bit."""
    from oracle import xmap_oracle as xo
    from xmap.engine import synth
    r = synth.make_two_domain(17, 3000, 700, 700, overlap=0.15)
    attrs = r.item_attrs()
    eng = _engine(dev, r.user_ptr, r.item, r.rating, r.time, r.n_items, attrs)
    S = eng.item_sim("adjust_cosine", CAP)
    E0 = eng.extend(S, 10, full=True)
    assert E0.mid is not None and E0.mid.n_nb > 100
    monkeypatch.setenv("XMAP_MID_ROWS_SPAN", "37")
    E1 = eng.extend(S, 10, full=True)
    monkeypatch.delenv("XMAP_MID_ROWS_SPAN")
    assert E1.mid.n_tiles == E0.mid.n_tiles and E1.mid.n_records == E0.mid.n_records
    assert np.array_equal(E1.mid.dir_ptr.cpu().numpy(), E0.mid.dir_ptr.cpu().numpy())
    d0, d1 = E0.mid.dir.cpu().numpy().reshape(-1, 3), E1.mid.dir.cpu().numpy().reshape(-1, 3)
    assert np.array_equal(d0[:E0.mid.n_tiles], d1[:E1.mid.n_tiles])          # same tiles, same x order, same offsets
    assert E1.n_paths == E0.n_paths and E1.n_out == E0.n_out
    a, b = _xsim_lists(E0, r.n_items), _xsim_lists(E1, r.n_items)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *attrs)
    So = xo.item_sim(T, "adjust_cosine", CAP, nthreads=8)
    Xo = xo.extend(T, So, 10)
    assert E1.n_paths == Xo.n_paths
    ost, oen = csr_to_pairs(Xo.xs_ptr, Xo.xs_end)
    assert np.array_equal(b[0], ost) and np.array_equal(b[1], oen) and np.array_equal(b[2], Xo.xs_val)
    xo.ext_free(Xo)
    xo.sim_free(So)


def test_determinism_and_partitions(dev):
    """two runs give identical bytes; the result does not depend on the table partitioning."""
    from xmap.engine import synth
    r = synth.make_two_domain(9, 3000, 600, 600)
    eng = _engine(dev, r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs())
    a = _sorted_sim(eng.item_sim("adjust_cosine", CAP))
    b = _sorted_sim(eng.item_sim("adjust_cosine", CAP))
    c = _sorted_sim(eng.item_sim("adjust_cosine", CAP, slot_target=48))  # many partitions per item
    d = _sorted_sim(eng.item_sim("adjust_cosine", CAP, algo="rows"))     # first formulation: complete rows
    e = _sorted_sim(eng.item_sim("adjust_cosine", CAP, algo="rows", slot_target=48))
    f = _sorted_sim(eng.item_sim_tri("adjust_cosine", CAP, ch_min=64))   # forces heavy rows + rater chunks
    for x, y, z, w, v, t in zip(a, b, c, d, e, f):
        assert np.array_equal(x, y) and np.array_equal(x, z) and np.array_equal(x, w) and np.array_equal(x, v)
        assert np.array_equal(x, t)
    for m in ("cosine",):
        g = _sorted_sim(eng.item_sim(m, CAP))
        h = _sorted_sim(eng.item_sim(m, CAP, algo="rows"))
        k2 = _sorted_sim(eng.item_sim_tri(m, CAP, ch_min=64))
        for x, y, z in zip(g, h, k2):
            assert np.array_equal(x, y) and np.array_equal(x, z)
    # stage B: heavy starts split into chunks with dedicated rows + device merge == one wave per start
    S = eng.item_sim("adjust_cosine", CAP)
    E1 = eng.extend(S, 5, full=True, chunk=1 << 40)
    E2 = eng.extend(S, 5, full=True, chunk=64, n_slots=64)
    E3 = eng.extend(S, 5, full=True, algo="mid")               # middle lists + register-tile accumulation
    E4 = eng.extend(S, 5, full=True, algo="mid", chunk=64)
    E6 = eng.extend(S, 5, full=True, algo="enum")              # one accumulate per path
    os.environ["XMAP_MID_TABLE"] = "1"                        # middle lists through the dense tile table (n_nb > 40 000 form)
    try:
        E5 = eng.extend(S, 5, full=True, algo="mid")
    finally:
        del os.environ["XMAP_MID_TABLE"]
    os.environ["XMAP_SLOW_DIV"] = "1"                         # k_paths4<false>: the IEEE division of calculate_path_confidence
    try:
        E7 = eng.extend(S, 5, full=True)
    finally:
        del os.environ["XMAP_SLOW_DIV"]
    assert E1.fast_div == 1                                   # stage A's output always meets div_mid's precondition
    assert E5.mid.n_records == E3.mid.n_records and E5.mid.n_tiles == E3.mid.n_tiles
    assert np.array_equal(E5.mid.dir.view(-1, 3)[:, 0].cpu().numpy(), E3.mid.dir.view(-1, 3)[:, 0].cpu().numpy())   # (x, ne) per tile
    for Ex in (E3, E4, E5, E6, E7):
        assert Ex.n_paths == E1.n_paths and Ex.n_out == E1.n_out
        for x, y in zip(_xsim_lists(E1, r.n_items), _xsim_lists(Ex, r.n_items)):
            assert np.array_equal(x, y)
        assert np.array_equal(E1.top_end.cpu().numpy(), Ex.top_end.cpu().numpy())
        assert np.array_equal(E1.top_val.cpu().numpy(), Ex.top_val.cpu().numpy())
    assert E1.units.n_heavy == 0 and E2.units.n_heavy > 10
    assert E1.n_paths == E2.n_paths and E1.n_out == E2.n_out
    for x, y in zip(_xsim_lists(E1, r.n_items), _xsim_lists(E2, r.n_items)):
        assert np.array_equal(x, y)
    assert np.array_equal(E1.top_end.cpu().numpy(), E2.top_end.cpu().numpy())
    assert np.array_equal(E1.top_val.cpu().numpy(), E2.top_val.cpu().numpy())
    assert np.array_equal(E1.n_cand.cpu().numpy(), E2.n_cand.cpu().numpy())


def test_heavy_starts_with_long_candidate_lists(dev):
    """Starts split over dedicated rows whose candidate lists are long enough for every wave of the merge block to cut
    its running selection back several times (k_merge_groups + k_merge + finalize_slice with 16 waves) against the
    one-wave-per-start form (finalize_start), which test_c1_vs_oracle pins to the oracle at the same size."""
    from xmap.engine import synth
    r = synth.config_c1()
    eng = _engine(dev, r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs())
    S = eng.item_sim("adjust_cosine", CAP)
    E1 = eng.extend(S, 10, full=True, chunk=1 << 40)
    assert E1.units.n_heavy == 0
    assert int(E1.n_cand.max().item()) > 16 * 128          # slices longer than the selection buffer
    for chunk in (1 << 14, 1 << 11):                       # few rows per start / more than one merge group
        E2 = eng.extend(S, 10, full=True, chunk=chunk)
        assert E2.units.n_heavy > 10
        g = E2.units.unit_G.cpu().numpy()[:E2.units.n_units]
        if chunk == 1 << 11:
            assert g.max() > 12                            # more than one merge group
        assert E1.n_paths == E2.n_paths and E1.n_out == E2.n_out
        assert np.array_equal(E1.n_cand.cpu().numpy(), E2.n_cand.cpu().numpy())
        assert np.array_equal(E1.top_end.cpu().numpy(), E2.top_end.cpu().numpy())
        assert np.array_equal(E1.top_val.cpu().numpy(), E2.top_val.cpu().numpy())
        for x, y in zip(_xsim_lists(E1, r.n_items), _xsim_lists(E2, r.n_items)):
            assert np.array_equal(x, y)


def test_k50_vs_oracle(dev):
    """the list length of BASELINE configs[1] (k = 50) against the CPU oracle, every stage bit for bit: 9.5e7 paths, the
    largest case the one-thread oracle enumerates in about half a minute"""
    from xmap.engine import synth
    _check_all_stages(dev, synth.make_two_domain(11, 2000, 1000, 1000), "adjust_cosine", 50)


@pytest.mark.parametrize("method", METHODS)
def test_long_rows_of_the_reverse_lists(dev, method, monkeypatch):
    """every row of more than 64 entries through the 16-wave form of k_reverse (XMAP_REV_LONG): all stages against the
    oracle."""
    monkeypatch.setenv("XMAP_REV_LONG", "64")
    from xmap.engine import synth
    # (oracle census, cosine | adjusted cosine: 415 704 | 270 038 paths, longest candidate list 469 | 467, 99 | 131 replaced items)
    _check_all_stages(dev, synth.make_two_domain(5, 2000, 600, 600, overlap=0.1), method, 5, need=dict(paths=10 ** 5))


def knn_chunk_ratings():
    """test_rows_longer_than_one_knn_chunk's input (also run through the coarse ABI: test_gpu_coarse_oracle.py)"""
    from xmap.engine import synth
    return synth.make_two_domain(17, 2500, 3000, 3000, overlap=0.12, mu=3.6, sigma=1.0)


def test_rows_longer_than_one_knn_chunk(dev):
    """similarity rows of several thousand entries (k_knn_classify streams what follows its first 2048-entry chunk
    against the lists' thresholds): knn tables and everything downstream against the oracle.  One user in eight rates in
    both domains, so the long rows also feed paths (oracle census: 438 non-bridge items, 234 118 paths, 622 starts, longest
    candidate list 387, 127 replaced items, 14 402 AlterEgo rows of replaced items)."""
    r = knn_chunk_ratings()
    eng = _engine(dev, r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs())
    S = eng.item_sim("cosine", CAP)
    ln = np.diff(S.row_ptr.cpu().numpy())
    assert (ln > 2048).sum() > 200 and ln.max() > 4096
    del eng, S
    _check_all_stages(dev, r, "cosine", 3, need=dict(paths=10 ** 5, mapped=50))


def _ext_bytes(E, I):
    return [E.n_paths, E.n_out, E.n_cand.cpu().numpy()[:I], E.top_end.cpu().numpy()[:I], E.top_val.cpu().numpy()[:I]] + \
        list(_xsim_lists(E, I))


@pytest.mark.parametrize("case", ["c1", "s9"])
def test_second_pass_after_a_capacity_refusal(dev, case, monkeypatch):
    """Candidate lists that do not fit the list buffer (xs_cap): the enumeration refuses with XMAP_ERR_CAPACITY after a
    complete pass and extend_tables runs it again with the exact size, on the accumulator rows the refused pass left zeroed.
    xs_cap = 1, n_out - 1 (refused) and n_out (fits exactly: the kernel's test is off + nt <= xs_cap) give the default
    capacity's bytes in every formulation; the same engine at default capacity afterwards shows the rows it keeps are clean."""
    from xmap.engine import synth
    r = synth.config_c1() if case == "c1" else synth.make_two_domain(9, 3000, 600, 600)
    I = r.n_items
    eng = _engine(dev, r.user_ptr, r.item, r.rating, r.time, I, r.item_attrs())
    S = eng.item_sim("adjust_cosine", CAP)
    confs = [("cols", {}, None), ("enum", dict(algo="enum"), None), ("mid", dict(algo="mid"), None),
             ("heavy", dict(chunk=64), None), ("slow_div", {}, "1")]
    for name, kw, slow in confs:
        if slow:
            monkeypatch.setenv("XMAP_SLOW_DIV", slow)
        E0 = eng.extend(S, 5, full=True, **kw)
        want = _ext_bytes(E0, I)
        n_out = E0.n_out
        assert n_out > 2, name
        if name == "heavy":
            assert E0.units.n_heavy > 0
        for cap in (1, n_out - 1, n_out):
            E = eng.extend(S, 5, full=True, xs_cap=cap, **kw)
            assert E.xs_end.numel() == n_out, (name, cap)
            for x, y in zip(_ext_bytes(E, I), want):
                assert np.array_equal(x, y), (name, cap)
        for x, y in zip(_ext_bytes(eng.extend(S, 5, full=True, **kw), I), want):
            assert np.array_equal(x, y), (name, "after")
        monkeypatch.delenv("XMAP_SLOW_DIV", raising=False)


# ---------------------------------------------------------------------------------------------- index spaces with gaps
def engine_result(eng, S, E, sel, G, I, U, k):
    """what _check_all_stages returns, downloaded into a dict with the names golden_util.reindexed knows (entries of the knn
    tables behind a list's count: -1 / 0)"""
    rows, cols, sim, mutu, nij = _sorted_sim(S)
    n_top, choice, mp = sel
    cut = lambda t: t.cpu().numpy()[:I]
    kcnt = cut(E.kcnt)
    held = np.arange(k)[None, None, :] < kcnt[:, :, None]
    return dict(rows=rows, cols=cols, sim=sim, mutu=mutu, nij=nij, info=S.info.cpu().numpy(), uavg=S.u_avg.cpu().numpy()[:U],
                bb=cut(E.bb), cls=cut(E.cls), kcnt=kcnt, kcol=np.where(held, cut(E.kcol), -1), kval=np.where(held[..., None], cut(E.kval), 0.0),      # (kval: [I][2][k][3])
                n_paths=E.n_paths, n_out=E.n_out, n_cand=cut(E.n_cand), top_end=cut(E.top_end), top_val=cut(E.top_val),
                lists=_xsim_lists(E, I), n_top=cut(n_top), choice=cut(choice), map=cut(mp), user=G.user.cpu().numpy(),
                item=G.item.cpu().numpy(), rating=G.rating.cpu().numpy(), time=G.time.cpu().numpy(),
                n_target_rows=G.n_target_rows, n_profiles=eng.n_profiles(G))


def assert_same_results(got, want, what):
    assert got.keys() == want.keys(), what
    for name in got:
        x, y = got[name], want[name]
        for xx, yy in (zip(x, y) if isinstance(x, tuple) else [(x, y)]):
            assert np.array_equal(np.asarray(xx), np.asarray(yy)), (what, name)


# (SWEEP_B entry, arguments of Engine.extend, environment): the tiny entry; the entry with stage A's heavy rows, its starts
# split over dedicated rows as well; the tiny entry with the partitioned rater count, whole buckets of which are empty
GAPS = [(201, None, {}), (206, dict(chunk=64, n_slots=64), {}), (201, None, {"XMAP_COUNT_PART_MIN": "1"})]


def gap_case(seed):
    """(the SWEEP_B entry, its ratings, the stretched ratings, item map, user map)"""
    from golden_util import with_gaps
    cfg, = [c for c in SWEEP_B if c["seed"] == seed]
    r = sweep_ratings(cfg)
    return (cfg, r) + with_gaps(r, seed)


@pytest.mark.parametrize("seed,ext_kw,env", GAPS, ids=["tiny", "heavy", "tiny-partitioned-count"])
@pytest.mark.parametrize("method", METHODS)
def test_index_spaces_with_gaps(dev, method, seed, ext_kw, env, monkeypatch):
    """Item indices nobody rated and users without ratings, singly and in runs that empty whole waves, blocks, tiles and
    count buckets (golden_util.with_gaps), as a host that does not compact its ids uploads them: (a) every stage of the
    stretched input against the oracle, bit for bit; (b) against the engine's own results on the compact input, re-indexed
    -- pairs, similarities, item info, user averages, bridge flags, classes, knn tables, paths, candidate lists, top-10,
    choices, replacement map and AlterEgo rows; an unrated item has zero info, no class, no candidate and no replacement,
    a user without ratings the average 0.0 and no row.  (b) does not involve the oracle."""
    from golden_util import reindexed
    cfg, r, g, item_map, user_map = gap_case(seed)
    assert g.n_items > r.n_items + 4500 and g.n_users > r.n_users + 1470
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    kw = dict(private=(seed % 2 == 0), picks_seed=seed, need=cfg["need"], ext_kw=ext_kw)
    sim_kw = dict(cfg.get("sim_kw", {}))
    if env and not sim_kw:
        sim_kw = dict(slot_target=96)            # (item_sim_tri, the formulation test_keys_larger_than_a_tile forces the count on)
    res = _check_all_stages(dev, r, method, cfg["k"], **kw, **sim_kw)
    if ext_kw:
        assert res[2].units.n_heavy > 0
    compact = engine_result(*res, r.n_items, r.n_users, cfg["k"])
    del res
    stretched = engine_result(*_check_all_stages(dev, g, method, cfg["k"], **kw, **sim_kw), g.n_items, g.n_users, cfg["k"])   # (a)
    assert_same_results(stretched, reindexed(compact, item_map, user_map, g.n_items, g.n_users), "stretched vs compact")   # (b)
    assert compact["n_paths"] > 0 and (compact["map"] >= 0).any()
