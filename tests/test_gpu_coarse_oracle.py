"""The coarse C ABI (include/xmap_hip.h: xmap_ctx_*) against the CPU oracle on synthetic inputs chosen to reach each of its
own paths in csrc/api.hip: the stage-A retry loops and heavy-row phases, the row sizing and work-unit plan of stage B, the
xmap_extend_paths branch (no middle lists), the accumulator rows kept on a context across calls, and the upload from the
native feeder.  The coarse side is driven as a foreign host drives it: NumPy arrays through ctypes, no torch.  Every
stage is compared bit for bit (the coarse twin of test_gpu_parity._check_all_stages)."""
import ctypes as C
import re

import numpy as np
import pytest

from golden_util import CAP, METHODS, census, check_census, csr_to_pairs
from test_gpu_coarse_abi import Ctx, _draw, _p
from test_gpu_parity import GAPS, SWEEP, SWEEP_B, gap_case, hub_ratings, knn_chunk_ratings, sweep_ratings

pytestmark = pytest.mark.gpu

CODE = {"cosine": 0, "adjust_cosine": 1}


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """some tests plan the same input with the Python engine: torch opens the device before the first coarse context does
    (in the other order torch finds no device)"""
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")
SIGNED = (-2.5, -1.3, 0.0, 0.7, 1.9, 3.3)       # test_gpu_ratings.SIGNED


# ------------------------------------------------------------------------------------------------- the coarse driver
def upload(ctx, r):
    """xmap_ctx_upload_ratings on a synth.Ratings (or anything with its fields)"""
    pre, suf, mask, flags = [np.ascontiguousarray(a, t) for a, t in zip(r.item_attrs(), (np.int32, np.int32, np.uint32, np.uint8))]
    ptr, item = np.ascontiguousarray(r.user_ptr, np.int64), np.ascontiguousarray(r.item, np.int32)
    rating, time = np.ascontiguousarray(r.rating, np.float32), np.ascontiguousarray(r.time, np.int64)
    ctx.call("xmap_ctx_upload_ratings", len(ptr) - 1, r.n_items, _p(ptr, C.c_int64), _p(item, C.c_int32), _p(rating, C.c_float),
             _p(time, C.c_int64), _p(pre, C.c_int32), _p(suf, C.c_int32), _p(mask, C.c_uint32), _p(flags, C.c_uint8))


def stage_a(ctx, method, I, U):
    n_kept, n_eval = C.c_int64(0), C.c_int64(0)
    ctx.call("xmap_ctx_item_sim", CODE[method], CAP, C.byref(n_kept), C.byref(n_eval))
    n = n_kept.value
    rp, col, sim = np.zeros(I + 1, np.int64), np.zeros(n, np.int32), np.zeros(n)
    mutu, nij, info, uavg = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((I, 4)), np.zeros(U)
    ctx.call("xmap_ctx_sim_download", _p(rp, C.c_int64), _p(col, C.c_int32), _p(sim, C.c_double), _p(mutu, C.c_int32),
             _p(nij, C.c_int32), _p(info, C.c_double), _p(uavg, C.c_double))
    rows, cols = csr_to_pairs(rp, col)
    o = np.lexsort((cols, rows))
    return dict(n_eval=n_eval.value, rows=rows[o], cols=cols[o], sim=sim[o], mutu=mutu[o], nij=nij[o], info=info, uavg=uavg)


def per_start(n_cand, off, xe, xv):
    """the per-start lists of one enumeration, each start's ends ascending: (start, end, value)"""
    st, en, va = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0)]
    for s in np.nonzero(n_cand)[0]:
        e, v = xe[off[s]:off[s] + n_cand[s]], xv[off[s]:off[s] + n_cand[s]]
        o = np.argsort(e)
        st.append(np.full(len(e), s, np.int64)); en.append(e[o].astype(np.int64)); va.append(v[o])
    return np.concatenate(st), np.concatenate(en), np.concatenate(va)


def ext_download(ctx, I):
    n_cand, top_end, top_val = np.zeros(I, np.int32), np.zeros((I, 10), np.int32), np.zeros((I, 10))
    ctx.call("xmap_ctx_ext_download", _p(n_cand, C.c_int32), _p(top_end, C.c_int32), _p(top_val, C.c_double))
    return n_cand, top_end, top_val


def ext_lists(ctx, I, n_cand, n_out):
    off, xe, xv = np.zeros(I, np.int64), np.zeros(n_out, np.int32), np.zeros(n_out)
    ctx.call("xmap_ctx_ext_lists", _p(off, C.c_int64), _p(xe, C.c_int32), _p(xv, C.c_double))
    return per_start(n_cand, off, xe, xv)


def stage_b(ctx, k, I):
    n_out, n_paths = C.c_int64(0), C.c_int64(0)
    ctx.call("xmap_ctx_extend", k, C.byref(n_out), C.byref(n_paths))
    n_cand, top_end, top_val = ext_download(ctx, I)
    lists = ext_lists(ctx, I, n_cand, n_out.value)
    return dict(n_out=n_out.value, n_paths=n_paths.value, n_cand=n_cand, top_end=top_end, top_val=top_val, lists=lists)


def candidates(ctx, I):
    n_top = np.zeros(I, np.int32)
    ctx.call("xmap_ctx_candidates", _p(n_top, C.c_int32))
    return n_top


def stage_c(ctx, I, private, picks):
    choice = np.zeros(I, np.int32)
    n_rows, n_tgt = C.c_int64(0), C.c_int64(0)
    pk = None if picks is None else np.ascontiguousarray(picks, np.int32)
    ctx.call("xmap_ctx_generate", 1 if private else 0, _p(pk, C.c_int32), _p(choice, C.c_int32), C.byref(n_rows), C.byref(n_tgt))
    m = n_rows.value
    gu, gi, gr, gt = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m), np.zeros(m, np.int64)
    ctx.call("xmap_ctx_gen_download", _p(gu, C.c_int32), _p(gi, C.c_int32), _p(gr, C.c_double), _p(gt, C.c_int64))
    return dict(choice=choice, n_target_rows=n_tgt.value, user=gu, item=gi, rating=gr, time=gt)


def top10(n_cand, lists, I):
    """the fused top-XMAP_TOPC of stage B restated in NumPy: the 10 best of each list by (|xsim| desc, end asc); -1 / 0 behind"""
    te, tv = np.full((I, 10), -1, np.int32), np.zeros((I, 10))
    st, en, va = lists
    bounds = np.concatenate([[0], np.cumsum(n_cand[n_cand > 0])])
    for q, s in enumerate(np.nonzero(n_cand)[0]):
        e, v = en[bounds[q]:bounds[q + 1]], va[bounds[q]:bounds[q + 1]]
        best = np.lexsort((e, -np.abs(v)))[:10]
        te[s, :len(best)], tv[s, :len(best)] = e[best], v[best]
    return te, tv


def _same(a, b, what):
    """two results of the driver (dicts of arrays / numbers / tuples) bit for bit"""
    assert a.keys() == b.keys(), what
    for key in a:
        x, y = a[key], b[key]
        for xx, yy in (zip(x, y) if isinstance(x, tuple) else [(x, y)]):
            assert np.array_equal(np.asarray(xx), np.asarray(yy)), (what, key)
            assert np.asarray(xx).dtype == np.asarray(yy).dtype, (what, key)


# ------------------------------------------------------------------------------------------- the expected results
class Oracle(object):
    """every stage of one input on the CPU oracle"""

    def __init__(self, r, method):
        from oracle import xmap_oracle as xo
        self.xo, self.r, self.I = xo, r, r.n_items
        self.T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
        self.So = xo.item_sim(self.T, method, CAP, nthreads=8)
        self.Xo = None

    def stage_a(self):
        So = self.So
        rows, cols = csr_to_pairs(So.row_ptr, So.col)
        return dict(n_eval=So.n_eval, rows=rows, cols=cols, sim=So.sim, mutu=So.mutu, nij=So.nij, info=So.info,
                    uavg=self.xo.user_info(self.T)[0])

    def stage_b(self, k):
        if self.Xo is None or self.Xo.k != k:           # (asked twice where a census precedes the comparison)
            if self.Xo is not None:
                self.xo.ext_free(self.Xo)
            self.Xo = self.xo.extend(self.T, self.So, k)
        Xo = self.Xo
        n_cand = np.diff(Xo.xs_ptr).astype(np.int32)
        rows, ends = csr_to_pairs(Xo.xs_ptr, Xo.xs_end)
        lists = (rows, ends, Xo.xs_val)
        te, tv = top10(n_cand, lists, self.I)
        return dict(n_out=len(Xo.xs_end), n_paths=Xo.n_paths, n_cand=n_cand, top_end=te, top_val=tv, lists=lists)

    def n_top4(self):
        return self.xo.select(self.T, self.Xo, False, None)[0]

    def stage_c(self, private, picks):
        _, choice, m = self.xo.select(self.T, self.Xo, private, picks)
        ae = self.xo.alterego(self.T, m)
        return dict(choice=choice, n_target_rows=ae["n_target_rows"], user=ae["user"], item=ae["item"], rating=ae["rating"],
                    time=ae["time"])

    def census(self, private, picks):
        """golden_util.census of the extension last made and the generation it leads to"""
        _, _, m = self.xo.select(self.T, self.Xo, private, picks)
        return census(self.So, self.Xo, m, self.xo.alterego(self.T, m))

    def close(self):
        if self.Xo is not None:
            self.xo.ext_free(self.Xo)
        self.xo.sim_free(self.So)


def _engine(r):
    from xmap.engine import device
    return device.Engine(device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))


class EngineStagesBC(Oracle):
    """stage A on the oracle, stages B and C on the Python engine (which the parity suite pins to the oracle): for inputs
    whose oracle extension is too slow"""

    def __init__(self, r, method):
        Oracle.__init__(self, r, method)
        self.eng = _engine(r)
        self.S = self.eng.item_sim(method, CAP)

    def stage_b(self, k):
        from test_gpu_parity import _xsim_lists
        I = self.I
        E = self.E = self.eng.extend(self.S, k, full=True)
        st, en, va = _xsim_lists(E, I)
        lists = (st.astype(np.int64), en.astype(np.int64), va)
        n_cand = E.n_cand.cpu().numpy()[:I]
        te, tv = top10(n_cand, lists, I)
        assert np.array_equal(E.top_end.cpu().numpy()[:I], te) and np.array_equal(E.top_val.cpu().numpy()[:I], tv)
        return dict(n_out=E.n_out, n_paths=E.n_paths, n_cand=n_cand, top_end=te, top_val=tv, lists=lists)

    def n_top4(self):
        return self.eng.select(self.E, False, None)[0].cpu().numpy()[:self.I]

    def stage_c(self, private, picks):
        _, choice, mp = self.eng.select(self.E, private, picks)
        G = self.eng.alterego(mp)
        return dict(choice=choice.cpu().numpy()[:self.I], n_target_rows=G.n_target_rows, user=G.user.cpu().numpy(),
                    item=G.item.cpu().numpy(), rating=G.rating.cpu().numpy(), time=G.time.cpu().numpy())


def _gen_args(n_top, private, picks_seed):
    """(private, picks) of one generation: seeded picks from n_top, or private where the reference's draw refuses"""
    if private:
        return True, None
    np.random.seed(picks_seed)
    try:
        return False, _draw(n_top)
    except ValueError:
        return True, None


def check_coarse(r, method, ks, private=True, picks_seed=None, ref=Oracle, ctx=None, need=None):
    """every stage of the coarse ABI on r against `ref`: stage A; for each k stage B, the non-private candidate counts and
    stage C (private, or non-private with seeded picks; a start with a single candidate makes the reference's randint
    refuse the draw: then private, as in test_gpu_parity._check_all_stages).  need: lower bounds on the oracle's census
    (golden_util.census) at every k, checked on the oracle's results before the context is touched.  Returns the coarse
    results."""
    I, U = r.n_items, len(r.user_ptr) - 1
    want = ref(r, method)
    own = ctx is None
    out = []
    try:
        if need is not None:
            for k in ks:
                want.stage_b(k)
                check_census(want.census(*_gen_args(want.n_top4(), private, picks_seed)), need, "%s, k = %d" % (method, k))
        ctx = ctx or Ctx()
        upload(ctx, r)
        A = stage_a(ctx, method, I, U)
        _same(A, want.stage_a(), "stage A")
        for k in ks:
            B = stage_b(ctx, k, I)
            _same(B, want.stage_b(k), "stage B, k = %d" % k)
            assert int(B["n_cand"].sum()) == B["n_out"]
            n_top = candidates(ctx, I)
            assert np.array_equal(n_top, want.n_top4())
            priv, picks = _gen_args(n_top, private, picks_seed)
            Cc = stage_c(ctx, I, priv, picks)
            _same(Cc, want.stage_c(priv, picks), "stage C, k = %d" % k)
            out.append((A, B, Cc))
    finally:
        want.close()
        if own and ctx is not None:
            ctx.close()
    return out


# ------------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("method", METHODS)
def test_c1_through_the_coarse_abi(method):
    """BASELINE configs[0] end to end, k = 5 and 10, private and non-private; at k = 20 the plan splits heavy starts into
    dedicated rows (a start needs more than 2^22 paths: xmap_path_plan's smallest chunk), checked against the Python engine"""
    from xmap.engine import synth
    r = synth.config_c1()
    check_coarse(r, method, (5, 10))
    check_coarse(r, method, (5,), private=False, picks_seed=3)
    eng = _engine(r)
    S = eng.item_sim(method, CAP)
    assert eng.extend(S, 10).units.n_heavy == 0
    assert eng.extend(S, 20).units.n_heavy > 0      # the same plan (default chunk divisor) as xmap_ctx_extend's
    del eng, S
    check_coarse(r, method, (20,), ref=EngineStagesBC)


@pytest.mark.parametrize("cfg", SWEEP + SWEEP_B, ids=lambda c: "s%d" % c["seed"])
@pytest.mark.parametrize("method", METHODS)
def test_shape_sweep_through_the_coarse_abi(method, cfg):
    """test_gpu_parity's sweeps: tiny, skewed and one-sided shapes, k up to 100; SWEEP_B's entries with the work for stages
    B and C that their census demands"""
    check_coarse(sweep_ratings(cfg), method, (cfg["k"],), private=(cfg["seed"] % 2 == 0), picks_seed=cfg["seed"],
                 need=cfg.get("need"))


def test_k50_through_the_coarse_abi():
    """the list length of BASELINE configs[1]"""
    from xmap.engine import synth
    check_coarse(synth.make_two_domain(11, 2000, 1000, 1000), "adjust_cosine", (50,))


@pytest.mark.parametrize("method", METHODS)
def test_hub_items_through_the_coarse_abi(method):
    """items with 8000 raters, far above the coarse stage A's heavy-row threshold (ch_min = 2048): k_pair_heavy and
    k_heavy_merge run; stages B and C against the Python engine"""
    r, hubs = hub_ratings()
    assert np.bincount(r.item, minlength=r.n_items)[list(hubs)].min() > 2048
    check_coarse(r, method, (5,), ref=EngineStagesBC)


@pytest.mark.parametrize("method", METHODS)
def test_wide_light_rows_through_the_coarse_abi(method):
    """light rows of 2 048 raters and more (test_cpu_stage_a_layout.wide_few: at the coarse stage A's own parameters, ch_min = 2048
    and slot_target = 768, two hubs of exactly 2 048 raters are class 4, five heavier ones heavy): the default route launches
    the 16-wave table; every stage against the oracle"""
    from test_cpu_stage_a_layout import plan_of, wide_few
    r, hubs = wide_few()
    P = plan_of("wide_few", 2048, 768)
    assert int((P.cls == 4).sum()) == 2 and P.n_heavy == 5
    check_coarse(r, method, (5,), need=dict(paths=1000, mapped=1))


@pytest.mark.parametrize("method", METHODS)
def test_long_profiles_through_the_coarse_abi(method):
    from xmap.engine import synth
    r = synth.make_two_domain(21, 600, 1500, 1500, overlap=0.5, mu=4.0, sigma=1.6)
    assert np.diff(r.user_ptr).max() > 1024
    check_coarse(r, method, (5,), private=False, picks_seed=21)


def test_rows_longer_than_one_knn_chunk_through_the_coarse_abi():
    r = knn_chunk_ratings()
    (A, _, _), = check_coarse(r, "cosine", (3,), need=dict(paths=10 ** 5, mapped=50))
    ln = np.bincount(A["rows"], minlength=r.n_items)
    assert (ln > 2048).sum() > 200 and ln.max() > 4096


@pytest.mark.parametrize("values", ["fractional", "signed"])
@pytest.mark.parametrize("method", METHODS)
def test_c1_nonintegral_ratings_through_the_coarse_abi(method, values):
    """ratings whose fp64 sums round: the upload picks XMAP_COSINE_EXACT, next to the heavy rows of configs[0]"""
    from xmap.engine import synth
    r = synth.config_c1()
    r = synth.fractional(r, seed=1) if values == "fractional" else synth.fractional(r, seed=4, values=SIGNED)
    check_coarse(r, method, (5,))


def _no_middle_items():
    """every user rates one source and one target item: each item with a pair has a neighbour of the other domain (all
    bridges); a second group rates two source items only (pairs without a bridge: class 0).  No class-2 item."""
    from xmap.engine import synth
    ptr, item = [0], []
    for u in range(60):
        item += [u % 5, 8 + u % 7]
        ptr.append(len(item))
    for u in range(21):
        item += [(5, 6), (6, 7), (5, 7)][u % 3]
        ptr.append(len(item))
    n = len(item)
    rng = np.random.default_rng(12)
    return synth.Ratings(np.asarray(ptr, np.int64), np.asarray(item, np.int32), (rng.integers(1, 6, n)).astype(np.float32),
                         rng.integers(synth.T0, synth.T1, n), 15, 8, None, None)


@pytest.mark.parametrize("method", METHODS)
def test_no_middle_lists_through_the_coarse_abi(method):
    """n_nb == 0 with kept pairs: run_enumeration's xmap_extend_paths branch over item-indexed rows"""
    r = _no_middle_items()
    eng = _engine(r)
    S = eng.item_sim(method, CAP)
    assert S.n_kept > 0
    E = eng.ext_tables(S, 3)
    assert eng.mid_lists(E) is None and int((E.cls.cpu().numpy()[:r.n_items] == 1).sum()) > 0
    del eng, S, E
    for k in (1, 3):
        check_coarse(r, method, (k,))


def _degenerate_inputs():
    from xmap.engine import synth
    z32, z64 = np.zeros(0, np.int32), np.zeros(0, np.int64)
    t = lambda n: np.arange(1, n + 1, dtype=np.int64)
    return [
        ("no items", synth.Ratings(np.zeros(4, np.int64), z32, np.zeros(0, np.float32), z64, 0, 0, None, None)),
        ("no users", synth.Ratings(np.zeros(1, np.int64), z32, np.zeros(0, np.float32), z64, 3, 2, None, None)),
        ("one rating each", synth.Ratings(np.arange(4, dtype=np.int64), np.arange(3, dtype=np.int32),
                                          np.asarray([5, 4, 3], np.float32), t(3), 3, 2, None, None)),
        ("one user, one domain", synth.Ratings(np.asarray([0, 2], np.int64), np.asarray([0, 1], np.int32),
                                               np.asarray([5, 3], np.float32), t(2), 3, 2, None, None)),
    ]


@pytest.mark.parametrize("method", METHODS)
def test_degenerate_inputs_through_the_coarse_abi(method):
    """empty and pairless inputs: every call returns XMAP_OK with empty or zero outputs, downloads take NULL and zero sizes"""
    for name, r in _degenerate_inputs():
        (A, B, Cc), = check_coarse(r, method, (3,))
        assert B["n_out"] == 0 and B["n_paths"] == 0 and len(Cc["user"]) == Cc["n_target_rows"], name
        assert len(A["rows"]) == (2 if name == "one user, one domain" else 0), name
        ctx = Ctx()
        try:
            upload(ctx, r)
            n_kept, n_eval = C.c_int64(-1), C.c_int64(-1)
            ctx.call("xmap_ctx_item_sim", CODE[method], CAP, C.byref(n_kept), C.byref(n_eval))
            ctx.call("xmap_ctx_item_sim", CODE[method], CAP, None, None)
            ctx.call("xmap_ctx_sim_download", None, None, None, None, None, None, None)
            ctx.call("xmap_ctx_extend", 3, None, None)
            ctx.call("xmap_ctx_ext_download", None, None, None)
            off = np.zeros(max(r.n_items, 1), np.int64)
            ctx.call("xmap_ctx_ext_lists", _p(off, C.c_int64), None, None)
            assert not off.any(), name
            ctx.call("xmap_ctx_generate", 1, None, None, None, None)
            ctx.call("xmap_ctx_gen_download", None, None, None, None)
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------------ 1b. index spaces with gaps
@pytest.mark.parametrize("seed,ext_kw,env", GAPS, ids=["tiny", "heavy", "tiny-partitioned-count"])
@pytest.mark.parametrize("method", METHODS)
def test_index_spaces_with_gaps_through_the_coarse_abi(method, seed, ext_kw, env, monkeypatch):
    """test_gpu_parity.test_index_spaces_with_gaps through the coarse door: the stretched upload (unrated item indices, users
    without ratings, in runs of thousands) against the oracle, and against the compact upload's own results re-indexed"""
    from golden_util import reindexed
    cfg, r, g, item_map, user_map = gap_case(seed)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    kw = dict(private=(seed % 2 == 0), picks_seed=seed, need=cfg["need"])
    (A, B, Cc), = check_coarse(r, method, (cfg["k"],), **kw)
    (Ag, Bg, Cg), = check_coarse(g, method, (cfg["k"],), **kw)                                      # (a)
    for got, compact, what in ((Ag, A, "stage A"), (Bg, B, "stage B"), (Cg, Cc, "stage C")):            # (b)
        _same(got, reindexed(compact, item_map, user_map, g.n_items, g.n_users), what + ", stretched vs compact")
    unrated = np.ones(g.n_items, bool)
    unrated[item_map] = False
    assert not Ag["info"][unrated].any() and not Bg["n_cand"][unrated].any() and (Cg["choice"][unrated] == -1).all()
    empty = np.ones(g.n_users, bool)
    empty[user_map] = False
    assert not Ag["uavg"][empty].any() and not empty[Cg["user"]].any()
    assert B["n_paths"] > 0 and len(Cc["user"]) > Cc["n_target_rows"]


# ------------------------------------------------------------------------------------- 1c. uploads the stages cannot take
def _arrays(r):
    pre, suf, mask, flags = [np.ascontiguousarray(a, t).copy() for a, t in zip(r.item_attrs(), (np.int32, np.int32, np.uint32, np.uint8))]
    return dict(ptr=np.ascontiguousarray(r.user_ptr, np.int64).copy(), item=np.ascontiguousarray(r.item, np.int32).copy(),
                rating=np.ascontiguousarray(r.rating, np.float32), time=np.ascontiguousarray(r.time, np.int64), pre=pre, suf=suf,
                mask=mask, flags=flags)


def _upload_rc(ctx, a, n_items):
    rc = ctx.lib.xmap_ctx_upload_ratings(ctx.h, len(a["ptr"]) - 1, n_items, _p(a["ptr"], C.c_int64), _p(a["item"], C.c_int32),
                                         _p(a["rating"], C.c_float), _p(a["time"], C.c_int64), _p(a["pre"], C.c_int32),
                                         _p(a["suf"], C.c_int32), _p(a["mask"], C.c_uint32), _p(a["flags"], C.c_uint8))
    return rc, ctx.lib.xmap_last_error().decode()


def _bad_uploads(r):
    """(what, arrays, the text xmap_last_error() has to hold): one offence each, the first offending position named"""
    u = r.n_users // 2
    e = int(r.user_ptr[u])                                   # user u holds at least five ratings (synth.make_two_domain)
    out = []
    a = _arrays(r); a["ptr"][0] = 1
    out.append(("user_ptr[0] != 0", a, r"user_ptr\[0\] = 1, not 0"))
    a = _arrays(r); a["ptr"][u + 1] = a["ptr"][u] - 1        # (user_ptr[n_users], all the old check read, is unchanged)
    out.append(("user_ptr decreases", a, r"user_ptr\[%d\] < user_ptr\[%d\]" % (u + 1, u)))
    a = _arrays(r); a["item"][e + 3] = a["item"][e + 1]
    out.append(("an item twice in a profile", a, r"user %d holds item %d twice \(item\[%d\] and item\[%d\]\)"
                % (u, a["item"][e + 1], e + 1, e + 3)))
    a = _arrays(r); a["item"][e + 2] = r.n_items
    out.append(("item out of range", a, r"item\[%d\] = %d outside \[0, %d\)" % (e + 2, r.n_items, r.n_items)))
    a = _arrays(r); a["suf"][7] = 32
    out.append(("suffix_cls = 32", a, r"suffix_cls\[7\] = 32 outside \[0, 32\)"))
    a = _arrays(r); a["suf"][r.n_items - 1] = -1
    out.append(("suffix_cls < 0", a, r"suffix_cls\[%d\] = -1 outside \[0, 32\)" % (r.n_items - 1)))
    a = _arrays(r); a["pre"][3] = -2
    out.append(("prefix_cls < 0", a, r"prefix_cls\[3\] = -2 is negative"))
    return out


def test_uploads_the_stages_cannot_take_are_refused():
    """xmap_ctx_upload_ratings checks what every stage assumes (xmap_check_ratings) before it drops, allocates or launches
    anything: XMAP_ERR_ARG with the first offending position in xmap_last_error(), on a fresh context and on one that holds
    an upload -- which then still answers xmap_ctx_item_sim with its previous result.  No stage is called after a refused
    upload on a context without a good one."""
    from xmap.engine import synth
    r = synth.make_two_domain(9, 300, 70, 70, overlap=0.4)
    bad = _bad_uploads(r)
    fresh = Ctx()
    try:
        for what, a, text in bad:
            rc, msg = _upload_rc(fresh, a, r.n_items)
            assert rc == fresh.abi.ERR_ARG, (what, msg)
            assert re.search(text, msg), (what, msg)
    finally:
        fresh.close()
    ctx = Ctx()
    try:
        upload(ctx, r)
        A = stage_a(ctx, "adjust_cosine", r.n_items, r.n_users)
        assert A["rows"].size > 0
        for what, a, text in bad:
            rc, msg = _upload_rc(ctx, a, r.n_items)
            assert rc == ctx.abi.ERR_ARG and re.search(text, msg), (what, msg)
            _same(stage_a(ctx, "adjust_cosine", r.n_items, r.n_users), A, "stage A after the refused upload: " + what)
    finally:
        ctx.close()


def test_the_engine_door_refuses_the_same_uploads():
    """DeviceRatings raises ValueError with the coarse door's text before anything is uploaded; AlterEgo profiles (rating64)
    may hold an item twice, nothing else"""
    from xmap.engine import device, synth
    r = synth.make_two_domain(9, 300, 70, 70, overlap=0.4)
    for what, a, text in _bad_uploads(r):
        attrs = (a["pre"], a["suf"], a["mask"], a["flags"])
        with pytest.raises(ValueError, match=text):
            device.DeviceRatings(a["ptr"], a["item"], a["rating"], a["time"], r.n_items, attrs)
        if what != "an item twice in a profile":
            with pytest.raises(ValueError, match=text):
                device.DeviceRatings(a["ptr"], a["item"], a["rating"], a["time"], r.n_items, attrs, rating64=True)
    a = [x for x in _bad_uploads(r) if x[0] == "an item twice in a profile"][0][1]
    P = device.DeviceRatings(a["ptr"], a["item"], a["rating"], a["time"], r.n_items, (a["pre"], a["suf"], a["mask"], a["flags"]),
                             rating64=True)
    assert P.nnz == r.nnz


# ---------------------------------------------------------------------------------------------- 2. context lifecycle
def _fresh(r, method, k, gen=((True, None),)):
    """one full pass on a new context: (stage A, stage B, [stage C per gen])"""
    ctx = Ctx()
    try:
        upload(ctx, r)
        A = stage_a(ctx, method, r.n_items, r.n_users)
        B = stage_b(ctx, k, r.n_items)
        return A, B, [stage_c(ctx, r.n_items, p, pk) for p, pk in gen]
    finally:
        ctx.close()


def test_context_lifecycle_equals_fresh_contexts():
    """One context through k changes (the end universe and so the row length change: rows reallocated and reused),
    repeated enumerations, private / non-private generation, a change of method, re-uploads of a larger, then a smaller
    dataset with fractional ratings, and a misuse error: every result equals a fresh context's for the same call."""
    from xmap.engine import synth
    r = synth.make_two_domain(9, 3000, 600, 600)
    big = synth.config_c1(seed=7)
    small = synth.fractional(synth.make_two_domain(106, 1200, 250, 250, overlap=0.4, mu=2.0), seed=6)
    I, U = r.n_items, r.n_users
    ctx = Ctx()
    try:
        upload(ctx, r)
        A = stage_a(ctx, "adjust_cosine", I, U)
        fresh = {}
        for k in (10, 3, 50, 10):                                        # 1. extend: realloc and reuse of the rows
            if k not in fresh:
                fresh[k] = _fresh(r, "adjust_cosine", k)
            _same(A, fresh[k][0], "stage A")
            B = stage_b(ctx, k, I)
            _same(B, fresh[k][1], "stage B, k = %d" % k)
        n_cand, top_end, top_val = ext_download(ctx, I)                  # 2. enumerations again: lists, then the candidates
        for _ in range(2):
            assert all(np.array_equal(x, y) for x, y in zip(ext_lists(ctx, I, n_cand, B["n_out"]), B["lists"]))
        for x, y in zip(ext_download(ctx, I), (B["n_cand"], B["top_end"], B["top_val"])):
            assert np.array_equal(x, y)
        np.random.seed(5)                                                # 3. private, non-private, private
        picks = _draw(candidates(ctx, I))
        gen = ((True, None), (False, picks), (True, None))
        want = _fresh(r, "adjust_cosine", 10, gen)[2]
        for (p, pk), w in zip(gen, want):
            _same(stage_c(ctx, I, p, pk), w, "stage C, private = %s" % p)
        fc = _fresh(r, "cosine", 10)                                     # 4. the other method in between
        _same(stage_a(ctx, "cosine", I, U), fc[0], "stage A, cosine")
        _same(stage_b(ctx, 10, I), fc[1], "stage B, cosine")
        _same(stage_c(ctx, I, True, None), fc[2][0], "stage C, cosine")
        _same(stage_a(ctx, "adjust_cosine", I, U), A, "stage A again")
        _same(stage_b(ctx, 10, I), fresh[10][1], "stage B again")
        for rr, method in ((big, "adjust_cosine"), (small, "cosine")):   # 5. re-uploads: larger, then smaller (fractional)
            f = _fresh(rr, method, 10)
            upload(ctx, rr)
            _same(stage_a(ctx, method, rr.n_items, rr.n_users), f[0], "stage A, re-upload")
            _same(stage_b(ctx, 10, rr.n_items), f[1], "stage B, re-upload")
            _same(stage_c(ctx, rr.n_items, True, None), f[2][0], "stage C, re-upload")
        abi = ctx.abi                                                    # 6. misuse, then a normal pass
        upload(ctx, r)
        assert ctx.lib.xmap_ctx_extend(ctx.h, 10, None, None) == abi.ERR_ARG and b"have_sim" in ctx.lib.xmap_last_error()
        assert ctx.lib.xmap_ctx_generate(ctx.h, 1, None, None, None, None) == abi.ERR_ARG
        assert ctx.lib.xmap_ctx_item_sim(ctx.h, 7, CAP, None, None) == abi.ERR_ARG
        _same(stage_a(ctx, "adjust_cosine", I, U), A, "stage A after misuse")
        assert ctx.lib.xmap_ctx_extend(ctx.h, 0, None, None) == abi.ERR_ARG
        _same(stage_b(ctx, 10, I), fresh[10][1], "stage B after misuse")
        _same(stage_c(ctx, I, True, None), want[0], "stage C after misuse")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------- 3. native feeder
def _feed_texts(r):
    """r as two Amazon-format texts (source, target) written by xmap_feed_format, as bench.py --api --feed does"""
    from xmap.engine import hipabi
    numbers = np.concatenate([r.src_numbers, r.tgt_numbers]).astype(np.int64)
    rating = np.ascontiguousarray(r.rating, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def text_of(lo, hi, fmt):
        n = C.c_int64(0)
        args = (C.c_int64(r.n_users), p(r.user_ptr), p(r.item), p(rating), p(r.time), b"A%013lld", fmt, p(numbers), C.c_int32(lo),
                C.c_int32(hi))
        hipabi.check(hipabi.lib.xmap_feed_format(*args, None, C.c_int64(0), C.byref(n)))
        buf = C.create_string_buffer(int(n.value))
        hipabi.check(hipabi.lib.xmap_feed_format(*args, buf, C.c_int64(int(n.value)), C.byref(n)))
        return buf.raw[:int(n.value)]
    return [(text_of(0, r.n_src_items, b"%010lld"), "S:"), (text_of(r.n_src_items, r.n_items, b"B0%08lld"), "T:")]


class _FeedRatings(object):
    """a feed's arrays as the coarse ABI's upload_feed sees them: ratings as float32, times = positions"""

    def __init__(self, feed):
        ptr, item, rating, _, attrs = feed.arrays()
        self.user_ptr, self.item, self.n_items, self.n_users = ptr, item, feed.n_items, feed.n_users
        self.rating = rating.astype(np.float32)
        assert np.array_equal(self.rating.astype(np.float64), rating)
        self.time = np.arange(len(item), dtype=np.int64)
        self._attrs = attrs

    def item_attrs(self):
        return self._attrs


@pytest.mark.parametrize("method", METHODS)
def test_upload_feed_equals_upload_ratings_and_the_oracle(method):
    """text -> native feeder -> xmap_ctx_upload_feed: every stage equals xmap_ctx_upload_ratings on the feed's arrays, and
    the oracle"""
    from xmap.engine import feeder, synth
    r = synth.make_two_domain(5, 2000, 400, 400)
    feed = feeder.Feed.from_texts(_feed_texts(r), 1970, 2100, 1)
    assert feed.nnz == r.nnz and feed.n_items == r.n_items and feed.n_users == r.n_users
    fr = _FeedRatings(feed)
    via_arrays = check_coarse(fr, method, (5,))
    ctx = Ctx()
    try:
        ctx.call("xmap_ctx_upload_feed", feed._h)
        A = stage_a(ctx, method, fr.n_items, fr.n_users)
        B = stage_b(ctx, 5, fr.n_items)
        Cc = stage_c(ctx, fr.n_items, True, None)
    finally:
        ctx.close()
    for x, y, what in zip((A, B, Cc), via_arrays[0], ("stage A", "stage B", "stage C")):
        _same(x, y, what + " from the feed")


def test_upload_feed_refuses_ratings_float32_cannot_hold():
    """the drop-in's rule at the coarse upload: 4.1 is refused naming the uid, the iid and the value; 4.5 is accepted.
    A refused upload leaves the context as it was."""
    from xmap.engine import feeder
    src = "u1\tA01\t4.0\t1356998400\nu1\tA02\t%s\t1356998401\nu2\tA01\t3.0\t1356998402\nu2\tA02\t2.0\t1356998403\n"
    tgt = "u1\tB01\t2.0\t1356998400\nu2\tB01\t5.0\t1356998401\nu2\tB02\t1.0\t1356998404\n"
    good = feeder.Feed.from_texts([(src % "4.5", "S:"), (tgt, "T:")], 1970, 2100, 1)
    bad = feeder.Feed.from_texts([(src % "4.1", "S:"), (tgt, "T:")], 1970, 2100, 1)
    ctx = Ctx()
    try:
        ctx.call("xmap_ctx_upload_feed", good._h)
        A = stage_a(ctx, "cosine", good.n_items, good.n_users)
        rc = ctx.lib.xmap_ctx_upload_feed(ctx.h, bad._h)
        msg = ctx.lib.xmap_last_error().decode()
        assert rc == ctx.abi.ERR_ARG, msg
        assert re.search(r"rating 4\.1 of user 'u1', item 'A02S:'.*float32", msg), msg
        _same(stage_a(ctx, "cosine", good.n_items, good.n_users), A, "stage A after a refused upload")
        nan = feeder.Feed.from_texts([(src % "nan", "S:"), (tgt, "T:")], 1970, 2100, 1)
        assert np.isnan(nan.arrays()[2]).sum() == 1
        ctx.call("xmap_ctx_upload_feed", nan._h)                       # NaN passes (session.check_float32)
    finally:
        ctx.close()
    assert A["rows"].size > 0 and 4.5 in good.arrays()[2]
