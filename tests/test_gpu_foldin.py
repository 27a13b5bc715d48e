"""Fold-in (csrc/stage_c_foldin.hip; xmap_foldin_count / xmap_foldin_fill, xmap_ctx_foldin*, Engine.foldin_profiles,
session.recommend_topn_profiles / recommend_profiles): AlterEgo profiles, predictions and top-N lists for raw profiles that were
not rows of the ratings upload, from a model that stays frozen.

The training shape is one whose replacement map is not empty (each test asserts what it relies on).  Expected profiles come from
the CPU oracle's build_alterEgo over the batch with the map derived from the downloaded `choice`, or from a dozen-line Python
statement; expected lists and scores from the brute-force statement of test_gpu_topn.py over the expected profiles."""
import ctypes as C
import datetime

import numpy as np
import pytest

from golden_util import CAP
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_coarse_oracle import upload
from test_gpu_tail import _few_times, generate, group_by_user, neighbors, predict, rec_sim, select, wtab
from test_gpu_topn import KEEP_HELD, _tool, check_output, expected, recommend, score_users

pytestmark = pytest.mark.gpu
SHAPE = (7, 2000, 500, 500)
LADDER = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]      # both sides of the 16-lane / wave switch and of
ALPHA = 1.5                                                                      # the 64-entry chunk


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


# ------------------------------------------------------------------------------------------------------- the drivers
def foldin(ctx, ptr, item, rating, time):
    ptr, item = np.ascontiguousarray(ptr, np.int64), np.ascontiguousarray(item, np.int32)
    rating, time = np.ascontiguousarray(rating, np.float32), np.ascontiguousarray(time, np.int64)
    counts = np.full(3, -7, np.int64)
    ctx.call("xmap_ctx_foldin", len(ptr) - 1, _p(ptr, C.c_int64), _p(item, C.c_int32), _p(rating, C.c_float), _p(time, C.c_int64),
             _p(counts, C.c_int64))
    return counts.tolist()


def foldin_download(ctx, B, rows):
    ptr, it, ra, tm = np.full(B + 1, -7, np.int64), np.full(rows, -7, np.int32), np.full(rows, -7.0), np.full(rows, -7, np.int64)
    ctx.call("xmap_ctx_foldin_download", _p(ptr, C.c_int64), _p(it, C.c_int32), _p(ra, C.c_double), _p(tm, C.c_int64))
    return ptr, it, ra, tm


def foldin_recommend(ctx, queries, n, rank_by, flags, alpha=ALPHA, n_w=66):
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    cnt, item = np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32)
    plain, decay, stats = np.full((Q, n), -7.0), np.full((Q, n), -7.0), np.zeros(4, np.int64)
    ctx.call("xmap_ctx_foldin_recommend", Q, _p(q, C.c_int32), n, rank_by, flags, _p(w, C.c_double), n_w, _p(cnt, C.c_int32),
             _p(item, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), _p(stats, C.c_int64))
    return cnt, item, plain, decay, stats.tolist()


def foldin_predict(ctx, tu, ti, real, alpha=ALPHA, n_w=66):
    T = len(tu)
    tu, ti = np.ascontiguousarray(tu, np.int32), np.ascontiguousarray(ti, np.int32)
    real = None if real is None else np.ascontiguousarray(real, np.float64)
    w = wtab(alpha, n_w)
    plain, decay, status, mae, max_now = np.zeros(T), np.zeros(T), np.full(T, -1, np.int32), np.zeros(3), C.c_int32(-1)
    ctx.call("xmap_ctx_foldin_predict", T, _p(tu, C.c_int32), _p(ti, C.c_int32), _p(real, C.c_double), _p(w, C.c_double), n_w,
             _p(plain, C.c_double), _p(decay, C.c_double), _p(status, C.c_int32), _p(mae if real is not None else None, C.c_double),
             C.byref(max_now))
    return plain, decay, status, mae, max_now.value


def map_of(choice):
    """the replacement map a host derives from the downloaded choice: the largest start choosing an item wins"""
    m = np.full(len(choice), -1, np.int32)
    for s in range(len(choice)):
        if choice[s] >= 0:
            m[choice[s]] = s
    return m


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


class Trained(object):
    pass


@pytest.fixture(scope="module")
def trained():
    """upload -> item_sim (cosine, CAP) -> extend (k = 5) -> generate (private) -> rec_sim -> rec_select(10) on one context that
    the tests share (each leaves it with its tail and keep = 10), the downloaded arrays, and the oracle's map and rows"""
    from oracle import xmap_oracle as xo
    from xmap.engine import synth
    t = Trained()
    t.r = r = _few_times(synth.make_two_domain(*SHAPE))
    t.I, t.U = r.n_items, r.n_users
    t.ctx = Ctx()
    try:
        t.rows = generate(t.ctx, r)
        t.n_rows = len(t.rows["user"])
        t.T = rec_sim(t.ctx, t.I, t.U, t.n_rows)
        t.nb = select(t.ctx, t.I, 10)
        t.map = map_of(t.rows["choice"])
        To = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
        So = xo.item_sim(To, "cosine", CAP, nthreads=8)
        Xo = xo.extend(To, So, 5)
        _, _, m_o = xo.select(To, Xo, True, None)
        t.ae = xo.alterego(To, m_o)
        xo.ext_free(Xo); xo.sim_free(So)
        # what every test below relies on: a map with entries, equal to the oracle's, mapped rows, users with both kinds of row
        assert np.array_equal(t.map, m_o) and int((t.map >= 0).sum()) > 10
        assert len(t.ae["user"]) == t.n_rows and t.n_rows - t.rows["n_target_rows"] > 1000
        print("map entries %d, AlterEgo rows %d, mapped %d" % ((t.map >= 0).sum(), t.n_rows, t.n_rows - t.rows["n_target_rows"]))
        yield t
    finally:
        t.ctx.close()


# ------------------------------------------------------------------------------------ 1. the upload folded into itself
def test_the_upload_folded_into_itself(trained):
    t, ctx, r = trained, trained.ctx, trained.r
    U, I, T = t.U, t.I, t.T
    d = np.diff(r.user_ptr)
    assert (d == 16).any() and (d == 17).any() and (d > 16).sum() > 100 and d.max() < 64      # both paths of the AlterEgo kernel
    drawn = np.random.default_rng(7).integers(0, U, 300)
    queries = np.concatenate([drawn, [-1, U + 5, drawn[0]]]).astype(np.int32)
    rng = np.random.default_rng(8)
    tu, ti = rng.integers(0, U, 2000).astype(np.int32), rng.choice(np.unique(T["item"]), 2000).astype(np.int32)
    ti[::17] = -1
    tu[5::23] = -1
    real = rng.integers(1, 6, 2000).astype(np.float64)
    settings = [(n, rank_by, flags) for n in (1, 10, 64) for rank_by in (0, 1) for flags in (0, KEEP_HELD)]
    before = [recommend(ctx, queries, n, rank_by, flags, ALPHA) for n, rank_by, flags in settings]
    p_before = predict(ctx, tu, ti, real, ALPHA)
    assert before[2][4][0] > 0 and before[settings.index((10, 0, 0))][0].max() == 10 and (p_before[2] == 0).sum() > 1000
    assert (p_before[2] == 1).any() and p_before[3][0] > 0

    counts = foldin(ctx, r.user_ptr, r.item, r.rating, r.time)
    assert counts == [t.n_rows, t.rows["n_target_rows"], t.ae["n_profiles"]]
    first = foldin_download(ctx, U, t.n_rows)
    assert np.array_equal(first[0], T["ptr"]) and np.array_equal(first[1], T["item"]) and np.array_equal(first[3], T["time"])
    assert np.array_equal(first[2].view(np.uint64), T["rating"].view(np.uint64))
    for (n, rank_by, flags), want in zip(settings, before):
        got = foldin_recommend(ctx, queries, n, rank_by, flags)
        assert _same(got[:4], want[:4]) and got[4] == want[4], (n, rank_by, flags)
    p_got = foldin_predict(ctx, tu, ti, real)
    assert _same(p_got[:4], p_before[:4]) and p_got[4] == p_before[4]
    # the resident calls return what they returned before the fold-in
    for (n, rank_by, flags), want in zip(settings[2:5], before[2:5]):
        again = recommend(ctx, queries, n, rank_by, flags, ALPHA)
        assert _same(again[:4], want[:4]) and again[4] == want[4]
    p_again = predict(ctx, tu, ti, real, ALPHA)
    assert _same(p_again[:4], p_before[:4]) and p_again[4] == p_before[4]
    ptr2, it2, ra2, tm2 = np.zeros(U + 1, np.int64), np.zeros(t.n_rows, np.int32), np.zeros(t.n_rows), np.zeros(t.n_rows, np.int64)
    ctx.call("xmap_ctx_rec_profiles_download", _p(ptr2, C.c_int64), _p(it2, C.c_int32), _p(ra2, C.c_double), _p(tm2, C.c_int64))
    assert _same((ptr2, it2, ra2, tm2), (T["ptr"], T["item"], T["rating"], T["time"]))
    # a second identical fold-in gives identical bytes
    assert foldin(ctx, r.user_ptr, r.item, r.rating, r.time) == counts
    assert _same(foldin_download(ctx, U, t.n_rows), first)
    got = foldin_recommend(ctx, queries, 10, 1, 0)
    assert _same(got[:4], before[settings.index((10, 1, 0))][:4])


# ------------------------------------------------------- 2. an ad-hoc batch against the oracle and the brute-force statement
def _adhoc_batch(t, B=203, seed=11):
    rng = np.random.default_rng(seed)
    I, Is, m = t.I, t.r.n_src_items, t.map
    src = np.arange(Is)
    pools = [np.arange(I), src[m[:Is] >= 0], src[m[:Is] < 0], np.concatenate([np.arange(Is, I), src[m[:Is] >= 0]])]
    assert all(len(p) > 10 for p in pools)
    lens = [LADDER[b % 16] for b in range(B)]
    kinds = [(b // 16 + b) % 4 for b in range(B)]
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    item = np.concatenate([pools[k][rng.integers(0, len(pools[k]), n)] for k, n in zip(kinds, lens)]).astype(np.int32)
    rating = (rng.integers(2, 21, len(item)) / 4.0).astype(np.float32)        # multiples of 0.25: every group sum is exact
    time = 1000 + rng.integers(0, 7, len(item)).astype(np.int64)
    return ptr, item, rating, time, kinds


def test_an_adhoc_batch_against_the_oracle_and_the_statement(trained):
    from oracle import xmap_oracle as xo
    t, ctx = trained, trained.ctx
    I, B = t.I, 203
    ptr, item, rating, time, kinds = _adhoc_batch(t, B)
    assert B % 4 == 3 and len(item) == ptr[-1] > 10000
    ae = xo.alterego(xo.Train(ptr, item, rating, time, I, *t.r.item_attrs()), t.map)
    eptr, eit, era, eti = group_by_user(ae, B)
    n_rows, n_pass = len(ae["user"]), ae["n_target_rows"]
    rows_of, raw = np.diff(eptr), np.diff(ptr)
    n_mapped_entries = int((t.map[item] >= 0).sum())
    print("raw %d -> rows %d: pass-through %d, mapped %d (merged away %d); non-empty profiles without a row %d; > 64 rows: %d, "
          "> 128: %d" % (len(item), n_rows, n_pass, n_rows - n_pass, n_mapped_entries - (n_rows - n_pass),
                         ((raw > 0) & (rows_of == 0)).sum(), (rows_of > 64).sum(), (rows_of > 128).sum()))
    assert n_pass > 1000 and n_rows - n_pass > 500 and n_mapped_entries - (n_rows - n_pass) > 200
    assert ((raw > 0) & (rows_of == 0)).sum() > 10 and (rows_of > 64).sum() > 5 and (rows_of > 128).sum() > 0
    both = (t.r.item_attrs()[3][item] & 2 != 0) & (t.map[item] >= 0)                       # one entry, two rows
    print("entries that are pass-through and mapped: %d" % both.sum())

    counts = foldin(ctx, ptr, item, rating, time)
    assert counts == [n_rows, n_pass, ae["n_profiles"]] and ae["n_profiles"] == (rows_of > 0).sum()
    got = foldin_download(ctx, B, n_rows)
    assert np.array_equal(got[0], eptr) and np.array_equal(got[1], eit) and np.array_equal(got[3], eti)
    assert np.array_equal(got[2].view(np.uint64), era.view(np.uint64))

    cnt, col, sim, _ = neighbors(ctx, I, 10)
    queries = np.concatenate([np.arange(B), [-1, B, B + 7, 5]]).astype(np.int32)
    scored = score_users(ALPHA, queries, eptr, eit, era, eti, cnt, col, sim, t.T["avg"], 10)
    tool, pairs, full = _tool(ALPHA), set(), False
    for n, rank_by, flags in ((10, 0, 0), (10, 1, 0), (64, 1, KEEP_HELD), (1, 0, KEEP_HELD)):
        want = expected(scored, queries, n, rank_by, bool(flags), 66)
        out = foldin_recommend(ctx, queries, n, rank_by, flags)
        check_output(out, want, n)
        assert want[1][0] > 0 and want[1][2] <= 66                          # candidates were scored, none for want of a table
        full |= any(len(l) == n for l in want[0]) and n > 1
        assert out[0][-4] == 0 and out[0][-3] == 0 and out[0][-2] == 0     # -1, B, B + 7: users without rows
        pairs.update((int(u), it, p, d) for u, l in zip(queries, want[0]) for it, p, d in l)
    assert full
    pairs = sorted(pairs)
    assert len(pairs) > 500
    p_plain, p_decay, p_status, _, _ = foldin_predict(ctx, [p[0] for p in pairs], [p[1] for p in pairs], None)
    assert not p_status.any()
    assert p_plain.tolist() == [tool.bound_rating(p[2]) for p in pairs]
    assert p_decay.tolist() == [tool.bound_rating(p[3]) for p in pairs]


# ------------------------------------------------------------------------- 3. the fine-grained entries, a hand-made map
def alterego_statement(prof, flags, m):
    """build_alterEgo on one raw profile [(item, rating, time)*]: the pass-through rows in profile order, then one row per
    distinct replacement in first-seen order (np.mean of the group, the time of its first entry)"""
    rows = [(it, float(r), tm) for it, r, tm in prof if flags[it] & 2]
    groups = {}
    for it, r, tm in prof:
        if m[it] >= 0:
            groups.setdefault(int(m[it]), []).append((float(r), tm))
    return rows + [(tgt, float(np.mean([g[0] for g in grp])), grp[0][1]) for tgt, grp in groups.items()]


def _fine_case():
    I = 40
    flags = np.where(np.arange(I) < 20, 1, 2).astype(np.uint8)
    m = np.full(I, -1, np.int32)
    m[0:10] = [21, 22, 23, 21, 22, 23, 21, 21, 22, 23]      # ten sources onto three targets: different sources merge
    m[15:20] = [30, 31, 32, 33, 34]                         # 10 .. 14 have no replacement
    m[25] = 35                                              # a TARGET item with a replacement: one entry, two rows
    return I, flags, m


def _device_foldin(ptr, item, rating, time, I, flags, m, guard=False):
    """xmap_foldin_count (+ xmap_foldin_fill) on device copies; (rc, counts, cnt_t, cnt_m, prof_ptr[, rows])"""
    import torch
    from xmap.engine import hipabi as abi
    dev = "cuda:0"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    d_ptr, d_item, d_rating, d_time = up(ptr, np.int64), up(item, np.int32), up(rating, np.float32), up(time, np.int64)
    d_flags, d_map = up(flags, np.uint8), up(m, np.int32)
    B, nnz = len(ptr) - 1, len(item)
    cnt_t = torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev)
    cnt_m = torch.full((max(B, 1),), -7, dtype=torch.int32, device=dev)
    pptr = torch.full((B + 1,), -7, dtype=torch.int64, device=dev)
    h = (C.c_int64 * 3)(-7, -7, -7)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = abi.lib.xmap_foldin_count(st, abi.i64(B), abi.i64(nnz), abi.vp(d_ptr), abi.vp(d_item), abi.i32(I), abi.vp(d_flags), abi.vp(d_map),
                                   abi.vp(cnt_t), abi.vp(cnt_m), abi.vp(pptr), h)
    head = (rc, [int(x) for x in h], cnt_t.cpu().numpy(), cnt_m.cpu().numpy(), pptr.cpu().numpy())
    if rc != 0 or guard:
        return head
    n = int(h[0])
    pit = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    pra = torch.full((max(n, 1),), -7.0, dtype=torch.float64, device=dev)
    pti = torch.full((max(n, 1),), -7, dtype=torch.int64, device=dev)
    abi.check(abi.lib.xmap_foldin_fill(st, abi.i64(B), abi.i64(nnz), abi.vp(d_ptr), abi.vp(d_item), abi.vp(d_rating), abi.vp(d_time),
                                       abi.i32(I), abi.vp(d_flags), abi.vp(d_map), abi.vp(cnt_t), abi.vp(pptr), abi.vp(pit), abi.vp(pra),
                                       abi.vp(pti)))
    torch.cuda.synchronize()
    return head + ((pit.cpu().numpy()[:n], pra.cpu().numpy()[:n], pti.cpu().numpy()[:n]),)


def _ladder_batch(rng, B, I):
    lens = [LADDER[b % 16] for b in range(B)]
    ptr = np.zeros(B + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    item = rng.integers(0, I, ptr[-1]).astype(np.int32)
    rating = (rng.integers(2, 21, len(item)) / 4.0).astype(np.float32)
    time = rng.integers(0, 7, len(item)).astype(np.int64)
    return ptr, item, rating, time


def test_fine_grained_entries_with_a_hand_made_map():
    I, flags, m = _fine_case()
    B = 38                                                  # not a multiple of 4: the last group of four is partly empty
    ptr, item, rating, time = _ladder_batch(np.random.default_rng(3), B, I)
    want = [alterego_statement(list(zip(item[a:b].tolist(), rating[a:b].tolist(), time[a:b].tolist())), flags, m)
            for a, b in zip(ptr[:-1], ptr[1:])]
    flat = [row for w in want for row in w]
    assert any(len(w) > 2 * 16 for w in want)
    rc, counts, cnt_t, cnt_m, pptr, rows = _device_foldin(ptr, item, rating, time, I, flags, m)
    assert rc == 0
    n_t = [sum(1 for it in item[a:b] if flags[it] & 2) for a, b in zip(ptr[:-1], ptr[1:])]
    assert cnt_t.tolist() == n_t and cnt_m.tolist() == [len(w) - k for w, k in zip(want, n_t)]
    assert pptr.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert counts == [len(flat), sum(n_t), sum(1 for w in want if w)]
    assert rows[0].tolist() == [x[0] for x in flat] and rows[2].tolist() == [x[2] for x in flat]
    assert np.array_equal(rows[1].view(np.uint64), np.asarray([x[1] for x in flat], np.float64).view(np.uint64))
    # what the case is for: merged groups of different sources, the two-row entry, entries without a row, a mean float32 lacks
    assert sum(cnt_m) < int((m[item] >= 0).sum()) and (item == 25).any() and (m[item] < 0).any() and ((flags[item] & 2) == 0).any()
    assert any(float(np.float32(x[1])) != x[1] for x in flat)
    # an empty batch, and a batch of empty profiles
    rc, counts, _, _, pptr, rows = _device_foldin(np.zeros(1, np.int64), [], [], [], I, flags, m)
    assert rc == 0 and counts == [0, 0, 0] and pptr.tolist() == [0] and len(rows[0]) == 0
    rc, counts, cnt_t, cnt_m, pptr, rows = _device_foldin(np.zeros(6, np.int64), [], [], [], I, flags, m)
    assert rc == 0 and counts == [0, 0, 0] and not pptr.any() and not cnt_t.any() and not cnt_m.any()


# -------------------------------------------------------------------------------------------- 4. validation and lifecycle
def _bad_batches(ptr, item, I, nnz_argument=True):
    """(what, ptr, item) for each kind of bad input; nnz stays len(item).  xmap_ctx_foldin has no nnz argument (nnz IS
    ptr[n_new] there), so the last kind exists for xmap_foldin_count only."""
    out = []
    for what, v in (("item = n_items", I), ("item = -1", -1)):
        it = item.copy()
        it[len(it) // 2] = v
        out.append((what, ptr, it))
    p = ptr.copy()
    p[3] = p[4] + 1                                           # p[2] <= p[3], p[3] > p[4]
    out.append(("decreasing ptr", p, item))
    p = ptr.copy()
    p[0] = 1
    out.append(("ptr[0] != 0", p, item))
    if nnz_argument:
        p = ptr.copy()
        p[-1] -= 1
        out.append(("ptr[n_new] != nnz", p, item))
    return out


def test_bad_batches_are_refused_by_the_device_check():
    """every bad batch goes to xmap_foldin_count alone, whose first step is k_foldin_check (it reads ptr[0 .. n_new] and
    item[0 .. nnz) only); nothing is written"""
    from xmap.engine import hipabi as abi
    I, flags, m = _fine_case()
    ptr, item, rating, time = _ladder_batch(np.random.default_rng(4), 20, I)
    assert _device_foldin(ptr, item, rating, time, I, flags, m, guard=True)[0] == 0
    for what, p, it in _bad_batches(ptr, item, I):
        rc, counts, cnt_t, cnt_m, pptr = _device_foldin(p, it, rating, time, I, flags, m, guard=True)
        assert rc == abi.ERR_ARG and abi.lib.xmap_last_error(), what
        assert counts == [-7] * 3 and (cnt_t == -7).all() and (cnt_m == -7).all() and (pptr == -7).all(), what


def test_validation_and_lifecycle_of_the_coarse_entries(trained):
    r = trained.r
    I = r.n_items
    B = 40
    ptr = np.ascontiguousarray(r.user_ptr[:B + 1], np.int64)
    item, rating, time = r.item[:ptr[-1]], r.rating[:ptr[-1]], r.time[:ptr[-1]]
    queries = np.arange(-1, B + 1).astype(np.int32)
    c = Ctx()
    try:
        ERR = c.abi.ERR_ARG

        def raw_foldin(p=ptr, it=item, n=B):
            p, it = np.ascontiguousarray(p, np.int64), np.ascontiguousarray(it, np.int32)
            return c.lib.xmap_ctx_foldin(c.h, n, _p(p, C.c_int64), _p(it, C.c_int32), _p(np.ascontiguousarray(rating, np.float32), C.c_float),
                                         _p(np.ascontiguousarray(time, np.int64), C.c_int64), None)

        def raw_recommend():
            q, w = np.zeros(1, np.int32), wtab(0.2, 8)
            oc, oi, op, od = np.zeros(1, np.int32), np.zeros(4, np.int32), np.zeros(4), np.zeros(4)
            return c.lib.xmap_ctx_foldin_recommend(c.h, 1, _p(q, C.c_int32), 4, 0, 0, _p(w, C.c_double), 8, _p(oc, C.c_int32),
                                                   _p(oi, C.c_int32), _p(op, C.c_double), _p(od, C.c_double), None)

        def raw_predict():
            q, w, o, s = np.zeros(1, np.int32), wtab(0.2, 8), np.zeros(1), np.zeros(1, np.int32)
            return c.lib.xmap_ctx_foldin_predict(c.h, 1, _p(q, C.c_int32), _p(q, C.c_int32), None, _p(w, C.c_double), 8, _p(o, C.c_double),
                                                 _p(o.copy(), C.c_double), _p(s, C.c_int32), None, None)
        assert raw_foldin() == ERR                                              # before upload
        upload(c, r)
        c.call("xmap_ctx_item_sim", 0, CAP, None, None)
        c.call("xmap_ctx_extend", 5, None, None)
        assert raw_foldin() == ERR and b"have_gen" in c.lib.xmap_last_error()  # before generate
        c.call("xmap_ctx_generate", 1, None, None, None, None)
        c.call("xmap_ctx_rec_sim", CAP, None)
        c.call("xmap_ctx_rec_select", 10)
        assert raw_recommend() == ERR and b"have_fold" in c.lib.xmap_last_error()      # before any fold-in
        assert raw_predict() == ERR
        assert c.lib.xmap_ctx_foldin_download(c.h, None, None, None, None) == ERR
        c.call("xmap_ctx_generate", 1, None, None, None, None)                 # drops the tail
        counts = foldin(c, ptr, item, rating, time)
        assert counts[0] > counts[1] > 0
        assert raw_recommend() == ERR and raw_predict() == ERR                 # before rec_sim / rec_select
        c.call("xmap_ctx_rec_sim", CAP, None)                                  # rec_sim and rec_select leave the batch
        assert raw_recommend() == ERR
        c.call("xmap_ctx_rec_select", 10)
        assert raw_recommend() == 0 and raw_predict() == 0
        batch = foldin_download(c, B, counts[0])
        lists = foldin_recommend(c, queries, 10, 1, 0)
        resident = recommend(c, queries, 10, 1, 0, ALPHA)
        assert lists[4][0] > 0 and lists[0][0] == 0 and lists[0][-1] == 0
        assert _same([x[:-1] for x in lists[:4]], [x[:-1] for x in resident[:4]])      # (the first B users of the upload, folded in)
        c.call("xmap_ctx_rec_select", 3)                                       # another keep: the batch stays
        assert _same(foldin_download(c, B, counts[0]), batch)
        assert not _same(foldin_recommend(c, queries, 10, 1, 0)[:4], lists[:4])
        c.call("xmap_ctx_rec_select", 10)
        assert _same(foldin_recommend(c, queries, 10, 1, 0)[:4], lists[:4])
        # bad input: refused on the host, the batch and the resident answers as they were
        for what, p, it in _bad_batches(ptr, np.ascontiguousarray(item, np.int32), I, nnz_argument=False):
            assert raw_foldin(p, it) == ERR and c.lib.xmap_last_error(), what
        assert raw_foldin(n=-1) == ERR
        assert _same(foldin_download(c, B, counts[0]), batch)
        assert _same(foldin_recommend(c, queries, 10, 1, 0)[:4], lists[:4])
        assert _same(recommend(c, queries, 10, 1, 0, ALPHA)[:4], resident[:4])
        # an empty batch replaces the batch
        assert foldin(c, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int64)) == [0, 0, 0]
        assert foldin_download(c, 0, 0)[0].tolist() == [0]
        empty = foldin_recommend(c, [0, -1], 10, 0, 0)
        assert empty[0].tolist() == [0, 0] and empty[4] == [0, 0, 0, 0]
        some = trained.T["item"][:50].tolist()                                 # a user without rows: what the resident call gives index -1
        assert _same(foldin_predict(c, [0] * 50, some, None)[:3], predict(c, [-1] * 50, some, None, ALPHA)[:3])
        # generate again drops the batch
        foldin(c, ptr, item, rating, time)
        c.call("xmap_ctx_generate", 1, None, None, None, None)
        assert raw_recommend() == ERR and c.lib.xmap_ctx_foldin_download(c.h, None, None, None, None) == ERR
        c.call("xmap_ctx_rec_sim", CAP, None)
        c.call("xmap_ctx_rec_select", 10)
        assert raw_recommend() == ERR                                          # the tail is back, the batch is not
        foldin(c, ptr, item, rating, time)
        assert _same(foldin_recommend(c, queries, 10, 1, 0)[:4], lists[:4])    # the reused context: the bytes of before
        c.call("xmap_ctx_extend", 5, None, None)                               # extend drops it too
        assert c.lib.xmap_ctx_foldin_download(c.h, None, None, None, None) == ERR
    finally:
        c.close()


# --------------------------------------------------------------------------------------------------- 5. the Python route
def test_session_profiles_equal_the_resident_route():
    """the training of test_gpu_topn.test_session_recommend_topn_equals_the_statement_on_id_strings at the shape whose map has
    entries; 120 train users' own records under NEW uids"""
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.engine import session, synth
    from xmap.engine.localrdd import LocalRDD
    from xmap.utils.assist import baseliner_calculate_sim_pipeline, extender_pipeline, generator_pipeline
    r = synth.make_two_domain(*SHAPE)
    t0 = datetime.datetime(2013, 3, 1)
    recs = [(u, [(i, ra, t0 + datetime.timedelta(days=(t * 7919) % 6)) for i, ra, t in prof]) for u, prof in r.train_records()]
    sc = SparkContext(conf=SparkConf())
    trainRDD = sc.parallelize(recs, 8).cache()
    tool = BaselinerSim("cosine", CAP)
    sim = baseliner_calculate_sim_pipeline(sc, tool, trainRDD)
    ext = extender_pipeline(sc, SQLContext(sc), tool, ExtendSim(5), sim)
    ae = generator_pipeline(Generator(1, 0.6, "cosine", 0.1), trainRDD, ext, True)
    assert int((ae.G.map >= 0).sum().item()) > 10 and ae.G.n_rows > ae.G.n_target_rows
    rng = np.random.default_rng(9)
    picked = [recs[int(x)] for x in rng.choice(len(recs), 120, replace=False)]
    assert any(len(p) > 16 for _, p in picked) and any(any("S:" in e[0] for e in p) and any("T:" in e[0] for e in p) for _, p in picked)
    uids = [u for u, _ in picked]
    profiles = [("new-" + u, list(p)) for u, p in picked]
    alpha = 1.5
    for n, decay, keep_held in ((10, False, False), (10, True, False), (3, True, True)):
        want = session.recommend_topn(ae, uids, CAP, 10, alpha, n, decay=decay, keep_held=keep_held)
        got = session.recommend_topn_profiles(ae, sc.parallelize(profiles, 4), CAP, 10, alpha, n, decay=decay, keep_held=keep_held)
        assert [l for _, l in got.collect()] == [l for _, l in want.collect()]
        assert [u for u, _ in got.collect()] == ["new-" + u for u in uids]
        assert got.stats == want.stats and got.unknown_items == 0 and got.counts[0] > got.counts[1] > 0
        assert got.sim_pairs == want.sim_pairs
    assert any(len(l) == 3 for _, l in got.collect()) and want.stats[0] > 0
    # an iid the train set does not know is dropped and counted
    extra = [(u, p[:1] + [("0000000000-unknown", 3.0, t0)] + p[1:]) for u, p in profiles[:7]] + profiles[7:]
    got2 = session.recommend_topn_profiles(ae, extra, CAP, 10, alpha, 3, decay=True, keep_held=True)
    assert got2.collect() == got.collect() and got2.unknown_items == 7
    with pytest.raises(ValueError):
        session.recommend_topn_profiles(ae, profiles + [profiles[3]], CAP, 10, alpha, 3)
    with pytest.raises(ValueError):                                            # a rating float32 does not hold
        session.recommend_topn_profiles(ae, [("x", [(picked[0][1][0][0], 0.1, t0)])], CAP, 10, alpha, 3)
    with pytest.raises(TypeError):
        session.recommend_topn_profiles(LocalRDD(ae.collect()), profiles, CAP, 10, alpha, 3)
    with pytest.raises(TypeError):
        session.recommend_profiles(LocalRDD(ae.collect()), profiles, [], CAP, 10, alpha)
    # held-out pairs: target items the neighbour lists know, for the same users under both names
    listed = sorted(want.sim_pairs)
    test = [[(listed[int(k)], float(rng.integers(1, 6))) for k in rng.integers(0, len(listed), 6)] + [("0000000000-unknown", 2.0)]
            for _ in uids]
    res = session.recommend(ae, [(u, prs) for u, prs in zip(uids, test)], CAP, 10, alpha)
    res2 = session.recommend_profiles(ae, profiles, [("new-" + u, prs) for u, prs in zip(uids, test)] + [("nobody", test[0])], CAP, 10, alpha)
    assert [l for _, l in res2.collect()[:-1]] == [l for _, l in res.collect()]
    assert res2.collect()[-1][0] == "nobody" and res.mae[0] > 100
    nobody = session.recommend(ae, [("A%013d" % (10 ** 9 + 1), test[0])], CAP, 10, alpha)
    assert res2.collect()[-1][1] == nobody.collect()[0][1]
    assert res2.mae[0] == res.mae[0] + nobody.mae[0] and res2.unknown_items == 0
    only = session.recommend_profiles(ae, profiles, [("new-" + u, prs) for u, prs in zip(uids, test)], CAP, 10, alpha)
    assert only.mae == res.mae and any(len(set(x[2:])) == 2 for _, l in only.collect() for x in l if x)
