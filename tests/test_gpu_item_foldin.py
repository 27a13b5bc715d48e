"""Item fold-in on the device (csrc/stage_e_itemfold.hip; xmap_itemfold_count / _fill / _audience_rows, xmap_ctx_item_foldin*,
Engine.item_foldin / item_foldin_tables / audience(batch=), session.recommend_audience_items / recommend_items): one row of
RecommenderSim for an item that arrived after training, its neighbour list, and the prediction, top-N and audience kernels
over the extended tables of I + n_new items.

The expected rows are tests/test_cpu_item_foldin_statement.py's Python statement, compared exactly (rows sorted by col; sim, ls,
avg and norm as uint64 views, a NaN ls as NaN); the expected lists are the oracle's ordering (|sim| descending, index ascending)
over those rows; the expected predictions, top-N lists and audiences are the brute-force statements of test_gpu_topn.py and
test_gpu_audience.py fed with the extended arrays."""
import ctypes as C
import types

import numpy as np
import pytest

from golden_util import CAP
from test_cpu_item_foldin_statement import FAMILIES, bits, copy_batch, dd_sum, item_foldin_statement, random_profiles, same_doubles
from test_gpu_audience import KEEP_HOLDERS, _window, audience, by_item
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_tail import _few_times, generate, neighbors, rec_sim, select, wtab
from test_gpu_topn import _random_case, _tool, check_output, expected, recommend, score_users, topn_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALPHA = 1.5


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


# ------------------------------------------------------------------------------------------------------------ helpers
def norms_of(I, item, rating):
    """the norms RecommenderSim uses: sqrt of the exact sum of squares of an item's ratings"""
    return np.asarray([np.sqrt(dd_sum([r * r for r in rating[item == i].tolist()])) for i in range(I)], np.float64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def sort_rows(row_ptr, col, *cols):
    """every row ordered by col (the order inside a row is unspecified)"""
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    o = np.lexsort((col, rows))
    return [col[o]] + [c[o] for c in cols]


def itemfold_rows(batch, prof, I, norms, cap, max_records=0):
    """xmap_itemfold_count + xmap_itemfold_fill on device copies: (row_ptr, col, sim, ls, nij, avg, norm, counts), rows sorted"""
    import torch
    from xmap.engine import hipabi as abi
    ptr, user, rating = _dev(batch[0].astype(np.int64)), _dev(batch[1].astype(np.int32)), _dev(batch[2].astype(np.float64))
    pptr, pitem, prating, d_norm = _dev(prof[0]), _dev(prof[1]), _dev(prof[2]), _dev(norms)
    B, nnz, U = len(batch[0]) - 1, len(batch[1]), len(prof[0]) - 1
    cnt = torch.full((max(B, 1),), -7, dtype=torch.int32, device=DEV)
    row_ptr = torch.full((B + 1,), -7, dtype=torch.int64, device=DEV)
    h = (C.c_int64 * 3)(-7, -7, -7)
    st = _stream()
    abi.check(abi.lib.xmap_itemfold_count(st, abi.i64(B), abi.i64(nnz), abi.vp(ptr), abi.vp(user), abi.i64(U), abi.i32(I), abi.vp(pptr),
                                          abi.vp(pitem), abi.i64(max_records), abi.vp(cnt), abi.vp(row_ptr), h))
    n = int(h[0])
    col = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    nij = torch.full((max(n, 1),), -7, dtype=torch.int32, device=DEV)
    sim, ls = [torch.full((max(n, 1),), -7.0, dtype=torch.float64, device=DEV) for _ in range(2)]
    avg, norm = [torch.full((max(B, 1),), -7.0, dtype=torch.float64, device=DEV) for _ in range(2)]
    abi.check(abi.lib.xmap_itemfold_fill(st, abi.i64(B), abi.i64(nnz), abi.vp(ptr), abi.vp(user), abi.vp(rating), abi.i64(U), abi.i32(I),
                                         abi.vp(pptr), abi.vp(pitem), abi.vp(prating), abi.vp(d_norm), abi.i32(cap), abi.i64(max_records),
                                         abi.vp(row_ptr), abi.vp(col), abi.vp(sim), abi.vp(ls), abi.vp(nij), abi.vp(avg), abi.vp(norm)))
    torch.cuda.synchronize()
    rp = row_ptr.cpu().numpy()
    assert rp[0] == 0 and rp[-1] == n and np.array_equal(np.diff(rp), cnt.cpu().numpy()[:B])
    c, s, l, k = sort_rows(rp, col.cpu().numpy()[:n], sim.cpu().numpy()[:n], ls.cpu().numpy()[:n], nij.cpu().numpy()[:n])
    return rp, c, s, l, k, avg.cpu().numpy()[:B], norm.cpu().numpy()[:B], tuple(int(x) for x in h)


def check_rows(got, want):
    row_ptr, col, sim, ls, nij, avg, norm = want
    assert got[0].tolist() == row_ptr.tolist()
    assert got[1].tolist() == col.tolist() and got[4].tolist() == nij.tolist()
    assert np.array_equal(bits(got[2]), bits(sim))
    assert same_doubles(got[3], ls)
    assert np.array_equal(bits(got[5]), bits(avg)) and np.array_equal(bits(got[6]), bits(norm))


def random_batch(rng, B, U, max_raters, family, prof_ptr):
    """B items with 0 .. max_raters raters: repeated raters and raters without rows among them"""
    lens = rng.integers(0, max_raters + 1, B)
    lens[0] = 0
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    user = rng.integers(0, U, int(ptr[-1])).astype(np.int32)
    empty = np.nonzero(np.diff(prof_ptr) == 0)[0]
    for q in range(1, B, 3):                            # a repeated rater and a rater without rows in every third item
        a, b = int(ptr[q]), int(ptr[q + 1])
        if b - a >= 3:
            user[a + 1] = user[a]
            if len(empty):
                user[a + 2] = empty[q % len(empty)]
    return ptr, user, np.asarray(FAMILIES[family](rng, int(ptr[-1])), np.float64)


def python_select(row_ptr, col, sim, ls, keep):
    """the oracle's rec_select ordering over sorted rows: |sim| descending, index ascending"""
    B = len(row_ptr) - 1
    cnt, ocol, osim, ols = np.zeros(B, np.int32), np.zeros((B, keep), np.int32), np.zeros((B, keep)), np.zeros((B, keep))
    for q in range(B):
        a, b = int(row_ptr[q]), int(row_ptr[q + 1])
        o = sorted(range(a, b), key=lambda k: (- abs(sim[k]), col[k]))[:keep]
        cnt[q] = len(o)
        ocol[q, :len(o)], osim[q, :len(o)], ols[q, :len(o)] = col[o], sim[o], ls[o]
    return cnt, ocol, osim, ols


def check_lists(got, want):
    """lists as (cnt, col, sim, ls): equal up to the count of every row"""
    assert got[0].tolist() == want[0].tolist()
    for q, c in enumerate(want[0].tolist()):
        assert got[1][q, :c].tolist() == want[1][q, :c].tolist(), q
        assert np.array_equal(bits(got[2][q, :c]), bits(want[2][q, :c])), q
        assert same_doubles(got[3][q, :c], want[3][q, :c]), q


def light_engine():
    """an Engine for the calls that take everything as arguments"""
    from xmap.engine import device
    eng = object.__new__(device.Engine)
    eng.dev, eng.timers, eng._scratch = DEV, None, {}
    return eng


def profile_view(U, I, ptr, item, rating, time=None):
    time = np.zeros(len(item), np.int64) if time is None else time
    return types.SimpleNamespace(n_users=U, n_items=I, user_ptr=_dev(ptr), user_item=_dev(item.astype(np.int32)),
                                 user_rating64=_dev(rating.astype(np.float64)), user_time=_dev(time.astype(np.int64)))


# ------------------------------------------------------------------------------------- 1. rows against the statement
@pytest.mark.parametrize("cap", [1, 5, 50])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_rows_equal_the_statement(family, cap):
    U, I, B = 300, 200, 40
    rng = np.random.default_rng(100 * cap + sorted(FAMILIES).index(family))
    prof = random_profiles(rng, U, I, 12, family)
    norms = norms_of(I, prof[1], prof[2])
    batch = random_batch(rng, B, U, 60, family, prof[0])
    want = item_foldin_statement(*batch, *prof, norms, cap)
    first = None
    for max_records in (1, 7, 1000, 0):
        got = itemfold_rows(batch, prof, I, norms, cap, max_records)
        check_rows(got, want)
        records = sum(int(prof[0][u + 1] - prof[0][u]) for u in batch[1].tolist())
        assert got[7] == (len(want[1]), records, int((np.diff(want[0]) > 0).sum()))
        first = first or got
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:7], first[:7]))
    assert want[0][1] == 0 and want[4].max() > 1 and len(want[1]) > 1000


def test_runs_on_either_side_of_a_wave():
    """one partner every user holds: the batch item rated by the first L users has a run of L records against it"""
    U, I, cap = 300, 50, 5
    rng = np.random.default_rng(7)
    ptr, item, rating = random_profiles(rng, U, I - 1, 4, "thirds")
    rows = [[(I - 1, float(rng.integers(1, 16)) / 3.0)] + list(zip(item[ptr[u]:ptr[u + 1]].tolist(), rating[ptr[u]:ptr[u + 1]].tolist()))
            for u in range(U)]
    for u in range(0, U, 9):
        rows[u] = rows[u][1:] + rows[u][:1]             # the shared partner last in some profiles
    pptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    prof = (pptr, np.asarray([x[0] for r in rows for x in r], np.int32), np.asarray([x[1] for r in rows for x in r], np.float64))
    norms = norms_of(I, prof[1], prof[2])
    lengths = [1, 63, 64, 65, 257, U]
    bptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    batch = (bptr, np.concatenate([np.arange(L) for L in lengths]).astype(np.int32),
             np.asarray(FAMILIES["thirds"](rng, int(bptr[-1])), np.float64))
    want = item_foldin_statement(*batch, *prof, norms, cap)
    runs = [int(want[4][k]) for q in range(len(lengths)) for k in range(want[0][q], want[0][q + 1]) if want[1][k] == I - 1]
    assert runs == lengths
    for max_records in (0, 100):
        check_rows(itemfold_rows(batch, prof, I, norms, cap, max_records), want)


# ----------------------------------------------------------------- 2. a copy of a resident item, through the coarse ABI
def item_foldin(ctx, batch):
    ptr, user, rating = batch[0].astype(np.int64), batch[1].astype(np.int32), batch[2].astype(np.float64)
    counts = np.full(3, -7, np.int64)
    ctx.call("xmap_ctx_item_foldin", len(ptr) - 1, _p(ptr, C.c_int64), _p(user, C.c_int32), _p(rating, C.c_double), _p(counts, C.c_int64))
    return tuple(counts.tolist())


def item_foldin_download(ctx, B, pairs, keep):
    rp, col, sim, ls, nij = np.full(B + 1, -7, np.int64), np.zeros(pairs, np.int32), np.zeros(pairs), np.zeros(pairs), np.zeros(pairs, np.int32)
    avg, norm = np.full(B, -7.0), np.full(B, -7.0)
    cnt, ncol, nsim, nls = np.full(B, -7, np.int32), np.zeros((B, keep), np.int32), np.zeros((B, keep)), np.zeros((B, keep))
    ctx.call("xmap_ctx_item_foldin_download", _p(rp, C.c_int64), _p(col, C.c_int32), _p(sim, C.c_double), _p(ls, C.c_double),
             _p(nij, C.c_int32), _p(avg, C.c_double), _p(norm, C.c_double), _p(cnt, C.c_int32), _p(ncol, C.c_int32),
             _p(nsim, C.c_double), _p(nls, C.c_double))
    assert rp[-1] == pairs
    c, s, l, k = sort_rows(rp, col, sim, ls, nij)
    return (rp, c, s, l, k, avg, norm), (cnt, ncol, nsim, nls)


def _resident_bytes(ctx, I, U, n_rows, keep):
    T = rec_sim_download(ctx, I, U, n_rows)
    return [T[k].tobytes() for k in sorted(T)] + [a.tobytes() for a in neighbors(ctx, I, keep)]


def rec_sim_download(ctx, I, U, n_rows):
    """test_gpu_tail.rec_sim without running the stage again"""
    ptr, pit, pra, pti = np.zeros(U + 1, np.int64), np.zeros(n_rows, np.int32), np.zeros(n_rows), np.zeros(n_rows, np.int64)
    ctx.call("xmap_ctx_rec_profiles_download", _p(ptr, C.c_int64), _p(pit, C.c_int32), _p(pra, C.c_double), _p(pti, C.c_int64))
    rp = np.zeros(I + 1, np.int64)
    ctx.call("xmap_ctx_rec_download", _p(rp, C.c_int64), None, None, None, None, None, None)
    n = int(rp[-1])
    col, sim, ls, nij, avg, norm = np.zeros(n, np.int32), np.zeros(n), np.zeros(n), np.zeros(n, np.int32), np.zeros(I), np.zeros(I)
    ctx.call("xmap_ctx_rec_download", _p(rp, C.c_int64), _p(col, C.c_int32), _p(sim, C.c_double), _p(ls, C.c_double),
             _p(nij, C.c_int32), _p(avg, C.c_double), _p(norm, C.c_double))
    return dict(ptr=ptr, item=pit, rating=pra, time=pti, row_ptr=rp, col=col, sim=sim, ls=ls, nij=nij, avg=avg, norm=norm)


@pytest.mark.parametrize("seed,users,src,tgt,overlap", [(5, 1500, 300, 300, 0.4), (7, 3000, 600, 80, 0.5)])
def test_a_copy_of_a_resident_item_through_the_coarse_abi(seed, users, src, tgt, overlap):
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(seed, users, src, tgt, overlap=overlap))
    I, U, keep = r.n_items, users, 10
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        cnt, col, sim, ls = select(ctx, I, keep)
        items = [i for i in range(r.n_src_items, I) if cnt[i] > 0]
        assert len(items) > 20
        before = _resident_bytes(ctx, I, U, len(rows["user"]), keep)
        batch = copy_batch(items, T["ptr"], T["item"], T["rating"])
        counts = item_foldin(ctx, batch)
        got, lists = item_foldin_download(ctx, len(items), counts[0], keep)
        assert counts[2] == len(items) and counts[1] >= counts[0] > 0
        res = sort_rows(T["row_ptr"], T["col"], T["sim"], T["ls"], T["nij"])
        compared = 0
        for q, i in enumerate(items):
            mine = np.arange(got[0][q], got[0][q + 1])
            mine = mine[got[1][mine] != i]
            theirs = np.arange(T["row_ptr"][i], T["row_ptr"][i + 1])
            theirs = theirs[res[0][theirs] != i]
            assert got[1][mine].tolist() == res[0][theirs].tolist(), i
            assert np.array_equal(bits(got[2][mine]), bits(res[1][theirs])), i
            assert same_doubles(got[3][mine], res[2][theirs]), i
            assert got[4][mine].tolist() == res[3][theirs].tolist(), i
            compared += len(mine)
        assert compared > 1000
        assert np.array_equal(bits(got[5]), bits(T["avg"][items])) and np.array_equal(bits(got[6]), bits(T["norm"][items]))
        # the whole result is the statement's, the lists the oracle's ordering over it
        want = item_foldin_statement(*batch, T["ptr"], T["item"], T["rating"], T["norm"], CAP)
        check_rows(got, want)
        check_lists(lists, python_select(*want[:4], keep))
        assert _resident_bytes(ctx, I, U, len(rows["user"]), keep) == before
    finally:
        ctx.close()


# --------------------------------------------------------------------------------- 3. lists and the extended tables
def _twin_case(seed):
    """items come as twins (j, j ^ 1) that every holder holds at one rating, with one norm: every batch row ties pairwise, and
    an odd keep cuts a pair; the batch names some raters twice"""
    U, I, B = 120, 60, 12
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(U):
        js = rng.choice(I // 2, int(rng.integers(0, 5)), replace=False) * 2
        rs = rng.integers(1, 11, len(js)) / 2.0
        rows.append([x for j, ra in zip(js.tolist(), rs.tolist()) for x in ((j, ra), (j + 1, ra))])
    pptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    prof = (pptr, np.asarray([x[0] for l in rows for x in l], np.int32), np.asarray([x[1] for l in rows for x in l], np.float64))
    norms = norms_of(I, prof[1], prof[2])
    assert np.array_equal(norms[0::2], norms[1::2])
    lens = rng.integers(1, 7, B)
    bptr = np.concatenate([[0], np.cumsum(2 * lens)]).astype(np.int64)
    raters = [rng.integers(0, U, int(n)) for n in lens]
    user = np.concatenate([np.concatenate([x, x]) for x in raters]).astype(np.int32)             # every rater twice
    batch = (bptr, user, rng.integers(1, 11, len(user)) / 2.0)
    return U, I, B, prof, norms, batch


@pytest.mark.parametrize("keep", [1, 5, 64])
def test_lists_and_extended_tables(keep):
    import torch
    U, I, B, prof, norms, batch = _twin_case(11)
    cap = 3
    want = item_foldin_statement(*batch, *prof, norms, cap)
    ties = sum(1 for q in range(B) for k in range(want[0][q], want[0][q + 1] - 1) if want[1][k] ^ 1 == want[1][k + 1] and want[2][k] == want[2][k + 1])
    assert ties > 20 and (np.diff(want[0]) > keep).any() == (keep < 64)
    rng = np.random.default_rng(12)
    r_cnt = rng.integers(0, keep + 1, I).astype(np.int32)
    r_col, r_sim, r_ls = rng.integers(0, I, (I, keep)).astype(np.int32), rng.normal(size=(I, keep)), rng.uniform(size=(I, keep))
    r_avg = rng.uniform(1.0, 5.0, I)
    eng = light_engine()
    P = profile_view(U, I, *prof)
    rows, avg, norm = eng.item_foldin(P, batch[0], batch[1], batch[2], _dev(norms), cap)
    assert rows.counts[0] == len(want[1]) and np.array_equal(bits(avg.cpu().numpy()), bits(want[5]))
    (x_cnt, x_col, x_sim, x_ls), x_avg = eng.item_foldin_tables((_dev(r_cnt), _dev(r_col), _dev(r_sim), _dev(r_ls)), _dev(r_avg), rows, keep)
    torch.cuda.synchronize()
    x_cnt, x_col, x_sim, x_ls, x_avg = [t.cpu().numpy() for t in (x_cnt, x_col, x_sim, x_ls, x_avg)]
    assert x_cnt.shape == (I + B,) and x_col.shape == (I + B, keep)
    assert all(a[:I].tobytes() == b.tobytes() for a, b in zip((x_cnt, x_col, x_sim, x_ls, x_avg), (r_cnt, r_col, r_sim, r_ls, r_avg)))
    check_lists((x_cnt[I:], x_col[I:], x_sim[I:], x_ls[I:]), python_select(*want[:4], keep))
    assert np.array_equal(bits(x_avg[I:]), bits(want[5])) and x_col[I:][x_cnt[I:, None] > np.arange(keep)[None, :]].max() < I


# ------------------------------------------------------- 4. predictions, top-N and audiences over the extended tables
def _extended_case(seed, U, I, B, keep, user_pool=None):
    """random profiles and resident lists (test_gpu_topn._random_case), a random batch, the extended arrays through the Engine"""
    import torch
    arrays = _random_case(seed, U, I, keep, np.arange(0, I, 2), lambda u: 2 + u % 7)
    rng = np.random.default_rng(seed + 1)
    norms = norms_of(I, arrays[1], arrays[2])
    lens = rng.integers(0, 9, B)
    bptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pool = np.arange(U) if user_pool is None else np.asarray(user_pool)
    batch = (bptr, pool[rng.integers(0, len(pool), int(bptr[-1]))].astype(np.int32), rng.integers(1, 16, int(bptr[-1])) / 3.0)
    eng = light_engine()
    P = profile_view(U, I, *arrays[:4])
    rows, _, _ = eng.item_foldin(P, batch[0], batch[1], batch[2], _dev(norms), 5)
    nb, x_avg = eng.item_foldin_tables(tuple(_dev(a) for a in arrays[4:7]), _dev(arrays[7]), rows, keep)
    torch.cuda.synchronize()
    ext = list(arrays[:4]) + [t.cpu().numpy() for t in nb[:3]] + [x_avg.cpu().numpy()]
    return eng, P, rows, nb, x_avg, ext, batch


def _with_raters_as_holders(inv, I, batch):
    """the brute-force statement knows holders from the profiles only: the holders of a batch item are its raters"""
    out = dict(inv)
    for q in range(len(batch[0]) - 1):
        raters = set(batch[1][batch[0][q]:batch[0][q + 1]].tolist())
        if I + q in out:
            out[I + q] = [(u, p, d, now, u in raters) for u, p, d, now, _ in out[I + q]]
    return out


def test_predictions_topn_and_audiences_over_the_extended_tables():
    import torch
    U, I, B, keep = 300, 400, 30, 3
    eng, P, rows, nb, x_avg, ext, batch = _extended_case(34, U, I, B, keep)
    scored = score_users(ALPHA, range(U), *ext, keep)
    assert sum(1 for l in scored.values() for c in l if c[0] >= I) > 100
    # top-N: batch items are listed as I + q (also for their raters: the frozen profiles do not hold them)
    for n, rank_by, flags in ((64, 0, 0), (10, 1, 1)):
        want = expected(scored, range(U), n, rank_by, bool(flags), 66)
        check_output(topn_rows(ext, U, I + B, keep, ALPHA, 66, list(range(U)), n, rank_by, flags), want, n)
    assert any(c[0] >= I for l in want[0] for c in l)
    # audience: the raters are the holders
    inv = _with_raters_as_holders(by_item(scored), I, batch)
    queries = list(range(I, I + B)) + [0, 2, I + B, -1, I]
    w = _dev(wtab(ALPHA, 66))
    seen = 0
    for n, rank_by, flags in ((1024, 0, 0), (1024, 1, KEEP_HOLDERS), (5, 0, KEEP_HOLDERS)):
        want = expected(inv, queries, n, rank_by, bool(flags), 66)
        got = eng.audience(P, nb, _dev(np.asarray(queries, np.int32)), x_avg, w, n, rank_by, bool(flags), batch=(rows.ptr, rows.user))
        torch.cuda.synchronize()
        check_output([t.cpu().numpy() for t in got[:4]] + [got[4]], want, n)
        if n == 1024:
            for q in range(B):
                raters = set(batch[1][batch[0][q]:batch[0][q + 1]].tolist())
                with_evidence = {c[0] for c in inv.get(I + q, []) if c[4] and c[1] is not None}
                assert with_evidence <= raters
                listed = {c[0] for c in want[0][q]}
                assert (with_evidence <= listed) if flags else not (raters & listed)
                seen += len(with_evidence)
    assert seen > 20
    # predictions of (user, batch item) pairs: the rounded scores of the statement
    tool = _tool(ALPHA)
    pairs = [(u, c[0]) for u in sorted(scored) for c in scored[u] if c[0] >= I and c[1] is not None][::3]
    score = {(u, c[0]): c for u in scored for c in scored[u]}
    plain, decay, status, _ = eng.predict(P, nb, _dev(np.asarray([p[0] for p in pairs], np.int32)),
                                          _dev(np.asarray([p[1] for p in pairs], np.int32)), x_avg, w, n_items=I + B)
    torch.cuda.synchronize()
    assert len(pairs) > 50 and not status.cpu().numpy().any()
    assert plain.cpu().numpy().tolist() == [tool.bound_rating(score[p][1]) for p in pairs]
    assert decay.cpu().numpy().tolist() == [tool.bound_rating(score[p][2]) for p in pairs]


def test_a_rater_in_the_last_word_of_a_window():
    import torch
    W = _window()
    U, I, B, keep = W + 70, 12, 3, 8            # keep = the most partners a batch item can have: every rater with rows has evidence
    rng = np.random.default_rng(35)
    users = np.unique(np.concatenate([[0, W - 33, W - 1, W, W + 69], rng.integers(0, U, 25)]))
    rows = {int(u): [(int(i), float(rng.integers(2, 21)) / 4.0, int(rng.integers(0, 4))) for i in rng.choice(I, 4, replace=False)] for u in users}
    ptr = np.zeros(U + 1, np.int64)
    for u, l in rows.items():
        ptr[u + 1] = len(l)
    np.cumsum(ptr, out=ptr)
    flat = [x for u in sorted(rows) for x in rows[u]]
    prof = (ptr, np.asarray([x[0] for x in flat], np.int32), np.asarray([x[1] for x in flat], np.float64), np.asarray([x[2] for x in flat], np.int64))
    norms = norms_of(I, prof[1], prof[2])
    batch = (np.asarray([0, 2, 4, 5], np.int64), np.asarray([W - 1, 0, W - 33, W + 69, W], np.int32), np.asarray([4.0, 2.5, 3.0, 1.5, 5.0]))
    eng = light_engine()
    P = profile_view(U, I, *prof)
    fold, _, _ = eng.item_foldin(P, batch[0], batch[1], batch[2], _dev(norms), 5)
    r_cnt, r_col, r_sim = np.zeros(I, np.int32), np.zeros((I, keep), np.int32), np.zeros((I, keep))
    nb, x_avg = eng.item_foldin_tables((_dev(r_cnt), _dev(r_col), _dev(r_sim)), _dev(np.round(rng.uniform(1.0, 5.0, I), 1)), fold, keep)
    torch.cuda.synchronize()
    ext = list(prof) + [t.cpu().numpy() for t in nb[:3]] + [x_avg.cpu().numpy()]
    inv = _with_raters_as_holders(by_item(score_users(ALPHA, sorted(rows), *ext, keep)), I, batch)
    queries = [I, I + 1, I + 2]
    w = _dev(wtab(ALPHA, 66))
    for flags in (0, KEEP_HOLDERS):
        want = expected(inv, queries, 64, 0, bool(flags), 66)
        got = eng.audience(P, nb, _dev(np.asarray(queries, np.int32)), x_avg, w, 64, 0, bool(flags), batch=(fold.ptr, fold.user))
        torch.cuda.synchronize()
        check_output([t.cpu().numpy() for t in got[:4]] + [got[4]], want, 64)
        listed = [{c[0] for c in l} for l in want[0]]
        assert ((W - 1) in listed[0]) == bool(flags) and ((W - 33) in listed[1]) == bool(flags) and (W in listed[2]) == bool(flags)
        assert all(len(l) > (2 if flags else 0) for l in listed)


def test_the_coarse_twins_over_the_extended_tables():
    from xmap.engine import synth
    r = _few_times(synth.make_two_domain(3, 800, 200, 200, overlap=0.4))
    I, U, keep, B = r.n_items, 800, 10, 25
    rng = np.random.default_rng(36)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        cnt, col, sim, ls = select(ctx, I, keep)
        lens = rng.integers(0, 30, B)
        bptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        batch = (bptr, rng.integers(0, U, int(bptr[-1])).astype(np.int32), rng.integers(2, 21, int(bptr[-1])) / 4.0)
        users = list(range(0, U, 3))
        before = recommend(ctx, users, 20, 1, 0, ALPHA)
        counts = item_foldin(ctx, batch)
        got, lists = item_foldin_download(ctx, B, counts[0], keep)
        want = item_foldin_statement(*batch, T["ptr"], T["item"], T["rating"], T["norm"], CAP)
        check_rows(got, want)
        check_lists(lists, python_select(*want[:4], keep))
        x_cnt = np.concatenate([cnt, lists[0]])
        x_col, x_sim = np.concatenate([col, lists[1]]), np.concatenate([sim, lists[2]])
        ext = [T["ptr"], T["item"], T["rating"], T["time"], x_cnt, x_col, x_sim, np.concatenate([T["avg"], got[5]])]
        scored = score_users(ALPHA, range(U), *ext, keep)
        # recommend: over all I + B items, batch items as I + q
        for n, rank_by, flags in ((20, 1, 0), (64, 0, 1)):
            q = np.ascontiguousarray(users, np.int32)
            o = [np.full(len(q), -7, np.int32), np.full((len(q), n), -7, np.int32), np.full((len(q), n), -7.0), np.full((len(q), n), -7.0)]
            stats = np.zeros(4, np.int64)
            ctx.call("xmap_ctx_item_foldin_recommend", len(q), _p(q, C.c_int32), n, rank_by, flags, _p(wtab(ALPHA, 66), C.c_double), 66,
                     _p(o[0], C.c_int32), _p(o[1], C.c_int32), _p(o[2], C.c_double), _p(o[3], C.c_double), _p(stats, C.c_int64))
            check_output(o + [stats.tolist()], expected(scored, users, n, rank_by, bool(flags), 66), n)
        assert (o[1] >= I).any()
        # audience: indices into the batch; outside the batch: no list
        inv = _with_raters_as_holders(by_item(scored), I, batch)
        for n, rank_by, flags in ((10, 0, 0), (200, 1, KEEP_HOLDERS)):
            qs = list(range(B)) + [-1, B, 0]
            want_a = expected(inv, [I + q if 0 <= q < B else -1 for q in qs], n, rank_by, bool(flags), 66)
            check_output(audience(ctx, qs, n, rank_by, flags, name="xmap_ctx_item_foldin_audience"), want_a, n)
        assert want_a[1][0] > 0
        # predict: (resident user, index into the batch)
        tool = _tool(ALPHA)
        score = {(u, c[0]): c for u in scored for c in scored[u]}
        pairs = [p for p in sorted(score) if p[1] >= I and score[p][1] is not None][::5]
        tu, ti = np.asarray([p[0] for p in pairs] + [0, 0], np.int32), np.asarray([p[1] - I for p in pairs] + [B, -1], np.int32)
        T_ = len(tu)
        plain, decay, status = np.zeros(T_), np.zeros(T_), np.full(T_, -1, np.int32)
        ctx.call("xmap_ctx_item_foldin_predict", T_, _p(tu, C.c_int32), _p(ti, C.c_int32), None, _p(wtab(ALPHA, 66), C.c_double), 66,
                 _p(plain, C.c_double), _p(decay, C.c_double), _p(status, C.c_int32), None, None)
        assert len(pairs) > 50 and status.tolist() == [0] * len(pairs) + [1, 1]
        assert plain[:-2].tolist() == [tool.bound_rating(score[p][1]) for p in pairs]
        assert decay[:-2].tolist() == [tool.bound_rating(score[p][2]) for p in pairs]
        # no resident answer has changed
        again = recommend(ctx, users, 20, 1, 0, ALPHA)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[:4], before[:4])) and again[4] == before[4]
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------- 5. misuse
def test_misuse_and_lifecycle():
    import torch
    from xmap.engine import hipabi as abi, synth
    # the fine-grained entry: every bad batch names its position and leaves the outputs untouched
    U, I = 50, 20
    rng = np.random.default_rng(37)
    prof = random_profiles(rng, U, I, 5, "halves")
    good = (np.asarray([0, 2, 2, 5], np.int64), np.asarray([1, 2, 3, 4, 5], np.int32), np.ones(5))
    bad = [((np.asarray([1, 2, 2, 5], np.int64), good[1]), b"ptr[0]"),
           ((np.asarray([0, 3, 2, 5], np.int64), good[1]), b"ptr[2]"),
           ((np.asarray([0, 2, 2, 4], np.int64), good[1]), b"ptr[3]"),
           ((good[0], np.asarray([1, 2, U, 4, 5], np.int32)), b"user[2]"),
           ((good[0], np.asarray([1, 2, 3, 4, -1], np.int32)), b"user[4]")]
    pptr, pitem = _dev(prof[0]), _dev(prof[1])
    for (ptr, user), where in bad:
        cnt = torch.full((3,), -7, dtype=torch.int32, device=DEV)
        row_ptr = torch.full((4,), -7, dtype=torch.int64, device=DEV)
        h = (C.c_int64 * 3)(-7, -7, -7)
        d_ptr, d_user = _dev(ptr), _dev(user)           # (named: the tensors must outlive the call)
        rc = abi.lib.xmap_itemfold_count(_stream(), abi.i64(3), abi.i64(5), abi.vp(d_ptr), abi.vp(d_user), abi.i64(U), abi.i32(I),
                                         abi.vp(pptr), abi.vp(pitem), abi.i64(0), abi.vp(cnt), abi.vp(row_ptr), h)
        assert rc == abi.ERR_ARG and where in abi.lib.xmap_last_error(), where
        assert (cnt.cpu().numpy() == -7).all() and (row_ptr.cpu().numpy() == -7).all() and list(h) == [-7, -7, -7]
    empty = itemfold_rows((np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0)), prof, I, np.ones(I), 5)
    assert empty[0].tolist() == [0] and empty[7] == (0, 0, 0)                # n_new = 0 is accepted
    # the coarse entry
    r = _few_times(synth.make_two_domain(3, 800, 200, 200, overlap=0.4))
    I, U, keep = r.n_items, 800, 10
    ctx = Ctx()
    try:
        ERR = ctx.abi.ERR_ARG

        def raw(batch):
            ptr, user, rating = batch[0].astype(np.int64), batch[1].astype(np.int32), np.ascontiguousarray(batch[2], np.float64)
            return ctx.lib.xmap_ctx_item_foldin(ctx.h, len(ptr) - 1, _p(ptr, C.c_int64), _p(user, C.c_int32), _p(rating, C.c_double), None)
        generate(ctx, r)
        assert raw(good) == ERR and b"have_rec" in ctx.lib.xmap_last_error()
        ctx.call("xmap_ctx_rec_sim", CAP, None)
        assert raw(good) == ERR and b"have_nb" in ctx.lib.xmap_last_error()         # before rec_select
        ctx.call("xmap_ctx_rec_select", keep)
        assert ctx.lib.xmap_ctx_item_foldin_download(ctx.h, *([None] * 11)) == ERR    # no batch yet
        counts = item_foldin(ctx, good)
        first = item_foldin_download(ctx, 3, counts[0], keep)
        coarse_bad = bad[:2] + [((good[0], np.asarray([1, 2, U, 4, 5], np.int32)), b"user[2]"),         # (ptr[n_new] defines nnz here)
                                ((good[0], np.asarray([1, 2, 3, 4, -1], np.int32)), b"user[4]")]
        for (ptr, user), where in coarse_bad:
            where = where.replace(b"ptr[2]", b"ptr[2] < ptr[1]")
            assert raw((ptr, user, good[2])) == ERR and where in ctx.lib.xmap_last_error(), where
            again = item_foldin_download(ctx, 3, counts[0], keep)                    # the previous batch is untouched
            assert all(a.tobytes() == b.tobytes() for x, y in zip(first, again) for a, b in zip(x, y))
        assert item_foldin(ctx, (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0))) == (0, 0, 0)       # n_new = 0
        assert audience(ctx, [0], 5, 0, 0, name="xmap_ctx_item_foldin_audience")[0].tolist() == [0]
        item_foldin(ctx, good)
        ctx.call("xmap_ctx_rec_select", keep)                                        # rec_select drops the batch
        assert ctx.lib.xmap_ctx_item_foldin_download(ctx.h, *([None] * 11)) == ERR and b"have_ifold" in ctx.lib.xmap_last_error()
        item_foldin(ctx, good)
        ctx.call("xmap_ctx_rec_sim", CAP, None)                                      # and so does rec_sim
        assert ctx.lib.xmap_ctx_item_foldin_download(ctx.h, *([None] * 11)) == ERR
    finally:
        ctx.close()


def test_item_foldin_on_a_union_context():
    from test_gpu_union import _trained_domains, _union
    doms = _trained_domains("multi", 2)
    numbers = np.unique(np.concatenate([r.tgt_numbers for r in doms]))
    U, I, keep, B = doms[0].n_users, len(numbers), 10, 12
    rng = np.random.default_rng(38)
    srcs, dst = [Ctx(), Ctx()], Ctx()
    try:
        user_maps, item_maps = [], []
        for c, r in zip(srcs, doms):
            generate(c, r)
            user_maps.append(rng.permutation(U).astype(np.int32))
            im = np.full(r.n_items, -1, np.int32)
            im[r.n_src_items:] = np.searchsorted(numbers, r.tgt_numbers)
            item_maps.append(im)
        rc, counts = _union(dst, srcs, user_maps, item_maps, U, I, 1)
        assert rc == 0 and counts[0] > 0
        T = rec_sim(dst, I, U, counts[0])
        cnt, col, sim, _ = select(dst, I, keep)
        lens = rng.integers(0, 20, B)
        bptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        batch = (bptr, rng.integers(0, U, int(bptr[-1])).astype(np.int32), rng.integers(2, 21, int(bptr[-1])) / 4.0)
        pairs = item_foldin(dst, batch)[0]
        got, lists = item_foldin_download(dst, B, pairs, keep)
        want = item_foldin_statement(*batch, T["ptr"], T["item"], T["rating"], T["norm"], CAP)
        check_rows(got, want)
        check_lists(lists, python_select(*want[:4], keep))
        ext = [T["ptr"], T["item"], T["rating"], T["time"], np.concatenate([cnt, lists[0]]), np.concatenate([col, lists[1]]),
               np.concatenate([sim, lists[2]]), np.concatenate([T["avg"], got[5]])]
        inv = _with_raters_as_holders(by_item(score_users(ALPHA, range(U), *ext, keep)), I, batch)
        want_a = expected(inv, [I + q for q in range(B)], 50, 1, False, 66)
        check_output(audience(dst, list(range(B)), 50, 1, 0, name="xmap_ctx_item_foldin_audience"), want_a, 50)
        assert want_a[1][0] > 0
    finally:
        for c in srcs + [dst]:
            c.close()


# -------------------------------------------------------------------------------------------------------- 6. session
def test_session_recommend_audience_items_equals_the_coarse_results():
    """the items of a batch under their labels, the users under their ids: label for label what the coarse ABI returns for the
    same rows, lists and batch in index space"""
    import datetime
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.engine import session, synth
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
    uids = ae.state.idt.uids
    rng = np.random.default_rng(39)
    B, keep = 15, 10
    new_items = [("N%03dT:" % q, [(uids[int(u)], float(rng.integers(2, 21)) / 4.0) for u in rng.integers(0, len(uids), int(rng.integers(0, 25)))])
                 for q in range(B)]
    new_items[3][1].append(("nobody", 3.0))
    # the same model and batch in index space, through the Engine calls the coarse ABI mirrors
    st, eng2, P, S, nb, item_avg = session._tail_setup(ae, CAP, keep, None, "test")
    I = len(st.idt.iids)
    uidx = {u: k for k, u in enumerate(uids)}
    bptr = np.concatenate([[0], np.cumsum([sum(1 for e in l if e[0] in uidx) for _, l in new_items])]).astype(np.int64)
    buser = np.asarray([uidx[e[0]] for _, l in new_items for e in l if e[0] in uidx], np.int32)
    brating = np.asarray([e[1] for _, l in new_items for e in l if e[0] in uidx], np.float64)
    prof = [t.cpu().numpy() for t in (P.user_ptr, P.user_item, P.user_rating64, P.user_time)]
    n_rows = int(prof[0][-1])
    want_rows = item_foldin_statement(bptr, buser, brating, prof[0], prof[1][:n_rows], prof[2][:n_rows], S.norm.cpu().numpy(), CAP)
    lists = python_select(*want_rows[:4], keep)
    ext_arrays = [prof[0], prof[1][:n_rows], prof[2][:n_rows], prof[3][:n_rows]] + \
                 [np.concatenate([a.cpu().numpy(), b]) for a, b in zip(nb, lists[:3])] + [np.concatenate([item_avg.cpu().numpy(), want_rows[5]])]
    inv = _with_raters_as_holders(by_item(score_users(ALPHA, range(len(uids)), *ext_arrays, keep)), I, (bptr, buser, brating))
    for n, decay, keep_holders in ((10, False, False), (100, True, True)):
        out = session.recommend_audience_items(ae, new_items, CAP, keep, ALPHA, n, decay=decay, keep_holders=keep_holders)
        want = expected(inv, [I + q for q in range(B)], n, 1 if decay else 0, keep_holders, 66)
        assert out.collect() == [(iid, [(uids[u], p, d) for u, p, d in l]) for (iid, _), l in zip(new_items, want[0])]
        assert out.unknown_users == 1 and tuple(out.stats) == tuple(want[1]) and out.counts[0] == len(want_rows[1])
    assert any(len(l) == 10 for _, l in session.recommend_audience_items(ae, new_items, CAP, keep, ALPHA, 10).collect())
    # held-out ratings of the new items
    some = score_users(ALPHA, range(0, len(uids), 7), *ext_arrays, keep)
    flat = {(u, c[0]): c for u, l in some.items() for c in l}
    test = []
    for u in sorted(some):
        mine = [c for c in some[u] if c[0] >= I and c[1] is not None]
        if mine:
            test.append((uids[u], [("N%03dT:" % (mine[0][0] - I), 4.0)]))
    res = session.recommend_items(ae, new_items, test, CAP, keep, ALPHA)
    ptool = _tool(ALPHA)
    for (uid, line), (_, pairs) in zip(res.collect(), test):
        c = flat[uidx[uid], I + int(pairs[0][0][1:4])]
        assert line == [(pairs[0][0], 4.0, ptool.bound_rating(c[1]), ptool.bound_rating(c[2]))]
    assert len(test) > 0 and res.mae is not None and res.mae[0] == len(test)
    with pytest.raises(ValueError):
        session.recommend_audience_items(ae, [(st.idt.iids[0], [])], CAP, keep, ALPHA, 10)
