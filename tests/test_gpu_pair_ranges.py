"""The launches of the pair kernels in ranges (csrc/predict_rows.h: PAIR_RANGE, for_pair_ranges; the two launches of
pair_rows_run behind xmap_predict_rows, xmap_topn_rows, xmap_audience_rows and xmap_explain_rows, and xmap_explain_sources).

Part 1, small shapes: the designed cases of test_gpu_tail.py, test_gpu_explain.py, test_gpu_topn.py and test_gpu_audience.py
with XMAP_PAIR_RANGE = 1, 3, 4, 5 and 64 -- each result equals the Python statement the case is checked with there AND the
bytes of the same call with the variable unset (max_now, the stats and every status among them).  Where the test orders the
pairs itself, pairs with more than 128 evidence entries (the arena launch) sit on both sides of a range edge and at the end.

Part 2, the real limit: the smallest calls whose single grid would have 2^32 threads, on the designed model of
pair_range_statement.py (exact scores, no ties, a closed form: see test_cpu_pair_ranges.py).  Nothing of that size is made on
the host or copied from it."""
import ctypes as C
import functools
import os
import re
import time

import numpy as np
import pytest

import pair_range_statement as prs
import test_gpu_audience as t_aud
import test_gpu_explain as t_exp
import test_gpu_tail as t_tail
import test_gpu_topn as t_top

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ENV = "XMAP_PAIR_RANGE"
RANGES = [1, 3, 4, 5, 64]
PR_CAP = 128
ARENA_AT = (0, 2, 3, 4, 5, 63, 64)       # pair indices on both sides of an edge of every range in RANGES


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


def _pair_range():
    """work items per launch, read from the source"""
    src = open(os.path.join(ROOT, "x-map_amd", "csrc", "predict_rows.h")).read()
    m = re.search(r"constexpr long long PAIR_RANGE = (\d+)ll << (\d+);", src)
    assert m
    return int(m.group(1)) << int(m.group(2))


def test_the_range_constant_keeps_a_grid_below_2_32_threads():
    assert _pair_range() * 64 < 2 ** 32 and prs.THREADS_LIMIT_PAIRS > _pair_range() and prs.EXPLAIN_LIMIT_PAIRS * 16 > _pair_range()


def _blob(x):
    """the bytes of a result: arrays, numbers and nested tuples / lists of them"""
    if isinstance(x, (tuple, list)):
        return [_blob(y) for y in x]
    if x is None or isinstance(x, (int, float)):
        return x
    return (str(np.asarray(x).dtype), np.asarray(x).shape, np.asarray(x).tobytes())


def _arena_on_both_sides_of_an_edge(big, r):
    return any(big[e - 1] and big[e] for e in range(r, len(big), r))


def _place(filler, special, at=ARENA_AT):
    """`filler` with `special` (cycled) at the indices `at` and at the end; a length that is no multiple of 4"""
    out, f, s = [], list(filler), 0
    while f or len(out) <= max(at):
        if len(out) in at or not f:
            out.append(special[s % len(special)])
            s += 1
        else:
            out.append(f.pop(0))
    if len(out) % 4 == 3:
        out.append(out[1])
    return out + [special[s % len(special)]]


# ====================================================================================== part 1: the ranges on small shapes
# ------------------------------------------------------------------------------------- test_gpu_tail: evidence of 70 and 300
@functools.lru_cache(maxsize=None)
def _tail_case(copies):
    alpha = 1.5
    ratings, sims, info, test, line, sizes = t_tail._long_evidence_case(copies)
    single = [(u, [p]) for u, pairs in test for p in pairs]                 # one pair per line: the pair index is the line index
    test = _place(single, [line])
    want, nows, n_ev = t_tail._long_evidence_statement(ratings, sims, info, test, alpha)
    arrays = t_tail._case_arrays(ratings, sims, info, test, sizes[0], sizes[1], sizes[2])
    return test, want, nows, n_ev, arrays, sizes, alpha


def _tail_run(copies):
    """both calls of test_evidence_beyond_64_entries on the re-ordered pairs, each against the statement; what they returned"""
    test, want, nows, n_ev, arrays, (n_users, n_items, keep), alpha = _tail_case(copies)
    real = [p[1] for _, pairs in test for p in pairs]
    names = [p[0] for _, pairs in test for p in pairs]
    full = t_tail._predict_rows(arrays, n_users, n_items, keep, alpha, max(nows))
    plain, decay, status, max_now = full
    got = [(n, r, float(p), float(d)) if s == 0 else (() if s == 1 else None) for n, r, p, d, s in zip(names, real, plain, decay, status)]
    assert got == want and status[-1] == 0 and max_now == max(nows)
    short = t_tail._predict_rows(arrays, n_users, n_items, keep, alpha, 66)       # the table too short
    plain, decay, status, max_now = short
    assert max_now == max(nows) and status[-1] == 2
    for q, now in enumerate(nows):
        assert (status[q] == 2) == (now > 66)
        if status[q] != 2:
            assert got[q] == ((names[q], real[q], float(plain[q]), float(decay[q])) if status[q] == 0 else ())
    return _blob([full, short])


@functools.lru_cache(maxsize=None)
def _tail_whole(copies):
    return _tail_run(copies)


@pytest.mark.parametrize("r", RANGES)
@pytest.mark.parametrize("copies", [70, 300])
def test_tail_cases_in_ranges(monkeypatch, copies, r):
    monkeypatch.delenv(ENV, raising=False)
    n_ev = _tail_case(copies)[3]
    big = [n > PR_CAP for n in n_ev]
    assert max(n_ev) >= copies > 64 and len(n_ev) % 4 != 0 and len(n_ev) > 64
    if copies > PR_CAP:
        assert big[-1] and sum(big) >= 2 and _arena_on_both_sides_of_an_edge(big, r)
    whole = _tail_whole(copies)
    monkeypatch.setenv(ENV, str(r))
    assert _tail_run(copies) == whole


# ------------------------------------------------------------------- test_gpu_explain: the hand case and the staging case
def _explain_hand_run():
    """test_hand_case_through_the_engine for n_ev = 2 and 16, both orders, both tables, the sources with the merging map"""
    arrays, U, I, keep, cnt_t, raw_ptr, raw_item, flags, m = t_exp._tiny_case()
    pu, pi = [p[0] for p in t_exp.TINY_PAIRS], [p[1] for p in t_exp.TINY_PAIRS]
    eng, P = t_exp._engine(), t_exp._view(arrays, U, I)
    src = (t_exp._to(raw_ptr), t_exp._to(raw_item), t_exp._to(cnt_t), None, t_exp._to(flags), t_exp._to(m))
    out = []
    for n_ev in (2, 16):
        for rank_by in (0, 1):
            for n_w in (66, 2):
                w = t_exp.wtab(0.5, n_w)
                want = t_exp.explain_statement(pu, pi, arrays, keep, w, n_ev, rank_by)
                got = t_exp.engine_explain(arrays, U, I, pu, pi, w, n_ev, rank_by, P)
                t_exp.same(got[:7], want[:7], "n_w %d" % n_w)
                assert got[7] == want[7] == 6
                out.append(got)
            got = t_exp.engine_explain(arrays, U, I, pu, pi, t_exp.wtab(0.5, 66), n_ev, rank_by, P)
            for n_src in (1, 2, 8):
                total, pos = eng.explain_sources(P, t_exp._to(pu, np.int32), t_exp._to(got[2]), t_exp._to(got[4]), n_src, sources=src)
                want = t_exp.sources_statement(pu, got[2], got[4], arrays[0], arrays[1], cnt_t, raw_ptr, raw_item, flags, m, n_src)
                t_exp.same((total.cpu().numpy(), pos.cpu().numpy()), want, "n_src %d" % n_src)
                out.append((total.cpu().numpy(), pos.cpu().numpy()))
    return _blob(out)


@functools.lru_cache(maxsize=None)
def _explain_hand_whole():
    return _explain_hand_run()


@pytest.mark.parametrize("r", RANGES)
def test_explain_hand_case_in_ranges(monkeypatch, r):
    monkeypatch.delenv(ENV, raising=False)
    whole = _explain_hand_whole()
    monkeypatch.setenv(ENV, str(r))
    assert _explain_hand_run() == whole


@functools.lru_cache(maxsize=None)
def _staging_pairs():
    """the 300 / 129 / 128-entry case of test_evidence_beyond_the_lds_staging, its pairs re-ordered: arena pairs (300 and 129
    entries) at ARENA_AT and at the end"""
    arrays, U2, I, keep, dup_user, star = t_exp._staging_case()
    U = U2 - 2
    cnt, col = arrays[4], arrays[5]
    owners = [i for i in range(I) if 1 in col[i, :min(max(int(cnt[i]), 0), keep)].tolist()]     # items whose list holds the item held 300 times
    assert owners
    filler = [(dup_user, i) for i in range(I)] + [(U + 1, star), (3, 5), (4, 5), (5, 5), (-1, 5), (3, -1), (3, I), (U2, 5)]
    pairs = _place(filler, [(dup_user, owners[0]), (U, star)])
    pu, pi = [p[0] for p in pairs], [p[1] for p in pairs]
    # sources for the walk: the profile is its own raw profile, the first half of a user's rows pass-through rows (every item a
    # target item), the rest "mapped" by the identity: the group of a mapped row is every raw entry of its item -- 300 for one
    ptr, pit = arrays[0], arrays[1]
    cnt_t = (np.diff(ptr) // 2).astype(np.int32)
    flags, m = np.full(I, 2, np.uint8), np.arange(I, dtype=np.int32)
    return arrays, U2, I, keep, pu, pi, (ptr, pit, cnt_t, flags, m)


def _staging_run():
    arrays, U2, I, keep, pu, pi, (ptr, pit, cnt_t, flags, m) = _staging_pairs()
    eng, P = t_exp._engine(), t_exp._view(arrays, U2, I)
    src = (t_exp._to(ptr), t_exp._to(pit), t_exp._to(cnt_t), None, t_exp._to(flags), t_exp._to(m))
    out, totals = [], set()
    for n_ev, rank_by, n_w in ((16, 0, 400), (16, 1, 400), (3, 0, 400), (16, 1, 66)):
        w = t_exp.wtab(1.5, n_w)
        want = t_exp.explain_statement(pu, pi, arrays, keep, w, n_ev, rank_by)
        got = t_exp.engine_explain(arrays, U2, I, pu, pi, w, n_ev, rank_by, P)
        t_exp.same(got[:7], want[:7], (n_ev, rank_by, n_w))
        assert got[7] == want[7] > 129 and (n_w > 66 or (want[0] == 2).any())
        out.append(got)
        if n_w == 400:
            for n_src in (1, 8):
                total, pos = eng.explain_sources(P, t_exp._to(pu, np.int32), t_exp._to(got[2]), t_exp._to(got[4]), n_src, sources=src)
                want_s = t_exp.sources_statement(pu, got[2], got[4], ptr, pit, cnt_t, ptr, pit, flags, m, n_src)
                t_exp.same((total.cpu().numpy(), pos.cpu().numpy()), want_s, "sources %d" % n_src)
                totals |= set(want_s[0].ravel().tolist())
                out.append((total.cpu().numpy(), pos.cpu().numpy()))
    assert {0, 1, 129} <= totals         # padding, pass-through rows, a group of more raw entries than two chunks of the wave
    return _blob(out)


@functools.lru_cache(maxsize=None)
def _staging_whole():
    return _staging_run()


@pytest.mark.parametrize("r", RANGES)
def test_explain_staging_case_in_ranges(monkeypatch, r):
    monkeypatch.delenv(ENV, raising=False)
    arrays, U2, I, keep, pu, pi, _ = _staging_pairs()
    total = t_exp.explain_statement(pu, pi, arrays, keep, t_exp.wtab(1.5, 400), 1, 0)[1]
    big = (total > PR_CAP).tolist()
    assert sorted(set(total[total >= PR_CAP].tolist()))[:2] == [128, 129] and total.max() >= 300
    assert len(pu) % 4 != 0 and big[-1] and sum(big) >= 2 and _arena_on_both_sides_of_an_edge(big, r)
    whole = _staging_whole()
    monkeypatch.setenv(ENV, str(r))
    assert _staging_run() == whole


# ------------------------------------------------------------------------------------------- test_gpu_topn: the hand case
@functools.lru_cache(maxsize=None)
def _topn_case():
    arrays, U, I, keep, dup_user = t_top._hand_case()
    queries = list(range(U)) + [U + 5]
    return arrays, U, I, keep, queries, t_top.score_users(1.5, queries, *arrays[:8], keep)


def _topn_run():
    arrays, U, I, keep, queries, scored = _topn_case()
    out = []
    for n, rank_by, flags in ((10, 0, 0), (64, 1, t_top.KEEP_HELD), (5, 1, 0)):
        short = t_top.topn_rows(arrays, U, I, keep, 1.5, 66, queries, n, rank_by, flags)
        want = t_top.expected(scored, queries, n, rank_by, bool(flags), 66)
        assert short[4][2] > 66 and short[4][1] == want[1][1] > 0
        t_top.check_output(short, want, n)
        full = t_top.topn_rows(arrays, U, I, keep, 1.5, short[4][2], queries, n, rank_by, flags)
        t_top.check_output(full, t_top.expected(scored, queries, n, rank_by, bool(flags), short[4][2]), n)
        assert full[4][2] == short[4][2] > PR_CAP + 1       # a `now` only the arena launch can have met
        out += [short, full]
    return _blob(out)


@functools.lru_cache(maxsize=None)
def _topn_whole():
    return _topn_run()


@pytest.mark.parametrize("r", RANGES)
def test_topn_hand_case_in_ranges(monkeypatch, r):
    monkeypatch.delenv(ENV, raising=False)
    whole = _topn_whole()
    monkeypatch.setenv(ENV, str(r))
    assert _topn_run() == whole


# --------------------------------------------------------------------------------------- test_gpu_audience: the hand case
@functools.lru_cache(maxsize=None)
def _audience_case():
    arrays, U, I, keep = t_aud._hand_case()
    return arrays, U, I, keep, t_aud.statement(arrays, keep), [0, 5, -1, I, 7, 6, 0]


def _audience_run():
    arrays, U, I, keep, inv, queries = _audience_case()
    D = t_aud.OnDevice(arrays)
    out = []
    for rank_by in (0, 1):
        for flags in (0, t_aud.KEEP_HOLDERS):
            for n in (1, 3, 10, 64, 1024):
                for n_w in (4, 6):
                    got = t_aud.audience_rows(D, U, I, keep, t_aud.ALPHA, n_w, queries, n, rank_by, flags)
                    t_top.check_output(got, t_top.expected(inv, queries, n, rank_by, bool(flags), n_w), n)
                    assert got[4][2] == 6
                    out.append(got)
    return _blob(out)


@functools.lru_cache(maxsize=None)
def _audience_whole():
    return _audience_run()


@pytest.mark.parametrize("r", RANGES)
def test_audience_hand_case_in_ranges(monkeypatch, r):
    monkeypatch.delenv(ENV, raising=False)
    whole = _audience_whole()
    monkeypatch.setenv(ENV, str(r))
    assert _audience_run() == whole


# ============================================================================================== part 2: at the real limit
def _free():
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()


def _report(what, t0, lib_bytes):
    """wall time and peak device memory (torch's own + what the library takes for the call, by its documented sizes)"""
    import torch
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() + lib_bytes
    print("%s: %.2f s, peak device memory %.2f GB" % (what, time.perf_counter() - t0, peak / 1e9))
    assert peak < 8e9


@pytest.fixture(scope="module")
def model():
    return prs.model()


def _bits_equal(got, want, what):
    import torch
    a, b = got.view(torch.int64) if got.dtype == torch.float64 else got, want.view(torch.int64) if want.dtype == torch.float64 else want
    if not torch.equal(a, b):
        bad = (a != b).reshape(-1)
        where = bad.nonzero()[:8, 0].tolist()
        raise AssertionError("%s: %d of %d entries differ, first at %r: got %r, want %r" % (
            what, int(bad.sum()), bad.numel(), where, got.reshape(-1)[where].tolist(), want.reshape(-1)[where].tolist()))


def _planted(n, zero_item):
    """(indices, users, items) of the planted pairs of test a"""
    U, Q, I = prs.U, prs.Q, prs.Q + 2
    items = [zero_item, 1, Q, 2, zero_item, 3]
    kinds = dict(e300=lambda k: (U + 2, items[k % 6]), e129=lambda k: (U + 1, items[k % 6]), e128=lambda k: (U, items[k % 6]),
                 empty=lambda k: (k % U, Q + 1), u_lo=lambda k: (-1, items[k % 6]), u_hi=lambda k: (U + 3, items[k % 6]),
                 i_lo=lambda k: (k % U, -1), i_hi=lambda k: (k % U, I))
    at = {}
    L = prs.THREADS_LIMIT_PAIRS
    for k, kind in zip(range(L - 2, L + 2), ("e129", "e300", "e128", "e300")):       # 67 108 859 .. 67 108 862
        at[k] = kind
    R = _pair_range()
    for edge in range(R, n, R):                                                        # both sides of every range edge
        for k, kind in zip(range(edge - 4, edge + 4), ("i_lo", "u_lo", "e128", "e300", "e129", "empty", "e300", "u_hi")):
            at[k] = kind
    for k, kind in ((0, "e300"), (1, "empty"), (2, "i_hi"), (3, "e129"), (n - 3, "e128"), (n - 2, "u_hi"), (n - 1, "e300")):
        at[k] = kind
    assert all(0 <= k < n for k in at) and set(at.values()) == set(kinds) and len(range(R, n, R)) >= 1
    idx = sorted(at)
    pairs = [kinds[at[k]](j) for j, k in enumerate(idx)]
    return idx, [p[0] for p in pairs], [p[1] for p in pairs]


def test_predict_rows_beyond_2_32_threads(model):
    """test a: xmap_predict_rows over 67 112 962 pairs, t -> (t % U, 1 + (t // U) % Q) made on the device, with planted pairs
    (128 / 129 / 300 evidence entries, the empty list, users and items out of range) at the first and last index, around the
    index where the single grid reached 2^32 threads and on both sides of every range edge.  Every pair is compared."""
    import torch
    from xmap.engine import hipabi as abi
    _free()
    t0 = time.perf_counter()
    n, U, Q, I = prs.N_PAIRS_A, prs.U, prs.Q, prs.Q + 2
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ptr, pit, pra, pti, cnt, col, sim, avg = [to(a) for a in model["arrays"]]
    sign, R, w = to(model["sign"]), to(np.concatenate([model["R"], [0.0]])), to(model["wtab"])
    zero_item = int(np.nonzero(model["arrays"][7][1:Q + 1] == 0)[0][0]) + 1
    t = torch.arange(n, dtype=torch.int32, device=DEV)
    tu = t % U
    ti = 1 + torch.div(t, U, rounding_mode="floor") % Q
    del t
    idx, pu, pi = _planted(n, zero_item)
    idx = torch.tensor(idx, dtype=torch.int64, device=DEV)
    tu[idx], ti[idx] = torch.tensor(pu, dtype=torch.int32, device=DEV), torch.tensor(pi, dtype=torch.int32, device=DEV)
    plain = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    decay = torch.full((n,), -7.0, dtype=torch.float64, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    h = C.c_int32(-1)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = abi.lib.xmap_predict_rows(st, abi.i64(n), abi.vp(tu), abi.vp(ti), abi.i64(U + 3), abi.i32(I), abi.i32(1), abi.vp(cnt), abi.vp(col),
                                   abi.vp(sim), abi.vp(ptr), abi.vp(pit), abi.vp(pra), abi.vp(pti), abi.vp(avg), abi.vp(w),
                                   abi.i32(prs.N_W), abi.vp(plain), abi.vp(decay), abi.vp(status), C.byref(h))
    assert rc == 0, abi.lib.xmap_last_error()
    torch.cuda.synchronize()
    # the expected values: the closed form's tables gathered by class -- an item with a list or not, a user in range or not
    listed = (ti >= 1) & (ti <= Q)
    known = (tu >= 0) & (tu < U + 3)
    want = R[torch.where(known, tu, torch.full_like(tu, U + 3)).long()]         # R[U + 3] = 0: an unknown user's score is the average
    del known
    it = ti.clamp(0, I - 1).long()
    want.mul_(sign[it]).add_(avg[it])                                           # the score: exact (test_cpu_pair_ranges.py)
    del it
    # bound_rating: max(0, min(int(score + 0.5), 5)); + 0.0 turns the -0.0 of a truncated (-1, 0) into 0.0; then 0.0 without a list
    want.add_(0.5).trunc_().clamp_(0.0, 5.0).add_(0.0).mul_(listed)
    want_status = 1 - listed.to(torch.int32)
    del listed
    assert h.value == 301
    _bits_equal(status, want_status, "status")
    _bits_equal(plain, want, "plain")
    _bits_equal(decay, want, "decayed")
    assert sorted(set(want[idx].tolist())) == [0.0, 3.0, 4.0, 5.0] and int(want_status[idx].sum()) >= 3      # what was planted shows
    _report("predict_rows, %d pairs" % n, t0, 16 * n)          # + the library's list of overflowed pairs: 16 B per pair
    del tu, ti, plain, decay, status, want, want_status
    _free()


def _closed_matrix(model, rows_are_items):
    import torch
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    Q = prs.Q
    avg, sign = to(model["arrays"][7][1:Q + 1]), to(model["sign"][1:Q + 1])
    if rows_are_items:
        return avg[:, None] + sign[:, None] * to(model["R"])[None, :]          # [Q][U + 3]
    return avg[None, :] + sign[None, :] * to(model["R"][:prs.U])[:, None]       # [U][Q]


def _check_lists(got, S, n, offset, what):
    """lists and score bits against torch.topk of the closed form in fp64 (no ties: the order is the scores' alone)"""
    import torch
    cnt, who, plain, decay, stats = got
    val, idx = torch.topk(S, n, dim=1, largest=True, sorted=True)
    assert (cnt == n).all(), what
    assert np.array_equal(who, (idx + offset).to(torch.int32).cpu().numpy()), what
    want = val.cpu().numpy().view(np.uint64)
    assert np.array_equal(plain.view(np.uint64), want) and np.array_equal(decay.view(np.uint64), want), what
    return val, idx


def test_topn_rows_beyond_2_32_threads(model):
    """test b: xmap_topn_rows for all U one-row users, N = 10: Q * U = 7 * 10^7 candidate pairs in one scoring pass"""
    import torch
    _free()
    t0 = time.perf_counter()
    U, Q = prs.U, prs.Q
    got = t_top.topn_rows(model["arrays"], U + 3, Q + 2, 1, 0.0, prs.N_W, np.arange(U, dtype=np.int32), 10)
    assert got[4][0] == Q * U >= prs.THREADS_LIMIT_PAIRS and got[4][1] == 0 and got[4][2] == 2      # every pair scored, none dropped
    S = _closed_matrix(model, False)
    val, idx = _check_lists(got, S, 10, 1, "top-10")
    few = [0, 1, U // 2, U - 1]
    items, scores = prs.closed_topn(model, few, 10)                             # the NumPy closed form on a few rows
    assert np.array_equal(got[1][few], items) and np.array_equal(got[2][few], scores)
    _report("topn_rows, %d pairs" % got[4][0], t0, 28 * Q * U)                  # + the library's 28 B per candidate pair
    del S, val, idx
    _free()


@pytest.mark.parametrize("n_top", [10, 1000])
def test_audience_rows_beyond_2_32_threads(model, n_top):
    """test c: xmap_audience_rows for all Q listed items: every user holds the one neighbour, so Q * (U + 3) candidate pairs
    (the three long users are candidates too: their pairs go through the arena launch).  The winners are the users with the
    largest rating where the similarity is positive, with the smallest where it is negative."""
    import torch
    _free()
    t0 = time.perf_counter()
    U, Q = prs.U, prs.Q
    got = t_aud.audience_rows(model["arrays"], U + 3, Q + 2, 1, 0.0, prs.N_W, np.arange(1, Q + 1, dtype=np.int32), n_top)
    assert got[4][0] == Q * (U + 3) >= prs.THREADS_LIMIT_PAIRS and got[4][1] == 0 and got[4][2] == 301
    S = _closed_matrix(model, True)
    val, idx = _check_lists(got, S, n_top, 0, "audience %d" % n_top)
    order = np.argsort(model["R"], kind="stable")
    up = model["sign"][1:Q + 1] > 0
    assert up.any() and (~ up).any()
    assert (got[1][up] == order[::-1][:n_top].astype(np.int32)[None, :]).all() and (got[1][~ up] == order[:n_top].astype(np.int32)[None, :]).all()
    assert got[1][up][0, :3].tolist() == [U + 2, U + 1, U]
    _report("audience_rows, N = %d, %d pairs" % (n_top, got[4][0]), t0, 28 * Q * (U + 3))
    del S, val, idx
    _free()


def test_explain_sources_beyond_2_32_threads():
    """test d: xmap_explain_sources with n_ev = 16 over 4 194 309 pairs (one wave per pair and entry: 2^32 threads at 4 194 304),
    cycling over 1 000 users of the raw-profile model; ex_cnt cycles over 0 .. 16, ex_row over the user's rows and one row that
    is not the user's.  Expected: the plain-loop statement per (user, row), gathered."""
    import torch
    _free()
    t0 = time.perf_counter()
    n, n_ev, n_users, I = prs.N_PAIRS_D, 16, 1000, 8
    ptr, pit, cnt_t, raw_ptr, raw_item, flags, m = prs.raw_profile_model(n_users, 5)
    length = np.diff(ptr)
    K = int(length.max()) + 1
    # the table: row k of user u, k = length[u] is the first row behind the user's
    tu = np.repeat(np.arange(n_users), length + 1).astype(np.int32)
    tk = np.concatenate([np.arange(c + 1) for c in length])
    rows = (ptr[tu] + tk).reshape(-1, 1)
    total, pos = t_exp.sources_statement(tu, np.ones(len(tu), np.int32), rows, ptr, pit, cnt_t, raw_ptr, raw_item, flags, m, 1)
    assert (total == -1).sum() == n_users and (total == 1).any() and total.max() > 10
    tab_total, tab_pos = np.full((n_users, K), -9, np.int32), np.full((n_users, K), -9, np.int64)
    tab_total[tu, tk], tab_pos[tu, tk] = total[:, 0], pos[:, 0, 0]
    to = t_exp._to
    tab_total, tab_pos, d_len, d_ptr = to(tab_total), to(tab_pos), to(length), to(ptr)
    t = torch.arange(n, dtype=torch.int64, device=DEV)
    user = t % n_users
    ex_cnt = (t % 17).to(torch.int32)
    e = torch.arange(n_ev, dtype=torch.int64, device=DEV)[None, :]
    k = (torch.div(t, n_users, rounding_mode="floor")[:, None] + 3 * e) % (d_len[user] + 1)[:, None]
    ex_row = d_ptr[user][:, None] + k
    live = e < ex_cnt[:, None]
    want_total = torch.where(live, tab_total[user[:, None], k], torch.zeros((), dtype=torch.int32, device=DEV))
    want_pos = torch.where(live, tab_pos[user[:, None], k], torch.full((), -1, dtype=torch.int64, device=DEV))
    del k, live, t
    eng = t_exp._engine()
    zeros = np.zeros(len(pit))
    P = t_exp._view([ptr, pit, zeros, zeros.astype(np.int64)], n_users, I)
    src = (to(raw_ptr), to(raw_item), to(cnt_t), None, to(flags), to(m))
    pair_user = user.to(torch.int32)
    del user
    got_total, got_pos = eng.explain_sources(P, pair_user, ex_cnt, ex_row, 1, sources=src)
    torch.cuda.synchronize()
    assert got_total.shape == (n, n_ev) and got_pos.shape == (n, n_ev, 1)
    _bits_equal(got_total, want_total, "src_total")
    _bits_equal(got_pos[:, :, 0], want_pos, "src_pos")
    assert int((want_total == -1).sum()) > 0 and int((want_total > 1).sum()) > 0
    _report("explain_sources, %d pairs x %d entries" % (n, n_ev), t0, 0)
    del got_total, got_pos, want_total, want_pos, ex_row, ex_cnt, pair_user, eng, P
    _free()
