"""Top-N and audience under eligibility rules (xmap_rec_filter: a mask over the id space, exclusion lists per query, a score
floor) against tests/filter_statement.py -- the rules of the header restated in Python over the statements of
tests/test_gpu_topn.py and tests/test_gpu_audience.py.  Items and users are compared exactly, scores as uint64 views, the six
stats as tuples.  The rules act before scoring: stats[0] is asserted everywhere, it counts the pairs that were scored."""
import ctypes as C

import numpy as np
import pytest

from filter_statement import allowed, expected_filtered
from golden_util import CAP
from test_gpu_audience import ALPHA, KEEP_HOLDERS, OnDevice, _lists, _profiles, _window, audience, audience_rows, statement
from test_gpu_audience import _hand_case as _au_hand_case
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_tail import _few_times, generate, rec_sim, select, wtab
from test_gpu_topn import KEEP_HELD, TN_WINDOW, _random_case, check_output, recommend, score_users, topn_rows
from test_gpu_topn import _hand_case as _tn_hand_case

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


# ------------------------------------------------------------------------------------------------------- the drivers
def _words(on):
    """a bool array [n] as mask words, the bits beyond n SET (they may hold anything)"""
    n = len(on)
    pad = np.ones((n + 31) // 32 * 32, np.uint8)
    pad[:n] = on
    return np.packbits(pad, bitorder="little").view("<u4").astype(np.uint32)


def _csr(lists):
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return ptr, np.asarray([x for l in lists for x in l], np.int32)


class Filter(object):
    """what a test asks for: allow = bool array [n] or None, exclude = one list of ids per query or None, min_score or None;
    null = pass F == NULL instead of the struct"""

    def __init__(self, allow=None, exclude=None, min_score=None, null=False):
        self.allow, self.exclude, self.min_score, self.null = allow, exclude, min_score, null

    def statement(self):
        return dict(allow=self.allow, exclude=self.exclude, min_score=self.min_score)

    def on_device(self):
        """(xmap_rec_filter with device pointers or None, the tensors it points into)"""
        import torch
        from xmap.engine import hipabi as abi
        if self.null:
            return None, ()
        words = None if self.allow is None else torch.from_numpy(_words(self.allow).view(np.int32)).to("cuda:0")
        ptr = ids = None
        if self.exclude is not None:
            p, i = _csr(self.exclude)
            ptr = torch.from_numpy(p).to("cuda:0")
            ids = torch.from_numpy(np.concatenate([i, [0]]).astype(np.int32)).to("cuda:0")
        return abi.rec_filter(words, ptr, ids, self.min_score), (words, ptr, ids)

    def on_host(self):
        """(xmap_rec_filter with host pointers or None, the arrays it points into)"""
        from xmap.engine import hipabi as abi
        if self.null:
            return None, ()
        words = None if self.allow is None else _words(self.allow)
        ptr, ids = (None, None) if self.exclude is None else _csr(self.exclude)
        F = abi.RecFilter(None if words is None else words.ctypes.data, None if ptr is None else ptr.ctypes.data,
                          None if ids is None or not len(ids) else ids.ctypes.data, -INF if self.min_score is None else self.min_score)
        return F, (words, ptr, ids)


def _rows_filtered(name, D, n_users, n_items, keep, n_w, queries, n, rank_by, flags, filt, batch=None, alpha=ALPHA):
    """xmap_topn_rows_filtered / xmap_audience_rows_filtered on an OnDevice of (ptr, item, rating, time, cnt, col, sim, avg)"""
    import torch
    from xmap.engine import hipabi as abi
    dev = "cuda:0"
    ptr, pit, pra, pti, cnt, col, sim, avg = D.t
    q = torch.from_numpy(np.ascontiguousarray(queries, np.int32)).to(dev)
    Q = int(q.numel())
    w = torch.from_numpy(wtab(alpha, n_w)).to(dev)
    o_cnt = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    o_id = torch.full((Q, n), -7, dtype=torch.int32, device=dev)
    o_plain = torch.full((Q, n), -7.0, dtype=torch.float64, device=dev)
    o_decay = torch.full((Q, n), -7.0, dtype=torch.float64, device=dev)
    h = (C.c_int64 * 6)(*([-7] * 6))
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    F, alive = filt.on_device()
    head = [st, abi.i64(Q), abi.vp(q), abi.i32(n), abi.i32(rank_by), abi.i32(flags), abi.i64(n_users), abi.i32(n_items), abi.i32(keep),
            abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ptr), abi.vp(pit), abi.vp(pra), abi.vp(pti), abi.vp(avg), abi.vp(w), abi.i32(n_w),
            abi.vp(o_cnt), abi.vp(o_id), abi.vp(o_plain), abi.vp(o_decay)]
    if name == "xmap_audience_rows_filtered":
        if batch is None:
            head += [abi.i32(0), None, None]
        else:
            b_ptr, b_user = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in batch[1:]]
            head += [abi.i32(batch[0]), abi.vp(b_ptr), abi.vp(b_user)]
    rc = getattr(abi.lib, name)(*(head + [None if F is None else C.byref(F), h]))
    torch.cuda.synchronize()
    del alive
    return rc, (o_cnt.cpu().numpy(), o_id.cpu().numpy(), o_plain.cpu().numpy(), o_decay.cpu().numpy(), [int(x) for x in h])


def topn_f(D, U, I, keep, n_w, queries, n, rank_by, flags, filt, alpha=1.5):
    rc, out = _rows_filtered("xmap_topn_rows_filtered", D, U, I, keep, n_w, queries, n, rank_by, flags, filt, alpha=alpha)
    assert rc == 0
    return out


def audience_f(D, U, I, keep, n_w, queries, n, rank_by, flags, filt, batch=None):
    rc, out = _rows_filtered("xmap_audience_rows_filtered", D, U, I, keep, n_w, queries, n, rank_by, flags, filt, batch=batch)
    assert rc == 0
    return out


def check6(got, want, n):
    check_output(got[:4], want, n)
    print("stats", got[4], "statement", list(want[1]))
    assert tuple(got[4]) == tuple(want[1])


def _same_bits(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:4], b[:4]))


def _blank(out, n):
    """every count 0, the padding everywhere"""
    cnt, ids, plain, decay = out[:4]
    return not cnt.any() and (ids == -1).all() and not plain.any() and not decay.any() and ids.shape[1] == n


# ------------------------------------------------------------------------------------------------- 1. the empty filter
def test_the_empty_filter_is_the_unfiltered_call():
    arrays, U, I, keep, _ = _tn_hand_case()
    D = OnDevice(arrays)
    queries = list(range(U)) + [U + 5]
    for n, rank_by, flags in ((10, 0, 0), (64, 1, KEEP_HELD)):
        plain = topn_rows(arrays, U, I, keep, 1.5, 66, queries, n, rank_by, flags)
        assert plain[4][0] > 0 and plain[4][1] > 0
        for filt in (Filter(null=True), Filter()):
            got = topn_f(D, U, I, keep, 66, queries, n, rank_by, flags, filt)
            assert _same_bits(got, plain) and got[4][:4] == plain[4] and got[4][4:] == [0, 0]
    arrays, U, I, keep = _au_hand_case()
    D = OnDevice(arrays)
    queries = [0, 5, -1, I, 7, 6, 0]
    for n, rank_by, flags in ((3, 0, 0), (64, 1, KEEP_HOLDERS), (1024, 0, 0)):
        plain = audience_rows(D, U, I, keep, ALPHA, 6, queries, n, rank_by, flags)
        assert plain[4][0] > 0 and plain[4][1] > 0
        for filt in (Filter(null=True), Filter()):
            got = audience_f(D, U, I, keep, 6, queries, n, rank_by, flags, filt)
            assert _same_bits(got, plain) and got[4][:4] == plain[4] and got[4][4:] == [0, 0]
    # no queries: six zeros
    assert audience_f(D, U, I, keep, 6, [], 5, 0, 0, Filter(allow=np.ones(U, bool)))[4] == [0] * 6


# ----------------------------------------------------------------------------------------- 2. top-N across the window
def _exclusions(scored, key, n_ids, edge, held, keep_flag):
    """an exclusion list for one query: candidates from both sides of `edge`, one of them three times, ids outside the id
    space, a held id and a non-candidate"""
    cand = [c[0] for c in scored.get(int(key), []) if keep_flag or not c[4]]
    edges = (0, edge - 1, edge, n_ids - 1)              # (the tests watch these four through the mask)
    low, high = [i for i in cand if i < edge and i not in edges], [i for i in cand if i >= edge and i not in edges]
    out = low[:2] + high[:2]
    out = out + out[:1] * 2 + [-1, n_ids, n_ids + 5]
    if held is not None:
        out.append(int(held))
    free = next(i for i in range(edge - 3, edge + 40) if i not in set(c[0] for c in scored.get(int(key), [])))
    return out + [free]


def test_topn_across_the_window():
    U, I, keep = 20, TN_WINDOW + 100, 2
    assert I & 31 == 4
    rng = np.random.default_rng(23)                     # the builder of test_an_item_space_just_above_the_window
    listed = np.unique(np.concatenate([[0, TN_WINDOW - 1, TN_WINDOW, I - 1], rng.integers(0, I, 100), rng.integers(TN_WINDOW, I, 96)]))
    pool = rng.integers(0, I, 30)
    arrays = _random_case(23, U, I, keep, listed, lambda u: 8)
    arrays[5][listed] = pool[rng.integers(0, 30, (len(listed), keep))]
    arrays[4][listed] = keep
    arrays[1][:] = pool[rng.integers(0, 30, len(arrays[1]))]
    arrays[1][arrays[0][4]] = TN_WINDOW
    arrays[1][arrays[0][5]] = TN_WINDOW - 1
    ptr, pit = arrays[0], arrays[1]
    queries = list(range(U)) + [4, 7]                   # users 4 and 7 twice, with another list each
    scored = score_users(1.5, queries, *arrays[:8], keep)
    mask = np.ones(I, bool)
    mask[[0, TN_WINDOW - 1]] = False
    mask[listed[5::3]] = False
    mask[[TN_WINDOW, I - 1]] = True
    D = OnDevice(arrays)
    for flags in (0, KEEP_HELD):
        held = lambda u: pit[ptr[u]]
        exclude = [_exclusions(scored, u, I, TN_WINDOW, held(u), bool(flags)) for u in queries[:U]] + [[], [TN_WINDOW, I - 1]]
        filt = Filter(allow=mask, exclude=exclude)
        want = expected_filtered(scored, queries, 64, 0, bool(flags), 66, I, **filt.statement())
        got = topn_f(D, U, I, keep, 66, queries, 64, 0, flags, filt)
        check6(got, want, 64)
        plain = topn_rows(arrays, U, I, keep, 1.5, 66, queries, 64, 0, flags)
        assert got[4][5] == plain[4][0] - got[4][0] > 0 and got[4][0] > 0
        listed_now = {c[0] for l in want[0] for c in l}
        assert {TN_WINDOW, I - 1} <= listed_now and not {0, TN_WINDOW - 1} & listed_now
        assert min(listed_now) < TN_WINDOW <= max(listed_now)                  # both windows are left in
        assert got[1][4].tolist() != got[1][U].tolist() and got[1][7].tolist() != got[1][U + 1].tolist()    # lists go by query
        only = topn_f(D, U, I, keep, 66, queries, 64, 0, flags, Filter(exclude=exclude))   # the lists alone
        check6(only, expected_filtered(scored, queries, 64, 0, bool(flags), 66, I, exclude=exclude), 64)
        assert 0 < only[4][5] < got[4][5]


# ----------------------------------------------------------------------------------------------- 3. degenerate masks
def test_masks_of_all_ones_and_all_zeros():
    arrays, U, I, keep, _ = _tn_hand_case()
    D = OnDevice(arrays)
    queries = list(range(U)) + [U + 5]
    plain = topn_rows(arrays, U, I, keep, 1.5, 66, queries, 10, 1, 0)
    ones = topn_f(D, U, I, keep, 66, queries, 10, 1, 0, Filter(allow=np.ones(I, bool)))
    assert _same_bits(ones, plain) and ones[4] == plain[4] + [0, 0]
    zeros = topn_f(D, U, I, keep, 66, queries, 10, 1, 0, Filter(allow=np.zeros(I, bool)))
    assert _blank(zeros, 10) and zeros[4] == [0, 0, 0, 0, 0, plain[4][0]] and plain[4][0] > 0
    arrays, U, I, keep = _au_hand_case()
    D = OnDevice(arrays)
    queries = [0, 5, -1, I, 7, 6, 0]
    for n in (5, 1024):
        plain = audience_rows(D, U, I, keep, ALPHA, 6, queries, n, 0, KEEP_HOLDERS)
        ones = audience_f(D, U, I, keep, 6, queries, n, 0, KEEP_HOLDERS, Filter(allow=np.ones(U, bool)))
        assert _same_bits(ones, plain) and ones[4] == plain[4] + [0, 0]
        zeros = audience_f(D, U, I, keep, 6, queries, n, 0, KEEP_HOLDERS, Filter(allow=np.zeros(U, bool)))
        assert _blank(zeros, n) and zeros[4] == [0, 0, 0, 0, 0, plain[4][0]] and plain[4][0] > 0


def test_many_queries_per_block():
    """more queries than the candidate passes have blocks (2 048 and 512): a block then serves query after query on one bitmap,
    which the rules must leave as clean as the unfiltered pass does"""
    U, I, keep = 50, 400, 5
    arrays = _random_case(24, U, I, keep, np.arange(0, I, 3), lambda u: 2 + u % 9)
    D = OnDevice(arrays)
    rng = np.random.default_rng(42)
    queries = rng.integers(-2, U + 2, 5000).tolist()
    scored = score_users(1.5, queries, *arrays[:8], keep)
    mask = rng.integers(0, 2, I) > 0
    exclude = [rng.integers(-3, I + 3, int(rng.integers(0, 25))).tolist() for _ in queries]
    for flags in (0, KEEP_HELD):
        filt = Filter(allow=mask, exclude=exclude, min_score=2.5)
        want = expected_filtered(scored, queries, 3, 1, bool(flags), 66, I, **filt.statement())
        check6(topn_f(D, U, I, keep, 66, queries, 3, 1, flags, filt), want, 3)
        assert want[1][0] > 0 and want[1][4] > 0 and want[1][5] > 0
    inv = statement(arrays, keep)
    queries = rng.integers(-2, I + 2, 1500).tolist()
    mask = rng.integers(0, 2, U) > 0
    exclude = [rng.integers(-3, U + 3, int(rng.integers(0, 25))).tolist() for _ in queries]
    for flags in (0, KEEP_HOLDERS):
        filt = Filter(allow=mask, exclude=exclude, min_score=2.5)
        want = expected_filtered(inv, queries, 7, 0, bool(flags), 66, U, **filt.statement())
        check6(audience_f(D, U, I, keep, 66, queries, 7, 0, flags, filt), want, 7)
        assert want[1][0] > 0 and want[1][4] > 0 and want[1][5] > 0


# ---------------------------------------------------------------------------------------------------------- 4. floor
def test_the_floor_on_hand_built_scores():
    arrays, U, I, keep, dup_user = _tn_hand_case()
    D = OnDevice(arrays)
    queries = list(range(U)) + [U + 5, 3]
    scored = score_users(1.5, queries, *arrays[:8], keep)

    def run(n, rank_by, flags, floor, n_w=66):
        want = expected_filtered(scored, queries, n, rank_by, bool(flags), n_w, I, min_score=floor)
        got = topn_f(D, U, I, keep, n_w, queries, n, rank_by, flags, Filter(min_score=floor))
        check6(got, want, n)
        return want

    ok = sorted(c[1] for l in scored.values() for c in l if c[1] is not None and not c[4] and c[3] <= 66)
    at = ok[len(ok) // 2]                               # a floor equal to a candidate's score: that candidate is kept
    want = run(64, 0, 0, at)
    assert any(c[1] == at for l in want[0] for c in l) and 0 < want[1][4] < want[1][0]
    assert want[1][1] > 0                               # status 2 (the long evidence at n_w = 66): in [1], never in [4]
    assert any(0 < len(l) < 64 for l in want[0])        # fewer survivors than n_top: padding (check_output)
    lo, hi = max(x for x in ok if x < at), at           # a floor between two scores
    between = run(64, 0, 0, (lo + hi) / 2.0)
    assert between[1][4] == want[1][4] and [len(l) for l in between[0]] == [len(l) for l in want[0]]
    below = run(64, 0, 0, lo)
    assert below[1][4] < want[1][4]
    # plain and decayed on different sides of one floor
    split = [c for l in scored.values() for c in l if c[1] is not None and not c[4] and c[3] <= 66 and abs(c[1] - c[2]) > 1e-3]
    assert split
    c = split[len(split) // 2]
    floor = (c[1] + c[2]) / 2.0
    by_plain, by_decay = run(64, 0, 0, floor), run(64, 1, 0, floor)
    in_plain = {(q, x[0]) for q, l in enumerate(by_plain[0]) for x in l}
    in_decay = {(q, x[0]) for q, l in enumerate(by_decay[0]) for x in l}
    assert in_plain - in_decay and in_decay - in_plain
    # +inf: nothing is kept; [4] = scored - dropped, with and without the status-2 candidates of the short table
    for n_w in (66, 400):
        none = expected_filtered(scored, queries, 10, 1, True, n_w, I, min_score=INF)
        got = topn_f(D, U, I, keep, n_w, queries, 10, 1, KEEP_HELD, Filter(min_score=INF))
        check6(got, none, 10)
        assert _blank(got, 10) and got[4][4] == got[4][0] - got[4][1] > 0 and (got[4][1] > 0) == (n_w == 66)
    # more survivors than n_top, and a tie across the cut: the twins 10 and 20 score the same, the floor sits AT their score
    done = 0
    for q, u in enumerate(queries[:U]):
        l = expected_filtered(scored, [u], 64, 0, True, 400, I)[0][0]
        pos = {x[0]: k for k, x in enumerate(l)}
        if 10 in pos and 20 in pos and pos[20] == pos[10] + 1 and len(l) > pos[20] + 1:
            n, floor = pos[10] + 1, l[pos[10]][1]
            want = expected_filtered(scored, [u, u], n, 0, True, 400, I, min_score=floor)
            got = topn_f(D, U, I, keep, 400, [u, u], n, 0, KEEP_HELD, Filter(min_score=floor))
            check6(got, want, n)
            assert got[1][0, n - 1] == 10 and 20 not in got[1][0] and want[1][4] > 0
            more = topn_f(D, U, I, keep, 400, [u, u], n + 1, 0, KEEP_HELD, Filter(min_score=floor))
            assert more[1][0, n] == 20 and more[2][0, n] == more[2][0, n - 1]
            done += 1
            if done == 3:
                break
    assert done > 0


# --------------------------------------------------------------------------------------- 5. audience across the window
def test_audience_across_the_window():
    W = _window()
    U, I, keep = W + 70, 30, 3
    assert U & 31
    rng = np.random.default_rng(31)                     # the builder of test_a_user_space_just_above_the_window
    users = np.unique(np.concatenate([[0, W - 1, W, W + 69], rng.integers(0, U, 20), rng.integers(W, U, 12)]))
    rows = {int(u): [(int(i), float(rng.integers(2, 21)) / 4.0, int(rng.integers(0, 4))) for i in rng.choice(np.arange(8, I), 5, replace=False)]
            for u in users}
    lists = {i: (keep, rng.choice(np.arange(8, I), keep, replace=False).tolist(), np.round(rng.normal(size=keep), 2).tolist()) for i in range(8)}
    for u, i in ((W - 1, 2), (W, 2), (W + 69, 3)):
        rows[u] += [(i, 3.0, 0), (lists[i][1][0], 2.5, 2)]
    avg = np.round(rng.uniform(1.0, 5.0, I), 1)
    arrays = list(_profiles(U, rows)) + list(_lists(I, keep, lists)) + [avg]
    inv = statement(arrays, keep)
    D = OnDevice(arrays)
    queries = list(range(8)) + [2, 3]
    mask = np.ones(U, bool)
    mask[[0, W - 1]] = False
    mask[users[3::4]] = False
    mask[[W, W + 69]] = True
    holder = {2: W - 1, 3: W + 69}
    for n, rank_by, flags in ((64, 0, 0), (64, 1, KEEP_HOLDERS), (5, 0, KEEP_HOLDERS), (1024, 1, 0)):
        exclude = [_exclusions(inv, i, U, W, holder.get(i), bool(flags)) for i in queries[:8]] + [[W, W + 5], []]
        filt = Filter(allow=mask, exclude=exclude)
        want = expected_filtered(inv, queries, n, rank_by, bool(flags), 66, U, **filt.statement())
        got = audience_f(D, U, I, keep, 66, queries, n, rank_by, flags, filt)
        check6(got, want, n)
        plain = audience_rows(D, U, I, keep, ALPHA, 66, queries, n, rank_by, flags)
        assert got[4][5] == plain[4][0] - got[4][0] > 0 and got[4][0] > 0
        if n >= 64:
            seen = {c[0] for l in want[0] for c in l}
            assert {W + 69} <= seen and not {0, W - 1} & seen and min(seen) < W <= max(seen)
            assert got[1][2].tolist() != got[1][8].tolist()                # item 2 twice, another list
        only = audience_f(D, U, I, keep, 66, queries, n, rank_by, flags, Filter(exclude=exclude))
        check6(only, expected_filtered(inv, queries, n, rank_by, bool(flags), 66, U, exclude=exclude), n)
        assert 0 < only[4][5] < got[4][5]


@pytest.mark.parametrize("n_top", [1, 256, 1024])
def test_audience_floor_at_a_tie_on_designed_score_orders(n_top):
    """the design of test_selection_edges_on_designed_score_orders -- query item q = (length, order) has the single neighbour
    Q + q, held by the users [0, length) -- with every score given to TWO users, so that a floor at a score is a floor at a tie;
    n_top = 256 / 1024 are the two sizes of the selection kernel, 1 its smallest list"""
    lengths = [0, 1, n_top - 1, n_top, n_top + 1, 3000]
    cases = [(L, order) for L in lengths for order in ("rising", "falling", "random")]
    Q, U, keep = len(cases), 3000, 1
    I = 2 * Q + 1
    rng = np.random.default_rng(33)
    rows = {u: [] for u in range(U)}
    for q, (L, order) in enumerate(cases):
        score = ({"rising": np.arange(L), "falling": np.arange(L)[::-1], "random": rng.permutation(L)}[order] // 2) / 8.0
        for u in range(L):
            rows[u].append((Q + q, float(score[u]), u % 2))
    lists = {q: (1, [Q + q], [1.0]) for q in range(Q)}
    arrays = list(_profiles(U, rows)) + list(_lists(I, keep, lists)) + [np.zeros(I)]
    inv = statement(arrays, keep)
    assert [len(inv.get(q, [])) for q in range(Q)] == [L for L, _ in cases]
    queries = list(range(Q)) + [Q - 1, 0]
    D = OnDevice(arrays)
    mask = np.ones(U, bool)
    mask[np.arange(7, U, 13)] = False
    for rank_by in (0, 1):
        for floor in (0.0, (n_top // 4) / 8.0, (3000 - n_top) // 2 / 8.0, 1499 / 8.0, 1500 / 8.0):
            want = expected_filtered(inv, queries, n_top, rank_by, False, 66, U, min_score=floor)
            check6(audience_f(D, U, I, keep, 66, queries, n_top, rank_by, 0, Filter(min_score=floor)), want, n_top)
        tied = [c for c in inv[Q - 1] if c[1] == floor]
        assert floor == 187.5 and not tied and want[1][4] == want[1][0] > 0            # above every score: all below the floor
        floor = 1499 / 8.0                                                           # the top score, held by two users
        want = expected_filtered(inv, queries, n_top, rank_by, False, 66, U, allow=mask, min_score=floor)
        got = audience_f(D, U, I, keep, 66, queries, n_top, rank_by, 0, Filter(allow=mask, min_score=floor))
        check6(got, want, n_top)
        rising = cases.index((3000, "rising"))
        assert got[1][rising, :min(n_top, 2)].tolist() == [2998, 2999][:min(n_top, 2)] and got[0][rising] == min(n_top, 2)
        assert want[1][5] > 0


# ------------------------------------------------------------------------------------------------------ 6. item fold-in
def test_item_foldin_audience_with_a_mask_and_an_excluded_rater():
    arrays, U, I, keep = _au_hand_case()
    cnt, col, sim, avg = arrays[4:8]
    # two batch items behind the I resident ones: I lists neighbours 1 and 2, I + 1 has no list; their raters are their holders
    x_cnt = np.concatenate([cnt, [2, 0]]).astype(np.int32)
    x_col = np.concatenate([col, [[1, 2, -1, -1], [-1] * 4]]).astype(np.int32)
    x_sim = np.concatenate([sim, [[1.0, 0.5, 0.0, 0.0], [0.0] * 4]])
    x_avg = np.concatenate([avg, [1.0, 2.0]])
    raters = {I: [0, 3, 20], I + 1: [5]}
    batch = (I, np.asarray([0, 3, 4], np.int64), np.asarray([0, 3, 20, 5], np.int32))
    ext = arrays[:4] + [x_cnt, x_col, x_sim, x_avg]
    inv = statement(ext, keep)
    inv = {i: [(c[0], c[1], c[2], c[3], c[0] in raters[i]) if i >= I else c for c in l] for i, l in inv.items()}   # no profile holds a batch item
    assert {0, 3, 20} <= {c[0] for c in inv[I]} and len(inv[I]) > 6
    D = OnDevice(ext)
    queries = [I, 0, I, I + 1, I + 2, 5]
    mask = np.ones(U, bool)
    mask[[2, 21]] = False
    for n, rank_by, flags in ((5, 0, KEEP_HOLDERS), (64, 1, KEEP_HOLDERS), (64, 0, 0), (1024, 0, 0)):
        exclude = [[20], [20, 22], [], [], [0], [15, 15]]       # rater 20 for the first query of I only
        filt = Filter(allow=mask, exclude=exclude, min_score=-1.5)
        want = expected_filtered(inv, queries, n, rank_by, bool(flags), 6, U, **filt.statement())
        got = audience_f(D, U, I + 2, keep, 6, queries, n, rank_by, flags, filt, batch=batch)
        check6(got, want, n)
        none = audience_f(D, U, I + 2, keep, 6, queries, n, rank_by, flags, Filter(), batch=batch)
        assert got[4][5] == none[4][0] - got[4][0] > 0
        first, second = set(got[1][0][:got[0][0]].tolist()), set(got[1][2][:got[0][2]].tolist())
        if n >= 64:
            assert 20 not in first and (20 in second) == bool(flags) and (0 in second) == bool(flags) and 2 not in second
        # F == NULL with a batch is xmap_itemfold_audience_rows
        null = audience_f(D, U, I + 2, keep, 6, queries, n, rank_by, flags, Filter(null=True), batch=batch)
        assert _same_bits(null, none) and null[4] == none[4]
        check6(none, expected_filtered(inv, queries, n, rank_by, bool(flags), 6, U), n)


# ------------------------------------------------------------------------------------------------------- 7. one pair set
def test_the_filtered_pair_set_is_one():
    """top-N under an item mask M with (u, i) excluded and audience over the items of M with (i, u) excluded score the same
    pairs with the same bits (the case of test_the_pair_set_is_the_one_of_topn)"""
    U, I, keep = 300, 400, 3
    arrays = _random_case(34, U, I, keep, np.arange(0, I, 2), lambda u: 2 + u % 7)
    D = OnDevice(arrays)
    rng = np.random.default_rng(37)
    M = rng.integers(0, 3, I) > 0
    plain = topn_rows(arrays, U, I, keep, ALPHA, 66, list(range(U)), 64, 0, 0)
    pairs = [(u, int(plain[1][u, k])) for u in range(U) for k in range(plain[0][u])]
    gone = [pairs[k] for k in rng.choice(len(pairs), 200, replace=False)]
    by_user = [[i for u, i in gone if u == q] for q in range(U)]
    items = np.nonzero(M)[0].tolist()
    by_item = [[u for u, i in gone if i == q] for q in items]
    for mine, theirs in ((0, 0), (KEEP_HOLDERS, KEEP_HELD)):
        t = topn_f(D, U, I, keep, 66, list(range(U)), 64, 0, theirs, Filter(allow=M, exclude=by_user), alpha=ALPHA)
        a = audience_f(D, U, I, keep, 66, items, 1024, 0, mine, Filter(exclude=by_item))
        assert 0 < a[4][3] < 1024 and 0 < t[4][3] < 64 and a[4][1] == t[4][1]            # no list was cut; the same pairs dropped
        from_items = {(int(a[1][q, k]), i): (a[2][q, k].tobytes(), a[3][q, k].tobytes()) for q, i in enumerate(items) for k in range(a[0][q])}
        from_users = {(u, int(t[1][u, k])): (t[2][u, k].tobytes(), t[3][u, k].tobytes()) for u in range(U) for k in range(t[0][u])}
        assert a[4][0] == t[4][0] > 500 and len(from_items) == a[4][0] - a[4][1]
        assert from_items == from_users
        assert not set(from_users) & {(u, i) for u, i in gone} and all(M[i] for _, i in from_users)
        assert t[4][5] > a[4][5] > 0                    # the mask removed pairs from top-N that audience never asked for


# --------------------------------------------------------------------------------------------------------- 8. coarse ABI
def _coarse(ctx, name, source, queries, n, rank_by, flags, filt, n_w=66, alpha=ALPHA):
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(alpha, n_w)
    cnt, ids = np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32)
    plain, decay, stats = np.full((Q, n), -7.0), np.full((Q, n), -7.0), np.full(6, -7, np.int64)
    F, alive = filt.on_host()
    rc = getattr(ctx.lib, name)(ctx.h, source, Q, _p(q, C.c_int32), n, rank_by, flags, _p(w, C.c_double), n_w, _p(cnt, C.c_int32),
                                _p(ids, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), None if F is None else C.byref(F),
                                _p(stats, C.c_int64))
    del alive
    return rc, (cnt, ids, plain, decay, stats.tolist())


def _host_filtered(plain, n, rank_by, filt, n_ids):
    """the unfiltered lists (which hold EVERY kept candidate: asserted by the caller) under the rules, cut at n"""
    cnt, ids, p, d = plain[:4]
    ok_id = allowed(filt.allow, n_ids)
    floor = -INF if filt.min_score is None else filt.min_score
    lists = []
    for q in range(len(cnt)):
        ex = set() if filt.exclude is None else set(filt.exclude[q])
        l = [(int(ids[q, k]), p[q, k], d[q, k]) for k in range(cnt[q])]
        lists.append([c for c in l if c[0] not in ex and ok_id[c[0]] and c[1 + rank_by] >= floor][:n])
    return lists


def _short_lists(ctx, twin, queries, n, at_least):
    """the queries whose unfiltered list is shorter than n -- it then holds every candidate that was kept -- the first one again
    at the end; the inputs are such that there are `at_least` of them with a list (asserted: the cross-check does not go quiet)"""
    queries = np.ascontiguousarray(queries, np.int32)
    cnt = _twin(ctx, twin, queries, n)[0]
    assert ((cnt > 0) & (cnt < n)).sum() >= at_least, (twin, cnt.tolist())
    qs = queries[cnt < n][:400]
    return np.ascontiguousarray(np.concatenate([qs, qs[:1]]), np.int32)


def _check_lists(got, lists, n):
    check_output(got[:4], (lists, None), n)


def test_the_coarse_entries_over_the_three_sources():
    from test_gpu_foldin import foldin, foldin_download
    from test_gpu_item_foldin import item_foldin, item_foldin_download
    from xmap.engine import synth
    seed, users, src, tgt, overlap = 5, 1500, 300, 300, 0.4          # the smallest case of test_recommend_through_the_coarse_abi
    r = _few_times(synth.make_two_domain(seed, users, src, tgt, overlap=overlap))
    I, U, keep = r.n_items, users, 1
    rng = np.random.default_rng(seed)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        cnt, col, sim, _ = select(ctx, I, keep)
        arrays = [T["ptr"], T["item"], T["rating"], T["time"], cnt, col, sim, T["avg"]]
        # a fold-in batch of users and one of items, for the sources 1 and 2
        B = 120
        lens = rng.integers(0, 30, B)
        f_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        f_item = rng.integers(0, I, f_ptr[-1]).astype(np.int32)
        f_counts = foldin(ctx, f_ptr, f_item, (rng.integers(2, 21, len(f_item)) / 4.0).astype(np.float32),
                          1000 + rng.integers(0, 7, len(f_item)).astype(np.int64))
        NB = 6
        b_lens = rng.integers(3, 25, NB)
        b_ptr = np.concatenate([[0], np.cumsum(b_lens)]).astype(np.int64)
        b_user = np.concatenate([rng.choice(U, k, replace=False) for k in b_lens]).astype(np.int32)
        b_counts = item_foldin(ctx, (b_ptr, b_user, rng.integers(2, 21, len(b_user)) / 4.0))
        # the arrays the statement reads for each source: 1 = the batch's AlterEgo profiles with the resident tables, 2 = the resident
        # profiles with the extended tables of I + NB items (no profile holds a batch item: its raters are its holders)
        folded = list(foldin_download(ctx, B, f_counts[0])) + arrays[4:]
        b_rows, (n_cnt, n_col, n_sim, _) = item_foldin_download(ctx, NB, b_counts[0], keep)
        extended = arrays[:4] + [np.concatenate([cnt, n_cnt]), np.concatenate([col, n_col]), np.concatenate([sim, n_sim]),
                                 np.concatenate([T["avg"], b_rows[5]])]
        raters = [set(b_user[b_ptr[q]:b_ptr[q + 1]].tolist()) for q in range(NB)]
        by_source = {0: arrays, 1: folded, 2: extended}
        # ---- top-N
        qu = np.arange(-1, U + 1)
        for source, twin, n_ids, qs in ((0, "xmap_ctx_recommend", I, qu), (1, "xmap_ctx_foldin_recommend", I, np.arange(-1, B + 1)),
                                        (2, "xmap_ctx_item_foldin_recommend", I + NB, qu)):
            qs = _short_lists(ctx, twin, qs, 64, 60)
            scored = score_users(ALPHA, qs, *by_source[source], keep)
            plain = _twin(ctx, twin, qs, 64)
            assert 0 < plain[4][3] <= 64 and plain[4][1] == 0, "the cross-check needs every candidate in the unfiltered list"
            mask = rng.integers(0, 4, n_ids) > 0
            exclude = [plain[1][q, :plain[0][q]][::3].tolist() + [-1, n_ids, int(qs[q]) % n_ids] for q in range(len(qs))]
            exclude[-1] = []
            floor = float(np.median(plain[2][plain[1] >= 0]))
            for n, rank_by, filt in ((64, 0, Filter(allow=mask, exclude=exclude, min_score=floor)), (5, 1, Filter(allow=mask, exclude=exclude)),
                                     (64, 1, Filter(min_score=floor)), (64, 0, Filter()), (10, 0, Filter(null=True))):
                rc, got = _coarse(ctx, "xmap_ctx_recommend_filtered", source, qs, n, rank_by, 0, filt)
                assert rc == 0
                base = plain if rank_by == 0 else _twin(ctx, twin, qs, 64, rank_by)
                _check_lists(got, _host_filtered(base, n, rank_by, filt, n_ids), n)
                assert got[4][0] + got[4][5] == plain[4][0] and got[4][1] == 0
                check6(got, expected_filtered(scored, qs, n, rank_by, False, 66, n_ids, **filt.statement()), n)
            assert got[4][4:] == [0, 0] and got[4][:4] == _twin(ctx, twin, qs, 10)[4]
        # ---- audience
        qi = np.concatenate([np.arange(r.n_src_items, r.n_src_items + 60), [-1, I, r.n_src_items]]).astype(np.int32)
        inv2 = statement(extended, keep)             # source 2 asks by batch index q for item I + q
        inv2 = {q: [(c[0], c[1], c[2], c[3], c[0] in raters[q]) for c in inv2.get(I + q, [])] for q in range(NB)}
        invs = {0: statement(arrays, keep), 1: statement(folded, keep), 2: inv2}
        for source, twin, n_ids, qs in ((0, "xmap_ctx_audience", U, qi), (1, "xmap_ctx_foldin_audience", B, qi),
                                        (2, "xmap_ctx_item_foldin_audience", U, np.arange(-1, NB + 1))):
            qs = _short_lists(ctx, twin, qs, 1024, 6)
            plain = _twin(ctx, twin, qs, 1024)
            assert 0 < plain[4][3] <= 1024 and plain[4][1] == 0, "the cross-check needs every candidate in the unfiltered list"
            mask = rng.integers(0, 4, n_ids) > 0
            exclude = [plain[1][q, :plain[0][q]][::3].tolist() + [-1, n_ids] for q in range(len(qs))]
            exclude[-1] = []
            floor = float(np.median(plain[2][plain[1] >= 0]))
            for n, rank_by, filt in ((1024, 0, Filter(allow=mask, exclude=exclude, min_score=floor)), (5, 1, Filter(allow=mask, exclude=exclude)),
                                     (300, 1, Filter(min_score=floor)), (10, 0, Filter(null=True))):
                rc, got = _coarse(ctx, "xmap_ctx_audience_filtered", source, qs, n, rank_by, 0, filt)
                assert rc == 0
                base = plain if rank_by == 0 else _twin(ctx, twin, qs, 1024, rank_by)
                _check_lists(got, _host_filtered(base, n, rank_by, filt, n_ids), n)
                assert got[4][0] + got[4][5] == plain[4][0] and got[4][1] == 0
                check6(got, expected_filtered(invs[source], qs, n, rank_by, False, 66, n_ids, **filt.statement()), n)
            assert got[4][4:] == [0, 0] and got[4][:4] == _twin(ctx, twin, qs, 10)[4]
    finally:
        ctx.close()


def _twin(ctx, name, queries, n, rank_by=0, flags=0):
    """an unfiltered coarse call (the signatures of xmap_ctx_recommend and xmap_ctx_audience are one)"""
    q = np.ascontiguousarray(queries, np.int32)
    Q, w = len(q), wtab(ALPHA, 66)
    cnt, ids = np.full(Q, -7, np.int32), np.full((Q, n), -7, np.int32)
    plain, decay, stats = np.full((Q, n), -7.0), np.full((Q, n), -7.0), np.zeros(4, np.int64)
    ctx.call(name, Q, _p(q, C.c_int32), n, rank_by, flags, _p(w, C.c_double), 66, _p(cnt, C.c_int32), _p(ids, C.c_int32),
             _p(plain, C.c_double), _p(decay, C.c_double), _p(stats, C.c_int64))
    return cnt, ids, plain, decay, stats.tolist()


# ------------------------------------------------------------------------------------------------------------ 9. errors
def test_bad_filters_are_argument_errors_and_start_nothing():
    from xmap.engine import hipabi as abi, synth
    r = _few_times(synth.make_two_domain(3, 400, 100, 100, overlap=0.4))
    I, U, keep = r.n_items, 400, 5
    Q = 40
    asked = dict(xmap_ctx_recommend_filtered=np.random.default_rng(2).integers(0, U, Q).astype(np.int32),
                 xmap_ctx_audience_filtered=np.arange(I - Q, I, dtype=np.int32))
    ctx = Ctx()
    try:
        generate(ctx, r)
        ctx.call("xmap_ctx_rec_sim", CAP, None)
        ctx.call("xmap_ctx_rec_select", keep)
        good = [[1, 2]] * Q
        bad_first = Filter(exclude=good)
        decreasing = Filter(exclude=good)
        for name, n_ids in (("xmap_ctx_recommend_filtered", I), ("xmap_ctx_audience_filtered", U)):
            queries = asked[name]
            rc, want = _coarse(ctx, name, 0, queries, 10, 0, 0, Filter(exclude=good, min_score=1.0))
            assert rc == 0 and want[4][0] > 0

            def refused(source, filt, patch=None):
                F, alive = filt.on_host()
                if patch:
                    patch(F, alive)
                q, w = queries, wtab(ALPHA, 66)
                cnt, ids = np.full(Q, -7, np.int32), np.full((Q, 10), -7, np.int32)
                plain, decay, stats = np.full((Q, 10), -7.0), np.full((Q, 10), -7.0), np.full(6, -7, np.int64)
                rc = getattr(ctx.lib, name)(ctx.h, source, Q, _p(q, C.c_int32), 10, 0, 0, _p(w, C.c_double), 66, _p(cnt, C.c_int32),
                                            _p(ids, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), C.byref(F), _p(stats, C.c_int64))
                # refused before any device work: the outputs are as they were
                assert rc == abi.ERR_ARG and (cnt == -7).all() and (ids == -7).all() and (plain == -7.0).all() and (stats == -7).all()
                again = _coarse(ctx, name, 0, queries, 10, 0, 0, Filter(exclude=good, min_score=1.0))
                assert again[0] == 0 and _same_bits(again[1], want) and again[1][4] == want[4]      # the context answers the next call

            refused(0, Filter(min_score=float("nan")))

            def first(F, alive):
                alive[1][0] = 1
            refused(0, bad_first, first)

            def down(F, alive):
                alive[1][0] = 0
                alive[1][Q // 2] = alive[1][Q // 2 - 1] - 1
            refused(0, decreasing, down)

            def no_ids(F, alive):
                F.ex_id = None
            refused(0, Filter(exclude=good), no_ids)
            refused(3, Filter())
            refused(-1, Filter())
            refused(1, Filter())                        # no fold-in batch on this context
            refused(2, Filter())                        # no item fold-in batch either
    finally:
        ctx.close()
    # the fine-grained calls check ex_ptr on the device before any candidate work: the outputs stay as they were
    arrays, U, I, keep = _au_hand_case()
    D = OnDevice(arrays)
    qs = [0, 5, 0]

    class Broken(Filter):
        def __init__(self, ptr, ids=True, **kw):
            Filter.__init__(self, **kw)
            self.ptr, self.ids = ptr, ids

        def on_device(self):
            import torch
            p = torch.tensor(self.ptr, dtype=torch.int64, device="cuda:0")
            i = torch.zeros(8, dtype=torch.int32, device="cuda:0")
            return abi.rec_filter(None, p, i if self.ids else None, self.min_score), (p, i)

    for name, n_users in (("xmap_topn_rows_filtered", U), ("xmap_audience_rows_filtered", U)):
        for filt in (Broken([1, 2, 3, 4]), Broken([0, 3, 2, 4]), Broken([0, 1, 1, 0]), Broken([0, 0, 0, 2], ids=False),
                     Broken([0, 0, 0, 0], min_score=float("nan")), Filter(min_score=float("nan"))):
            rc, out = _rows_filtered(name, D, U, I, keep, 6, qs, 4, 0, 0, filt)
            assert rc == abi.ERR_ARG and (out[0] == -7).all() and (out[1] == -7).all() and (out[2] == -7.0).all()
        rc, out = _rows_filtered(name, D, U, I, keep, 6, qs, 4, 0, 0, Broken([0, 0, 0, 0], ids=False))      # no ids listed: fine
        assert rc == 0 and out[4][5] == 0


# ------------------------------------------------------------------------------------------------ 10. the Python route
def test_session_rules_on_id_strings_and_their_explanations():
    """the construction of test_session_recommend_topn_equals_the_statement_on_id_strings and of its audience twin: every
    candidate of every query from the collected dictionaries, on id strings, then the rules of filter_statement"""
    import datetime
    from pyspark import SparkContext, SparkConf
    from pyspark.sql import SQLContext
    from test_gpu_topn import _tool
    from xmap.core.baselinerSim import BaselinerSim
    from xmap.core.extender import ExtendSim
    from xmap.core.generator import Generator
    from xmap.core.recommenderSim import RecommenderSim
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
    idt = ae.state.idt
    iidx, uidx = {i: k for k, i in enumerate(idt.iids)}, {u: k for k, u in enumerate(idt.uids)}
    I, U = len(iidx), len(uidx)
    item_based = RecommenderSim("cosine_item", CAP).build_sthbased_profile(ae, "item").collectAsMap()
    ptool = _tool(ALPHA)
    held = {}                                     # {uid: {iid: [(rating, time)*]}} in the order of the item's list
    for iid, lst in item_based.items():
        for who, ra, when in lst:
            held.setdefault(who, {}).setdefault(iid, []).append((ra, when))
    rng = np.random.default_rng(41)
    no_uid, no_iid = "A%013d" % (10 ** 9 + 1), "B%013dT:" % (10 ** 9 + 1)
    uids = [recs[int(x)][0] for x in rng.integers(0, len(recs), 60)] + [no_uid]
    known = sorted(item_based)
    iids = [known[int(x)] for x in rng.integers(0, len(known), 30)] + [no_iid]
    base = session.recommend_topn(ae, uids, CAP, 10, ALPHA, 1)
    sim_pairs, item_info = base.sim_pairs, base.item_info

    def score(uid, iid):
        ev = [(s * (ra - item_info[nid][0]), abs(s), when) for nid, s in sim_pairs[iid] for ra, when in held.get(uid, {}).get(nid, ())]
        if not ev:
            return None
        b = item_info[iid][0]
        return b + sum(e[0] for e in ev) / sum(e[1] for e in ev), float(b + ptool._decayed_ratio(ev))

    def strings(lists, labels, names):
        return [(lab, [(names[c[0]], c[1], c[2]) for c in l]) for lab, l in zip(labels, lists)]

    # ---- top-N: {position in uids: [(item index, plain, decayed, now, held)*]}, items ascending
    scored = {}
    for q, uid in enumerate(uids):
        l = [(iidx[iid],) + s + (1, iid in held.get(uid, {})) for iid in sorted(sim_pairs) for s in [score(uid, iid)] if s]
        scored[q] = sorted(l)
    allow = [i for i in known if rng.integers(0, 3)] + [no_iid]
    mask = np.zeros(I, bool)
    mask[[iidx[i] for i in allow[:-1]]] = True
    exclude = {uid: [idt.iids[c[0]] for c in scored[q][::4]] + [no_iid] for q, uid in enumerate(uids) if q % 2 == 0}
    exclude[no_uid + "x"] = [known[0]]
    ex_lists = [[iidx[i] for i in exclude.get(uid, []) if i in iidx] for uid in uids]
    floor = float(np.median([c[1] for l in scored.values() for c in l]))
    for n, decay, keep_held, kw in ((10, False, False, dict(allow_items=allow, exclude=exclude, min_score=floor)),
                                    (3, True, True, dict(allow_items=allow)), (64, False, False, dict(exclude=exclude)),
                                    (5, True, False, dict(min_score=floor))):
        out = session.recommend_topn(ae, uids, CAP, 10, ALPHA, n, decay=decay, keep_held=keep_held, explain=2, **kw)
        want = expected_filtered(scored, range(len(uids)), n, int(decay), keep_held, 10 ** 9, I, allow=mask if "allow_items" in kw else None,
                                 exclude=ex_lists if "exclude" in kw else None, min_score=kw.get("min_score"))
        assert out.collect() == strings(want[0], uids, idt.iids)
        assert len(out.stats) == 6 and tuple(out.stats[:2]) + tuple(out.stats[3:]) == want[1][:2] + want[1][3:]
        assert out.stats[0] > 0 and (out.stats[5] > 0) == ("allow_items" in kw or "exclude" in kw) and (out.stats[4] > 0) == ("min_score" in kw)
        # the explanations cover exactly the filtered lists
        assert [(u, [i for i, _ in l]) for u, l in out.explanations] == [(u, [c[0] for c in l]) for u, l in out.collect()]
        assert all(entries for _, l in out.explanations for _, entries in l)
    assert len(base.stats) == 4 and out.collect()[-1] == (no_uid, [])
    # ---- audience: {position in iids: [(user index, plain, decayed, now, held)*]}, users in the train set's order
    inv = {}
    for q, iid in enumerate(iids):
        l = [(uidx[uid],) + s + (1, iid in held[uid]) for uid in held for s in [score(uid, iid) if iid in sim_pairs else None] if s]
        inv[q] = sorted(l)
    allow_u = [u for u in idt.uids if rng.integers(0, 3)] + [no_uid]
    mask = np.zeros(U, bool)
    mask[[uidx[u] for u in allow_u[:-1]]] = True
    exclude = {iid: [idt.uids[c[0]] for c in inv[q][::4]] + [no_uid] for q, iid in enumerate(iids) if q % 2 == 0}
    ex_lists = [[uidx[u] for u in exclude.get(iid, []) if u in uidx] for iid in iids]
    floor = float(np.median([c[1] for l in inv.values() for c in l]))
    for n, decay, keep_holders, kw in ((10, False, False, dict(allow_users=allow_u, exclude=exclude, min_score=floor)),
                                       (300, True, True, dict(allow_users=allow_u)), (1024, False, False, dict(exclude=exclude)),
                                       (5, True, False, dict(min_score=floor))):
        out = session.recommend_audience(ae, iids, CAP, 10, ALPHA, n, decay=decay, keep_holders=keep_holders, **kw)
        want = expected_filtered(inv, range(len(iids)), n, int(decay), keep_holders, 10 ** 9, U, allow=mask if "allow_users" in kw else None,
                                 exclude=ex_lists if "exclude" in kw else None, min_score=kw.get("min_score"))
        assert out.collect() == strings(want[0], iids, idt.uids)
        assert len(out.stats) == 6 and tuple(out.stats[:2]) + tuple(out.stats[3:]) == want[1][:2] + want[1][3:]
        assert out.stats[0] > 0 and (out.stats[5] > 0) == ("allow_users" in kw or "exclude" in kw) and (out.stats[4] > 0) == ("min_score" in kw)
    assert out.collect()[-1] == (no_iid, [])
    # the folded-in twins take the same rules: the same records under new uids give the same audiences under the new names
    kw = dict(allow_users=allow_u, exclude=exclude, min_score=floor)
    first = session.recommend_audience(ae, iids, CAP, 10, ALPHA, 10, **kw)
    renamed = dict(allow_users=["N" + u for u in allow_u], exclude={i: ["N" + u for u in l] for i, l in exclude.items()}, min_score=floor)
    again = session.recommend_audience_profiles(ae, [("N" + u, prof) for u, prof in recs], iids, CAP, 10, ALPHA, 10, **renamed)
    assert again.collect() == [(iid, [("N" + u, p, d) for u, p, d in l]) for iid, l in first.collect()] and again.stats == first.stats


# ----------------------------------------------------------------------------------------------- 11. Engine, on tensors
def test_engine_takes_a_bool_mask_or_packed_words_and_checks_its_arguments():
    """Engine.topn / Engine.audience: a bool mask is packed on the device -- the same answer as filters.pack_mask words, with an
    id space that is no multiple of 32 -- and arguments of the wrong kind raise before any call"""
    import torch
    from test_gpu_explain import _engine, _to, _view
    from xmap.engine.filters import exclusion_csr, pack_mask
    U, I, keep = 50, 403, 5
    assert I & 31 and U & 31
    arrays = _random_case(24, U, I, keep, np.arange(0, I, 3), lambda u: 2 + u % 9)
    eng, P = _engine(), _view(arrays, U, I)
    nb = tuple(_to(a) for a in arrays[4:7])
    avg, w = _to(arrays[7]), _to(wtab(1.5, 66))
    rng = np.random.default_rng(43)
    for call, space, queries in ((eng.topn, I, rng.integers(-1, U + 1, 200)), (eng.audience, U, rng.integers(-1, I + 1, 200))):
        q = _to(queries, np.int32)
        on = rng.integers(0, 2, space) > 0
        on[-1] = True                                   # the id at n - 1, in the partial last word
        ptr, ids = exclusion_csr([rng.integers(-2, space + 2, int(rng.integers(0, 9))).tolist() for _ in queries])
        ex = (_to(ptr), _to(ids))
        by_bool = call(P, nb, q, avg, w, 7, allow=_to(on), exclude=ex, min_score=2.0)
        by_words = call(P, nb, q, avg, w, 7, allow=_to(pack_mask(on, space).view(np.int32)), exclude=ex, min_score=2.0)
        by_ids = call(P, nb, q, avg, w, 7, allow=_to(pack_mask(np.nonzero(on)[0], space).view(np.int32)), exclude=ex, min_score=2.0)
        assert len(by_bool[4]) == 6 and by_bool[4][0] > 0 and by_bool[4][4] > 0 and by_bool[4][5] > 0
        for other in (by_words, by_ids):
            assert all(torch.equal(a, b) for a, b in zip(by_bool[:4], other[:4])) and by_bool[4] == other[4]
        scored = score_users(1.5, queries, *arrays[:8], keep) if call == eng.topn else statement(arrays, keep)
        excl = [ids[ptr[k]:ptr[k + 1]].tolist() for k in range(len(queries))]
        want = expected_filtered(scored, queries, 7, 0, False, 66, space, allow=on, exclude=excl, min_score=2.0)
        check6(tuple(x.cpu().numpy() for x in by_bool[:4]) + (list(by_bool[4]),), want, 7)
        plain = call(P, nb, q, avg, w, 7)
        assert len(plain[4]) == 4                       # no rule: the old entry, four stats
        only_floor = call(P, nb, q, avg, w, 7, min_score=float("-inf"))
        assert all(torch.equal(a, b) for a, b in zip(plain[:4], only_floor[:4])) and only_floor[4] == plain[4] + (0, 0)
        for bad in (dict(allow=_to(on[:-1])), dict(allow=_to(pack_mask(on, space).view(np.int32))[:-1]), dict(allow=_to(on.astype(np.float32))),
                    dict(exclude=(_to(ptr[:-1]), _to(ids))), dict(exclude=(_to(ptr.astype(np.int32)), _to(ids))),
                    dict(exclude=(_to(ptr), _to(ids.astype(np.int64)))), dict(min_score=float("nan"))):
            with pytest.raises(ValueError):
                call(P, nb, q, avg, w, 7, **bad)
