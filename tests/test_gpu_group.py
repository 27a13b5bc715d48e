"""Group lists on the device (csrc/stage_e_group.hip; xmap_group_topn_rows, xmap_ctx_recommend_group, Engine.group_topn,
session.recommend_group) against tests/group_statement.py -- the statement of the header in Python over the per-member scores of
tests/test_gpu_topn.py.  Items and the least-happy member are compared exactly, scores as uint64 views, the padding behind the
count and all eight stats.  What an input is meant to show is counted from the statement and asserted before the device is asked."""
import ctypes as C
import math

import numpy as np
import pytest

import group_statement as gs
from group_statement import MAX, MEAN, MIN, check_group_output, expected_group, held_sets
from golden_util import CAP
from test_gpu_audience import OnDevice, _lists, _profiles
from test_gpu_coarse_abi import Ctx, _p
from test_gpu_filter import Filter, _same_bits, topn_f
from test_gpu_tail import _few_times, generate, rec_sim, select, wtab
from test_gpu_topn import KEEP_HELD, TN_WINDOW, _hand_case, _random_case, score_users

pytestmark = pytest.mark.gpu
HOWS = (MEAN, MIN, MAX)
NO_FILTER = Filter(null=True)


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


# ------------------------------------------------------------------------------------------------------- the drivers
def _csr(groups):
    ptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    return ptr, np.asarray([u for g in groups for u in g] + [0], np.int32)     # (one entry behind the end: never an empty tensor)


def group_rows_rc(D, n_users, n_items, keep, n_w, groups, n, rank_by, flags, how, veto=None, filt=NO_FILTER, alpha=1.5, csr=None):
    """xmap_group_topn_rows on an OnDevice of (ptr, item, rating, time, cnt, col, sim, avg): (rc, (cnt, item, plain, decayed, low,
    stats)); the outputs are pre-filled with -7"""
    import torch
    from xmap.engine import hipabi as abi
    dev = "cuda:0"
    ptr, pit, pra, pti, cnt, col, sim, avg = D.t
    g_ptr, g_user = _csr(groups) if csr is None else csr
    G = len(g_ptr) - 1
    d_ptr, d_user = torch.from_numpy(np.ascontiguousarray(g_ptr, np.int64)).to(dev), torch.from_numpy(np.ascontiguousarray(g_user, np.int32)).to(dev)
    w = torch.from_numpy(wtab(alpha, n_w)).to(dev)
    o_cnt = torch.full((max(G, 1),), -7, dtype=torch.int32, device=dev)
    o_item, o_low = [torch.full((max(G, 1), n), -7, dtype=torch.int32, device=dev) for _ in range(2)]
    o_plain, o_decay = [torch.full((max(G, 1), n), -7.0, dtype=torch.float64, device=dev) for _ in range(2)]
    h = (C.c_int64 * 8)(*([-7] * 8))
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    F, alive = filt.on_device()
    rc = abi.lib.xmap_group_topn_rows(st, abi.i64(G), abi.vp(d_ptr), abi.vp(d_user), abi.i32(n), abi.i32(rank_by), abi.i32(flags), abi.i32(how),
                                      C.c_double(-math.inf if veto is None else veto), abi.i64(n_users), abi.i32(n_items), abi.i32(keep),
                                      abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ptr), abi.vp(pit), abi.vp(pra), abi.vp(pti), abi.vp(avg),
                                      abi.vp(w), abi.i32(n_w), abi.vp(o_cnt), abi.vp(o_item), abi.vp(o_plain), abi.vp(o_decay), abi.vp(o_low),
                                      None if F is None else C.byref(F), h)
    torch.cuda.synchronize()
    del alive
    return rc, (o_cnt[:G].cpu().numpy(), o_item[:G].cpu().numpy(), o_plain[:G].cpu().numpy(), o_decay[:G].cpu().numpy(),
                o_low[:G].cpu().numpy(), [int(x) for x in h])


def group_rows(*a, **kw):
    rc, out = group_rows_rc(*a, **kw)
    assert rc == 0
    return out


def make_groups(U, G, gseed):
    """the shared construction: sizes 1 .. 8 in turn, then a group of 64 and an empty one; members drawn from [-2, U + 2)"""
    rng = np.random.default_rng(gseed)
    sizes = [(g % 8) + 1 for g in range(G)] + [64, 0]
    return [rng.integers(-2, U + 2, m).tolist() for m in sizes]


class Case(object):
    """arrays on the device + the per-member scores and the held sets of the statement, computed once"""

    def __init__(self, arrays, U, I, keep, alpha=1.5):
        self.arrays, self.U, self.I, self.keep, self.alpha = arrays, U, I, keep, alpha
        self.D = OnDevice(arrays)
        self.scored = score_users(alpha, range(U), *arrays[:8], keep)
        self.held = held_sets(arrays[0], arrays[1], I)

    def want(self, groups, n, rank_by, flags, how, n_w=66, veto=None, filt=NO_FILTER, census=None):
        return expected_group(self.scored, self.held, groups, self.arrays[7], n, rank_by, bool(flags), n_w, how, self.I, veto=veto,
                              census=census, **({} if filt.null else filt.statement()))

    def got(self, groups, n, rank_by, flags, how, n_w=66, veto=None, filt=NO_FILTER):
        return group_rows(self.D, self.U, self.I, self.keep, n_w, groups, n, rank_by, flags, how, veto, filt, self.alpha)

    def check(self, groups, n, rank_by, flags, how, **kw):
        want = self.want(groups, n, rank_by, flags, how, **kw)
        got = self.got(groups, n, rank_by, flags, how, **kw)
        print("stats", got[5], "statement", want[1])
        check_group_output(got, want, n)
        return got, want


@pytest.fixture(scope="module")
def case2():
    U, I, keep = 50, 400, 5
    return Case(_random_case(24, U, I, keep, np.arange(0, I, 3), lambda u: 2 + u % 9), U, I, keep)


# ------------------------------------------------------------------------------------------- 1. a group of one is top-N
def test_a_group_of_one_is_top_n():
    arrays, U, I, keep, dup_user = _hand_case()
    D = OnDevice(arrays)
    queries = list(range(U)) + [U + 5]
    groups = [[u] for u in queries]
    for n, rank_by, flags in ((10, 0, 0), (64, 1, KEEP_HELD), (5, 1, 0)):
        short = topn_f(D, U, I, keep, 66, queries, n, rank_by, flags, NO_FILTER)
        assert short[4][2] > 66 and short[4][1] > 0                 # evidence beyond the LDS staging (the arena launch), a short table
        full = topn_f(D, U, I, keep, short[4][2], queries, n, rank_by, flags, NO_FILTER)
        assert full[4][1] < short[4][1]
        for how in HOWS:
            for n_w, ref in ((66, short), (short[4][2], full)):
                got = group_rows(D, U, I, keep, n_w, groups, n, rank_by, flags, how)
                assert _same_bits(got, ref)
                assert got[5][:4] == ref[4][:4] and got[5][2] > 66 and got[5][4:7] == [0, 0, 0] and got[5][7] == ref[4][0]
                for g in range(len(groups)):
                    assert (got[4][g, :got[0][g]] == 0).all() and (got[4][g, got[0][g]:] == -1).all()


# ------------------------------------------------------------------------------ 2. random groups against the statement
def test_random_groups_against_the_statement(case2):
    groups = make_groups(case2.U, 200, 31)
    cz = {}
    case2.want(groups, 64, 0, 0, MEAN, census=cz)
    print("census", cz)
    assert cz == dict(candidates=3779, held_by_another=289, two_or_more=496, lacking=3639, empty=4, widest=54, ghosts=67)
    for how in HOWS:
        for rank_by in (0, 1):
            for flags in (0, KEEP_HELD):
                for n in (3, 64):
                    got, want = case2.check(groups, n, rank_by, flags, how)
                    assert got[0][-1] == 0 and got[0][-2] > 0       # the empty group, the group of 64
    # the orders differ between the aggregates, and the least-happy member is not always the first
    by_how = [case2.want(groups, 3, 0, 0, how)[0] for how in HOWS]
    assert sum([c[0] for c in a] != [c[0] for c in b] for a, b in zip(by_how[0], by_how[1])) > 0
    assert sum([c[0] for c in a] != [c[0] for c in b] for a, b in zip(by_how[0], by_how[2])) > 0
    assert any(c[3] > 0 for l in by_how[0] for c in l)
    # a veto at the median member score, a floor at the median aggregate
    flat = sorted(c[1] for l in case2.want(groups, 64, 0, 0, MEAN)[0] for c in l)
    mid = flat[len(flat) // 2]
    for how in HOWS:
        got, want = case2.check(groups, 64, 0, 0, how, veto=mid - 1.0, filt=Filter(min_score=mid))
        assert want[1][6] > 0 and want[1][4] > 0 and sum(len(l) for l in want[0]) > 0


# ---------------------------------------------------------------------------------------------------- 3. wide groups
def test_wide_groups():
    U, I, keep = 6, 3000, 4
    case = Case(_random_case(21, U, I, keep, np.arange(0, I, 2), lambda u: 1000 if u == 2 else 3 + u), U, I, keep)
    groups = make_groups(U, 40, 32)
    cz = {}
    case.want(groups, 64, 0, 0, MEAN, census=cz)
    print("census", cz)
    assert cz["widest"] == 604 > 256 and cz["candidates"] == 11705 and cz["held_by_another"] == 134
    for how, rank_by, flags in ((MEAN, 0, 0), (MIN, 1, KEEP_HELD), (MAX, 0, 0)):
        got, want = case.check(groups, 64, rank_by, flags, how)
        assert want[1][3] > 256 and max(len(l) for l in want[0]) == 64 and want[1][1] > 0


# ----------------------------------------------------------------------------------------------- 4. across the window
def test_groups_across_the_window():
    U, I, keep = 20, TN_WINDOW + 100, 2
    rng = np.random.default_rng(23)                     # the builder of test_an_item_space_just_above_the_window
    listed = np.unique(np.concatenate([[0, TN_WINDOW - 1, TN_WINDOW, I - 1], rng.integers(0, I, 100), rng.integers(TN_WINDOW, I, 96)]))
    pool = rng.integers(0, I, 30)
    arrays = _random_case(23, U, I, keep, listed, lambda u: 8)
    arrays[5][listed] = pool[rng.integers(0, 30, (len(listed), keep))]
    arrays[4][listed] = keep
    arrays[1][:] = pool[rng.integers(0, 30, len(arrays[1]))]
    arrays[1][arrays[0][4]] = TN_WINDOW                 # user 4 holds TN_WINDOW, user 5 holds TN_WINDOW - 1
    arrays[1][arrays[0][5]] = TN_WINDOW - 1
    case = Case(arrays, U, I, keep)
    edges = [0, TN_WINDOW - 1, TN_WINDOW, I - 1]
    both = [u for u in range(U) if u not in (4, 5) and {TN_WINDOW - 1, TN_WINDOW} <= {c[0] for c in case.scored[u]}]
    assert both, "a third member with evidence for both edge items"
    third = both[0]
    grng = np.random.default_rng(33)
    groups = [[4, 5, third], [third, 5, 4, third]] + [grng.integers(-1, U + 1, int(grng.integers(2, 5))).tolist() for _ in range(30)]
    exclude = [[] for _ in groups]
    for g in range(2, len(groups), 3):
        exclude[g] = edges + [-1, I, I + 7, -5] + edges[:2] + [int(x) for x in grng.integers(0, I, 3)]
    exclude[1] = [TN_WINDOW, TN_WINDOW, 5]
    few = np.zeros(I, bool)                             # a mask of the edges and some more: short lists, nothing is cut
    few[edges] = True
    few[listed[::5]] = True
    for flags in (0, KEEP_HELD):
        got, want = case.check(groups, 64, 0, flags, MEAN)
        assert want[1][3] > 64 and len(want[0][0]) == 64
        got, want = case.check(groups, 64, 0, flags, MAX, filt=Filter(allow=few))
        assert want[1][3] < 64
        first = {c[0] for c in want[0][0]}              # held by members 4 and 5, candidates of the third: both leave without the flag
        assert len({TN_WINDOW - 1, TN_WINDOW} & first) == (2 if flags else 0)
        assert set(edges) <= {c[0] for l in want[0] for c in l}
        got, want = case.check(groups, 64, 1, flags, MIN, filt=Filter(allow=few, exclude=exclude))
        assert want[1][5] > 0 and not set(edges) & {c[0] for g in range(2, len(groups), 3) for c in want[0][g]}
        second = {c[0] for c in want[0][1]}
        assert TN_WINDOW not in second and (TN_WINDOW - 1 in second) == bool(flags)
        only = case.check(groups, 64, 1, flags, MIN, filt=Filter(exclude=exclude))[1]
        assert only[1][5] >= want[1][5] > 0             # the lists alone


# ----------------------------------------------------------------------------------------------- 5. designed aggregates
def _designed():
    """candidate item q has the single neighbour Q + q with similarity 1.0 and every average is 0.0, so the plain score of a
    member that holds Q + q with rating r is r exactly (0 + (1.0 * (r - 0)) / |1.0|); a member that does not hold it has no
    evidence and predicts the average, 0.0.  Item 4's neighbour has similarity 0.0: a zero weight sum for whoever holds it."""
    Q, U, keep = 8, 6, 1
    I = 2 * Q
    score = {0: {0: 2.0, 1: 3.0, 2: 2.0, 3: 2.0, 4: 1.0, 5: 4.0, 6: 2.5, 7: -5e-324},    # member: {item: rating of its neighbour}
             1: {0: 4.0, 1: 3.0, 2: 5.0, 3: 3.0, 5: 4.0, 6: 2.5, 7: 0.0},
             2: {0: 3.0, 1: 3.0, 2: 2.0, 3: 2.0, 5: 1.0, 6: 2.5},
             3: {5: 4.0}}
    rows = {u: [(Q + q, r, (u + q) % 3) for q, r in d.items()] for u, d in score.items()}
    # item 7, average -0.0: member 0 holds its neighbour twice, -5e-324 and 0.0 -- (-5e-324 + 0.0) / 2 rounds to -0.0, and
    # -0.0 + -0.0 = -0.0; member 1's 0.0 gives -0.0 + 0.0 = 0.0; member 2 has no evidence: the average, -0.0
    rows[0].append((Q + 7, 0.0, 2))
    lists = {q: (1, [Q + q], [0.0 if q == 4 else 1.0]) for q in range(Q)}
    avg = np.zeros(I)
    avg[7] = -0.0
    arrays = list(_profiles(U, rows)) + list(_lists(I, keep, lists)) + [avg]
    return Case(arrays, U, I, keep), score


def test_designed_aggregates():
    case, score = _designed()
    assert [c[1] for c in case.scored[0]] == [2.0, 3.0, 2.0, 2.0, None, 4.0, 2.5, -0.0]  # the design holds: scores are the ratings
    assert [math.copysign(1.0, case.scored[u][-1][1]) for u in (0, 1)] == [-1.0, 1.0] and case.scored[2][-1][0] == 6
    pair = [[0, 1]]
    # items 0 and 1: the means tie (3.0) while the minima do not (2.0, 3.0); items 2 and 3: the minima tie, the means do not
    mean = {c[0]: c for c in case.want(pair, 64, 0, 0, MEAN)[0][0]}
    low = {c[0]: c for c in case.want(pair, 64, 0, 0, MIN)[0][0]}
    assert mean[0][1] == mean[1][1] == 3.0 and low[0][1] == 2.0 and low[1][1] == 3.0
    assert low[2][1] == low[3][1] == 2.0 and mean[2][1] == 3.5 and mean[3][1] == 2.5
    assert mean[1][3] == 0 and mean[6][3] == 0 and mean[0][3] == 0      # the least-happy member on a tie: the first
    assert 4 not in mean                                                # member 0 has a zero weight sum for item 4: gone for the group
    for how in HOWS:
        for rank_by in (0, 1):
            got, want = case.check(pair + [[1, 0], [1], [0], [1, 2, 0], [3, 3], [5, 4]], 64, rank_by, 0, how)
            assert want[1][1] == 4                                      # item 4, in every group with member 0
            if rank_by == 0:
                assert got[1][0, :2].tolist() == {MEAN: [5, 2], MIN: [5, 1], MAX: [2, 0]}[how]
    # a veto equal to one member's score: it stays; the next double above: it leaves
    for how in HOWS:
        at, _ = case.check(pair, 64, 0, 0, how, veto=2.0)
        above, want = case.check(pair, 64, 0, 0, how, veto=math.nextafter(2.0, 3.0))
        assert {0, 2, 3} <= set(at[1][0].tolist()) and not {0, 2, 3} & set(above[1][0].tolist()) and want[1][6] == 4    # and item 7
    # a floor on a tie of aggregates: both stay at the score, both leave above it
    at, want = case.check(pair, 64, 0, 0, MEAN, filt=Filter(min_score=3.0))
    assert at[1][0, :at[0][0]].tolist() == [5, 2, 0, 1] and want[1][4] == 3
    above, want = case.check(pair, 64, 0, 0, MEAN, filt=Filter(min_score=math.nextafter(3.0, 4.0)))
    assert above[1][0, :above[0][0]].tolist() == [5, 2] and want[1][4] == 5
    # -0.0 and 0.0: min and max take the first member's bits, the mean's sum starts from the first score
    for how in HOWS:
        got, _ = case.check([[0, 1], [1, 0], [0], [0, 0], [2, 0], [1, 2]], 64, 0, 0, how)
        bits = [got[2][g, got[1][g].tolist().index(7)].tobytes() for g in range(6)]
        neg, pos = np.float64(-0.0).tobytes(), np.float64(0.0).tobytes()
        assert bits == ([pos, pos, neg, neg, neg, pos] if how == MEAN else [neg, pos, neg, neg, neg, pos])
    # one user three times against the same user once plus two others
    got, want = case.check([[0, 0, 0], [0, 1, 2], [0]], 64, 0, 0, MEAN)
    assert _same_bits([x[:1] for x in got[1:3]], [x[2:3] for x in got[1:3]]) and want[1][0] == 3 * 8 + (8 + 7 + 6) + 8
    assert got[2][1, got[1][1].tolist().index(0)] == 3.0 and got[2][0, got[1][0].tolist().index(0)] == 2.0


# ---------------------------------------------------------------------------------------------- 6. many groups per block
def test_many_groups_per_block(case2):
    """more groups than the candidate pass has blocks (2 048): a block then serves group after group on one bitmap"""
    rng = np.random.default_rng(36)
    distinct = [rng.integers(-2, case2.U + 2, int(rng.integers(1, 7))).tolist() for _ in range(1250)]
    groups = distinct * 4
    for g in range(0, 1250, 5):
        groups[g] = groups[g] + groups[g][:2]           # members repeat
    groups[4999] = rng.integers(0, case2.U, 64).tolist()
    exclude = [rng.integers(-3, case2.I + 3, int(rng.integers(0, 12))).tolist() for _ in groups]
    got, want = case2.check(groups, 3, 1, 0, MEAN, filt=Filter(exclude=exclude, min_score=2.5))
    assert want[1][5] > 0 and want[1][4] > 0 and got[0][4999] == 3
    assert got[1][1].tolist() == got[1][1251].tolist() or exclude[1] != exclude[1251]
    got, _ = case2.check(groups, 3, 0, KEEP_HELD, MAX)
    assert all(got[1][g].tolist() == got[1][g + 1250].tolist() for g in range(1, 1250, 5))     # a repeated group, the same list
    empty = case2.got([], 10, 0, 0, MEAN)
    assert empty[5] == [0] * 8
    none = case2.got([[], [], []], 10, 0, 0, MEAN)
    assert none[5] == [0] * 8 and not none[0].any() and (none[1] == -1).all() and (none[4] == -1).all()


# ------------------------------------------------------------------------------------------------------------ 7. masks
def test_masks(case2):
    groups = make_groups(case2.U, 60, 37)
    plain = case2.got(groups, 10, 0, 0, MEAN)
    ones = case2.got(groups, 10, 0, 0, MEAN, filt=Filter(allow=np.ones(case2.I, bool)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain[:5], ones[:5])) and plain[5] == ones[5] and plain[5][0] > 0
    zeros = case2.got(groups, 10, 0, 0, MEAN, filt=Filter(allow=np.zeros(case2.I, bool)))
    assert not zeros[0].any() and (zeros[1] == -1).all() and (zeros[4] == -1).all() and zeros[5] == [0] * 8    # nothing is scored
    mask = np.random.default_rng(38).random(case2.I) < 0.3
    for how in HOWS:
        got, want = case2.check(groups, 10, 1, KEEP_HELD, how, filt=Filter(allow=mask))
        assert 0 < want[1][0] < plain[5][0] and all(mask[c[0]] for l in want[0] for c in l)
    # the statement restricted to the mask: the unmasked lists (n = 64 holds every candidate here) cut down on the host
    full = case2.want(groups, 64, 0, 0, MIN)
    assert full[1][3] <= 64
    got, _ = case2.check(groups, 64, 0, 0, MIN, filt=Filter(allow=mask))
    for g, l in enumerate(full[0]):
        assert got[1][g, :got[0][g]].tolist() == [c[0] for c in l if mask[c[0]]]


# ------------------------------------------------------------------------------------------------------ 8. pair ranges
def test_the_member_pass_in_pair_ranges(case2, monkeypatch):
    groups = make_groups(case2.U, 200, 31)
    whole = case2.got(groups, 64, 1, 0, MEAN)
    monkeypatch.setenv("XMAP_PAIR_RANGE", "3")
    cut = case2.got(groups, 64, 1, 0, MEAN)
    monkeypatch.delenv("XMAP_PAIR_RANGE")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole[:5], cut[:5])) and whole[5] == cut[5] and whole[5][0] > 3


# ------------------------------------------------------------------------------------------------------ 9. coarse entry
def _coarse_group(ctx, source, groups, n, rank_by, flags, how, veto=None, filt=NO_FILTER, n_w=66, alpha=1.5, csr=None, fill=-7):
    g_ptr, g_user = _csr(groups) if csr is None else csr
    G, w = len(g_ptr) - 1, wtab(alpha, n_w)
    cnt, ids, low = np.full(G, fill, np.int32), np.full((G, n), fill, np.int32), np.full((G, n), fill, np.int32)
    plain, decay, stats = np.full((G, n), float(fill)), np.full((G, n), float(fill)), np.full(8, fill, np.int64)
    F, alive = filt.on_host()
    rc = ctx.lib.xmap_ctx_recommend_group(ctx.h, source, G, _p(g_ptr, C.c_int64), _p(g_user, C.c_int32), n, rank_by, flags, how,
                                          C.c_double(-math.inf if veto is None else veto), _p(w, C.c_double), n_w, _p(cnt, C.c_int32),
                                          _p(ids, C.c_int32), _p(plain, C.c_double), _p(decay, C.c_double), _p(low, C.c_int32),
                                          None if F is None else C.byref(F), _p(stats, C.c_int64))
    del alive
    return rc, (cnt, ids, plain, decay, low, stats.tolist())


def test_the_coarse_entry_over_the_three_sources():
    from test_gpu_foldin import foldin, foldin_download
    from test_gpu_item_foldin import item_foldin, item_foldin_download
    from xmap.engine import hipabi as abi, synth
    seed, users, src, tgt, overlap = 5, 1500, 300, 300, 0.4          # the contexts of test_gpu_filter's coarse test
    r = _few_times(synth.make_two_domain(seed, users, src, tgt, overlap=overlap))
    I, U, keep = r.n_items, users, 1
    rng = np.random.default_rng(seed)
    ctx = Ctx()
    try:
        rows = generate(ctx, r)
        T = rec_sim(ctx, I, U, len(rows["user"]))
        cnt, col, sim, _ = select(ctx, I, keep)
        arrays = [T["ptr"], T["item"], T["rating"], T["time"], cnt, col, sim, T["avg"]]
        groups0 = make_groups(U, 40, 39)
        # before any fold-in: the source is refused, the outputs are untouched
        for source in (1, 2):
            rc, out = _coarse_group(ctx, source, groups0, 5, 0, 0, MEAN)
            assert rc == abi.ERR_ARG and ctx.lib.xmap_last_error() and (out[0] == -7).all() and out[5] == [-7] * 8
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
        folded = list(foldin_download(ctx, B, f_counts[0])) + arrays[4:]
        b_rows, (n_cnt, n_col, n_sim, _) = item_foldin_download(ctx, NB, b_counts[0], keep)
        extended = arrays[:4] + [np.concatenate([cnt, n_cnt]), np.concatenate([col, n_col]), np.concatenate([sim, n_sim]),
                                 np.concatenate([T["avg"], b_rows[5]])]
        for source, arr, n_users, n_ids in ((0, arrays, U, I), (1, folded, B, I), (2, extended, U, I + NB)):
            D = OnDevice(arr)
            groups = make_groups(n_users, 40, 39 + source)
            mask = rng.integers(0, 4, n_ids) > 0
            exclude = [rng.integers(-2, n_ids + 2, int(rng.integers(0, 30))).tolist() for _ in groups]
            for n, rank_by, flags, how, veto, filt in ((10, 0, 0, MEAN, None, NO_FILTER), (64, 1, KEEP_HELD, MIN, 2.0, Filter(allow=mask, exclude=exclude)),
                                                       (5, 0, 0, MAX, None, Filter(exclude=exclude, min_score=3.0))):
                fine = group_rows(D, n_users, n_ids, keep, 66, groups, n, rank_by, flags, how, veto, filt)
                rc, got = _coarse_group(ctx, source, groups, n, rank_by, flags, how, veto, filt)
                assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got[:5], fine[:5])) and got[5] == fine[5]
                assert got[5][0] > 0 and got[5][7] > 0 and got[0].max() > 0
            if source == 2:                         # batch items are returned as I + q: a mask of the batch alone
                only_batch = Filter(allow=np.arange(n_ids) >= I)
                fine = group_rows(D, n_users, n_ids, keep, 66, groups, 10, 0, KEEP_HELD, MEAN, None, only_batch)
                rc, got = _coarse_group(ctx, source, groups, 10, 0, KEEP_HELD, MEAN, None, only_batch)
                assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got[:5], fine[:5])) and got[5] == fine[5]
                assert got[0].max() > 0 and (got[1][got[1] >= 0] >= I).all()
        # the statement over the downloaded arrays, once (the fine call is held to it everywhere else)
        case = Case(arrays, U, I, keep)
        rc, got = _coarse_group(ctx, 0, groups0, 10, 0, 0, MEAN)
        assert rc == 0
        want = case.want(groups0, 10, 0, 0, MEAN)
        check_group_output(got, want, 10)
        good = got
        # ---- argument errors: a message, the outputs as they were, and the context answers the next call
        ptr, user = _csr(groups0)

        def refused(**kw):
            kw.setdefault("how", MEAN)
            rc, out = _coarse_group(ctx, kw.pop("source", 0), groups0, kw.pop("n", 10), 0, 0, kw.pop("how"), **kw)
            assert rc == abi.ERR_ARG and ctx.lib.xmap_last_error(), kw
            assert (out[0] == -7).all() and (out[1] == -7).all() and (out[2] == -7.0).all() and (out[4] == -7).all() and out[5] == [-7] * 8
            rc, again = _coarse_group(ctx, 0, groups0, 10, 0, 0, MEAN)
            assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(again[:5], good[:5])) and again[5] == good[5]

        refused(how=3)
        refused(how=-1)
        refused(veto=float("nan"))
        refused(n=0)
        refused(n=65)
        first = ptr.copy()
        first[0] = 1
        refused(csr=(first, user))
        down = ptr.copy()
        down[20] = down[19] - 1
        refused(csr=(down, user))
        big = np.asarray([0, 65], np.int64)
        rc, out = _coarse_group(ctx, 0, None, 10, 0, 0, MEAN, csr=(big, np.zeros(66, np.int32)))
        assert rc == abi.ERR_ARG and b"65" in ctx.lib.xmap_last_error() and (out[0] == -7).all()
        refused(filt=Filter(min_score=float("nan")))
        refused(source=3)
        # the fine-grained call checks grp_ptr on the device before any other work
        D = OnDevice(arrays)
        for csr in ((first, user), (down, user), (big, np.zeros(66, np.int32))):
            rc, out = group_rows_rc(D, U, I, keep, 66, None, 10, 0, 0, MEAN, csr=csr)
            assert rc == abi.ERR_ARG and (out[0] == -7).all() and (out[1] == -7).all() and (out[4] == -7).all()
        for kw in (dict(how=3), dict(veto=float("nan")), dict(filt=Filter(min_score=float("nan")))):
            kw.setdefault("how", MEAN)
            rc, out = group_rows_rc(D, U, I, keep, 66, groups0, 10, 0, 0, kw.pop("how"), **kw)
            assert rc == abi.ERR_ARG and (out[0] == -7).all()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 10. the Python routes
def test_engine_group_topn_on_tensors(case2):
    import torch
    from test_gpu_explain import _engine, _to, _view
    from xmap.engine.filters import exclusion_csr
    eng, P = _engine(), _view(case2.arrays, case2.U, case2.I)
    nb = tuple(_to(a) for a in case2.arrays[4:7])
    avg, w = _to(case2.arrays[7]), _to(wtab(1.5, 66))
    groups = make_groups(case2.U, 60, 40)
    ptr, user = _csr(groups)
    rng = np.random.default_rng(40)
    on = rng.integers(0, 2, case2.I) > 0
    excl = [rng.integers(-2, case2.I + 2, int(rng.integers(0, 9))).tolist() for _ in groups]
    e_ptr, e_ids = exclusion_csr(excl)
    out = eng.group_topn(P, nb, _to(ptr), _to(user[:-1]), avg, w, 7, how="min", veto=1.5, rank_by=1, keep_held=True, allow=_to(on),
                         exclude=(_to(e_ptr), _to(e_ids)), min_score=2.0)
    want = case2.want(groups, 7, 1, KEEP_HELD, MIN, veto=1.5, filt=Filter(allow=on, exclude=excl, min_score=2.0))
    check_group_output(tuple(x.cpu().numpy() for x in out[:5]) + (out[5],), want, 7)
    assert isinstance(out[5], list) and len(out[5]) == 8 and want[1][6] > 0 and want[1][5] > 0 and want[1][4] > 0
    # the layout of topn(): diversify() takes the lists as a pool; weight 0 returns the pool's prefix
    pool = eng.group_topn(P, nb, _to(ptr), _to(user[:-1]), avg, w, 20)
    for bad in (dict(how="median"), dict(how=3), dict(veto=float("nan")), dict(min_score=float("nan")), dict(allow=_to(on[:-1]))):
        with pytest.raises(ValueError):
            eng.group_topn(P, nb, _to(ptr), _to(user[:-1]), avg, w, 7, **bad)
    with pytest.raises(ValueError):
        eng.group_topn(P, nb, _to(ptr), _to(user[:-1]), avg, w, 65)
    assert torch.equal(pool[0], torch.from_numpy(case2.got(groups, 20, 0, 0, MEAN)[0]).to(pool[0].device))


def test_session_recommend_group_on_id_strings():
    """the construction of test_session_recommend_topn_equals_the_statement_on_id_strings; the per-member scores from the
    collected dictionaries, then the statement, on id strings"""
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
    alpha = 1.5
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
    iidx = {i: k for k, i in enumerate(idt.iids)}
    I = len(iidx)
    item_based = RecommenderSim("cosine_item", CAP).build_sthbased_profile(ae, "item").collectAsMap()
    ptool = _tool(alpha)
    mine = {}                                     # {uid: {iid: [(rating, time)*]}} in the order of the item's list
    for iid, lst in item_based.items():
        for who, ra, when in lst:
            mine.setdefault(who, {}).setdefault(iid, []).append((ra, when))
    rng = np.random.default_rng(44)
    no_uid, no_iid = "A%013d" % (10 ** 9 + 1), "B%013dT:" % (10 ** 9 + 1)
    uids = [recs[int(x)][0] for x in rng.integers(0, len(recs), 40)] + [no_uid]
    pos = {u: k for k, u in enumerate(uids)}
    groups = [("g%02d" % g, [uids[int(x)] for x in rng.integers(0, len(uids), 1 + g % 5)]) for g in range(24)]
    groups += [("ghosts", [no_uid, no_uid]), ("nobody", []), ("with a ghost", [uids[0], no_uid, uids[1]])]
    base = session.recommend_group(ae, groups, CAP, 10, alpha, 1)
    sim_pairs, item_info = base.sim_pairs, base.item_info
    avg = np.zeros(I)
    for iid, info in item_info.items():
        avg[iidx[iid]] = info[0]
    scored = {}
    for q, uid in enumerate(uids):
        l = []
        for iid in sorted(sim_pairs):
            ev = [(s * (ra - item_info[nid][0]), abs(s), when) for nid, s in sim_pairs[iid] for ra, when in mine.get(uid, {}).get(nid, ())]
            if ev:
                b = item_info[iid][0]
                l.append((iidx[iid], b + sum(e[0] for e in ev) / sum(e[1] for e in ev), float(b + ptool._decayed_ratio(ev)), 1,
                          iid in mine.get(uid, {})))
        scored[q] = sorted(l)
    held = [{iidx[i] for i in mine.get(uid, {})} for uid in uids]
    members = [[pos[u] for u in m] for _, m in groups]
    allow = [i for i in sorted(item_based) if rng.integers(0, 3)] + [no_iid]
    mask = np.zeros(I, bool)
    mask[[iidx[i] for i in allow[:-1]]] = True
    first = expected_group(scored, held, members, avg, 64, 0, False, 10 ** 9, MEAN, I)
    exclude = {gid: [idt.iids[c[0]] for c in first[0][g][::3]] + [no_iid] for g, (gid, _) in enumerate(groups) if g % 2 == 0}
    exclude["no such group"] = [idt.iids[0]]
    ex_lists = [[iidx[i] for i in exclude.get(gid, []) if i in iidx] for gid, _ in groups]
    floor = float(np.median([c[1] for l in first[0] for c in l]))
    for n, how, decay, keep_held, veto, kw in ((10, "mean", False, False, None, {}), (5, "min", True, False, floor - 1.0, dict(exclude=exclude)),
                                               (64, "max", False, True, None, dict(allow_items=allow, min_score=floor)),
                                               (3, "mean", True, True, floor - 0.5, dict(allow_items=allow, exclude=exclude, min_score=floor))):
        out = session.recommend_group(ae, groups, CAP, 10, alpha, n, how=how, veto=veto, decay=decay, keep_held=keep_held, **kw)
        want = expected_group(scored, held, members, avg, n, int(decay), keep_held, 10 ** 9, gs.MEAN if how == "mean" else gs.MIN if how == "min" else gs.MAX,
                              I, veto=veto, allow=mask if "allow_items" in kw else None, exclude=ex_lists if "exclude" in kw else None,
                              min_score=kw.get("min_score"))
        assert out.collect() == [(gid, [(idt.iids[c[0]], c[1], c[2], m[c[3]]) for c in l]) for (gid, m), l in zip(groups, want[0])]
        assert all(low in m for (gid, m), (_, l) in zip(groups, out.collect()) for _, _, _, low in l)     # low_uid is a member
        assert len(out.stats) == 8 and out.stats[:2] + out.stats[3:] == want[1][:2] + want[1][3:] and out.stats[0] > 0
        assert (out.stats[6] > 0) == (veto is not None) and (out.stats[5] > 0) == ("exclude" in kw) and (out.stats[4] > 0) == ("min_score" in kw)
    got = dict(base.collect())
    assert got["ghosts"] == [] and got["nobody"] == []
    with pytest.raises(ValueError):
        session.recommend_group(ae, [("big", [uids[0]] * 65)], CAP, 10, alpha, 5)
    # members that are profiles folded in: the same records under new uids give the same lists under the new names
    again = session.recommend_group_profiles(ae, [("N" + u, prof) for u, prof in recs], [(gid, ["N" + u for u in m]) for gid, m in groups],
                                             CAP, 10, alpha, 10)
    ref = session.recommend_group(ae, groups, CAP, 10, alpha, 10)
    assert again.collect() == [(gid, [(i, p, d, "N" + u) for i, p, d, u in l]) for gid, l in ref.collect()] and again.stats == ref.stats
