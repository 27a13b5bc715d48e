"""The candidate passes of top-N, audience and group lists at every boundary their emit step has (csrc/id_bitmap.h: the windowed
bitmap, its summary level and the two-pass emit the three kernels share).  The window tests of test_gpu_topn.py,
test_gpu_audience.py, test_gpu_group.py and test_gpu_filter.py pin the window edge and use random ids elsewhere; here ONE designed
id set E sits on both sides of every edge: the bitmap word (31 | 32), the summary word (1023 | 1024), the thread (2047 | 2048
where a thread emits two summary words: top-N and group; for the audience the thread edge is the summary edge) and the window
(W - 1 | W), with the word edges once more at the end of the first window and in the second.

The expected lists and stats come from the Python statements of tests/ alone (score_users, filter_statement, group_statement);
items, users, counts, padding and every h_stats entry are compared exactly, scores as uint64 views."""
import numpy as np
import pytest

from filter_statement import expected_filtered
from test_gpu_audience import ALPHA, KEEP_HOLDERS, OnDevice, _lists, _profiles, _window, audience_rows, statement
from test_gpu_filter import Filter, audience_f, check6, topn_f
from test_gpu_group import Case
from test_gpu_topn import KEEP_HELD, TN_WINDOW, check_output, topn_rows
from test_gpu_topn import expected as expected_plain
from group_statement import MEAN, MIN

pytestmark = pytest.mark.gpu
N_TOP = 64                      # >= |E|: all of E comes back


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


def edge_ids(W):
    return [0, 31, 32, 1023, 1024, 2047, 2048, W - 33, W - 32, W - 1, W, W + 31, W + 32, W + 63]


# what case (c) removes, by position in E: on a query's exclusion list (31, 1024 twice, W - 1; 2048 is masked as well and counts
# once), and cleared in the mask (2047, 2048, W, W + 32)
EXCLUDED, MASKED = (1, 4, 4, 9, 6), (5, 6, 10, 12)


def _mask(n, E):
    on = np.ones(n, bool)
    on[[E[k] for k in MASKED]] = False
    return on


def _left(E, held=(), excluded=(), masked=()):
    """E without the ids at the given positions"""
    gone = set(held) | set(excluded) | set(masked)
    return [e for k, e in enumerate(E) if k not in gone]


def _ids(lists):
    return [sorted(c[0] for c in l) for l in lists]


# ------------------------------------------------------------------------------------------------- top-N and group lists
A, A_EVEN, A_ODD = 5, 6, 7      # the anchors: every id of E lists A, the even positions of E list A_EVEN, the odd ones A_ODD


def item_design():
    """I = TN_WINDOW + 64, keep = 2, five users: 0 holds A (all of E are its candidates), 1 holds A and every second id of E, 2 holds
    A_EVEN and 3 holds A_ODD (their candidates are the even and the odd half of E), 4 has no rows"""
    E = edge_ids(TN_WINDOW)
    U, I, keep = 5, TN_WINDOW + 64, 2
    rows = {0: [(A, 4.0, 1), (A, 2.5, 3)],
            1: [(A, 3.0, 0)] + [(e, 2.0 + (k % 5) / 2.0, k % 3) for k, e in enumerate(E) if k % 2 == 0],
            2: [(A_EVEN, 4.5, 2)], 3: [(A_ODD, 1.5, 1)]}
    lists = {e: (2, [A, A_ODD if k % 2 else A_EVEN], [0.5 + k / 16.0, -0.25 - k / 32.0]) for k, e in enumerate(E)}
    avg = np.round(np.random.default_rng(41).uniform(1.0, 5.0, I), 1)
    return list(_profiles(U, rows)) + list(_lists(I, keep, lists)) + [avg], U, I, keep, E


@pytest.fixture(scope="module")
def items():
    arrays, U, I, keep, E = item_design()
    return Case(arrays, U, I, keep), E


def item_filter(E, I, U):
    """case (c) for the queries [0, 1, 0, U + 1]: query 1 excludes a held id (32), 1023 twice and W + 63"""
    queries = [0, 1, 0, U + 1]
    exclude = [[E[k] for k in EXCLUDED] + [-1, I + 3], [E[2], E[3], E[3], E[13]], [], [E[0]]]
    return queries, Filter(allow=_mask(I, E), exclude=exclude)


def test_topn_every_id_of_E_is_a_candidate(items):
    case, E = items
    queries = [0, 2, 3, 4, -1, 0]
    for rank_by in (0, 1):
        want = expected_plain(case.scored, queries, N_TOP, rank_by, False, 66)
        assert _ids(want[0]) == [E, E[0::2], E[1::2], [], [], E] and want[1][:2] == (3 * len(E), 0)
        check_output(topn_rows(case.arrays, case.U, case.I, case.keep, 1.5, 66, queries, N_TOP, rank_by, 0), want, N_TOP)


@pytest.mark.parametrize("flags", [0, KEEP_HELD])
def test_topn_every_second_id_of_E_is_held(items, flags):
    case, E = items
    queries = [1, 0, 1]
    want = expected_plain(case.scored, queries, N_TOP, 0, bool(flags), 66)
    mine = E if flags else E[1::2]
    assert _ids(want[0]) == [mine, E, mine]
    check_output(topn_rows(case.arrays, case.U, case.I, case.keep, 1.5, 66, queries, N_TOP, 0, flags), want, N_TOP)


@pytest.mark.parametrize("flags", [0, KEEP_HELD])
def test_topn_filtered(items, flags):
    case, E = items
    queries, filt = item_filter(E, case.I, case.U)
    want = expected_filtered(case.scored, queries, N_TOP, 1, bool(flags), 66, case.I, **filt.statement())
    held = () if flags else range(0, len(E), 2)
    assert _ids(want[0]) == [_left(E, (), EXCLUDED, MASKED), _left(E, held, (2, 3, 13), MASKED), _left(E, (), (), MASKED), []]
    removed = [len(E) - len(l) for l in want[0][:3]]
    removed[1] -= 0 if flags else len(E) // 2           # the held ids are no candidates: not removed by the rules
    assert want[1][5] == sum(removed) and want[1][0] == sum(len(l) for l in want[0])
    check6(topn_f(case.D, case.U, case.I, case.keep, 66, queries, N_TOP, 1, flags, filt), want, N_TOP)


@pytest.mark.parametrize("flags", [0, KEEP_HELD])
def test_groups_of_the_even_and_the_odd_half(items, flags):
    case, E = items
    groups = [[2, 3], [3, 2, 1], [2], [0, 4], []]
    exclude = [[E[k] for k in EXCLUDED] + [-1, case.I + 3], [E[3], E[3], E[2]], [], [E[0]], []]
    filt = Filter(allow=_mask(case.I, E), exclude=exclude)
    # the union of the members' candidates, the mask applied, and what the group's list clears of it -- [5] counts that alone
    held = () if flags else range(0, len(E), 2)
    union = [_left(E, (), (), MASKED), _left(E, held, (), MASKED), _left(E[0::2], (), (), [k // 2 for k in MASKED if k % 2 == 0]),
             _left(E, (), (), MASKED), []]
    cleared = [len(set(u) & set(x)) for u, x in zip(union, exclude)]
    assert cleared == [3, 2 if flags else 1, 0, 1, 0]
    for rank_by, how in ((0, MEAN), (1, MIN)):
        got, want = case.check(groups, N_TOP, rank_by, flags, how, filt=filt)
        assert _ids(want[0]) == [sorted(set(u) - set(x)) for u, x in zip(union, exclude)]
        assert got[5][5] == sum(cleared) and got[5][7] == sum(len(u) for u in union) - sum(cleared)
    plain = case.check(groups, N_TOP, 0, flags, MEAN)[1]           # no filter: both halves, nothing counted
    assert _ids(plain[0])[0] == E and plain[1][5] == 0


# ----------------------------------------------------------------------------------------------------------- audience
def user_design():
    """U = AU_WINDOW + 64 users, all without rows but the 14 of E; I = 8, keep = 2.  The user at position k of E holds item 2 (k
    even) or 3 (k odd), and the even positions hold item 0 as well.  Items 0 and 1 list (2, 3): their candidates are all of E, and
    item 0 has every second id of E as a holder; item 4 lists 2 alone: the even half"""
    W = _window()
    E = edge_ids(W)
    U, I, keep = W + 64, 8, 2
    rows = {e: [(3 if k % 2 else 2, 2.0 + (k % 5) / 2.0, k % 4)] + ([] if k % 2 else [(0, 3.0, 1)]) for k, e in enumerate(E)}
    lists = {0: (2, [2, 3], [0.75, -0.5]), 1: (2, [2, 3], [0.25, 0.5]), 4: (1, [2], [1.0])}
    avg = np.asarray([3.0, 2.5, 4.0, 1.5, 3.5, 2.0, 2.0, 2.0])
    return list(_profiles(U, rows)) + list(_lists(I, keep, lists)) + [avg], U, I, keep, E


@pytest.fixture(scope="module")
def users():
    arrays, U, I, keep, E = user_design()
    return OnDevice(arrays), statement(arrays, keep), U, I, keep, E


def user_filter(E, U):
    """case (c) for the queries [1, 0, 1]: query 0 excludes a holder (32), 1023 twice and W + 63"""
    queries = [1, 0, 1]
    exclude = [[E[k] for k in EXCLUDED] + [-1, U + 3], [E[2], E[3], E[3], E[13]], []]
    return queries, Filter(allow=_mask(U, E), exclude=exclude)


@pytest.mark.parametrize("flags", [0, KEEP_HOLDERS])
def test_audience_candidates_and_holders(users, flags):
    D, inv, U, I, keep, E = users
    queries = [1, 0, 4, 2, -1, I, 0]
    for n, rank_by in ((N_TOP, 0), (1024, 1)):
        want = expected_plain(inv, queries, n, rank_by, bool(flags), 66)
        mine = E if flags else E[1::2]
        assert _ids(want[0]) == [E, mine, E[0::2], [], [], [], mine]
        check_output(audience_rows(D, U, I, keep, ALPHA, 66, queries, n, rank_by, flags), want, n)


@pytest.mark.parametrize("flags", [0, KEEP_HOLDERS])
def test_audience_filtered(users, flags):
    D, inv, U, I, keep, E = users
    queries, filt = user_filter(E, U)
    want = expected_filtered(inv, queries, N_TOP, 0, bool(flags), 66, U, **filt.statement())
    held = () if flags else range(0, len(E), 2)
    assert _ids(want[0]) == [_left(E, (), EXCLUDED, MASKED), _left(E, held, (2, 3, 13), MASKED), _left(E, (), (), MASKED)]
    removed = [len(E) - len(l) for l in want[0]]
    removed[1] -= 0 if flags else len(E) // 2
    assert want[1][5] == sum(removed) and want[1][0] == sum(len(l) for l in want[0])
    check6(audience_f(D, U, I, keep, 66, queries, N_TOP, 0, flags, filt), want, N_TOP)
