"""RecommenderSim on the device over the designed inputs of tests/rec_sim_rows.py (tests/test_cpu_rec_sim_rows.py states what each
family reaches and asserts it on the CPU): Engine.rec_sim over DeviceRatings(..., rating64=True) -- the LS instantiation of the
pair kernels, which no other path runs -- at two slot targets,

  * the plan the device made equals the NumPy statement of the plan without a heavy set (check_plan, duplicates allowed),
  * the result equals the CPU oracle's, whole: rows, columns and n_ij as integers, sim, ls and the norms as bit patterns
    (same_doubles: a NaN equals a NaN, everything else by its 64 bits), and
  * the rows of the value families, and the chosen rows of the layout families, equal the Python statement (math.fsum).

Further: an overflowing table is answered by a halved slot target and the same bytes as a direct run, two runs give the same
bytes, the round-2 mirror (XMAP_A_V2=1: k_scatter's j == i branch) gives the same result on the self-pair inputs, and the
coarse ABI (NumPy only) computes the oracle's result on profiles it made itself -- with every row held twice through
xmap_ctx_union.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import rec_sim_rows as rs
from rec_sim_rows import CAPS, LAYOUT_FAMILIES, SMALL_TARGET, VALUE_FAMILIES, bits, same_doubles, same_row
from test_cpu_stage_a_layout import check_plan, plan_statement

pytestmark = pytest.mark.gpu
CAP = 50
TARGETS = (768, SMALL_TARGET)          # the engine's default, and one that cuts rows into many hash partitions


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    """torch opens the device before the first coarse context does"""
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


def _engine(r):
    from xmap.engine import device          # raises if libxmap_hip.so is missing: no CPU fallback
    ptr, item, rating, time = [np.array(a) for a in (r.user_ptr, r.item, r.rating, r.time)]       # (writable copies for torch)
    return device.Engine(device.DeviceRatings(ptr, item, rating, time, r.n_items, r.item_attrs(), "cuda:0", rating64=True))


@functools.lru_cache(maxsize=2)
def engine(kind, name, cap=CAP):
    return _engine(rs.value_family(name, cap) if kind == "value" else rs.layout_family(name))


def sorted_rec(S, I):
    """a rec_sim result of the engine in (row, column) order: rows, col, sim, ls, nij, row_ptr, norm"""
    row_ptr = S.row_ptr.cpu().numpy()
    rows = np.repeat(np.arange(I, dtype=np.int64), np.diff(row_ptr))
    col = S.col.cpu().numpy().astype(np.int64)
    o = np.lexsort((col, rows))
    return rows[o], col[o], S.sim.cpu().numpy()[o], S.ls.cpu().numpy()[o], S.nij.cpu().numpy()[o], row_ptr, S.norm.cpu().numpy()[:I]


def check_rec(got, O):
    """a sorted result against the oracle's, whole"""
    rows, col, sim, ls, nij, row_ptr, norm = got
    assert np.array_equal(row_ptr, O.row_ptr)
    assert np.array_equal(rows, O.rows) and np.array_equal(col, O.col) and np.array_equal(nij, O.nij)
    assert same_doubles(sim, O.sim) and same_doubles(ls, O.ls) and same_doubles(norm, O.norm)


def check_statement_rows(got, r, norms, cap, which):
    rows, col, sim, ls, nij, row_ptr, norm = got
    assert np.array_equal(bits(norm), bits(norms)) or same_doubles(norm, norms)
    for i in which:
        assert same_row(rs.row_of(row_ptr, col, sim, ls, nij, i), rs.rec_row_statement(r.user_ptr, r.item, r.rating, norms, i, cap)), i


def check_symmetry(got, I):
    """(a, b) and (b, a) carry the same bits"""
    rows, col, sim, ls, nij = got[:5]
    o1, o2 = np.argsort(rows * I + col, kind="stable"), np.argsort(col * I + rows, kind="stable")
    assert np.array_equal(rows[o1], col[o2]) and np.array_equal(col[o1], rows[o2]) and np.array_equal(nij[o1], nij[o2])
    assert same_doubles(sim[o1], sim[o2]) and same_doubles(ls[o1], ls[o2])


def run(eng, r, cap, target):
    S = eng.rec_sim(cap, slot_target=target)
    assert S.layout.slot_target == target              # (no table overflowed)
    P = check_plan(S, r, r.n_users + 2, dups=True)
    assert P.n_heavy == 0
    return S, P


# ------------------------------------------------------------------------------------------------------ value families
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", VALUE_FAMILIES)
def test_value_family(name, cap):
    r, O, norms = rs.value_family(name, cap), rs.oracle_value(name, cap), rs.norms_of("value", name, cap)
    eng = engine("value", name, cap)
    for target in TARGETS:
        S, P = run(eng, r, cap, target)
        got = sorted_rec(S, r.n_items)
        check_rec(got, O)
        check_statement_rows(got, r, norms, cap, range(r.n_items))
        check_symmetry(got, r.n_items)
    if name == "slot_chains":              # the designed row sums its seventeen partners in one 128-slot table at either target
        assert P.cls[0] == 1 and P.Q[0] == 1 and P.bound[0] == 17


# ----------------------------------------------------------------------------------------------------- layout families
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("name", LAYOUT_FAMILIES)
def test_layout_family(name, target):
    r, O, norms = rs.layout_family(name), rs.oracle_layout(name), rs.norms_of("layout", name)
    S, P = run(engine("layout", name), r, CAP, target)
    want = rs.rec_plan(name, target)
    assert np.array_equal(P.cls, want.cls) and np.array_equal(P.Q, want.Q) and P.units.tolist() == want.units.tolist()
    got = sorted_rec(S, r.n_items)
    check_rec(got, O)
    check_statement_rows(got, r, norms, CAP, rs.chosen_rows(name))
    if len(O.col) < 1 << 20:
        check_symmetry(got, r.n_items)


def test_table_overflow_halves_the_slot_target():
    """overflowing+fp64 holds a row of exactly 2 048 partners: two partitions at slot target 1024, one of which meets more
    partners than its table has slots.  k_pair_tri raises the flag before its finalisation in LDS, the engine plans again with
    half the target: the result is the oracle's and that of a direct run at the final target -- nothing of the abandoned
    pass (s_ls, the doubled counts) survives"""
    from test_cpu_stage_a_layout import overflowing
    name = "overflowing+fp64"
    r, O, lone = rs.layout_family(name), rs.oracle_layout(name), overflowing()[1]
    eng = engine("layout", name)
    S = eng.rec_sim(CAP, slot_target=1024)
    final = S.layout.slot_target
    assert final in (512, 256, 128, 64, 32)
    P = check_plan(S, r, r.n_users + 2, dups=True)
    assert P.bound[lone] == 2048 and P.Q[lone] == 2048 // final
    got = sorted_rec(S, r.n_items)
    check_rec(got, O)
    D = eng.rec_sim(CAP, slot_target=final)
    assert D.layout.slot_target == final
    for x, y in zip(got, sorted_rec(D, r.n_items)):
        assert x.tobytes() == y.tobytes()


def test_two_runs_give_the_same_bytes():
    """wide_many+fp64: 47 class-4 rows -- 16 waves raise the maxima of one table in an order that differs from run to run"""
    name = "wide_many+fp64"
    r, eng = rs.layout_family(name), engine("layout", name)
    for target in TARGETS:
        a = sorted_rec(eng.rec_sim(CAP, slot_target=target), r.n_items)
        b = sorted_rec(eng.rec_sim(CAP, slot_target=target), r.n_items)
        assert len(a[0]) > 0
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("kind,name", [("value", "self_pairs"), ("layout", "wide_self"), ("layout", "wide_repeat")])
def test_round2_sequence_on_self_pairs(kind, name, monkeypatch):
    """the cursor-atomic mirror around the same pair kernels: a row paired with itself is one entry (k_scatter: j == i), with
    the local sensitivity as a sixth column"""
    monkeypatch.setenv("XMAP_A_V2", "1")
    r = rs.value_family(name, CAP) if kind == "value" else rs.layout_family(name)
    O = rs.oracle_value(name, CAP) if kind == "value" else rs.oracle_layout(name)
    for target in TARGETS:
        S, P = run(engine(kind, name), r, CAP, target)
        got = sorted_rec(S, r.n_items)
        check_rec(got, O)
        assert int((got[0] == got[1]).sum()) == int((rs.unordered_self_pairs(r) > 0).sum()) > 0


# ------------------------------------------------------------------------------------------------- coarse ABI, NumPy only
def _coarse_profiles(T, I):
    return rs.Input(T["ptr"], T["item"], T["rating"], I)


def _check_coarse(T, r, I, cap):
    """what xmap_ctx_rec_download gave against the oracle on the profiles xmap_ctx_rec_profiles_download gave"""
    O = rs.oracle_rec(r, cap)
    rows = np.repeat(np.arange(I, dtype=np.int64), np.diff(T["row_ptr"]))
    o = np.lexsort((T["col"], rows))
    got = (rows[o], T["col"][o].astype(np.int64), T["sim"][o], T["ls"][o], T["nij"][o], T["row_ptr"], T["norm"])
    check_rec(got, O)
    return got, O


def test_value_family_through_the_coarse_abi():
    """cap_edges as a foreign host uploads it: float32 ratings, every item a target item, so every rating passes through stage
    C into the profiles RecommenderSim runs over"""
    from test_gpu_coarse_abi import Ctx
    from test_gpu_tail import generate, rec_sim
    src = rs.value_family("cap_edges", CAP)
    r32 = rs.Input(src.user_ptr, src.item, src.rating.astype(np.float32), src.n_items)
    assert np.any(r32.rating != src.rating)
    ctx = Ctx()
    try:
        rows = generate(ctx, r32)
        assert len(rows["user"]) == rows["n_target_rows"] == r32.nnz
        T = rec_sim(ctx, r32.n_items, r32.n_users, r32.nnz, cap=CAP)
    finally:
        ctx.close()
    got_r = _coarse_profiles(T, r32.n_items)
    assert np.array_equal(got_r.user_ptr, r32.user_ptr)
    users = np.repeat(np.arange(r32.n_users), np.diff(r32.user_ptr))
    o1, o2 = np.lexsort((got_r.item, users)), np.lexsort((r32.item, users))
    assert np.array_equal(got_r.item[o1], r32.item[o2]) and np.array_equal(bits(got_r.rating[o1]), bits(r32.rating[o2]))
    got, O = _check_coarse(T, got_r, r32.n_items, CAP)
    assert set(O.nij.tolist()) == set(src.meta["targets"])
    norms = rs.rec_norms_statement(got_r.item, got_r.rating, got_r.n_items)
    check_statement_rows(got, got_r, norms, CAP, range(r32.n_items))


def test_wide_repeat_through_the_coarse_abi():
    """two contexts hold the two halves of wide_repeat (the same profiles, other ratings); their union without
    XMAP_UNION_DISTINCT gives every user every item twice: the class-4 rows whose every rater holds the row's item twice"""
    from test_gpu_coarse_abi import Ctx
    from test_gpu_tail import generate, rec_sim
    from test_gpu_union import _union
    ptr, item, ra, rb, (H0, H1) = rs.repeat_parts()
    I, U = int(item.max()) + 1, len(ptr) - 1
    parts = [rs.Input(ptr, item, x.astype(np.float32), I) for x in (ra, rb)]
    srcs, dst = [Ctx(), Ctx()], Ctx()
    try:
        for c, p in zip(srcs, parts):
            rows = generate(c, p)
            assert len(rows["user"]) == rows["n_target_rows"] == p.nnz
        ident_u, ident_i = np.arange(U, dtype=np.int32), np.arange(I, dtype=np.int32)
        rc, counts = _union(dst, srcs, [ident_u, ident_u], [ident_i, ident_i], U, I, 0)
        assert rc == 0 and counts[0] == 2 * len(item)
        T = rec_sim(dst, I, U, counts[0], cap=CAP)
    finally:
        for c in srcs + [dst]:
            c.close()
    r = _coarse_profiles(T, I)
    assert np.array_equal(r.user_ptr, 2 * ptr)
    users = np.repeat(np.arange(U), np.diff(r.user_ptr))
    for h, raters in ((H0, rs.REPEAT_HUBS[0]), (H1, rs.REPEAT_HUBS[1])):
        u, k = np.unique(users[r.item == h], return_counts=True)
        assert len(u) == raters >= 2048 and np.all(k == 2)
    P = plan_statement(r.user_ptr, r.item, I, U + 2, 768, dups=True)
    assert np.nonzero(P.cls == 4)[0].tolist() == [H0, H1] and P.n_heavy == 0
    got, O = _check_coarse(T, r, I, CAP)
    assert O.nij[(O.rows == H0) & (O.col == H0)].tolist() == [2 * rs.REPEAT_HUBS[0]]
    norms = rs.rec_norms_statement(r.item, r.rating, I)
    check_statement_rows(got, r, norms, CAP, [H0, H1, 0, 1, 2])
