"""Stage B on caller-fed similarity matrices over the whole fp64 range (run on the MI355X: `pytest -m gpu`): the families of
tests/test_cpu_fed_sim.py -- in-range values with signed zeros, thousands of exact |sim| ties, subnormals, 2^700, everything
mixed -- uploaded with Engine.sim_from_host and compared with the CPU oracle on the same arrays (xo.sim_from_arrays), every
table and every X-Sim with array_equal and no tolerance.  The oracle divides a path's sums with the IEEE `/` and adds in
double-double, so for `in` and `ties` this is the comparison of k_paths4<true>'s bare division (div_mid) with `/` over the
range xmap_edge_ranges admits, and for the other families the proof that the range check sends them to k_paths4<false>.
"""
import ctypes as C

import numpy as np
import pytest

from golden_util import METHODS, csr_to_pairs
from test_cpu_fed_sim import FAMILIES, fast_div_ok, fed_case, listed_values
from test_gpu_parity import _ext_bytes, _xsim_lists

pytestmark = pytest.mark.gpu

CASES = [(f, m) for f in FAMILIES for m in METHODS]


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device  # raises if libxmap_hip.so is missing: no CPU fallback
    return device


@pytest.fixture(scope="module")
def eng(dev):
    """one upload of the ratings for the whole module (both methods keep pairs of the same input)"""
    r = fed_case("in", METHODS[0]).r
    return dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))


def _upload(eng, c, frac=None):
    """(copies: the shared arrays are read-only, which torch.from_numpy warns about)"""
    return eng.sim_from_host(*[a.copy() for a in (c.row_ptr, c.col, c.sim, c.mutu, c.nij, c.info)], frac=frac)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_ext(c, E, what):
    """the knn tables, the path count and the X-Sim lists of one extension against the oracle's, as
    test_gpu_parity._check_all_stages compares them (plus the three value columns of the lists, bit for bit: they are copies
    of the caller's values, the sign of a zero included)"""
    I, k, Xo = c.I, c.k, c.Xo
    assert np.array_equal(E.bb.cpu().numpy()[:I], Xo.bb), what
    assert np.array_equal(E.cls.cpu().numpy()[:I], Xo.cls), what
    assert np.array_equal(E.kcnt.cpu().numpy()[:I], Xo.cnt), what
    held = np.arange(k)[None, None, :] < Xo.cnt[:, :, None]
    assert np.array_equal(E.kcol.cpu().numpy()[:I][held], Xo.col[held]), what
    assert np.array_equal(_bits(E.kval.cpu().numpy()[:I][held]), _bits(Xo.val[held])), what
    assert E.n_paths == Xo.n_paths, what
    st, en, va = _xsim_lists(E, I)
    ost, oen = csr_to_pairs(Xo.xs_ptr, Xo.xs_end)
    assert np.array_equal(st, ost) and np.array_equal(en, oen), what
    differ = int((va != Xo.xs_val).sum())
    print("%s %s %s: %d of %d X-Sim values differ from the oracle's" % (c.family, c.method, what, differ, len(va)))
    assert np.array_equal(va, Xo.xs_val), what


def _check_select(c, eng, E, what, rows=False):
    """the private selection (it reads the fused top-10: select_topc's order on ties and zeros) and the AlterEgo rows"""
    I = c.I
    n_top, choice, mp = eng.select(E, True)
    assert np.array_equal(n_top.cpu().numpy()[:I], c.n_top), what
    assert np.array_equal(choice.cpu().numpy()[:I], c.choice), what
    assert np.array_equal(mp.cpu().numpy()[:I], c.map), what
    if rows:
        G, ae = eng.alterego(mp), c.ae
        assert np.array_equal(G.user.cpu().numpy(), ae["user"]) and np.array_equal(G.item.cpu().numpy(), ae["item"]), what
        assert np.array_equal(G.rating.cpu().numpy(), ae["rating"]) and np.array_equal(G.time.cpu().numpy(), ae["time"]), what
        assert eng.n_profiles(G) == ae["n_profiles"], what


def _same_bytes(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


# the formulations of the enumeration: k_paths4 (one accumulator row per start), its heavy starts over dedicated rows
# (k_merge_groups / k_merge), one accumulate per path, and the tile-major form of the cross-check library
FORMS = [("cols", {}), ("heavy", dict(chunk=64, n_slots=64)), ("enum", dict(algo="enum")), ("mid", dict(algo="mid"))]


@pytest.mark.parametrize("family,method", CASES)
def test_fed_matrix_vs_oracle(dev, eng, family, method, monkeypatch):
    monkeypatch.delenv("XMAP_SLOW_DIV", raising=False)
    c = fed_case(family, method)
    S = _upload(eng, c)
    first = None
    for name, kw in FORMS:
        E = eng.extend(S, c.k, full=True, **kw)
        assert E.fast_div == c.fast, name            # the range check's answer (FAMILIES)
        if name == "heavy":
            assert E.units.n_heavy > 0
        _check_ext(c, E, name)
        _check_select(c, eng, E, name, rows=first is None)
        if first is None:
            first = _ext_bytes(E, c.I)
        else:
            _same_bytes(_ext_bytes(E, c.I), first, name)          # (n_cand and the fused top-10 as well)
    if c.fast:
        # div_mid against `/` over the admitted range: k_paths4<false> on the same tables gives the same bytes
        monkeypatch.setenv("XMAP_SLOW_DIV", "1")
        for name, kw in FORMS[:2]:
            E = eng.extend(S, c.k, full=True, **kw)
            assert E.fast_div == 1
            _check_ext(c, E, "slow_div " + name)
            _same_bytes(_ext_bytes(E, c.I), first, "slow_div " + name)


@pytest.mark.parametrize("family,method", CASES)
def test_host_twin_of_the_range_check(dev, eng, family, method, monkeypatch):
    """Engine.ext_tables_from_knn decides fast / slow in NumPy from the listed pairs; xmap_edge_ranges on the device from
    every kept pair.  Where the pairs that decide the answer are listed (checked on the oracle's tables) the two agree, and
    the tables built on the host from the GPU's own lists give the extension's bytes."""
    monkeypatch.delenv("XMAP_SLOW_DIV", raising=False)
    c = fed_case(family, method)
    assert fast_div_ok(*listed_values(c.Xo.cnt, c.Xo.val)) == fast_div_ok(c.sim, c.mutu) == c.fast
    E = eng.extend(_upload(eng, c), c.k, full=True)
    assert E.fast_div == c.fast
    want = _ext_bytes(E, c.I)
    tables = [t.cpu().numpy()[:c.I] for t in (E.cls, E.kcnt, E.kcol, E.kval)]
    E2 = eng.ext_tables_from_knn(c.k, *tables)
    assert E2.fast_div == E.fast_div
    E2 = eng.extend_tables(E2, full=True)
    _check_ext(c, E2, "twin")
    _same_bytes(_ext_bytes(E2, c.I), want, "twin")


@pytest.mark.parametrize("method", METHODS)
def test_fed_fractions(dev, eng, method, monkeypatch):
    """frac_mutu handed over by the caller (sim_from_host(frac=)): generic records, so the checked division whatever the
    values -- and with the fractions the engine would have derived itself, the bytes of the run without them"""
    monkeypatch.delenv("XMAP_SLOW_DIV", raising=False)
    c = fed_case("in", method)
    derived = 1.0 * c.mutu.astype(np.float64) / (c.info[c.rows, 3] + c.info[c.col, 3] - c.nij.astype(np.float64))
    assert derived.max() > 1.0 and derived.min() > 0.0
    E0 = eng.extend(_upload(eng, c), c.k, full=True)
    E1 = eng.extend(_upload(eng, c, frac=derived), c.k, full=True)
    assert E0.fast_div == 1 and E1.fast_div == 0
    _check_ext(c, E1, "frac")
    _check_select(c, eng, E1, "frac")
    _same_bytes(_ext_bytes(E1, c.I), _ext_bytes(E0, c.I), "frac")


# ------------------------------------------------------------------------------------------------ the range check alone
N_RANGE = 513                      # three blocks of k_edge_ranges: 256 + 256 + 1
POSITIONS = (0, 255, 256, 512)     # first entry, both sides of a block edge, the one entry of the last block
BIG = (1 << 31) - 1
# (name, sim or None = keep, mutu or None = keep, the answer)
REPLACED = [
    ("product 2^-400", 2.0 ** -415, 1 << 15, 0),
    ("above 2^-400", float(np.nextafter(2.0 ** -400, 1.0)), 1, 1),
    ("product 2^400", 2.0 ** 385, 1 << 15, 0),
    ("below 2^400", float(np.nextafter(2.0 ** 400, 0.0)), 1, 1),
    ("+0.0", 0.0, None, 1),
    ("-0.0", -0.0, None, 1),
    ("smallest subnormal", 5e-324, 1, 0),
    ("nan", float("nan"), None, 0),
    ("+inf", float("inf"), None, 0),
    ("mutu 0", None, 0, 0),
    ("mutu -1", None, -1, 0),
    ("2^368 x (2^31 - 1)", 2.0 ** 368, BIG, 1),
    ("2^370 x (2^31 - 1)", 2.0 ** 370, BIG, 0),
]


def _edge_ranges(dev, eng, sim, mutu, frac=None):
    """xmap_edge_ranges on a sim_from_host matrix with these entries, in rows of 0, 1, 2, ... entries"""
    I, n = eng.R.n_items, len(sim)
    row_ptr = np.minimum(np.cumsum(np.arange(I + 1, dtype=np.int64) % 7), n)
    row_ptr[-1] = n
    assert row_ptr[-2] <= n and np.all(np.diff(row_ptr) >= 0)
    S = eng.sim_from_host(row_ptr, np.zeros(n, np.int32), sim, mutu, np.zeros(n, np.int32), np.zeros((I, 4)), frac=frac)
    ok = C.c_int32(-1)
    dev.check(dev.lib.xmap_edge_ranges(dev._stream(eng.dev), C.byref(S.c), C.byref(ok)))
    return int(ok.value)


@pytest.mark.parametrize("name,sim_v,mutu_v,answer", REPLACED, ids=[r[0] for r in REPLACED])
def test_range_check_one_entry(dev, eng, name, sim_v, mutu_v, answer):
    """513 in-range entries, exactly one replaced -- at the first position, on both sides of a block edge and in the last
    block's single thread: the kernel's answer is the NumPy statement of the predicate (which gives the expected table)"""
    c = fed_case("in", "adjust_cosine")
    base_sim, base_mutu = c.sim[:N_RANGE].copy(), c.mutu[:N_RANGE].copy()
    assert fast_div_ok(base_sim, base_mutu) == 1 and (base_sim[list(POSITIONS)] != 0.0).all()
    assert _edge_ranges(dev, eng, base_sim, base_mutu) == 1
    for pos in POSITIONS:
        sim, mutu = base_sim.copy(), base_mutu.copy()
        if sim_v is not None:
            sim[pos] = sim_v
        if mutu_v is not None:
            mutu[pos] = mutu_v
        want = fast_div_ok(sim, mutu)
        assert want == answer, (name, pos)
        assert _edge_ranges(dev, eng, sim, mutu) == want, (name, pos)


def test_range_check_without_values(dev, eng):
    """no kept pairs: nothing to refuse; fractions supplied by the caller: the checked division whatever the values"""
    c = fed_case("in", "adjust_cosine")
    assert _edge_ranges(dev, eng, np.zeros(0), np.zeros(0, np.int32)) == 1
    sim, mutu = c.sim[:N_RANGE].copy(), c.mutu[:N_RANGE].copy()
    assert _edge_ranges(dev, eng, sim, mutu) == 1
    assert _edge_ranges(dev, eng, sim, mutu, frac=np.full(N_RANGE, 0.5)) == 0
