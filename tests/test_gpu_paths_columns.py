"""k_paths4 on designed tables (run on the MI355X: `pytest -m gpu`): the families of tests/paths_families.py -- every width class
of a column, every record-count class of a visit, every head-count class of a start, later batches, heavy starts on both
sides of MERGE_GROUP with and without column ranges -- uploaded with Engine.sim_from_host and run in every formulation of the
enumeration.  Each run is compared with the CPU oracle on the same arrays as tests/test_gpu_fed_sim.py compares (knn tables,
n_paths, the full X-Sim lists, the fused top-10 and the private selection, as bit patterns, no tolerance), and the structures
the kernel reads and the counters it leaves are compared, element for element, with the independent statement of
tests/paths_statement.py: the tile directory, n_paths, n_updates, the per-start path counts and the work units;
xmap_path_plan is called directly on the designed path counts of tests/test_cpu_paths_columns.py.  That the families reach the
classes they are written for, and that the statement agrees with the per-path oracle, is proven without a GPU in
tests/test_cpu_paths_columns.py.
"""
import ctypes as C

import numpy as np
import pytest

from paths_families import BUILDERS, HEAVY, family_case
from paths_statement import plan_statement
from test_cpu_paths_columns import PLANS
from test_gpu_fed_sim import _check_ext, _check_select, _same_bytes
from test_gpu_parity import _ext_bytes

pytestmark = pytest.mark.gpu

FAMILIES = list(BUILDERS)
BIG = 1 << 40       # a row budget no designed plan reaches


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device  # raises if libxmap_hip.so is missing: no CPU fallback
    return device


_UP = {}


def _uploaded(dev, name):
    """one engine and one upload per family for the whole module"""
    if name not in _UP:
        c = family_case(name)
        r = c.r
        eng = dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, c.attrs))
        S = eng.sim_from_host(*[a.copy() for a in (c.row_ptr, c.col, c.sim, c.mutu, c.nij, c.info)])
        _UP[name] = (c, eng, S)
    return _UP[name]


SLOTS = (1, 3, 64)


def forms(name):
    """the formulations a family runs in: (label, arguments of Engine.extend, n_slots to force or None).  Every heavy setting
    of the family at its written slot count, the family's last one at all of 1, 3 and 64 accumulator rows, and `cols` -- every
    start light -- once more through one row."""
    own = [(chunk, n_slots) for fam, chunk, n_slots, _, _ in HEAVY if fam == name] or [(64, 64)]
    runs = own + [(own[-1][0], n) for n in SLOTS if n != own[-1][1]]
    heavy = [("heavy-%d@%d" % (chunk, n), dict(chunk=chunk, n_slots=max(n, 4)), n if n < 4 else None) for chunk, n in runs]
    return [("cols", {}, None)] + heavy + [("cols@1", {}, 1), ("enum", dict(algo="enum"), None)]


def _extend(dev, monkeypatch, eng, S, c, kw, force):
    """Engine.extend; force = 1 or 3: the kernel's own slot count (xmap_path_rows.n_slots) below the four rows the engine
    always allocates -- every unit then goes through that many accumulator rows.  Engine._enumerate raises whatever it is
    asked for (the n_slots argument, XMAP_N_SLOTS) to at least 4 rows, so neither reaches 1 or 3; the kernel takes any count
    >= 1 (slots beyond it return at once), and the struct the engine hands it is the one place to say so."""
    with monkeypatch.context() as m:
        handed = []
        if force is not None:
            real = dev.abi.PathRows

            def rows(n_slots, *rest):
                handed.append(min(force, n_slots))
                return real(handed[-1], *rest)
            m.setattr(dev.abi, "PathRows", rows)
        E = eng.extend(S, c.k, full=True, start_range=c.start_range, **kw)
        assert force is None or handed == [force]
        return E


def _check_structure(c, E, label, kw):
    """what the kernel reads and counts against the statement"""
    St, I = c.St, c.I
    lo, hi = c.start_range or (0, I)
    assert E.n_paths == St.n_paths, label
    assert np.array_equal(E.n_cand.cpu().numpy()[:I], St.n_cand), label
    U = E.units
    assert np.array_equal(U.P.cpu().numpy()[:I], St.P), label                 # xmap_path_weights
    pl = plan_statement(St.P, lo, hi, kw.get("chunk", 0), 0 if "chunk" in kw else 8192, BIG)
    assert [U.n_units, U.n_heavy, U.n_rows, U.total, U.chunk] == pl["h_out"], label
    for name in ("unit_start", "unit_c", "unit_G", "unit_row"):
        assert np.array_equal(getattr(U, name).cpu().numpy()[:U.n_units], pl[name]), (label, name)
    assert np.array_equal(U.heavy_unit0.cpu().numpy()[:U.n_heavy], pl["heavy_unit0"]), label
    if kw.get("algo") == "enum":
        return
    assert E.n_updates == St.n_updates, label
    M = E.mid
    assert M.n_nb == len(St.nb) and np.array_equal(M.nb_list.cpu().numpy(), St.nb), label
    assert M.n_tiles == St.n_tiles and M.n_records == St.n_records, label
    assert np.array_equal(M.dir_ptr.cpu().numpy(), St.dir_ptr), label
    d64 = M.dir.cpu().numpy()[:3 * M.n_tiles].reshape(-1, 3)                  # MidDir: int x, ne, cnt, pad; long long off
    d32 = np.ascontiguousarray(d64).view(np.int32).reshape(-1, 6)
    assert np.array_equal(d32[:, 0], St.dir_x) and np.array_equal(d32[:, 1], St.dir_ne) and np.array_equal(d32[:, 2], St.dir_cnt), label
    assert np.array_equal(d32[:, 3], np.searchsorted(St.nb, St.dir_x)), label            # the column's index in nb_list
    assert np.array_equal(d64[:, 2], np.cumsum(St.dir_cnt) - St.dir_cnt), label          # records in directory order


@pytest.mark.parametrize("name", FAMILIES)
def test_family_vs_oracle_and_statement(dev, name, monkeypatch):
    monkeypatch.delenv("XMAP_SLOW_DIV", raising=False)
    monkeypatch.delenv("XMAP_N_SLOTS", raising=False)
    monkeypatch.delenv("XMAP_CHUNK_DIV", raising=False)
    c, eng, S = _uploaded(dev, name)
    first, n_updates = None, set()
    fs = forms(name)
    assert {f[2] or f[1].get("n_slots") for f in fs if f[0].startswith("heavy")} >= set(SLOTS)
    for label, kw, force in fs:
        E = _extend(dev, monkeypatch, eng, S, c, kw, force)
        assert E.fast_div == 1, label
        if label.startswith("heavy"):
            assert E.units.n_heavy > 0, label
        _check_ext(c, E, label)
        _check_select(c, eng, E, label)
        _check_structure(c, E, label, kw)
        if kw.get("algo") != "enum":
            n_updates.add(E.n_updates)
        if first is None:
            first = _ext_bytes(E, c.I)
        else:
            _same_bytes(_ext_bytes(E, c.I), first, label)
    # twice the same bytes
    E = _extend(dev, monkeypatch, eng, S, c, {}, None)
    _same_bytes(_ext_bytes(E, c.I), first, "cols again")
    assert n_updates == {E.n_updates}          # the same row updates whatever the unit plan and the rows
    # k_paths4<false>: the IEEE division on the same tables
    monkeypatch.setenv("XMAP_SLOW_DIV", "1")
    for label, kw, force in fs[:2]:
        E = _extend(dev, monkeypatch, eng, S, c, kw, force)
        assert E.fast_div == 1
        _check_ext(c, E, "slow_div " + label)
        _check_structure(c, E, "slow_div " + label, kw)
        _same_bytes(_ext_bytes(E, c.I), first, "slow_div " + label)


def _plan(dev, P, lo, hi, chunk, div, max_rows, cap_units, guard=3, fill=-7):
    """xmap_path_plan on a host array of path counts; the unit arrays are pre-filled and longer than cap_units"""
    import torch
    d = "cuda:0"
    I = len(P)
    Pd = torch.from_numpy(np.ascontiguousarray(P, np.int64)).to(d)
    arr = [torch.full((max(cap_units, 0) + guard,), fill, dtype=torch.int32, device=d) for _ in range(4)]
    h0 = torch.full((I + guard,), fill, dtype=torch.int32, device=d)
    h = (C.c_int64 * 5)(*([-1] * 5))
    rc = dev.lib.xmap_path_plan(dev._stream(torch.device(d)), dev.i32(I), dev.vp(Pd), dev.i32(lo), dev.i32(hi), dev.i64(chunk),
                                dev.i64(div), dev.i64(max_rows), dev.i64(cap_units), *[dev.vp(a) for a in arr], dev.vp(h0), h)
    torch.cuda.synchronize()
    return rc, [int(v) for v in h], [a.cpu().numpy() for a in arr], h0.cpu().numpy()


@pytest.mark.parametrize("plan", PLANS, ids=[p[0] for p in PLANS])
def test_path_plan_vs_statement(dev, plan):
    name, P, lo, hi, chunk, div, max_rows, _, _ = plan
    pl = plan_statement(P, lo, hi, chunk, div, max_rows)
    n_units, n_heavy = pl["h_out"][0], pl["h_out"][1]
    rc, h, arr, h0 = _plan(dev, P, lo, hi, chunk, div, max_rows, n_units)          # the arrays fit exactly
    assert rc == 0 and h == pl["h_out"]
    for got, key in zip(arr, ("unit_start", "unit_c", "unit_G", "unit_row")):
        assert np.array_equal(got[:n_units], pl[key]), key
        assert (got[n_units:] == -7).all(), key                                    # nothing written beyond the units
    assert np.array_equal(h0[:n_heavy], pl["heavy_unit0"]) and (h0[n_heavy:] == -7).all()
    if n_units > 0:       # one unit short: refused, the sizes reported all the same, nothing written
        rc, h, arr, h0 = _plan(dev, P, lo, hi, chunk, div, max_rows, n_units - 1)
        assert rc == dev.abi.ERR_CAPACITY and h == pl["h_out"]
        assert all((a == -7).all() for a in arr) and (h0 == -7).all()
