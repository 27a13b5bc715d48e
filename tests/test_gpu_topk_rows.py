"""The designed rows of tests/test_cpu_topk_rows.py on the MI355X (`pytest -m gpu`): rows whose lengths sit on the structural
edges of k_knn_classify, value families with thousands of |sim| ties at the k-th place, and five storage orders inside every
row -- among them the exact reverse of the sorted order, which fills the stream's survivor buffer within a window.

  1  the knn tables of every family x order x k against the CPU oracle and a NumPy statement, bit for bit
  2  the contract of xmap_knn_classify on tables that come uninitialised: every entry of the rows given, nothing else
  3  xmap_knn_thresholds against NumPy
  4  the reverse adjacencies (k_reverse, k_reverse_long: membership from the k-th entry alone) against
     Engine.ext_tables_from_knn, which builds them in NumPy from the lists alone

What a subtly wrong kernel would do here: `before()` without its column tie-break leaves the order inside a |sim| tie to the
bitonic network, i.e. to the storage order -- for `one` every list is cut inside a tie, and under `col_desc` the lists then
hold other columns than under `col_asc`; `a <= th.col` written `a < th.col` in in_list drops the last listed neighbour of
every FULL list from the reverse lists (at k = 3 that is 10 000 full lists A of non-bridge items: the attach pointers differ).
No path is enumerated in this file: a joint pair of 6 000-entry attach lists is more than 10^8 paths.
"""
import ctypes as C

import numpy as np
import pytest

from test_cpu_topk_rows import (BIG_K_FAMILIES, CASES, FAMILIES, K_MAX, ORDERS, bits, held, numpy_tables, oracle_tables,
                                stored, structure, thresholds)

pytestmark = pytest.mark.gpu

PATTERN = 0xA5
REV_FAMILIES = ("one", "levels4", "zeros")


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import device  # raises if libxmap_hip.so is missing: no CPU fallback
    return device


@pytest.fixture(scope="module")
def eng(dev):
    """one upload of the item space for the whole module"""
    r = structure().r
    return dev.Engine(dev.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs()))


def _upload(eng, family, order):
    return eng.sim_from_host(*stored(family, order))


def _on_device(eng, ref):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(eng.dev) for a in ref]


def _same_tables(E, I, k, ref, what):
    """bb, cls, kcnt and the held part of kcol and kval (bits: zero signs included) of E against device copies of reference
    tables (bb, cls, cnt, col, val); the comparison runs on the device (at k = 512 a set of tables is 0.4 GB)"""
    import torch
    bb, cls, cnt, col, val = ref
    assert torch.equal(E.bb[:I], bb), what
    assert torch.equal(E.cls[:I], cls), what
    assert torch.equal(E.kcnt[:I], cnt), what
    h = torch.arange(k, device=cnt.device)[None, None, :] < cnt[:, :, None]
    assert bool(((E.kcol[:I] == col) | ~h).all()), what
    assert bool(((E.kval[:I].view(torch.int64) == val.view(torch.int64)) | ~h[..., None]).all()), what


# ------------------------------------------------------------------------------------------------------ 1: knn tables
@pytest.mark.parametrize("family,k", CASES)
def test_knn_tables_designed_rows(dev, eng, family, k):
    """every storage order of one family and k: the oracle's tables and the NumPy statement's (k = 512, the largest k
    admitted, on `levels4` and `one` only: the host holds two sets of tables of 0.4 GB each)"""
    assert k < K_MAX or family in BIG_K_FAMILIES
    I = structure().I
    X = oracle_tables(family, k)
    ref_o = _on_device(eng, (X.bb, X.cls, X.cnt, X.col, X.val))
    ref_n = _on_device(eng, numpy_tables(family, k)[:5])
    del X
    for order in ORDERS:
        E = eng.knn(_upload(eng, family, order), k)
        _same_tables(E, I, k, ref_o, (order, "oracle"))
        _same_tables(E, I, k, ref_n, (order, "numpy"))


def test_knn_refuses_a_k_past_the_chunk(dev, eng):
    """2 k entries are carried from chunk to chunk and have to leave half a chunk free: k = 513 is ERR_ARG, nothing runs
    (the tables are sized for it all the same)"""
    import torch
    from xmap.engine import hipabi as abi
    I, k = structure().I, K_MAX + 1
    S = _upload(eng, "one", "col_asc")
    R = eng.R
    bb = eng.bridge_flags(S)
    cls = torch.zeros(I, dtype=torch.uint8, device=eng.dev)
    kcnt = torch.zeros((I, 2), dtype=torch.int32, device=eng.dev)
    kcol = torch.zeros((I, 2, k), dtype=torch.int32, device=eng.dev)
    kval = torch.zeros((I, 2, k, 3), dtype=torch.float64, device=eng.dev)
    st = dev._stream(eng.dev)
    args = lambda kk: (st, C.byref(S.c), kk, abi.vp(bb), abi.vp(R.suffix_cls), abi.vp(R.contains_mask), abi.vp(cls), abi.vp(kcnt),
                       abi.vp(kcol), abi.vp(kval), abi.i32(0), abi.i32(I))
    assert abi.lib.xmap_knn_classify(*args(k)) == abi.ERR_ARG
    assert abi.lib.xmap_knn_classify(*args(0)) == abi.ERR_ARG
    torch.cuda.synchronize()
    assert not bool(kcnt.any()) and not bool(kcol.any())


# ------------------------------------------------------------------------------------------- 2: tail and range contract
def _pattern_tables(eng, I, k):
    import torch
    raw = lambda n: torch.full((n,), PATTERN, dtype=torch.uint8, device=eng.dev)
    return (raw(I), raw(I * 2 * 4).view(torch.int32).view(I, 2), raw(I * 2 * k * 4).view(torch.int32).view(I, 2, k),
            raw(I * 2 * k * 3 * 8).view(torch.float64).view(I, 2, k, 3))


@pytest.mark.parametrize("k", [3, 65])          # (both instance layouts: 8 KB + 32 KB, and every row on the 32 KB one)
def test_knn_writes_its_rows_and_nothing_else(dev, eng, k):
    """Engine.knn allocates the tables with torch.empty: xmap_knn_classify writes every entry of the rows [row_lo, row_hi)
    -- the tail of a listed row as zeros, rows without entries too -- and not a byte of any other row.  The tables are
    filled with 0xA5 before the call.  "Written" is checked per element (a class, a count, a column, a double), not per
    byte: column 165 is a legitimate value with a pattern byte in it, no legitimate element is all pattern bytes."""
    import torch
    from xmap.engine import hipabi as abi
    c = structure()
    I = c.I
    S = _upload(eng, "levels4", "shuffle")
    R = eng.R
    bb = eng.bridge_flags(S)
    ref = _on_device(eng, numpy_tables("levels4", k)[:5])
    st = dev._stream(eng.dev)
    n = np.diff(c.row_ptr)
    # the sub-range starts at one designed row and ends just before another: hubs inside and outside, long ones on both sides
    lo, hi = c.hub["sb"][5121], c.hub["tb"][6200]
    inside = [i for kind in c.hub for i in c.hub[kind].values() if lo <= i < hi]
    assert 0 < lo < hi < I and 20 < len(inside) < 3 * 29 - 20
    assert int((n[lo:hi] > 2048).sum()) >= 5 and int((n[:lo] > 2048).sum()) >= 2 and int((n[hi:] > 2048).sum()) >= 1
    assert int((n[lo:hi] == 0).sum()) >= 1 and n[lo] == 5121
    p32 = int(np.array([PATTERN] * 4, np.uint8).view(np.int32)[0])
    p64 = int(np.array([PATTERN] * 8, np.uint8).view(np.int64)[0])
    for row_lo, row_hi in ((0, I), (lo, hi)):
        cls, kcnt, kcol, kval = _pattern_tables(eng, I, k)
        abi.check(abi.lib.xmap_knn_classify(st, C.byref(S.c), k, abi.vp(bb), abi.vp(R.suffix_cls), abi.vp(R.contains_mask),
                                            abi.vp(cls), abi.vp(kcnt), abi.vp(kcol), abi.vp(kval), abi.i32(row_lo), abi.i32(row_hi)))
        torch.cuda.synchronize()
        what = (row_lo, row_hi)
        # outside the range: every byte is still the pattern
        for t in (cls, kcnt, kcol, kval):
            b = t.view(I, -1).view(torch.uint8)
            assert bool((b[:row_lo] == PATTERN).all()) and bool((b[row_hi:] == PATTERN).all()), what
        # inside: no element is left unwritten
        rows = slice(row_lo, row_hi)
        assert not bool((cls[rows] == PATTERN).any()), what
        assert not bool((kcnt[rows] == p32).any()) and not bool((kcol[rows] == p32).any()), what
        assert not bool((kval[rows].view(torch.int64) == p64).any()), what
        # the rows are the reference's, and behind the count of a listed row everything is 0 / +0.0
        assert torch.equal(cls[rows], ref[1][rows]) and torch.equal(kcnt[rows], ref[2][rows]), what
        h = torch.arange(k, device=eng.dev)[None, None, :] < kcnt[rows][:, :, None]
        assert bool(((kcol[rows] == ref[3][rows]) | ~h).all()), what
        assert bool(((kval[rows].view(torch.int64) == ref[4][rows].view(torch.int64)) | ~h[..., None]).all()), what
        listed = (cls[rows] != 0)[:, None, None]
        tail = ~h & listed
        assert int(tail.sum()) > 1000 and int((~listed).sum()) > 10
        assert not bool((kcol[rows] != 0)[tail].any()), what
        assert not bool((kval[rows].view(torch.int64) != 0)[tail[..., None].expand(-1, -1, -1, 3)].any()), what


# --------------------------------------------------------------------------------------------------------- 3: thresholds
@pytest.mark.parametrize("k", [1, 3, 50, 65])
@pytest.mark.parametrize("family", FAMILIES)
def test_knn_thresholds(dev, eng, family, k):
    """xmap_knn_thresholds: (|value| of the last entry, its column, the count) of both lists of every row, zeros for an
    empty list"""
    I = structure().I
    E = eng.knn(_upload(eng, family, "shuffle"), k)
    eng.ext_thresholds(E)
    rec = E.thr.cpu().numpy()[:4 * I].view(np.dtype([("la", "<f8"), ("col", "<i4"), ("cnt", "<i4")])).reshape(I, 2)
    _, _, cnt, col, val, _ = numpy_tables(family, k)
    w_cnt, w_la, w_col = thresholds(cnt, col, val)
    assert np.array_equal(rec["cnt"], w_cnt)
    assert np.array_equal(bits(rec["la"]), bits(w_la))
    assert np.array_equal(rec["col"], w_col)
    assert int((w_cnt == k).sum()) > 50 and int((w_cnt == 0).sum()) > 100          # full lists, empty lists


# ------------------------------------------------------------------------------------------------ 4: reverse adjacencies
def _sorted_lists(out, I):
    """(ptr, idx, val bits, flag) of one reverse adjacency with the entries of every row sorted by idx"""
    ptr, idx, val, flag, n = out
    ptr = ptr.cpu().numpy()[:I + 1]
    assert int(ptr[-1]) == n
    idx, val, flag = idx.cpu().numpy()[:n], val.cpu().numpy()[:n], flag.cpu().numpy()[:n]
    rows = np.repeat(np.arange(I), np.diff(ptr))
    o = np.lexsort((idx, rows))
    assert len(np.unique(rows * I + idx)) == n          # an item is listed once per row: the order by idx is total
    return ptr, idx[o], bits(val[o]), flag[o]


def _check_reverse(eng, family, k, orders, n_long):
    """ext_reverse of the device's own knn tables against the host twin on the oracle's tables: pointers equal, and per row
    the same set of (idx, three values bit for bit, flag) -- the device lists follow storage order, the twin's list order"""
    c = structure()
    I = c.I
    X = oracle_tables(family, k)
    twin = eng.ext_tables_from_knn(k, X.cls, X.cnt, X.col, X.val)
    want = {name: _sorted_lists(getattr(twin, name), I) for name in ("att", "rnn", "src")}
    n = np.diff(c.row_ptr)
    long_rows = np.nonzero(n > 4096)[0]
    for name in ("att", "rnn"):
        per_row = np.diff(want[name][0])[long_rows]
        assert np.all(per_row[(X.bb[long_rows] != 0) | (name == "rnn")] >= 1000)      # the long rows' lists are long (CPU census)
    assert len(want["src"][1]) >= 50 and int(want["src"][3].sum()) >= 30
    for order in orders:
        S = _upload(eng, family, order)
        E = eng.ext_reverse(S, eng.knn(S, k))
        assert int(E.long_rows[0].item()) == n_long, order          # rows that went to k_reverse_long
        for name in ("att", "rnn", "src"):
            got = _sorted_lists(getattr(E, name), I)
            for g, w, part in zip(got, want[name], ("ptr", "idx", "val", "flag")):
                assert np.array_equal(g, w), (order, name, part)


@pytest.mark.parametrize("rev_long", [None, 8], ids=["default", "long8"])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("family", REV_FAMILIES)
def test_reverse_lists_vs_host_twin(dev, eng, family, k, rev_long, monkeypatch):
    """at the default XMAP_REV_LONG the nine rows above 4 096 entries go to k_reverse_long, with XMAP_REV_LONG=8 every row
    above 8 entries does: the threshold's tie rule on long rows, in both kernels"""
    monkeypatch.delenv("XMAP_REV_SEPARATE", raising=False)
    if rev_long is None:
        monkeypatch.delenv("XMAP_REV_LONG", raising=False)
    else:
        monkeypatch.setenv("XMAP_REV_LONG", str(rev_long))
    n = np.diff(structure().row_ptr)
    n_long = int((n > (4096 if rev_long is None else rev_long)).sum())
    assert n_long == 9 if rev_long is None else n_long > 1000
    _check_reverse(eng, family, k, ORDERS, n_long)


def test_reverse_lists_separate_counts(dev, eng, monkeypatch):
    """XMAP_REV_SEPARATE=1: the attach and rnn lists counted in a pass each instead of the fused one"""
    monkeypatch.delenv("XMAP_REV_LONG", raising=False)
    monkeypatch.setenv("XMAP_REV_SEPARATE", "1")
    _check_reverse(eng, "levels4", 3, ORDERS, 9)
