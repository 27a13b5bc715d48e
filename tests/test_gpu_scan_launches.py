"""The exclusive scans of csrc/util.hip against numpy.cumsum, exactly (int64 results).

Up to xmap_scan_self_tiles() tiles of 2048 values a scan is two launches: tile sums, then tile scans in which every block adds
up the tile sums in front of it.  Beyond that a one-block scan of the tile sums runs in between.  Both forms, the sizes around
one tile and around the switch, n = 0 and 1, all-zero input, INT32_MAX entries whose sum passes 2^32, the total read back by
the host or not -- for xmap_exclusive_scan_i32_to_i64, xmap_exclusive_scan_i64 and the two-array twin
xmap_exclusive_scan2_i32_to_i64 (with and without in_a + in_b as the first array)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 2048
INT32_MAX = 2 ** 31 - 1


def _lib():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    from xmap.engine import hipabi
    return hipabi.lib


def _sizes():
    t = _lib().xmap_scan_self_tiles()
    assert 256 <= t <= 8192            # "a few thousand": one strided loop of a block
    return [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, t * TILE - 1, t * TILE, t * TILE + 1, (t + 1) * TILE, (t + 3) * TILE + 5]


@functools.lru_cache(maxsize=None)
def _input(n, kind):
    """(a, b, exclusive scan of a, of b, of a + b), each scan with the total as entry n"""
    rng = np.random.default_rng(n * 7 + len(kind))
    if kind == "zero":
        a = np.zeros(n, np.int32)
        b = np.zeros(n, np.int32)
    elif kind == "max":
        a = np.full(n, INT32_MAX, np.int32)
        b = np.full(n, INT32_MAX, np.int32)
        b[::3] = 1
    else:
        a = rng.integers(0, 1000, n).astype(np.int32)
        b = rng.integers(0, 5, n).astype(np.int32)

    def ex(v):
        return np.concatenate([np.zeros(1, np.int64), np.cumsum(v.astype(np.int64))])
    out = (a, b, ex(a), ex(b), ex(a.astype(np.int64) + b.astype(np.int64)))
    for x in out:
        x.setflags(write=False)
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda() if len(a) else torch.zeros(0, dtype=torch.from_numpy(a).dtype, device="cuda")


def _scan1(a, want_total, wide=False):
    import torch
    from xmap.engine.hipabi import check, vp, i64
    lib = _lib()
    n = len(a)
    d_in = _dev(a.astype(np.int64) if wide else a)
    out = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    tot = C.c_int64(-1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = lib.xmap_exclusive_scan_i64 if wide else lib.xmap_exclusive_scan_i32_to_i64
    check(f(st, vp(d_in), vp(out), i64(n), C.byref(tot) if want_total else None))
    return out.cpu().numpy(), (int(tot.value) if want_total else None)


def _scan2(a, b, plus, want_total):
    import torch
    from xmap.engine.hipabi import check, vp, i64, i32
    lib = _lib()
    n = len(a)
    d_a, d_b = _dev(a), _dev(b)
    out_a = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    out_b = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    tot = (C.c_int64 * 2)(-1, -1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.xmap_exclusive_scan2_i32_to_i64(st, vp(d_a), vp(d_b), i32(plus), vp(out_a), vp(out_b), i64(n), tot if want_total else None))
    return out_a.cpu().numpy(), out_b.cpu().numpy(), ([int(tot[0]), int(tot[1])] if want_total else None)


def test_the_sizes_straddle_the_switch():
    t = _lib().xmap_scan_self_tiles()
    tiles = [(n + TILE - 1) // TILE for n in _sizes()]
    assert t in tiles and t + 1 in tiles and max(tiles) > t + 1 and 1 in tiles and 2 in tiles


@pytest.mark.parametrize("want_total", [False, True], ids=["device_total", "host_total"])
@pytest.mark.parametrize("kind", ["random", "zero"])
def test_scan_every_size(kind, want_total):
    for n in _sizes():
        a, _, ex_a, _, _ = _input(n, kind)
        out, tot = _scan1(a, want_total)
        assert np.array_equal(out, ex_a), n
        if want_total:
            assert tot == int(ex_a[n]), n


@pytest.mark.parametrize("want_total", [False, True], ids=["device_total", "host_total"])
def test_scan_int32_max_entries(want_total):
    t = _lib().xmap_scan_self_tiles()
    for n in (3, TILE + 1, t * TILE, (t + 1) * TILE):
        a, _, ex_a, _, _ = _input(n, "max")
        assert int(ex_a[n]) == n * INT32_MAX and int(ex_a[n]) > 2 ** 32
        out, tot = _scan1(a, want_total)
        assert np.array_equal(out, ex_a), n
        if want_total:
            assert tot == n * INT32_MAX


def test_scan_int64_input():
    t = _lib().xmap_scan_self_tiles()
    for n in (0, 1, TILE + 1, t * TILE, (t + 1) * TILE):
        a, _, ex_a, _, _ = _input(n, "random")
        out, tot = _scan1(a, True, wide=True)
        assert np.array_equal(out, ex_a) and tot == int(ex_a[n]), n


@pytest.mark.parametrize("want_total", [False, True], ids=["device_total", "host_total"])
@pytest.mark.parametrize("plus", [0, 1], ids=["a", "a_plus_b"])
@pytest.mark.parametrize("kind", ["random", "zero", "max"])
def test_two_arrays_in_one_pass(kind, plus, want_total):
    t = _lib().xmap_scan_self_tiles()
    sizes = _sizes() if kind == "random" else [0, 1, TILE, TILE + 1, t * TILE, (t + 1) * TILE]
    for n in sizes:
        a, b, ex_a, ex_b, ex_ab = _input(n, kind)
        out_a, out_b, tot = _scan2(a, b, plus, want_total)
        first = ex_ab if plus else ex_a
        assert np.array_equal(out_a, first), n
        assert np.array_equal(out_b, ex_b), n
        if want_total:
            assert tot == [int(first[n]), int(ex_b[n])], n
