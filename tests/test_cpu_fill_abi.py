"""The popularity-fill calls are part of the C ABI: include/xmap_hip.h declares xmap_pop_index, xmap_topn_fill_rows,
xmap_ctx_popular and xmap_ctx_recommend_filled; both libraries export them and the binding carries argtypes generated from the
header.  The host-side argument checks of the two coarse calls run before the context is looked at or any device work is done,
so they are tested here, without a device.  (What the calls compute is tests/test_gpu_fill.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_pop_index", "xmap_topn_fill_rows", "xmap_ctx_popular", "xmap_ctx_recommend_filled"]


def test_fill_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64, f64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert P["xmap_pop_index"] == [v, i32, v, v, i32, f64, i32, v, v, v, v]
    assert P["xmap_topn_fill_rows"] == [v, i64, v, i32, i32, i64, i32, v, v, v, i32, v, v, i32] + [v] * 7
    assert P["xmap_ctx_popular"] == [v, i32, f64, i32, i64, v, v, v]
    assert P["xmap_ctx_recommend_filled"] == [v, i32, i64, v, i32, i32, i32, v, i32, i32, f64, i32] + [v] * 7
    assert hipabi.lib.xmap_version() >= 120
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n
    assert X.xmap_version() == hipabi.lib.xmap_version()


def test_the_constants_match_the_header():
    import fill_statement as fs
    from xmap.engine import hipabi
    consts = hipabi.header_constants(prefixes=("XMAP_POP_", "XMAP_FILL_"))
    assert consts == {"POP_COUNT": 0, "POP_MEAN": 1, "FILL_WINDOW": 4096}
    assert {n: getattr(hipabi, n) for n in consts} == consts
    assert hipabi.POP_HOW == {"count": 0, "mean": 1}
    assert (fs.COUNT, fs.MEAN, fs.FILL_WINDOW, fs.KEEP_HELD) == (hipabi.POP_COUNT, hipabi.POP_MEAN, hipabi.FILL_WINDOW, hipabi.TOPN_KEEP_HELD)


def test_the_makefile_builds_the_new_file():
    mk = open(os.path.join(ROOT, "x-map_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bstage_e_fill\.hip\b", mk, flags=re.M)


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _popular(**change):
    from xmap.engine import hipabi
    a = dict(how=0, damping=0.0, min_count=1, n_max=5)
    a.update(change)
    n = max(1, min(int(a["n_max"]), 8))
    outs = [np.full(n, 77, np.int32), np.full(n, 7.5), np.full(1, 77, np.int64)]
    before = [o.tobytes() for o in outs]
    rc = hipabi.lib.xmap_ctx_popular(None, a["how"], a["damping"], a["min_count"], a["n_max"], *[_p(o) for o in outs])
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs] == before


def _filled(**change):
    from xmap.engine import hipabi
    a = dict(source=0, n_top=4, rank_by=0, flags=0, how=0, damping=0.0, min_count=1, floor=None)
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    users, wtab = np.arange(3, dtype=np.int32), np.ones(4)
    outs = [np.full(n_q, 77, np.int32), np.full((n_q, n), 77, np.int32), np.full((n_q, n), 7.5), np.full((n_q, n), 7.5),
            np.full((n_q, n), 77, np.int32)]
    stats = np.full(10, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    F = None if a["floor"] is None else ctypes.byref(hipabi.RecFilter(None, None, None, a["floor"]))
    rc = hipabi.lib.xmap_ctx_recommend_filled(None, a["source"], n_q, _p(users), a["n_top"], a["rank_by"], a["flags"], _p(wtab), 4, a["how"],
                                              a["damping"], a["min_count"], *([_p(o) for o in outs] + [F, _p(stats)]))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


NAN, INF = float("nan"), float("inf")
BAD_POPULAR = [("how -1", dict(how=-1), "how"), ("how 2", dict(how=2), "how"), ("a NaN damping", dict(damping=NAN), "damping"),
               ("an infinite damping", dict(damping=INF), "damping"), ("a negative damping", dict(damping=-0.5), "damping"),
               ("min_count 0", dict(min_count=0), "min_count"), ("n_max -1", dict(n_max=-1), "n_max")]
BAD_FILLED = [("n_top 0", dict(n_top=0), "n_top"), ("n_top 65", dict(n_top=65), "n_top"), ("rank_by 2", dict(rank_by=2), "rank_by"),
              ("an unknown flag", dict(flags=2), "flags"), ("how 2", dict(how=2), "how"), ("how -1", dict(how=-1), "how"),
              ("a NaN damping", dict(damping=NAN), "damping"), ("an infinite damping", dict(damping=INF), "damping"),
              ("a negative damping", dict(damping=-1.0), "damping"), ("min_count 0", dict(min_count=0), "min_count"),
              ("source 3", dict(source=3), "source"), ("source -1", dict(source=-1), "source"), ("a NaN floor", dict(floor=NAN), "min_score")]


@pytest.mark.parametrize("what,change,names", BAD_POPULAR, ids=[b[0] for b in BAD_POPULAR])
def test_popular_checks_its_arguments_on_the_host(what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before the context is read (none exists without a device): the outputs
    keep every byte"""
    from xmap.engine import hipabi
    rc, msg, unchanged = _popular(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


@pytest.mark.parametrize("what,change,names", BAD_FILLED, ids=[b[0] for b in BAD_FILLED])
def test_recommend_filled_checks_its_arguments_on_the_host(what, change, names):
    from xmap.engine import hipabi
    rc, msg, unchanged = _filled(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


def test_good_arguments_reach_the_context_check():
    """the same calls with valid values fail only on the context they were not given"""
    from xmap.engine import hipabi
    for change in (dict(), dict(how=hipabi.POP_MEAN, damping=25.0, min_count=3, n_max=0), dict(damping=1e308, n_max=1 << 40)):
        rc, msg, unchanged = _popular(**change)
        assert rc == hipabi.ERR_ARG and "have_rec" in msg and unchanged, msg
    for change in (dict(), dict(source=2, n_top=64, rank_by=1, flags=hipabi.TOPN_KEEP_HELD, how=hipabi.POP_MEAN, damping=0.5, min_count=7,
                                floor=0.25), dict(source=1, n_top=1, floor=-INF)):
        rc, msg, unchanged = _filled(**change)
        assert rc == hipabi.ERR_ARG and "have_nb" in msg and unchanged, msg
