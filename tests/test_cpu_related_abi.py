"""The related-items calls are part of the C ABI: include/xmap_hip.h declares xmap_related_rows and xmap_ctx_related; both libraries
export them and the binding carries argtypes generated from the header.  The host-side argument checks of the coarse call run
before the context is looked at or any device work is done, so they are tested here, without a device.  (What the calls compute
is tests/test_gpu_related.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_related_rows", "xmap_ctx_related"]


def test_related_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert P["xmap_related_rows"] == [v, i64, v, v, v, i32, v, v, v, i32, i32, i32, i32, i64] + [v] * 6
    assert P["xmap_ctx_related"] == [v, i64, v, v, v, i32, i32, i32, i32, i64] + [v] * 6
    assert hipabi.lib.xmap_version() >= 119
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n
    assert X.xmap_version() == hipabi.lib.xmap_version()


def test_the_constants_match_the_header():
    from xmap.engine import hipabi
    consts = hipabi.header_constants(prefixes=("XMAP_RELATED_",))
    assert consts == {"RELATED_SUM": 0, "RELATED_MEAN": 1, "RELATED_MAX": 2, "RELATED_KEEP_MEMBERS": 1}
    assert {n: getattr(hipabi, n) for n in consts} == consts
    assert hipabi.RELATED_HOW == {"sum": 0, "mean": 1, "max": 2}


def test_the_makefile_builds_the_new_file():
    mk = open(os.path.join(ROOT, "x-map_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bstage_e_related\.hip\b", mk, flags=re.M)


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _related(**change):
    from xmap.engine import hipabi
    a = dict(how=0, flags=0, n_top=4, min_support=1, max_records=0, floor=None, b_ptr=[0, 2, 2, 3])
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    b_ptr, b_item, b_w = np.asarray(a["b_ptr"], np.int64), np.arange(3, dtype=np.int32), np.ones(3)
    outs = [np.full(n_q, 77, np.int32), np.full((n_q, n), 77, np.int32), np.full((n_q, n), 7.5), np.full((n_q, n), 77, np.int32)]
    stats = np.full(6, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    F = None if a["floor"] is None else ctypes.byref(hipabi.RecFilter(None, None, None, a["floor"]))
    rc = hipabi.lib.xmap_ctx_related(None, n_q, _p(b_ptr), _p(b_item), _p(b_w), a["how"], a["flags"], a["n_top"], a["min_support"],
                                     a["max_records"], *([_p(o) for o in outs] + [F, _p(stats)]))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


BAD = [("n_top 0", dict(n_top=0), "n_top"), ("n_top 1025", dict(n_top=1025), "n_top"), ("how -1", dict(how=-1), "how"),
       ("how 3", dict(how=3), "how"), ("an unknown flag", dict(flags=2), "flags"), ("min_support 0", dict(min_support=0), "min_support"),
       ("a NaN floor", dict(floor=float("nan")), "min_score"), ("max_records -1", dict(max_records=-1), "max_records"),
       ("b_ptr not from 0", dict(b_ptr=[1, 2, 2, 3]), "b_ptr[0]"), ("b_ptr decreasing", dict(b_ptr=[0, 2, 1, 3]), "b_ptr[2]")]


@pytest.mark.parametrize("what,change,names", BAD, ids=[b[0] for b in BAD])
def test_related_checks_its_arguments_on_the_host(what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before the context is read (none exists without a device): the outputs
    keep every byte"""
    from xmap.engine import hipabi
    rc, msg, unchanged = _related(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


def test_good_arguments_reach_the_context_check():
    """the same call with valid values fails only on the context it was not given"""
    from xmap.engine import hipabi
    for change in (dict(), dict(how=hipabi.RELATED_MAX, flags=hipabi.RELATED_KEEP_MEMBERS, n_top=1024, min_support=3, max_records=17,
                               floor=0.25), dict(how=hipabi.RELATED_MEAN, n_top=1, floor=float("-inf"))):
        rc, msg, unchanged = _related(**change)
        assert rc == hipabi.ERR_ARG and "have_rec" in msg and unchanged, msg
