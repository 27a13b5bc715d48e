"""The top-N recommendation is part of the C ABI: include/xmap_hip.h declares xmap_topn_rows and xmap_ctx_recommend, both
libraries export them and the binding carries argtypes generated from the header.  (What they compute, and calling the coarse
entry out of order, is tests/test_gpu_topn.py's: a coarse context cannot be created without a device.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_topn_rows", "xmap_ctx_recommend"]


def test_topn_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert P["xmap_topn_rows"] == [v, i64, v, i32, i32, i32, i64, i32, i32] + [v] * 9 + [i32] + [v] * 5
    assert P["xmap_ctx_recommend"] == [v, i64, v, i32, i32, i32, v, i32] + [v] * 5
    assert re.search(r"^#define\s+XMAP_TOPN_KEEP_HELD\s+1\b", hdr, flags=re.M) and hipabi.TOPN_KEEP_HELD == 1
    assert hipabi.lib.xmap_version() >= 103
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n
