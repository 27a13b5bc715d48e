"""The explanation of a recommendation is part of the C ABI: include/xmap_hip.h declares xmap_explain_rows,
xmap_explain_sources, xmap_ctx_explain and xmap_ctx_foldin_explain, both libraries export them and the binding carries argtypes
generated from the header.  (What they compute, and calling the coarse entries out of order, is tests/test_gpu_explain.py's: a
coarse context cannot be created without a device.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_explain_rows", "xmap_explain_sources", "xmap_ctx_explain", "xmap_ctx_foldin_explain"]


def test_explain_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    # the middle arguments of xmap_explain_rows are the arrays of xmap_predict_rows, in its order
    middle = P["xmap_predict_rows"][4:17]
    assert middle == [i64, i32, i32] + [v] * 9 + [i32]
    assert P["xmap_explain_rows"] == [v, i64, v, v, i32, i32] + middle + [v] * 7 + [v]
    assert P["xmap_explain_sources"] == [v, i64, v, i32, v, v, i64, i32] + [v] * 8 + [i32, v, v]
    coarse = [v, i64, v, v, i32, i32, i32, v, i32] + [v] * 7 + [v, v, v]
    assert P["xmap_ctx_explain"] == coarse and P["xmap_ctx_foldin_explain"] == coarse
    assert hipabi.EXPLAIN_MAX_EV == 16 and hipabi.EXPLAIN_MAX_SRC == 8
    assert hipabi.lib.xmap_version() >= 107
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n


def test_the_limits_are_the_kernels():
    src = open(os.path.join(ROOT, "x-map_amd", "csrc", "predict_rows.h")).read()
    assert re.search(r"constexpr int EX_MAX_EV = 16;", src) and re.search(r"constexpr int EX_MAX_SRC = 8;", src)
