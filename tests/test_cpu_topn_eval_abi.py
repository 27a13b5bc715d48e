"""The hold-out evaluation of the top-N lists is part of the C ABI: include/xmap_hip.h declares xmap_eval_users, xmap_topn_eval
and xmap_ctx_evaluate_topn, both libraries export them and the binding carries argtypes generated from the header.  (What they
compute is tests/test_gpu_topn_eval.py's.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_eval_users", "xmap_topn_eval", "xmap_ctx_evaluate_topn"]


def test_topn_eval_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64, f64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert P["xmap_eval_users"] == [v, i64, v, v, v, f64, i64, i32, v, v, v]
    assert P["xmap_topn_eval"] == [v, i64, v, v, v, f64, i64, i32, v, i64, v, i32, v, v, i32, v, v, v, v, v, v]
    assert P["xmap_ctx_evaluate_topn"] == [v, i64, v, v, v, f64, i32, i32, i32, v, i32, i32] + [v] * 7
    assert hipabi.lib.xmap_version() >= 104
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n


def test_the_makefile_builds_the_evaluation_kernels():
    mk = open(os.path.join(ROOT, "x-map_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bstage_e_eval\.hip\b", mk, flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "x-map_amd", "csrc", "stage_e_eval.hip"))
