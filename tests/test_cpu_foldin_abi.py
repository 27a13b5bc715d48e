"""Fold-in is part of the C ABI: include/xmap_hip.h declares the two fine-grained entries (xmap_foldin_count, xmap_foldin_fill)
and the four coarse ones (xmap_ctx_foldin, _download, _recommend, _predict), both libraries export them and the binding carries
argtypes generated from the header.  The batch variants of recommend / predict take the parameter lists of the resident entries.
(What they compute, and calling them out of order, is tests/test_gpu_foldin.py's: a coarse context needs a device.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_foldin_count", "xmap_foldin_fill", "xmap_ctx_foldin", "xmap_ctx_foldin_download", "xmap_ctx_foldin_recommend",
         "xmap_ctx_foldin_predict"]


def test_foldin_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert P["xmap_foldin_count"] == [v, i64, i64, v, v, i32] + [v] * 6
    assert P["xmap_foldin_fill"] == [v, i64, i64, v, v, v, v, i32] + [v] * 7
    assert P["xmap_ctx_foldin"] == [v, i64] + [v] * 5
    assert P["xmap_ctx_foldin_download"] == [v] * 5
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n


def test_the_batch_entries_take_the_parameter_lists_of_the_resident_ones():
    from xmap.engine import hipabi
    P = hipabi.PROTOTYPES
    assert P["xmap_ctx_foldin_recommend"] == P["xmap_ctx_recommend"]
    assert P["xmap_ctx_foldin_predict"] == P["xmap_ctx_predict"]

    def params(name):           # the declared parameters of the header, names included (ctx aside)
        hdr = re.sub(r"/\*.*?\*/", " ", open(hipabi.HEADER_PATH).read(), flags=re.S)
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        return [" ".join(a.split()) for a in m.group(1).split(",")]
    assert params("xmap_ctx_foldin_recommend") == params("xmap_ctx_recommend")
    assert params("xmap_ctx_foldin_predict") == params("xmap_ctx_predict")


def test_the_version_says_fold_in():
    from xmap.engine import hipabi
    assert hipabi.lib.xmap_version() >= 105
