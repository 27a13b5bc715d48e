"""The device-resident recommender tail is part of the C ABI: include/xmap_hip.h declares its fine-grained and coarse entry
points, libxmap_hip.so exports them and the binding carries argtypes generated from the header.  (What they compute is
tests/test_gpu_tail.py's; a coarse context cannot be created without a device, so calling them out of order is checked
there too.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINE = ["xmap_rec_profiles", "xmap_predict_rows", "xmap_mae"]
COARSE = ["xmap_ctx_rec_sim", "xmap_ctx_rec_profiles_download", "xmap_ctx_rec_download", "xmap_ctx_rec_select",
          "xmap_ctx_rec_set_neighbors", "xmap_ctx_rec_neighbors_download", "xmap_ctx_predict"]


def test_tail_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in FINE + COARSE:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert P["xmap_rec_profiles"] == [v, i64, i64, i64] + [v] * 10
    assert P["xmap_predict_rows"] == [v, i64, v, v, i64, i32, i32] + [v] * 9 + [i32] + [v] * 4
    assert P["xmap_mae"] == [v, i64] + [v] * 5
    assert P["xmap_ctx_rec_sim"] == [v, i32, v]
    assert P["xmap_ctx_rec_select"] == [v, i32]
    assert P["xmap_ctx_rec_set_neighbors"] == [v, i32, v, v, v]
    assert P["xmap_ctx_predict"] == [v, i64, v, v, v, v, i32, v, v, v, v, v]
    assert hipabi.lib.xmap_version() >= 101
    # the xcheck library is built from the same sources
    X = hipabi.xlib()
    for n in FINE + COARSE:
        assert hasattr(X, n), n
