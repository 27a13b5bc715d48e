"""The item fold-in is part of the C ABI: include/xmap_hip.h declares the three fine-grained entries (xmap_itemfold_count,
xmap_itemfold_fill, xmap_itemfold_audience_rows) and the five coarse ones (xmap_ctx_item_foldin, _download, _audience, _predict,
_recommend), both libraries export them and the binding carries argtypes generated from the header.  The coarse twins take the
parameter lists of the resident entries, the audience entry those of xmap_audience_rows and three more.
(What they compute, and calling them out of order, is tests/test_gpu_item_foldin.py's: a coarse context needs a device.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_itemfold_count", "xmap_itemfold_fill", "xmap_itemfold_audience_rows", "xmap_ctx_item_foldin",
         "xmap_ctx_item_foldin_download", "xmap_ctx_item_foldin_audience", "xmap_ctx_item_foldin_predict",
         "xmap_ctx_item_foldin_recommend"]
TWINS = [("xmap_ctx_item_foldin_audience", "xmap_ctx_audience"), ("xmap_ctx_item_foldin_predict", "xmap_ctx_predict"),
         ("xmap_ctx_item_foldin_recommend", "xmap_ctx_recommend")]


def _params(name):
    """the declared parameters of the header, names included"""
    from xmap.engine import hipabi
    hdr = re.sub(r"/\*.*?\*/", " ", open(hipabi.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_item_foldin_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert P["xmap_itemfold_count"] == [v, i64, i64, v, v, i64, i32, v, v, i64, v, v, v]
    assert P["xmap_itemfold_fill"] == [v, i64, i64, v, v, v, i64, i32, v, v, v, v, i32, i64] + [v] * 7
    assert P["xmap_ctx_item_foldin"] == [v, i64] + [v] * 4
    assert P["xmap_ctx_item_foldin_download"] == [v] * 12
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n


def test_the_coarse_twins_take_the_parameter_lists_of_the_resident_entries():
    from xmap.engine import hipabi
    P = hipabi.PROTOTYPES
    for mine, theirs in TWINS:
        assert P[mine] == P[theirs], mine
        assert _params(mine) == _params(theirs), mine


def test_the_audience_entry_extends_xmap_audience_rows_by_three_arguments():
    from xmap.engine import hipabi
    P = hipabi.PROTOTYPES
    mine, theirs = _params("xmap_itemfold_audience_rows"), _params("xmap_audience_rows")
    assert mine[:len(theirs)] == theirs
    assert mine[len(theirs):] == ["int32_t n_resident", "const int64_t *new_ptr", "const int32_t *new_user"]
    assert P["xmap_itemfold_audience_rows"] == P["xmap_audience_rows"] + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]


def test_no_new_flag_macro():
    from xmap.engine import hipabi
    assert hipabi.header_constants(("XMAP_AUDIENCE_",)) == {"AUDIENCE_KEEP_HOLDERS": 1}
    assert hipabi.header_constants(("XMAP_TOPN_",)) == {"TOPN_KEEP_HELD": 1}


def test_the_version_says_item_fold_in():
    from xmap.engine import hipabi
    assert hipabi.lib.xmap_version() >= 110
