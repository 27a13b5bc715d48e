"""The eligibility rules are part of the C ABI: include/xmap_hip.h declares xmap_rec_filter, the two fine-grained and the two
coarse filtered entry points and the XMAP_SRC_* sources; both libraries export the four names and the binding carries argtypes
generated from the header.  (What they compute is tests/test_gpu_filter.py's.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_topn_rows_filtered", "xmap_audience_rows_filtered", "xmap_ctx_recommend_filtered", "xmap_ctx_audience_filtered"]


def test_filter_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    # the arguments of the unfiltered twins up to out_decay, then (the batch of an item fold-in,) the filter and the stats
    assert P["xmap_topn_rows_filtered"] == P["xmap_topn_rows"][:-1] + [v, v]
    assert P["xmap_audience_rows_filtered"] == P["xmap_itemfold_audience_rows"][:-4] + [i32, v, v] + [v, v]
    assert P["xmap_audience_rows_filtered"][:-5] == P["xmap_audience_rows"][:-1]
    assert P["xmap_ctx_recommend_filtered"] == [v, i32] + P["xmap_ctx_recommend"][1:-1] + [v, v]
    assert P["xmap_ctx_audience_filtered"] == [v, i32] + P["xmap_ctx_audience"][1:-1] + [v, v]
    assert P["xmap_topn_rows"] == [v, i64, v, i32, i32, i32, i64, i32, i32] + [v] * 9 + [i32] + [v] * 5      # the twins keep theirs
    for k, name in enumerate(("RESIDENT", "FOLDIN", "ITEM_FOLDIN")):
        assert re.search(r"^#define\s+XMAP_SRC_%s\s+%d\b" % (name, k), hdr, flags=re.M)
        assert getattr(hipabi, "SRC_" + name) == k
    assert hipabi.header_constants(("XMAP_SRC_",)) == dict(SRC_RESIDENT=0, SRC_FOLDIN=1, SRC_ITEM_FOLDIN=2)
    assert hipabi.lib.xmap_version() >= 111
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n


def test_the_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    m = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*xmap_rec_filter\s*;", hdr, flags=re.S)
    assert m, "xmap_rec_filter is not declared"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        name = re.search(r"(\w+)\s*$", decl).group(1)
        fields.append((name, ctypes.c_void_p if "*" in decl else ctypes.c_double if decl.startswith("double ") else None))
    assert fields == [("allow", ctypes.c_void_p), ("ex_ptr", ctypes.c_void_p), ("ex_id", ctypes.c_void_p), ("min_score", ctypes.c_double)]
    assert list(hipabi.RecFilter._fields_) == fields
    assert re.search(r"const\s+uint32_t\s*\*\s*allow", body) and re.search(r"const\s+int64_t\s*\*\s*ex_ptr", body)
    assert re.search(r"const\s+int32_t\s*\*\s*ex_id", body)
    assert ctypes.sizeof(hipabi.RecFilter) == 3 * ctypes.sizeof(ctypes.c_void_p) + 8 == 32
    assert hipabi.RecFilter.min_score.offset == 24
    # rec_filter(): no tensors = the empty filter, no floor
    F = hipabi.rec_filter()
    assert F.allow is None and F.ex_ptr is None and F.ex_id is None and F.min_score == float("-inf")
    assert hipabi.rec_filter(min_score=2.5).min_score == 2.5
