"""The audience of an item is part of the C ABI: include/xmap_hip.h declares xmap_audience_rows, xmap_ctx_audience and
xmap_ctx_foldin_audience, both libraries export them and the binding carries argtypes generated from the header.  The three
take the arguments of their top-N counterparts position for position (query_item for query_user, out_user for out_item).
(What they compute, and calling the coarse entries out of order, is tests/test_gpu_audience.py's.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {"xmap_audience_rows": "xmap_topn_rows", "xmap_ctx_audience": "xmap_ctx_recommend",
         "xmap_ctx_foldin_audience": "xmap_ctx_foldin_recommend"}
RENAMED = {"query_user": "query_item", "out_item": "out_user"}


def _parameters(hdr, name):
    """[(type, name)*] of a declaration in the header, comments removed"""
    text = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S)
    assert m, "%s is not declared in the header" % name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        k = re.search(r"(\w+)$", a)
        out.append((a[:k.start()].strip(), k.group(1)))
    return out


def test_audience_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in TWINS:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert P["xmap_audience_rows"] == [v, i64, v, i32, i32, i32, i64, i32, i32] + [v] * 9 + [i32] + [v] * 5
    assert P["xmap_ctx_audience"] == P["xmap_ctx_foldin_audience"] == [v, i64, v, i32, i32, i32, v, i32] + [v] * 5
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in TWINS:
        assert hasattr(X, n), n


def test_the_prototypes_are_the_recommend_ones_position_for_position():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for mine, twin in TWINS.items():
        a, b = _parameters(hdr, mine), _parameters(hdr, twin)
        assert [t for t, _ in a] == [t for t, _ in b], mine
        assert [n for _, n in a] == [RENAMED.get(n, n) for _, n in b], mine
        assert hipabi.PROTOTYPES[mine] == hipabi.PROTOTYPES[twin]


def test_the_flag_and_the_version():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    assert re.search(r"^#define\s+XMAP_AUDIENCE_KEEP_HOLDERS\s+1\b", hdr, flags=re.M) and hipabi.AUDIENCE_KEEP_HOLDERS == 1
    assert hipabi.header_constants(("XMAP_AUDIENCE_",)) == {"AUDIENCE_KEEP_HOLDERS": hipabi.AUDIENCE_KEEP_HOLDERS}
    assert hipabi.lib.xmap_version() >= 109
