"""The union of AlterEgo rows is part of the C ABI: declared in include/xmap_hip.h, exported by libxmap_hip.so, typed by hipabi
from the header like every other entry, and the descriptor hipabi passes has the header's layout."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("xmap_union_count", "xmap_union_fill", "xmap_ctx_union")


def _header():
    with open(os.path.join(ROOT, "include", "xmap_hip.h")) as f:
        return f.read()


def test_union_entries_are_declared_exported_and_typed():
    from xmap.engine import hipabi as abi
    protos = abi.header_prototypes()
    for n in NAMES:
        assert n in protos and n in abi.EXPORTS
        f = getattr(abi.lib, n)
        assert f.argtypes == protos[n] and f.restype is C.c_int
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert protos["xmap_union_count"] == [vp, i32, vp, i64, i32, i32, vp, vp]
    assert protos["xmap_union_fill"] == [vp, i32, vp, i64, i32, i32, vp, i64, vp, vp, vp]
    assert protos["xmap_ctx_union"] == [vp, i32, vp, vp, vp, i64, i32, i32, vp]


def test_union_flag_and_descriptor_match_the_header():
    from xmap.engine import hipabi as abi
    text = _header()
    m = re.search(r"^#define\s+XMAP_UNION_DISTINCT\s+(\d+)\b", text, flags=re.M)
    assert m and int(m.group(1)) == abi.UNION_DISTINCT
    body = re.search(r"typedef struct xmap_union_part \{(.*?)\} xmap_union_part;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        kind = C.c_void_p if "*" in decl else (C.c_int64 if "int64_t" in decl else C.c_int32)
        for name in decl.replace("*", " ").split(",")[0:]:
            fields.append((name.split()[-1], kind))
    assert fields == [(n, t) for n, t in abi.UnionPart._fields_]
    assert C.sizeof(abi.UnionPart) == 96


def test_union_entries_refuse_bad_host_arguments_without_a_device():
    """the checks that need no GPU: a part count outside 1 .. 16, unknown flags, a null descriptor array"""
    from xmap.engine import hipabi as abi
    parts = (abi.UnionPart * 1)()
    ptr, h = (C.c_int64 * 1)(), (C.c_int64 * 4)()
    for n_parts, flags, p in ((0, 0, parts), (17, 0, parts), (1, 2, parts), (1, 0, None)):
        assert abi.lib.xmap_union_count(None, n_parts, p, 0, 0, flags, ptr, h) == abi.ERR_ARG
        assert abi.lib.xmap_union_fill(None, n_parts, p, 0, 0, flags, ptr, 0, None, None, None) == abi.ERR_ARG
    assert abi.lib.xmap_ctx_union(None, 1, None, None, None, 0, 0, 0, None) == abi.ERR_ARG
