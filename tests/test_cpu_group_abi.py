"""The group lists are part of the C ABI: include/xmap_hip.h declares xmap_group_topn_rows, xmap_ctx_recommend_group and the
XMAP_GROUP_* constants; both libraries export the two names and the binding carries argtypes generated from the header.  (What
they compute is tests/test_gpu_group.py's.)"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_group_topn_rows", "xmap_ctx_recommend_group"]


def test_group_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64, dbl = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    model = P["xmap_topn_rows"][6:19]           # n_users .. n_w
    assert model == [i64, i32, i32] + [v] * 9 + [i32]
    assert P["xmap_group_topn_rows"] == [v, i64, v, v, i32, i32, i32, i32, dbl] + model + [v] * 5 + [v, v]
    assert P["xmap_ctx_recommend_group"] == [v, i32, i64, v, v, i32, i32, i32, i32, dbl, v, i32] + [v] * 5 + [v, v]
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n
    assert hipabi.lib.xmap_version() >= 113 and X.xmap_version() == hipabi.lib.xmap_version()


def test_the_constants_match_the_header():
    from xmap.engine import hipabi
    consts = hipabi.header_constants(("XMAP_GROUP_",))
    assert consts == dict(GROUP_MEAN=0, GROUP_MIN=1, GROUP_MAX=2, GROUP_MAX_MEMBERS=64)
    assert {n: getattr(hipabi, n) for n in consts} == consts
    assert hipabi.GROUP_HOW == dict(mean=hipabi.GROUP_MEAN, min=hipabi.GROUP_MIN, max=hipabi.GROUP_MAX)
    import group_statement as gs
    assert (gs.MEAN, gs.MIN, gs.MAX, gs.MAX_MEMBERS) == (0, 1, 2, 64)
    # the member pass is shared, not copied: the group file holds no candidate kernel of its own over the reverse lists
    src = open(os.path.join(ROOT, "x-map_amd", "csrc", "stage_e_group.hip")).read()
    assert "tn_score_candidates" in src and "k_tn_rev<" not in src
    mk = open(os.path.join(ROOT, "x-map_amd", "csrc", "Makefile")).read()
    assert "stage_e_group.hip" in mk and "topn_pass.h" in mk
