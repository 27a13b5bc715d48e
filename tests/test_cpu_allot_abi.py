"""The allot calls are part of the C ABI: include/xmap_hip.h declares xmap_allot_pool, xmap_allot_rows and xmap_ctx_recommend_allot;
both libraries export them and the binding carries argtypes generated from the header.  The host-side argument checks of the coarse
call run before the context is looked at or any device work is done, so they are tested here, without a device.  (What the calls
compute is tests/test_gpu_allot.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_allot_pool", "xmap_allot_rows", "xmap_ctx_recommend_allot"]


def test_allot_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    # stream, n_query, n_pool, the pool's four columns, rank_by, n_items, cap, item_cap, n_top, the five outputs, item_taken, h_stats
    assert P["xmap_allot_pool"] == [v, i64, i32, v, v, v, v, i32, i32, i32, v, i32] + [v] * 5 + [v, v]
    filtered_up_to_n_w = P["xmap_topn_rows_filtered"][:19]
    # ... n_top, cap, item_cap, the five outputs, item_taken, F, h_stats
    assert P["xmap_allot_rows"] == filtered_up_to_n_w + [i32, i32, v] + [v] * 5 + [v, v, v]
    # ctx, source, n_query, query_user, n_pool, n_top, rank_by, flags, wtab, n_w, cap, item_cap, n_cap, five outputs, item_taken, F, stats
    assert P["xmap_ctx_recommend_allot"] == [v, i32, i64, v, i32, i32, i32, i32, v, i32, i32, v, i32] + [v] * 5 + [v, v, v]
    assert hipabi.lib.xmap_version() >= 125
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n
    assert X.xmap_version() == hipabi.lib.xmap_version()


def test_the_constant_matches_the_header_and_the_statement():
    import allot_statement as al
    from xmap.engine import hipabi
    assert hipabi.header_constants(prefixes=("XMAP_ALLOT_",)) == {"ALLOT_MAX_POOL": 1024}
    assert hipabi.ALLOT_MAX_POOL == al.MAX_POOL == 1024


def test_the_makefile_builds_the_new_file():
    mk = open(os.path.join(ROOT, "x-map_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bstage_e_allot\.hip\b", mk, flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "x-map_amd", "csrc", "stage_e_allot.hip"))


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _allot(**change):
    from xmap.engine import hipabi
    a = dict(source=0, n_query=3, n_pool=8, n_top=4, rank_by=0, flags=0, cap=1, item_cap=None, floor=None, taken=True)
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    users, wtab = np.arange(3, dtype=np.int32), np.ones(4)
    caps = None if a["item_cap"] is None else np.asarray(a["item_cap"], np.int32)
    outs = [np.full(n_q, 77, np.int32), np.full((n_q, n), 77, np.int32), np.full((n_q, n), 7.5), np.full((n_q, n), 7.5),
            np.full((n_q, n), 77, np.int32), np.full(6, 77, np.int32)]
    stats = np.full(12, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    F = None if a["floor"] is None else ctypes.byref(hipabi.RecFilter(None, None, None, a["floor"]))
    rc = hipabi.lib.xmap_ctx_recommend_allot(None, a["source"], a["n_query"], _p(users), a["n_pool"], a["n_top"], a["rank_by"], a["flags"],
                                             _p(wtab), 4, a["cap"], None if caps is None else _p(caps), 0 if caps is None else len(caps),
                                             *([_p(o) for o in outs[:5]] + [_p(outs[5]) if a["taken"] else None, F, _p(stats)]))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


NAN, INF = float("nan"), float("inf")
BAD = [("n_pool 0", dict(n_pool=0, n_top=1), "n_pool"), ("n_pool 65", dict(n_pool=65), "n_pool"), ("n_top 0", dict(n_top=0), "n_top"),
       ("n_top n_pool + 1", dict(n_pool=8, n_top=9), "n_top"), ("rank_by 2", dict(rank_by=2), "rank_by"),
       ("cap 0 with item_cap NULL", dict(cap=0), "cap"), ("a negative item_cap entry", dict(item_cap=[1, 0, 2, -1, 5, -2]), r"item_cap\[3\]"),
       ("an unknown flag", dict(flags=2), "flags"), ("source 3", dict(source=3), "source"), ("a NaN floor", dict(floor=NAN), "min_score"),
       ("n_query -1", dict(n_query=-1), "n_query")]


@pytest.mark.parametrize("what,change,names", BAD, ids=[b[0] for b in BAD])
def test_recommend_allot_checks_its_arguments_on_the_host(what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before the context is read (none exists without a device): the outputs
    keep every byte"""
    from xmap.engine import hipabi
    rc, msg, unchanged = _allot(**change)
    assert rc == hipabi.ERR_ARG
    assert re.search(r"\b%s" % names, msg), msg
    assert "have_nb" not in msg
    assert unchanged


def test_good_arguments_reach_the_context_check():
    """the same call with valid values fails only on the context it was not given"""
    from xmap.engine import hipabi
    for change in (dict(), dict(source=2, n_pool=64, n_top=64, rank_by=1, flags=hipabi.TOPN_KEEP_HELD, floor=0.25),
                   dict(source=1, n_pool=1, n_top=1, cap=2 ** 31 - 1, floor=-INF), dict(cap=0, item_cap=[0, 1, 2 ** 31 - 1]),
                   dict(cap=-5, item_cap=[], taken=False), dict(n_query=0)):
        rc, msg, unchanged = _allot(**change)
        assert rc == hipabi.ERR_ARG and "have_nb" in msg and unchanged, msg
