"""The quota calls are part of the C ABI: include/xmap_hip.h declares xmap_quota_pool, xmap_quota_rows and xmap_ctx_recommend_quota;
both libraries export them and the binding carries argtypes generated from the header.  The host-side argument checks of the coarse
call run before the context is looked at or any device work is done, so they are tested here, without a device, with the host
helper labels.label_values.  (What the calls compute is tests/test_gpu_quota.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_quota_pool", "xmap_quota_rows", "xmap_ctx_recommend_quota"]


def test_quota_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    # stream, n_query, n_pool, the pool's four columns, rank_by, mode, cap, lab_cap, lab_weight, query_user, n_users, prof_ptr, prof_item,
    # n_items, n_labels, lab_ptr, lab_id, lab_allow, n_top, the six outputs, h_stats
    assert P["xmap_quota_pool"] == [v, i64, i32, v, v, v, v, i32, i32, i32, v, v, v, i64, v, v, i32, i32, v, v, v, i32] + [v] * 6 + [v]
    filtered_up_to_n_w = P["xmap_topn_rows_filtered"][:19]
    assert filtered_up_to_n_w == [v, i64, v, i32, i32, i32, i64, i32, i32] + [v] * 9 + [i32]
    # ... n_pool, mode, cap, lab_cap, lab_weight, n_labels, lab_ptr, lab_id, lab_allow, the six outputs, F, h_stats
    assert P["xmap_quota_rows"] == filtered_up_to_n_w + [i32, i32, i32, v, v, i32, v, v, v] + [v] * 6 + [v, v]
    # ctx, source, n_query, query_user, n_pool, n_top, rank_by, flags, wtab, n_w, mode, cap, lab_cap, lab_weight, lab_allow, six outputs, F, stats
    assert P["xmap_ctx_recommend_quota"] == [v, i32, i64, v, i32, i32, i32, i32, v, i32, i32, i32, v, v, v] + [v] * 6 + [v, v]
    assert hipabi.lib.xmap_version() >= 124
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n
    assert X.xmap_version() == hipabi.lib.xmap_version()


def test_the_constants_match_the_header_and_the_statement():
    import quota_statement as qs
    from xmap.engine import hipabi
    consts = hipabi.header_constants(prefixes=("XMAP_QUOTA_",))
    assert consts == {"QUOTA_CAP": 0, "QUOTA_SHARE": 1, "QUOTA_MAX_POOL": 1024, "QUOTA_MAX_RECORDS": 8192}
    assert {n: getattr(hipabi, n) for n in consts} == consts
    assert hipabi.QUOTA_MODE == {"cap": 0, "share": 1} == qs.MODE
    assert (qs.CAP, qs.SHARE, qs.MAX_POOL, qs.MAX_RECORDS) == (hipabi.QUOTA_CAP, hipabi.QUOTA_SHARE, hipabi.QUOTA_MAX_POOL,
                                                              hipabi.QUOTA_MAX_RECORDS)


def test_the_makefile_builds_the_new_file():
    mk = open(os.path.join(ROOT, "x-map_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bstage_e_quota\.hip\b", mk, flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "x-map_amd", "csrc", "stage_e_quota.hip"))


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _quota(**change):
    from xmap.engine import hipabi
    a = dict(source=0, n_query=3, n_pool=8, n_top=4, rank_by=0, flags=0, mode=0, cap=1, lab_cap=False, floor=None)
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    users, wtab, caps = np.arange(3, dtype=np.int32), np.ones(4), np.ones(4, np.int32)
    outs = [np.full(n_q, 77, np.int32), np.full((n_q, n), 77, np.int32), np.full((n_q, n), 7.5), np.full((n_q, n), 7.5),
            np.full((n_q, n), 77, np.int32), np.full((n_q, n), 77, np.int32)]
    stats = np.full(10, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    F = None if a["floor"] is None else ctypes.byref(hipabi.RecFilter(None, None, None, a["floor"]))
    rc = hipabi.lib.xmap_ctx_recommend_quota(None, a["source"], a["n_query"], _p(users), a["n_pool"], a["n_top"], a["rank_by"], a["flags"],
                                             _p(wtab), 4, a["mode"], a["cap"], _p(caps) if a["lab_cap"] else None, None, None,
                                             *([_p(o) for o in outs] + [F, _p(stats)]))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


NAN, INF = float("nan"), float("inf")
BAD = [("n_pool 0", dict(n_pool=0, n_top=1), "n_pool"), ("n_pool 1025", dict(n_pool=1025), "n_pool"), ("n_top 0", dict(n_top=0), "n_top"),
       ("n_top n_pool + 1", dict(n_pool=8, n_top=9), "n_top"), ("rank_by 2", dict(rank_by=2), "rank_by"), ("mode 2", dict(mode=2), "mode"),
       ("mode -1", dict(mode=-1), "mode"), ("cap 0 with lab_cap NULL", dict(cap=0), "cap"), ("an unknown flag", dict(flags=2), "flags"),
       ("source 3", dict(source=3), "source"), ("a NaN floor", dict(floor=NAN), "min_score"), ("n_query -1", dict(n_query=-1), "n_query")]


@pytest.mark.parametrize("what,change,names", BAD, ids=[b[0] for b in BAD])
def test_recommend_quota_checks_its_arguments_on_the_host(what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before the context is read (none exists without a device): the outputs
    keep every byte"""
    from xmap.engine import hipabi
    rc, msg, unchanged = _quota(**change)
    assert rc == hipabi.ERR_ARG
    assert re.search(r"\b%s\b" % names, msg), msg
    assert "have_nb" not in msg
    assert unchanged


def test_good_arguments_reach_the_context_check():
    """the same call with valid values fails only on the context it was not given"""
    from xmap.engine import hipabi
    for change in (dict(), dict(source=2, n_pool=1024, n_top=1024, rank_by=1, flags=hipabi.TOPN_KEEP_HELD, mode=hipabi.QUOTA_SHARE, cap=0,
                                floor=0.25), dict(source=1, n_pool=1, n_top=1, cap=2 ** 31 - 1, floor=-INF),
                   dict(cap=0, lab_cap=True), dict(cap=-5, mode=hipabi.QUOTA_SHARE), dict(n_query=0)):
        rc, msg, unchanged = _quota(**change)
        assert rc == hipabi.ERR_ARG and "have_nb" in msg and unchanged, msg


def test_label_values_by_hand():
    from xmap.engine.labels import label_values
    names = ["art", "crime", "zen"]
    caps = label_values(names, {"zen": 0, "art": 2}, 2 ** 31 - 1, np.int32)
    assert caps.dtype == np.int32 and caps.tolist() == [2, 2 ** 31 - 1, 0]
    w = label_values(names, {"crime": 7}, 0, np.uint32)
    assert w.dtype == np.uint32 and w.tolist() == [0, 7, 0]
    assert label_values(names, {}, 3, np.int32).tolist() == [3, 3, 3]
    assert label_values([], {}, 3, np.int32).tolist() == []
    with pytest.raises(ValueError):
        label_values(names, {"ghost": 1}, 0, np.int32)
    with pytest.raises(ValueError):
        label_values(names, {"art": -1}, 0, np.uint32)
    with pytest.raises(ValueError):
        label_values(names, {"art": 2 ** 31}, 0, np.int32)
