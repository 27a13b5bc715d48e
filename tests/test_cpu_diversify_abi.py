"""Diversified top-N is part of the C ABI: include/xmap_hip.h declares xmap_div_index, xmap_diversify_rows and
xmap_ctx_recommend_diverse; both libraries export them and the binding carries argtypes generated from the header.  The host-side
argument checks of the coarse call run before the context is looked at or any device work is done, so they are tested here, without
a device.  (What the calls compute is tests/test_gpu_diversify.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_div_index", "xmap_diversify_rows", "xmap_ctx_recommend_diverse"]


def test_diversify_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64, f64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert P["xmap_div_index"] == [v, i32, i64] + [v] * 6
    assert P["xmap_diversify_rows"] == [v, i64, i32] + [v] * 4 + [i32, f64, i32, i32] + [v] * 3 + [v] * 7 + [v]
    assert P["xmap_ctx_recommend_diverse"] == [v, i32, i64, v, i32, i32, i32, i32, v, i32, f64, v] + [v] * 6 + [v]
    assert hipabi.lib.xmap_version() >= 112
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n


BAD = [("weight NaN", dict(weight=float("nan")), "weight"), ("weight negative", dict(weight=-0.5), "weight"),
       ("weight infinite", dict(weight=float("inf")), "weight"), ("n_top > n_pool", dict(n_pool=8, n_top=9), "n_top"),
       ("n_pool > 64", dict(n_pool=65, n_top=10), "n_pool"), ("source 2", dict(source=2), "source")]


@pytest.mark.parametrize("what,change,names", BAD, ids=[b[0] for b in BAD])
def test_the_coarse_call_checks_its_arguments_on_the_host(what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before the context is read (none exists without a device): the outputs
    keep every byte"""
    from xmap.engine import hipabi
    a = dict(source=0, n_pool=16, n_top=4, weight=0.5)
    a.update(change)
    Q, n = 3, 4
    query = np.arange(Q, dtype=np.int32)
    wtab = np.ones(4)
    outs = [np.full(Q, 77, np.int32), np.full((Q, n), 77, np.int32)] + [np.full((Q, n), 7.5) for _ in range(3)] + [np.full(Q, 7.5)]
    stats = np.full(8, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = hipabi.lib.xmap_ctx_recommend_diverse(None, a["source"], Q, p(query), a["n_pool"], a["n_top"], 0, 0, p(wtab), 4, a["weight"], None,
                                               *([p(o) for o in outs] + [p(stats)]))
    assert rc == hipabi.ERR_ARG
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    assert "bad argument" in msg and names in msg, msg
    assert [o.tobytes() for o in outs + [stats]] == before


def test_good_arguments_reach_the_context_check():
    """the same call with valid values fails only on the context it was not given"""
    from xmap.engine import hipabi
    rc = hipabi.lib.xmap_ctx_recommend_diverse(None, 1, 0, None, 64, 64, 0, 0, None, 0, 0.0, None, None, None, None, None, None, None, None)
    assert rc == hipabi.ERR_ARG
    assert "have_rec" in (hipabi.lib.xmap_last_error() or b"").decode()
