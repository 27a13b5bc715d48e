"""The user-kNN calls are part of the C ABI: include/xmap_hip.h declares xmap_uknn_means, xmap_uknn_predict_rows,
xmap_uknn_topn_rows, xmap_ctx_uknn_predict and xmap_ctx_uknn_recommend; both libraries export them and the binding carries argtypes
generated from the header.  The host-side argument checks of the coarse calls run before the context is looked at or any device
work is done, so they are tested here, without a device.  (What the calls compute is tests/test_gpu_uknn.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_uknn_means", "xmap_uknn_predict_rows", "xmap_uknn_topn_rows", "xmap_ctx_uknn_predict", "xmap_ctx_uknn_recommend"]


def test_uknn_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert P["xmap_uknn_means"] == [v, i64, i32] + [v] * 5
    assert P["xmap_uknn_predict_rows"] == [v, i64, v, v, i64, v, i32, v, v, v, i64, i32, v, v, v, v, i32] + [v] * 4
    assert P["xmap_uknn_topn_rows"] == [v, i64, v, i64, v, v, v, i32, v, v, v, i64, i32, v, v, v, v, i32, i32, i32, i64] + [v] * 6
    assert P["xmap_ctx_uknn_predict"] == [v, i32, i64, v, v, v, i32, i32, i32, i32, i32] + [v] * 5
    assert P["xmap_ctx_uknn_recommend"] == [v, i32, i64, v] + [i32] * 7 + [v] * 6
    assert hipabi.lib.xmap_version() >= 117
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n
    assert X.xmap_version() == hipabi.lib.xmap_version()


def test_the_constants_match_the_header():
    from xmap.engine import hipabi
    consts = hipabi.header_constants(prefixes=("XMAP_UKNN_",))
    assert consts == {"UKNN_OWN_MEAN": 1, "UKNN_KEEP_HELD": 2}
    assert {n: getattr(hipabi, n) for n in consts} == consts


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _filter(floor):
    from xmap.engine import hipabi
    return None if floor is None else ctypes.byref(hipabi.RecFilter(None, None, None, floor))


def _recommend(**change):
    from xmap.engine import hipabi
    a = dict(source=0, n_nb=5, peer_flags=0, cap=1, min_common=1, flags=0, n_top=4, min_support=1, floor=None)
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    query = np.arange(n_q, dtype=np.int32)
    outs = [np.full(n_q, 77, np.int32), np.full((n_q, n), 77, np.int32), np.full((n_q, n), 7.5), np.full((n_q, n), 77, np.int32)]
    stats = np.full(6, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    rc = hipabi.lib.xmap_ctx_uknn_recommend(None, a["source"], n_q, _p(query), a["n_nb"], a["peer_flags"], a["cap"], a["min_common"],
                                            a["flags"], a["n_top"], a["min_support"], *([_p(o) for o in outs] + [_filter(a["floor"]), _p(stats)]))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


def _predict(**change):
    from xmap.engine import hipabi
    a = dict(source=0, n_nb=5, peer_flags=0, cap=1, min_common=1, flags=0)
    a.update(change)
    n_t = 4
    user, item = np.arange(n_t, dtype=np.int32), np.arange(n_t, dtype=np.int32)
    real = np.full(n_t, 3.0)
    outs = [np.full(n_t, 7.5), np.full(n_t, 7.5), np.full(n_t, 77, np.int32), np.full(n_t, 77, np.int32), np.full(2, 7.5)]
    before = [o.tobytes() for o in outs]
    rc = hipabi.lib.xmap_ctx_uknn_predict(None, a["source"], n_t, _p(user), _p(item), _p(real), a["n_nb"], a["peer_flags"], a["cap"],
                                          a["min_common"], a["flags"], *[_p(o) for o in outs])
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs] == before


BAD_BOTH = [("n_nb 0", dict(n_nb=0), "n_nb"), ("n_nb 1025", dict(n_nb=1025), "n_nb"), ("cap 0", dict(cap=0), "cap"),
            ("min_common 0", dict(min_common=0), "min_common"), ("source 2", dict(source=2), "source"),
            ("an unknown peer flag", dict(peer_flags=8), "peer_flags"), ("the peers' own flag SAME", dict(peer_flags=1), "peer_flags"),
            ("an unknown flag", dict(flags=4), "flags")]
BAD_RECOMMEND = BAD_BOTH + [("n_top 0", dict(n_top=0), "n_top"), ("n_top 1025", dict(n_top=1025), "n_top"),
                            ("min_support 0", dict(min_support=0), "min_support"), ("a NaN floor", dict(floor=float("nan")), "min_score")]
BAD_PREDICT = BAD_BOTH + [("KEEP_HELD, a top-N flag", dict(flags=2), "flags")]


@pytest.mark.parametrize("what,change,names", BAD_RECOMMEND, ids=[b[0] for b in BAD_RECOMMEND])
def test_recommend_checks_its_arguments_on_the_host(what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before the context is read (none exists without a device): the outputs
    keep every byte"""
    from xmap.engine import hipabi
    rc, msg, unchanged = _recommend(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


@pytest.mark.parametrize("what,change,names", BAD_PREDICT, ids=[b[0] for b in BAD_PREDICT])
def test_predict_checks_its_arguments_on_the_host(what, change, names):
    from xmap.engine import hipabi
    rc, msg, unchanged = _predict(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


def test_good_arguments_reach_the_context_check():
    """the same calls with valid values fail only on the context they were not given"""
    from xmap.engine import hipabi
    peer = hipabi.PEERS_KEEP_SELF | hipabi.PEERS_CENTRED
    for change in (dict(), dict(n_nb=1024, n_top=1024, cap=7, min_common=3, min_support=3, peer_flags=peer, source=1, floor=0.25,
                               flags=hipabi.UKNN_OWN_MEAN | hipabi.UKNN_KEEP_HELD)):
        rc, msg, unchanged = _recommend(**change)
        assert rc == hipabi.ERR_ARG and "have_rec" in msg and unchanged, msg
    for change in (dict(), dict(n_nb=1024, cap=7, min_common=3, peer_flags=peer, source=1, flags=hipabi.UKNN_OWN_MEAN)):
        rc, msg, unchanged = _predict(**change)
        assert rc == hipabi.ERR_ARG and "have_rec" in msg and unchanged, msg
