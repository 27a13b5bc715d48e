"""The peers calls are part of the C ABI: include/xmap_hip.h declares xmap_peer_index, xmap_peer_centre, xmap_peer_rows and
xmap_ctx_peers (and the measurement hook xmap_debug_sort_pairs); both
libraries export them and the binding carries argtypes generated from the header.  The host-side argument checks run before the
context is looked at or any device work is done, so they are tested here, without a device.  (What the calls compute is
tests/test_gpu_peers.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_peer_index", "xmap_peer_centre", "xmap_peer_rows", "xmap_ctx_peers"]


def test_peers_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert P["xmap_peer_index"] == [v, i64, i32] + [v] * 9
    assert P["xmap_peer_centre"] == [v, i32, v, v, v]
    assert P["xmap_debug_sort_pairs"] == [v, v, v, i64, i32] and "xmap_debug_sort_pairs" in hipabi.EXPORTS
    assert P["xmap_peer_rows"] == [v, i64, v, i64, v, v, v, i32, i32, i32, i32, i64, i32] + [v] * 5 + [i64] + [v] * 6
    assert P["xmap_ctx_peers"] == [v, i32, i64, v, i32, i32, i32, i32] + [v] * 6
    assert hipabi.lib.xmap_version() >= 116
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n


def test_the_constants_match_the_header():
    from xmap.engine import hipabi
    consts = hipabi.header_constants(prefixes=("XMAP_PEERS_",))
    assert consts == {"PEERS_SAME": 1, "PEERS_KEEP_SELF": 2, "PEERS_CENTRED": 4}
    assert {n: getattr(hipabi, n) for n in consts} == consts


def _coarse(**change):
    from xmap.engine import hipabi
    a = dict(source=0, n_top=4, flags=0, cap=1, min_common=1, floor=None)
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    query = np.arange(n_q, dtype=np.int32)
    outs = [np.full(n_q, 77, np.int32), np.full((n_q, n), 77, np.int32), np.full((n_q, n), 7.5), np.full((n_q, n), 77, np.int32)]
    stats = np.full(6, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    F = None if a["floor"] is None else ctypes.byref(hipabi.RecFilter(None, None, None, a["floor"]))
    rc = hipabi.lib.xmap_ctx_peers(None, a["source"], n_q, p(query), a["n_top"], a["flags"], a["cap"], a["min_common"],
                                   *([p(o) for o in outs] + [F, p(stats)]))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


BAD = [("n_top 0", dict(n_top=0), "n_top"), ("n_top 1025", dict(n_top=1025), "n_top"), ("cap 0", dict(cap=0), "cap"),
       ("min_common 0", dict(min_common=0), "min_common"), ("source 2", dict(source=2), "source"),
       ("an unknown flag", dict(flags=8), "flags"), ("a NaN floor", dict(floor=float("nan")), "min_score")]


@pytest.mark.parametrize("what,change,names", BAD, ids=[b[0] for b in BAD])
def test_the_coarse_call_checks_its_arguments_on_the_host(what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before the context is read (none exists without a device): the outputs
    keep every byte"""
    from xmap.engine import hipabi
    rc, msg, unchanged = _coarse(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


def test_good_arguments_reach_the_context_check():
    """the same call with valid values fails only on the context it was not given"""
    from xmap.engine import hipabi
    for change in (dict(), dict(n_top=1024, cap=7, min_common=3, flags=hipabi.PEERS_KEEP_SELF | hipabi.PEERS_CENTRED, source=1,
                               floor=0.25)):
        rc, msg, unchanged = _coarse(**change)
        assert rc == hipabi.ERR_ARG and "have_rec" in msg and unchanged, msg
