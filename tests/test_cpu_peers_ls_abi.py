"""xmap_peer_rows_ls and xmap_ctx_peers_ls are part of the C ABI: include/xmap_hip.h declares them, both libraries export them and
the binding carries argtypes generated from the header.  Their host-side argument checks run before any device work, so they
are tested here, without a device.  (What the calls compute is tests/test_gpu_user_sim.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_peer_rows_ls", "xmap_ctx_peers_ls"]


def test_the_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert P["xmap_peer_rows_ls"] == P["xmap_peer_rows"][:23] + [v] + P["xmap_peer_rows"][23:]      # out_ls behind out_common
    assert P["xmap_ctx_peers_ls"] == P["xmap_ctx_peers"][:12] + [v] + P["xmap_ctx_peers"][12:]
    assert hipabi.lib.xmap_version() >= 118
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    assert X.xmap_version() == hipabi.lib.xmap_version()
    for n in NAMES:
        assert hasattr(X, n), n


def _outs(n_q, n):
    return [np.full(n_q, 77, np.int32), np.full((n_q, n), 77, np.int32), np.full((n_q, n), 7.5), np.full((n_q, n), 77, np.int32),
            np.full((n_q, n), 7.5)]


def _fine(**change):
    """xmap_peer_rows_ls with host memory behind every pointer: a bad argument returns before any of it is read"""
    from xmap.engine import hipabi
    a = dict(n_top=4, cap=1, min_common=1, flags=0, null_ls=False)
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    query = np.arange(n_q, dtype=np.int32)
    ptr, item, rating = np.zeros(4, np.int64), np.zeros(1, np.int32), np.zeros(1)
    outs, stats = _outs(n_q, n), np.full(6, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = hipabi.lib.xmap_peer_rows_ls(None, n_q, p(query), 3, p(ptr), p(item), p(rating), a["flags"], a["n_top"], a["cap"], a["min_common"],
                                      3, 1, None, p(ptr), p(item), p(rating), p(rating), 0, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]),
                                      None if a["null_ls"] else p(outs[4]), None, p(stats))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


def _coarse(**change):
    from xmap.engine import hipabi
    a = dict(source=0, n_top=4, flags=0, cap=1, min_common=1, null_ls=False)
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    query = np.arange(n_q, dtype=np.int32)
    outs, stats = _outs(n_q, n), np.full(6, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = hipabi.lib.xmap_ctx_peers_ls(None, a["source"], n_q, p(query), a["n_top"], a["flags"], a["cap"], a["min_common"], p(outs[0]),
                                      p(outs[1]), p(outs[2]), p(outs[3]), None if a["null_ls"] else p(outs[4]), None, p(stats))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


BAD = [("n_top 0", dict(n_top=0), "n_top"), ("n_top 1025", dict(n_top=1025), "n_top"), ("cap 0", dict(cap=0), "cap"),
       ("a NULL out_ls", dict(null_ls=True), "out_ls")]


@pytest.mark.parametrize("call", [_fine, _coarse], ids=["xmap_peer_rows_ls", "xmap_ctx_peers_ls"])
@pytest.mark.parametrize("what,change,names", BAD, ids=[b[0] for b in BAD])
def test_the_calls_check_their_arguments_on_the_host(call, what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before any device work: the sentinel-filled outputs keep every byte"""
    from xmap.engine import hipabi
    rc, msg, unchanged = call(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


def test_good_arguments_reach_the_context_check():
    from xmap.engine import hipabi
    rc, msg, unchanged = _coarse(n_top=1024, cap=7, min_common=3, flags=hipabi.PEERS_KEEP_SELF | hipabi.PEERS_CENTRED, source=1)
    assert rc == hipabi.ERR_ARG and "have_rec" in msg and unchanged, msg
