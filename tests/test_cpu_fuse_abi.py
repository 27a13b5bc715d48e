"""The fused-list calls are part of the C ABI: include/xmap_hip.h declares xmap_fuse_rows, xmap_ctx_fuse and
xmap_ctx_recommend_hybrid; both libraries export them and the binding carries argtypes generated from the header.  The host-side
argument checks of the coarse calls run before the context is looked at or any device work is done, so they are tested here,
without a device.  (What the calls compute is tests/test_gpu_fuse.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_fuse_rows", "xmap_ctx_fuse", "xmap_ctx_recommend_hybrid"]
NAN, INF = float("nan"), float("inf")


def test_fuse_entry_points_are_declared_exported_typed_and_versioned():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64, d = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert P["xmap_fuse_rows"] == [v, i64, i32, v, i32, i32, d, i32, i32, i64] + [v] * 5
    assert P["xmap_ctx_fuse"] == [v, i64, i32, v, i32, i32, d, i32, i32] + [v] * 5
    assert P["xmap_ctx_recommend_hybrid"] == [v, i32, i64, v, i32, i32, i32, i32, v, i32] + [i32] * 7 + [d, d, i32, d, i32] + [v] * 6
    assert hipabi.lib.xmap_version() >= 121
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n
    assert X.xmap_version() == hipabi.lib.xmap_version()


def test_the_constants_and_the_structure_match_the_header():
    from xmap.engine import hipabi
    consts = hipabi.header_constants(prefixes=("XMAP_FUSE_",))
    assert consts == {"FUSE_RRF": 0, "FUSE_SUM": 1, "FUSE_MEAN": 2, "FUSE_MAX_LISTS": 16, "FUSE_BLOCK_RECORDS": 2048}
    assert {n: getattr(hipabi, n) for n in consts} == consts
    assert hipabi.FUSE_HOW == {"rrf": 0, "sum": 1, "mean": 2}
    # xmap_fuse_list is an anonymous typedef (it holds doubles; the named structs of the header are int and pointer members only)
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "xmap_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*xmap_fuse_list\s*;", hdr).group(1)
    members = [" ".join(m.split()) for m in body.split(";") if m.strip()]
    assert members == ["const int32_t *cnt", "const int32_t *item", "const double *score", "int32_t width", "double weight"]
    assert [(n, t) for n, t in hipabi.FuseList._fields_] == [("cnt", ctypes.c_void_p), ("item", ctypes.c_void_p), ("score", ctypes.c_void_p),
                                                             ("width", ctypes.c_int32), ("weight", ctypes.c_double)]
    assert ctypes.sizeof(hipabi.FuseList) == 40 and "xmap_fuse_list" not in hipabi.header_structs()


def test_the_makefile_builds_the_new_file():
    mk = open(os.path.join(ROOT, "x-map_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bstage_e_fuse\.hip\b", mk, flags=re.M)


def _p(x):
    return None if x is None else x.ctypes.data_as(ctypes.c_void_p)


def _fuse(**change):
    from xmap.engine import hipabi
    a = dict(n_query=3, n_lists=2, widths=[4, 5], weights=[1.0, 2.0], scores=[True, True], n_ids=9, how=0, rrf_c=60.0, min_lists=1, n_top=4,
             null=())
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    arr = (hipabi.FuseList * 2)()
    keep = []
    for l in range(2):
        w = max(1, min(a["widths"][l], 8))
        t = [np.full(n_q, 2, np.int32), np.arange(n_q * w, dtype=np.int32).reshape(n_q, w) % 9, np.ones((n_q, w)) if a["scores"][l] else None]
        keep.append(t)
        p = [None if (x is None or (l, k) in a["null"]) else x.ctypes.data for k, x in enumerate(t)]
        arr[l] = hipabi.FuseList(p[0], p[1], p[2], a["widths"][l], a["weights"][l])
    outs = [np.full(n_q, 77, np.int32), np.full((n_q, n), 77, np.int32), np.full((n_q, n), 7.5), np.full((n_q, n), 77, np.int32)]
    stats = np.full(5, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    rc = hipabi.lib.xmap_ctx_fuse(None, a["n_query"], a["n_lists"], None if "lists" in a["null"] else ctypes.cast(arr, ctypes.c_void_p),
                                  a["n_ids"], a["how"], a["rrf_c"], a["min_lists"], a["n_top"],
                                  *([None if ("out", k) in a["null"] else _p(o) for k, o in enumerate(outs)] + [_p(stats)]))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    del keep
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


BAD_FUSE = [("n_lists 0", dict(n_lists=0), "n_lists"), ("n_lists 17", dict(n_lists=17), "n_lists"), ("no lists", dict(null=["lists"]), "lists"),
            ("width 0", dict(widths=[4, 0]), "lists[1].width"), ("width 1025", dict(widths=[1025, 5]), "lists[0].width"),
            ("a NaN weight", dict(weights=[NAN, 1.0]), "lists[0].weight"), ("an inf weight", dict(weights=[1.0, -INF]), "lists[1].weight"),
            ("rrf_c -1", dict(rrf_c=-1.0), "rrf_c"), ("rrf_c NaN", dict(rrf_c=NAN), "rrf_c"), ("rrf_c inf", dict(rrf_c=INF), "rrf_c"),
            ("how -1", dict(how=-1), "how"), ("how 3", dict(how=3), "how"), ("min_lists 0", dict(min_lists=0), "min_lists"),
            ("min_lists 3", dict(min_lists=3), "min_lists"), ("n_top 0", dict(n_top=0), "n_top"), ("n_top 1025", dict(n_top=1025), "n_top"),
            ("no score under sum", dict(how=1, scores=[True, False]), "lists[1].score"),
            ("no score under mean", dict(how=2, scores=[False, True]), "lists[0].score"),
            ("n_query above 2^28", dict(n_query=(1 << 28) + 1), "n_query"), ("n_query -1", dict(n_query=-1), "n_query"),
            ("n_ids -1", dict(n_ids=-1), "n_ids"), ("no cnt", dict(null=[(1, 0)]), "lists[1].cnt"), ("no item", dict(null=[(0, 1)]), "lists[0].item"),
            ("no out_cnt", dict(null=[("out", 0)]), "out_cnt"), ("no out_id", dict(null=[("out", 1)]), "out_id"),
            ("no out_score", dict(null=[("out", 2)]), "out_score"), ("no out_lists", dict(null=[("out", 3)]), "out_lists")]


@pytest.mark.parametrize("what,change,names", BAD_FUSE, ids=[b[0] for b in BAD_FUSE])
def test_fuse_checks_its_arguments_on_the_host(what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before the context is read (none exists without a device): the outputs
    keep every byte"""
    from xmap.engine import hipabi
    rc, msg, unchanged = _fuse(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


def test_good_fuse_arguments_reach_the_context_check():
    from xmap.engine import hipabi
    for change in (dict(), dict(how=1, weights=[-1.0, 0.0], min_lists=2, n_top=1024), dict(how=0, scores=[False, False], rrf_c=0.0),
                   dict(how=2, widths=[1024, 1], n_top=1), dict(n_query=0, null=[("out", 0), ("out", 1), ("out", 2), ("out", 3), (0, 0), (1, 1)])):
        rc, msg, unchanged = _fuse(**change)
        assert rc == hipabi.ERR_ARG and msg.endswith("bad argument: c") and unchanged, msg


def _hybrid(**change):
    from xmap.engine import hipabi
    a = dict(source=0, n_query=3, n_top=4, pool_i=8, rank_by=0, tflags=0, n_w=5, pool_u=8, n_nb=6, pf=0, cap=1, mc=1, uflags=0, ms=1, wi=1.0,
             wu=1.0, how=0, rrf_c=60.0, min_lists=1, floor=None, no_query=False)
    a.update(change)
    n_q, n = 3, max(1, min(int(a["n_top"]), 8))
    q, w = np.arange(n_q, dtype=np.int32), np.ones(5)
    outs = [np.full(n_q, 77, np.int32), np.full((n_q, n), 77, np.int32), np.full((n_q, n), 7.5), np.full((n_q, n), 77, np.int32)]
    stats = np.full(17, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    F = None if a["floor"] is None else ctypes.byref(hipabi.RecFilter(None, None, None, a["floor"]))
    rc = hipabi.lib.xmap_ctx_recommend_hybrid(None, a["source"], a["n_query"], None if a["no_query"] else _p(q), a["n_top"], a["pool_i"],
                                              a["rank_by"], a["tflags"], _p(w), a["n_w"], a["pool_u"], a["n_nb"], a["pf"], a["cap"], a["mc"],
                                              a["uflags"], a["ms"], a["wi"], a["wu"], a["how"], a["rrf_c"], a["min_lists"], F,
                                              *([_p(o) for o in outs] + [_p(stats)]))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


BAD_HYBRID = [("n_top 0", dict(n_top=0), "n_top"), ("n_top 1025", dict(n_top=1025), "n_top"), ("pool_items 0", dict(pool_i=0), "n_pool_items"),
              ("pool_items 65", dict(pool_i=65), "n_pool_items"), ("rank_by 2", dict(rank_by=2), "rank_by"),
              ("an unknown top-N flag", dict(tflags=2), "topn_flags"), ("no decay table", dict(n_w=0), "n_w"),
              ("pool_users 0", dict(pool_u=0), "n_pool_users"), ("pool_users 1025", dict(pool_u=1025), "n_pool_users"),
              ("n_nb 0", dict(n_nb=0), "n_nb"), ("n_nb 1025", dict(n_nb=1025), "n_nb"), ("the library's peer flag", dict(pf=1), "peer_flags"),
              ("cap 0", dict(cap=0), "cap"), ("min_common 0", dict(mc=0), "min_common"), ("an unknown user-kNN flag", dict(uflags=4), "uknn_flags"),
              ("min_support 0", dict(ms=0), "min_support"), ("a NaN item weight", dict(wi=NAN), "w_items"),
              ("an inf user weight", dict(wu=INF), "w_users"), ("how 3", dict(how=3), "how"), ("rrf_c -1", dict(rrf_c=-1.0), "rrf_c"),
              ("rrf_c NaN", dict(rrf_c=NAN), "rrf_c"), ("min_lists 0", dict(min_lists=0), "min_lists"), ("min_lists 3", dict(min_lists=3), "min_lists"),
              ("an item fold-in", dict(source=2), "source"), ("source 3", dict(source=3), "source"), ("a NaN floor", dict(floor=NAN), "min_score"),
              ("no queries array", dict(no_query=True), "query_user"), ("n_query -1", dict(n_query=-1), "n_query")]


@pytest.mark.parametrize("what,change,names", BAD_HYBRID, ids=[b[0] for b in BAD_HYBRID])
def test_hybrid_checks_its_arguments_on_the_host(what, change, names):
    from xmap.engine import hipabi
    rc, msg, unchanged = _hybrid(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


def test_good_hybrid_arguments_reach_the_context_check():
    from xmap.engine import hipabi
    for change in (dict(), dict(source=1, n_top=1024, pool_i=64, rank_by=1, tflags=1, pool_u=1024, n_nb=1024, pf=6, cap=9, mc=2, uflags=3, ms=4,
                               wi=-0.5, wu=0.0, how=2, rrf_c=0.0, min_lists=2, floor=0.5), dict(how=1, n_top=1, pool_i=1, pool_u=1, n_nb=1)):
        rc, msg, unchanged = _hybrid(**change)
        assert rc == hipabi.ERR_ARG and "have_gen" in msg and unchanged, msg


def test_engine_fuse_checks_its_arguments():
    import torch
    from types import SimpleNamespace
    from xmap.engine import device
    eng = device.Engine(SimpleNamespace(device=torch.device("cpu"), n_items=9))
    cnt, item, score = torch.zeros(3, dtype=torch.int32), torch.zeros((3, 4), dtype=torch.int32), torch.zeros((3, 4), dtype=torch.float64)
    good = [(cnt, item, score), (cnt, item, score, "more", "members")]
    for lists, kw in ((good, dict(n_top=0)), (good, dict(n_top=1025)), (good, dict(how="borda")), (good, dict(weights=[1.0])),
                      (good, dict(weights=[1.0, NAN])), (good, dict(weights=[INF, 1.0])), (good, dict(rrf_c=-1.0)), (good, dict(rrf_c=NAN)),
                      (good, dict(min_lists=0)), (good, dict(min_lists=3)), (good, dict(n_ids=-1)), (good, dict(max_records=-1)),
                      ([], dict()), (good * 9, dict()), ([(cnt, item, None)], dict(how="sum")), ([(cnt, item, None)], dict(how="mean")),
                      ([(cnt.long(), item, score)], dict()), ([(cnt, item.long(), score)], dict()), ([(cnt, item, score.float())], dict()),
                      ([(cnt[:2], item, score)], dict()), ([(cnt, item, score[:, :3])], dict()),
                      ([(cnt, torch.zeros((3, 1025), dtype=torch.int32), None)], dict())):
        a = dict(n_top=5)
        a.update(kw)
        with pytest.raises(ValueError):
            eng.fuse(lists, a.pop("n_top"), **a)


def test_the_session_checks_the_hybrid_arguments_before_any_device_work():
    from xmap.engine import session
    good = dict(n_nb=5)
    for bad in (dict(diversify=0.5), dict(fill="count"), dict(pool=20)):
        with pytest.raises(ValueError):
            session.evaluate_topn(None, [], 50, 10, 0.3, 10, hybrid=good, **bad)
    for hybrid in (dict(), dict(n_nb=5, borda=1), dict(n_nb=0), dict(n_nb=5, how="borda"), dict(n_nb=5, weights=(1.0,)),
                   dict(n_nb=5, pool_items=65), dict(n_nb=5, pool_users=1025), dict(n_nb=5, min_lists=3), dict(n_nb=5, rrf_c=-1.0)):
        with pytest.raises(ValueError):
            session.evaluate_topn(None, [], 50, 10, 0.3, 10, hybrid=hybrid)
    with pytest.raises(ValueError):
        session.evaluate_topn(None, [], 50, 10, 0.3, 65, hybrid=good)          # the evaluation takes lists of 1 .. 64
    with pytest.raises(TypeError):
        session.evaluate_topn(None, [], 50, 10, 0.3, 10, hybrid=good)          # good arguments reach the handle check
    assert session._hybrid_spec(10, 5)["weights"] == (1.0, 1.0) and session._hybrid_spec(10, 5)["pool_items"] == 64
    with pytest.raises(ValueError):
        session.fuse_lists([[("u", [("a", 1.0)])], [("v", [("a", 1.0)])]], 5)  # the results list different labels
    with pytest.raises(ValueError):
        session.fuse_lists([], 5)
