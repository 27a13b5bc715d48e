"""The shelf calls are part of the C ABI: include/xmap_hip.h declares xmap_shelf_segments, xmap_shelf_rows, xmap_ctx_set_labels and
xmap_ctx_recommend_shelves; both libraries export them and the binding carries argtypes generated from the header.  The host-side
argument checks of the two coarse calls run before the context is looked at or any device work is done, so they are tested here,
without a device, with the host helpers of xmap/engine/labels.py.  (What the calls compute is tests/test_gpu_shelf.py's.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["xmap_shelf_segments", "xmap_shelf_rows", "xmap_ctx_set_labels", "xmap_ctx_recommend_shelves"]


def test_shelf_entry_points_are_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), "%s is not declared in the header" % n
        assert n in hipabi.EXPORTS and hasattr(hipabi.lib, n), n
        f = getattr(hipabi.lib, n)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[n], n
        assert f.restype is ctypes.c_int
    P, v, i32, i64, f64 = hipabi.PROTOTYPES, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert P["xmap_shelf_segments"] == [v, i64, v, v, v, v, v, f64, i32, i32, v, v, v, i32, i32, i32, i32, i32, i64] + [v] * 9
    filtered_up_to_n_w = P["xmap_topn_rows_filtered"][:19]
    assert filtered_up_to_n_w == [v, i64, v, i32, i32, i32, i64, i32, i32] + [v] * 9 + [i32]
    assert P["xmap_shelf_rows"] == filtered_up_to_n_w + [i32, v, v, v, i32, i32, i32, i64] + [v] * 8 + [v, v]
    assert P["xmap_ctx_set_labels"] == [v, i32, v, v]
    assert P["xmap_ctx_recommend_shelves"] == [v, i32, i64, v, i32, i32, i32, i32, v, i32, i32, i32, v] + [v] * 8 + [v, v]
    assert hipabi.lib.xmap_version() >= 122
    X = hipabi.xlib()           # the xcheck library is built from the same sources
    for n in NAMES:
        assert hasattr(X, n), n
    assert X.xmap_version() == hipabi.lib.xmap_version()


def test_the_constants_match_the_header():
    import shelf_statement as ss
    from xmap.engine import hipabi, labels
    consts = hipabi.header_constants(prefixes=("XMAP_SHELF_",))
    assert consts == {"SHELF_BY_BEST": 0, "SHELF_BY_MEAN": 1, "SHELF_BY_LABEL": 2, "SHELF_MAX_LABELS": 1 << 24}
    assert {n: getattr(hipabi, n) for n in consts} == consts
    assert hipabi.SHELF_BY == {"best": 0, "mean": 1, "label": 2}
    assert (ss.BEST, ss.MEAN, ss.LABEL, ss.MAX_LABELS) == (hipabi.SHELF_BY_BEST, hipabi.SHELF_BY_MEAN, hipabi.SHELF_BY_LABEL,
                                                           hipabi.SHELF_MAX_LABELS)
    assert labels.MAX_LABELS == hipabi.SHELF_MAX_LABELS


def test_the_makefile_builds_the_new_file():
    mk = open(os.path.join(ROOT, "x-map_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bstage_e_shelf\.hip\b", mk, flags=re.M)


def _p(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _shelves(**change):
    from xmap.engine import hipabi
    a = dict(source=0, n_query=3, n_shelf=2, n_top=4, rank_by=0, flags=0, shelf_by=0, min_fill=1, floor=None)
    a.update(change)
    n_q, ns, n = 3, max(1, min(int(a["n_shelf"]), 4)), max(1, min(int(a["n_top"]), 8))
    users, wtab = np.arange(3, dtype=np.int32), np.ones(4)
    outs = [np.full(n_q, 77, np.int32), np.full((n_q, ns), 77, np.int32), np.full((n_q, ns), 7.5), np.full((n_q, ns), 77, np.int32),
            np.full((n_q, ns), 77, np.int32), np.full((n_q, ns, n), 77, np.int32), np.full((n_q, ns, n), 7.5), np.full((n_q, ns, n), 7.5)]
    stats = np.full(10, 77, np.int64)
    before = [o.tobytes() for o in outs + [stats]]
    F = None if a["floor"] is None else ctypes.byref(hipabi.RecFilter(None, None, None, a["floor"]))
    rc = hipabi.lib.xmap_ctx_recommend_shelves(None, a["source"], a["n_query"], _p(users), a["n_shelf"], a["n_top"], a["rank_by"], a["flags"],
                                               _p(wtab), 4, a["shelf_by"], a["min_fill"], None, *([_p(o) for o in outs] + [F, _p(stats)]))
    msg = (hipabi.lib.xmap_last_error() or b"").decode()
    return rc, msg, [o.tobytes() for o in outs + [stats]] == before


def _set_labels(n_labels):
    from xmap.engine import hipabi
    lab_ptr, lab_id = np.asarray([0, 1, 2], np.int64), np.asarray([0, 0], np.int32)
    rc = hipabi.lib.xmap_ctx_set_labels(None, n_labels, _p(lab_ptr), _p(lab_id))
    return rc, (hipabi.lib.xmap_last_error() or b"").decode()


NAN, INF = float("nan"), float("inf")
BAD = [("n_shelf 0", dict(n_shelf=0), "n_shelf"), ("n_shelf 65", dict(n_shelf=65), "n_shelf"), ("n_top 0", dict(n_top=0), "n_top"),
       ("n_top 65", dict(n_top=65), "n_top"), ("rank_by 2", dict(rank_by=2), "rank_by"), ("shelf_by 3", dict(shelf_by=3), "shelf_by"),
       ("shelf_by -1", dict(shelf_by=-1), "shelf_by"), ("min_fill 0", dict(min_fill=0), "min_fill"),
       ("an unknown flag", dict(flags=2), "flags"), ("source 3", dict(source=3), "source"), ("a NaN floor", dict(floor=NAN), "min_score"),
       ("n_query -1", dict(n_query=-1), "n_query")]


@pytest.mark.parametrize("what,change,names", BAD, ids=[b[0] for b in BAD])
def test_recommend_shelves_checks_its_arguments_on_the_host(what, change, names):
    """XMAP_ERR_ARG from the check that names the argument, before the context is read (none exists without a device): the outputs
    keep every byte"""
    from xmap.engine import hipabi
    rc, msg, unchanged = _shelves(**change)
    assert rc == hipabi.ERR_ARG
    assert names in msg, msg
    assert unchanged


@pytest.mark.parametrize("n_labels", [-1, (1 << 24) + 1])
def test_set_labels_checks_the_number_of_labels_on_the_host(n_labels):
    from xmap.engine import hipabi
    rc, msg = _set_labels(n_labels)
    assert rc == hipabi.ERR_ARG and "n_labels" in msg, msg


def test_good_arguments_reach_the_context_check():
    """the same calls with valid values fail only on the context they were not given"""
    from xmap.engine import hipabi
    for change in (dict(), dict(source=2, n_shelf=64, n_top=64, rank_by=1, flags=hipabi.TOPN_KEEP_HELD, shelf_by=hipabi.SHELF_BY_LABEL,
                                min_fill=65, floor=0.25), dict(source=1, n_shelf=1, n_top=1, shelf_by=hipabi.SHELF_BY_MEAN, floor=-INF),
                   dict(n_query=0)):
        rc, msg, unchanged = _shelves(**change)
        assert rc == hipabi.ERR_ARG and "have_nb" in msg and unchanged, msg
    for n_labels in (0, 1, 1 << 24):
        rc, msg = _set_labels(n_labels)
        assert rc == hipabi.ERR_ARG and "have_ratings" in msg, msg


def test_label_csr_and_label_mask_by_hand():
    from xmap.engine.labels import label_csr, label_mask
    # unsorted and repeated names per item, an item without labels, an item index the space does not hold
    n, ptr, ids, names = label_csr({0: ["crime", "art", "crime"], 2: ["zen", "art"], 3: [], 9: ["ghost"], -1: ["ghost"]}, 4)
    assert names == ["art", "crime", "zen"] and n == 3
    assert ptr.dtype == np.int64 and ptr.tolist() == [0, 2, 2, 4, 4]
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1, 0, 2]
    # a sequence, one entry per item
    n, ptr, ids, names = label_csr([None, ("b", "a", "b", "a")], 2)
    assert (n, ptr.tolist(), ids.tolist(), names) == (2, [0, 0, 2], [0, 1], ["a", "b"])
    n, ptr, ids, names = label_csr({}, 3)
    assert (n, ptr.tolist(), ids.tolist(), names) == (0, [0, 0, 0, 0], [], [])
    with pytest.raises(ValueError):
        label_csr([["a"]], 2)
    import shelf_statement as ss
    n, ptr, ids, names = label_csr({0: ["crime", "art", "crime"], 2: ["zen", "art"]}, 4)
    assert ss.check_tables(4, n, ptr, ids) is None
    names = ["l%02d" % k for k in range(40)]
    w = label_mask(names, ["l33", "l00", "l31", "l00"])
    assert w.dtype == np.uint32 and w.tolist() == [(1 << 0) | (1 << 31), 1 << 1]
    assert label_mask(names, []).tolist() == [0, 0]
    with pytest.raises(ValueError):
        label_mask(names, ["l40"])
