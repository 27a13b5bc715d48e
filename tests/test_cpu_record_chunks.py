"""The chunk plan of the calls that take max_records (peers, user-kNN top-N, item fold-in, related items, fused lists, shelves) is
one host function, pr_plan_chunks of sorted_runs.h; xmap_debug_record_chunks calls it and nothing else -- no stream, no device --
so the plan is tested here against the statement's chunks (tests/shelf_statement.py), the clamp and the capacity error included:
the prefix sums are built here, nothing of 2^31 records is ever allocated."""
import ctypes
import os
import re

import numpy as np
import pytest

import shelf_statement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "xmap_debug_record_chunks"
DEFAULT = 1 << 22           # the library's default chunk
LIMIT = 2147483646          # the most records of a chunk of several queries


def _plan(records, max_records, L=None):
    """(rc, chunks [(q0, q1)], n_max, nq_max, message) of the hook for the records per query"""
    from xmap.engine import hipabi
    L = L or hipabi.lib
    n = len(records)
    rec = np.zeros(n + 1, np.int64)
    rec[1:] = np.cumsum(np.asarray(records, np.int64))
    cut = np.full(n + 1, -7, np.int64)
    out = np.full(3, -7, np.int64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = getattr(L, NAME)(n, p(rec), max_records, p(cut), p(out))
    msg = (L.xmap_last_error() or b"").decode()
    if rc:
        return rc, None, None, None, msg
    k = int(out[0])
    assert (cut[k + 1:] == -7).all()            # nothing behind the last border is written
    return rc, [(int(cut[j]), int(cut[j + 1])) for j in range(k)], int(out[1]), int(out[2]), msg


def _expected(records, max_records):
    ch = S.chunks(list(records), max_records)
    return ch, max([sum(records[a:b]) for a, b in ch], default=0), max([b - a for a, b in ch], default=0)


def test_the_hook_is_declared_exported_and_typed():
    hdr = open(os.path.join(ROOT, "include", "xmap_hip.h")).read()
    from xmap.engine import hipabi
    assert re.search(r"\bint\s+%s\s*\(" % NAME, hdr), "%s is not declared in the header" % NAME
    assert NAME in hipabi.EXPORTS
    i64, v = ctypes.c_int64, ctypes.c_void_p
    assert hipabi.PROTOTYPES[NAME] == [i64, v, i64, v, v]           # no stream: the hook does no device work
    for L in (hipabi.lib, hipabi.xlib()):
        f = getattr(L, NAME)
        assert f.argtypes is not None and list(f.argtypes) == hipabi.PROTOTYPES[NAME]
        assert f.restype is ctypes.c_int
    assert hipabi.lib.xmap_version() >= 123
    assert hipabi.xlib().xmap_version() == hipabi.lib.xmap_version()


CASES = [([], (1, 5, 0)), ([0, 0, 0], (1, 5, 0)), ([5], (1, 5)), ([3, 3, 3], (1, 2, 3, 5, 6, 8, 9, 10)), ([1, 0, 0, 7, 0, 2], (7, 8))]


@pytest.mark.parametrize("records,limits", CASES, ids=[str(c[0]) for c in CASES])
def test_the_plan_is_the_statement(records, limits):
    """borders, the most records and the most queries of a chunk; 6 and 9 of [3, 3, 3] are the equal-to-limit boundaries,
    [1, 0, 0, 7, 0, 2] has empty queries inside and at the ends of chunks and (at 7) a query that fills a chunk alone"""
    from xmap.engine import hipabi
    for m in limits:
        want = _expected(records, m if m > 0 else DEFAULT)
        for L in (hipabi.lib, hipabi.xlib()):
            rc, ch, n_max, nq_max, msg = _plan(records, m, L)
            assert rc == 0, msg
            assert (ch, n_max, nq_max) == want, (records, m)


def test_a_query_over_the_limit_is_a_chunk_of_its_own():
    rc, ch, n_max, nq_max, _ = _plan([1, 0, 0, 7, 0, 2], 3)
    assert rc == 0 and (3, 4) in ch and n_max == 7
    assert (ch, n_max, nq_max) == _expected([1, 0, 0, 7, 0, 2], 3)


def test_zero_selects_the_default_chunk():
    """2^22 records in two queries fit one default chunk, one record more does not"""
    half = DEFAULT // 2
    for records in ([half, half], [half, half + 1], [half, half, 1]):
        rc, ch, n_max, nq_max, msg = _plan(records, 0)
        assert rc == 0, msg
        assert (ch, n_max, nq_max) == _expected(records, DEFAULT)
    assert _plan([half, half], 0)[1] == [(0, 2)] and _plan([half, half + 1], 0)[1] == [(0, 1), (1, 2)]


def test_any_max_records_is_clamped_below_2_to_the_31():
    """2^31 - 1 records in two queries: one chunk would not fit the int positions of the sort, so the limit 2^40 is cut to 2^31 - 2
    and the two split"""
    rc, ch, n_max, nq_max, msg = _plan([LIMIT, 1], 1 << 40)
    assert rc == 0, msg
    assert ch == [(0, 1), (1, 2)] and n_max == LIMIT and nq_max == 1
    rc, ch, n_max, nq_max, msg = _plan([LIMIT - 1, 1], 1 << 40)     # exactly the limit: one chunk
    assert rc == 0 and ch == [(0, 2)] and n_max == LIMIT and nq_max == 2, msg


@pytest.mark.parametrize("max_records", [0, 1, 1 << 40])
@pytest.mark.parametrize("records,q", [([LIMIT + 1], 0), ([1, LIMIT + 1], 1)], ids=["query 0", "query 1"])
def test_a_query_of_2_to_the_31_records_is_a_capacity_error(records, q, max_records):
    from xmap.engine import hipabi
    rc, _, _, _, msg = _plan(records, max_records)
    assert rc == hipabi.ERR_CAPACITY
    assert "query %d expands to %d records" % (q, LIMIT + 1) in msg and "fewer than 2^31" in msg, msg
