"""k_rec_select (csrc/stage_e.hip) through xmap_rec_select on the designed rows of tests/rec_select_rows.py against the NumPy
statement there: every family x storage order x keep, the same rows under other row partitions, and misuse through the
return code.  Everything is compared exactly: integers as integers, doubles through their uint64 views.  The outputs are
pre-filled with a byte pattern and allocated GUARD elements longer than [I][keep]: every element of the result is
overwritten and the guard keeps the pattern.  The census of the inputs is tests/test_cpu_rec_select_rows.py's."""
import ctypes as C

import numpy as np
import pytest

import rec_select_rows as rr
from rec_select_rows import FAMILIES, KEEPS, ORDERS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
FILL = 0xA5                                     # every byte of the outputs before a call
FILL_I32 = int(np.frombuffer(bytes([FILL] * 4), np.int32)[0])
FILL_U64 = int(np.frombuffer(bytes([FILL] * 8), np.uint64)[0])


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


def _dev(a):
    import torch
    a = np.array(a, order="C")              # (a copy: the designed arrays are read-only)
    return torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(DEV)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


class DevRows(object):
    def __init__(self, R):
        self.R, self.row_ptr, self.col, self.sim, self.ls = R, _dev(R.row_ptr), _dev(R.col), _dev(R.sim), _dev(R.ls)


def dev_select(D, keep, n_items=None, shape_keep=None):
    """xmap_rec_select on device copies -> (rc, cnt, col, sim, ls) as the flat host arrays WITH their guards: int32, int32 and
    the uint64 views of the two double outputs.  shape_keep sizes the outputs where keep itself is refused."""
    import torch
    from xmap.engine import hipabi as abi
    I = D.R.I if n_items is None else n_items
    k = keep if shape_keep is None else shape_keep
    n = D.R.I * k + GUARD
    cnt = torch.full(((D.R.I + GUARD) * 4,), FILL, dtype=torch.uint8, device=DEV).view(torch.int32)
    col = torch.full((n * 4,), FILL, dtype=torch.uint8, device=DEV).view(torch.int32)
    sim, ls = [torch.full((n * 8,), FILL, dtype=torch.uint8, device=DEV).view(torch.float64) for _ in range(2)]
    rc = abi.lib.xmap_rec_select(_stream(), abi.i32(I), abi.vp(D.row_ptr), abi.vp(D.col), abi.vp(D.sim), abi.vp(D.ls), abi.i32(keep),
                                 abi.vp(cnt), abi.vp(col), abi.vp(sim), abi.vp(ls))
    torch.cuda.synchronize()
    return (rc, cnt.cpu().numpy(), col.cpu().numpy(), sim.cpu().numpy().view(np.uint64), ls.cpu().numpy().view(np.uint64))


def untouched(out):
    _, cnt, col, sim, ls = out
    return bool(np.all(cnt == FILL_I32) and np.all(col == FILL_I32) and np.all(sim == FILL_U64) and np.all(ls == FILL_U64))


def result_of(out, I, keep):
    """the result proper, after the checks on what lies around it: the guards keep the pattern"""
    rc, cnt, col, sim, ls = out
    assert rc == 0
    assert np.all(cnt[I:] == FILL_I32) and np.all(col[I * keep:] == FILL_I32), "guard"
    assert np.all(sim[I * keep:] == FILL_U64) and np.all(ls[I * keep:] == FILL_U64), "guard"
    return (cnt[:I], col[:I * keep].reshape(I, keep), sim[:I * keep].reshape(I, keep).view(np.float64),
            ls[:I * keep].reshape(I, keep).view(np.float64))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("family", FAMILIES)
def test_designed_rows_equal_the_statement(family, order):
    R = rr.design(family, order)
    D = DevRows(R)
    for keep in KEEPS:
        got = result_of(dev_select(D, keep), R.I, keep)
        want = rr.statement(R, keep)
        # (the statement's padding is -1 / 0.0 / 0.0 and its counts are in [0, keep]: equality with it means every element
        # of [I][keep] and of cnt[I] was overwritten -- no int32 of the pattern is a count or -1, no double of it is 0.0)
        assert rr.same(got, want), (family, order, keep, rr.rows_that_differ(got, want))


@pytest.mark.parametrize("family", FAMILIES)
def test_other_row_partitions(family):
    """a row's result does not depend on the rows around it: the 41-chunk row alone (one wave of one block) and all rows
    in reverse row order (other waves, other blocks, the single row of the last block now an empty one of the other end)"""
    for order in ("abs_asc", "shuffle"):
        R = rr.design(family, order)
        long_row = int(np.argmax(np.diff(R.row_ptr)))
        for which in ([long_row], np.arange(R.I)[::-1]):
            P = rr.take_rows(R, which)
            D = DevRows(P)
            for keep in KEEPS:
                got = result_of(dev_select(D, keep), P.I, keep)
                want = tuple(a[np.asarray(which)] for a in rr.statement(R, keep))
                assert rr.same(got, want), (family, order, keep, rr.rows_that_differ(got, want))


def test_misuse_is_a_return_code():
    """keep outside [1, 64] is XMAP_ERR_ARG, no row is XMAP_OK; nothing is launched, the outputs keep their pattern"""
    from xmap.engine import hipabi as abi
    D = DevRows(rr.design("levels4", "shuffle"))
    for keep in (0, 65):
        out = dev_select(D, keep, shape_keep=65)
        assert out[0] == abi.ERR_ARG and untouched(out), keep
    out = dev_select(D, 10, n_items=0)
    assert out[0] == 0 and untouched(out)
