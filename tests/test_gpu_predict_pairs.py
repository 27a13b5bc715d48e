"""k_predict (csrc/stage_e.hip) through xmap_predict, called directly, on the designed pairs of tests/predict_pairs.py: per
decay table length n_w and alpha the status of every pair equals the statement's, plain and decay are bit-equal (doubles
through their uint64 views), and every output is written -- they are pre-filled with a byte pattern and allocated GUARD
elements longer than n_test; the guard keeps the pattern.  The census of the pairs is tests/test_cpu_predict_pairs.py's."""
import ctypes as C

import numpy as np
import pytest

import predict_pairs as pp
from predict_pairs import ALPHAS, N_WS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
FILL = 0xA5
FILL_I32 = int(np.frombuffer(bytes([FILL] * 4), np.int32)[0])
FILL_U64 = int(np.frombuffer(bytes([FILL] * 8), np.uint64)[0])


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.zeros(1, device="cuda")


@pytest.fixture(scope="module")
def uploaded():
    """the arrays of the case on the device, in the order of xmap_predict's parameters (one upload for every call)"""
    import torch
    A = pp.arrays()
    return [torch.from_numpy(np.array(a, order="C")).to(DEV) for a in (A.tu, A.ti, A.nb_ptr, A.nb_item, A.nb_sim, A.rt_ptr, A.rt_user,
                                                                        A.rt_rating, A.rt_time, A.avg)]


def dev_predict(d, alpha, n_w, n_test=pp.N_TEST, table=None):
    """-> (rc, status int32, plain, decay as uint64), the flat host arrays WITH their guards"""
    import torch
    from xmap.engine import hipabi as abi
    w = torch.from_numpy(pp.wtab(alpha, n_w if table is None else table)).to(DEV)
    n = pp.N_TEST + GUARD
    plain, decay = [torch.full((n * 8,), FILL, dtype=torch.uint8, device=DEV).view(torch.float64) for _ in range(2)]
    status = torch.full((n * 4,), FILL, dtype=torch.uint8, device=DEV).view(torch.int32)
    rc = abi.lib.xmap_predict(C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream), abi.i64(n_test), *[abi.vp(x) for x in d],
                              abi.vp(w), abi.i32(n_w), abi.vp(plain), abi.vp(decay), abi.vp(status))
    torch.cuda.synchronize()
    return rc, status.cpu().numpy(), plain.cpu().numpy().view(np.uint64), decay.cpu().numpy().view(np.uint64)


def untouched(out):
    _, status, plain, decay = out
    return bool(np.all(status == FILL_I32) and np.all(plain == FILL_U64) and np.all(decay == FILL_U64))


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n_w", N_WS)
def test_designed_pairs_equal_the_statement(uploaded, n_w, alpha):
    c = pp.case()
    A = pp.arrays()
    rc, status, plain, decay = dev_predict(uploaded, alpha, n_w)
    assert rc == 0
    T = pp.N_TEST
    assert np.all(status[T:] == FILL_I32) and np.all(plain[T:] == FILL_U64) and np.all(decay[T:] == FILL_U64), "guard"
    want_status, want_plain, want_decay = pp.expected(alpha, n_w)
    # (no status is the pattern's int32 and no result its double: equality means that every output was written)
    bad = np.nonzero(status[:T] != want_status)[0]
    assert len(bad) == 0, [(c.tags[A.pair_of[t]], int(status[t]), int(want_status[t])) for t in bad[:8]]
    bad = np.nonzero((plain[:T] != pp.bits(want_plain)) | (decay[:T] != pp.bits(want_decay)))[0]
    assert len(bad) == 0, [(c.tags[A.pair_of[t]], float(plain[t:t + 1].view(np.float64)[0]), float(want_plain[t]),
                            float(decay[t:t + 1].view(np.float64)[0]), float(want_decay[t])) for t in bad[:8]]


def test_misuse_is_a_return_code(uploaded):
    """a decay table of one entry is XMAP_ERR_ARG, no pair is XMAP_OK; nothing is launched, the outputs keep their pattern"""
    from xmap.engine import hipabi as abi
    out = dev_predict(uploaded, 0.05, 1, table=2)
    assert out[0] == abi.ERR_ARG and untouched(out)
    out = dev_predict(uploaded, 0.05, 66, n_test=0)
    assert out[0] == 0 and untouched(out)
