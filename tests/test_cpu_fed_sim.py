"""Caller-fed similarity matrices over the whole fp64 range (Engine.sim_from_host, session.sim_from_records,
ExtendSim.sim_extend hand stage B values stage A never produces): the FAMILIES below, and the conditions the CPU oracle's
results on them have to meet before a comparison with the GPU (tests/test_gpu_fed_sim.py) says anything.

The kept-pair structure (row_ptr, col, nij, info) is the oracle's own stage A of one small input; sim and mutu are replaced
per UNORDERED pair from a hash of (min(i, j), max(i, j), seed), so the matrix stays symmetric bit for bit (k_reverse tests
"b lists a" on a's own entry for b).  mutu is drawn from MUTU, the sign is random, the mantissa is 1 + 20 random bits:

  family   exponent of |sim|                                  also                       xmap_edge_ranges must say
  in       -399 .. 368                                        one pair in 16 is +-0.0    1
  ties     -399 .. 361 in steps of 95, mantissa exactly 1.0   --                         1
  tiny     -1074 .. -432 (subnormals included)                --                         0
  huge     401 .. 700                                         --                         0
  mixed    -1074 .. 700                                       one pair in 16 is +-0.0    0

|sim| < 2^369 times a mutuality < 2^31 stays below 2^400 and 2^-399 times a mutuality >= 1 above 2^-400: `in` and `ties`
meet the precondition of the bare division (csrc/paths4.hip: k_edge_ranges) on every pair; `tiny` (< 2^-431 * 2^31) and
`huge` violate it on every pair.  The upper exponent 700 keeps every sum of s_p * c_p finite: frac = mutu / (n_i + n_j -
n_ij) exceeds 1 for the large mutualities, a path weight reaches 2^155.
"""
import functools

import numpy as np
import pytest

from golden_util import CAP, METHODS

K = 5
SEED = 10       # (a seed at which both methods yield exactly-zero X-Sims for `in` and subnormal ones for `tiny`: few inputs do)
MUTU = np.array([1, 2, 3, 7, 1 << 15, (1 << 31) - 1], np.int64)
#            exponents (lo, hi, step), random mantissa, one pair in 16 is a zero, the range check's answer
FAMILIES = dict(
    **{"in": (-399, 368, 1, True, True, 1)},
    ties=(-399, 361, 95, False, False, 1),
    tiny=(-1074, -432, 1, True, False, 0),
    huge=(401, 700, 1, True, False, 0),
    mixed=(-1074, 700, 1, True, True, 0))


def fast_div_ok(sim, mutu):
    """the precondition of the bare division, as k_edge_ranges states it: every entry has a mutuality >= 1 and a product
    |sim * mutu| that is zero or strictly inside (2^-400, 2^400)"""
    with np.errstate(all="ignore"):
        m = np.asarray(mutu).astype(np.float64)
        sm = np.abs(np.asarray(sim, np.float64) * m)
        return int(bool(np.all(m >= 1.0) and np.all((sm == 0.0) | ((sm > 2.0 ** -400) & (sm < 2.0 ** 400)))))


def _mix(x):
    """splitmix64's finaliser on a uint64 array (wraps modulo 2^64)"""
    x = x.copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xbf58476d1ce4e5b9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94d049bb133111eb)
    x ^= x >> np.uint64(31)
    return x


def fed_values(family, rows, cols, seed=SEED):
    """(sim, mutu) of the directed pairs (rows[p], cols[p]): a function of the unordered pair and the seed alone"""
    e_lo, e_hi, e_step, rand_mant, zeros, _ = FAMILIES[family]
    a, b = np.minimum(rows, cols).astype(np.uint64), np.maximum(rows, cols).astype(np.uint64)
    h1 = _mix(((a << np.uint64(32)) | b) + np.uint64((0x9e3779b97f4a7c15 * (seed + 1)) & 0xffffffffffffffff))
    h2 = _mix(h1 + np.uint64(0x9e3779b97f4a7c15))
    mutu = MUTU[(h1 % np.uint64(6)).astype(np.int64)].astype(np.int32)
    sign = np.where((h1 >> np.uint64(8)) & np.uint64(1), -1.0, 1.0)
    mant = 1.0 + (((h1 >> np.uint64(16)) & np.uint64(0xfffff)).astype(np.float64) * 2.0 ** -20 if rand_mant else 0.0)
    n_exp = (e_hi - e_lo) // e_step + 1
    expo = e_lo + e_step * (h2 % np.uint64(n_exp)).astype(np.int64)
    sim = sign * np.ldexp(mant, expo.astype(np.int32))       # (below 2^-1022: rounded into the subnormals, never to zero)
    if zeros:
        sim = np.where((h2 >> np.uint64(40)) % np.uint64(16) == 0, sign * 0.0, sim)
    return np.ascontiguousarray(sim, np.float64), mutu


class Fed(object):
    pass


@functools.lru_cache(maxsize=None)
def fed_base(method):
    """the input and the oracle's own stage A of it: (ratings, oracle Train, row_ptr, col, nij, info)"""
    from oracle import xmap_oracle as xo
    from xmap.engine import synth
    r = synth.make_two_domain(5, 2000, 600, 600, overlap=0.1)
    T = xo.Train(r.user_ptr, r.item, r.rating, r.time, r.n_items, *r.item_attrs())
    So = xo.item_sim(T, method, CAP, nthreads=8)
    out = (r, T, So.row_ptr, So.col, So.nij, So.info)
    xo.sim_free(So)
    return out


@functools.lru_cache(maxsize=None)
def fed_case(family, method):
    """One fed matrix and everything the oracle makes of it (computed once per process, shared, never changed): the arrays
    (row_ptr, col, sim, mutu, nij, info), So = xo.sim_from_arrays of them, Xo = xo.extend(T, So, K), the private selection
    (n_top, choice, map) and the AlterEgo rows ae."""
    from oracle import xmap_oracle as xo
    c = Fed()
    c.family, c.method, c.k = family, method, K
    c.r, c.T, c.row_ptr, c.col, c.nij, c.info = fed_base(method)
    c.I = c.T.I
    c.rows = np.repeat(np.arange(c.I, dtype=np.int64), np.diff(c.row_ptr))
    c.sim, c.mutu = fed_values(family, c.rows, c.col.astype(np.int64))
    c.fast = FAMILIES[family][5]
    c.So = xo.sim_from_arrays(c.I, c.row_ptr, c.col, c.sim, c.mutu, c.nij, c.info)
    c.Xo = xo.extend(c.T, c.So, K)
    c.n_top, c.choice, c.map = xo.select(c.T, c.Xo, True, None)
    c.ae = xo.alterego(c.T, c.map)
    for a in (c.sim, c.mutu, c.row_ptr, c.col, c.nij, c.info, c.Xo.xs_val, c.Xo.xs_end, c.Xo.val, c.Xo.col, c.Xo.cnt, c.Xo.cls):
        a.setflags(write=False)
    return c


def listed_values(cnt, val):
    """(sim, mutu) of the valid entries of knn tables cnt [I][2], val [I][2][k][3]: what Engine.ext_tables_from_knn sees"""
    valid = np.arange(val.shape[2])[None, None, :] < cnt[:, :, None]
    return val[..., 0][valid], val[..., 1][valid]


def test_sim_from_arrays_is_the_oracles_own_matrix():
    """xo.extend on sim_from_arrays of the oracle's own stage-A arrays = xo.extend on the stage-A handle itself; freeing
    the borrowed matrix leaves NumPy's arrays alone"""
    from oracle import xmap_oracle as xo
    r, T, _, _, _, _ = fed_base("adjust_cosine")
    So = xo.item_sim(T, "adjust_cosine", CAP, nthreads=8)
    Sa = xo.sim_from_arrays(T.I, So.row_ptr, So.col, So.sim, So.mutu, So.nij, So.info)
    Xo, Xa = xo.extend(T, So, K), xo.extend(T, Sa, K)
    assert Xo.n_paths == Xa.n_paths > 10 ** 5
    for name in ("bb", "cls", "cnt", "xs_ptr", "xs_end", "xs_val"):
        assert np.array_equal(getattr(Xo, name), getattr(Xa, name)), name
    held = np.arange(K)[None, None, :] < Xo.cnt[:, :, None]          # (the oracle leaves the tail of a list unwritten)
    assert np.array_equal(Xo.col[held], Xa.col[held]) and np.array_equal(Xo.val[held], Xa.val[held])
    xo.ext_free(Xo); xo.ext_free(Xa)
    xo.sim_free(So)
    kept = Sa.sim.copy()
    xo.sim_free(Sa)
    assert Sa._h is None and np.array_equal(Sa.sim, kept)
    xo.sim_free(Sa)             # (a second call is a no-op, as for the library's own)
    E = xo.sim_from_arrays(3, np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(0, np.int32),
                           np.zeros(0, np.int32), np.zeros((3, 4)))
    assert len(E.col) == 0 and E._h.contents.I == 3
    xo.sim_free(E)


@pytest.mark.parametrize("method", METHODS)
def test_fed_matrix_is_symmetric_and_keeps_the_structure(method):
    c = fed_case("mixed", method)
    assert int(c.row_ptr[-1]) == len(c.sim) > 60000
    if method == "adjust_cosine":
        assert len(c.sim) == 66760
    back = {(int(a), int(b)): (s.tobytes(), int(m)) for a, b, s, m in zip(c.rows, c.col, c.sim, c.mutu)}
    assert all(back[(b, a)] == v for (a, b), v in back.items())          # sign of a zero included


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_fed_family_conditions(family, method):
    """what the oracle's results on a family must show for the GPU comparison to mean something"""
    c = fed_case(family, method)
    Xo = c.Xo
    e_lo, e_hi, e_step, rand_mant, zeros, fast = FAMILIES[family]
    # the values are what the table says
    nz = c.sim != 0.0
    with np.errstate(all="ignore"):
        expo = np.floor(np.log2(np.abs(c.sim[nz]))).astype(np.int64)
    assert expo.min() >= e_lo and expo.max() <= e_hi
    assert expo.min() <= e_lo + (e_hi - e_lo) // 50 and expo.max() >= e_hi - (e_hi - e_lo) // 50       # the range is used
    assert set(np.unique(c.mutu).tolist()) == set(MUTU.tolist())
    assert (c.sim[nz] > 0).any() and (c.sim[nz] < 0).any()
    if zeros:
        z = c.sim[~nz]
        assert 0.03 < len(z) / len(c.sim) < 0.1 and np.signbit(z).any() and not np.signbit(z).all()
    else:
        assert nz.all()
    if family == "ties":
        assert len(np.unique(np.abs(c.sim))) == 9
    # the range check's answer, from the arrays
    assert fast_div_ok(c.sim, c.mutu) == fast
    per_pair = np.array([fast_div_ok(c.sim[p:p + 1], c.mutu[p:p + 1]) for p in range(0, len(c.sim), 7)])
    if family in ("in", "ties"):
        assert per_pair.all()
    elif family in ("tiny", "huge"):
        assert not per_pair.any()
    else:
        assert 0.3 < 1.0 - per_pair.mean() < 0.7
    # the knn tables list a pair that decides the answer, so Engine.ext_tables_from_knn (which sees only listed pairs)
    # has to agree with xmap_edge_ranges (which sees every kept pair)
    assert fast_div_ok(*listed_values(Xo.cnt, Xo.val)) == fast
    # enough work, and finite results
    n_cand = np.diff(Xo.xs_ptr)
    assert Xo.n_paths >= 10 ** 5
    assert int((n_cand > 0).sum()) >= 400
    assert n_cand.max() > 10                               # a list the fused top-10 cuts
    assert np.isfinite(Xo.xs_val).all()
    tiny_f = np.finfo(np.float64).tiny
    if family in ("in", "ties"):
        assert int((Xo.xs_val == 0.0).sum()) >= 1
    if family == "tiny":
        assert int(((Xo.xs_val != 0.0) & (np.abs(Xo.xs_val) < tiny_f)).sum()) >= 1
        assert int(((c.sim != 0.0) & (np.abs(c.sim) < tiny_f)).sum()) >= 1000
    # the selection sees candidates and replaces items
    assert int((c.n_top > 0).sum()) >= 400 and int((c.map >= 0).sum()) >= 50
