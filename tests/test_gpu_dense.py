"""Dense item-factor variant (BASELINE.json configs[4]; no reference counterpart, parity unpinned by construction):
the MFMA contraction + fused row top-k against the oracle's fp32 fmaf chain, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def factors(seed, n, K, dup=0, zero_rows=()):
    rng = np.random.RandomState(seed)
    F = rng.standard_normal((n, K)).astype(np.float32)
    if dup:   # exact duplicates and negated copies: ties in |sim| that the index order has to break
        src = rng.randint(0, n, dup)
        dst = rng.randint(0, n, dup)
        F[dst] = F[src] * np.where(rng.rand(dup) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    for z in zero_rows:
        F[z] = 0.0
    return F


def engine():
    import torch
    assert torch.cuda.is_available()
    from xmap.engine import device, synth
    r = synth.make_two_domain(3, 60, 30, 30, overlap=0.5)
    R = device.DeviceRatings(r.user_ptr, r.item, r.rating, r.time, r.n_items, r.item_attrs(), "cuda:0")
    return device.Engine(R), r


@pytest.mark.parametrize("n_t,n_s,K,k", [
    (1, 1, 128, 1),            # single pair
    (5, 3, 128, 8),            # fewer sources than k: padded lists
    (129, 33, 64, 10),         # one row past a workgroup, one column past a tile
    (1000, 1500, 128, 50),     # ragged in both dimensions, headline k
    (300, 2049, 64, 64),       # maximum list length
    (257, 700, 128, 3),
])
def test_dense_topk_bit_exact(n_t, n_s, K, k):
    from oracle import xmap_oracle as xo
    eng, _ = engine()
    Ft = factors(n_t * 7 + 1, n_t, K, dup=n_t // 8, zero_rows=(0,) if n_t > 4 else ())
    Fs = factors(n_s * 5 + 2, n_s, K, dup=n_s // 4, zero_rows=(n_s // 2,) if n_s > 4 else ())
    Fs[: min(n_s, n_t) // 2] = Ft[: min(n_s, n_t) // 2]     # exact matches: |sim| = 1 candidates
    idx, val = eng.dense_topk(Ft, Fs, k)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    oi, ov = xo.dense_topk(xo.dense_normalize(Ft), xo.dense_normalize(Fs), k)
    assert np.array_equal(idx, oi)
    assert np.array_equal(val.view(np.uint32), ov.view(np.uint32))
    # size-independent properties: sorted by (|v| desc, idx asc), padding only at the tail
    a = np.abs(val)
    assert np.all(a[:, :-1] >= a[:, 1:]) if k > 1 else True
    tie = (a[:, :-1] == a[:, 1:]) & (idx[:, 1:] >= 0) if k > 1 else np.zeros((n_t, 0), bool)
    assert np.all(idx[:, :-1][tie] < idx[:, 1:][tie])
    assert np.all((idx >= 0).sum(1) == min(k, n_s))


@pytest.mark.parametrize("n_t,n_s", [(600, 9000), (70, 40000), (5000, 3000)])
def test_dense_pieces(n_t, n_s):
    """Sizes at which a row block's source tiles fall into several workgroup shares (pieces + merge)."""
    from oracle import xmap_oracle as xo
    eng, _ = engine()
    Ft, Fs = factors(41, n_t, 64, dup=n_t // 10), factors(42, n_s, 64, dup=n_s // 5)
    idx, val = eng.dense_topk(Ft, Fs, 50)
    oi, ov = xo.dense_topk(xo.dense_normalize(Ft), xo.dense_normalize(Fs), 50)
    assert np.array_equal(idx.cpu().numpy(), oi)
    assert np.array_equal(val.cpu().numpy().view(np.uint32), ov.view(np.uint32))


# ------------------------------------------------------------------------------------------------ designed families
D_ROWS, D_TILE, D_MAXSPLIT = 256, 32, 16      # csrc/stage_d.hip


def dense_segments(n_t, n_s, cus):
    """Python restatement of dense_layout and of the segment loop of k_dense_topk (csrc/stage_d.hip): the (row block, first
    tile, end tile) of every piece, and the largest number of pieces of a row block"""
    n_tiles = max((n_s + D_TILE - 1) // D_TILE, 1)
    n_rb = (n_t + D_ROWS - 1) // D_ROWS
    total = n_rb * n_tiles
    share = max((total + cus - 1) // cus, (n_tiles + D_MAXSPLIT - 3) // (D_MAXSPLIT - 2), 16)
    n_wg = (total + share - 1) // share
    segs = []
    for wg in range(n_wg):
        at, w_hi = wg * share, min(total, (wg + 1) * share)
        while at < w_hi:
            rb = at // n_tiles
            t0 = at - rb * n_tiles
            t1 = min(n_tiles, t0 + (w_hi - at))
            segs.append((rb, t0, t1))
            at += t1 - t0
    n_pieces = max(((rb + 1) * n_tiles - 1) // share - (rb * n_tiles) // share + 1 for rb in range(n_rb))
    return segs, n_pieces


def designed_factors(family, n_t, n_s, K):
    """(F_t, F_s) of one designed family (test_dense_topk_designed)"""
    rng = np.random.RandomState(77)
    Ft, Fs = np.zeros((n_t, K), np.float32), np.zeros((n_s, K), np.float32)
    theta = (np.arange(n_s) + 1.0) / (n_s + 1.0) * (np.pi / 2)
    if family in ("alphabet8", "short_piece"):      # source rows: +- copies of 8 prototypes
        Ft = rng.standard_normal((n_t, K)).astype(np.float32)
        proto = rng.standard_normal((8, K)).astype(np.float32)
        Fs = proto[rng.randint(0, 8, n_s)] * np.where(rng.rand(n_s) < 0.5, -1.0, 1.0).astype(np.float32)[:, None]
    elif family == "all_equal":                     # one source row repeated
        Ft = rng.standard_normal((n_t, K)).astype(np.float32)
        Fs[:] = rng.standard_normal(K).astype(np.float32)
    elif family in ("ascending", "descending"):     # |sim| grows (falls) with the column: every tile raises the bar (none passes)
        Ft[:, 0] = 1.0
        Fs[:, 0], Fs[:, 1] = np.sin(theta), np.cos(theta)
        if family == "descending":
            Fs = Fs[::-1].copy()
    elif family == "subnormal":                     # every product is m_j * 2^-140: an fp32 subnormal
        Ft[:, 0], Ft[:, 1] = 1.0, 2.0 ** -70
        Fs[:, 1] = 2.0 ** -70 * rng.randint(1, 1001, n_s)
        Fs[:, 2] = 1.0
    else:
        raise ValueError(family)
    return Ft, Fs


DESIGNED = [(f, 300, 4500, 50) for f in ("alphabet8", "all_equal", "ascending", "descending", "subnormal")] + \
           [("short_piece", 300, 4609, 64)]


@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("family,n_t,n_s,k", DESIGNED, ids=[d[0] for d in DESIGNED])
def test_dense_topk_designed(family, n_t, n_s, k, K):
    """The register insertion of k_dense_topk (a candidate passes |v| >= thr, its place comes from ballot + popcount, place
    >= k drops it) and k_dense_merge on inputs standard_normal factors never give -- the comparison of
    test_dense_topk_bit_exact, on several pieces per row block:
      alphabet8    8 values of |sim| per row: every list is cut inside a tie of hundreds, and the tie spans the pieces
      all_equal    one value: the first k columns win, every later candidate passes the threshold and loses on the index
      ascending    every tile raises the bar: the last k columns, the last one first
      descending   no tile passes after the first two of a piece: the first k columns
      subnormal    all listed values are fp32 subnormals (the guide: MFMA keeps them; not measured on this kernel before)
      short_piece  k = 64 and a piece of ONE tile that holds fewer than 64 columns: a partial list with padding is merged"""
    import ctypes as C
    import torch
    from oracle import xmap_oracle as xo
    from xmap.engine import hipabi as abi
    eng, _ = engine()
    npc = C.c_int32(0)
    abi.check(abi.lib.xmap_dense_layout(abi.i32(n_t), abi.i32(n_s), C.byref(npc)))
    assert npc.value > 1
    segs, n_pieces = dense_segments(n_t, n_s, torch.cuda.get_device_properties(0).multi_processor_count)
    assert n_pieces == npc.value
    if family == "short_piece":
        assert any(t1 - t0 == 1 and min(n_s, t1 * D_TILE) - t0 * D_TILE < 64 for _, t0, t1 in segs)
    Ft, Fs = designed_factors(family, n_t, n_s, K)
    oi, ov = xo.dense_topk(xo.dense_normalize(Ft), xo.dense_normalize(Fs), k)
    oa = np.abs(ov)
    # what the family is there for, on the oracle
    if family in ("alphabet8", "short_piece"):
        assert np.all(oa[:, k - 1] == oa[:, k - 2]) and np.all(oa[:, 0] == oa[:, k - 1])
        _, proto = np.unique(np.abs(Fs), axis=0, return_inverse=True)      # the tie of every prototype has columns in the pieces:
        proto = proto.reshape(-1)                                          # full partial lists of it lose in the merge
        assert proto.max() == 7 and np.bincount(proto).min() > 8 * k
        for p in range(8):
            assert sum(1 for _, t0, t1 in segs if (proto[t0 * D_TILE:t1 * D_TILE] == p).sum() >= k // 2) >= len(segs) - 2
    if family in ("all_equal", "descending"):
        assert np.array_equal(oi, np.tile(np.arange(k, dtype=np.int32), (n_t, 1)))
    if family == "ascending":
        assert np.array_equal(oi, np.tile(np.arange(n_s - 1, n_s - 1 - k, -1, dtype=np.int32), (n_t, 1)))
    if family in ("ascending", "descending"):
        assert np.all(oa[:, :-1] > oa[:, 1:])
    if family == "subnormal":
        assert ov.size == 15000 and np.all(oa > 0) and np.all(oa < np.finfo(np.float32).tiny)
    idx, val = eng.dense_topk(Ft, Fs, k)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    if family == "subnormal" and not np.array_equal(val.view(np.uint32), ov.view(np.uint32)):
        bad = np.nonzero(val.view(np.uint32) != ov.view(np.uint32))
        print("subnormal: %d of %d values differ; first: device %08x (index %d), oracle %08x (index %d)" % (
            len(bad[0]), val.size, val.view(np.uint32)[bad][0], idx[bad][0], ov.view(np.uint32)[bad][0], oi[bad][0]))
    assert np.array_equal(idx, oi)
    assert np.array_equal(val.view(np.uint32), ov.view(np.uint32))
    # size-independent properties: sorted by (|v| desc, idx asc), padding only at the tail
    a = np.abs(val)
    assert np.all(a[:, :-1] >= a[:, 1:])
    tie = (a[:, :-1] == a[:, 1:]) & (idx[:, 1:] >= 0)
    assert np.all(idx[:, :-1][tie] < idx[:, 1:][tie])
    assert np.all((idx >= 0).sum(1) == min(k, n_s))


def test_dense_normalize_matches_oracle_and_fp64():
    import torch
    from oracle import xmap_oracle as xo
    from xmap.engine import hipabi as abi
    F = factors(9, 777, 128, zero_rows=(5,))
    d = torch.from_numpy(F).cuda()
    out = torch.empty_like(d)
    import ctypes as C
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    abi.check(abi.lib.xmap_dense_normalize(st, abi.i32(777), abi.i32(128), abi.vp(d), abi.vp(out)))
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), xo.dense_normalize(F).view(np.uint32))
    ref = F.astype(np.float64) / np.maximum(np.linalg.norm(F.astype(np.float64), axis=1, keepdims=True), 1e-300)
    assert np.allclose(got, ref, rtol=2e-7, atol=0)      # fp32 rounding of an fp64 quotient
    assert np.all(got[5] == 0)


def test_dense_against_fp64_gemm():
    """The defining arithmetic: fp64 normalised GEMM.  The fp32 chain agrees within 1e-5 on the
    values (north_star's fp32 tolerance) and the top-k sets agree wherever the fp64 gap at rank k exceeds it."""
    eng, _ = engine()
    Ft, Fs = factors(21, 400, 128), factors(22, 900, 128)
    k = 20
    idx, val = eng.dense_topk(Ft, Fs, k)
    idx, val = idx.cpu().numpy(), val.cpu().numpy().astype(np.float64)
    nt = Ft.astype(np.float64) / np.linalg.norm(Ft.astype(np.float64), axis=1, keepdims=True)
    ns = Fs.astype(np.float64) / np.linalg.norm(Fs.astype(np.float64), axis=1, keepdims=True)
    G = nt @ ns.T
    assert np.allclose(val, np.take_along_axis(G, idx, 1), rtol=0, atol=1e-5)
    order = np.argsort(-np.abs(G), axis=1, kind="stable")
    srt = np.take_along_axis(np.abs(G), order, 1)
    clear = (srt[:, k - 1] - srt[:, k]) > 1e-5
    assert clear.sum() > 300
    assert all(set(idx[i]) == set(order[i, :k]) for i in np.nonzero(clear)[0])


def test_dense_extend_feeds_stage_c():
    """Dense replacement of stages A+B -> the unchanged stage C: private mapping = the best |sim| source item."""
    import torch
    from oracle import xmap_oracle as xo
    eng, r = engine()
    I = r.n_items
    F = factors(31, I, 64)
    E = eng.dense_extend(F, 10)
    flags = eng.R.flags[:I].cpu().numpy()
    tgt, src = np.nonzero(flags & 2)[0], np.nonzero(flags & 1)[0]
    Fn = xo.dense_normalize(F)
    oi, ov = xo.dense_topk(Fn[tgt], Fn[src], 10)
    te = E.top_end.cpu().numpy()
    assert np.array_equal(te[tgt], src[oi].astype(np.int32))
    assert np.array_equal(E.top_val.cpu().numpy()[tgt], ov.astype(np.float64))
    n_top, choice, mp = eng.select(E, True)
    mp = mp.cpu().numpy()
    # last-writer-wins over starts in ascending order (assist.py:210 map_to_dict): the mapping is source -> target
    exp = {}
    for t, s in zip(tgt, src[oi[:, 0]]):
        exp[int(s)] = int(t)
    assert {int(s): int(mp[s]) for s in range(I) if mp[s] >= 0} == exp
    G = eng.alterego(torch.from_numpy(mp).cuda())
    assert G.n_rows > 0


def test_dense_error_codes():
    """the C ABI reports misuse through its return code and xmap_last_error, it never launches on bad shapes"""
    import ctypes as C
    import torch
    from xmap.engine import hipabi as abi
    lib, vp, i32 = abi.lib, abi.vp, abi.i32
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    F = torch.randn(300, 96, device="cuda")
    out_i = torch.empty((300, 8), dtype=torch.int32, device="cuda")
    out_v = torch.empty((300, 8), dtype=torch.float32, device="cuda")
    rc = lib.xmap_dense_topk(st, i32(300), i32(300), i32(96), vp(F), vp(F), i32(8), i32(1), vp(None), vp(None), vp(out_i), vp(out_v))
    assert rc == abi.ERR_ARG and b"96" in lib.xmap_last_error()
    G = torch.randn(300, 128, device="cuda")
    rc = lib.xmap_dense_topk(st, i32(300), i32(300), i32(128), vp(G), vp(G), i32(65), i32(1), vp(None), vp(None), vp(out_i), vp(out_v))
    assert rc == abi.ERR_ARG
    big = torch.randn(70, 128, device="cuda")
    many = torch.randn(40000, 128, device="cuda")
    npc = C.c_int32(0)
    abi.check(lib.xmap_dense_layout(i32(70), i32(40000), C.byref(npc)))
    assert npc.value > 1
    oi = torch.empty((70, 8), dtype=torch.int32, device="cuda")
    ov = torch.empty((70, 8), dtype=torch.float32, device="cuda")
    rc = lib.xmap_dense_topk(st, i32(70), i32(40000), i32(128), vp(big), vp(many), i32(8), i32(1), vp(None), vp(None), vp(oi), vp(ov))
    assert rc == abi.ERR_CAPACITY and b"pieces" in lib.xmap_last_error()
    with pytest.raises(abi.XmapError):
        abi.check(rc)
