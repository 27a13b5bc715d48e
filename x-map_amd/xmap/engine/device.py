"""Device engine: drives the three stages of the hot path through the C ABI (include/xmap_hip.h).

torch is used only as the container for HBM buffers and for the current HIP stream; every
computation on the path is a kernel of libxmap_hip.so.  All results stay resident in HBM as
torch tensors until a caller asks for host copies.
"""
import ctypes as C
import math
import os

import numpy as np
import torch

from . import hipabi as abi
from .exactness import plain_sums_exact

lib = abi.lib
vp, i32, i64, check = abi.vp, abi.i32, abi.i64, abi.check


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# Stage A: partner bound of one hash partition of a row in the 1024-slot LDS table (75 % load, like the 96 / 192 / 384 of the
# smaller table classes) and the least rater count of a heavy row (profiles/tools/tune_a.py at BASELINE configs[1]: pair kernels
# 1.28 ms at 640 / 1024, 1.20 ms at 768 / 2048)
SLOT_TARGET = 768
CH_MIN = 2048
# Test-only switch, read once: the stage-A sequence (layout3 .. tri_mirror) with a stream synchronisation after every
# fine-grained call, i.e. nothing runs under a host wait.  tests/test_gpu_stage_a_waits.py holds the overlapped sequence to it.
STEPWISE = os.environ.get("XMAP_STAGE_A_STEPWISE") == "1"


class DeviceRatings(object):
    """trainRDD in index space, resident in HBM: CSR by user (trainRDD / profile order).  The CSC by item is
    derived on the device at the start of every stage-A pass (Engine.build_csc); only the id dictionary and the
    H2D upload are one-off host work."""

    def __init__(self, user_ptr, item, rating, time, n_items, attrs, device="cuda:0", rating64=False):
        """rating64: also keep the ratings as fp64 (RecommenderSim runs over AlterEgo rows, whose ratings are np.float64 means,
        reference core/generator.py:123-138 -> core/recommenderSim.py:64-133; the three stages of the path read float32).
        The arrays are checked on the host before anything is uploaded (xmap_check_ratings, the coarse upload's check):
        ValueError naming the first offending position.  A trainRDD holds one rating per (user, item); only the AlterEgo
        profiles (rating64) may hold an item twice -- RecommenderSim sizes its tables for that, stage A does not."""
        self.device = torch.device(device)
        user_ptr = np.ascontiguousarray(user_ptr, np.int64)
        item = np.ascontiguousarray(item, np.int32)
        if user_ptr.ndim != 1 or len(user_ptr) < 1:
            raise ValueError("user_ptr must hold n_users + 1 entries")
        prefix_cls, suffix_cls = [np.ascontiguousarray(a, np.int32) for a in attrs[:2]]
        if len(prefix_cls) != int(n_items) or len(suffix_cls) != int(n_items) or len(item) < max(int(user_ptr[-1]), 0):
            raise ValueError("prefix_cls / suffix_cls must hold n_items entries, item user_ptr[-1]")
        if abi.lib.xmap_check_ratings(len(user_ptr) - 1, int(n_items), user_ptr.ctypes.data, item.ctypes.data, prefix_cls.ctypes.data,
                                      suffix_cls.ctypes.data, 1 if rating64 else 0):
            raise ValueError((abi.lib.xmap_last_error() or b"").decode())
        r64 = np.ascontiguousarray(rating, np.float64) if rating64 else None
        rating = np.ascontiguousarray(rating, np.float32)
        time = np.ascontiguousarray(time, np.int64)
        self.n_users = len(user_ptr) - 1
        self.n_items = int(n_items)
        self.nnz = int(user_ptr[-1])
        # cosine may run on the plain fp64 sums (fast kernels) only when they are exact in any order (xmap.engine.exactness)
        self.plain_exact = plain_sums_exact(rating[:self.nnz], self.n_users)
        # contributions of the "tri" formulation (every unordered pair of a profile once): a property of the profile
        # lengths, so the engine sizes its pair buffers and unit arrays without asking the device
        d = np.diff(user_ptr)
        self.half_contrib = int((d * (d - 1) // 2).sum())
        contains_mask, flags = attrs[2:]
        d = self.device
        t = torch.from_numpy
        self.user_ptr = t(user_ptr).to(d)
        self.user_item = t(item).to(d)
        self.user_rating = t(rating).to(d)
        self.user_rating64 = t(r64).to(d) if r64 is not None else None
        self.user_time = t(time).to(d)
        self.item_ptr = torch.zeros(self.n_items + 1, dtype=torch.int64, device=d)
        self.item_user = torch.zeros(max(self.nnz, 1), dtype=torch.int32, device=d)
        self.item_rating = torch.zeros(max(self.nnz, 1), dtype=torch.float32, device=d)
        self.csc_ready = False
        self.prefix_cls = t(prefix_cls).to(d)
        self.suffix_cls = t(suffix_cls).to(d)
        self.contains_mask = t(np.ascontiguousarray(contains_mask, np.uint32).view(np.int32)).to(d)
        self.flags = t(np.ascontiguousarray(flags, np.uint8)).to(d)
        self.c = abi.Ratings(self.n_users, self.n_items, self.nnz,
                             self.user_ptr.data_ptr(), self.user_item.data_ptr(), self.user_rating.data_ptr(),
                             self.user_time.data_ptr(), self.item_ptr.data_ptr(), self.item_user.data_ptr(),
                             self.item_rating.data_ptr(), self.prefix_cls.data_ptr(), self.suffix_cls.data_ptr(),
                             self.contains_mask.data_ptr(), self.flags.data_ptr())

    def bytes_resident(self):
        return sum(x.numel() * x.element_size() for x in (
            self.user_ptr, self.user_item, self.user_rating, self.user_time, self.item_ptr,
            self.item_user, self.item_rating))


class SimResult(object):
    """Stage-A output in HBM: CSR (row_ptr, col, sim fp64, mutu, nij) + item/user info."""
    pass


class ExtResult(object):
    pass


class DivIndex(object):
    """what Engine.div_index returns: the diversity index of a rec_sim result"""
    pass


class PeerIndex(object):
    """what Engine.peer_index returns: the item-major transposition of a set of profiles and every user's norm"""
    pass


class PopIndex(object):
    """what Engine.pop_index returns: the popularity ranking of the items of a peer index"""
    pass


class LabelTable(object):
    """what Engine.set_labels returns: the label table of an item space on the device (lab_ptr, lab_id) and the labels' names"""
    pass


class AllotLists(tuple):
    """what allot_pool() / allot_topn() return: the tuple (cnt, item, plain, decayed) of every list call, with .positions, .taken
    and .stats"""

    def __new__(cls, lists, positions, taken, stats):
        self = tuple.__new__(cls, lists)
        self.positions, self.taken, self.stats = positions, taken, stats
        return self


class GenResult(object):
    pass


class _Timed(object):
    """HIP-event bracket around one C-ABI call on the engine's stream (only when profiling is on)."""

    def __init__(self, eng, name):
        self.eng, self.name = eng, name

    def __enter__(self):
        if self.eng.timers is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream(self.eng.dev))
        return self

    def __exit__(self, *exc):
        if self.eng.timers is not None:
            self.b.record(torch.cuda.current_stream(self.eng.dev))
            self.eng.timers.setdefault(self.name, []).append((self.a, self.b))
        return False


class Engine(object):
    def __init__(self, ratings):
        self.R = ratings
        self.dev = ratings.device
        self.timers = None  # set to {} to collect per-call HIP-event timings
        self._scratch = {}  # persistent zero-filled accumulator rows (the path kernels leave them zeroed)

    def _zero_scratch(self, name, numel, dtype):
        """Zero-filled scratch that kernels return zeroed: allocated (and cleared) once, reused across passes."""
        t = self._scratch.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.zeros(numel, dtype=dtype, device=self.dev)
            self._scratch[name] = t
        return t

    def hbm_available(self, *own):
        """bytes this process could allocate now: free on the device + unused blocks of torch's caching allocator + the
        scratch buffers named in `own` (about to be re-used or replaced)"""
        free, _ = torch.cuda.mem_get_info(self.dev)
        cached = torch.cuda.memory_reserved(self.dev) - torch.cuda.memory_allocated(self.dev)
        held = sum(t.numel() * t.element_size() for n, t in self._scratch.items() if n in own)
        return int(free + max(cached, 0) + held)

    def _drop_scratch(self, *names):
        """forget persistent zero-filled scratch (after a failed pass its rows may hold partial sums)"""
        for n in names:
            self._scratch.pop(n, None)

    def timed(self, name):
        return _Timed(self, name)

    def timer_ms(self):
        """{name: [ms, ...]} of everything recorded since timers was set (synchronises)."""
        torch.cuda.synchronize(self.dev)
        return {k: [a.elapsed_time(b) for a, b in v] for k, v in (self.timers or {}).items()}

    def _empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.dev)

    def _step(self):
        """STEPWISE: drain the stream after a fine-grained call of stage A"""
        if STEPWISE:
            torch.cuda.current_stream(self.dev).synchronize()

    def _out(self, shape, dtype, written):
        """buffer a kernel is about to fill completely (`written`: it will run, i.e. the input is not empty): no
        zero-fill launch in that case"""
        return self._empty(shape, dtype) if written else self._zeros(shape, dtype)

    def _zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.dev)

    # ------------------------------------------------------------------ stage A
    def pair_method(self, method):
        """the method code the pair kernels run: cosine over ratings whose plain fp64 sums may round (R.plain_exact False)
        takes the double-double route, XMAP_COSINE_EXACT"""
        m = abi.METHODS[method] if isinstance(method, str) else int(method)
        return abi.COSINE_EXACT if (m == abi.COSINE and not self.R.plain_exact) else m

    def build_csc(self):
        """item -> raters layout of the ratings (device counting sort; part of every stage-A pass)"""
        R = self.R
        st = _stream(self.dev)
        cnt = self._empty(max(R.n_items, 1), torch.int32)
        with self.timed("build_csc"):
            check(lib.xmap_build_csc(st, i64(R.n_users), i32(R.n_items), i64(R.nnz), vp(R.user_ptr), vp(R.user_item),
                                     vp(R.user_rating), vp(cnt), vp(R.item_ptr), vp(R.item_user), vp(R.item_rating)))
        R.csc_ready = True

    def stats(self, packed=False, item_range=None):
        """A2 + A3: CSC layout, user info, item info and (packed=True: the complete-rows formulation needs them)
        the flag-packed index copies.  item_range = (lo, hi): item info of that share only (item-sharded ranks
        all-gather the rest: xmap.engine.sharded)."""
        R = self.R
        st = _stream(self.dev)
        self.build_csc()
        u_avg = self._empty(max(R.n_users, 1), torch.float64)
        u_norm = self._empty(max(R.n_users, 1), torch.float64)
        check(lib.xmap_user_stats(st, C.byref(R.c), vp(u_avg), vp(u_norm)))
        info = self._out((max(R.n_items, 1), 4), torch.float64, R.n_items > 0)
        self.norms = self._out(2 * max(R.n_items, 1), torch.float64, R.n_items > 0)
        ua_item = self._empty(max(R.nnz, 1), torch.int32) if packed else None
        ia_user = self._empty(max(R.nnz, 1), torch.int32) if packed else None
        lo, hi = (0, R.n_items) if item_range is None else (int(item_range[0]), int(item_range[1]))
        if packed:      # (the flag-packed copies are filled by the cross-check library: only the complete-rows test formulation reads them)
            abi.xcheck(abi.xlib().xmap_item_stats(st, C.byref(R.c), vp(u_avg), vp(info), vp(self.norms), vp(ua_item), vp(ia_user), i32(lo), i32(hi)))
        else:
            check(lib.xmap_item_stats(st, C.byref(R.c), vp(u_avg), vp(info), vp(self.norms), vp(ua_item), vp(ia_user), i32(lo), i32(hi)))
        return u_avg, u_norm, info, ua_item, ia_user

    def stats_partial(self):
        """user-sharded input: CSC of this rank's users, their user info, and the rank's share of the item sums
        [I][7] = (sum r, sum r^2, adjusted norm^2, each as an exact (value, error) pair, raters) --
        xmap.engine.sharded.run_step_users"""
        R = self.R
        st = _stream(self.dev)
        self.build_csc()
        u_avg = self._empty(max(R.n_users, 1), torch.float64)
        u_norm = self._empty(max(R.n_users, 1), torch.float64)
        check(lib.xmap_user_stats(st, C.byref(R.c), vp(u_avg), vp(u_norm)))
        partial = self._out((max(R.n_items, 1), 7), torch.float64, R.n_items > 0)
        check(lib.xmap_item_partials(st, C.byref(R.c), vp(u_avg), vp(partial)))
        return u_avg, u_norm, partial

    def stats_merge(self, parts):
        """parts [n_parts][I][7] (the ranks' shares in rank order) -> info [I][4]; sets self.norms"""
        I = self.R.n_items
        parts = parts.contiguous()
        info = self._out((max(I, 1), 4), torch.float64, I > 0)
        self.norms = self._out(2 * max(I, 1), torch.float64, I > 0)
        check(lib.xmap_item_merge(_stream(self.dev), i32(I), i32(int(parts.shape[0])), vp(parts), vp(info), vp(self.norms)))
        return info

    def pack_pairs(self, coo, n):
        """valid entries of a half COO -> [n][3] int64 records for the exchange of a sharded step"""
        rec = self._empty((max(n, 1), 3), torch.int64)
        cnt = C.c_int64(0)
        check(lib.xmap_sim2_pack_pairs(_stream(self.dev), i64(int(coo[0].numel())), vp(coo[0]), vp(coo[1]), vp(coo[2]), vp(coo[3]),
                                       vp(coo[4]), vp(rec), C.byref(cnt)))
        assert int(cnt.value) == n, (int(cnt.value), n)
        return rec[:n]

    def unpack_pairs(self, rec):
        n = int(rec.shape[0])
        coo = (self._empty(max(n, 1), torch.int32), self._empty(max(n, 1), torch.int32), self._empty(max(n, 1), torch.float64),
               self._empty(max(n, 1), torch.int32), self._empty(max(n, 1), torch.int32))
        if n == 0:
            coo[0].fill_(-1)
        check(lib.xmap_sim2_unpack_pairs(_stream(self.dev), i64(n), vp(rec.contiguous()), *[vp(x) for x in coo]))
        return [x[:max(n, 1)] for x in coo]

    def partial_records(self, coo, n, n_owners):
        """raw half COO (tri_pairs(raw=True)) -> [n][4] int64 records grouped by the rank that owns the pair's lower item"""
        st = _stream(self.dev)
        coo_i, coo_j, coo_hi, coo_mutu, coo_nij, coo_lo = coo
        rec = self._empty((max(n, 1), 4), torch.int64)
        cnt = C.c_int64(0)
        check(lib.xmap_sim2_pack_partials(st, i64(int(coo_i.numel())), vp(coo_i), vp(coo_j), vp(coo_hi), vp(coo_lo), vp(coo_mutu),
                                          vp(coo_nij), vp(rec), C.byref(cnt)))
        assert int(cnt.value) == n, (int(cnt.value), n)
        return self.sort_records(rec[:n], n_owners)

    def sort_records(self, rec, n_owners=0):
        """stable sort of partial records: by owner of the lower item (n_owners > 0) or by pair key"""
        n = int(rec.shape[0])
        out = self._empty((max(n, 1), 4), torch.int64)
        if n:
            check(lib.xmap_sim2_sort_partials(_stream(self.dev), i64(n), vp(rec.contiguous()), vp(out), i32(self.R.n_items),
                                              i32(n_owners)))
        return out[:n]

    def merge_records(self, rec_sorted, method, cap):
        """all records of the pairs this rank owns (sorted by key, equal keys in rank order) -> (coo, rowcnt, kept, evaluated)"""
        st = _stream(self.dev)
        I = self.R.n_items
        m = abi.METHODS[method] if isinstance(method, str) else int(method)
        # cosine shares are always added up exactly: a rank's predicate covers its own users only, and its records hold
        # exact (value, error) pairs either way (integer ratings: error 0, the same bits as the plain sum)
        if m == abi.COSINE:
            m = abi.COSINE_EXACT
        n = int(rec_sorted.shape[0])
        coo_i = torch.full((max(n, 1),), -1, dtype=torch.int32, device=self.dev)
        coo_j = self._empty(max(n, 1), torch.int32)
        coo_sim = self._empty(max(n, 1), torch.float64)
        coo_mutu = self._empty(max(n, 1), torch.int32)
        coo_nij = self._empty(max(n, 1), torch.int32)
        rowcnt = self._empty(max(I, 1), torch.int32)
        h = (C.c_int64 * 2)()
        check(lib.xmap_sim2_merge_partials(st, m, int(cap), i32(I), i64(n), vp(rec_sorted.contiguous()), vp(self.norms), vp(coo_i),
                                           vp(coo_j), vp(coo_sim), vp(coo_mutu), vp(coo_nij), vp(rowcnt), h))
        kept, evaluated = int(h[0]), int(h[1])
        k1 = max(kept, 1)
        return (coo_i[:k1], coo_j[:k1], coo_sim[:k1], coo_mutu[:k1], coo_nij[:k1]), rowcnt, kept, evaluated

    def plan(self, slot_target=640):
        """work decomposition of the pair kernel: units = (item, hash partition of its partner space)"""
        R = self.R
        st = _stream(self.dev)
        I = R.n_items
        Pn = SimResult()
        Pn.slot_target = slot_target
        Pn.Q = self._zeros(max(I, 1), torch.int32)
        Pn.W = self._zeros(max(I, 1), torch.int64)
        Pn.unit_ptr = self._zeros(I + 1, torch.int64)
        n_units, contrib = C.c_int64(0), C.c_int64(0)
        with self.timed("plan"):
            abi.xcheck(abi.xlib().xmap_sim_plan(st, C.byref(R.c), i32(slot_target), vp(Pn.Q), vp(Pn.W), vp(Pn.unit_ptr),
                                    C.byref(n_units), C.byref(contrib)))
        Pn.nu, Pn.contrib = int(n_units.value), int(contrib.value)
        Pn.unit_item = self._empty(max(Pn.nu, 1), torch.int32)
        Pn.unit_q = self._empty(max(Pn.nu, 1), torch.int32)
        abi.xcheck(abi.xlib().xmap_sim_units(st, i32(I), vp(Pn.Q), vp(Pn.unit_ptr), vp(Pn.unit_item), vp(Pn.unit_q)))
        return Pn

    def item_weights(self, Pn):
        """per-item cost proxy of the pair kernel: raters x partitions (rater-steps of its units)"""
        R = self.R
        n = (R.item_ptr[1:] - R.item_ptr[:-1])
        return n * Pn.Q[:R.n_items].to(torch.int64)

    def item_sim(self, method, cap, slot_target=SLOT_TARGET, item_range=None, stats=None, plan=None, algo="tri"):
        """baseliner_calculate_sim_pipeline.  algo "tri" (default): each unordered pair once + mirror
        (tri_pairs.hip and its siblings); algo "rows": complete rows per unit (stage_a.hip), supports item_range -- a TEST formulation: its
        kernels live in libxmap_hip_xcheck.so (abi.xlib()), not in the product library."""
        if algo == "tri" and item_range is None and plan is None:
            return self.item_sim_tri(method, cap, slot_target)
        R = self.R
        st = _stream(self.dev)
        m = self.pair_method(method)
        if stats is None or stats[3] is None:
            with self.timed("stats"):
                stats = self.stats(packed=True)
        u_avg, u_norm, info, ua_item, ia_user = stats
        I = R.n_items
        while True:
            Pn = plan if plan is not None else self.plan(slot_target)
            Q, unit_ptr, unit_item, unit_q, nu, contrib = Pn.Q, Pn.unit_ptr, Pn.unit_item, Pn.unit_q, Pn.nu, Pn.contrib
            if item_range is None:
                lo, hi = 0, nu
            else:
                ends = unit_ptr[[int(item_range[0]), int(item_range[1])]].tolist()
                lo, hi = int(ends[0]), int(ends[1])
            unit_cnt = self._zeros(max(nu, 1), torch.int32)
            d_cnt = self._zeros(4, torch.int64)
            h_cnt = [0, 0, 0, 0]
            with self.timed("pair_count"):
                rc = abi.xlib().xmap_sim_count(st, C.byref(R.c), m, int(cap), vp(u_avg), vp(info), vp(ua_item),
                                        vp(ia_user), vp(Q), vp(unit_item), vp(unit_q), i64(lo), i64(hi),
                                        vp(unit_cnt), vp(d_cnt), None)
            abi.xcheck(rc)
            h_cnt = d_cnt.tolist()  # synchronises the stream
            if h_cnt[2]:
                if slot_target > 32:
                    slot_target //= 2
                    plan = None
                    continue
                raise abi.XmapError(abi.ERR_OVERFLOW, "pair-table overflow")
            break
        kept, evaluated = int(h_cnt[0]), int(h_cnt[1])
        unit_off = self._zeros(nu + 1, torch.int64)
        check(lib.xmap_exclusive_scan_i32_to_i64(st, vp(unit_cnt), vp(unit_off), i64(nu), None))
        row_ptr = self._empty(I + 1, torch.int64)
        abi.xcheck(abi.xlib().xmap_sim_row_ptr(st, i32(I), vp(unit_ptr), vp(unit_off), vp(row_ptr)))
        col = self._empty(max(kept, 1), torch.int32)
        sim = self._empty(max(kept, 1), torch.float64)
        mutu = self._empty(max(kept, 1), torch.int32)
        nij = self._empty(max(kept, 1), torch.int32)
        with self.timed("pair_fill"):
            abi.xcheck(abi.xlib().xmap_sim_fill(st, C.byref(R.c), m, int(cap), vp(u_avg), vp(info), vp(ua_item), vp(ia_user),
                                    vp(Q), vp(unit_item), vp(unit_q), i64(lo), i64(hi), vp(unit_off),
                                    vp(col), vp(sim), vp(mutu), vp(nij)))
        S = SimResult()
        S.method, S.cap, S.n_items = abi.METHODS[method] if isinstance(method, str) else int(method), int(cap), I
        S.u_avg, S.u_norm, S.info = u_avg, u_norm, info
        S.row_ptr, S.col, S.sim, S.mutu, S.nij = row_ptr, col[:kept], sim[:kept], mutu[:kept], nij[:kept]
        S.n_kept, S.n_eval, S.n_contrib, S.n_units = kept, evaluated, int(contrib), hi - lo
        S.plan = Pn
        S.slot_target = slot_target
        S.c = abi.Sim(I, row_ptr.data_ptr(), col.data_ptr(), sim.data_ptr(), mutu.data_ptr(), nij.data_ptr(),
                      info.data_ptr(), 0)
        S._keep = (col, sim, mutu, nij)
        return S

    # ---- stage A, second formulation (csrc/tri.h, tri_*.hip): each unordered pair once, mirrored into the CSR
    def tri_layout(self, stats, slot_target=SLOT_TARGET, ch_min=CH_MIN, dups=False):
        """weight-sorted private profiles, rater records, heavy set, work units (method independent).
        dups: a profile may hold an item more than once (AlterEgo rows)."""
        R, I = self.R, self.R.n_items
        L = self._layout_buffers(dups)
        h_ctl = (C.c_int32 * 2)()
        with self.timed("tri_layout"):
            check(lib.xmap_sim2_layout(_stream(self.dev), C.byref(R.c), vp(stats[2]), i32(ch_min), vp(L.hist), vp(L.pre), vp(L.ctl),
                                       vp(L.hid), vp(L.hlist), vp(L.ub_key), vp(L.ub), vp(L.rc), vp(L.Wp),
                                       i32(1 if dups else 0), h_ctl))
        L.CH, L.n_heavy = int(h_ctl[0]), int(h_ctl[1])
        L.slot_target = slot_target
        self._tri_plan(L, slot_target)
        both = torch.stack([L.Wp[:I].sum(), L.Wp[L.hlist[:L.n_heavy].long()].sum()]).tolist() if I else [0, 0]   # one sync
        L.half_contrib, L.heavy_half = int(both[0]), int(both[1])
        return L

    def _layout_buffers(self, dups, wide=False):
        """what both layouts (tri_layout, layout3) fill for the plan and the pair kernels"""
        I, U, nnz = self.R.n_items, self.R.n_users, self.R.nnz
        n1, i1 = max(nnz, 1), max(I, 1)
        L = SimResult()
        L.hist = self._empty(U + 2, torch.int32)
        L.pre = self._empty(U + 3, torch.int64)
        L.ctl = self._empty(4, torch.int32)
        L.hid = self._empty(i1, torch.int32)
        L.hlist = self._zeros(1024, torch.int32)
        L.ub_key = self._empty(n1, torch.int64)
        L.ub = self._empty(n1 * (2 if wide else 1), torch.int64)    # (item | flag, rating bits) pairs; wide: 16-byte entries
        L.rc = self._empty(n1 * 2, torch.int64)                      # 16-byte rater records
        L.Wp = self._empty(i1, torch.int64)
        L.dups = bool(dups)
        return L

    def _plan_buffers(self, L):
        """what both plans (_tri_plan, _tri_plan3) fill per item"""
        I = self.R.n_items
        L.Q = self._out(max(I, 1), torch.int32, I > 0)
        L.C = self._out(max(I, 1), torch.int32, I > 0)
        L.small = self._out(max(I, 1), torch.uint8, I > 0)
        L.Qcat = self._empty(5 * max(I, 1), torch.int32)
        L.uq_ptr = self._out(5 * I + 1, torch.int64, I > 0)     # light units class-major: [table class rank][item]
        L.uc_ptr = self._out(I + 1, torch.int64, I > 0)

    def _tri_plan(self, L, slot_target):
        R = self.R
        st = _stream(self.dev)
        I = R.n_items
        self._plan_buffers(L)
        h = (C.c_int64 * 8)()
        with self.timed("tri_plan"):
            check(lib.xmap_sim2_plan(st, C.byref(R.c), i32(slot_target), vp(L.rc), vp(L.pre), vp(L.hid),
                                     vp(L.ctl), vp(L.Q), vp(L.C), vp(L.small), vp(L.Wp), vp(L.Qcat), vp(L.uq_ptr),
                                     vp(L.uc_ptr), i32(1 if getattr(L, "dups", False) else 0), h))
            L.n_light, L.n_heavy_units = int(h[0]), int(h[1])
            L.cls_ptr = (C.c_int64 * 6)(*[int(h[2 + c]) for c in range(6)])
            L.uq_item = self._empty(max(L.n_light, 1), torch.int32)
            L.uq_q = self._empty(4 * max(L.n_light, 1), torch.int32)
            L.uc_item = self._empty(max(L.n_heavy_units, 1), torch.int32)
            L.uc_c = self._empty(max(L.n_heavy_units, 1), torch.int32)
            check(lib.xmap_sim2_units(st, i32(I), vp(R.item_ptr), vp(L.Qcat), vp(L.uq_ptr), vp(L.uq_item), vp(L.uq_q),
                                      vp(L.C), vp(L.uc_ptr), vp(L.uc_item), vp(L.uc_c)))
        L.slot_target = slot_target

    def _tri_plan3(self, L, slot_target, under_wait=None):
        """_tri_plan with one host wait (xmap_sim3_plan_begin / _wait): unit arrays sized from host-known bounds, the counts the
        launches need and the heavy set's {CH, |H|} in one copy into pinned memory with an event behind it.  under_wait():
        launches that do not depend on the counts (the profile copy's flag pass); they are queued behind the copy and run while
        the host waits for the event, reads the counts and launches the pair kernels.  L.pairs_hint (set by the caller that will
        run tri_pairs next): the pair kernels' buffers are allocated before the wait as well."""
        R = self.R
        st = _stream(self.dev)
        I = R.n_items
        self._plan_buffers(L)
        cap_light = L.half_contrib // max(int(slot_target), 1) + I + 1
        cap_heavy = R.nnz // max(int(L.ch_min), 1) + 1025
        L.uq_item = self._empty(cap_light, torch.int32)
        L.uq_q = self._empty(4 * cap_light, torch.int32)
        L.uc_item = self._empty(cap_heavy, torch.int32)
        L.uc_c = self._empty(cap_heavy, torch.int32)
        h = (C.c_int64 * 10)()
        with self.timed("tri_plan"):
            check(lib.xmap_sim3_plan_begin(st, C.byref(R.c), i32(slot_target), vp(L.pre), vp(L.hid), vp(L.ctl), vp(L.Q), vp(L.C),
                                           vp(L.small), vp(L.Wp), vp(L.Qcat), vp(L.uq_ptr), vp(L.uc_ptr),
                                           i32(1 if getattr(L, "dups", False) else 0), vp(L.uq_item), vp(L.uq_q), vp(L.uc_item),
                                           vp(L.uc_c), i64(cap_light), i64(cap_heavy)))
            self._step()
            if under_wait is not None:
                under_wait()
                self._step()
            hint = getattr(L, "pairs_hint", None)
            if hint is not None and getattr(L, "_pairs_pre", None) is None:
                L._pairs_pre = self._pairs_buffers(L, 1.0, **hint)
            check(lib.xmap_sim3_plan_wait(i64(cap_light), i64(cap_heavy), h))
        L.n_light, L.n_heavy_units = int(h[0]), int(h[1])
        L.cls_ptr = (C.c_int64 * 6)(*[int(h[2 + c]) for c in range(6)])
        L.CH, L.n_heavy = int(h[8]), int(h[9])
        L.slot_target = slot_target
        L.replan = self._tri_plan3

    def heavy_half(self, L):
        """contributions of the heavy rows (reporting only: the bench's per-kernel byte counts)"""
        if getattr(L, "_heavy_half", None) is None:
            L._heavy_half = int(L.Wp[L.hlist[:L.n_heavy].long()].sum().item()) if L.n_heavy else 0
        return L._heavy_half

    def tri_pairs(self, method, cap, stats, L, unit_range=None, do_heavy=True, retry=True, rec=False, raw=False, split=False,
                  heavy_deal=None, marks=True, count_mir=False):
        """half COO of the kept pairs computed by the light units in unit_range (+ the heavy rows).
        rec: the RecommenderSim variant (nothing filtered, self pairs, a 6th COO column with the local sensitivity).
        split: count a row's own pairs (rowcnt) and the pairs lighter rows computed for it (a 5th return value) apart --
        what tri_mirror takes.  heavy_deal = (rank, world): of the heavy rows only those with item index % world == rank
        (item-sharded ranks deal them round-robin; chunk partials and merge of a row stay on one rank).  split: the mirrored
        counts are NOT taken (the returned array is cleared): tri_mirror / mir_counts count them from the COO.  marks=False:
        the unused COO entries are left unmarked (for a consumer that goes by the shard cursors: tri_mirror with shards).
        count_mir (with split, all units on this device): the mirrored counts are taken here, launched BEFORE the read-back of
        the kept-pair count so that the host's wait falls into their 0.2 ms; tri_mirror is then called with counted=True."""
        R = self.R
        st = _stream(self.dev)
        m = self.pair_method(method)
        u_avg, u_norm, info, _, _ = stats
        I = R.n_items
        coo_slack = 1.0
        while True:
            lo, hi = (0, L.n_light) if unit_range is None else (int(unit_range[0]), int(unit_range[1]))
            # (taken under the plan's wait when the caller announced this call: _tri_plan3; else, and on a retry, here)
            pre = L.__dict__.pop("_pairs_pre", None)
            if pre is None or pre["key"] != self._pairs_key(L, coo_slack, rec or raw, split, count_mir and split and not raw):
                pre = self._pairs_buffers(L, coo_slack, rec or raw, split, count_mir and split and not raw)
            cap_coo = pre["cap_coo"]
            coo_i, coo_j, coo_sim, coo_mutu, coo_nij, coo_ls = pre["coo"]
            rowcnt, mircnt, d_cnt, d_shards = pre["rowcnt"], pre["mircnt"], pre["d_cnt"], pre["d_shards"]
            nh = L.n_heavy_units if do_heavy else 0
            hp_hi = self._empty(max(nh, 1) * 1024, torch.float64)
            hp_lo = self._empty(max(nh, 1) * 1024, torch.float64)
            hp_cnt = self._empty(max(nh, 1) * 1024, torch.int32)
            hp_mut = self._empty(max(nh, 1) * 1024, torch.int32)

            deal = 0 if heavy_deal is None else abi.pairs_deal(heavy_deal[1], heavy_deal[0])
            heavy, merge = (abi.PAIRS_HEAVY, abi.PAIRS_HEAVY_MERGE) if do_heavy else (0, 0)
            light = abi.PAIRS_LIGHT | (abi.PAIRS_RAW if raw else 0)

            def run(phases):
                phases |= deal | (0 if marks else abi.PAIRS_NO_MARKS)
                check(lib.xmap_sim2_pairs(
                    st, C.byref(R.c), m, int(cap), vp(u_avg), vp(self.norms), vp(L.rc), vp(L.ub), vp(L.Q), vp(L.small),
                    vp(L.uq_item),
                    vp(L.uq_q), L.cls_ptr, i64(lo), i64(hi), vp(L.hid), vp(L.hlist), vp(L.ctl), vp(L.C), vp(L.uc_ptr),
                    vp(L.uc_item), vp(L.uc_c), i32(nh), i32(L.n_heavy), phases,
                    vp(hp_hi), vp(hp_lo), vp(hp_cnt), vp(hp_mut), i64(cap_coo), vp(coo_i), vp(coo_j), vp(coo_sim),
                    vp(coo_mutu), vp(coo_nij), vp(coo_ls), vp(rowcnt), vp(d_shards), vp(d_cnt), vp(mircnt)))
                self._step()
            if os.environ.get("XMAP_SPLIT_PHASES") == "1":        # one timer per phase (analysis)
                with self.timed("pair_heavy"):
                    run(abi.PAIRS_RESET | heavy)
                with self.timed("pair_tri"):
                    run(light)
                with self.timed("heavy_merge"):
                    run(merge | abi.PAIRS_MIRCOUNT)
            else:       # the heavy rows (chunk partials + merge) on a side stream next to the class launches of the light rows
                with self.timed("pair_tri"):
                    run(abi.PAIRS_RESET | heavy | light | merge | abi.PAIRS_MIRCOUNT | abi.PAIRS_SHARD_SUMS)
            # the one host wait of the pair kernels (flags + kept / evaluated pairs): the copy into pinned memory and its event
            # are queued here, the mirrored counts behind them; the host waits for the event alone, so the counts arrive while
            # the 0.2 ms of the count kernels still run, and the mirror's allocations and launches fall under them
            check(lib.xmap_sim3_counters_begin(st, vp(d_cnt)))
            self._step()
            if count_mir and split and not raw:
                with self.timed("mir_count"):
                    check(lib.xmap_sim3_mircount(st, i32(I), i64(cap_coo), vp(coo_i), vp(coo_j), vp(d_shards), i64(cap_coo),
                                                 i32(1 if rec else 0), vp(pre["mir_scratch"]), vp(mircnt)))
                    self._step()
                L._mirror_pre = self._mirror_buffers(cap_coo, 4 if rec else 3)
            hc = (C.c_int64 * 6)()
            check(lib.xmap_sim3_counters_wait(hc))
            h = [int(x) for x in hc]
            if h[2]:
                if L.slot_target <= 32:
                    raise abi.XmapError(abi.ERR_OVERFLOW, "pair-table overflow")
                if not retry:      # sharded callers re-plan collectively
                    return (None, rowcnt, 0, 0) + ((None, None) if split else ()) + (1,)
                getattr(L, "replan", self._tri_plan)(L, L.slot_target // 2)
                continue
            if h[3]:            # a COO shard overflowed: more slack
                if coo_slack > 64:
                    raise abi.XmapError(abi.ERR_CAPACITY, "half-COO overflow")
                coo_slack *= 2
                continue
            break
        if os.environ.get("XMAP_SPLIT_PHASES") == "1":      # (the split run has no shard-sum phase)
            h[4:6] = d_shards.view(2, 4096).sum(dim=1).tolist()
        n, n_unordered = int(h[4]), int(h[5])
        coo = (coo_i, coo_j, coo_sim, coo_mutu, coo_nij) + ((coo_ls,) if (rec or raw) else ())
        out = (coo, rowcnt, n, n_unordered)
        if split:
            return out + (mircnt, d_shards) + (() if retry else (0,))
        return out if retry else out + (0,)

    def _pairs_key(self, L, coo_slack, has_ls, split, count_mir):
        # per-shard capacity >= one full table (1024 kept pairs) + the expected share with slack
        cap_coo = (max(int(L.half_contrib * coo_slack), 1) // 4096 + 1100) * 4096
        return (cap_coo, bool(has_ls), bool(split), bool(count_mir))

    def _pairs_buffers(self, L, coo_slack, has_ls, split, count_mir):
        """what tri_pairs needs that does not depend on the plan's counts: half COO, row counts, counters, shard cursors"""
        I = self.R.n_items
        key = self._pairs_key(L, coo_slack, has_ls, split, count_mir)
        cap_coo = key[0]
        coo = (self._empty(cap_coo, torch.int32), self._empty(cap_coo, torch.int32), self._empty(cap_coo, torch.float64),
               self._empty(cap_coo, torch.int32), self._empty(cap_coo, torch.int32),
               self._empty(cap_coo, torch.float64) if has_ls else None)            # raw: the error column of the dot
        return {"key": key, "cap_coo": cap_coo, "coo": coo,
                "rowcnt": self._empty(max(I, 1), torch.int32),
                "mircnt": self._empty(max(I, 1), torch.int32) if split else None,
                "d_cnt": self._empty(6, torch.int64),       # (cleared by PAIRS_RESET) [4], [5]: the shard sums (PAIRS_SHARD_SUMS)
                "d_shards": self._empty(2 * 4096, torch.int64),
                "mir_scratch": self._empty(cap_coo, torch.int32) if count_mir else None}

    def _mirror_buffers(self, n_rec, rw):
        """what tri_mirror needs apart from the CSR columns, for at most n_rec records of rw words"""
        I = self.R.n_items
        return {"n_rec": int(n_rec), "rw": rw,
                "row_ptr": self._out(I + 1, torch.int64, I > 0), "mptr": self._empty(I + 1, torch.int64),
                "tot": self._empty(max(I, 1), torch.int32), "fill": self._empty(max(I, 1), torch.int32),
                "buf_a": self._empty(max(int(n_rec), 1) * rw, torch.int64), "buf_b": self._empty(max(int(n_rec), 1) * rw, torch.int64)}

    def tri_scatter(self, coo, rowcnt, info, n=None, L=None):
        """mirror a (complete) half COO (n valid entries; unused ones have coo_i = -1) into the CSR"""
        R = self.R
        st = _stream(self.dev)
        I = R.n_items
        coo_i, coo_j, coo_sim, coo_mutu, coo_nij = [x.contiguous() for x in coo[:5]]
        coo_ls = coo[5].contiguous() if len(coo) > 5 else None
        n_scan = int(coo_i.numel())
        if n is None:
            n = n_scan
        row_ptr = self._out(I + 1, torch.int64, I > 0)
        tot = C.c_int64(0)
        check(lib.xmap_exclusive_scan_i32_to_i64(st, vp(rowcnt), vp(row_ptr), i64(I), C.byref(tot) if coo_ls is not None else None))
        kept = 2 * n if coo_ls is None else int(tot.value)      # a row paired with itself is one entry
        ls = self._empty(max(kept, 1), torch.float64) if coo_ls is not None else None
        col = self._empty(max(kept, 1), torch.int32)
        sim = self._empty(max(kept, 1), torch.float64)
        mutu = self._empty(max(kept, 1), torch.int32)
        nij = self._empty(max(kept, 1), torch.int32)
        fill = self._empty(max(I, 1), torch.int32)
        with self.timed("scatter"):
          if n:
            check(lib.xmap_sim2_scatter(st, i32(I), i64(n_scan), vp(coo_i), vp(coo_j), vp(coo_sim), vp(coo_mutu),
                                        vp(coo_nij), vp(coo_ls), vp(row_ptr), vp(fill), vp(L.hid), vp(L.hlist), vp(col),
                                        vp(sim), vp(mutu), vp(nij), vp(ls)))
        S = self.sim_from_device(row_ptr, col[:kept], sim[:kept], mutu[:kept], nij[:kept], info)
        S.ls = ls[:kept] if ls is not None else None
        return S

    def rec_sim(self, cap, slot_target=SLOT_TARGET):
        """RecommenderSim.calculate_sim (reference core/recommenderSim.py:65-133,188-195; both method names take the
        cosine branch) over this engine's ratings, which are AlterEgo rows: weighted cosine and leave-one-out local
        sensitivity of every directed item pair with a co-rater, CSR by first item (col, sim, nij, ls).  The same
        pair machinery as stage A: exact (double-double) sums with a zero user average, no heavy set."""
        R = self.R
        with self.timed("rec_stats"):
            stats, L = self.layout3(slot_target, ch_min=max(64, R.n_users + 2), wide=True,      # no heavy set
                                    pairs_hint=dict(has_ls=True, split=True, count_mir=True))
        S, n_unordered = self._pairs_to_csr("adjust_cosine", cap, stats, L, rec=True)
        S.cap, S.n_unordered, S.layout = int(cap), n_unordered, L
        S.norm = self.norms[R.n_items:2 * R.n_items]
        return S

    def rec_select(self, S, keep):
        """RecommenderPrivacy.nonprivate_neighbor_selection on a rec_sim result: per item the `keep` neighbours by
        (|sim| desc, index asc).  Returns (cnt [I], col [I][keep], sim [I][keep], ls [I][keep]) on the device."""
        st = _stream(self.dev)
        I = self.R.n_items
        cnt = self._zeros(max(I, 1), torch.int32)
        col = self._empty((max(I, 1), keep), torch.int32)
        sim = self._empty((max(I, 1), keep), torch.float64)
        ls = self._empty((max(I, 1), keep), torch.float64)
        with self.timed("rec_select"):
            check(lib.xmap_rec_select(st, i32(I), vp(S.row_ptr), vp(S.col), vp(S.sim), vp(S.ls), i32(keep), vp(cnt),
                                      vp(col), vp(sim), vp(ls)))
        return cnt[:I], col[:I], sim[:I], ls[:I]

    def layout3(self, slot_target=SLOT_TARGET, ch_min=CH_MIN, wide=False, item_range=None, pairs_hint=None):
        """Round-3 layout of the "tri" formulation, one transposition per pass (xmap_sim3_layout): item counts, user and
        item info, weight-sorted profiles, rater records through the tile sort, heavy set, work units.  Returns (stats, L)
        like stats() + tri_layout().  wide: fp64 ratings (R.user_rating64) with zero user averages -- the RecommenderSim
        variant.  item_range (item-sharded ranks): the item statistics of that share of the items only; the caller then
        completes stats[2] (info) and self.norms on every rank -- the all-gather of per-item norms -- and calls L.finish(),
        which sets the mutuality flags from them and plans the work units.  Without item_range the profile copy's flag pass
        (k_ub_flags) is queued behind the plan's read-back instead of in front of the plan: neither the plan nor the unit kernel
        reads those flags, and the pass then runs while the host waits for the plan's counts (its time moves from the
        "layout3" bracket into "tri_plan").  pairs_hint = {has_ls, split, count_mir} of the tri_pairs call that follows: its
        buffers are allocated under that wait too."""
        R = self.R
        st = _stream(self.dev)
        I, U, nnz = R.n_items, R.n_users, R.nnz
        n1, i1 = max(nnz, 1), max(I, 1)
        rw = 3 if wide else 2                                    # 64-bit words per sort record
        L = self._layout_buffers(wide, wide)
        cnt = self._empty(i1, torch.int32)
        u_avg = self._zeros(max(U, 1), torch.float64) if wide else self._empty(max(U, 1), torch.float64)
        u_norm = None if wide else self._empty(max(U, 1), torch.float64)
        srec = self._empty(n1 * rw, torch.int64)
        buf_a = self._empty(n1 * rw, torch.int64)
        buf_b = self._empty(n1 * rw, torch.int64)
        L.wide = bool(wide)
        info = self._out((i1, 4), torch.float64, I > 0)
        self.norms = self._out(2 * i1, torch.float64, I > 0)
        r64 = None
        if wide:
            r64 = R.user_rating64 if R.user_rating64 is not None else R.user_rating.double()
        def call(phases, lo, hi):
            check(lib.xmap_sim3_layout(st, C.byref(R.c), vp(R.item_ptr), vp(r64), i32(ch_min), i32(phases), i32(lo), i32(hi), vp(cnt),
                                       vp(u_avg), vp(u_norm), vp(L.hist), vp(L.pre), vp(L.ctl), vp(L.hid), vp(L.hlist),
                                       vp(L.ub_key), vp(L.ub), vp(srec), vp(buf_a), vp(buf_b), vp(L.rc), vp(L.Wp), vp(info),
                                       vp(self.norms), None))
        R.csc_ready = False             # item_ptr is current; item_user / item_rating are not built on this path
        L.ch_min = int(ch_min)
        L.half_contrib = R.half_contrib          # = sum of W+ over the items (the host knows it from the profile lengths)
        if item_range is None:
            with self.timed("layout3"):
                call(abi.LAYOUT_RECORDS | abi.LAYOUT_STATS, 0, I)
                self._step()
            L.pairs_hint = pairs_hint
            # (fp64 ratings: no mutuality, no flag pass)
            self._tri_plan3(L, slot_target, under_wait=None if wide else (lambda: call(abi.LAYOUT_UB_FLAGS, 0, I)))
        else:
            with self.timed("layout3"):
                call(abi.LAYOUT_RECORDS | abi.LAYOUT_STATS, int(item_range[0]), int(item_range[1]))
                self._step()

            def finish():
                with self.timed("layout3_flags"):
                    call(abi.LAYOUT_UB_FLAGS | abi.LAYOUT_RC_FLAGS, 0, I)
                    self._step()
                self._tri_plan3(L, slot_target)
            L.finish = finish
        return (u_avg, u_norm, info, None, None), L

    def mir_counts(self, coo, n, mir, shards=None, skip_self=False):
        """mir[j] = entries of the half COO (n valid ones) whose partner is j (xmap_sim3_mircount)"""
        I = self.R.n_items
        scratch = self._empty(max(int(n), 1), torch.int32)
        check(lib.xmap_sim3_mircount(_stream(self.dev), i32(I), i64(int(coo[0].numel())), vp(coo[0].contiguous()), vp(coo[1].contiguous()),
                                     vp(shards), i64(n), i32(1 if skip_self else 0), vp(scratch), vp(mir)))
        return mir

    def tri_mirror(self, coo, own, mir, info, n, shards=None, rows=None, counted=False, pre=None):
        """round-3 mirror (xmap_sim3_mirror): a complete half COO with n valid entries, own[i] = pairs row i computed,
        mir[j] = pairs computed in lighter rows -> CSR, row = [own | mirrored].  shards: the cursors tri_pairs left (the
        COO is cut into 4096 shards filled from their start); None: the COO is one range of n records.  rows = (lo, hi):
        only these rows are built (the others stay empty) -- an item-sharded rank's share of the matrix, which is all its
        knn and reverse-list shares read.  mir is filled here from the COO unless counted=True (mir_counts ran already).
        pre: _mirror_buffers taken before the kept count was known (room for the whole COO); the CSR columns are sized here."""
        R = self.R
        st = _stream(self.dev)
        I = R.n_items
        coo_i, coo_j, coo_sim, coo_mutu, coo_nij = [x.contiguous() for x in coo[:5]]
        coo_ls = coo[5].contiguous() if len(coo) > 5 else None       # RecommenderSim: local sensitivities, self pairs
        cap = int(coo_i.numel())
        kept = 2 * int(n)                                            # (an upper bound with self pairs: one entry each)
        lo, hi = (0, I) if rows is None else (int(rows[0]), int(rows[1]))
        if rows is not None and I > 0:
            own = own.clone()
            own[:lo].zero_(); own[hi:].zero_()
            if counted:
                mir = mir.clone()
                mir[:lo].zero_(); mir[hi:].zero_()
                kept = int((own[lo:hi].long().sum() + mir[lo:hi].long().sum()).item())
        rw = 4 if coo_ls is not None else 3
        if pre is None or pre["rw"] != rw or pre["n_rec"] < int(n):
            pre = self._mirror_buffers(n, rw)
        row_ptr, mptr, tot, fill, buf_a, buf_b = [pre[k] for k in ("row_ptr", "mptr", "tot", "fill", "buf_a", "buf_b")]
        col = self._empty(max(kept, 1), torch.int32)
        sim = self._empty(max(kept, 1), torch.float64)
        mutu = self._empty(max(kept, 1), torch.int32)
        nij = self._empty(max(kept, 1), torch.int32)
        ls = self._empty(max(kept, 1), torch.float64) if coo_ls is not None else None
        with self.timed("scatter"):
            if not counted:
                check(lib.xmap_sim3_mircount(st, i32(I), i64(cap), vp(coo_i), vp(coo_j), vp(shards), i64(n), i32(1 if coo_ls is not None else 0),
                                             vp(buf_a), vp(mir)))
                if rows is not None and I > 0:
                    mir[:lo].zero_(); mir[hi:].zero_()
                    kept = int((own[lo:hi].long().sum() + mir[lo:hi].long().sum()).item())
            check(lib.xmap_sim3_mirror(st, i32(I), i64(cap), vp(coo_i), vp(coo_j), vp(coo_sim), vp(coo_mutu), vp(coo_nij), vp(shards), i64(n),
                                       vp(own), vp(mir), vp(tot), vp(row_ptr), vp(mptr), vp(fill), vp(buf_a), vp(buf_b), vp(col),
                                       vp(sim), vp(mutu), vp(nij), vp(coo_ls), vp(ls), i32(lo), i32(hi)))
            self._step()
        if coo_ls is not None:
            kept = int(row_ptr[I].item()) if I > 0 else 0
        S = self.sim_from_device(row_ptr, col[:kept], sim[:kept], mutu[:kept], nij[:kept], info)
        S.ls = ls[:kept] if ls is not None else None
        return S

    def _pairs_to_csr(self, method, cap, stats, L, rec=False):
        """pair kernels + mirror over a layout -> (CSR, unordered pairs evaluated).  XMAP_A_V2=1: the round-2 mirror (one
        combined count per row, cursor atomics) -- kept as a cross-check of the round-3 one (own and mirrored counts apart,
        tile sort).  rec: the RecommenderSim variant, no heavy rows."""
        if os.environ.get("XMAP_A_V2") == "1":
            coo, rowcnt, n, n_unordered = self.tri_pairs(method, cap, stats, L, do_heavy=not rec, rec=rec)
            return self.tri_scatter(coo, rowcnt, stats[2], n, L), n_unordered
        coo, own, n, n_unordered, mir, shards = self.tri_pairs(method, cap, stats, L, do_heavy=not rec, rec=rec, split=True,
                                                               marks=False, count_mir=True)
        return self.tri_mirror(coo, own, mir, stats[2], n, shards, counted=True, pre=L.__dict__.pop("_mirror_pre", None)), n_unordered

    def item_sim_tri(self, method, cap, slot_target=SLOT_TARGET, ch_min=CH_MIN):
        """baseliner_calculate_sim_pipeline, second formulation (all rows, one GPU).  XMAP_A_V2=1: the round-2 sequence
        (CSC build, CSC-driven rater records, cursor-atomic mirror) -- kept as a cross-check of the round-3 one."""
        if os.environ.get("XMAP_A_V2") == "1":
            with self.timed("stats"):
                stats = self.stats()
            L = self.tri_layout(stats, slot_target, ch_min)
        else:
            stats, L = self.layout3(slot_target, ch_min, pairs_hint=dict(has_ls=False, split=True, count_mir=True))
        S, n_unordered = self._pairs_to_csr(method, cap, stats, L)
        S.method = abi.METHODS[method] if isinstance(method, str) else int(method)
        S.cap = int(cap)
        S.u_avg, S.u_norm = stats[0], stats[1]
        S.n_eval, S.n_contrib = 2 * n_unordered, 2 * L.half_contrib
        S.n_units, S.layout, S.slot_target = L.n_light + L.n_heavy_units, L, L.slot_target
        return S

    def sim_from_device(self, row_ptr, col, sim, mutu, nij, info):
        """Wrap device tensors (e.g. rows gathered from several ranks) as a SimResult."""
        S = SimResult()
        S.n_items = self.R.n_items
        n = int(col.numel())
        if n == 0:
            col = self._zeros(1, torch.int32); sim = self._zeros(1, torch.float64)
            mutu = self._zeros(1, torch.int32); nij = self._zeros(1, torch.int32)
        S.row_ptr, S.info = row_ptr.contiguous(), info
        col, sim, mutu, nij = col.contiguous(), sim.contiguous(), mutu.contiguous(), nij.contiguous()
        S.col, S.sim, S.mutu, S.nij = col[:n], sim[:n], mutu[:n], nij[:n]
        S.n_kept = n
        S.c = abi.Sim(S.n_items, S.row_ptr.data_ptr(), col.data_ptr(), sim.data_ptr(), mutu.data_ptr(),
                      nij.data_ptr(), info.data_ptr())
        S._keep = (col, sim, mutu, nij)
        return S

    def sim_from_host(self, row_ptr, col, sim, mutu, nij, info, frac=None):
        """Wrap a host-side stage-A result (e.g. a canonically re-fed RDD) as a device SimResult.
        With `frac`, frac_mutu is taken from the records instead of being derived from (info, nij)."""
        d = self.dev
        n = int(row_ptr[-1])

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a if n else np.zeros(1), dt)).to(d)
        row_ptr_d = torch.from_numpy(np.ascontiguousarray(row_ptr, np.int64)).to(d)
        info_d = torch.from_numpy(np.ascontiguousarray(info, np.float64)).to(d)
        S = self.sim_from_device(row_ptr_d, up(col, np.int32)[:n], up(sim, np.float64)[:n], up(mutu, np.int32)[:n],
                                 up(nij if nij is not None else np.zeros(max(n, 1)), np.int32)[:n], info_d)
        if frac is not None:
            S.frac = up(frac, np.float64)
            S.c.frac = S.frac.data_ptr()
        return S

    # ------------------------------------------------------------------ stage B
    def knn(self, S, top_k, bb=None, rows=None):
        """B1-B4: bridge flags (computed, or given by the caller) + classified top-k lists.  rows = (lo, hi): the lists of
        that share of the items only (item-sharded ranks all-gather the tables)."""
        R = self.R
        st = _stream(self.dev)
        I, k = R.n_items, int(top_k)
        E = ExtResult()
        E.k = k
        if bb is not None:
            E.bb = bb.to(torch.uint8).contiguous()
        else:
            E.bb = self._zeros(max(I, 1), torch.uint8)
            check(lib.xmap_bridge_flags(st, C.byref(S.c), vp(R.prefix_cls), vp(E.bb)))
        alloc = self._empty if I > 0 else self._zeros      # xmap_knn_classify writes every entry of the rows it is given
        E.cls = alloc(max(I, 1), torch.uint8)                # (item-sharded ranks all-gather the other rows: ext_gather)
        E.kcnt = alloc((max(I, 1), 2), torch.int32)
        E.kcol = alloc((max(I, 1), 2, k), torch.int32)
        E.kval = alloc((max(I, 1), 2, k, 3), torch.float64)
        with self.timed("knn_classify"):
            lo, hi = (0, I) if rows is None else (int(rows[0]), int(rows[1]))
            check(lib.xmap_knn_classify(st, C.byref(S.c), k, vp(E.bb), vp(R.suffix_cls), vp(R.contains_mask),
                                        vp(E.cls), vp(E.kcnt), vp(E.kcol), vp(E.kval), i32(lo), i32(hi)))
        return E

    def _reverse(self, S, E, mode, attach_ptr):
        """one reverse adjacency (mode 0 attach, 1 src, 2 rnn), all rows on this device"""
        st8 = self.reverse_count(S, E, mode, attach_ptr, None)
        self.reverse_fill(st8)
        return st8.out

    def reverse_count(self, S, E, mode, attach_ptr, rows):
        """count pass of one reverse adjacency over the rows [lo, hi) (None: all).  The list of a row is built from that row
        of the similarity matrix alone (the matrix is symmetric: "b lists a" is tested on a's own entry for b), so a rank's
        share of the rows is a contiguous share of the lists -- item-sharded ranks all-gather the pieces (reverse_gather_*)."""
        R = self.R
        I = R.n_items
        st8 = ExtResult()
        st8.S, st8.E, st8.mode = S, E, mode
        st8.rows = (0, I) if rows is None else (int(rows[0]), int(rows[1]))
        st8.rcnt = self._zeros(max(I, 1), torch.int32)
        # one byte per entry of these rows: what the count pass finds, for the fill pass (which then gathers nothing)
        st8.eflag = self._empty(max(int(S.col.numel()), 1), torch.uint8)       # (indexed from the first entry of row lo)
        st8.args = (C.byref(S.c), mode, E.k, vp(E.bb), vp(E.cls), vp(E.kcnt), vp(E.kcol), vp(E.kval),
                    vp(R.suffix_cls), vp(R.contains_mask), vp(R.flags), vp(attach_ptr), vp(getattr(E, "thr", None)),
                    vp(getattr(E, "long_rows", None)), vp(st8.eflag))
        st8.keep = attach_ptr
        check(lib.xmap_reverse_count(_stream(self.dev), *st8.args, vp(st8.rcnt), i32(st8.rows[0]), i32(st8.rows[1])))
        return st8

    def reverse_count_pair(self, S, E, rows):
        """the count passes of the attach (mode 0) and rnn (mode 2) lists as ONE pass over the rows (both ask the non-bridge
        neighbours of an entry, about their two lists): two handles like reverse_count's, sharing the per-entry bytes"""
        R = self.R
        I = R.n_items
        lo, hi = (0, I) if rows is None else (int(rows[0]), int(rows[1]))
        eflag = self._empty(max(int(S.col.numel()), 1), torch.uint8)
        sts = []
        for mode in (0, 2):
            st8 = ExtResult()
            st8.S, st8.E, st8.mode, st8.rows = S, E, mode, (lo, hi)
            st8.rcnt = self._zeros(max(I, 1), torch.int32)
            st8.eflag = eflag
            st8.args = (C.byref(S.c), mode, E.k, vp(E.bb), vp(E.cls), vp(E.kcnt), vp(E.kcol), vp(E.kval),
                        vp(R.suffix_cls), vp(R.contains_mask), vp(R.flags), vp(None), vp(E.thr),
                        vp(getattr(E, "long_rows", None)), vp(eflag))
            st8.keep = None
            sts.append(st8)
        check(lib.xmap_reverse_count_att_rnn(_stream(self.dev), C.byref(S.c), E.k, vp(E.bb), vp(E.cls), vp(E.kcnt), vp(E.kcol),
                                             vp(E.kval), vp(R.suffix_cls), vp(R.contains_mask), vp(R.flags), vp(E.thr),
                                             vp(getattr(E, "long_rows", None)), vp(eflag), vp(sts[0].rcnt), vp(sts[1].rcnt),
                                             i32(lo), i32(hi)))
        return sts

    def reverse_gather_counts(self, sts, comm):
        """collective: every rank's counts of its rows -> the counts of all rows (of several lists in one exchange)"""
        I = self.R.n_items
        lo, hi = sts[0].rows
        for st8, c in zip(sts, comm.all_gather_multi([st8.rcnt[lo:hi] for st8 in sts])):
            st8.rcnt[:I] = c

    def reverse_fill(self, st8):
        """offsets of all rows (scan of the complete counts), then the entries of this device's rows"""
        I = self.R.n_items
        st = _stream(self.dev)
        rptr = self._zeros(I + 1, torch.int64)
        tot = C.c_int64(0)
        check(lib.xmap_exclusive_scan_i32_to_i64(st, vp(st8.rcnt), vp(rptr), i64(I), C.byref(tot)))
        n = int(tot.value)
        ridx = self._empty(max(n, 1), torch.int32)
        rval = self._empty((max(n, 1), 3), torch.float64)
        rflag = self._zeros(max(n, 1), torch.uint8)
        check(lib.xmap_reverse_fill(st, *st8.args, vp(rptr), vp(ridx), vp(rval), vp(rflag), i32(st8.rows[0]), i32(st8.rows[1])))
        st8.out = (rptr, ridx, rval, rflag, n)

    def reverse_gather(self, sts, comm):
        """collective: the ranks' pieces of the lists, in rank (= row) order -- ONE exchange for all the lists given"""
        send = []
        for st8 in sts:
            rptr, ridx, rval, rflag, n = st8.out
            lo, hi = st8.rows
            ends = rptr[[lo, hi]].tolist()
            a, b = int(ends[0]), int(ends[1])
            send += [ridx[a:b], rval[a:b].reshape(-1), rflag[a:b]]
        got = comm.all_gather_multi(send)
        for j, st8 in enumerate(sts):
            rptr, ridx, rval, rflag, n = st8.out
            if n:
                ridx[:n] = got[3 * j]
                rval[:n] = got[3 * j + 1].view(n, 3)
                rflag[:n] = got[3 * j + 2]
        return [st8.out for st8 in sts]

    def path_units(self, E, start_range=None, chunk=None, row_budget=48 << 30, start_split=None):
        """Work units of the path enumeration from the exact per-start path counts: starts with more than
        `chunk` paths are split into G round-robin chunks with dedicated accumulator rows (merged on the
        device afterwards); units are ordered heaviest first."""
        R = self.R
        st = _stream(self.dev)
        I = R.n_items
        tmp = self._zeros(4 * max(I, 1), torch.int64)
        P = self._zeros(max(I, 1), torch.int64)
        with self.timed("path_weights"):
            check(lib.xmap_path_weights(st, C.byref(self._ext_tables(E)), vp(tmp), vp(P)))
        # planning in the library (xmap_path_plan: chunk counts, heaviest-first order by its own radix sort, unit arrays)
        if start_split is not None:   # (rank, world): contiguous start ranges of equal path counts
            from .sharded import balanced_ranges
            start_range = balanced_ranges(P[:I].cpu().numpy(), start_split[1])[start_split[0]]
        lo, hi = (0, I) if start_range is None else (int(start_range[0]), int(start_range[1]))
        row_bytes = 36 * max(I, 1)
        row_budget = int(float(os.environ.get("XMAP_ROW_BUDGET_GB", row_budget / (1 << 30))) * (1 << 30))
        row_budget = min(row_budget, int(0.15 * self.hbm_available("qhacc", "hacc")))      # (the rows of the split heavy starts)
        max_rows = max(row_budget // row_bytes, 2)
        cap_units = max(I, 1) + max_rows
        U = ExtResult()
        U.unit_start = self._empty(cap_units, torch.int32)
        U.unit_c = self._empty(cap_units, torch.int32)
        U.unit_G = self._empty(cap_units, torch.int32)
        U.unit_row = self._empty(cap_units, torch.int32)
        U.heavy_unit0 = self._empty(max(I, 1), torch.int32)
        h = (C.c_int64 * 5)()
        with self.timed("path_plan"):
            check(lib.xmap_path_plan(st, i32(I), vp(P), i32(lo), i32(hi), i64(chunk or 0),
                                     i64(0 if chunk else int(os.environ.get("XMAP_CHUNK_DIV", "8192"))), i64(max_rows),
                                     i64(cap_units), vp(U.unit_start), vp(U.unit_c), vp(U.unit_G), vp(U.unit_row),
                                     vp(U.heavy_unit0), h))
        U.n_units, U.n_heavy, U.n_rows, U.total, U.chunk = int(h[0]), int(h[1]), int(h[2]), int(h[3]), int(h[4])
        U.P = P          # exact path count per start (B5d / B5e)
        # all starts, not only this call's range: what the refusal of extend_tables goes by, so that the ranks of a sharded
        # step decide alike and the message carries the whole problem's count
        U.total_all = int(P[:I].sum().item()) if (I and (start_range is not None or start_split is not None)) else U.total
        U.unit_nt = self._zeros(max(U.n_units, 1), torch.int32)
        return U

    def end_universe(self, E):
        """items that can end a path, ranked by item index: E.urank [I] (-1: not an end), E.uitem [n_ends]"""
        R = self.R
        st = _stream(self.dev)
        I = R.n_items
        T = self._ext_tables(E)
        mark = self._empty(max(I, 1), torch.int32)
        rank = self._empty(I + 1, torch.int64)
        E.urank = self._empty(max(I, 1), torch.int32)
        E.uitem = self._empty(max(I, 1), torch.int32)
        n = C.c_int64(0)
        check(lib.xmap_end_universe(st, C.byref(T), vp(mark), vp(rank), vp(E.urank), vp(E.uitem), C.byref(n)))
        E.n_ends = int(n.value)
        M = getattr(E, "mid", None)
        if os.environ.get("XMAP_URANK_HOME", "1") == "1" and E.n_ends and M is not None:
            # row order: the ends of a column side by side (a column's row update then touches few lines)
            check(lib.xmap_end_order(st, i32(I), E.k, i32(M.n_nb), vp(M.nb_list), vp(E.kcnt), vp(E.kcol), i32(E.n_ends),
                                     vp(E.urank), vp(E.uitem)))

    def _ext_tables(self, E, M=None):
        """xmap_ext_tables of a pass: the one place that maps an ExtResult (and its middle lists M) to pointers.  What E or
        M does not hold yet (reverse lists, middle lists, end universe) comes out 0."""
        p = lambda t: (t.data_ptr() if t is not None else 0)
        g = lambda o, n: getattr(o, n, None) if o is not None else None
        lst = lambda n, w: [p(t) for t in (g(E, n) or (None,) * w)[:w]]      # (ptr, idx, val[, flag]) of a reverse list
        return abi.ExtTables(self.R.n_items, E.k, p(E.cls), p(E.kcnt), p(E.kcol), p(E.kval), p(self.R.flags),
                             *lst("att", 3), *lst("src", 4), *lst("rnn", 3),
                             (M.n_nb if M is not None else 0), p(g(M, "nb_id")), p(g(M, "nb_list")), p(g(M, "midX")),
                             p(g(M, "dir")), p(g(M, "dir_ptr")),
                             getattr(E, "n_ends", 0), p(g(E, "urank")), p(g(E, "uitem")))

    def mid_lists(self, E, table_budget=24 << 30, rows=None):
        """middle lists of all joint paths, one tile of records per (x', x) (csrc/mid_rows.hip).
        rows (default): built row-wise, one block per x' with the row's tile sizes in LDS (abi.MID_ROWS_SPAN columns at a
        time); rows=False / XMAP_MID_TABLE=1: through the dense n_nb x n_nb tile table (cross-check; None when it does not
        fit the budget -- callers fall back to the per-path enumeration)."""
        R = self.R
        st = _stream(self.dev)
        I = R.n_items
        nb_list = self._empty(max(I, 1), torch.int32)
        nb_id = self._empty(max(I, 1), torch.int32)
        nn = C.c_int64(0)
        check(lib.xmap_nb_index(st, i32(I), vp(E.cls), vp(nb_list), vp(nb_id), C.byref(nn)))
        n_nb = int(nn.value)
        nb_list = nb_list[:n_nb]
        if rows is None:
            rows = os.environ.get("XMAP_MID_TABLE") != "1"
        if n_nb == 0 or (not rows and n_nb * n_nb * 12 > table_budget):
            return None
        M = ExtResult()
        M.n_nb, M.nb_list = n_nb, nb_list
        M.nb_id = nb_id
        T = self._ext_tables(E, M)
        if rows:
            with self.timed("mid_build"):
                M.ng = self._empty(n_nb, torch.int32)
                nrec = self._empty(n_nb, torch.int64)
                check(lib.xmap_mid_rows_count(st, C.byref(T), vp(M.ng), vp(nrec)))
                M.dir_ptr = self._zeros(n_nb + 1, torch.int64)
                rec_ptr = self._zeros(n_nb + 1, torch.int64)
                tx, tg = C.c_int64(0), C.c_int64(0)
                check(lib.xmap_exclusive_scan_i32_to_i64(st, vp(M.ng), vp(M.dir_ptr), i64(n_nb), C.byref(tg)))
                check(lib.xmap_exclusive_scan_i64(st, vp(nrec), vp(rec_ptr), i64(n_nb), C.byref(tx)))
                M.n_records, M.n_tiles = int(tx.value), int(tg.value)
                budget = float(os.environ.get("XMAP_MID_BUDGET_GB", "100")) * 1e9
                if 64.0 * M.n_records + 24.0 * M.n_tiles > budget:
                    return None         # the lists do not fit: the caller enumerates path by path
                M.dir = self._empty(max(M.n_tiles, 1) * 3, torch.int64)
                M.midX = self._empty(max(M.n_records, 1) * 8, torch.float64)
                T.dir_ptr = M.dir_ptr.data_ptr()
                check(lib.xmap_mid_rows_place(st, C.byref(T), vp(rec_ptr), vp(M.dir), vp(M.midX)))
            return M
        with self.timed("mid_build"):
            tile_cnt = self._empty(n_nb * n_nb, torch.int32)
            M.ng = self._zeros(n_nb, torch.int32)
            abi.xcheck(abi.xlib().xmap_mid_tally(st, C.byref(T), vp(tile_cnt), vp(M.ng)))
            tile_off = self._empty(n_nb * n_nb + 1, torch.int64)
            M.dir_ptr = self._zeros(n_nb + 1, torch.int64)
            tx, tg = C.c_int64(0), C.c_int64(0)
            check(lib.xmap_exclusive_scan_i32_to_i64(st, vp(tile_cnt), vp(tile_off), i64(n_nb * n_nb), C.byref(tx)))
            check(lib.xmap_exclusive_scan_i32_to_i64(st, vp(M.ng), vp(M.dir_ptr), i64(n_nb), C.byref(tg)))
            M.n_records, M.n_tiles = int(tx.value), int(tg.value)
            M.dir = self._empty(max(M.n_tiles, 1) * 3, torch.int64)
            M.midX = self._empty(max(M.n_records, 1) * 8, torch.float64)
            T.dir_ptr = M.dir_ptr.data_ptr()
            abi.xcheck(abi.xlib().xmap_mid_place(st, C.byref(T), vp(tile_cnt), vp(tile_off), vp(M.dir), vp(M.midX)))
        return M

    def _enumerate(self, E, U, M, full, xs_cap, start_range, row_len, scratch, n_slots, slot_budget, n_cnt, call, chk=check):
        """What the forms of the enumeration share: n_slots (capped by slot_budget and the units) + U.n_rows zero-filled
        accumulator rows of row_len entries -- scratch = the names of the two buffers --, the candidate arrays, n_cnt
        counters and the list buffers, sized again when the pass reports ERR_CAPACITY.  call(T, Un, Rw, O, d_cnt, h_cnt)
        makes the one library call and returns its code (chk raises on it).  Returns (n_slots, h_cnt)."""
        I = self.R.n_items
        n_slots = int(max(4, min(n_slots, slot_budget // (36 * row_len), max(U.n_units, 4))))
        acc = self._zero_scratch(scratch[0], n_slots * row_len * 4, torch.float64)
        touched = self._empty(n_slots * row_len, torch.int32)
        hacc = self._zero_scratch(scratch[1], max(U.n_rows, 1) * row_len * 4, torch.float64) if U.n_rows else None
        htouched = self._empty(max(U.n_rows, 1) * row_len, torch.int32) if U.n_rows else None
        E.n_cand = self._zeros(max(I, 1), torch.int32)
        E.top_end = torch.full((max(I, 1), abi.TOPC), -1, dtype=torch.int32, device=self.dev)
        E.top_val = self._zeros((max(I, 1), abi.TOPC), torch.float64)
        d_cnt = self._zeros(n_cnt, torch.int64)
        h_cnt = (C.c_int64 * n_cnt)()
        T = self._ext_tables(E, M)
        Un = abi.PathUnits(U.n_units, U.unit_start.data_ptr(), U.unit_c.data_ptr(), U.unit_G.data_ptr(), U.unit_row.data_ptr(),
                           U.unit_nt.data_ptr(), U.n_heavy, U.heavy_unit0.data_ptr())
        Rw = abi.PathRows(n_slots, acc.data_ptr(), touched.data_ptr(), hacc.data_ptr() if hacc is not None else 0,
                          htouched.data_ptr() if htouched is not None else 0)
        cap = 0
        if full:
            cap = int(xs_cap) if xs_cap else 1 << 22
        while True:
            xs_off = self._zeros(max(I, 1), torch.int64) if cap else None
            xs_end = self._empty(max(cap, 1), torch.int32) if cap else None
            xs_val = self._empty(max(cap, 1), torch.float64) if cap else None
            O = abi.PathOut(E.n_cand.data_ptr(), E.top_end.data_ptr(), E.top_val.data_ptr(), cap,
                            xs_off.data_ptr() if cap else 0, xs_end.data_ptr() if cap else 0, xs_val.data_ptr() if cap else 0)
            try:
                with self.timed("paths"):
                    rc = call(T, Un, Rw, O, d_cnt, h_cnt)
                if rc == abi.ERR_CAPACITY:      # the pass itself completed (rows are back to zero): lists did not fit
                    cap = int(h_cnt[0])
                    continue
                chk(rc)
            except BaseException:
                self._drop_scratch(*scratch)    # a failed pass may leave partial sums behind
                raise
            break
        E.n_out, E.n_paths = int(h_cnt[0]), int(h_cnt[1])
        E.xs_off, E.xs_end, E.xs_val = xs_off, xs_end, xs_val
        E.start_range = (0, I) if start_range is None else tuple(start_range)
        return n_slots, h_cnt

    def _extend_cols(self, E, U, M, full, xs_cap, start_range, n_slots):
        """xmap_extend_cols: one set of lanes and one row update per column, rows indexed by end rank"""
        st = _stream(self.dev)
        with self.timed("paths_prep"):
            self.end_universe(E)
        nU = max(E.n_ends, 1)
        # the accumulator rows (36 B x ends each: one per resident wave) take what the device can spare: 45 % of the HBM this
        # process could still get (free + what its caching allocator holds unused + the rows of an earlier pass), at most
        # XMAP_SLOT_BUDGET_GB -- fewer rows only mean fewer waves in flight (the S1 shape of the reference's report, 5.3e5
        # ends, peaked at 129 GB with a fixed 120 GB allowance)
        slot_budget = min(int(float(os.environ.get("XMAP_SLOT_BUDGET_GB", "120")) * (1 << 30)), int(0.45 * self.hbm_available("qacc")))
        if "XMAP_N_SLOTS" in os.environ:
            n_slots = int(os.environ["XMAP_N_SLOTS"])
        else:       # one row per wave the kernel keeps resident (P_WAVES per SIMD: csrc/paths4.hip)
            ns = C.c_int32(0)
            check(lib.xmap_extend_cols_slots(C.byref(ns)))
            n_slots = min(n_slots, int(ns.value))
        fast = 0 if os.environ.get("XMAP_SLOW_DIV") == "1" else int(getattr(E, "fast_div", 0))
        n_slots, h_cnt = self._enumerate(
            E, U, M, full, xs_cap, start_range, nU, ("qacc", "qhacc"), n_slots, slot_budget, 8,
            lambda T, Un, Rw, O, d_cnt, h_cnt: lib.xmap_extend_cols(st, C.byref(T), C.byref(Un), C.byref(Rw), C.byref(O), fast,
                                                                    vp(d_cnt), h_cnt))
        E.n_updates = int(h_cnt[4])
        E.row_info = dict(n_slots=n_slots, ends=nU, slot_rows_gb=n_slots * nU * 36 / 1e9, heavy_rows=int(U.n_rows),
                          heavy_rows_gb=int(U.n_rows) * nU * 36 / 1e9, slot_budget_gb=slot_budget / 1e9)
        return E

    def ext_tables(self, S, top_k, comm=None):
        """B1-B5b: bridge flags, classified top-k lists and the three reverse adjacencies (attach / src / rnn).
        comm (xmap.engine.sharded.Comm of several ranks): every rank classifies a share of the rows -- contiguous ranges of
        equal entry counts -- and the tables are all-gathered (the reference broadcasts them, utils/assist.py:93-95).
        Three phases (a sharded caller puts its collective error check between them: ext_knn and ext_reverse may raise,
        ext_gather holds every collective and nothing else)."""
        E = self.ext_knn(S, top_k, comm)
        self.ext_gather(E, comm)
        return self.ext_reverse(S, E)

    def row_shares(self, tot, world):
        """cut points of `world` contiguous row shares of (about) equal entries; tot [I] = entries per row"""
        I = self.R.n_items
        cum = torch.cumsum(tot[:I].long(), 0)
        tgt = (cum[I - 1].double() * torch.arange(1, world, dtype=torch.float64, device=self.dev) / world).long()
        cuts = [0] + (torch.searchsorted(cum, tgt, right=False) + 1).clamp(max=I).tolist() + [I]
        return np.maximum.accumulate(np.asarray(cuts))

    def bridge_flags(self, S):
        """B1: has the item a neighbour of the other domain?  From the rows S holds (an item-sharded rank: its share; the
        flags of the other rows come out 0 and are all-reduced by the caller)."""
        I = self.R.n_items
        bb = self._zeros(max(I, 1), torch.uint8)
        check(lib.xmap_bridge_flags(_stream(self.dev), C.byref(S.c), vp(self.R.prefix_cls), vp(bb)))
        return bb

    def ext_knn(self, S, top_k, comm=None, rows=None, bb=None):
        """local part: the classified top-k lists of this rank's share of the rows (all rows without comm; rows = (lo, hi):
        that share -- S then holds only those rows, and bb must be the complete bridge flags: a neighbour's class is read)"""
        I = self.R.n_items
        if rows is None and comm is not None and comm.world > 1 and I > 0:
            w = comm.world
            tgt = (S.row_ptr[I].double() * torch.arange(1, w, dtype=torch.float64, device=self.dev) / w).long()
            cuts = [0] + torch.searchsorted(S.row_ptr[:I + 1].contiguous(), tgt).clamp(max=I).tolist() + [I]
            cuts = np.maximum.accumulate(np.asarray(cuts))
            rows = (int(cuts[comm.rank]), int(cuts[comm.rank + 1]))
        E = self.knn(S, top_k, bb=bb, rows=rows)
        E.rows = rows
        E.row_share = rows          # (kept for the reverse lists of a sharded step)
        ok = C.c_int32(1)
        check(lib.xmap_edge_ranges(_stream(self.dev), C.byref(S.c), C.byref(ok)))
        E.fast_div = int(ok.value)       # the bare division sequence of k_paths4 is the division for these edge values
        return E

    def ext_gather(self, E, comm):
        """collectives only: the ranks' shares of the knn tables, all-gathered"""
        rows = getattr(E, "rows", None)
        if rows is None:
            return E
        I = self.R.n_items
        lo, hi = rows
        with self.timed("knn_gather"):
            k = E.k
            fd = torch.tensor([E.fast_div], dtype=torch.int64, device=self.dev)      # (every rank checked its own rows' edges)
            comm.all_reduce(fd, "min")
            E.fast_div = int(fd.item())
            cls, kcnt, kcol, kval = comm.all_gather_multi([E.cls[lo:hi], E.kcnt[lo:hi].reshape(-1), E.kcol[lo:hi].reshape(-1),
                                                           E.kval[lo:hi].reshape(-1)])       # (one exchange for the four tables)
            E.cls[:I] = cls
            E.kcnt[:I] = kcnt.view(I, 2)
            E.kcol[:I] = kcol.view(I, 2, k)
            E.kval[:I] = kval.view(I, 2, k, 3)
        E.rows = None
        return E

    def ext_thresholds(self, E):
        I = self.R.n_items
        E.thr = self._empty(max(I, 1) * 4, torch.float64)      # last entry of every list, 16 B each
        check(lib.xmap_knn_thresholds(_stream(self.dev), i32(I), E.k, vp(E.kcnt), vp(E.kcol), vp(E.kval), vp(E.thr)))
        E.long_rows = self._empty(max(I, 1) + 1, torch.int32)

    def ext_reverse(self, S, E):
        """local part: list thresholds and the three reverse adjacencies from the complete knn tables (item-sharded ranks
        run the three in row shares: xmap.engine.sharded._stage_b)"""
        with self.timed("reverse"):
            self.ext_thresholds(E)
            if getattr(E, "thr", None) is not None and os.environ.get("XMAP_REV_SEPARATE") != "1":
                st_att, st_rnn = self.reverse_count_pair(S, E, None)      # attach + rnn: one count pass for both
                self.reverse_fill(st_att)
                self.reverse_fill(st_rnn)
                E.att, E.rnn = st_att.out, st_rnn.out
            else:
                E.att = self._reverse(S, E, 0, None)
                E.rnn = self._reverse(S, E, 2, None)
            E.src = self._reverse(S, E, 1, E.att[0])
        return E

    def ext_tables_from_knn(self, top_k, cls, kcnt, kcol, kval):
        """The same tables from classified top-k lists alone (host arrays: cls [I], kcnt [I][2], kcol [I][2][k],
        kval [I][2][k][3]) -- what ExtendSim.sim_extend is handed by a caller that ran find_knn_items /
        extract_siminfo itself (reference core/extender.py:46-81,171-178).  The reverse lists are small (<= 2 k I
        entries): built on the host, in list order."""
        R = self.R
        I, k = R.n_items, int(top_k)
        dev = self.dev
        flags = R.flags[:I].cpu().numpy()
        cls = np.ascontiguousarray(cls, np.uint8)
        kcnt = np.ascontiguousarray(kcnt, np.int32).reshape(I, 2)
        kcol = np.ascontiguousarray(kcol, np.int32).reshape(I, 2, k)
        kval = np.ascontiguousarray(kval, np.float64).reshape(I, 2, k, 3)

        def entries(rows, lst):
            """(row item, position) of the valid entries of list `lst` of the given rows"""
            c = kcnt[rows, lst]
            r = np.repeat(rows, c)
            q = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
            return r, q

        def csr(keys, idx, vals, flag=None):
            o = np.argsort(keys, kind="stable")
            ptr = np.zeros(I + 1, np.int64)
            np.cumsum(np.bincount(keys, minlength=I), out=ptr[1:])
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a if len(a) else np.zeros((1,) + a.shape[1:]), dt)).to(dev)
            return (torch.from_numpy(ptr).to(dev), t(idx[o], np.int32), t(vals[o], np.float64),
                    t((flag[o] if flag is not None else np.zeros(len(o))), np.uint8), len(o))
        nb = np.nonzero(cls == 2)[0]
        # attach(b) = [x : x non-bridge record, b in NB_BB(x)];  rnn(y) = [x : y in NB_NN(x)]
        x0, q0 = entries(nb, 0)
        att = csr(kcol[x0, 0, q0].astype(np.int64), x0, kval[x0, 0, q0])
        x1, q1 = entries(nb, 1)
        rnn = csr(kcol[x1, 1, q1].astype(np.int64), x1, kval[x1, 1, q1])
        natt = np.diff(att[0].cpu().numpy())
        # src(t) = [s : s bridge, "S:" in s, attach(s) not empty, t in the lists of s, "T:" in t]; joint iff (t, s) is in TGT too
        bs = np.nonzero((cls == 1) & ((flags & 1) != 0) & (natt > 0))[0]
        s_, t_, v_ = [], [], []
        for lst in (0, 1):
            r, q = entries(bs, lst)
            s_.append(r); t_.append(kcol[r, lst, q]); v_.append(kval[r, lst, q])
        s_ = np.concatenate(s_) if s_ else np.zeros(0, np.int64)
        t_ = np.concatenate(t_).astype(np.int64) if t_ else np.zeros(0, np.int64)
        v_ = np.concatenate(v_) if v_ else np.zeros((0, 3))
        keep = (flags[t_] & 2) != 0
        s_, t_, v_ = s_[keep], t_[keep], v_[keep]
        # TGT: t bridge, "T:" in t, attach(t) not empty, s in the lists of t
        tgt_ok = (cls[t_] == 1) & (natt[t_] > 0)
        in_t = np.zeros(len(t_), bool)
        for lst in (0, 1):
            m = (np.arange(k)[None, :] < kcnt[t_, lst][:, None]) & (kcol[t_, lst, :] == s_[:, None])
            in_t |= m.any(axis=1)
        src = csr(t_, s_, v_, (tgt_ok & in_t).astype(np.uint8))
        E = ExtResult()
        E.k = k
        t = lambda a: torch.from_numpy(a).to(dev)
        E.cls, E.kcnt, E.kcol, E.kval = t(cls), t(kcnt), t(kcol), t(kval)
        E.bb = t((cls == 1).astype(np.uint8))
        E.att, E.src, E.rnn = att, src, rnn
        valid = np.arange(k)[None, None, :] < kcnt[:, :, None]
        mu, smv = kval[..., 1][valid], np.abs(kval[..., 0][valid] * kval[..., 1][valid])
        E.fast_div = int(bool(np.all(mu >= 1.0) and np.all((smv == 0) | ((smv > 2.0 ** -400) & (smv < 2.0 ** 400)))))
        return E

    def extend(self, S, top_k, full=False, start_range=None, n_slots=5120, xs_cap=None, chunk=None,
               start_split=None, algo="cols", comm=None):
        """extender_pipeline: knn tables, reverse adjacencies, streamed path enumeration."""
        return self.extend_tables(self.ext_tables(S, top_k, comm), full, start_range, n_slots, xs_cap, chunk, start_split, algo)

    def extend_lists(self, E):
        """the full X-Sim lists of a pass that kept the candidate arrays only (lazy extended_simRDD): the enumeration is
        run once more with the list buffers sized exactly from n_cand"""
        if getattr(E, "xs_end", None) is None:
            total = int(E.n_cand.sum().item())
            self.extend_tables(E, True, E.start_range, xs_cap=max(total, 1), algo=E.algo)
        return E

    def extend_tables(self, E, full=False, start_range=None, n_slots=5120, xs_cap=None, chunk=None,
                      start_split=None, algo="cols"):
        """B5c-B6 on prepared tables: work units, middle lists, path enumeration, fused top-XMAP_TOPC"""
        R = self.R
        I = R.n_items
        st = _stream(self.dev)
        E.algo = algo
        U = self.path_units(E, start_range, chunk, start_split=start_split)
        # The path count is the reference's algorithm, not the engine's: every joint (t, s) multiplies the attach lists of
        # both ends (core/extender.py:142-169), so a thin bridge set with long lists and a long k explode it (the S1 shape
        # of the reference's report has 2.9e10 paths at its own k = 10 and 5.8e13 at k = 50).  Refuse up front what would
        # take hours, instead of dying in an allocation.
        max_paths = float(os.environ.get("XMAP_MAX_PATHS", "5e12"))
        if U.total_all > max_paths:
            raise abi.XmapError(abi.ERR_CAPACITY, "the extension has %.3g paths at top_k = %d (limit XMAP_MAX_PATHS = %.3g): "
                                "use a shorter list" % (U.total_all, E.k, max_paths))
        M = getattr(E, "mid", None)
        if M is None:
            M = self.mid_lists(E) if algo in ("mid", "cols") else None
        if algo == "cols" and M is None:
            algo = "enum"           # no non-bridge records (nothing joint) or the lists do not fit: per-path enumeration
        E.units = U
        E.mid = M
        if algo == "cols":
            return self._extend_cols(E, U, M, full, xs_cap, start_range, n_slots)
        # one private accumulator row (36 B per item) per resident wave: 5 waves per SIMD = 5120 rows on 256 CUs
        slot_budget = int(float(os.environ.get("XMAP_SLOT_BUDGET_GB", "100")) * (1 << 30))
        n_slots = int(os.environ.get("XMAP_N_SLOTS", n_slots))
        if M is not None:       # algo="mid": the tile-major test formulation over the middle lists
            call = lambda T, Un, Rw, O, d_cnt, h_cnt: abi.xlib().xmap_extend_paths2(
                st, C.byref(T), C.byref(Un), C.byref(Rw), C.byref(O), vp(M.ng), vp(d_cnt), h_cnt)
        else:
            call = lambda T, Un, Rw, O, d_cnt, h_cnt: lib.xmap_extend_paths(
                st, C.byref(T), C.byref(Un), C.byref(Rw), C.byref(O), vp(d_cnt), h_cnt)
        self._enumerate(E, U, M, full, xs_cap, start_range, max(I, 1), ("acc", "hacc"), n_slots, slot_budget, 4, call,
                        abi.xcheck if M is not None else check)
        return E

    # ------------------------------------------------------------------ dense item-factor variant
    def dense_topk(self, F_t, F_s, top_k):
        """Row-wise top-k of cosine(F_t[i], F_s[j]) by (|sim| desc, j asc) on the fp32 matrix cores.
        F_t [n_t, K], F_s [n_s, K]: host or device float32.  Returns (idx int32 [n_t, k], val float32 [n_t, k])."""
        st = _stream(self.dev)
        to = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.float32))).to(
            self.dev, torch.float32).contiguous()
        Ft, Fs = to(F_t), to(F_s)
        n_t, K = Ft.shape
        n_s = Fs.shape[0]
        Fnt, Fns = torch.empty_like(Ft), torch.empty_like(Fs)
        with self.timed("dense_normalize"):
            check(lib.xmap_dense_normalize(st, i32(n_t), i32(K), vp(Ft), vp(Fnt)))
            check(lib.xmap_dense_normalize(st, i32(n_s), i32(K), vp(Fs), vp(Fns)))
        idx = self._empty((max(n_t, 1), top_k), torch.int32)
        val = self._empty((max(n_t, 1), top_k), torch.float32)
        npc = C.c_int32(1)
        check(lib.xmap_dense_layout(i32(n_t), i32(n_s), C.byref(npc)))
        n_pieces = int(npc.value)
        pidx = self._empty((max(n_t, 1), n_pieces, top_k), torch.int32) if n_pieces > 1 else None
        pval = self._empty((max(n_t, 1), n_pieces, top_k), torch.float32) if n_pieces > 1 else None
        with self.timed("dense_topk"):
            check(lib.xmap_dense_topk(st, i32(n_t), i32(n_s), i32(K), vp(Fnt), vp(Fns), i32(top_k), i32(n_pieces),
                                      vp(pidx), vp(pval), vp(idx), vp(val)))
        return idx[:n_t], val[:n_t]

    def dense_extend(self, F, top_k):
        """Dense replacement of stages A+B (BASELINE configs[4]): F [I, K] item factors; target-side items ("T:" in
        iid) are the starts, source-side items ("S:" in iid) the candidates.  Returns an ExtResult with the same
        candidate arrays extend() produces, so select() / alterego() run unchanged."""
        R = self.R
        I = R.n_items
        F = (F if torch.is_tensor(F) else torch.from_numpy(np.ascontiguousarray(F, np.float32))).to(self.dev)
        tgt = torch.nonzero((R.flags[:I] & 2) != 0).flatten()
        src = torch.nonzero((R.flags[:I] & 1) != 0).flatten()
        idx, val = self.dense_topk(F[tgt], F[src], top_k)
        E = ExtResult()
        E.k = top_k
        E.dense_idx, E.dense_val, E.tgt, E.src = idx, val, tgt, src
        E.n_cand = self._zeros(max(I, 1), torch.int32)
        E.top_end = torch.full((max(I, 1), abi.TOPC), -1, dtype=torch.int32, device=self.dev)
        E.top_val = self._zeros((max(I, 1), abi.TOPC), torch.float64)
        c = min(abi.TOPC, top_k)
        valid = idx >= 0
        E.n_cand[tgt] = valid.sum(dim=1).to(torch.int32)
        ends = torch.where(valid[:, :c], src[idx[:, :c].clamp(min=0).long()].to(torch.int32),
                           torch.full_like(idx[:, :c], -1))
        E.top_end[tgt, :c] = ends
        E.top_val[tgt, :c] = val[:, :c].double()
        return E

    # ------------------------------------------------------------------ stage C
    def select(self, E, private, picks=None):
        R = self.R
        st = _stream(self.dev)
        I = R.n_items
        n_top = self._out(max(I, 1), torch.int32, I > 0)      # written for every start / filled by the library
        choice = self._out(max(I, 1), torch.int32, I > 0)
        mp = self._out(max(I, 1), torch.int32, I > 0)
        pk = None
        if picks is not None:
            pk = torch.from_numpy(np.ascontiguousarray(picks, np.int32)).to(self.dev)
        with self.timed("c_select"):
            check(lib.xmap_select_map(st, i32(I), 1 if private else 0, vp(E.n_cand), vp(E.top_end), vp(pk),
                                      vp(n_top), vp(choice), vp(mp)))
        return n_top, choice, mp

    def alterego(self, mp, users=None):
        """build_alterEgo (core/generator.py:113-157) over all users, or over the users [users[0], users[1])"""
        R = self.R
        st = _stream(self.dev)
        U = R.n_users
        Rc = R.c
        if users is not None:       # a share of the users (an item-sharded rank's part of stage C): rows carry GLOBAL user indices
            u_lo, u_hi = int(users[0]), int(users[1])
            U = u_hi - u_lo
            Rc = abi.Ratings.from_buffer_copy(R.c)
            Rc.n_users = U
            Rc.user_ptr = R.user_ptr.data_ptr() + 8 * u_lo
        cnt_t = self._empty(max(U, 1), torch.int32)
        cnt_m = self._empty(max(U, 1), torch.int32)
        if U == 0:
            cnt_t.zero_(); cnt_m.zero_()
        d_prof = self._zeros(64, torch.int64)            # sharded counter of the users with output rows
        with self.timed("c_count"):
            check(lib.xmap_alterego_count(st, C.byref(Rc), vp(mp), vp(cnt_t), vp(cnt_m), vp(d_prof)))
            off_t = self._empty(U + 1, torch.int64)
            off_m = self._empty(U + 1, torch.int64)
            check(lib.xmap_exclusive_scan_i32_to_i64(st, vp(cnt_t), vp(off_t), i64(U), None))
            check(lib.xmap_exclusive_scan_i32_to_i64(st, vp(cnt_m), vp(off_m), i64(U), None))
            # the three totals in ONE synchronisation (the scans leave theirs in out[U])
            h = self._pinned3()
            h[0:1].copy_(off_t[U:U + 1], non_blocking=True)
            h[1:2].copy_(off_m[U:U + 1], non_blocking=True)
            h[2:66].copy_(d_prof, non_blocking=True)
            torch.cuda.current_stream(self.dev).synchronize()
            nt, nm, n_prof = int(h[0]), int(h[1]), int(h[2:66].sum())
        n = nt + nm
        G = GenResult()
        G.user = self._empty(max(n, 1), torch.int32)
        G.item = self._empty(max(n, 1), torch.int32)
        G.rating = self._empty(max(n, 1), torch.float64)      # pass-through ratings and np.mean of the merged ones (fp64)
        G.time = self._empty(max(n, 1), torch.int64)
        with self.timed("c_fill"):
            check(lib.xmap_alterego_fill(st, C.byref(Rc), vp(mp), vp(off_t), vp(off_m), i64(nt),
                                         vp(G.user), vp(G.item), vp(G.rating), vp(G.time)))
            if users is not None and u_lo:
                G.user += u_lo
        G.n_rows, G.n_target_rows = n, nt
        G.cnt_t, G.cnt_m = cnt_t, cnt_m
        G.off_t, G.off_m = off_t, off_m      # (the device-resident tail groups the rows by user from these: alterego_profiles)
        G.n_profiles = n_prof
        G.map = mp                           # (fold-in builds the profiles of later arrivals with it: foldin_profiles)
        G.user, G.item, G.rating, G.time = G.user[:n], G.item[:n], G.rating[:n], G.time[:n]
        return G

    def alterego_profiles(self, G, time_key=None):
        """The AlterEgo rows of alterego() as user-major profiles, built on the device (xmap_rec_profiles): a user's rows
        contiguous and in stage-C row order, item indices unchanged.  Returns a DeviceRatings-compatible view (fp64 ratings,
        rating64) -- Engine(view).rec_sim(cap) is RecommenderSim over the rows without a host copy.  time_key: an int64
        tensor to carry instead of G.time (a caller whose G.time holds positions passes the rank of its time objects)."""
        R = self.R
        st = _stream(self.dev)
        U, n = R.n_users, int(G.n_rows)
        n1 = max(n, 1)
        tm = G.time if time_key is None else time_key.contiguous()
        ptr = self._empty(U + 1, torch.int64)
        item = self._empty(n1, torch.int32)
        rating = self._empty(n1, torch.float64)
        time = self._empty(n1, torch.int64)
        with self.timed("rec_profiles"):
            check(lib.xmap_rec_profiles(st, i64(U), i64(n), i64(G.n_target_rows), vp(G.off_t), vp(G.off_m), vp(G.user), vp(G.item),
                                        vp(G.rating), vp(tm), vp(ptr), vp(item), vp(rating), vp(time)))
        P = self._profile_view(U, n, ptr, item, rating, time)
        if getattr(G, "map", None) is not None and int(G.off_t.numel()) == U + 1:
            # what explain_sources walks: the raw profiles the rows were made from, the scan of the pass-through counts, the map
            P.sources = (R.user_ptr, R.user_item, None, G.off_t, R.flags, G.map)
        return P

    def _profile_view(self, U, n, ptr, item, rating, time):
        """user-major AlterEgo profiles (ptr [U + 1], item / rating fp64 / time of max(n, 1) entries) as a
        DeviceRatings-compatible view over the item space of the engine's ratings"""
        R = self.R
        n1 = max(n, 1)
        P = object.__new__(DeviceRatings)
        P.device, P.n_users, P.n_items, P.nnz = R.device, U, R.n_items, n
        P.plain_exact = False
        d = ptr[1:] - ptr[:-1]
        P.half_contrib = int((d * (d - 1) // 2).sum().item()) if U else 0
        P.user_ptr, P.user_item, P.user_rating64, P.user_time = ptr, item, rating, time
        P.user_rating = rating.float()
        P.item_ptr = torch.zeros(R.n_items + 1, dtype=torch.int64, device=self.dev)
        P.item_user = torch.zeros(n1, dtype=torch.int32, device=self.dev)
        P.item_rating = torch.zeros(n1, dtype=torch.float32, device=self.dev)
        P.csc_ready = False
        P.prefix_cls, P.suffix_cls, P.contains_mask, P.flags = R.prefix_cls, R.suffix_cls, R.contains_mask, R.flags
        P.c = abi.Ratings(U, R.n_items, n, ptr.data_ptr(), item.data_ptr(), P.user_rating.data_ptr(), time.data_ptr(),
                          P.item_ptr.data_ptr(), P.item_user.data_ptr(), P.item_rating.data_ptr(), R.prefix_cls.data_ptr(),
                          R.suffix_cls.data_ptr(), R.contains_mask.data_ptr(), R.flags.data_ptr())
        return P

    def foldin_profiles(self, ptr, item, rating, time, mp):
        """Fold-in (xmap_foldin_count / xmap_foldin_fill): the AlterEgo profiles of a batch of raw profiles that are not rows
        of the engine's ratings, with the replacement map mp of select() / alterego().map.  ptr [B + 1] int64, item int32 (the
        engine's index space, source and target items mixed, repeats allowed), rating float32, time int64 -- NumPy arrays or
        tensors.  The batch is checked on the device before anything indexes the map (an item outside [0, n_items), a ptr that
        is not a CSR's: XmapError, code ERR_ARG).  Returns the DeviceRatings-compatible view alterego_profiles returns, with
        n_users = B -- predict() and topn() take it as is, user indices then count within the batch -- and .counts = (rows,
        pass-through rows, profiles with a row).  The model stays frozen: nothing resident changes."""
        R = self.R
        st = _stream(self.dev)

        def dev(a, dt):
            if not torch.is_tensor(a):
                a = torch.from_numpy(np.ascontiguousarray(a, dt))
            return a.to(device=self.dev, dtype=getattr(torch, np.dtype(dt).name)).contiguous()
        ptr, item, rating, time = dev(ptr, np.int64), dev(item, np.int32), dev(rating, np.float32), dev(time, np.int64)
        B, nnz = int(ptr.numel()) - 1, int(item.numel())
        if B < 0 or rating.numel() != nnz or time.numel() != nnz:
            raise ValueError("fold-in batch: ptr needs an entry, item / rating / time one length")
        cnt_t = self._empty(max(B, 1), torch.int32)
        cnt_m = self._empty(max(B, 1), torch.int32)
        pptr = self._empty(B + 1, torch.int64)
        h = (C.c_int64 * 3)(0, 0, 0)
        with self.timed("foldin_count"):
            check(lib.xmap_foldin_count(st, i64(B), i64(nnz), vp(ptr), vp(item), i32(R.n_items), vp(R.flags), vp(mp), vp(cnt_t),
                                        vp(cnt_m), vp(pptr), h))
        n = int(h[0])
        pit = self._empty(max(n, 1), torch.int32)
        pra = self._empty(max(n, 1), torch.float64)
        pti = self._empty(max(n, 1), torch.int64)
        with self.timed("foldin_fill"):
            check(lib.xmap_foldin_fill(st, i64(B), i64(nnz), vp(ptr), vp(item), vp(rating), vp(time), i32(R.n_items), vp(R.flags),
                                       vp(mp), vp(cnt_t), vp(pptr), vp(pit), vp(pra), vp(pti)))
        P = self._profile_view(B, n, pptr, pit, pra, pti)
        P.counts = tuple(int(x) for x in h)
        P.sources = (ptr, item, cnt_t, None, R.flags, mp)       # the batch's own raw profiles (explain_sources)
        return P

    def item_foldin(self, P, ptr, user, rating, item_norm, cap, max_records=0):
        """Item fold-in (xmap_itemfold_count / xmap_itemfold_fill): one row of RecommenderSim per item of a batch of items that are
        not in the model, against the frozen profiles P (alterego_profiles / union_profiles) and the norms item_norm [I] of
        rec_sim (S.norm), weighted with its cap.  The batch is a CSR of raters: ptr [B + 1] int64, user int32 (indices of P's
        users, repeats allowed), rating float64 -- NumPy arrays or tensors; there are no times, and a batch rating is never
        evidence.  The batch is checked on the device first (a user outside [0, n_users), a ptr that is not a CSR's: XmapError,
        code ERR_ARG).  max_records: records (rater entry x profile row) per chunk of the sort, 0 = the library's default; the
        result does not depend on it.  Returns (rows, avg [B], norm [B]) on the device; rows is a SimResult-like object with
        row_ptr [B + 1], col (resident indices), sim, ls, nij -- rows not sorted -- .avg / .norm, .ptr / .user (the batch's CSR on the device,
        what audience(batch=) takes) and .counts = (pairs, records, items with a pair).  Nothing resident changes."""
        st = _stream(self.dev)

        def dev(a, dt):
            if not torch.is_tensor(a):
                a = torch.from_numpy(np.ascontiguousarray(a, dt))
            return a.to(device=self.dev, dtype=getattr(torch, np.dtype(dt).name)).contiguous()
        ptr, user, rating = dev(ptr, np.int64), dev(user, np.int32), dev(rating, np.float64)
        B, nnz = int(ptr.numel()) - 1, int(user.numel())
        if B < 0 or rating.numel() != nnz:
            raise ValueError("item fold-in batch: ptr needs an entry, user / rating one length")
        norm_in = item_norm.to(device=self.dev, dtype=torch.float64).contiguous()
        if int(norm_in.numel()) < P.n_items:
            raise ValueError("item fold-in: item_norm holds %d norms, the profiles' item space has %d" % (norm_in.numel(), P.n_items))
        cnt = self._empty(max(B, 1), torch.int32)
        row_ptr = self._empty(B + 1, torch.int64)
        h = (C.c_int64 * 3)(0, 0, 0)
        with self.timed("itemfold_count"):
            check(lib.xmap_itemfold_count(st, i64(B), i64(nnz), vp(ptr), vp(user), i64(P.n_users), i32(P.n_items), vp(P.user_ptr),
                                          vp(P.user_item), i64(max_records), vp(cnt), vp(row_ptr), h))
        n = int(h[0])
        S = SimResult()
        S.n_items, S.n_kept, S.row_ptr = B, n, row_ptr
        S.col = self._empty(max(n, 1), torch.int32)
        S.sim = self._empty(max(n, 1), torch.float64)
        S.ls = self._empty(max(n, 1), torch.float64)
        S.nij = self._empty(max(n, 1), torch.int32)
        avg = self._empty(max(B, 1), torch.float64)
        norm = self._empty(max(B, 1), torch.float64)
        with self.timed("itemfold_fill"):
            check(lib.xmap_itemfold_fill(st, i64(B), i64(nnz), vp(ptr), vp(user), vp(rating), i64(P.n_users), i32(P.n_items),
                                         vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64), vp(norm_in), i32(cap), i64(max_records),
                                         vp(row_ptr), vp(S.col), vp(S.sim), vp(S.ls), vp(S.nij), vp(avg), vp(norm)))
        S.col, S.sim, S.ls, S.nij = S.col[:n], S.sim[:n], S.ls[:n], S.nij[:n]
        S.ptr, S.user, S.cap, S.avg, S.norm = ptr, user, int(cap), avg[:B], norm[:B]
        S.counts = tuple(int(x) for x in h)
        return S, avg[:B], norm[:B]

    def item_foldin_tables(self, neighbors, item_avg, rows, keep=None):
        """The extended tables of I + B items for predict() / topn() / audience(batch=) / explain() (pass n_items = I + B there):
        rows [0, I) are copies of the resident neighbors = (cnt, col, sim, ls) and item_avg, row I + q is the list of batch item
        q -- rec_select's rule over its item_foldin rows, keep = the resident lists' width -- and rows.avg[q].  List entries are
        resident indices; a batch item is nobody's neighbour.  Returns ((cnt, col, sim, ls), avg) on the device."""
        st = _stream(self.dev)
        cnt, col, sim = [x.contiguous() for x in neighbors[:3]]
        I, B = int(cnt.numel()), int(rows.n_items)
        width = int(col.shape[1]) if col.dim() == 2 else 1
        keep = width if keep is None else int(keep)
        if keep != width:
            raise ValueError("item fold-in tables: keep = %d, the resident lists are %d wide" % (keep, width))
        ls = neighbors[3].contiguous() if len(neighbors) > 3 and neighbors[3] is not None else torch.zeros_like(sim)
        x_cnt = self._zeros(max(I + B, 1), torch.int32)
        x_col = self._zeros((max(I + B, 1), keep), torch.int32)
        x_sim = self._zeros((max(I + B, 1), keep), torch.float64)
        x_ls = self._zeros((max(I + B, 1), keep), torch.float64)
        x_avg = self._zeros(max(I + B, 1), torch.float64)
        x_cnt[:I], x_col[:I], x_sim[:I], x_ls[:I], x_avg[:I] = cnt, col.view(I, keep), sim.view(I, keep), ls.view(I, keep), item_avg[:I]
        x_avg[I:I + B] = rows.avg[:B]
        if rows.n_kept > 0:
            with self.timed("itemfold_select"):
                check(lib.xmap_rec_select(st, i32(B), vp(rows.row_ptr), vp(rows.col), vp(rows.sim), vp(rows.ls), i32(keep), vp(x_cnt[I:]),
                                          vp(x_col[I:]), vp(x_sim[I:]), vp(x_ls[I:])))
        return (x_cnt[:I + B], x_col[:I + B], x_sim[:I + B], x_ls[:I + B]), x_avg[:I + B]

    @staticmethod
    def union_profiles(parts, n_users, n_items, distinct=True, timers=None):
        """The union of the AlterEgo rows of several two-domain problems as ONE set of user-major profiles
        (xmap_union_count / xmap_union_fill): the reference's alterEgo_profile1.union(alterEgo_profile2) and, with distinct,
        .distinct() (code/multidomain_demo.py:128), without a host copy.  The union space belongs to no single engine's ratings,
        hence a static method.  parts = [(G, user_map, item_map, time_key or None)*], 1 .. 16 of them on one device: G the
        result of alterego(); user_map [users of G's engine] -> union user (injective within a part), item_map [items of G's
        engine] -> union item or -1 (rows of that item are dropped) -- int32 tensors or NumPy arrays; time_key as
        alterego_profiles takes it (ranks must compare ACROSS the parts).  A union user's rows: parts in the order given, within
        a part pass-through rows, then mapped rows, in stage-C order; distinct removes a row equal (item, time, rating as a number)
        to an earlier one of the same user.  The maps, offsets and row items are checked on the device first (XmapError, code
        ERR_ARG).  Returns the DeviceRatings-compatible view alterego_profiles returns, over the union item space with every
        item in the target class -- Engine(view).rec_sim / rec_select / predict / topn / topn_eval / mae work as for one domain --
        with .counts = (rows, duplicates removed, rows dropped by item_map == -1, union users with a row).  timers: a dict that
        collects the HIP-event brackets "union_count" / "union_fill", like Engine.timers."""
        parts = list(parts)
        if not 1 <= len(parts) <= abi.UNION_MAX_PARTS:
            raise ValueError("a union takes 1 .. %d parts, not %d" % (abi.UNION_MAX_PARTS, len(parts)))
        dev = parts[0][0].item.device
        U, I = int(n_users), int(n_items)

        def dmap(a):
            if not torch.is_tensor(a):
                a = torch.from_numpy(np.ascontiguousarray(a, np.int32))
            return a.to(device=dev, dtype=torch.int32).contiguous()
        keep = []                                   # the tensors behind the descriptors' pointers
        desc = (abi.UnionPart * len(parts))()
        for d, (G, user_map, item_map, time_key) in enumerate(parts):
            um, im = dmap(user_map), dmap(item_map)
            tm = G.time if time_key is None else time_key.contiguous()
            n = int(G.n_rows)
            if G.item.device != dev or int(G.off_t.numel()) != int(um.numel()) + 1 or int(G.off_m.numel()) != int(um.numel()) + 1 \
                    or int(tm.numel()) < n:
                raise ValueError("union part %d: one device, user_map of one entry per user of the part, a time per row" % d)
            keep += [um, im, tm]
            desc[d] = abi.UnionPart(int(um.numel()), int(im.numel()), n, int(G.n_target_rows), G.user.data_ptr(), G.item.data_ptr(),
                                    G.rating.data_ptr(), tm.data_ptr(), G.off_t.data_ptr(), G.off_m.data_ptr(), um.data_ptr(),
                                    im.data_ptr())
        eng = object.__new__(Engine)
        eng.dev, eng.timers, eng._scratch = dev, timers, {}
        flags = abi.UNION_DISTINCT if distinct else 0
        with torch.cuda.device(dev):
            st = _stream(dev)
            ptr = torch.empty(U + 1, dtype=torch.int64, device=dev)
            h = (C.c_int64 * 4)(0, 0, 0, 0)
            with eng.timed("union_count"):
                check(lib.xmap_union_count(st, i32(len(parts)), desc, i64(U), i32(I), i32(flags), vp(ptr), h))
            n = int(h[0])
            item = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            rating = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
            time = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
            with eng.timed("union_fill"):
                check(lib.xmap_union_fill(st, i32(len(parts)), desc, i64(U), i32(I), i32(flags), vp(ptr), i64(n), vp(item), vp(rating),
                                          vp(time)))
        del keep
        # the union's item space: every item a target item ("T:" in iid, flag bit 1); no other predicate is asked of the tail
        R = object.__new__(DeviceRatings)
        R.device, R.n_items = dev, I
        z = torch.zeros(max(I, 1), dtype=torch.int32, device=dev)
        R.prefix_cls, R.suffix_cls, R.contains_mask = z, z, z
        R.flags = torch.full((max(I, 1),), 2, dtype=torch.uint8, device=dev)
        eng.R = R
        P = eng._profile_view(U, n, ptr, item, rating, time)
        P.counts = tuple(int(x) for x in h)
        return P

    def predict(self, P, neighbors, test_user, test_item, item_avg, wtab, n_items=None):
        """RecommenderPrediction.item_based_prediction on the device (xmap_predict_rows, one wave per test pair) over the
        profiles P of alterego_profiles: neighbors = (cnt [I], col [I][keep], sim [I][keep], ...) as rec_select returns
        them (or made by the host), test_user / test_item int32 tensors, item_avg [I] fp64, wtab = exp(-alpha d) fp64.
        Returns (plain, decayed, status, max_now); a pair with status 2 and max_now > len(wtab) needs a longer table.
        n_items: the items of the tables when they are the extended ones of item_foldin_tables (default: P's item space)."""
        st = _stream(self.dev)
        cnt, col, sim = [x.contiguous() for x in neighbors[:3]]
        T = int(test_user.numel())
        keep = int(col.shape[1]) if col.dim() == 2 else 1
        plain = self._empty(max(T, 1), torch.float64)
        decay = self._empty(max(T, 1), torch.float64)
        status = self._empty(max(T, 1), torch.int32)
        h = C.c_int32(0)
        with self.timed("predict_rows"):
            check(lib.xmap_predict_rows(st, i64(T), vp(test_user.contiguous()), vp(test_item.contiguous()), i64(P.n_users),
                                        i32(P.n_items if n_items is None else n_items), i32(keep), vp(cnt), vp(col), vp(sim), vp(P.user_ptr), vp(P.user_item),
                                        vp(P.user_rating64), vp(P.user_time), vp(item_avg.contiguous()), vp(wtab), i32(wtab.numel()),
                                        vp(plain), vp(decay), vp(status), C.byref(h)))
        return plain[:T], decay[:T], status[:T], int(h.value)

    def _rec_filter(self, n, n_query, allow, exclude, min_score):
        """the xmap_rec_filter of topn() / audience() over an id space of n ids + the tensors it points into (kept by the caller
        for the call).  allow: a bool tensor [n] (packed here, on the device) or the packed words [(n + 31) // 32] (int32 /
        uint32, filters.pack_mask); exclude: (ptr int64 [Q + 1], ids int32), filters.exclusion_csr; all on the device."""
        words = ptr = ids = None
        if allow is not None:
            n_words = (int(n) + 31) // 32
            if allow.dtype == torch.bool:
                if tuple(allow.shape) != (int(n),):
                    raise ValueError("allow: a bool mask of %d ids, not %s" % (n, tuple(allow.shape)))
                bits = torch.zeros(n_words * 32, dtype=torch.int64, device=self.dev)
                bits[:int(n)] = allow.to(self.dev)
                w = (bits.view(n_words, 32) << torch.arange(32, dtype=torch.int64, device=self.dev)).sum(dim=1)
                words = (w - ((w >> 31) << 32)).to(torch.int32)
            else:
                words = allow.contiguous()
                if words.element_size() != 4 or words.dtype.is_floating_point or int(words.numel()) != n_words:
                    raise ValueError("allow: %d packed 32-bit words for %d ids, not %s %s" % (n_words, n, words.dtype, tuple(words.shape)))
            words = words if words.numel() else torch.zeros(1, dtype=torch.int32, device=self.dev)
        if exclude is not None:
            ptr, ids = exclude[0].contiguous(), exclude[1].contiguous()
            if ptr.dtype != torch.int64 or ids.dtype != torch.int32 or int(ptr.numel()) != int(n_query) + 1:
                raise ValueError("exclude = (ptr int64 [%d], ids int32): one list per query" % (int(n_query) + 1))
            ids = ids if ids.numel() else torch.zeros(1, dtype=torch.int32, device=self.dev)
        if min_score is not None and min_score != min_score:
            raise ValueError("min_score is NaN")
        return abi.rec_filter(words, ptr, ids, min_score), (words, ptr, ids)

    def topn(self, P, neighbors, query_user, item_avg, wtab, n_top, rank_by=0, keep_held=False, n_items=None, allow=None,
             exclude=None, min_score=None):
        """Top-N recommendation on the device (xmap_topn_rows) over the profiles P of alterego_profiles: per query user the
        n_top (1..64) best items its own rows give evidence for, by the unrounded prediction (rank_by 0: plain, 1: decayed;
        score descending, item index ascending); items the user holds are left out unless keep_held.  neighbors, item_avg,
        wtab as predict() takes them; query_user an int32 tensor (any order, repeats allowed; an index outside the users: no
        items).  Returns (cnt [Q], item [Q][n_top] (-1 behind the count), plain, decayed [Q][n_top], stats) with stats =
        (candidates scored, candidates dropped, largest `now`, largest candidate count of a query): candidates were dropped
        for a short table when stats[2] > len(wtab).  n_items: as predict() takes it (the extended tables of an item fold-in; a
        batch item is listed as I + q, also for its own raters: the frozen profiles do not hold it).
        Eligibility (xmap_topn_rows_filtered; the rules act before scoring, so the n_top best ELIGIBLE items are selected):
        allow = the items that may be returned (bool tensor [items] or packed words), exclude = (ptr, ids) of items never returned
        per QUERY, min_score = floor on the rank_by score.  With any of the three the stats are 6: the four above over the
        eligible candidates, candidates below the floor, candidate pairs the mask or the lists removed."""
        st = _stream(self.dev)
        cnt, col, sim = [x.contiguous() for x in neighbors[:3]]
        Q, n_top = int(query_user.numel()), int(n_top)
        keep = int(col.shape[1]) if col.dim() == 2 else 1
        if not 1 <= n_top <= 64:
            raise ValueError("n_top = %d: the device selection takes 1 .. 64" % n_top)
        out_cnt = self._empty(max(Q, 1), torch.int32)
        out_item = self._empty((max(Q, 1), n_top), torch.int32)
        out_plain = self._empty((max(Q, 1), n_top), torch.float64)
        out_decay = self._empty((max(Q, 1), n_top), torch.float64)
        if allow is not None or exclude is not None or min_score is not None:
            F, alive = self._rec_filter(P.n_items if n_items is None else n_items, Q, allow, exclude, min_score)
            h = (C.c_int64 * 6)()
            with self.timed("topn"):
                check(lib.xmap_topn_rows_filtered(st, i64(Q), vp(query_user.contiguous()), i32(n_top), i32(rank_by),
                                                  i32(abi.TOPN_KEEP_HELD if keep_held else 0), i64(P.n_users),
                                                  i32(P.n_items if n_items is None else n_items), i32(keep), vp(cnt), vp(col), vp(sim),
                                                  vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64), vp(P.user_time),
                                                  vp(item_avg.contiguous()), vp(wtab), i32(wtab.numel()), vp(out_cnt), vp(out_item),
                                                  vp(out_plain), vp(out_decay), C.byref(F), h))
            del alive
            return out_cnt[:Q], out_item[:Q], out_plain[:Q], out_decay[:Q], tuple(int(x) for x in h)
        h = (C.c_int64 * 4)(0, 0, 0, 0)
        with self.timed("topn"):
            check(lib.xmap_topn_rows(st, i64(Q), vp(query_user.contiguous()), i32(n_top), i32(rank_by), i32(abi.TOPN_KEEP_HELD if keep_held else 0),
                                     i64(P.n_users), i32(P.n_items if n_items is None else n_items), i32(keep), vp(cnt), vp(col), vp(sim),
                                     vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64), vp(P.user_time), vp(item_avg.contiguous()),
                                     vp(wtab), i32(wtab.numel()), vp(out_cnt), vp(out_item), vp(out_plain), vp(out_decay), h))
        return out_cnt[:Q], out_item[:Q], out_plain[:Q], out_decay[:Q], tuple(int(x) for x in h)

    def group_topn(self, P, neighbors, grp_ptr, grp_user, item_avg, wtab, n_top, how="mean", veto=None, rank_by=0, keep_held=False,
                   n_items=None, allow=None, exclude=None, min_score=None):
        """Group lists on the device (xmap_group_topn_rows): ONE list of n_top (1..64) items per group of users, by aggregating
        the members' unrounded predictions.  Groups are a CSR: grp_ptr int64 [G + 1] (grp_ptr[0] = 0, non-decreasing, at most 64
        members each), grp_user int32 -- indices into P's users in list order; a repeated member counts as often as listed, an
        index outside the users is a member without rows.  Candidates: the items at least one member's rows give evidence for;
        unless keep_held every item ANY member holds leaves.  A member without evidence for a candidate predicts the item
        average.  how = "mean" (left-to-right fp64 sum, one division), "min" (least misery) or "max" (most pleasure); veto: a
        candidate leaves if some member's rank_by score is below it (None: no veto).  allow / exclude / min_score as topn()
        takes them, with one exclusion list per GROUP and the floor on the aggregate score.  Returns (cnt [G], item [G][n_top]
        (-1 behind the count), plain, decayed [G][n_top], low [G][n_top] = the list position of the least-happy member (-1
        behind the count), stats) with stats = [member pairs scored, candidates dropped (status 2), largest `now`, largest
        candidate count of a group, below the floor, removed by the exclusion lists, vetoed, group candidates]: candidates were
        dropped for a short table when stats[2] > len(wtab).  The first four tensors have the layout of topn(): diversify() takes
        them as a pool."""
        st = _stream(self.dev)
        cnt, col, sim = [x.contiguous() for x in neighbors[:3]]
        grp_ptr, grp_user = grp_ptr.contiguous(), grp_user.contiguous()
        G, n_top = int(grp_ptr.numel()) - 1, int(n_top)
        keep = int(col.shape[1]) if col.dim() == 2 else 1
        if not 1 <= n_top <= 64:
            raise ValueError("n_top = %d: the device selection takes 1 .. 64" % n_top)
        if isinstance(how, str):
            if how not in abi.GROUP_HOW:
                raise ValueError("how = %r: one of %s" % (how, sorted(abi.GROUP_HOW)))
            how = abi.GROUP_HOW[how]
        if how not in (abi.GROUP_MEAN, abi.GROUP_MIN, abi.GROUP_MAX):
            raise ValueError("how = %r: XMAP_GROUP_MEAN / _MIN / _MAX" % (how,))
        veto = float("-inf") if veto is None else float(veto)
        if veto != veto:
            raise ValueError("veto is NaN")
        if G < 0 or grp_ptr.dtype != torch.int64 or grp_user.dtype != torch.int32:
            raise ValueError("groups = (grp_ptr int64 [G + 1], grp_user int32)")
        n_ids = P.n_items if n_items is None else n_items
        F, alive = self._rec_filter(n_ids, G, allow, exclude, min_score)
        grp_user = grp_user if grp_user.numel() else torch.zeros(1, dtype=torch.int32, device=self.dev)
        out_cnt = self._empty(max(G, 1), torch.int32)
        out_item, out_low = self._empty((max(G, 1), n_top), torch.int32), self._empty((max(G, 1), n_top), torch.int32)
        out_plain, out_decay = self._empty((max(G, 1), n_top), torch.float64), self._empty((max(G, 1), n_top), torch.float64)
        h = (C.c_int64 * 8)()
        with self.timed("group_topn"):
            check(lib.xmap_group_topn_rows(st, i64(G), vp(grp_ptr), vp(grp_user), i32(n_top), i32(rank_by),
                                           i32(abi.TOPN_KEEP_HELD if keep_held else 0), i32(how), C.c_double(veto), i64(P.n_users),
                                           i32(n_ids), i32(keep), vp(cnt), vp(col), vp(sim), vp(P.user_ptr), vp(P.user_item),
                                           vp(P.user_rating64), vp(P.user_time), vp(item_avg.contiguous()), vp(wtab), i32(wtab.numel()),
                                           vp(out_cnt), vp(out_item), vp(out_plain), vp(out_decay), vp(out_low), C.byref(F), h))
        del alive
        return out_cnt[:G], out_item[:G], out_plain[:G], out_decay[:G], out_low[:G], [int(x) for x in h]

    def div_index(self, S):
        """The diversity index of a rec_sim result (xmap_div_index): every row's columns ascending with |sim| beside them, what
        diversify() searches.  Returns a handle (n_items, row_ptr -- S's own --, dv_col, dv_abs, nnz) on the device; it belongs to
        the matrix, whatever neighbour lists are selected from it.  A row that holds a column twice raises XmapError."""
        I, nnz = int(S.row_ptr.numel()) - 1, int(S.col.numel())
        X = DivIndex()
        X.n_items, X.nnz, X.row_ptr = I, nnz, S.row_ptr.contiguous()
        X.dv_col, X.dv_abs = self._empty(max(nnz, 1), torch.int32), self._empty(max(nnz, 1), torch.float64)
        dups = C.c_int64(0)
        with self.timed("div_index"):
            check(lib.xmap_div_index(_stream(self.dev), i32(I), i64(nnz), vp(X.row_ptr), vp(S.col.contiguous()), vp(S.sim.contiguous()),
                                     vp(X.dv_col), vp(X.dv_abs), C.byref(dups)))
        return X

    def diversify(self, lists, index, weight, n_top, rank_by=0):
        """Greedy maximal-marginal-relevance re-ranking on the device (xmap_diversify_rows) of the pools `lists` = what topn()
        returned with n_top = the pool's width (1..64; the stats are ignored), over a div_index() handle: the next item is the one
        with the largest score - weight * (its largest |sim| to an item picked so far), the earlier pool position on equal
        values.  weight finite and >= 0; weight 0 returns the pool's prefix.  Returns (cnt [Q], item [Q][n_top] (-1 behind the
        count), plain, decayed [Q][n_top], pos [Q][n_top] = the pool position of each pick (-1 behind the count), pen [Q][n_top] =
        the penalty it was picked at, ils [Q] = the mean pairwise |sim| of the returned items (0.0 below two), stats = (lists that
        differ from the pool's prefix, items returned))."""
        in_cnt, in_item, in_plain, in_decay = [x.contiguous() for x in lists[:4]]
        Q, n_top = int(in_cnt.numel()), int(n_top)
        n_pool = int(in_item.shape[1]) if in_item.dim() == 2 else 1
        weight = float(weight)
        if not (0.0 <= weight < float("inf")):
            raise ValueError("weight = %r: finite and >= 0" % weight)
        if not 1 <= n_top <= n_pool <= 64:
            raise ValueError("n_top = %d of a pool of %d: 1 <= n_top <= pool <= 64" % (n_top, n_pool))
        cnt = self._empty(max(Q, 1), torch.int32)
        item, pos = self._empty((max(Q, 1), n_top), torch.int32), self._empty((max(Q, 1), n_top), torch.int32)
        plain, decay, pen = [self._empty((max(Q, 1), n_top), torch.float64) for _ in range(3)]
        ils = self._empty(max(Q, 1), torch.float64)
        h = (C.c_int64 * 2)(0, 0)
        with self.timed("diversify"):
            check(lib.xmap_diversify_rows(_stream(self.dev), i64(Q), i32(n_pool), vp(in_cnt), vp(in_item), vp(in_plain), vp(in_decay),
                                          i32(rank_by), C.c_double(weight), i32(n_top), i32(index.n_items), vp(index.row_ptr),
                                          vp(index.dv_col), vp(index.dv_abs), vp(cnt), vp(item), vp(plain), vp(decay), vp(pos), vp(pen),
                                          vp(ils), h))
        return cnt[:Q], item[:Q], plain[:Q], decay[:Q], pos[:Q], pen[:Q], ils[:Q], (int(h[0]), int(h[1]))

    def audience(self, P, neighbors, query_item, item_avg, wtab, n_top, rank_by=0, keep_holders=False, batch=None, allow=None,
                 exclude=None, min_score=None):
        """The audience of an item on the device (xmap_audience_rows) over the profiles P of alterego_profiles: per query
        item the n_top (1..1024) best users among those whose own rows give evidence for it, by the unrounded prediction
        (rank_by 0: plain, 1: decayed; score descending, user index ascending); users who hold the item are left out unless
        keep_holders.  topn() seen from the item: the same pairs, the same score bits.  neighbors, item_avg, wtab as predict()
        takes them; query_item an int32 tensor (any order, repeats allowed; an index outside the items or an item without a
        list: no users).  Returns (cnt [Q], user [Q][n_top] (-1 behind the count), plain, decayed [Q][n_top], stats) with stats
        as topn() returns them.  batch = (ptr, user) of an item fold-in (item_foldin's rows.ptr / rows.user, device tensors):
        neighbors and item_avg are then the extended tables of item_foldin_tables, query items I + q are the batch's, and their
        raters are their holders (xmap_itemfold_audience_rows).
        Eligibility (xmap_audience_rows_filtered), as topn() takes it with users for items: allow = the users who may be returned,
        exclude = (ptr, ids) of users never returned per QUERY, min_score = floor on the rank_by score; then 6 stats."""
        st = _stream(self.dev)
        cnt, col, sim = [x.contiguous() for x in neighbors[:3]]
        Q, n_top = int(query_item.numel()), int(n_top)
        keep = int(col.shape[1]) if col.dim() == 2 else 1
        if not 1 <= n_top <= 1024:
            raise ValueError("n_top = %d: the device selection takes 1 .. 1024" % n_top)
        out_cnt = self._empty(max(Q, 1), torch.int32)
        out_user = self._empty((max(Q, 1), n_top), torch.int32)
        out_plain = self._empty((max(Q, 1), n_top), torch.float64)
        out_decay = self._empty((max(Q, 1), n_top), torch.float64)
        h = (C.c_int64 * 4)(0, 0, 0, 0)
        b_ptr = b_user = None
        n_all = n_res = int(P.n_items)
        if batch is not None:
            b_ptr, b_user = batch[0].contiguous(), batch[1].contiguous()
            n_all = int(cnt.numel())
            n_res = n_all - (int(b_ptr.numel()) - 1)
            if n_res < 0 or b_ptr.dtype != torch.int64 or b_user.dtype != torch.int32:
                raise ValueError("audience: batch = (ptr int64 [B + 1], user int32) of at most as many items as the tables hold")
        if allow is not None or exclude is not None or min_score is not None:
            F, alive = self._rec_filter(P.n_users, Q, allow, exclude, min_score)
            h = (C.c_int64 * 6)()
            with self.timed("audience"):
                check(lib.xmap_audience_rows_filtered(st, i64(Q), vp(query_item.contiguous()), i32(n_top), i32(rank_by),
                                                      i32(abi.AUDIENCE_KEEP_HOLDERS if keep_holders else 0), i64(P.n_users), i32(n_all),
                                                      i32(keep), vp(cnt), vp(col), vp(sim), vp(P.user_ptr), vp(P.user_item),
                                                      vp(P.user_rating64), vp(P.user_time), vp(item_avg.contiguous()), vp(wtab),
                                                      i32(wtab.numel()), vp(out_cnt), vp(out_user), vp(out_plain), vp(out_decay),
                                                      i32(n_res), vp(b_ptr), vp(b_user), C.byref(F), h))
            del alive
            return out_cnt[:Q], out_user[:Q], out_plain[:Q], out_decay[:Q], tuple(int(x) for x in h)
        if batch is not None:
            with self.timed("audience"):
                check(lib.xmap_itemfold_audience_rows(st, i64(Q), vp(query_item.contiguous()), i32(n_top), i32(rank_by),
                                                      i32(abi.AUDIENCE_KEEP_HOLDERS if keep_holders else 0), i64(P.n_users), i32(n_all),
                                                      i32(keep), vp(cnt), vp(col), vp(sim), vp(P.user_ptr), vp(P.user_item),
                                                      vp(P.user_rating64), vp(P.user_time), vp(item_avg.contiguous()), vp(wtab),
                                                      i32(wtab.numel()), vp(out_cnt), vp(out_user), vp(out_plain), vp(out_decay), h,
                                                      i32(n_res), vp(b_ptr), vp(b_user)))
            return out_cnt[:Q], out_user[:Q], out_plain[:Q], out_decay[:Q], tuple(int(x) for x in h)
        with self.timed("audience"):
            check(lib.xmap_audience_rows(st, i64(Q), vp(query_item.contiguous()), i32(n_top), i32(rank_by),
                                         i32(abi.AUDIENCE_KEEP_HOLDERS if keep_holders else 0), i64(P.n_users), i32(P.n_items), i32(keep),
                                         vp(cnt), vp(col), vp(sim), vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64), vp(P.user_time),
                                         vp(item_avg.contiguous()), vp(wtab), i32(wtab.numel()), vp(out_cnt), vp(out_user), vp(out_plain),
                                         vp(out_decay), h))
        return out_cnt[:Q], out_user[:Q], out_plain[:Q], out_decay[:Q], tuple(int(x) for x in h)

    def peer_index(self, P, centre=None):
        """The peer index of the profiles P (xmap_peer_index): the item-major transposition of P's valid rows in holder order
        (ascending row index) with x = rating - centre[item] beside the user (centre None: the rating itself), and nrm [users].
        Returns a handle (n_users, n_items, centre, hd_ptr, hd_user, hd_x, nrm, n_rows = rows indexed) on the device; it belongs
        to the profiles and the centring, whatever is asked of it."""
        X = PeerIndex()
        X.n_users, X.n_items = int(P.n_users), int(P.n_items)
        X.centre = None if centre is None else centre.contiguous()
        n = int(P.user_item.numel())
        X.hd_ptr = self._empty(X.n_items + 1, torch.int64)
        X.hd_user, X.hd_x = self._empty(max(n, 1), torch.int32), self._empty(max(n, 1), torch.float64)
        X.nrm = self._empty(max(X.n_users, 1), torch.float64)
        rows = C.c_int64(0)
        with self.timed("peer_index"):
            check(lib.xmap_peer_index(_stream(self.dev), i64(X.n_users), i32(X.n_items), vp(P.user_ptr), vp(P.user_item),
                                      vp(P.user_rating64), vp(X.centre), vp(X.hd_ptr), vp(X.hd_user), vp(X.hd_x), vp(X.nrm),
                                      C.byref(rows)))
        X.n_rows = int(rows.value)
        return X

    def peer_centre(self, index):
        """The item averages of the profiles behind an UNCENTRED peer_index() handle (xmap_peer_centre): per item the exact sum of
        its holders' ratings rounded once, divided by the entries -- the averages RecommenderSim computes, without its pair pass.
        Returns a float64 tensor [items]: pass it to peer_index(P, centre) for the centred index."""
        if index.centre is not None:
            raise ValueError("peer_centre: the averages are taken over an index built without a centre")
        avg = self._empty(max(index.n_items, 1), torch.float64)
        with self.timed("peer_centre"):
            check(lib.xmap_peer_centre(_stream(self.dev), i32(index.n_items), vp(index.hd_ptr), vp(index.hd_x), vp(avg)))
        return avg[:index.n_items]

    def pop_index(self, index, how="count", damping=0.0, min_count=1):
        """The popularity ranking of the items (xmap_pop_index) over an UNCENTRED peer_index() handle: how "count" ranks by the
        holders of an item, "mean" by (sum of its ratings + damping * the mean of all ratings) / (holders + damping); an item with
        fewer than min_count holders or a non-finite score is not ranked.  Score descending, item index ascending on equal scores.
        Returns a handle (n_items, item [I] (-1 behind the ranking), score [I], pos [I] (-1: not ranked), n_ranked, counts =
        (ranked, below min_count, non-finite), how, damping, min_count) on the device."""
        if index.centre is not None:
            raise ValueError("pop_index: the ranking is taken over an index built without a centre")
        if how not in abi.POP_HOW:
            raise ValueError("how = %r: one of %s" % (how, sorted(abi.POP_HOW)))
        damping, min_count = float(damping), int(min_count)
        if not (0.0 <= damping < float("inf")):
            raise ValueError("damping = %r: finite and >= 0" % damping)
        if min_count < 1:
            raise ValueError("min_count = %d: at least 1" % min_count)
        X = PopIndex()
        X.n_items, X.how, X.damping, X.min_count = int(index.n_items), how, damping, min_count
        X.item, X.pos = self._empty(max(X.n_items, 1), torch.int32), self._empty(max(X.n_items, 1), torch.int32)
        X.score = self._empty(max(X.n_items, 1), torch.float64)
        h = (C.c_int64 * 3)(0, 0, 0)
        with self.timed("pop_index"):
            check(lib.xmap_pop_index(_stream(self.dev), i32(X.n_items), vp(index.hd_ptr), vp(index.hd_x), i32(abi.POP_HOW[how]),
                                     C.c_double(damping), i32(min_count), vp(X.item), vp(X.score), vp(X.pos), h))
        X.counts = tuple(int(x) for x in h)
        X.n_ranked = X.counts[0]
        return X

    def fill(self, lists, pop, P, query_user, item_avg, keep_held=False, allow=None, exclude=None, n_items=None):
        """Completes short lists with the head of a popularity ranking (xmap_topn_fill_rows).  `lists` = what topn() / diversify()
        returned (cnt, item, plain, decayed, ...), for the queries query_user over the profiles P; pop a
        pop_index() handle.  A fill is the next ranked item the list does not contain, the user does not hold (unless keep_held),
        the query's exclusion list does not name and the mask allows; its plain and decayed value is item_avg[item], the
        prediction of a pair without evidence.  n_items: the size of the id space of item_avg and the mask when it exceeds the
        ranking's (the extended tables of an item fold-in: batch items are never filled).  The inputs are left as they are.
        Returns (cnt, item, plain, decayed, src [Q][n_top] (0: the model's, 1: a fill, -1 behind the count), stats = (queries
        short on entry, of those filled to n_top, fill entries written, queries still short))."""
        cnt, item, plain, decay = [x.clone().contiguous() for x in lists[:4]]
        Q = int(cnt.numel())
        n_top = int(item.shape[1]) if item.dim() == 2 else 1
        if not 1 <= n_top <= 64:
            raise ValueError("n_top = %d: the fill takes lists of 1 .. 64" % n_top)
        if int(query_user.numel()) != Q:
            raise ValueError("fill: %d lists for %d queries" % (Q, int(query_user.numel())))
        n_items = int(pop.n_items if n_items is None else n_items)
        src = self._empty((max(Q, 1), n_top), torch.int32)
        F = alive = None
        if allow is not None or exclude is not None:
            F, alive = self._rec_filter(n_items, Q, allow, exclude, None)
        h = (C.c_int64 * 4)(0, 0, 0, 0)
        with self.timed("fill"):
            check(lib.xmap_topn_fill_rows(_stream(self.dev), i64(Q), vp(query_user.contiguous()), i32(n_top),
                                          i32(abi.TOPN_KEEP_HELD if keep_held else 0), i64(P.n_users), i32(n_items), vp(P.user_ptr),
                                          vp(P.user_item), vp(item_avg.contiguous()), i32(pop.n_ranked), vp(pop.item), vp(pop.pos),
                                          i32(pop.n_items), vp(cnt), vp(item), vp(plain), vp(decay), vp(src),
                                          None if F is None else C.byref(F), h))
        del alive
        return cnt, item, plain, decay, src[:Q], tuple(int(x) for x in h)

    def set_labels(self, n_items, n_labels, lab_ptr, lab_id, names=None):
        """The label table of an item space of n_items items on the device, for shelves(): lab_ptr int64 [n_items + 1], lab_id
        int32 (NumPy arrays or tensors; labels.label_csr makes them), ids in [0, n_labels), the labels of one item strictly
        ascending -- the device call checks the table.  names: the labels' names in id order (kept on the handle for the caller).
        Returns a LabelTable handle."""
        n_items, n_labels = int(n_items), int(n_labels)
        if not 1 <= n_labels <= abi.SHELF_MAX_LABELS:
            raise ValueError("set_labels: n_labels = %d, not in 1 .. 2^24" % n_labels)
        T = LabelTable()
        T.n_items, T.n_labels, T.names = n_items, n_labels, None if names is None else list(names)
        T.ptr = torch.as_tensor(np.asarray(lab_ptr) if not torch.is_tensor(lab_ptr) else lab_ptr, dtype=torch.int64).to(self.dev).contiguous()
        ids = torch.as_tensor(np.asarray(lab_id) if not torch.is_tensor(lab_id) else lab_id, dtype=torch.int32).to(self.dev).contiguous()
        if int(T.ptr.numel()) != n_items + 1:
            raise ValueError("set_labels: lab_ptr has %d entries for %d items" % (int(T.ptr.numel()), n_items))
        T.id = ids if ids.numel() else torch.zeros(1, dtype=torch.int32, device=self.dev)
        return T

    def _lab_allow(self, labels, lab_allow):
        """the lab_allow words of a shelf call on the device: None, a bool tensor / array [n_labels], or the packed words of
        labels.label_mask"""
        if lab_allow is None:
            return None
        n_words = (labels.n_labels + 31) // 32
        a = lab_allow if torch.is_tensor(lab_allow) else torch.from_numpy(np.ascontiguousarray(
            np.asarray(lab_allow).view(np.int32) if np.asarray(lab_allow).dtype == np.uint32 else np.asarray(lab_allow)))
        if a.dtype == torch.bool:
            from .filters import pack_mask
            a = torch.from_numpy(pack_mask(a.cpu().numpy(), labels.n_labels).view(np.int32))
        if a.element_size() != 4 or a.dtype.is_floating_point or int(a.numel()) != n_words:
            raise ValueError("lab_allow: %d packed 32-bit words for %d labels, not %s %s" % (n_words, labels.n_labels, a.dtype, tuple(a.shape)))
        return a.to(self.dev).contiguous()

    def _shelf_outs(self, Q, n_shelf, n_top):
        Q1 = max(Q, 1)
        return [self._empty(Q1, torch.int32), self._empty((Q1, n_shelf), torch.int32), self._empty((Q1, n_shelf), torch.float64),
                self._empty((Q1, n_shelf), torch.int32), self._empty((Q1, n_shelf), torch.int32), self._empty((Q1, n_shelf, n_top), torch.int32),
                self._empty((Q1, n_shelf, n_top), torch.float64), self._empty((Q1, n_shelf, n_top), torch.float64)]

    @staticmethod
    def _shelf_args(n_shelf, n_top, shelf_by, min_fill):
        n_shelf, n_top, min_fill = int(n_shelf), int(n_top), int(min_fill)
        if not 1 <= n_shelf <= 64:
            raise ValueError("n_shelf = %d: a page takes 1 .. 64 shelves" % n_shelf)
        if not 1 <= n_top <= 64:
            raise ValueError("n_top = %d: a shelf takes 1 .. 64 entries" % n_top)
        if min_fill < 1:
            raise ValueError("min_fill = %d, not >= 1" % min_fill)
        by = abi.SHELF_BY.get(shelf_by, -1) if isinstance(shelf_by, str) else int(shelf_by)
        if by not in abi.SHELF_BY.values():
            raise ValueError("shelf_by = %r: one of %s" % (shelf_by, sorted(abi.SHELF_BY)))
        return n_shelf, n_top, by, min_fill

    def shelves(self, P, neighbors, query_user, item_avg, wtab, labels, n_shelf, n_top, shelf_by="best", min_fill=1, rank_by=0,
                keep_held=False, lab_allow=None, allow=None, exclude=None, min_score=None, n_items=None, max_records=0):
        """A page of shelves per query user (xmap_shelf_rows): a top-n_top per label of the items over the kept candidates of
        topn() under the same eligibility rules (allow, exclude, min_score as topn() takes them), and the n_shelf best shelves of
        the page by shelf_by: "best" (the score of a shelf's first entry), "mean" (the mean of its returned entries) or "label" (a
        fixed layout, label ascending).  labels: a set_labels() handle over the item space of the tables (n_items: as predict()
        takes it); lab_allow: the labels that may form a shelf (bool [n_labels] or labels.label_mask words; None: all); a shelf of
        fewer than min_fill members is not formed.  Returns (nshelf [Q], label [Q][n_shelf] (-1 behind the count), sscore, size
        (the whole shelf's members), cnt [Q][n_shelf], item (-1 behind a shelf's count), plain, decayed [Q][n_shelf][n_top], stats
        [10]: the six of the filtered topn(), then records, shelves with a member, of those the shelves below min_fill, the most
        formed shelves of one query).  item / plain / decayed viewed as [Q * n_shelf][n_top] with cnt as [Q * n_shelf] are lists
        for diversify() and fuse()."""
        st = _stream(self.dev)
        cnt, col, sim = [x.contiguous() for x in neighbors[:3]]
        Q = int(query_user.numel())
        keep = int(col.shape[1]) if col.dim() == 2 else 1
        n_shelf, n_top, by, min_fill = self._shelf_args(n_shelf, n_top, shelf_by, min_fill)
        I = int(P.n_items if n_items is None else n_items)
        if labels.n_items != I:
            raise ValueError("shelves: the label table covers %d items, the tables %d" % (labels.n_items, I))
        outs = self._shelf_outs(Q, n_shelf, n_top)
        words = self._lab_allow(labels, lab_allow)
        F = alive = None
        if allow is not None or exclude is not None or min_score is not None:
            F, alive = self._rec_filter(I, Q, allow, exclude, min_score)
        h = (C.c_int64 * 10)()
        with self.timed("shelves"):
            check(lib.xmap_shelf_rows(st, i64(Q), vp(query_user.contiguous()), i32(n_top), i32(rank_by),
                                      i32(abi.TOPN_KEEP_HELD if keep_held else 0), i64(P.n_users), i32(I), i32(keep), vp(cnt), vp(col), vp(sim),
                                      vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64), vp(P.user_time), vp(item_avg.contiguous()),
                                      vp(wtab), i32(wtab.numel()), i32(labels.n_labels), vp(labels.ptr), vp(labels.id), vp(words),
                                      i32(n_shelf), i32(by), i32(min_fill), i64(max_records), *([vp(t) for t in outs] +
                                                                                                 [None if F is None else C.byref(F), h])))
        del alive
        return tuple(t[:Q] for t in outs) + (tuple(int(x) for x in h),)

    def shelf_segments(self, scored, labels, n_shelf, n_top, shelf_by="best", min_fill=1, rank_by=0, lab_allow=None, min_score=None,
                       max_records=0):
        """The back half of shelves() over scored segments (xmap_shelf_segments): scored = (cand_ptr int64 [Q + 1], cand_item int32
        (ascending within a segment, each once), plain, decayed fp64, status int32) on the device; a candidate is kept iff its status
        is 0 and its rank_by score is >= min_score.  The other arguments and the first eight returns as shelves(); stats [4] =
        (records, shelves with a member, of those the shelves below min_fill, the most formed shelves of one query)."""
        st = _stream(self.dev)
        ptr, item, plain, decay, status = [x.contiguous() for x in scored[:5]]
        Q = int(ptr.numel()) - 1
        n_shelf, n_top, by, min_fill = self._shelf_args(n_shelf, n_top, shelf_by, min_fill)
        if min_score is not None and min_score != min_score:
            raise ValueError("min_score is NaN")
        outs = self._shelf_outs(Q, n_shelf, n_top)
        words = self._lab_allow(labels, lab_allow)
        h = (C.c_int64 * 4)()
        with self.timed("shelf_segments"):
            check(lib.xmap_shelf_segments(st, i64(Q), vp(ptr), vp(item), vp(plain), vp(decay), vp(status),
                                          C.c_double(float("-inf") if min_score is None else float(min_score)), i32(labels.n_items),
                                          i32(labels.n_labels), vp(labels.ptr), vp(labels.id), vp(words), i32(n_shelf), i32(n_top), i32(rank_by),
                                          i32(by), i32(min_fill), i64(max_records), *([vp(t) for t in outs] + [h])))
        return tuple(t[:Q] for t in outs) + (tuple(int(x) for x in h),)

    def _quota_args(self, labels, n_pool, n_top, mode, cap, lab_cap, lab_weight):
        """the checked scalars of a quota call and its per-label arrays on the device (None, a tensor or an array [n_labels])"""
        n_pool, n_top = int(n_pool), int(n_top)
        if not 1 <= n_pool <= abi.QUOTA_MAX_POOL:
            raise ValueError("n_pool = %d: a pool takes 1 .. %d positions" % (n_pool, abi.QUOTA_MAX_POOL))
        if not 1 <= n_top <= n_pool:
            raise ValueError("n_top = %d, not in 1 .. n_pool = %d" % (n_top, n_pool))
        m = abi.QUOTA_MODE.get(mode, -1) if isinstance(mode, str) else int(mode)
        if m not in abi.QUOTA_MODE.values():
            raise ValueError("mode = %r: one of %s" % (mode, sorted(abi.QUOTA_MODE)))
        if m == abi.QUOTA_CAP and lab_cap is None and int(cap) < 1:
            raise ValueError("cap = %d, not >= 1 (without lab_cap)" % int(cap))

        def per_label(x, name, np_dtype):
            if x is None:
                return None
            t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np_dtype)).view(np.int32))
            if int(t.numel()) != labels.n_labels or t.element_size() != 4 or t.dtype.is_floating_point:
                raise ValueError("%s: one 32-bit integer per label (%d), not %s %s" % (name, labels.n_labels, t.dtype, tuple(t.shape)))
            return t.to(self.dev).contiguous()
        return n_pool, n_top, m, int(cap), per_label(lab_cap, "lab_cap", np.int32), per_label(lab_weight, "lab_weight", np.uint32)

    def _quota_outs(self, Q, n_top):
        Q1 = max(Q, 1)
        return [self._empty(Q1, torch.int32), self._empty((Q1, n_top), torch.int32), self._empty((Q1, n_top), torch.float64),
                self._empty((Q1, n_top), torch.float64), self._empty((Q1, n_top), torch.int32), self._empty((Q1, n_top), torch.int32)]

    def quota_pool(self, lists, labels, n_top, mode="cap", cap=1, lab_cap=None, lab_weight=None, lab_allow=None, P=None, query_user=None,
                   n_items=None, rank_by=0):
        """ONE list per query with a guaranteed mix of labels (xmap_quota_pool), cut from the pools `lists` = (cnt [Q], item, plain,
        decayed [Q][n_pool], ...): what topn(), uknn_topn(), group_topn(), related(), fill() or quota_topn() returned, n_pool up to
        1 024; position is rank.  labels: a set_labels() handle; lab_allow: the labels the quota governs (as shelves() takes it;
        None: all).  mode "cap": at most cap entries of a label (lab_cap: one int32 cap per label instead; 0 bars a label), greedy
        in pool order.  mode "share": the seats go to the labels by Sainte-Lague quotients of lab_weight (uint32 per label), or,
        without it, of the history of query_user in the profiles P (rows per label).  Returns (cnt [Q], item (-1 behind the count),
        plain, decayed, pos = the pool position of each entry, label = the claiming label ("share"; -1: a fill) or the item's
        smallest governed label ("cap") [Q][n_top], stats = (lists that differ from the pool's prefix, entries, positions refused
        / slots filled off-profile, "cap": lists cut short by a full pool -- widen it))."""
        st = _stream(self.dev)
        cnt, item, plain, decay = [x.contiguous() for x in lists[:4]]
        Q = int(cnt.numel())
        n_pool = int(item.shape[1]) if item.dim() == 2 else int(item.numel()) // max(Q, 1)
        n_pool, n_top, m, cap, caps, weights = self._quota_args(labels, n_pool, n_top, mode, cap, lab_cap, lab_weight)
        I = int(labels.n_items if n_items is None else n_items)
        if labels.n_items != I:
            raise ValueError("quota_pool: the label table covers %d items, the pools' id space %d" % (labels.n_items, I))
        history = m == abi.QUOTA_SHARE and weights is None
        if history and (P is None or query_user is None):
            raise ValueError("quota_pool: mode \"share\" without lab_weight reads the history: P and query_user")
        outs = self._quota_outs(Q, n_top)
        words = self._lab_allow(labels, lab_allow)
        h = (C.c_int64 * 4)()
        with self.timed("quota_pool"):
            check(lib.xmap_quota_pool(st, i64(Q), i32(n_pool), vp(cnt), vp(item), vp(plain), vp(decay), i32(rank_by), i32(m), i32(cap), vp(caps),
                                      vp(weights), vp(query_user.contiguous() if history else None), i64(P.n_users if history else 0),
                                      vp(P.user_ptr if history else None), vp(P.user_item if history else None), i32(I),
                                      i32(labels.n_labels), vp(labels.ptr), vp(labels.id), vp(words), i32(n_top), *([vp(t) for t in outs] + [h])))
        return tuple(t[:Q] for t in outs) + (tuple(int(x) for x in h),)

    def quota_topn(self, P, neighbors, query_user, item_avg, wtab, labels, n_pool, n_top, mode="cap", cap=1, lab_cap=None, lab_weight=None,
                   lab_allow=None, rank_by=0, keep_held=False, allow=None, exclude=None, min_score=None, n_items=None):
        """The whole quota call (xmap_quota_rows): the candidates of topn() under the same eligibility rules (allow, exclude,
        min_score), ranked into a pool of n_pool (up to 1 024) that never leaves the device, and quota_pool() over it -- the history
        of mode "share" is the profiles P.  Returns (cnt, item, plain, decayed, pos, label, stats [10]: the six of the filtered
        topn(), then the four of quota_pool())."""
        st = _stream(self.dev)
        cnt, col, sim = [x.contiguous() for x in neighbors[:3]]
        Q = int(query_user.numel())
        keep = int(col.shape[1]) if col.dim() == 2 else 1
        n_pool, n_top, m, cap, caps, weights = self._quota_args(labels, n_pool, n_top, mode, cap, lab_cap, lab_weight)
        I = int(P.n_items if n_items is None else n_items)
        if labels.n_items != I:
            raise ValueError("quota_topn: the label table covers %d items, the tables %d" % (labels.n_items, I))
        outs = self._quota_outs(Q, n_top)
        words = self._lab_allow(labels, lab_allow)
        F = alive = None
        if allow is not None or exclude is not None or min_score is not None:
            F, alive = self._rec_filter(I, Q, allow, exclude, min_score)
        h = (C.c_int64 * 10)()
        with self.timed("quota_topn"):
            check(lib.xmap_quota_rows(st, i64(Q), vp(query_user.contiguous()), i32(n_top), i32(rank_by),
                                      i32(abi.TOPN_KEEP_HELD if keep_held else 0), i64(P.n_users), i32(I), i32(keep), vp(cnt), vp(col), vp(sim),
                                      vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64), vp(P.user_time), vp(item_avg.contiguous()),
                                      vp(wtab), i32(wtab.numel()), i32(n_pool), i32(m), i32(cap), vp(caps), vp(weights), i32(labels.n_labels),
                                      vp(labels.ptr), vp(labels.id), vp(words), *([vp(t) for t in outs] + [None if F is None else C.byref(F), h])))
        del alive
        return tuple(t[:Q] for t in outs) + (tuple(int(x) for x in h),)

    def _allot_args(self, n_pool, max_pool, n_top, cap, item_cap, n_items, rank_by):
        """the checked scalars of an allot call and its capacities on the device (None, a tensor or an array [n_items])"""
        n_pool, n_top, cap = int(n_pool), int(n_top), int(cap)
        if not 1 <= n_pool <= max_pool:
            raise ValueError("n_pool = %d: a pool takes 1 .. %d positions" % (n_pool, max_pool))
        if not 1 <= n_top <= n_pool:
            raise ValueError("n_top = %d, not in 1 .. n_pool = %d" % (n_top, n_pool))
        if rank_by not in (0, 1):
            raise ValueError("rank_by = %r, not 0 or 1" % (rank_by,))
        if item_cap is None:
            if cap < 1:
                raise ValueError("cap = %d, not >= 1 (without item_cap)" % cap)
            return n_pool, n_top, cap, None
        t = item_cap if torch.is_tensor(item_cap) else torch.from_numpy(np.ascontiguousarray(np.asarray(item_cap).astype(np.int32)))
        if int(t.numel()) != n_items or t.dtype != torch.int32:
            raise ValueError("item_cap: one int32 per item (%d), not %s %s" % (n_items, t.dtype, tuple(t.shape)))
        return n_pool, n_top, cap, t.to(self.dev).contiguous()

    def _allot_outs(self, Q, n_top, n_items):
        Q1 = max(Q, 1)
        return [self._empty(Q1, torch.int32), self._empty((Q1, n_top), torch.int32), self._empty((Q1, n_top), torch.float64),
                self._empty((Q1, n_top), torch.float64), self._empty((Q1, n_top), torch.int32), self._empty(max(n_items, 1), torch.int32)]

    def allot_pool(self, lists, n_top, cap=1, item_cap=None, rank_by=0, n_items=None):
        """Top-N for many queries under item capacities (xmap_allot_pool): item i goes to at most cap(i) of the queries, every
        query gets at most n_top items -- recipient-proposing deferred acceptance over the pools `lists` = (cnt [Q], item, plain,
        decayed [Q][n_pool], ...): what topn(), uknn_topn(), group_topn(), related(), fill(), fuse-like lists returned, n_pool up
        to 1 024; position is rank.  cap: one capacity for every item, or item_cap: an int32 per item (0 bars an item, 2^31 - 1 is
        no cap).  An item keeps its best offers by the rank_by score (ties: the smaller query index, then the smaller position).
        n_items: the size of the pools' id space (default: item_cap's length, else the largest id + 1).  Returns an AllotLists: the
        tuple (cnt [Q], item (-1 behind the count), plain, decayed [Q][n_top]) that fill(), fuse() and quota_pool() take, with
        .positions (the pool position of each entry), .taken (offers held per item [n_items]: a caller serving users in batches
        passes cap - taken on -- the batches are not one market) and .stats = (lists that differ from the pool's prefix,
        entries, positions refused, void positions, rounds, lists cut short by a full pool -- widen it)."""
        st = _stream(self.dev)
        cnt, item, plain, decay = [x.contiguous() for x in lists[:4]]
        Q = int(cnt.numel())
        n_pool = int(item.shape[1]) if item.dim() == 2 else int(item.numel()) // max(Q, 1)
        if n_items is None:
            n_items = len(item_cap) if item_cap is not None else (int(item.max()) + 1 if item.numel() else 0)
        I = max(int(n_items), 0)
        n_pool, n_top, cap, caps = self._allot_args(n_pool, abi.ALLOT_MAX_POOL, n_top, cap, item_cap, I, rank_by)
        outs = self._allot_outs(Q, n_top, I)
        h = (C.c_int64 * 6)()
        with self.timed("allot_pool"):
            check(lib.xmap_allot_pool(st, i64(Q), i32(n_pool), vp(cnt), vp(item), vp(plain), vp(decay), i32(rank_by), i32(I), i32(cap),
                                      vp(caps), i32(n_top), *([vp(t) for t in outs] + [h])))
        return AllotLists([t[:Q] for t in outs[:4]], outs[4][:Q], outs[5][:I], tuple(int(x) for x in h))

    def allot_topn(self, P, neighbors, query_user, item_avg, wtab, n_pool, n_top, cap=1, item_cap=None, rank_by=0, keep_held=False,
                   allow=None, exclude=None, min_score=None, n_items=None):
        """The whole allot call (xmap_allot_rows): the pool of every query is what topn() returns with n_top = n_pool (1 .. 64)
        under the same eligibility rules (allow, exclude, min_score), never leaving the device, and allot_pool() over the pools.
        Returns the AllotLists of allot_pool() with .stats [12]: the six of the filtered topn(), then the six of allot_pool()."""
        st = _stream(self.dev)
        cnt, col, sim = [x.contiguous() for x in neighbors[:3]]
        Q = int(query_user.numel())
        keep = int(col.shape[1]) if col.dim() == 2 else 1
        I = int(P.n_items if n_items is None else n_items)
        n_pool, n_top, cap, caps = self._allot_args(n_pool, 64, n_top, cap, item_cap, I, rank_by)
        outs = self._allot_outs(Q, n_top, I)
        F = alive = None
        if allow is not None or exclude is not None or min_score is not None:
            F, alive = self._rec_filter(I, Q, allow, exclude, min_score)
        h = (C.c_int64 * 12)()
        with self.timed("allot_topn"):
            check(lib.xmap_allot_rows(st, i64(Q), vp(query_user.contiguous()), i32(n_pool), i32(rank_by),
                                      i32(abi.TOPN_KEEP_HELD if keep_held else 0), i64(P.n_users), i32(I), i32(keep), vp(cnt), vp(col), vp(sim),
                                      vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64), vp(P.user_time), vp(item_avg.contiguous()),
                                      vp(wtab), i32(wtab.numel()), i32(n_top), i32(cap), vp(caps),
                                      *([vp(t) for t in outs] + [None if F is None else C.byref(F), h])))
        del alive
        return AllotLists([t[:Q] for t in outs[:4]], outs[4][:Q], outs[5][:I], tuple(int(x) for x in h))

    def peers(self, index, Q, query_user, n_top, cap=1, min_common=1, same=False, keep_self=False, allow=None, exclude=None,
              min_sim=None, max_records=0):
        """Similar users on the device (xmap_peer_rows): per query user -- an index into the profiles Q, the resident ones (same
        = True: the user itself leaves unless keep_self) or a fold-in batch -- the n_top (1..1024) users of the peer_index() handle
        with the largest sim = cosine of the centred profiles * min(common, cap) / cap; sim descending, user index ascending.
        allow = the users who may be returned (bool tensor [users] or packed words; it acts in the expansion), exclude = (ptr, ids)
        of users never returned per QUERY, min_sim = floor.  Returns (cnt [Q], user [Q][n_top] (-1 behind the count), sim
        [Q][n_top], common [Q][n_top], stats) with stats = (candidates, dropped by min_common, dropped as non-finite, dropped below
        the floor, largest candidate count of a query, records expanded).  max_records: the chunk bound (0: the library's)."""
        st = _stream(self.dev)
        n_q, n_top = int(query_user.numel()), int(n_top)
        if not 1 <= n_top <= 1024:
            raise ValueError("n_top = %d: the device selection takes 1 .. 1024" % n_top)
        if int(cap) < 1 or int(min_common) < 1:
            raise ValueError("cap = %r, min_common = %r: both >= 1" % (cap, min_common))
        out_cnt = self._empty(max(n_q, 1), torch.int32)
        out_user, out_common = self._empty((max(n_q, 1), n_top), torch.int32), self._empty((max(n_q, 1), n_top), torch.int32)
        out_sim = self._empty((max(n_q, 1), n_top), torch.float64)
        F = alive = None
        if allow is not None or exclude is not None or min_sim is not None:
            F, alive = self._rec_filter(index.n_users, n_q, allow, exclude, min_sim)
        flags = (abi.PEERS_SAME if same else 0) | (abi.PEERS_KEEP_SELF if keep_self else 0)
        h = (C.c_int64 * 6)()
        with self.timed("peers"):
            check(lib.xmap_peer_rows(st, i64(n_q), vp(query_user.contiguous()), i64(Q.n_users), vp(Q.user_ptr), vp(Q.user_item),
                                     vp(Q.user_rating64), i32(flags), i32(n_top), i32(cap), i32(min_common), i64(index.n_users),
                                     i32(index.n_items), vp(index.centre), vp(index.hd_ptr), vp(index.hd_user), vp(index.hd_x),
                                     vp(index.nrm), i64(max_records), vp(out_cnt), vp(out_user), vp(out_sim), vp(out_common),
                                     None if F is None else C.byref(F), h))
        del alive
        return out_cnt[:n_q], out_user[:n_q], out_sim[:n_q], out_common[:n_q], tuple(int(x) for x in h)

    def peers_ls(self, index, Q, query_user, n_top, cap=1, min_common=1, same=False, keep_self=False, allow=None, exclude=None,
                 min_sim=None, max_records=0):
        """peers() plus the local sensitivity of every returned entry (xmap_peer_rows_ls): the largest leave-one-out distance of
        the entry's sim over the records the two users share, the second half of the reference's ((id1, id2), [sim, LS]) record of
        a user method.  The arguments of peers(); cnt, user, sim, common and stats are the bytes peers() returns.  Returns (cnt,
        user, sim, common, ls [Q][n_top] (0.0 behind the count), stats)."""
        st = _stream(self.dev)
        n_q, n_top = int(query_user.numel()), int(n_top)
        if not 1 <= n_top <= 1024:
            raise ValueError("n_top = %d: the device selection takes 1 .. 1024" % n_top)
        if int(cap) < 1 or int(min_common) < 1:
            raise ValueError("cap = %r, min_common = %r: both >= 1" % (cap, min_common))
        out_cnt = self._empty(max(n_q, 1), torch.int32)
        out_user, out_common = self._empty((max(n_q, 1), n_top), torch.int32), self._empty((max(n_q, 1), n_top), torch.int32)
        out_sim, out_ls = self._empty((max(n_q, 1), n_top), torch.float64), self._empty((max(n_q, 1), n_top), torch.float64)
        F = alive = None
        if allow is not None or exclude is not None or min_sim is not None:
            F, alive = self._rec_filter(index.n_users, n_q, allow, exclude, min_sim)
        flags = (abi.PEERS_SAME if same else 0) | (abi.PEERS_KEEP_SELF if keep_self else 0)
        h = (C.c_int64 * 6)()
        with self.timed("peers_ls"):
            check(lib.xmap_peer_rows_ls(st, i64(n_q), vp(query_user.contiguous()), i64(Q.n_users), vp(Q.user_ptr), vp(Q.user_item),
                                        vp(Q.user_rating64), i32(flags), i32(n_top), i32(cap), i32(min_common), i64(index.n_users),
                                        i32(index.n_items), vp(index.centre), vp(index.hd_ptr), vp(index.hd_user), vp(index.hd_x),
                                        vp(index.nrm), i64(max_records), vp(out_cnt), vp(out_user), vp(out_sim), vp(out_common),
                                        vp(out_ls), None if F is None else C.byref(F), h))
        del alive
        return out_cnt[:n_q], out_user[:n_q], out_sim[:n_q], out_common[:n_q], out_ls[:n_q], tuple(int(x) for x in h)

    def user_means(self, P):
        """The mean rating of every user of the profiles P over its valid rows (xmap_uknn_means): the exact sum rounded once,
        divided by the count, as the item averages are taken.  Returns (avg float64 [users] -- 0.0 without valid rows --, cnt int32
        [users])."""
        U = int(P.n_users)
        avg, cnt = self._empty(max(U, 1), torch.float64), self._empty(max(U, 1), torch.int32)
        with self.timed("user_means"):
            check(lib.xmap_uknn_means(_stream(self.dev), i64(U), i32(P.n_items), vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64),
                                      vp(avg), vp(cnt)))
        return avg[:U], cnt[:U]

    @staticmethod
    def _uknn_lists(lists):
        cnt, user, sim = [x.contiguous() for x in lists[:3]]
        if user.dim() != 2 or tuple(sim.shape) != tuple(user.shape) or int(cnt.numel()) != int(user.shape[0]):
            raise ValueError("lists = (cnt [Q], user [Q][n_nb], sim [Q][n_nb]) as peers() returns them")
        if cnt.dtype != torch.int32 or user.dtype != torch.int32 or sim.dtype != torch.float64:
            raise ValueError("lists = (cnt int32, user int32, sim float64)")
        n_nb = int(user.shape[1])
        if not 1 <= n_nb <= 1024:
            raise ValueError("n_nb = %d: the lists hold 1 .. 1024 neighbours" % n_nb)
        return cnt, user, sim, n_nb

    def uknn_predict(self, P, lists, query_avg, test_q, test_item, user_avg=None, own_mean=False):
        """User-kNN prediction on the device (xmap_uknn_predict_rows, one wave per test pair): lists = what peers() returned for
        the queries (cnt, user, sim, ...), query_avg float64 [Q] = the queries' own means (user_means() of the profiles the
        queries index, gathered), test_q int32 = the pair's index into the lists, test_item int32.  P: the resident profiles the
        neighbours index.  pred = query mean + sum(sim * (rating - query mean)) / sum(|sim|) over the neighbours' rows that hold
        the item, in list order then profile order; own_mean: rating - the NEIGHBOUR's mean (Resnick; needs user_avg =
        user_means(P)[0]).  Returns (score, bound, n, status): the unrounded prediction, bound_rating of it, the evidence entries,
        and status 0 predicted / 1 no list / 2 the reference raises here / 3 pair out of range."""
        cnt, user, sim, n_nb = self._uknn_lists(lists)
        T, n_q = int(test_q.numel()), int(cnt.numel())
        if own_mean and user_avg is None:
            raise ValueError("own_mean needs user_avg = user_means(P)[0]")
        if int(query_avg.numel()) != n_q:
            raise ValueError("query_avg: one mean per list (%d), not %d" % (n_q, int(query_avg.numel())))
        score, bound = self._empty(max(T, 1), torch.float64), self._empty(max(T, 1), torch.float64)
        n, status = self._empty(max(T, 1), torch.int32), self._empty(max(T, 1), torch.int32)
        with self.timed("uknn_predict"):
            check(lib.xmap_uknn_predict_rows(_stream(self.dev), i64(T), vp(test_q.contiguous()), vp(test_item.contiguous()), i64(n_q),
                                             vp(query_avg.contiguous()), i32(n_nb), vp(cnt), vp(user), vp(sim), i64(P.n_users),
                                             i32(P.n_items), vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64),
                                             vp(None if user_avg is None else user_avg.contiguous()),
                                             i32(abi.UKNN_OWN_MEAN if own_mean else 0), vp(score), vp(bound), vp(n), vp(status)))
        return score[:T], bound[:T], n[:T], status[:T]

    def uknn_topn(self, P, Q, query_user, lists, query_avg, n_top, user_avg=None, own_mean=False, keep_held=False, min_support=1,
                  allow=None, exclude=None, min_score=None, max_records=0):
        """User-kNN top-N on the device (xmap_uknn_topn_rows): per query -- lists / query_avg as uknn_predict() takes them,
        query_user int32 = its index into the profiles Q (the resident ones or a fold-in batch), whose items it holds -- the n_top
        (1..1024) items its neighbours hold with the largest unrounded prediction; score descending, item index ascending.  Held
        items leave unless keep_held; an item with fewer than min_support records is dropped.  allow / exclude / min_score as
        topn() takes them (items; the mask acts in the expansion).  Returns (cnt [Q], item [Q][n_top] (-1 behind the count), score,
        support [Q][n_top], stats) with stats = (candidates, dropped by min_support, dropped as non-finite, dropped below the
        floor, largest candidate count of a query, records expanded).  max_records: the chunk bound (0: the library's)."""
        cnt, user, sim, n_nb = self._uknn_lists(lists)
        n_q, n_top = int(query_user.numel()), int(n_top)
        if not 1 <= n_top <= 1024:
            raise ValueError("n_top = %d: the device selection takes 1 .. 1024" % n_top)
        if int(min_support) < 1:
            raise ValueError("min_support = %r: >= 1" % (min_support,))
        if own_mean and user_avg is None:
            raise ValueError("own_mean needs user_avg = user_means(P)[0]")
        if int(cnt.numel()) != n_q or int(query_avg.numel()) != n_q:
            raise ValueError("one list and one mean per query (%d)" % n_q)
        out_cnt = self._empty(max(n_q, 1), torch.int32)
        out_item, out_support = self._empty((max(n_q, 1), n_top), torch.int32), self._empty((max(n_q, 1), n_top), torch.int32)
        out_score = self._empty((max(n_q, 1), n_top), torch.float64)
        F = alive = None
        if allow is not None or exclude is not None or min_score is not None:
            F, alive = self._rec_filter(P.n_items, n_q, allow, exclude, min_score)
        flags = (abi.UKNN_OWN_MEAN if own_mean else 0) | (abi.UKNN_KEEP_HELD if keep_held else 0)
        h = (C.c_int64 * 6)()
        with self.timed("uknn_topn"):
            check(lib.xmap_uknn_topn_rows(_stream(self.dev), i64(n_q), vp(query_user.contiguous()), i64(Q.n_users), vp(Q.user_ptr),
                                          vp(Q.user_item), vp(query_avg.contiguous()), i32(n_nb), vp(cnt), vp(user), vp(sim),
                                          i64(P.n_users), i32(P.n_items), vp(P.user_ptr), vp(P.user_item), vp(P.user_rating64),
                                          vp(None if user_avg is None else user_avg.contiguous()), i32(flags), i32(n_top),
                                          i32(min_support), i64(max_records), vp(out_cnt), vp(out_item), vp(out_score), vp(out_support),
                                          None if F is None else C.byref(F), h))
        del alive
        return out_cnt[:n_q], out_item[:n_q], out_score[:n_q], out_support[:n_q], tuple(int(x) for x in h)

    def related(self, S, b_ptr, b_item, n_top, how="sum", weights=None, keep_members=False, min_support=1, allow=None, exclude=None,
                min_score=None, max_records=0):
        """Related items for a basket on the device (xmap_related_rows): per basket -- a CSR, b_ptr int64 [Q + 1], b_item int32 --
        the n_top (1..1024) items most related to its members over the rows of the RecommenderSim CSR S (a rec_sim() result, or
        any (row_ptr int64 [I + 1], col int32, sim float64) on the device).  An item's records are the entries that name it in the
        members' rows, position by position, each row in storage order; its score is their sum ("sum"), their mean ("mean") or the
        largest ("max"), with weights (float64, one per basket position) multiplied into the similarities first; score descending,
        item index ascending.  No user and no rating takes part.  The basket's own members leave unless keep_members; a member
        outside the items has no row; an item with fewer than min_support records is dropped.  allow / exclude / min_score as
        topn() takes them (items; the mask and the lists act in the expansion).  Returns (cnt [Q], item [Q][n_top] (-1 behind the
        count), score, support [Q][n_top], stats) with stats = (candidates, dropped by min_support, dropped as non-finite, dropped
        below the floor, largest candidate count of a query, records expanded).  max_records: the chunk bound (0: the library's)."""
        row_ptr, col, sim = (S.row_ptr, S.col, S.sim) if hasattr(S, "row_ptr") else S
        n_items = int(row_ptr.numel()) - 1
        n_q, n_top = int(b_ptr.numel()) - 1, int(n_top)
        if how not in abi.RELATED_HOW:
            raise ValueError("how = %r: one of %s" % (how, sorted(abi.RELATED_HOW)))
        if not 1 <= n_top <= 1024:
            raise ValueError("n_top = %d: the device selection takes 1 .. 1024" % n_top)
        if int(min_support) < 1:
            raise ValueError("min_support = %r: >= 1" % (min_support,))
        if n_q < 0 or b_ptr.dtype != torch.int64 or b_item.dtype != torch.int32:
            raise ValueError("baskets = (b_ptr int64 [Q + 1], b_item int32)")
        if row_ptr.dtype != torch.int64 or col.dtype != torch.int32 or sim.dtype != torch.float64 or n_items < 0:
            raise ValueError("S = (row_ptr int64 [I + 1], col int32, sim float64)")
        if weights is not None and (weights.dtype != torch.float64 or int(weights.numel()) != int(b_item.numel())):
            raise ValueError("weights: float64, one per basket position (%d)" % int(b_item.numel()))
        out_cnt = self._empty(max(n_q, 1), torch.int32)
        out_item, out_support = self._empty((max(n_q, 1), n_top), torch.int32), self._empty((max(n_q, 1), n_top), torch.int32)
        out_score = self._empty((max(n_q, 1), n_top), torch.float64)
        F = alive = None
        if allow is not None or exclude is not None or min_score is not None:
            F, alive = self._rec_filter(n_items, n_q, allow, exclude, min_score)
        h = (C.c_int64 * 6)()
        with self.timed("related"):
            check(lib.xmap_related_rows(_stream(self.dev), i64(n_q), vp(b_ptr.contiguous()), vp(b_item.contiguous()),
                                        vp(None if weights is None else weights.contiguous()), i32(n_items), vp(row_ptr.contiguous()),
                                        vp(col.contiguous()), vp(sim.contiguous()), i32(abi.RELATED_HOW[how]),
                                        i32(abi.RELATED_KEEP_MEMBERS if keep_members else 0), i32(n_top), i32(min_support),
                                        i64(max_records), vp(out_cnt), vp(out_item), vp(out_score), vp(out_support),
                                        None if F is None else C.byref(F), h))
        del alive
        return out_cnt[:n_q], out_item[:n_q], out_score[:n_q], out_support[:n_q], tuple(int(x) for x in h)

    @staticmethod
    def _fuse_args(n_lists, n_top, how, weights, rrf_c, min_lists):
        """the argument checks fuse() and session.fuse_lists share; returns the weights as floats"""
        n_top = int(n_top)
        if not 1 <= n_lists <= abi.FUSE_MAX_LISTS:
            raise ValueError("lists: %d of them, 1 .. %d are fused" % (n_lists, abi.FUSE_MAX_LISTS))
        if how not in abi.FUSE_HOW:
            raise ValueError("how = %r: one of %s" % (how, sorted(abi.FUSE_HOW)))
        if not 1 <= n_top <= 1024:
            raise ValueError("n_top = %d: the device selection takes 1 .. 1024" % n_top)
        w = [1.0] * n_lists if weights is None else [float(x) for x in weights]
        if len(w) != n_lists:
            raise ValueError("weights: one per list (%d)" % n_lists)
        if not all(math.isfinite(x) for x in w):
            raise ValueError("weights = %r: finite" % (w,))
        if not (math.isfinite(float(rrf_c)) and float(rrf_c) >= 0.0):
            raise ValueError("rrf_c = %r: finite and >= 0" % (rrf_c,))
        if not 1 <= int(min_lists) <= n_lists:
            raise ValueError("min_lists = %r: 1 .. %d" % (min_lists, n_lists))
        return w

    def fuse(self, lists, n_top, how="rrf", weights=None, rrf_c=60.0, min_lists=1, n_ids=None, max_records=0):
        """Fused lists on the device (xmap_fuse_rows): lists is a sequence of (cnt int32 [Q], item int32 [Q][width], score float64
        [Q][width] or None, ...) device tensors -- the leading members of what topn(), uknn_topn(), related(), diversify() and
        group_topn() return; row q of every list belongs to the same query.  An id's records are its entries in the lists, list
        after list, rank after rank.  how = "rrf": the sum of weight / (rrf_c + rank) over them (ranks from 1; the scores may be
        None); "sum": the sum of weight * score; "mean": that sum / the sum of the weights.  An id in fewer than min_lists lists
        or with a score that is not finite is dropped; score descending, id ascending.  weights: one per list (None: 1.0 each),
        finite, any sign.  n_ids: the ids are those in [0, n_ids) (None: the items of the engine's ratings).  Returns (cnt [Q],
        id [Q][n_top] (-1 behind the count), score, lists [Q][n_top] (bit l: list l holds the id), stats) with stats =
        (candidates, dropped by min_lists, dropped as non-finite, largest candidate count of a query, records).  (cnt, id) go
        straight into topn_eval() when n_top <= 64.  max_records: the chunk bound of the long-list route (0: the library's)."""
        lists = [tuple(x[:3]) if len(x) >= 3 else (x[0], x[1], None) for x in lists]
        w = self._fuse_args(len(lists), n_top, how, weights, rrf_c, min_lists)
        n_top = int(n_top)
        n_q = int(lists[0][0].numel())
        n_ids = int(self.R.n_items if n_ids is None else n_ids)
        if n_ids < 0 or int(max_records) < 0:
            raise ValueError("n_ids = %r, max_records = %r: >= 0" % (n_ids, max_records))
        arr = (abi.FuseList * len(lists))()
        alive = []
        for l, (cnt, item, score) in enumerate(lists):
            if cnt.dtype != torch.int32 or item.dtype != torch.int32 or int(cnt.numel()) != n_q:
                raise ValueError("lists[%d] = (cnt int32 [%d], item int32 [%d][width], score float64 or None)" % (l, n_q, n_q))
            width = int(item.shape[1]) if item.dim() == 2 else (int(item.numel()) // max(n_q, 1))
            if not 1 <= width <= 1024 or int(item.numel()) != n_q * width:
                raise ValueError("lists[%d]: item is [%d][width] with width 1 .. 1024" % (l, n_q))
            if score is None and how != "rrf":
                raise ValueError("lists[%d]: how = %r needs the scores" % (l, how))
            if score is not None and (score.dtype != torch.float64 or int(score.numel()) != n_q * width):
                raise ValueError("lists[%d]: score is float64 [%d][%d]" % (l, n_q, width))
            cnt, item = cnt.contiguous(), item.contiguous()
            score = None if score is None else score.contiguous()
            alive.append((cnt, item, score))
            arr[l] = abi.FuseList(cnt.data_ptr(), item.data_ptr(), None if score is None else score.data_ptr(), width, w[l])
        out_cnt = self._empty(max(n_q, 1), torch.int32)
        out_id, out_lists = self._empty((max(n_q, 1), n_top), torch.int32), self._empty((max(n_q, 1), n_top), torch.int32)
        out_score = self._empty((max(n_q, 1), n_top), torch.float64)
        h = (C.c_int64 * 5)()
        with self.timed("fuse"):
            check(lib.xmap_fuse_rows(_stream(self.dev), i64(n_q), i32(len(lists)), C.cast(arr, C.c_void_p), i32(n_ids),
                                     i32(abi.FUSE_HOW[how]), C.c_double(float(rrf_c)), i32(min_lists), i32(n_top), i64(max_records),
                                     vp(out_cnt), vp(out_id), vp(out_score), vp(out_lists), h))
        del alive
        return out_cnt[:n_q], out_id[:n_q], out_score[:n_q], out_lists[:n_q], tuple(int(x) for x in h)

    def explain(self,P, neighbors, pair_user, pair_item, item_avg, wtab, n_ev, rank_by=0):
        """Why a pair scores what it scores (xmap_explain_rows, the pair body of predict() in its explain mode): for the (user,
        item) pairs -- int32 tensors, typically the lists of topn() -- the n_ev (1..16) strongest evidence entries of the
        unrounded score of rank_by (0 plain, 1 decayed), ranked by |share| descending, evidence order on ties.  P, neighbors,
        item_avg, wtab as predict() takes them.  Returns (status [T] as predict(), total [T] = evidence entries of the pair,
        cnt [T] = min(n_ev, total), score [T], row [T][n_ev] int64 = index into P's profile arrays (-1 behind the count), slot
        [T][n_ev] = position in the item's neighbour list (-1), share [T][n_ev] = what the entry adds to score - item_avg
        (0.0), max_now)."""
        st = _stream(self.dev)
        cnt, col, sim = [x.contiguous() for x in neighbors[:3]]
        T, n_ev = int(pair_user.numel()), int(n_ev)
        if not 1 <= n_ev <= abi.EXPLAIN_MAX_EV:
            raise ValueError("n_ev = %d: an explanation reports 1 .. %d entries" % (n_ev, abi.EXPLAIN_MAX_EV))
        keep = int(col.shape[1]) if col.dim() == 2 else 1
        T1 = max(T, 1)
        status, total, n_rep = [self._empty(T1, torch.int32) for _ in range(3)]
        score = self._empty(T1, torch.float64)
        row = self._empty((T1, n_ev), torch.int64)
        slot = self._empty((T1, n_ev), torch.int32)
        share = self._empty((T1, n_ev), torch.float64)
        h = C.c_int32(0)
        with self.timed("explain_rows"):
            check(lib.xmap_explain_rows(st, i64(T), vp(pair_user.contiguous()), vp(pair_item.contiguous()), i32(rank_by), i32(n_ev),
                                        i64(P.n_users), i32(P.n_items), i32(keep), vp(cnt), vp(col), vp(sim), vp(P.user_ptr),
                                        vp(P.user_item), vp(P.user_rating64), vp(P.user_time), vp(item_avg.contiguous()), vp(wtab),
                                        i32(wtab.numel()), vp(status), vp(total), vp(n_rep), vp(score), vp(row), vp(slot), vp(share),
                                        C.byref(h)))
        return status[:T], total[:T], n_rep[:T], score[:T], row[:T], slot[:T], share[:T], int(h.value)

    def explain_sources(self, P, pair_user, ex_cnt, ex_row, n_src, sources=None):
        """The provenance of explained rows through stage C (xmap_explain_sources): for every reported row of explain() the raw
        ratings of the user it was made from -- the one raw entry of a pass-through row, the group of raw entries a mapped row
        averages.  P as explain() took it; its .sources (set by alterego_profiles and foldin_profiles) names the raw profiles, or
        pass sources = (raw_ptr, raw_item, cnt_t or None, off_t or None, flags, map) yourself; the profiles of a union have
        none (one map and one raw profile per part).  Returns (src_total [T][n_ev] int32: 0 behind the count, -1 for a row
        outside the user's profile, src_pos [T][n_ev][n_src] int64: positions in the raw item / rating / time arrays, -1 behind
        min(n_src, src_total)); 1 <= n_src <= 8."""
        src = sources if sources is not None else getattr(P, "sources", None)
        if src is None:
            raise ValueError("these profiles carry no raw profiles to walk (a union of AlterEgo rows has one per part)")
        raw_ptr, raw_item, cnt_t, off_t, flags, mp = src
        T, n_src = int(pair_user.numel()), int(n_src)
        n_ev = int(ex_row.shape[1]) if ex_row.dim() == 2 else 1
        if not 1 <= n_src <= abi.EXPLAIN_MAX_SRC:
            raise ValueError("n_src = %d: an explanation reports 1 .. %d sources per entry" % (n_src, abi.EXPLAIN_MAX_SRC))
        T1 = max(T, 1)
        src_total = self._empty((T1, n_ev), torch.int32)
        src_pos = self._empty((T1, n_ev, n_src), torch.int64)
        with self.timed("explain_sources"):
            check(lib.xmap_explain_sources(_stream(self.dev), i64(T), vp(pair_user.contiguous()), i32(n_ev), vp(ex_cnt.contiguous()),
                                           vp(ex_row.contiguous()), i64(P.n_users), i32(P.n_items), vp(P.user_ptr), vp(P.user_item),
                                           vp(cnt_t), vp(off_t), vp(raw_ptr), vp(raw_item), vp(flags), vp(mp), i32(n_src),
                                           vp(src_total), vp(src_pos)))
        return src_total[:T], src_pos[:T]

    def eval_users(self, test_user, test_item, test_rating, rel_min, n_users, n_items):
        """The users worth ranking for (xmap_eval_users): held-out pairs as int32 / int32 / fp64 tensors -> (n_rel [U] int32:
        relevant pairs per user, eval_user int32: the users with n_rel > 0 ascending, counts = (evaluated users, relevant
        pairs, ignored pairs, pairs below rel_min)).  A pair with a user or item outside the index space or a NaN rating is
        ignored; relevant means rating >= rel_min."""
        T, U = int(test_user.numel()), int(n_users)
        n_rel = self._empty(max(U, 1), torch.int32)
        users = self._empty(max(U, 1), torch.int32)
        h = (C.c_int64 * 4)(0, 0, 0, 0)
        with self.timed("eval_users"):
            check(lib.xmap_eval_users(_stream(self.dev), i64(T), vp(test_user.contiguous()), vp(test_item.contiguous()),
                                      vp(test_rating.contiguous()), C.c_double(rel_min), i64(U), i32(n_items), vp(n_rel), vp(users), h))
        return n_rel[:U], users[:int(h[0])], tuple(int(x) for x in h)

    def topn_eval(self, test_user, test_item, test_rating, rel_min, n_rel, query_user, out_cnt, out_item, cutoffs, n_items,
                  per_query=False):
        """Hold-out evaluation of top-N lists on the device (xmap_topn_eval): the lists (out_cnt [Q], out_item [Q][n_top]) as
        topn() returned them for the DISTINCT users query_user, the held-out pairs and n_rel of eval_users(), cutoffs strictly
        ascending within 1 .. n_top (at most 8).  Returns (mask [Q] int64: bit r = position r is a relevant held-out item,
        q_metric [Q][n_cut][5] = (precision, recall, ndcg, ap, rr) or None without per_query, agg [n_cut][8] = (evaluated
        queries, queries with a hit, hits, sum precision, sum recall, sum ndcg, sum ap, sum rr), cover [n_cut] int64 = distinct
        items within the cutoff)."""
        st = _stream(self.dev)
        T, Q = int(test_user.numel()), int(query_user.numel())
        n_top = int(out_item.shape[1]) if out_item.dim() == 2 else 1
        cuts = np.ascontiguousarray([int(c) for c in cutoffs], np.int32)
        n_cut = len(cuts)
        dtab = torch.from_numpy(np.asarray([1.0 / np.log2(r + 2) for r in range(n_top)], np.float64)).to(self.dev)
        mask = self._empty(max(Q, 1), torch.int64)
        q_metric = self._empty((max(Q, 1), max(n_cut, 1), 5), torch.float64) if per_query else None
        agg = self._empty((max(n_cut, 1), 8), torch.float64)
        cover = self._empty(max(n_cut, 1), torch.int64)
        with self.timed("topn_eval"):
            check(lib.xmap_topn_eval(st, i64(T), vp(test_user.contiguous()), vp(test_item.contiguous()), vp(test_rating.contiguous()),
                                     C.c_double(rel_min), i64(n_rel.numel()), i32(n_items), vp(n_rel.contiguous()), i64(Q),
                                     vp(query_user.contiguous()), i32(n_top), vp(out_cnt.contiguous()), vp(out_item.contiguous()),
                                     i32(n_cut), cuts.ctypes.data_as(C.c_void_p), vp(dtab), vp(mask), vp(q_metric), vp(agg), vp(cover)))
        return mask[:Q], (q_metric[:Q] if per_query else None), agg[:n_cut], cover[:n_cut]

    def mae(self, status, real, plain, decay):
        """calculate_mae's sums on the device (xmap_mae): tensor [3] = (predicted pairs, sum |real - plain|, sum |real - decayed|)"""
        out = self._empty(3, torch.float64)
        with self.timed("mae"):
            check(lib.xmap_mae(_stream(self.dev), i64(status.numel()), vp(status.contiguous()), vp(real.contiguous()),
                               vp(plain.contiguous()), vp(decay.contiguous()), vp(out)))
        return out

    def _pinned3(self):
        h = getattr(self, "_h3", None)
        if h is None:
            h = self._h3 = torch.empty(66, dtype=torch.int64, pin_memory=True)
        return h

    def n_profiles(self, G):
        """distinct users present in the AlterEgo output (profiles/s numerator)."""
        n = getattr(G, "n_profiles", None)      # counted by the count pass of alterego()
        if n is not None:
            return int(n)
        U = self.R.n_users
        return int(((G.cnt_t[:U] + G.cnt_m[:U]) > 0).sum().item())


def draw_picks(n_top):
    """cross_nonprivate_mapping's draw (core/generator.py:110): one np.random.randint(0, len(top)-1)
    per start item in ascending start order from the GLOBAL NumPy RNG (the vectorised call consumes
    the stream exactly like the reference's sequential scalar calls).  Singleton candidate lists raise
    ValueError like the reference."""
    n_top = np.asarray(n_top)
    starts = np.nonzero(n_top)[0]
    picks = np.zeros(len(n_top), np.int32)
    if len(starts):
        high = n_top[starts].astype(np.int64) - 1
        if (high <= 0).any():
            raise ValueError("low >= high")
        picks[starts] = np.random.randint(0, high)
    return picks
