// paths.h -- what the files of stage B share: the kernel arguments (PathArgs, Path2Args, MidArgs) and how the host fills them
// from the structs of the C ABI, the carry of a path and its per-path walks, the row accumulator of the per-path kernels,
// the finalisation of a start's row, the middle-list records, the column tables and the list thresholds.
//   knn.hip        bridge flags, the classified top-k lists and their thresholds
//   reverse.hip    the reverse adjacencies (attach / src / rnn)
//   mid_rows.hip   the middle lists, built row-wise (k_mid_rows)
//   paths_enum.hip the per-start path counts, the per-path fallback k_paths, k_topc_lists
//   paths4.hip     the default enumeration k_paths4 and the merges of the heavy starts
//   plan.hip       the planning steps (work units, the order of the end universe)
//   stage_b_xcheck.hip (libxmap_hip_xcheck.so only): the dense-table middle lists and k_paths2
#pragma once
#include "common.h"

namespace xmap {

struct PathArgs {
    int I, k;
    const uint8_t *cls;
    const int *kcnt;
    const int *kcol;
    const double *kval;
    const uint8_t *flags;
    const long long *att_ptr; const int *att_idx; const double *att_val;
    const long long *src_ptr; const int *src_idx; const double *src_val; const uint8_t *src_flag;
    const long long *rnn_ptr; const int *rnn_idx; const double *rnn_val;
    // work units: (start, chunk c of G).  G == 1: the unit owns the start, accumulates in the wave's slot
    // row and finalises it.  G > 1: the start's (head, t) entries are dealt round-robin to G units, each
    // with a dedicated row (unit_row); k_merge adds the rows up and finalises.
    int n_units;
    const int *unit_start; const int *unit_c; const int *unit_G; const int *unit_row; int *unit_nt;
    int n_slots;
    double *acc; int *touched;     // slot rows   [n_slots][I][4] / [n_slots][I]
    double *hacc; int *htouched;   // heavy rows  [n_rows][I][4]  / [n_rows][I]
    int *n_cand; int *top_end; double *top_val;
    long long xs_cap; long long *xs_off; int *xs_end; double *xs_val;
    unsigned long long *counters;  // [0] total candidates, [1] paths, [2] work cursor, [3] xs cursor
    // rows of k_paths4 are indexed by the rank of an item among the items that can end a path (U of them) instead of by
    // the item: uitem[rank] = item, urank[item] = rank.  The older kernels leave these NULL / U = I.
    int U; const int *urank; const int *uitem;
    long long row_stride;          // entries per slot row of k_paths4 (= U)
};

struct Carry { double sm, mu, c; };  // sum sim*mutu, sum mutu, prod frac_mutu along the path so far

__device__ __forceinline__ Carry first_edge(double sim, double mutu, double frac) {
    Carry r; r.sm = sim * mutu; r.mu = mutu; r.c = frac; return r;   // python sum(): 0 + x == x
}
__device__ __forceinline__ Carry add_edge(Carry a, double sim, double mutu, double frac) {
    Carry r; r.sm = a.sm + sim * mutu; r.mu = a.mu + mutu; r.c = a.c * frac; return r;
}

// tails of one (t,s) after edge (t,s): end s is accumulated by the caller (vector step over s);
// here: for x in attach(s): end x, then end y for y in NN(x)         (extender.py:134-138 / :154-158)
template <class ACC>
__device__ __forceinline__ void tails(const PathArgs &A, ACC &W, int s, Carry c_ts) {
    const int lane = lane_id();
    const int k = A.k;
    long long a0 = A.att_ptr[s], a1 = A.att_ptr[s + 1];
    for (long long ap = a0; ap < a1; ap++) {
        const int x = A.att_idx[ap];
        const Carry c_sx = add_edge(c_ts, A.att_val[ap * 3], A.att_val[ap * 3 + 1], A.att_val[ap * 3 + 2]);
        const int nn = A.kcnt[(size_t)x * 2 + 1];
        for (int b = 0; b < nn + 1; b += 64) {
            int idx = b + lane;
            bool act = idx < nn + 1;
            int end = x;
            Carry c = c_sx;
            if (act && idx > 0) {
                size_t o = ((size_t)x * 2 + 1) * k + (idx - 1);
                end = A.kcol[o];
                c = add_edge(c_sx, A.kval[o * 3], A.kval[o * 3 + 1], A.kval[o * 3 + 2]);
            }
            W.add(act, end, c);
        }
    }
}

// all (t,s) of src(t) behind a given head carry (head_len = number of edges in front of (t,s))
template <class ACC>
__device__ __forceinline__ void through_t(const PathArgs &A, ACC &W, int t, bool has_head, Carry head) {
    const int lane = lane_id();
    long long s0 = A.src_ptr[t], s1 = A.src_ptr[t + 1];
    for (long long base = s0; base < s1; base += 64) {
        long long p = base + lane;
        bool act = p < s1;
        int s = 0;
        Carry c; c.sm = 0; c.mu = 0; c.c = 0;
        if (act) {
            if (has_head && !(A.src_flag[p] & 1)) act = false;  // joint paths need (t,s) in TGT as well
        }
        if (act) {
            s = A.src_idx[p];
            double sv = A.src_val[p * 3], mu = A.src_val[p * 3 + 1], fr = A.src_val[p * 3 + 2];
            c = has_head ? add_edge(head, sv, mu, fr) : first_edge(sv, mu, fr);
        }
        W.add(act, s, c);  // path ... -> t -> s
        unsigned long long m = __ballot(act);
        while (m) {
            int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            int sb = rl32(s, l);
            Carry cb;
            cb.sm = rld(c.sm, l); cb.mu = rld(c.mu, l); cb.c = rld(c.c, l);
            tails(A, W, sb, cb);
        }
    }
}

// Error-free accumulation (Knuth two-sum, double-double running sums): the per-(start,end) sums become
// independent of the order in which paths are enumerated (to ~2^-104), so items with identical
// path multisets tie exactly and the tie-break (ascending end index) is well defined.
struct WaveAcc {
    double *acc; int *touched; int nt; unsigned long long paths;
    __device__ __forceinline__ void add(bool active, int end, Carry p) {
        bool first = false;
        if (active) {
            double sp = (p.mu != 0.0) ? 1.0 * p.sm / p.mu : 0.0;   // calculate_path_confidence (extender.py:83-89)
            double *a = acc + (size_t)end * 4;
            double s_hi = a[0], s_lo = a[1], c_hi = a[2], c_lo = a[3];
            first = (c_hi == 0.0);
            dd_add(s_hi, s_lo, sp * p.c);
            dd_add(c_hi, c_lo, p.c);
            a[0] = s_hi; a[1] = s_lo; a[2] = c_hi; a[3] = c_lo;
        }
        unsigned long long m = __ballot(first);
        if (first) touched[nt + __popcll(m & lanemask_lt())] = end;
        nt += __popcll(m);
        paths += __popcll(__ballot(active));
    }
};

// wave-wide selection of the XMAP_TOPC best of nt candidates in the order (|xsim| desc, end asc);
// get(b, end, val) returns candidate b.  Lane 0 writes the result.
template <typename Get>
__device__ __forceinline__ void select_topc(int nt, Get get, int *top_end, double *top_val) {
    const int lane = lane_id();
    unsigned long long pk = 0;
    int pe = -1;
    int nsel = nt < XMAP_TOPC ? nt : XMAP_TOPC;
    for (int r = 0; r < nsel; r++) {
        unsigned long long bk = 0;
        int be = 0x7fffffff;
        double bv = 0.0;
        bool have = false;
        for (int b = lane; b < nt; b += 64) {
            int e; double v;
            get(b, e, v);
            unsigned long long key = (unsigned long long)__double_as_longlong(fabs(v));
            bool after_prev = (r == 0) || (key < pk) || (key == pk && e > pe);
            if (after_prev && (!have || key > bk || (key == bk && e < be))) { bk = key; be = e; bv = v; have = true; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            unsigned long long ok = __shfl_xor(bk, m, 64);
            int oe = __shfl_xor(be, m, 64);
            double ov = __shfl_xor(bv, m, 64);
            int oh = __shfl_xor((int)have, m, 64);
            if (oh && (!have || ok > bk || (ok == bk && oe < be))) { bk = ok; be = oe; bv = ov; have = true; }
        }
        pk = bk; pe = be;
        if (lane == 0) { top_end[r] = be; top_val[r] = bv; }
    }
}

// xsim = sum(s_p c_p) / sum(c_p) (get_sim, extender.py:198-201), fused top-XMAP_TOPC by (|xsim| desc,
// end asc) -- all a Generator reads (generator.py:85,109) --, optional full lists, row reset.
// ONE pass over the start's row: every touched entry is read once, divided, (full mode: written to the start's list,)
// zeroed, and offered to a running selection.  The row entries are random 32-byte accesses to HBM (a row is larger than
// an XCD's L2), so the earlier form -- a division pass, XMAP_TOPC selection passes over the row and a reset pass -- cost
// 12 random accesses per candidate against ~6 for accumulating it.  Running selection: candidates whose key is >= the
// key of the XMAP_TOPC-th best so far (ties included: the order among equal keys is by end index) are appended to a
// per-wave LDS buffer; when it passes FIN_CAP entries it is cut back to its exact XMAP_TOPC best, which raises the
// threshold.  An entry is only ever dropped when XMAP_TOPC entries with a strictly larger key exist, so the result is
// the exact top of the whole list; a stream in random order appends ~XMAP_TOPC ln(nt / XMAP_TOPC) entries.
constexpr int FIN_CAP = 128;
struct FinBuf { double v[FIN_CAP + 64]; int e[FIN_CAP + 64]; double ov[XMAP_TOPC]; int oe[XMAP_TOPC]; };

__device__ __forceinline__ unsigned long long xsim_key(double v) { return (unsigned long long)__double_as_longlong(fabs(v)); }

// the full-list cursor of one start (lane 0 draws it); returns whether the list fits
__device__ __forceinline__ bool fin_list_offset(const PathArgs &A, int nt, int start, unsigned long long &off) {
    off = 0;
    if (!(A.xs_cap > 0 && nt > 0)) return false;   // full candidate lists (extender_pipeline's RDD) via a cursor
    if (lane_id() == 0) off = atomicAdd(&A.counters[3], (unsigned long long)nt);
    off = ((unsigned long long)(unsigned)rl32((int)(off >> 32), 0) << 32) | (unsigned)rl32((int)(off & 0xffffffffull), 0);
    const bool full = (long long)(off + nt) <= A.xs_cap;
    if (lane_id() == 0) A.xs_off[start] = full ? (long long)off : -1;
    return full;
}

// exact XMAP_TOPC best of the nbuf buffered candidates; lane 0 writes them in order
__device__ __forceinline__ int fin_cut(FinBuf &F, int nbuf, int *out_e, double *out_v) {
    volatile double *bv = F.v;
    volatile int *be = F.e;
    select_topc(nbuf, [&](int b, int &e, double &v) { e = be[b]; v = bv[b]; }, out_e, out_v);
    return nbuf < XMAP_TOPC ? nbuf : XMAP_TOPC;
}

// One wave's share of the pass: candidates b = 64 (w + j NW) + lane.  Leaves the best ns of them, in order, in
// F.oe / F.ov and returns ns.
__device__ __forceinline__ int finalize_slice(const PathArgs &A, FinBuf &F, double *acc, const int *touched, int nt,
                                              unsigned long long off, bool full, int w, int NW, int gs = 1, int mem = 0) {
    const int lane = lane_id();
    volatile double *bv = F.v;
    volatile int *be = F.e;
    int nbuf = 0;
    unsigned long long thr = 0;   // key of the XMAP_TOPC-th best so far (0 while fewer have been seen)
    for (int b0 = 64 * w; b0 < nt; b0 += 64 * NW) {
        const int b = b0 + lane;
        const bool act = b < nt;
        int e = 0;
        double v = 0.0;
        unsigned long long key = 0;
        if (act) {
            e = touched[b];
            double *a = acc + ((size_t)e * gs + mem) * 4;
            v = 1.0 * (a[0] + a[1]) / (a[2] + a[3]);     // pairs of k_paths4 are not renormalised; a renormalised pair is its own sum
            a[0] = 0.0; a[1] = 0.0; a[2] = 0.0; a[3] = 0.0;
            key = xsim_key(v);
            if (full) { A.xs_end[off + b] = A.uitem ? A.uitem[e] : e; A.xs_val[off + b] = v; }
        }
        // (rows of k_paths4 are indexed by end RANK; the item behind a rank -- a random 4-byte gather, a third of the pass's
        //  memory requests -- is looked up only for the candidates that pass the running threshold: ~10 ln(n / 10) per start)
        const bool q = act && key >= thr;
        const unsigned long long m = __ballot(q);
        if (q) { const int p = nbuf + __popcll(m & lanemask_lt()); bv[p] = v; be[p] = A.uitem ? A.uitem[e] : e; }
        nbuf += __popcll(m);
        if (nbuf > FIN_CAP) {
            const int ns = fin_cut(F, nbuf, F.oe, F.ov);
            int te = 0;
            double tv = 0.0;
            if (lane < ns) { te = ((volatile int *)F.oe)[lane]; tv = ((volatile double *)F.ov)[lane]; }
            if (lane < ns) { be[lane] = te; bv[lane] = tv; }
            nbuf = ns;
            thr = (ns == XMAP_TOPC) ? xsim_key(rld(tv, XMAP_TOPC - 1)) : 0ull;
        }
    }
    return fin_cut(F, nbuf, F.oe, F.ov);
}

__device__ __forceinline__ int finalize_start(const PathArgs &A, FinBuf &F, double *acc, const int *touched, int nt, int start,
                                              int gs = 1, int mem = 0) {
    const int lane = lane_id();
    if (lane == 0) A.n_cand[start] = nt;
    unsigned long long off;
    const bool full = fin_list_offset(A, nt, start, off);
    const int ns = finalize_slice(A, F, acc, touched, nt, off, full, 0, 1, gs, mem);
    if (lane < ns) {
        A.top_end[(size_t)start * XMAP_TOPC + lane] = ((volatile int *)F.oe)[lane];
        A.top_val[(size_t)start * XMAP_TOPC + lane] = ((volatile double *)F.ov)[lane];
    }
    return nt;
}

// a middle-list record and a tile directory entry (built by k_mid_rows, mid_rows.hip)
struct MidX { double sm2, sm3, sm4, f2, f3, f4, mu; int xid; int pad; };   // 64 B; xid = index of x in nb_list
struct MidDir { int x; int ne; int cnt; int pad; long long off; };          // one tile of x': item x, 1+|NN(x)| ends, records [off, off+cnt); pad = index of x in nb_list

// Second formulation of the enumeration ("middle lists").  Every joint path has the shape
//   [y'] - x' - t - s - [x - [y]]      with x', x non-bridge items, t in NB_BB(x'), (t,s) joint.
// For each non-bridge x' the middles (t,s,x) are materialised ONCE, grouped by x (one "tile" per (x', x); a dense
// n_nb x n_nb count table gives the tile offsets, so the build is a tally pass + a placement pass over
// (x', t) work items -- no per-x' serial section).  A head (start, x') then streams the tiles of x': all
// records of one tile hit the same ends {x} U NN(x), so each lane keeps its end's double-double sums in
// REGISTERS across the tile and the start's row in HBM is touched once per (head, tile) instead of once per
// path.  The edge products sim*mutu and the fractions are stored per edge, so a path's (sum sim*mutu, sum
// mutu, prod frac) is rebuilt in the reference's left-to-right order, bit for bit.

struct MidArgs {
    int I, k;
    const uint8_t *cls; const int *kcnt; const int *kcol; const double *kval; const uint8_t *flags;
    const long long *att_ptr; const int *att_idx; const double *att_val;
    const long long *src_ptr; const int *src_idx; const double *src_val; const uint8_t *src_flag;
    int n_nb; const int *nb_list; const int *nb_id;
    const long long *jptr; const int *joff;     // joint (t, s) of every t, compacted: offsets into src(t) (k_joint_list; k_mid_rows)
    const int *axid;                            // column of every attach entry (k_att_columns)
    const long long *xoff; int *xl;             // rows wider than the LDS span: the columns of a row's records in walk order, [xoff[x'], xoff[x'+1])
    int *tile_cnt;                 // [n_nb * n_nb] tally, then placement cursor
    const long long *tile_off;     // [n_nb * n_nb + 1]
    MidX *midX;
};

// the value of lane SRC of every quad, in all four lanes of the quad (DPP quad_perm: no LDS traffic)
template <int SRC>
__device__ __forceinline__ double quad_bcast(double v) {
    constexpr int CTRL = SRC | (SRC << 2) | (SRC << 4) | (SRC << 6);
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

struct ColEnd { double sm, mu, f; int u; int pad; };     // one end of a column x: last edge (sim * mutu, mutu, frac; 0, 0, 1 for x itself), universe rank
struct Path2Args {
    PathArgs P;
    const ColEnd *cend;            // k_paths4: [n_nb][k + 1]
    const int *nb_id; const int *nb_list; int n_nb;
    const MidX *midX; const MidDir *dir; const long long *dir_ptr; const int *ng;
};

// paths [start -] x' - t - s of one head (end s): lanes over the joint (t,s) of each t in NB_BB(x')
template <class ACC>
__device__ __forceinline__ void head_S(const PathArgs &A, ACC &W, int xp, bool has_e1, Carry e1) {
    const int lane = lane_id();
    const int nb = A.kcnt[(size_t)xp * 2];
    for (int q = 0; q < nb; q++) {
        const size_t o = ((size_t)xp * 2) * A.k + q;
        const int t = A.kcol[o];
        if (!(A.flags[t] & 2)) continue;
        const Carry c2 = has_e1 ? add_edge(e1, A.kval[o * 3], A.kval[o * 3 + 1], A.kval[o * 3 + 2])
                                : first_edge(A.kval[o * 3], A.kval[o * 3 + 1], A.kval[o * 3 + 2]);
        const long long s0 = A.src_ptr[t], s1 = A.src_ptr[t + 1];
        for (long long base = s0; base < s1; base += 64) {
            const long long p = base + lane;
            const bool act = (p < s1) && (A.src_flag[p] & 1);
            int s = 0;
            Carry c = c2;
            if (act) {
                s = A.src_idx[p];
                c = add_edge(c2, A.src_val[p * 3], A.src_val[p * 3 + 1], A.src_val[p * 3 + 2]);
            }
            W.add(act, s, c);
        }
    }
}

// the last entry of every top-k list as one 16-byte record (12.8 MB for 4e5 items: resident in the Infinity Cache, where the
// lists themselves, 1.1 GB, are not): written by k_knn_thresholds (knn.hip), read by the membership tests of reverse.hip
struct KnnThr { double la; int col; int cnt; };

// the partial rows of the heavy starts added up and finalised (k_merge_groups, k_merge: paths4.hip)
int merge_heavy(hipStream_t st, const PathArgs &A, int n_heavy, const int *heavy_unit0);

// ---- host side: the kernel arguments from the structs of the C ABI (include/xmap_hip.h) ---------------------------------
// item-indexed rows (U = I, no rank tables): what k_paths and k_paths2 take; xmap_extend_cols puts the end universe on top
inline PathArgs path_args(const xmap_ext_tables *T, const xmap_path_units *U, const xmap_path_rows *R, const xmap_path_out *O,
                          int64_t *d_counters) {
    PathArgs A;
    A.I = T->n_items; A.k = T->top_k;
    A.cls = T->cls; A.kcnt = T->kcnt; A.kcol = T->kcol; A.kval = T->kval; A.flags = T->flags;
    A.att_ptr = (const long long *)T->att_ptr; A.att_idx = T->att_idx; A.att_val = T->att_val;
    A.src_ptr = (const long long *)T->src_ptr; A.src_idx = T->src_idx; A.src_val = T->src_val; A.src_flag = T->src_flag;
    A.rnn_ptr = (const long long *)T->rnn_ptr; A.rnn_idx = T->rnn_idx; A.rnn_val = T->rnn_val;
    A.n_units = U->n_units; A.unit_start = U->unit_start; A.unit_c = U->unit_c; A.unit_G = U->unit_G; A.unit_row = U->unit_row;
    A.unit_nt = U->unit_nt;
    A.n_slots = R->n_slots < U->n_units ? R->n_slots : U->n_units;
    A.acc = R->acc; A.touched = R->touched; A.hacc = R->hacc; A.htouched = R->htouched;
    A.n_cand = O->n_cand; A.top_end = O->top_end; A.top_val = O->top_val;
    A.xs_cap = O->xs_cap; A.xs_off = (long long *)O->xs_off; A.xs_end = O->xs_end; A.xs_val = O->xs_val;
    A.counters = (unsigned long long *)d_counters;
    A.U = T->n_items; A.urank = nullptr; A.uitem = nullptr; A.row_stride = T->n_items;
    return A;
}

// what the middle-list builders read of the tables (the call's own temporaries and outputs stay zero)
inline MidArgs mid_args(const xmap_ext_tables *T) {
    MidArgs A;
    memset(&A, 0, sizeof(A));
    A.I = T->n_items; A.k = T->top_k; A.cls = T->cls; A.kcnt = T->kcnt; A.kcol = T->kcol; A.kval = T->kval; A.flags = T->flags;
    A.att_ptr = (const long long *)T->att_ptr; A.att_idx = T->att_idx; A.att_val = T->att_val;
    A.src_ptr = (const long long *)T->src_ptr; A.src_idx = T->src_idx; A.src_val = T->src_val; A.src_flag = T->src_flag;
    A.n_nb = T->n_nb; A.nb_list = T->nb_list; A.nb_id = T->nb_id;
    return A;
}

// A per-path enumeration over item-indexed rows (xmap_extend_paths: paths_enum.hip; xmap_extend_paths2: stage_b_xcheck.hip):
// the argument checks, the counters, launch(A, grid, stream) of the caller's kernel, the merge of the heavy starts and the
// counters read back.
template <class Launch>
inline int extend_paths_run(void *stream, const xmap_ext_tables *T, const xmap_path_units *U, const xmap_path_rows *R,
                            const xmap_path_out *O, int64_t *d_counters, int64_t *h_counters, Launch &&launch) {
    XM_ARG(T && U && R && O);
    XM_ARG(T->cls && T->kcnt && T->kcol && T->kval && T->flags && T->att_ptr && T->src_ptr && T->rnn_ptr);
    XM_ARG(R->acc && R->touched && O->n_cand && O->top_end && O->top_val && d_counters);
    XM_ARG(R->n_slots > 0 && U->n_units >= 0 && U->n_heavy >= 0);
    XM_ARG(U->n_units == 0 || (U->unit_start && U->unit_c && U->unit_G && U->unit_row && U->unit_nt));
    XM_ARG(U->n_heavy == 0 || (U->heavy_unit0 && R->hacc && R->htouched));
    XM_ARG(O->xs_cap == 0 || (O->xs_off && O->xs_end && O->xs_val));
    hipStream_t st = (hipStream_t)stream;
    XM_HIP(hipMemsetAsync(d_counters, 0, 4 * sizeof(int64_t), st));
    if (U->n_units > 0) {
        const PathArgs A = path_args(T, U, R, O, d_counters);
        launch(A, dim3((unsigned)((A.n_slots + 3) / 4)), st);
        XM_LAUNCH_CHECK();
        if (U->n_heavy > 0) {
            const int rc = merge_heavy(st, A, U->n_heavy, U->heavy_unit0);
            if (rc) return rc;
        }
    }
    if (h_counters) {
        XM_HIP(hipMemcpyAsync(h_counters, d_counters, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
        if (O->xs_cap > 0 && h_counters[0] > O->xs_cap) {
            set_error("candidate buffer too small: need %lld entries, have %lld", (long long)h_counters[0],
                      (long long)O->xs_cap);
            return XMAP_ERR_CAPACITY;
        }
    }
    return XMAP_OK;
}

}  // namespace xmap
