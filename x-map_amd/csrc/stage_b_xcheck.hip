// stage_b_xcheck.hip -- the TEST formulations of stage B that the parity tests compare the product against; compiled into
// libxmap_hip_xcheck.so only (csrc/Makefile), never into the product library.
//
// Kernels:
//   k_mid_build<PLACE>, k_mid_dir<FILL> : the dense-table form of the middle lists (XMAP_MID_TABLE=1)
//   k_paths2 (heads_X, flush_end)       : round 1's tile-major enumeration over the middle lists (algo="mid")
// Entry points: xmap_mid_tally, xmap_mid_place, xmap_extend_paths2.
#ifndef XMAP_CROSSCHECK
#error "stage_b_xcheck.hip belongs to libxmap_hip_xcheck.so (-DXMAP_CROSSCHECK) only"
#endif
#include "paths.h"

namespace xmap {

// one wave per (x', position q in NB_BB(x')): lanes over the joint (t,s), each walks attach(s)
template <bool PLACE>
__global__ __launch_bounds__(256) void k_mid_build(MidArgs A) {
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long long)A.n_nb * A.k) return;
    const int xpid = (int)(w / A.k), q = (int)(w % A.k);
    const int xp = A.nb_list[xpid];
    if (q >= A.kcnt[(size_t)xp * 2]) return;
    const size_t o = ((size_t)xp * 2) * A.k + q;
    const int t = A.kcol[o];
    if (!(A.flags[t] & 2)) return;
    const int lane = lane_id();
    const double v2 = A.kval[o * 3], m2 = A.kval[o * 3 + 1], f2 = A.kval[o * 3 + 2];              // edge (x', t)
    for (long long p = A.src_ptr[t] + lane; p < A.src_ptr[t + 1]; p += 64) {
        if (!(A.src_flag[p] & 1)) continue;
        const int s = A.src_idx[p];
        const double v3 = A.src_val[p * 3], m3 = A.src_val[p * 3 + 1], f3 = A.src_val[p * 3 + 2];  // edge (t, s)
        for (long long ap = A.att_ptr[s]; ap < A.att_ptr[s + 1]; ap++) {
            const int xid = A.nb_id[A.att_idx[ap]];
            const size_t tile = (size_t)xpid * A.n_nb + xid;
            if (!PLACE) {
                atomicAdd(&A.tile_cnt[tile], 1);
            } else {
                const long long pos = A.tile_off[tile] + atomicAdd(&A.tile_cnt[tile], 1);
                const double v4 = A.att_val[ap * 3], m4 = A.att_val[ap * 3 + 1], f4 = A.att_val[ap * 3 + 2];  // edge (s, x)
                MidX r;
                r.sm2 = v2 * m2; r.sm3 = v3 * m3; r.sm4 = v4 * m4; r.f2 = f2; r.f3 = f3; r.f4 = f4;
                r.mu = (m2 + m3) + m4; r.xid = xid; r.pad = 0;
                A.midX[pos] = r;
            }
        }
    }
}

// directory of the non-empty tiles of every x' (row of the dense table): count, then fill
template <bool FILL>
__global__ __launch_bounds__(256) void k_mid_dir(int n_nb, const int *tile_cnt, const long long *tile_off,
                                                 int *ng, const long long *dir_ptr, MidDir *dir, const int *nb_list,
                                                 const int *kcnt) {
    const int xpid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (xpid >= n_nb) return;
    const int lane = lane_id();
    const size_t row = (size_t)xpid * n_nb;
    long long out = FILL ? dir_ptr[xpid] : 0;
    int total = 0;
    for (int b = 0; b < n_nb; b += 64) {
        const int xid = b + lane;
        const int c = (xid < n_nb) ? tile_cnt[row + xid] : 0;
        const unsigned long long m = __ballot(c > 0);
        if (FILL && c > 0) {
            MidDir d;
            d.x = nb_list[xid]; d.ne = 1 + kcnt[(size_t)d.x * 2 + 1]; d.cnt = c; d.pad = xid; d.off = tile_off[row + xid];
            dir[out + __popcll(m & lanemask_lt())] = d;
        }
        out += __popcll(m);
        total += __popcll(m);
    }
    if (!FILL && lane == 0) ng[xpid] = total;
}

// merge a lane's register sums into the start's row (distinct ends per call)
__device__ __forceinline__ void flush_end(WaveAcc &W, bool active, int end, double s_hi, double s_lo, double c_hi, double c_lo) {
    bool first = false;
    if (active) {
        double *a = W.acc + (size_t)end * 4;
        double h0 = a[0], l0 = a[1], h1 = a[2], l1 = a[3];
        first = (h1 == 0.0);
        dd_add(h0, l0, s_hi); dd_add(h0, l0, s_lo);
        dd_add(h1, l1, c_hi); dd_add(h1, l1, c_lo);
        a[0] = h0; a[1] = l0; a[2] = h1; a[3] = l1;
    }
    unsigned long long m = __ballot(first);
    if (first) W.touched[W.nt + __popcll(m & lanemask_lt())] = end;
    W.nt += __popcll(m);
}

// Tile-major reduction over the heads of one start.  Up to 64 heads (one per lane) are merged by item x: every
// head's tile directory is sorted by x, so the smallest current x over the lanes is the next tile column; all heads
// that own a tile (x', x) for it are reduced into the SAME register sums before the start's row is touched -- one
// row access per (start, x) instead of one per (head, x) (2.1x fewer at BASELINE configs[1], 25x for the starts
// with many heads).  [xlo, xhi) restricts the columns (work splitting of heavy starts).
__device__ __forceinline__ void heads_X(const Path2Args &B, WaveAcc &W, int start, long long h0, long long nH, int self,
                                        int xlo, int xhi) {
    const PathArgs &A = B.P;
    const int lane = lane_id();
    const int k = A.k;
    const int INF = 0x7fffffff;
    // this lane's head
    const long long h = h0 + lane;
    const bool hv = h < nH;
    double sm1 = 0.0, mu1 = 0.0, f1 = 1.0;
    bool has_e1 = false;
    long long dpos = 0, dend = 0;
    if (hv) {
        int xp = start;
        if (h >= self) {
            const long long rp = A.rnn_ptr[start] + (h - self);
            xp = A.rnn_idx[rp];
            const double sv = A.rnn_val[rp * 3], mu = A.rnn_val[rp * 3 + 1];
            sm1 = sv * mu; mu1 = mu; f1 = A.rnn_val[rp * 3 + 2];
            has_e1 = true;
        }
        const int xpid = B.nb_id[xp];
        dpos = B.dir_ptr[xpid];
        dend = B.dir_ptr[xpid + 1];
        if (xlo > 0) {   // lower bound of xlo in this head's directory (sorted by x)
            long long lo = dpos, hi = dend;
            while (lo < hi) {
                long long mid = (lo + hi) >> 1;
                if (B.dir[mid].x < xlo) lo = mid + 1; else hi = mid;
            }
            dpos = lo;
        }
    }
    MidDir cur;
    cur.x = INF; cur.ne = 0; cur.cnt = 0; cur.pad = 0; cur.off = 0;
    if (hv && dpos < dend) { cur = B.dir[dpos]; if (cur.x >= xhi) cur.x = INF; }
    for (;;) {
        int xmin = cur.x;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { int o = __shfl_xor(xmin, m, 64); xmin = o < xmin ? o : xmin; }
        if (xmin == INF) break;
        const unsigned long long part = __ballot(cur.x == xmin);
        const int x = xmin;
        const int ne = rl32(cur.ne, __ffsll((long long)part) - 1);
        for (int b = 0; b < ne; b += 64) {
            const int idx = b + lane;
            const bool act = idx < ne;
            int end = x;
            double sm5 = 0.0, mu5 = 0.0, f5 = 1.0;
            const bool has5 = act && idx > 0;
            if (has5) {
                size_t o = ((size_t)x * 2 + 1) * k + (idx - 1);
                end = A.kcol[o];
                const double v = A.kval[o * 3], m = A.kval[o * 3 + 1];
                sm5 = v * m; mu5 = m; f5 = A.kval[o * 3 + 2];
            }
            double s_hi = 0.0, s_lo = 0.0, c_hi = 0.0, c_lo = 0.0;
            unsigned long long np = 0;
            unsigned long long pm = part;
            while (pm) {
                const int l = __ffsll((long long)pm) - 1;
                pm &= pm - 1;
                const int cnt = rl32(cur.cnt, l);
                const long long off = rl64(cur.off, l);
                const bool he1 = rl32((int)has_e1, l) != 0;
                const double hsm1 = rld(sm1, l), hmu1 = rld(mu1, l), hf1 = rld(f1, l);
                np += (unsigned long long)cnt;
                for (int r0 = 0; r0 < cnt; r0 += 64) {
                    MidX m;
                    m.sm2 = m.sm3 = m.sm4 = m.f2 = m.f3 = m.f4 = m.mu = 0.0;
                    if (r0 + lane < cnt) m = B.midX[off + r0 + lane];
                    const int nr = (cnt - r0) < 64 ? (cnt - r0) : 64;
                    // the part of a path's value that does not depend on the end is computed once per (head, record),
                    // on the record's lane (same operations in the same order as the per-path statement), and three
                    // doubles instead of seven are broadcast per step
                    double bsm, bc;
                    if (he1) { bsm = ((hsm1 + m.sm2) + m.sm3) + m.sm4; bc = ((hf1 * m.f2) * m.f3) * m.f4; }
                    else { bsm = (m.sm2 + m.sm3) + m.sm4; bc = (m.f2 * m.f3) * m.f4; }
                    const double bmu = m.mu + (he1 ? hmu1 : 0.0);
                    for (int r = 0; r < nr; r++) {
                        double sm = rld(bsm, r), c = rld(bc, r), mu = rld(bmu, r);
                        if (has5) { sm = sm + sm5; c = c * f5; mu = mu + mu5; }
                        const double sp = (mu != 0.0) ? 1.0 * sm / mu : 0.0;
                        dd_add(s_hi, s_lo, sp * c);
                        dd_add(c_hi, c_lo, c);
                    }
                }
            }
            flush_end(W, act, end, s_hi, s_lo, c_hi, c_lo);
            W.paths += np * (unsigned long long)__popcll(__ballot(act));
        }
        if (cur.x == xmin) {    // advance the heads that took part
            dpos++;
            cur.x = INF;
            if (dpos < dend) { cur = B.dir[dpos]; if (cur.x >= xhi) cur.x = INF; }
        }
    }
}

// 5 waves per SIMD (94 VGPRs, 68 B of scratch per lane) measured 6 % faster than the 4 the unconstrained allocation
// (112 VGPRs) allows, 6 (80 VGPRs, 128 B of scratch) 8 % slower: the kernel is bound by its random row updates, more
// waves keep more of them in flight
constexpr int B_WAVES = 5;
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(B_WAVES, B_WAVES))) void k_paths2(Path2Args B) {
    __shared__ FinBuf fin[4];
    const PathArgs &A = B.P;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= A.n_slots) return;
    const int lane = lane_id();
    WaveAcc W;
    W.paths = 0;
    unsigned long long cand_total = 0;
    for (;;) {
        int u_ = 0;
        if (lane == 0) u_ = (int)atomicAdd(&A.counters[2], 1ull);
        const int unit = uniform(u_);
        if (unit >= A.n_units) break;  // every wave reaches this exit: the cursor only grows
        const int start = uniform(A.unit_start[unit]);
        const int c = uniform(A.unit_c[unit]);
        const int G = uniform(A.unit_G[unit]);
        const int row = uniform(A.unit_row[unit]);
        if (row < 0) {
            W.acc = A.acc + (size_t)slot * A.I * 4;
            W.touched = A.touched + (size_t)slot * A.I;
        } else {
            W.acc = A.hacc + (size_t)row * A.I * 4;
            W.touched = A.htouched + (size_t)row * A.I;
        }
        W.nt = 0;
        int ent = 0;  // work entries of a start: role T; per head its (t,s) part; per (64-head batch, column range) the tiles
        if (A.flags[start] & 2) {   // role T: non-joint paths from t = start (final_nonjoint_extend, extender.py:124-140,:180)
            if (G == 1 || ent % G == c) {
                Carry none; none.sm = 0; none.mu = 0; none.c = 0;
                through_t(A, W, start, false, none);
            }
            ent++;
        }
        const long long r0 = uniform((int)A.rnn_ptr[start]), r1 = uniform((int)A.rnn_ptr[start + 1]);
        const int self = (A.cls[start] == 2) ? 1 : 0;   // head 0 = the start itself (target_path, extender.py:160-163)
        const long long nH = self + (r1 - r0);          // heads >= self: start in NN(x') (longest_path, :164-167)
        for (long long h = 0; h < nH; h++) {
            if (G == 1 || ent % G == c) {
                const bool has_e1 = h >= self;
                const int xp = has_e1 ? A.rnn_idx[r0 + h - self] : start;
                Carry e1; e1.sm = 0; e1.mu = 0; e1.c = 1.0;
                if (has_e1) e1 = first_edge(A.rnn_val[(r0 + h - self) * 3], A.rnn_val[(r0 + h - self) * 3 + 1],
                                            A.rnn_val[(r0 + h - self) * 3 + 2]);
                head_S(A, W, xp, has_e1, e1);
            }
            ent++;
        }
        const long long nbatch = (nH + 63) / 64;
        const int RX = (nbatch > 0) ? (int)((G + nbatch - 1) / nbatch) : 1;   // column ranges: nbatch * RX >= G entries
        const int n_nb = B.n_nb;
        for (long long bt = 0; bt < nbatch; bt++)
            for (int rx = 0; rx < RX; rx++) {
                if (G == 1 || ent % G == c) {
                    const int xlo = (rx == 0) ? 0 : B.nb_list[(long long)rx * n_nb / RX];
                    const int xhi = (rx == RX - 1) ? 0x7fffffff : B.nb_list[(long long)(rx + 1) * n_nb / RX];
                    heads_X(B, W, start, bt * 64, nH, self, xlo, xhi);
                }
                ent++;
            }
        if (row < 0) cand_total += finalize_start(A, fin[threadIdx.x >> 6], W.acc, W.touched, W.nt, start);
        else if (lane == 0) A.unit_nt[unit] = W.nt;
    }
    if (lane == 0) {
        atomicAdd(&A.counters[0], cand_total);
        atomicAdd(&A.counters[1], W.paths);
    }
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_mid_tally(void *stream, const xmap_ext_tables *T, int32_t *tile_cnt /*[n_nb*n_nb], zeroed here*/, int32_t *ng /*[n_nb]*/) {
    XM_ARG(T);
    XM_ARG(T->cls && T->kcnt && T->kcol && T->kval && T->flags && T->att_ptr && T->src_ptr && T->nb_list && T->nb_id && tile_cnt && ng);
    const int n_nb = T->n_nb;
    if (n_nb == 0) return XMAP_OK;
    hipStream_t st = (hipStream_t)stream;
    MidArgs A = mid_args(T);
    A.tile_cnt = tile_cnt;
    XM_HIP(hipMemsetAsync(tile_cnt, 0, sizeof(int32_t) * (size_t)n_nb * (size_t)n_nb, st));
    const long long waves = (long long)n_nb * T->top_k;
    k_mid_build<false><<<dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st>>>(A);
    XM_LAUNCH_CHECK();
    k_mid_dir<false><<<dim3((unsigned)((n_nb + 3) / 4)), dim3(256), 0, st>>>(n_nb, tile_cnt, nullptr, ng, nullptr, nullptr,
                                                                             nullptr, nullptr);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

int xmap_mid_place(void *stream, const xmap_ext_tables *T, int32_t *tile_cnt, const int64_t *tile_off /*[n_nb*n_nb+1]*/,
                   void *dir /*24 B per tile*/, void *midX /*64 B per record*/) {
    XM_ARG(T);
    XM_ARG(T->cls && T->kcnt && T->kcol && T->kval && T->flags && T->att_ptr && T->src_ptr && T->nb_list && T->nb_id);
    XM_ARG(tile_cnt && tile_off && T->dir_ptr && dir && midX);
    const int n_nb = T->n_nb;
    if (n_nb == 0) return XMAP_OK;
    hipStream_t st = (hipStream_t)stream;
    MidArgs A = mid_args(T);
    A.tile_cnt = tile_cnt; A.tile_off = (const long long *)tile_off; A.midX = (MidX *)midX;
    k_mid_dir<true><<<dim3((unsigned)((n_nb + 3) / 4)), dim3(256), 0, st>>>(n_nb, tile_cnt, (const long long *)tile_off,
                                                                            nullptr, (const long long *)T->dir_ptr, (MidDir *)dir, T->nb_list, T->kcnt);
    XM_LAUNCH_CHECK();
    XM_HIP(hipMemsetAsync(tile_cnt, 0, sizeof(int32_t) * (size_t)n_nb * (size_t)n_nb, st));   // now the placement cursors
    const long long waves = (long long)n_nb * T->top_k;
    k_mid_build<true><<<dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st>>>(A);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

int xmap_extend_paths2(void *stream, const xmap_ext_tables *T, const xmap_path_units *U, const xmap_path_rows *R,
                       const xmap_path_out *O, const int32_t *ng, int64_t *d_counters, int64_t *h_counters) {
    XM_ARG(T && ng);
    XM_ARG(T->nb_id && T->nb_list && T->midX && T->dir && T->dir_ptr && T->n_nb > 0);
    Path2Args B;
    memset(&B, 0, sizeof(B));
    B.nb_id = T->nb_id; B.nb_list = T->nb_list; B.n_nb = T->n_nb; B.midX = (const MidX *)T->midX; B.dir = (const MidDir *)T->dir;
    B.dir_ptr = (const long long *)T->dir_ptr; B.ng = ng;
    return extend_paths_run(stream, T, U, R, O, d_counters, h_counters, [&B](const PathArgs &A, dim3 grid, hipStream_t st) {
        B.P = A;
        k_paths2<<<grid, dim3(256), 0, st>>>(B);
    });
}

}
