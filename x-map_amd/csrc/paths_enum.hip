// paths_enum.hip -- stage B: the exact per-start path counts and the per-path enumeration (ExtendSim.sim_extend +
// get_final_extension, core/extender.py:46-217).  The default enumeration over the middle lists is k_paths4 (paths4.hip);
// the carry of a path, its walks, the row accumulator and the finalisation of a start are in paths.h.
//
// Kernels:
//   k_w_tails, k_w_src, k_w_heads, k_w_starts : exact per-start path counts (scheduling weights)
//   k_paths      : per-path enumeration, one wave per start (the fallback beyond the middle-list budget and when nothing is
//                  joint; cross-check of k_paths4)
//   k_topc_lists : the top-10 of full candidate lists
// Entry points: xmap_path_weights, xmap_extend_paths, xmap_topc_from_lists.
#include "paths.h"

namespace xmap {

__global__ __launch_bounds__(256) void k_topc_lists(int I, const long long *xs_ptr, const int *xs_end, const double *xs_val,
                                                    int *n_cand, int *top_end, double *top_val) {
    int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= I) return;
    long long lo = xs_ptr[s];
    int nt = (int)(xs_ptr[s + 1] - lo);
    select_topc(nt, [&](int b, int &e, double &v) { e = xs_end[lo + b]; v = xs_val[lo + b]; },
                top_end + (size_t)s * XMAP_TOPC, top_val + (size_t)s * XMAP_TOPC);
    if (lane_id() == 0) n_cand[s] = nt;
}

__global__ __launch_bounds__(256) void k_paths(PathArgs A) {
    __shared__ FinBuf fin[4];
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= A.n_slots) return;
    const int lane = lane_id();
    const int k = A.k;
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
        int ent = 0;  // running index of the start's (head, t) entries; unit c takes ent % G == c
        // role T: start = t (final_nonjoint_extend on every SRC record, extender.py:124-140,:180)
        if (A.flags[start] & 2) {
            if (G == 1 || ent % G == c) {
                Carry none; none.sm = 0; none.mu = 0; none.c = 0;
                through_t(A, W, start, false, none);
            }
            ent++;
        }
        // role X': start = x' in attach(t) (target_path, extender.py:160-163)
        if (A.cls[start] == 2) {
            int nb = A.kcnt[(size_t)start * 2];
            for (int q = 0; q < nb; q++) {
                size_t o = ((size_t)start * 2) * k + q;
                int t = A.kcol[o];
                if (!(A.flags[t] & 2)) continue;  // BB_other_intra_target keeps "T:" bridges only (:175)
                if (G == 1 || ent % G == c) {
                    Carry h = first_edge(A.kval[o * 3], A.kval[o * 3 + 1], A.kval[o * 3 + 2]);
                    through_t(A, W, t, true, h);
                }
                ent++;
            }
        }
        // role Y': start = y' in NN(x'), x' in attach(t) (longest_path, extender.py:164-167)
        {
            long long r0 = A.rnn_ptr[start], r1 = A.rnn_ptr[start + 1];
            for (long long rp = r0; rp < r1; rp++) {
                int xp = A.rnn_idx[rp];
                Carry h0 = first_edge(A.rnn_val[rp * 3], A.rnn_val[rp * 3 + 1], A.rnn_val[rp * 3 + 2]);
                int nb = A.kcnt[(size_t)xp * 2];
                for (int q = 0; q < nb; q++) {
                    size_t o = ((size_t)xp * 2) * k + q;
                    int t = A.kcol[o];
                    if (!(A.flags[t] & 2)) continue;
                    if (G == 1 || ent % G == c) {
                        Carry h = add_edge(h0, A.kval[o * 3], A.kval[o * 3 + 1], A.kval[o * 3 + 2]);
                        through_t(A, W, t, true, h);
                    }
                    ent++;
                }
            }
        }
        if (row < 0) cand_total += finalize_start(A, fin[threadIdx.x >> 6], W.acc, W.touched, W.nt, start);
        else if (lane == 0) A.unit_nt[unit] = W.nt;
    }
    if (lane == 0) {
        atomicAdd(&A.counters[0], cand_total);
        atomicAdd(&A.counters[1], W.paths);
    }
}

// ---- per-start path counts (scheduling weights): T(s) tails of s, sums over src(t), heads of x' -------------
__global__ __launch_bounds__(256) void k_w_tails(int I, const long long *att_ptr, const int *att_idx, const int *kcnt,
                                                 long long *T) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= I) return;
    long long a0 = att_ptr[s], a1 = att_ptr[s + 1], t = 0;
    for (long long ap = a0; ap < a1; ap++) t += 1 + kcnt[(size_t)att_idx[ap] * 2 + 1];
    T[s] = (a1 > a0) ? t + 1 : 0;
}
__global__ __launch_bounds__(256) void k_w_src(int I, const long long *src_ptr, const int *src_idx, const uint8_t *src_flag,
                                               const long long *T, long long *ST_all, long long *ST_j) {
    int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= I) return;
    int lane = lane_id();
    long long a = 0, j = 0;
    for (long long p = src_ptr[t] + lane; p < src_ptr[t + 1]; p += 64) {
        long long v = T[src_idx[p]];
        a += v;
        if (src_flag[p] & 1) j += v;
    }
    a = wave_sum_ll(a);
    j = wave_sum_ll(j);
    if (lane == 0) { ST_all[t] = a; ST_j[t] = j; }
}
__global__ __launch_bounds__(256) void k_w_heads(int I, int k, const uint8_t *cls, const int *kcnt, const int *kcol,
                                                 const uint8_t *flags, const long long *ST_j, long long *HX) {
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= I) return;
    long long h = 0;
    if (cls[x] == 2) {
        int nb = kcnt[(size_t)x * 2];
        for (int q = 0; q < nb; q++) {
            int t = kcol[((size_t)x * 2) * k + q];
            if (flags[t] & 2) h += ST_j[t];
        }
    }
    HX[x] = h;
}
__global__ __launch_bounds__(256) void k_w_starts(int I, const uint8_t *flags, const long long *rnn_ptr, const int *rnn_idx,
                                                  const long long *ST_all, const long long *HX, long long *P) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= I) return;
    long long p = ((flags[s] & 2) ? ST_all[s] : 0) + HX[s];
    for (long long rp = rnn_ptr[s]; rp < rnn_ptr[s + 1]; rp++) p += HX[rnn_idx[rp]];
    P[s] = p;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_topc_from_lists(void *stream, int32_t n_items, const int64_t *xs_ptr, const int32_t *xs_end, const double *xs_val,
                         int32_t *n_cand, int32_t *top_end, double *top_val) {
    XM_ARG(xs_ptr && xs_end && xs_val && n_cand && top_end && top_val);
    if (n_items == 0) return XMAP_OK;
    k_topc_lists<<<dim3((unsigned)((n_items + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
        n_items, (const long long *)xs_ptr, xs_end, xs_val, n_cand, top_end, top_val);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

int xmap_path_weights(void *stream, const xmap_ext_tables *T, int64_t *tmp /*[4][I]*/, int64_t *paths /*[I]*/) {
    XM_ARG(T);
    XM_ARG(T->cls && T->kcnt && T->kcol && T->flags && T->att_ptr && T->src_ptr && T->rnn_ptr && tmp && paths);
    const int n_items = T->n_items;
    if (n_items == 0) return XMAP_OK;
    hipStream_t st = (hipStream_t)stream;
    long long *W = (long long *)tmp, *STa = W + n_items, *STj = STa + n_items, *HX = STj + n_items;
    unsigned g1 = (unsigned)((n_items + 255) / 256), g4 = (unsigned)((n_items + 3) / 4);
    k_w_tails<<<dim3(g1), dim3(256), 0, st>>>(n_items, (const long long *)T->att_ptr, T->att_idx, T->kcnt, W);
    XM_LAUNCH_CHECK();
    k_w_src<<<dim3(g4), dim3(256), 0, st>>>(n_items, (const long long *)T->src_ptr, T->src_idx, T->src_flag, W, STa, STj);
    XM_LAUNCH_CHECK();
    k_w_heads<<<dim3(g1), dim3(256), 0, st>>>(n_items, T->top_k, T->cls, T->kcnt, T->kcol, T->flags, STj, HX);
    XM_LAUNCH_CHECK();
    k_w_starts<<<dim3(g1), dim3(256), 0, st>>>(n_items, T->flags, (const long long *)T->rnn_ptr, T->rnn_idx, STa, HX,
                                                (long long *)paths);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

int xmap_extend_paths(void *stream, const xmap_ext_tables *T, const xmap_path_units *U, const xmap_path_rows *R,
                      const xmap_path_out *O, int64_t *d_counters, int64_t *h_counters) {
    return extend_paths_run(stream, T, U, R, O, d_counters, h_counters,
                            [](const PathArgs &A, dim3 grid, hipStream_t st) { k_paths<<<grid, dim3(256), 0, st>>>(A); });
}

}
