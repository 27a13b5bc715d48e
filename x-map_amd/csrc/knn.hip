// knn.hip -- stage B, first steps: bridge items and the classified top-k lists (extender_pipeline, reference
// utils/assist.py:80-133; core/extender.py:16-44).  DESIGN.md section "Stage B".
//
// Kernels:
//   k_bridge_flags   : bb[i] = any kept pair of row i whose 2-char prefixes differ        (HBM-bound, one pass over D')
//   k_knn_classify   : per row, chunked bitonic sort in LDS by (|sim| desc, col asc) and the two
//                      filtered top-k lists of find_knn_items                              (HBM-bound, one pass over D')
//   k_knn_thresholds : the last entry of every list as one 16-byte record (KnnThr, paths.h) for the reverse lists
// Entry points: xmap_bridge_flags, xmap_knn_classify, xmap_knn_thresholds.
#include "paths.h"

namespace xmap {

// =============================================================================================
__global__ __launch_bounds__(256) void k_bridge_flags(int I, const long long *row_ptr, const int *col,
                                                      const int *prefix_cls, uint8_t *bb) {
    int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= I) return;
    int lane = lane_id();
    long long lo = row_ptr[i], hi = row_ptr[i + 1];
    int pi = prefix_cls[i];
    int found = 0;
    for (long long b = lo; b < hi && !found; b += 64) {
        long long p = b + lane;
        int f = (p < hi) && (prefix_cls[col[p]] != pi);
        found = __ballot(f) != 0ull;
    }
    if (lane == 0) bb[i] = (uint8_t)found;
}

// =============================================================================================
constexpr int K_THREADS = 256;
constexpr int K_CH = 2048;  // entries sorted per chunk (32 KB of LDS)
constexpr int K_CH_SMALL = 512;   // rows up to this length: the 8 KB instance of k_knn_classify
constexpr int K_WIN = 1024;  // entries streamed against the thresholds per step (rows longer than one chunk)

__device__ __forceinline__ bool before(unsigned long long ka, int ca, unsigned long long kb, int cb) {
    return (ka > kb) || (ka == kb && ca < cb);
}

// exclusive scan of one long long per thread across the block (256 threads)
__device__ __forceinline__ long long block_scan_ll(long long v, long long *total, long long *smem) {
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) smem[w] = inc;
    __syncthreads();
    long long base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < K_THREADS / 64; k++) {
        long long s = smem[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

struct KnnArgs {
    int I, k, row_lo;
    const long long *row_ptr;
    const int *col;
    const double *sim;
    const int *mutu;
    const int *nij;
    const double *info;
    const double *frac;
    const uint8_t *bb;
    const int *suffix_cls;
    const uint32_t *contains_mask;
    uint8_t *cls;
    int *kcnt;
    int *kcol;
    double *kval;
};

// CH = entries sorted per chunk = the block's LDS (16 B each).  Two instances share the rows: rows of at most CH_SMALL
// entries (nearly all of them) run with 8 KB of LDS -- eight blocks per CU instead of five: a block is a chain of dependent
// gathers (row, class predicates, list values), and more blocks in flight is what hides them --, the long rows with 32 KB.
template <int CH, int MODE>      // MODE 0: every row; 1: rows of at most CH entries; 2: rows of more than K_CH_SMALL
__global__ __launch_bounds__(K_THREADS) void k_knn_classify(KnnArgs A) {
    __shared__ unsigned long long skey[CH];
    __shared__ int scol[CH];
    __shared__ int spos[CH];
    __shared__ long long sscan[4];
    __shared__ unsigned long long s_thrk[2];
    __shared__ int s_thrc[2], s_has[2], s_fill;

    const int i = blockIdx.x + A.row_lo;
    const int tid = threadIdx.x;
    const long long lo = A.row_ptr[i];
    const int n = (int)(A.row_ptr[i + 1] - lo);
    if ((MODE == 1 && n > CH) || (MODE == 2 && n <= K_CH_SMALL)) return;      // (the other instance's row)
    const int k = A.k;
    // the unused tail of a list is zero (the tables come uninitialised: a fill of the ~1 GB they take at k = 50 cost
    // more than the lists of the few short rows)
    auto zero_tail = [&](int nA, int nB) {
        for (int e = tid; e < 2 * k; e += K_THREADS) {
            const int l = e >= k, r = e - l * k;
            if (r < (l ? nB : nA)) continue;
            const size_t o = ((size_t)i * 2 + l) * k + r;
            A.kcol[o] = 0; A.kval[o * 3] = 0.0; A.kval[o * 3 + 1] = 0.0; A.kval[o * 3 + 2] = 0.0;
        }
    };
    if (n == 0) {
        if (tid == 0) {
            A.cls[i] = 0;
            A.kcnt[(size_t)i * 2] = 0;
            A.kcnt[(size_t)i * 2 + 1] = 0;
        }
        zero_tail(0, 0);
        return;
    }
    const bool isbb = A.bb[i] != 0;
    const int sc = A.suffix_cls[i];
    if (tid < 2) s_has[tid] = 0;
    int nc = 0, consumed = 0;
    for (;;) {
        int total;
        if (consumed == 0 || CH - nc < K_WIN) {
            const int take = (CH - nc) < (n - consumed) ? (CH - nc) : (n - consumed);
            for (int t = tid; t < take; t += K_THREADS) {
                int p = consumed + t;
                double s = A.sim[lo + p];
                skey[nc + t] = (unsigned long long)__double_as_longlong(fabs(s));
                scol[nc + t] = A.col[lo + p];
                spos[nc + t] = p;
            }
            total = nc + take;
            consumed += take;
        } else {
            // Rows longer than one chunk (the popular items: 1e5 entries and more): after the first sort the k-th best of
            // each list is known, and an entry that does not sort before it can never enter that list -- the rest of the
            // row is streamed against the two thresholds, K_WIN entries per step, and only the survivors are buffered
            // (a few hundred for 1e5 entries in random order) instead of sorting every 2048 of them.
            if (tid == 0) s_fill = nc;
            __syncthreads();
            for (;;) {
                const int f = s_fill;      // the same value for every thread: nobody is past the barrier below yet
                __syncthreads();
                if (consumed >= n || CH - f < K_WIN) break;
#pragma unroll
                for (int u = 0; u < K_WIN / K_THREADS; u++) {
                    const int p = consumed + tid + K_THREADS * u;
                    if (p < n) {
                        const unsigned long long key = (unsigned long long)__double_as_longlong(fabs(A.sim[lo + p]));
                        const int c = A.col[lo + p];
                        bool pa, pb;
                        if (isbb) {
                            bool has = (A.contains_mask[c] >> sc) & 1u;
                            pa = !has; pb = has;
                        } else {
                            pa = A.bb[c] != 0; pb = true;
                        }
                        const bool keep = (pa && (!s_has[0] || before(key, c, s_thrk[0], s_thrc[0]))) ||
                                          (pb && (!s_has[1] || before(key, c, s_thrk[1], s_thrc[1])));
                        if (keep) {
                            const int o = atomicAdd(&s_fill, 1);
                            skey[o] = key; scol[o] = c; spos[o] = p;
                        }
                    }
                }
                consumed = (consumed + K_WIN) < n ? (consumed + K_WIN) : n;
                __syncthreads();
            }
            total = s_fill;
        }
        int N = 2;
        while (N < total) N <<= 1;
        for (int t = total + tid; t < N; t += K_THREADS) {
            skey[t] = 0ull;
            scol[t] = 0x7fffffff;
            spos[t] = -1;
        }
        __syncthreads();
        // bitonic sort by (|sim| desc, col asc); pads (|sim| = 0) end up last.
        // Up to 128 entries (two thirds of the rows): ONE wave runs the whole network -- 64 compare-exchanges per step, the
        // LDS operations of a wave execute in order, so the 28 steps need no block barrier (a barrier per step, 36 of them
        // for 256 entries, was most of a short row's time: 400 000 blocks x ~17 us).
        if (N <= 128) {
            if (tid < 64) {
                for (int k2 = 2; k2 <= N; k2 <<= 1) {
                    for (int j = k2 >> 1; j > 0; j >>= 1) {
                        const int t = tid;
                        if (t < (N >> 1)) {
                            int a = 2 * t - (t & (j - 1));
                            int b = a + j;
                            bool up = (a & k2) == 0;
                            unsigned long long ka = skey[a], kb = skey[b];
                            int ca = scol[a], cb = scol[b];
                            bool sw = up ? before(kb, cb, ka, ca) : before(ka, ca, kb, cb);
                            if (sw) {
                                skey[a] = kb; skey[b] = ka;
                                scol[a] = cb; scol[b] = ca;
                                int pa = spos[a], pb = spos[b];
                                spos[a] = pb; spos[b] = pa;
                            }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    }
                }
            }
            __syncthreads();
        } else
        for (int k2 = 2; k2 <= N; k2 <<= 1) {
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (N >> 1); t += K_THREADS) {
                    int a = 2 * t - (t & (j - 1));
                    int b = a + j;
                    bool up = (a & k2) == 0;
                    unsigned long long ka = skey[a], kb = skey[b];
                    int ca = scol[a], cb = scol[b];
                    bool sw = up ? before(kb, cb, ka, ca) : before(ka, ca, kb, cb);
                    if (sw) {
                        skey[a] = kb; skey[b] = ka;
                        scol[a] = cb; scol[b] = ca;
                        int pa = spos[a], pb = spos[b];
                        spos[a] = pb; spos[b] = pa;
                    }
                }
                __syncthreads();
            }
        }
        // class predicates, ranks in sorted order
        const int per = (N + K_THREADS - 1) / K_THREADS;
        const int s0 = tid * per;
        int cA = 0, cB = 0;
        for (int t = s0; t < s0 + per && t < total; t++) {
            int c = scol[t];
            bool pa, pb;
            if (isbb) {
                bool has = (A.contains_mask[c] >> sc) & 1u;  // domain_label in pair[0]
                pa = !has; pb = has;
            } else {
                pa = A.bb[c] != 0; pb = true;                 // NB_NN keeps every neighbour
            }
            cA += pa; cB += pb;
        }
        long long tot;
        long long ex = block_scan_ll(((long long)cB << 32) | (unsigned)cA, &tot, sscan);
        int rA = (int)(ex & 0xffffffffll), rB = (int)(ex >> 32);
        const int totA = (int)(tot & 0xffffffffll), totB = (int)(tot >> 32);
        const bool last = consumed >= n;
        if (last) {
            for (int t = s0; t < s0 + per && t < total; t++) {
                int c = scol[t];
                bool pa, pb;
                if (isbb) {
                    bool has = (A.contains_mask[c] >> sc) & 1u;
                    pa = !has; pb = has;
                } else {
                    pa = A.bb[c] != 0; pb = true;
                }
                long long p = lo + spos[t];
                if ((pa && rA < k) || (pb && rB < k)) {
                    double sv = A.sim[p];
                    double mu = (double)A.mutu[p];
                    double fr = A.frac ? A.frac[p]
                                       : 1.0 * mu / (A.info[(size_t)i * 4 + 3] + A.info[(size_t)c * 4 + 3] - (double)A.nij[p]);
                    if (pa && rA < k) {
                        size_t o = ((size_t)i * 2 + 0) * k + rA;
                        A.kcol[o] = c; A.kval[o * 3] = sv; A.kval[o * 3 + 1] = mu; A.kval[o * 3 + 2] = fr;
                    }
                    if (pb && rB < k) {
                        size_t o = ((size_t)i * 2 + 1) * k + rB;
                        A.kcol[o] = c; A.kval[o * 3] = sv; A.kval[o * 3 + 1] = mu; A.kval[o * 3 + 2] = fr;
                    }
                }
                rA += pa; rB += pb;
            }
            if (tid == 0) {
                int nA = totA < k ? totA : k, nB = totB < k ? totB : k;
                uint8_t c = isbb ? 1 : (nA > 0 ? 2 : 0);  // no bridge neighbour -> dropped (extender.py:39)
                A.cls[i] = c;
                A.kcnt[(size_t)i * 2] = c ? nA : 0;
                A.kcnt[(size_t)i * 2 + 1] = c ? nB : 0;
            }
            zero_tail(totA < k ? totA : k, totB < k ? totB : k);
            return;
        }
        // carry the selected <= 2k entries to the front (sorted order kept), then take the next chunk
        unsigned long long rk[CH / K_THREADS];
        int rc[CH / K_THREADS], rp[CH / K_THREADS];
        int nk = 0;
        for (int t = s0; t < s0 + per && t < total; t++) {
            int c = scol[t];
            bool pa, pb;
            if (isbb) {
                bool has = (A.contains_mask[c] >> sc) & 1u;
                pa = !has; pb = has;
            } else {
                pa = A.bb[c] != 0; pb = true;
            }
            if ((pa && rA < k) || (pb && rB < k)) { rk[nk] = skey[t]; rc[nk] = c; rp[nk] = spos[t]; nk++; }
            if (pa && rA == k - 1) { s_thrk[0] = skey[t]; s_thrc[0] = c; s_has[0] = 1; }     // the k-th best of a list
            if (pb && rB == k - 1) { s_thrk[1] = skey[t]; s_thrc[1] = c; s_has[1] = 1; }
            rA += pa; rB += pb;
        }
        long long tk;
        long long ek = block_scan_ll((long long)nk, &tk, sscan);
        for (int q = 0; q < nk; q++) {
            skey[ek + q] = rk[q]; scol[ek + q] = rc[q]; spos[ek + q] = rp[q];
        }
        nc = (int)tk;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_knn_thresholds(int I, int k, const int *kcnt, const int *kcol, const double *kval, KnnThr *thr) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2ll * I) return;
    KnnThr th;
    th.cnt = kcnt[t]; th.col = 0; th.la = 0.0;
    if (th.cnt > 0) {
        const size_t o = (size_t)t * k + (th.cnt - 1);
        th.la = fabs(kval[o * 3]); th.col = kcol[o];
    }
    thr[t] = th;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_bridge_flags(void *stream, const xmap_sim *S, const int32_t *prefix_cls, uint8_t *bb) {
    XM_ARG(S && prefix_cls && bb);
    if (S->n_items == 0) return XMAP_OK;
    k_bridge_flags<<<dim3((unsigned)((S->n_items + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
        S->n_items, (const long long *)S->row_ptr, S->col, prefix_cls, bb);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

int xmap_knn_classify(void *stream, const xmap_sim *S, int top_k, const uint8_t *bb, const int32_t *suffix_cls,
                      const uint32_t *contains_mask, uint8_t *cls, int32_t *kcnt, int32_t *kcol, double *kval,
                      int32_t row_lo, int32_t row_hi) {
    XM_ARG(S && bb && suffix_cls && contains_mask && cls && kcnt && kcol && kval);
    XM_ARG(top_k >= 1 && 2 * top_k <= K_CH / 2);
    XM_ARG(row_lo >= 0 && row_lo <= row_hi && row_hi <= S->n_items);
    if (row_hi == row_lo) return XMAP_OK;
    KnnArgs A;
    A.I = S->n_items; A.k = top_k; A.row_lo = row_lo;
    A.row_ptr = (const long long *)S->row_ptr; A.col = S->col; A.sim = S->sim; A.mutu = S->mutu; A.nij = S->nij;
    A.info = S->info; A.frac = S->frac; A.bb = bb; A.suffix_cls = suffix_cls; A.contains_mask = contains_mask;
    A.cls = cls; A.kcnt = kcnt; A.kcol = kcol; A.kval = kval;
    if (2 * top_k <= K_CH_SMALL / 2) {
        k_knn_classify<K_CH_SMALL, 1><<<dim3((unsigned)(row_hi - row_lo)), dim3(K_THREADS), 0, (hipStream_t)stream>>>(A);
        XM_LAUNCH_CHECK();
        k_knn_classify<K_CH, 2><<<dim3((unsigned)(row_hi - row_lo)), dim3(K_THREADS), 0, (hipStream_t)stream>>>(A);
    } else {      // (lists too long for the small instance's carry-over: every row on the large one)
        k_knn_classify<K_CH, 0><<<dim3((unsigned)(row_hi - row_lo)), dim3(K_THREADS), 0, (hipStream_t)stream>>>(A);
    }
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

int xmap_knn_thresholds(void *stream, int32_t n_items, int top_k, const int32_t *kcnt, const int32_t *kcol, const double *kval,
                        void *thr) {
    XM_ARG(kcnt && kcol && kval && thr);
    if (n_items == 0) return XMAP_OK;
    k_knn_thresholds<<<dim3((unsigned)((2ll * n_items + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        n_items, top_k, kcnt, kcol, kval, (KnnThr *)thr);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

}
