// predict_rows.h -- the pair body of the device-resident prediction, shared by k_predict_rows (stage_e_rows.hip: the bounded
// predictions of item_based_prediction) and the scoring pass of the top-N recommendation (stage_e_topn.hip: the same two
// values before bound_rating).  One body with a compile-time switch: the two kernels are the same code.
#pragma once
#include <stdlib.h>
#include "common.h"
#include "rec_model.h"

namespace xmap {

constexpr int PR_CAP = 128;        // evidence entries of a pair staged in LDS (6 KB per wave; 7.5 KB in the explain mode)
constexpr int PR_WAVES = 4;
constexpr int EX_MAX_EV = 16;      // evidence entries an explanation reports per pair
constexpr int EX_MAX_SRC = 8;      // source positions it reports per entry

// Work items (one wave each) of one launch of a wave-per-item kernel.  A grid holds fewer than 2^32 threads, that is fewer than
// 2^26 waves: a call with more items than PAIR_RANGE is launched range by range, the kernel taking the first item of its range
// as a base for the wave index; a call with fewer is the one launch it always was.  15 / 16 of the 2^26: as large as a grid
// may be, less a margin -- the waves of two ranges do not overlap, so every cut costs the tail of one launch (about 1 ms in
// 600 at 5.5e7 pairs when the range was 2^25), and the calls that were one launch before ranges existed stay one.
constexpr long long PAIR_RANGE = 15ll << 22;
static_assert(PAIR_RANGE * 64 < (1ll << 32), "the grid of a range stays below 2^32 threads");

// launch(first item of the range, one past its last item, grid) for the ranges of n_work items, in ascending order;
// `waves` = work items per block; every launch is checked.  XMAP_PAIR_RANGE (tests: several ranges on small inputs) lowers the
// range, read once per call.
template <class Launch>
static int for_pair_ranges(long long n_work, int waves, Launch launch) {
    long long span = PAIR_RANGE;
    if (const char *e = getenv("XMAP_PAIR_RANGE")) {
        const long long v = atoll(e);
        if (v >= 1 && v < span) span = v;
    }
    for (long long base = 0; base < n_work; base += span) {
        const long long end = n_work - base < span ? n_work : base + span;
        launch(base, end, dim3((unsigned)((end - base + waves - 1) / waves)));
        XM_LAUNCH_CHECK();
    }
    return XMAP_OK;
}

// The explain mode's outputs (xmap_explain_rows, stage_e_explain.hip); unused -- and compiled out -- in the other modes.
struct ExplainOut {
    int rank_by, n_ev;
    int *total, *cnt;
    double *score;
    long long *row;
    int *slot;
    double *share;
};

// an explanation's empty tail: entries [from, n_ev) of pair t
__device__ __forceinline__ void explain_blank(const ExplainOut &X, long long t, int from, int lane) {
    if (lane >= from && lane < X.n_ev) {
        const size_t o = (size_t)t * X.n_ev + lane;
        X.row[o] = -1; X.slot[o] = -1; X.share[o] = 0.0;
    }
}

__device__ __forceinline__ double bound_rating_rows(double r) {
    const double x = r + 0.5;       // max(0, min(int(x), 5)): int() truncates towards zero
    return x >= 5.0 ? 5.0 : (x < 1.0 ? 0.0 : (double)(long long)x);
}

template <bool ARENA>
__device__ __forceinline__ void wave_sync() {
    if constexpr (ARENA) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ARENA = false: pair = wave index; a pair with more than PR_CAP evidence entries is appended to ovf_list with an arena
// offset (ovf[0] pairs, ovf[1] entries) and left for the second launch.  ARENA = true: wave w takes (pair, offset) =
// ovf_list[2 w ..] and stages its evidence in arena[6 offset ..].
// RAW = false: item_based_prediction (the bounded predictions, status 1 for an item without a list).  RAW = true: the two values
// as they stand before bound_rating (the scores the top-N selection ranks, stage_e_topn.hip); nothing else differs.
// EXPLAIN = true (with RAW; xmap_explain_rows): the same staging, sums, time ranks and status, and on top of them the
// explanation of the pair -- every entry also stages (profile row as an offset from the user's first, list position), the
// time sort keeps its permutation and the rank of every sorted position, and once the sums stand the share of every entry
// (rank_by 0: e0[q] / p1; 1: (e0[q] * wt_q) / d1, the product the decayed sum adds) overwrites a staging column that is done
// with; n_ev rounds of a wave-wide arg-max by (|share| desc, evidence index asc) report the strongest entries.  The shares are
// what an entry adds to score - item_avg; their rounded sum need not reproduce that difference bit for bit.  The arena slice of
// an entry is 8 doubles instead of 6.  The other instantiations compile none of this.
template <bool ARENA, bool RAW, bool EXPLAIN = false>
__device__ __forceinline__ void predict_pair(
    long long w_base, long long n_work, const int *tu, const int *ti, long long U, int I, int keep, const int *nb_cnt, const int *nb_col,
    const double *nb_sim, const long long *pptr, const int *pitem, const double *prating, const long long *ptime,
    const double *avg, const double *wtab, int n_w, double *out_plain, double *out_decay, int *status, int *max_now,
    unsigned long long *ovf, long long *ovf_list, double *arena, const ExplainOut X = ExplainOut()) {
    static_assert(!EXPLAIN || RAW, "the explanation reports the unrounded score");
    constexpr int COLS = EXPLAIN ? 8 : 6;       // doubles of an arena slice per evidence entry
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const long long w = w_base + (long long)blockIdx.x * PR_WAVES + wv;      // the launch covers the work items [w_base, n_work)
    if (w >= n_work) return;
    const long long t = ARENA ? ovf_list[2 * w] : w;
    const int u = tu[t], it = ti[t];
    int cnt = (it >= 0 && it < I) ? nb_cnt[it] : 0;
    cnt = cnt < keep ? cnt : keep;
    if (cnt <= 0) {       // item without a neighbour list: ()
        if constexpr (EXPLAIN) {
            if (lane == 0) { status[t] = 1; X.total[t] = 0; X.cnt[t] = 0; X.score[t] = 0.0; }
            explain_blank(X, t, 0, lane);
        } else {
            if (lane == 0) { status[t] = 1; out_plain[t] = 0.0; out_decay[t] = 0.0; }
        }
        return;
    }
    const double base = avg[it];
    int nb = -1;
    double s = 0.0, navg = 0.0;
    if (lane < cnt) {
        const size_t o = (size_t)it * keep + lane;
        nb = nb_col[o];
        if (nb < 0 || nb >= I) nb = -1;
        else { s = nb_sim[o]; navg = avg[nb]; }
    }
    long long a = 0, b = 0;
    if (u >= 0 && u < U) { a = pptr[u]; b = pptr[u + 1]; }
    // count pass: rows of the user's profile that hold this lane's neighbour
    int c = 0;
    for (long long p = a; p < b; p += 64) {
        const int pit = (p + lane < b) ? pitem[p + lane] : -2;
        const int lim = (int)min(64ll, b - p);
        for (int j = 0; j < lim; j++) c += (rl32(pit, j) == nb) ? 1 : 0;
    }
    int incl = c;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_up(incl, m, 64);
        if (lane >= m) incl += o;
    }
    const int n = rl32(incl, 63);
    double plain = base, decayed = base;
    bool bad = !isfinite(base);
    [[maybe_unused]] int reported = 0;  // EXPLAIN: entries written to the explanation
    if (n > 0) {
        double *e0, *e1, *s0, *s1;
        long long *tm, *st;
        [[maybe_unused]] int *xr = nullptr, *xs = nullptr, *xq = nullptr;    // EXPLAIN: row offset and list position of entry q; entry at sorted position
        if constexpr (ARENA) {
            double *slice = arena + COLS * (size_t)ovf_list[2 * w + 1];
            e0 = slice; e1 = e0 + n; s0 = e1 + n; s1 = s0 + n;
            tm = (long long *)(s1 + n); st = tm + n;
            if constexpr (EXPLAIN) { xr = (int *)(st + n); xs = xr + n; xq = xs + n; }
        } else {
            if (n > PR_CAP) {
                if (lane == 0) {
                    const unsigned long long slot = atomicAdd(&ovf[0], 1ull);
                    const unsigned long long off = atomicAdd(&ovf[1], (unsigned long long)n);
                    ovf_list[2 * slot] = t; ovf_list[2 * slot + 1] = (long long)off;
                    status[t] = 3;       // pending: the arena launch decides it
                }
                return;
            }
            __shared__ double sh_d[PR_WAVES][4 * PR_CAP];
            __shared__ long long sh_t[PR_WAVES][2 * PR_CAP];
            e0 = sh_d[wv]; e1 = e0 + PR_CAP; s0 = e1 + PR_CAP; s1 = s0 + PR_CAP;
            tm = sh_t[wv]; st = tm + PR_CAP;
            if constexpr (EXPLAIN) {
                __shared__ int sh_x[PR_WAVES][3 * PR_CAP];
                xr = sh_x[wv]; xs = xr + PR_CAP; xq = xs + PR_CAP;
            }
        }
        // fill pass: evidence order = neighbour-list order, within a neighbour the user's rows in profile order
        int k = incl - c;
        for (long long p = a; p < b; p += 64) {
            const bool in = p + lane < b;
            const int pit = in ? pitem[p + lane] : -2;
            const double pr = in ? prating[p + lane] : 0.0;
            const long long pt = in ? ptime[p + lane] : 0;
            const int lim = (int)min(64ll, b - p);
            for (int j = 0; j < lim; j++) {
                const int ji = rl32(pit, j);
                const double jr = rld(pr, j);
                const long long jt = rl64(pt, j);
                if (ji == nb) {
                    e0[k] = s * (jr - navg); e1[k] = fabs(s); tm[k] = jt;
                    if constexpr (EXPLAIN) { xr[k] = (int)(p - a) + j; xs[k] = lane; }
                    k++;
                }
            }
        }
        wave_sync<ARENA>();
        double p0 = 0.0, p1 = 0.0;          // Python's sum(): left to right
        for (int q = 0; q < n; q++) { p0 += e0[q]; p1 += e1[q]; }
        plain = base + p0 / p1;
        // stable order by time: position = entries with a smaller time + earlier entries with the same time
        for (int q = lane; q < n; q += 64) {
            const long long tq = tm[q];
            int pos = 0;
            for (int j = 0; j < n; j++) {
                const long long tj = tm[j];
                pos += (tj < tq || (tj == tq && j < q)) ? 1 : 0;
            }
            s0[pos] = e0[q]; s1[pos] = e1[q]; st[pos] = tq;
            if constexpr (EXPLAIN) xq[pos] = q;
        }
        wave_sync<ARENA>();
        int ranks = 0;                        // distinct times
        [[maybe_unused]] int *xk = (int *)tm; // EXPLAIN: time rank of a sorted position (tm is done with: st holds the sorted times)
        for (int q0 = 0; q0 < n; q0 += 64) {
            const int q = q0 + lane;
            const bool fresh = q < n && (q == 0 || st[q] != st[q - 1]);
            const unsigned long long fm = __ballot(fresh);
            if constexpr (EXPLAIN) {
                if (q < n) xk[q] = ranks + __popcll(fm & (lanemask_lt() | (1ull << lane)));
            }
            ranks += __popcll(fm);
        }
        const int now = ranks + 1;
        if (lane == 0) atomicMax(max_now, now);
        if (now > n_w) bad = true;            // the decay table is too short
        else {
            double d0 = 0.0, d1 = 0.0;
            int r = 0;
            long long prev = 0;
            for (int q = 0; q < n; q++) {
                const long long tq = st[q];
                if (q == 0 || tq != prev) r++;
                prev = tq;
                const double wt = wtab[now - r];
                d0 += s0[q] * wt; d1 += s1[q] * wt;
            }
            decayed = base + d0 / d1;
            // where Python raises (zero weight sum, int() of an infinity or a NaN): status 2
            if (p1 == 0.0 || d1 == 0.0 || !isfinite(plain) || !isfinite(decayed)) bad = true;
            if constexpr (EXPLAIN) {
                if (!bad) {
                    // shares: rank_by 0 over the entries q into e1, rank_by 1 over the sorted positions into s1 (every lane has
                    // read both columns to the end: the sums above); a lane reads back only what it wrote itself
                    wave_sync<ARENA>();
                    double *sh = X.rank_by ? s1 : e1;
                    for (int q = lane; q < n; q += 64)
                        sh[q] = X.rank_by ? (s0[q] * wtab[now - xk[q]]) / d1 : e0[q] / p1;
                    reported = n < X.n_ev ? n : X.n_ev;
                    double ws = 0.0;              // the previous round's winner: this round takes the next key after it
                    int wq = -1;
                    for (int r = 0; r < reported; r++) {
                        double bs = 0.0;
                        int bq = -1;
                        for (int x = lane; x < n; x += 64) {
                            const double cs = sh[x];
                            const int cq = X.rank_by ? xq[x] : x;
                            const double ca = fabs(cs), wa = fabs(ws), ba = fabs(bs);
                            if (wq >= 0 && !(ca < wa || (ca == wa && cq > wq))) continue;
                            if (bq < 0 || ca > ba || (ca == ba && cq < bq)) { bs = cs; bq = cq; }
                        }
#pragma unroll
                        for (int m = 32; m >= 1; m >>= 1) {
                            const double os = __shfl_xor(bs, m, 64);
                            const int oq = __shfl_xor(bq, m, 64);
                            const double oa = fabs(os), ba = fabs(bs);
                            if (oq >= 0 && (bq < 0 || oa > ba || (oa == ba && oq < bq))) { bs = os; bq = oq; }
                        }
                        ws = bs; wq = bq;
                        if (lane == 0) {
                            const size_t o = (size_t)t * X.n_ev + r;
                            X.row[o] = a + xr[wq]; X.slot[o] = xs[wq]; X.share[o] = ws;
                        }
                    }
                }
            }
        }
    }
    if constexpr (EXPLAIN) {
        if (lane == 0) {
            status[t] = bad ? 2 : 0;
            X.total[t] = bad ? 0 : n;
            X.cnt[t] = reported;
            X.score[t] = bad ? 0.0 : (X.rank_by ? decayed : plain);
        }
        explain_blank(X, t, reported, lane);
    } else {
        if (lane == 0) {
            status[t] = bad ? 2 : 0;
            out_plain[t] = bad ? 0.0 : (RAW ? plain : bound_rating_rows(plain));
            out_decay[t] = bad ? 0.0 : (RAW ? decayed : bound_rating_rows(decayed));
        }
    }
}

template <bool ARENA, bool RAW>
__global__ __launch_bounds__(64 * PR_WAVES) void k_predict_rows(
    long long w_base, long long n_work, const int *tu, const int *ti, long long U, int I, int keep, const int *nb_cnt, const int *nb_col,
    const double *nb_sim, const long long *pptr, const int *pitem, const double *prating, const long long *ptime,
    const double *avg, const double *wtab, int n_w, double *out_plain, double *out_decay, int *status, int *max_now,
    unsigned long long *ovf, long long *ovf_list, double *arena) {
    predict_pair<ARENA, RAW>(w_base, n_work, tu, ti, U, I, keep, nb_cnt, nb_col, nb_sim, pptr, pitem, prating, ptime, avg, wtab, n_w, out_plain,
                             out_decay, status, max_now, ovf, ovf_list, arena);
}

// The two launches of a pair kernel over n_test pairs: the wave-per-pair launch, then -- for the pairs whose evidence does not
// fit the LDS staging -- the same kernel over an arena of exactly the entries the first launch counted (arena_cols doubles per
// entry).  Either launch is cut into ranges of PAIR_RANGE work items (for_pair_ranges): launch(arena launch?, grid, first work
// item, one past the last, max_now, ctl, ovf_list, arena) starts the kernel on one range.  The counters, max_now, ovf_list and
// the arena belong to the whole call: every range adds to the same ctl and appends to the same ovf_list, and the arena launch
// reads the list that all ranges wrote.  One host wait per launch (not per range).  *h_max_now (may be NULL) = the largest
// `now` met.  Shared by the prediction, the top-N scores and the explanation.
template <class Launch>
static int pair_rows_run(hipStream_t st, int64_t n_test, int arena_cols, int32_t *h_max_now, Launch launch) {
    XM_SCOPE(st);
    if (h_max_now) *h_max_now = 0;
    if (n_test == 0) return XMAP_OK;
    unsigned long long *ctl = nullptr;          // [0], [1]: overflowed pairs, their evidence entries; [2]: largest `now`
    long long *ovf_list = nullptr;
    XM_HIP(xm_malloc_async((void **)&ctl, sizeof(unsigned long long) * 3, st));
    XM_HIP(xm_malloc_async((void **)&ovf_list, sizeof(long long) * 2 * (size_t)n_test, st));
    XM_HIP(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * 3, st));
    int *max_now = (int *)(ctl + 2);
    int rc = for_pair_ranges((long long)n_test, PR_WAVES, [&](long long base, long long end, dim3 grid) {
        launch(false, grid, base, end, max_now, ctl, ovf_list, (double *)nullptr);
    });
    if (rc) return rc;
    unsigned long long h[3] = {0, 0, 0};
    XM_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h[0] > 0) {       // pairs whose evidence does not fit the LDS staging: the same kernel over an arena of exactly h[1] entries
        double *arena = nullptr;
        XM_HIP(xm_malloc_async((void **)&arena, sizeof(double) * arena_cols * (size_t)h[1], st));
        rc = for_pair_ranges((long long)h[0], PR_WAVES, [&](long long base, long long end, dim3 grid) {
            launch(true, grid, base, end, max_now, ctl, ovf_list, arena);
        });
        if (rc) return rc;
        XM_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
    }
    if (h_max_now) *h_max_now = (int32_t)(h[2] & 0xffffffffull);
    return XMAP_OK;
}

template <bool RAW>
static int predict_rows_run(hipStream_t st, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const RecModel &M,
                            double *out_plain, double *out_decay, int32_t *status, int32_t *h_max_now) {
    return pair_rows_run(st, n_test, 6, h_max_now, [&](bool in_arena, dim3 grid, long long w_base, long long n_work, int *max_now,
                                                       unsigned long long *ctl, long long *ovf_list, double *arena) {
        auto k = in_arena ? k_predict_rows<true, RAW> : k_predict_rows<false, RAW>;
        k<<<grid, dim3(64 * PR_WAVES), 0, st>>>(w_base, n_work, test_user, test_item, M.n_users, M.n_items, M.keep, M.nb_cnt, M.nb_col,
                                                M.nb_sim, (const long long *)M.prof_ptr, M.prof_item, M.prof_rating,
                                                (const long long *)M.prof_time, M.item_avg, M.wtab, M.n_w, out_plain, out_decay, status,
                                                max_now, ctl, ovf_list, arena);
    });
}

}  // namespace xmap
