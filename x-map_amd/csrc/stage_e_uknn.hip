// stage_e_uknn.hip -- the user-kNN recommender on the device (DESIGN.md 4 "User-kNN"): predictions and top-N lists from the peer
// lists of xmap_peer_rows -- "people like you rated this highly".  The reference's user_based_prediction restated: for a pair
// (query a, item i) the evidence is, for each neighbour v_j of a's list in list order, each row of v_j's profile that holds i, in
// profile order, the entry (s_j, d) with d = rating - avg_a (XMAP_UKNN_OWN_MEAN: rating - avg_v, Resnick's formula);
// pred = avg_a + sum(s d) / sum(|s|), plain fp64 sums taken left to right from 0.0; no evidence: avg_a; no temporal decay.
//   k_uk_means   : one wave per user: the double-double sum of the valid rows (lane-strided, the fixed butterfly of dd_reduce)
//                  rounded once / the count -- as item_stats.h and xmap_peer_centre take an item average
//   k_uk_predict : one wave per test pair; lane j of a tile looks for the item in neighbour j's profile, the wave then visits the
//                  neighbours that hold it in list order, finds their rows by ballot, and every lane runs the same chain
// The top-N (xmap_uknn_topn_rows) is built as the peers are ("sort, don't hash", sorted_runs.h), one slot = (query, list position):
//   k_uk_count   : records per slot = the valid rows of the neighbour (under a mask: of eligible items), one wave per slot -> scan
//   k_uk_expand  : one wave per slot of the chunk compacts its records in profile order: key = (q - q0) << item_bits | item, value =
//                  the record's index, (s_j, d) beside it
//   pr_run_tables : (sorted_runs.h, as are the chunk plan pr_plan_chunks and the walk pr_each_chunk) the stable sort -- the records
//                  of one (q, item) stay in list order, then profile order --, the runs, per query of the chunk its first run
//   k_uk_reduce  : one lane per run: held items, exclusion list, min_support, the two sums left to right, the score, the floor
//   pr_select    : au_select_segment over the runs of a query; position in the segment ascends with the item
// No floating-point atomic anywhere: the bits depend on neither the grid nor the chunking.
#include <vector>

#include "common.h"
#include "au_select.h"
#include "predict_rows.h"
#include "rec_filter.h"
#include "sorted_runs.h"

namespace xmap {

// A record of the top-N takes 72 B of temporaries: the default chunk (PR_MAX_RECORDS) 302 MB.
constexpr int UK_MAX_NB = 1024;

__global__ __launch_bounds__(256) void k_uk_means(long long base, long long U, int I, const long long *pptr, const int *pitem,
                                                  const double *prating, double *avg, int *cnt) {
    const long long u = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    const bool on = u < U;
    const int lane = lane_id();
    long long p0 = 0, p1 = 0;
    if (on) { p0 = pptr[u]; p1 = pptr[u + 1]; }
    double s = 0.0, slo = 0.0;
    long long c = 0;
    for (long long p = p0 + lane; p < p1; p += WAVE) {
        const int it = pitem[p];
        if (it >= 0 && it < I) { dd_add(s, slo, prating[p]); c++; }
    }
    dd_reduce<WAVE>(s, slo);
    c = wave_sum_ll(c);
    if (on && lane == 0) { avg[u] = c > 0 ? 1.0 * s / (double)c : 0.0; cnt[u] = (int)c; }
}

// out[k] = src[sel[k]], 0.0 for an index outside [0, n_src)
__global__ __launch_bounds__(256) void k_uk_gather(long long n, const int *sel, long long n_src, const double *src, double *out) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const long long a = sel[k];
    out[k] = (a >= 0 && a < n_src) ? src[a] : 0.0;
}

__global__ __launch_bounds__(256) void k_uk_predict(long long base, long long n_test, const int *tq, const int *ti, long long n_query,
                                                    const double *qavg, int n_nb, const int *nb_cnt, const int *nb_user, const double *nb_sim,
                                                    long long U, int I, const long long *pptr, const int *pitem, const double *prating,
                                                    const double *uavg, int own, double *o_score, double *o_bound, int *o_n, int *status) {
    const long long t = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (t >= n_test) return;                    // (wave-uniform)
    const int lane = lane_id();
    const long long q = tq[t];
    const int it = ti[t];
    if (q < 0 || q >= n_query || it < 0 || it >= I) {
        if (lane == 0) { status[t] = 3; o_score[t] = 0.0; o_bound[t] = 0.0; o_n[t] = 0; }
        return;
    }
    int cnt = nb_cnt[q];
    cnt = cnt < n_nb ? cnt : n_nb;
    if (cnt <= 0) {                             // no neighbour list: ()
        if (lane == 0) { status[t] = 1; o_score[t] = 0.0; o_bound[t] = 0.0; o_n[t] = 0; }
        return;
    }
    const double a = qavg[q];
    double num = 0.0, den = 0.0;
    int n = 0;
    for (int j0 = 0; j0 < cnt; j0 += WAVE) {
        const int j = j0 + lane;
        int v = -1;
        double s = 0.0;
        long long p0 = 0, p1 = 0;
        bool has = false;
        if (j < cnt) {
            v = nb_user[(size_t)q * n_nb + j];
            s = nb_sim[(size_t)q * n_nb + j];
            if (v >= 0 && v < U) {
                p0 = pptr[v]; p1 = pptr[v + 1];
                for (long long p = p0; p < p1 && !has; p++) has = pitem[p] == it;
            }
        }
        unsigned long long holders = __ballot(has);
        while (holders) {                       // the neighbours that hold the item, in list order
            const int l = __ffsll((long long)holders) - 1;
            holders &= holders - 1;
            const long long b0 = __shfl(p0, l, WAVE), b1 = __shfl(p1, l, WAVE);
            const double sl = __shfl(s, l, WAVE);
            const double m = own ? uavg[__shfl(v, l, WAVE)] : a;
            for (long long b = b0; b < b1; b += WAVE) {
                const long long p = b + lane;
                const bool hit = p < b1 && pitem[p] == it;
                const double r = hit ? prating[p] : 0.0;
                unsigned long long rows = __ballot(hit);
                while (rows) {                  // every lane runs the same chain
                    const int k = __ffsll((long long)rows) - 1;
                    rows &= rows - 1;
                    const double d = __shfl(r, k, WAVE) - m;
                    num += sl * d;
                    den += fabs(sl);
                    n++;
                }
            }
        }
    }
    if (lane != 0) return;
    bool bad = false;
    double pred = a;
    if (n > 0) {
        bad = den == 0.0;                       // ZeroDivisionError
        pred = a + num / den;
    }
    bad = bad || !finite_f64(pred);              // int() of a NaN or an infinity raises
    status[t] = bad ? 2 : 0;
    o_score[t] = bad ? 0.0 : pred;
    o_bound[t] = bad ? 0.0 : bound_rating_rows(pred);
    o_n[t] = n;
}

// the neighbour of slot e = q n_nb + j: its rows [p0, p1), empty for a position behind the list or a user outside [0, U)
__device__ __forceinline__ int uk_slot(long long e, int n_nb, const int *nb_cnt, const int *nb_user, long long U, const long long *pptr,
                                       long long &q, long long &p0, long long &p1) {
    q = e / n_nb;
    const int j = (int)(e - q * n_nb);
    p0 = p1 = 0;
    int cnt = nb_cnt[q];
    cnt = cnt < n_nb ? cnt : n_nb;
    if (j >= cnt) return -1;
    const int v = nb_user[e];
    if (v < 0 || v >= U) return -1;
    p0 = pptr[v]; p1 = pptr[v + 1];
    return v;
}

__global__ __launch_bounds__(256) void k_uk_count(long long base, long long n_slots, int n_nb, const int *nb_cnt, const int *nb_user, long long U,
                                                  int I, const long long *pptr, const int *pitem, const unsigned int *allow, int *cnt) {
    const long long e = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (e >= n_slots) return;
    const int lane = lane_id();
    long long q, p0, p1;
    uk_slot(e, n_nb, nb_cnt, nb_user, U, pptr, q, p0, p1);
    int c = 0;
    for (long long b = p0; b < p1; b += WAVE) {
        const long long p = b + lane;
        const int it = p < p1 ? pitem[p] : -1;
        c += __popcll(__ballot(it >= 0 && it < I && (!allow || bit_allowed(allow, it))));
    }
    if (lane == 0) cnt[e] = c;
}

// one wave per slot e of the chunk (slots [e0 + base .. e1)): its records compacted in profile order at rec_off[e] - rec0
__global__ __launch_bounds__(256) void k_uk_expand(long long e0, long long e1, long long rec0, long long q0, int n_nb, const int *nb_cnt,
                                                   const int *nb_user, const double *nb_sim, const double *qavg, long long U, int I,
                                                   const long long *pptr, const int *pitem, const double *prating, const double *uavg,
                                                   int own, const unsigned int *allow, const long long *rec_off, int item_bits,
                                                   unsigned long long *keys, int *vals, double *sv, double *dv) {
    const long long e = e0 + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (e >= e1) return;
    const int lane = lane_id();
    const long long end = rec_off[e + 1] - rec0;
    long long o = rec_off[e] - rec0;
    if (o == end) return;                       // no record
    long long q, p0, p1;
    const int v = uk_slot(e, n_nb, nb_cnt, nb_user, U, pptr, q, p0, p1);
    if (v < 0) return;
    const double s = nb_sim[e];
    const double m = own ? uavg[v] : qavg[q];
    for (long long b = p0; b < p1; b += WAVE) {
        const long long p = b + lane;
        const int it = p < p1 ? pitem[p] : -1;
        const bool on = it >= 0 && it < I && (!allow || bit_allowed(allow, it));
        const unsigned long long mask = __ballot(on);
        const long long at = o + __popcll(mask & lanemask_lt());
        if (on && at < end) {                   // (at < end: the count pass saw the same rows)
            keys[at] = ((unsigned long long)(q - q0) << item_bits) | (unsigned long long)(unsigned)it;
            vals[at] = (int)at;
            sv[at] = s;
            dv[at] = prating[p] - m;
        }
        o += __popcll(mask);
    }
}

// one lane per run, records in sorted (= expansion) order.  cnt: [0] dropped by min_support, [1] non-finite, [2] below the floor
__global__ __launch_bounds__(256) void k_uk_reduce(long long n, const unsigned long long *keys, const int *vals, const double *sv,
                                                   const double *dv, const long long *run_idx, const int *run_start, int item_bits,
                                                   long long q0, const int *query_user, long long n_q_users, const long long *qptr,
                                                   const int *qitem, int keep_held, const long long *ex_ptr, const int *ex_id,
                                                   int min_support, double min_score, const double *qavg, int *r_status, double *r_score,
                                                   int *r_support, unsigned long long *cnt) {
    const long long n_runs = run_idx[n];
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_runs; r += step) {
        const int s = run_start[r], e = run_start[r + 1];
        const unsigned long long key = keys[s];
        const long long q = q0 + (long long)(key >> item_bits);
        const int it = (int)(key & ((1ull << item_bits) - 1ull));
        const int sup = e - s;
        r_support[r] = sup;
        r_score[r] = 0.0;
        bool out = false;
        if (!keep_held) {
            const long long a = query_user[q];
            if (a >= 0 && a < n_q_users) {
                const long long p1 = qptr[a + 1];
                for (long long p = qptr[a]; p < p1 && !out; p++) out = qitem[p] == it;
            }
        }
        if (!out && ex_ptr) {
            const long long x1 = ex_ptr[q + 1];
            for (long long x = ex_ptr[q]; x < x1 && !out; x++) out = ex_id[x] == it;
        }
        if (out) { r_status[r] = PR_NOT_CANDIDATE; continue; }
        if (sup < min_support) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[0], 1ull); continue; }
        double num = 0.0, den = 0.0;
        for (int t = s; t < e; t++) {
            const int k = vals[t];
            const double sl = sv[k];
            num += sl * dv[k];
            den += fabs(sl);
        }
        const double score = qavg[q] + num / den;       // a zero weight sum: an infinity or a NaN
        if (!finite_f64(score)) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[1], 1ull); continue; }
        if (score < min_score) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[2], 1ull); continue; }
        r_score[r] = score;
        r_status[r] = 0;
    }
}

int uknn_gather(hipStream_t st, long long n, const int *sel, long long n_src, const double *src, double *out) {
    if (n <= 0) return XMAP_OK;
    k_uk_gather<<<dim3(blocks_for(n, 256)), dim3(256), 0, st>>>(n, sel, n_src, src, out);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_uknn_means(void *stream, int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                    const double *prof_rating, double *user_avg, int32_t *user_cnt) {
    XM_ARG(n_users >= 0 && n_users < 2147483647ll && n_items >= 0);
    XM_ARG(n_users == 0 || (prof_ptr && user_avg && user_cnt));
    hipStream_t st = (hipStream_t)stream;
    return for_pair_ranges(n_users, 4, [&](long long base, long long, dim3 grid) {
        k_uk_means<<<grid, dim3(256), 0, st>>>(base, n_users, n_items, (const long long *)prof_ptr, prof_item, prof_rating, user_avg,
                                               user_cnt);
    });
}

int xmap_uknn_predict_rows(void *stream, int64_t n_test, const int32_t *test_q, const int32_t *test_item, int64_t n_query,
                           const double *query_avg, int32_t n_nb, const int32_t *nb_cnt, const int32_t *nb_user, const double *nb_sim,
                           int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                           const double *user_avg, int32_t flags, double *out_score, double *out_bound, int32_t *out_n, int32_t *status) {
    XM_ARG(n_nb >= 1 && n_nb <= UK_MAX_NB);
    XM_ARG((flags & ~XMAP_UKNN_OWN_MEAN) == 0);
    XM_ARG(n_test >= 0 && n_query >= 0 && n_query <= (1ll << 28) && n_users >= 0 && n_users < 2147483647ll && n_items >= 0);
    XM_ARG(n_test == 0 || (test_q && test_item && out_score && out_bound && out_n && status));
    XM_ARG(n_test == 0 || n_query == 0 || (query_avg && nb_cnt && nb_user && nb_sim));
    XM_ARG(n_test == 0 || n_query == 0 || n_users == 0 || (prof_ptr && prof_item && prof_rating));
    XM_ARG(!(flags & XMAP_UKNN_OWN_MEAN) || n_users == 0 || user_avg);
    hipStream_t st = (hipStream_t)stream;
    return for_pair_ranges(n_test, 4, [&](long long base, long long end, dim3 grid) {
        k_uk_predict<<<grid, dim3(256), 0, st>>>(base, end, test_q, test_item, n_query, query_avg, n_nb, nb_cnt, nb_user, nb_sim, n_users,
                                                 n_items, (const long long *)prof_ptr, prof_item, prof_rating, user_avg,
                                                 (flags & XMAP_UKNN_OWN_MEAN) ? 1 : 0, out_score, out_bound, out_n, status);
    });
}

int xmap_uknn_topn_rows(void *stream, int64_t n_query, const int32_t *query_user, int64_t n_q_users, const int64_t *q_ptr,
                        const int32_t *q_item, const double *query_avg, int32_t n_nb, const int32_t *nb_cnt, const int32_t *nb_user,
                        const double *nb_sim, int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                        const double *prof_rating, const double *user_avg, int32_t flags, int32_t n_top, int32_t min_support,
                        int64_t max_records, int32_t *out_cnt, int32_t *out_item, double *out_score, int32_t *out_support,
                        const xmap_rec_filter *F, int64_t *h_stats) {
    // the host checks: before any device work
    XM_ARG(n_top >= 1 && n_top <= AU_MAX_TOP);
    XM_ARG(n_nb >= 1 && n_nb <= UK_MAX_NB);
    XM_ARG(min_support >= 1);
    XM_ARG((flags & ~(XMAP_UKNN_OWN_MEAN | XMAP_UKNN_KEEP_HELD)) == 0);
    XM_ARG(n_query >= 0 && n_query <= (1ll << 28) && n_q_users >= 0 && n_users >= 0 && n_users < 2147483647ll && n_items >= 0 &&
           max_records >= 0);
    XM_ARG(n_query * (int64_t)n_nb < 2147483647ll);
    XM_ARG(n_query == 0 || (query_avg && nb_cnt && nb_user && nb_sim && out_cnt && out_item && out_score && out_support));
    XM_ARG(n_query == 0 || (flags & XMAP_UKNN_KEEP_HELD) || (query_user && (n_q_users == 0 || (q_ptr && q_item))));
    XM_ARG(n_query == 0 || n_users == 0 || n_items == 0 || (prof_ptr && prof_item && prof_rating));
    XM_ARG(!(flags & XMAP_UKNN_OWN_MEAN) || n_users == 0 || user_avg);
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    if (h_stats) for (int k = 0; k < 6; k++) h_stats[k] = 0;
    bool filt = false;
    double min_score = 0.0;
    int rc = rf_prepare(st, n_query, F, &filt, &min_score);     // a NaN floor; ex_ptr, on the device
    if (rc) return rc;
    if (n_query == 0) return XMAP_OK;
    const unsigned int *allow = filt ? (const unsigned int *)F->allow : nullptr;
    const long long *ex_ptr = filt ? (const long long *)F->ex_ptr : nullptr;
    const int *ex_id = filt ? F->ex_id : nullptr;
    const int I = n_items;
    const int own = (flags & XMAP_UKNN_OWN_MEAN) ? 1 : 0, keep_held = (flags & XMAP_UKNN_KEEP_HELD) ? 1 : 0;
    const size_t nq1 = (size_t)n_query + 1;
    const long long n_slots = n_query * (long long)n_nb;
    if (n_users == 0 || I == 0) {                 // no neighbour has a valid row (the profile arrays may be NULL)
        if ((rc = pr_blank(st, n_query, n_top, out_cnt, out_item, out_score, out_support))) return rc;
        XM_HIP(hipStreamSynchronize(st));
        return XMAP_OK;
    }
    // ---- records per slot (the outputs are first written once the record counts have passed)
    int *rcnt = nullptr;
    long long *rec_off = nullptr, *qrec = nullptr;
    XM_HIP(xm_malloc_async((void **)&rcnt, sizeof(int) * (size_t)n_slots, st));
    XM_HIP(xm_malloc_async((void **)&rec_off, sizeof(long long) * ((size_t)n_slots + 1), st));
    XM_HIP(xm_malloc_async((void **)&qrec, sizeof(long long) * nq1, st));
    rc = for_pair_ranges(n_slots, 4, [&](long long base, long long end, dim3 grid) {
        k_uk_count<<<grid, dim3(256), 0, st>>>(base, end, n_nb, nb_cnt, nb_user, n_users, I, (const long long *)prof_ptr, prof_item, allow,
                                               rcnt);
    });
    if (rc) return rc;
    if ((rc = xmap_exclusive_scan_i32_to_i64(st, rcnt, (int64_t *)rec_off, n_slots, nullptr))) return rc;
    k_pr_qrec<<<dim3(blocks_for(n_query + 1, 256)), dim3(256), 0, st>>>(n_query, nullptr, n_nb, rec_off, qrec);
    XM_LAUNCH_CHECK();
    RecordChunks C;
    C.rec.resize(nq1);
    XM_HIP(hipMemcpyAsync(C.rec.data(), qrec, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    // ---- the chunks, then the first write of the outputs
    if ((rc = pr_plan_chunks("user-kNN", n_query, max_records, PR_MAX_RECORDS, &C))) return rc;
    if ((rc = pr_blank(st, n_query, n_top, out_cnt, out_item, out_score, out_support))) return rc;
    unsigned long long *cnt = nullptr, h[5] = {0, 0, 0, 0, 0};
    XM_HIP(xm_malloc_async((void **)&cnt, sizeof(h), st));
    XM_HIP(hipMemsetAsync(cnt, 0, sizeof(h), st));
    if (C.n_max > 0) {
        const int item_bits = bits_for(I);
        const size_t nm = (size_t)C.n_max;
        RunTables T;
        int *r_status = nullptr, *r_support = nullptr;
        double *sv = nullptr, *dv = nullptr, *r_score = nullptr;
        if ((rc = pr_alloc_runs(st, C.n_max, C.nq_max, item_bits, true, &T))) return rc;
        XM_HIP(xm_malloc_async((void **)&sv, sizeof(double) * nm, st));
        XM_HIP(xm_malloc_async((void **)&dv, sizeof(double) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_status, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_support, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_score, sizeof(double) * nm, st));
        rc = pr_each_chunk(C, [&](long long q0, long long q1, long long n) {
            const unsigned nb = blocks_for(n, 256);
            const long long e0 = q0 * n_nb;
            int rc = for_pair_ranges((q1 - q0) * n_nb, 4, [&](long long base, long long end, dim3 grid) {  // slots [base, end) of the chunk
                k_uk_expand<<<grid, dim3(256), 0, st>>>(e0 + base, e0 + end, C.rec[q0], q0, n_nb, nb_cnt, nb_user, nb_sim, query_avg, n_users, I,
                                                        (const long long *)prof_ptr, prof_item, prof_rating, user_avg, own, allow, rec_off,
                                                        item_bits, T.keys, T.vals, sv, dv);
            });
            if (rc || (rc = pr_run_tables(st, T, n, q1 - q0, item_bits))) return rc;
            k_uk_reduce<<<dim3(nb < 4096u ? nb : 4096u), dim3(256), 0, st>>>(n, T.keys, T.vals, sv, dv, T.run_idx, T.run_start, item_bits, q0,
                                                                            query_user, n_q_users, (const long long *)q_ptr, q_item, keep_held,
                                                                            ex_ptr, ex_id, min_support, min_score, query_avg, r_status, r_score,
                                                                            r_support, cnt);
            XM_LAUNCH_CHECK();
            return pr_select(st, T, q1 - q0, q0, n_top, item_bits, r_status, r_score, r_support, out_cnt, out_item, out_score, out_support, cnt);
        });
        if (rc) return rc;
    }
    XM_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = (int64_t)h[3]; h_stats[1] = (int64_t)h[0]; h_stats[2] = (int64_t)h[1]; h_stats[3] = (int64_t)h[2];
        h_stats[4] = (int64_t)h[4]; h_stats[5] = C.rec[(size_t)n_query];
    }
    return XMAP_OK;
}
}
