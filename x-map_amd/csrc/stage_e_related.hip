// stage_e_related.hip -- related items for a basket on the device (DESIGN.md 4 "Related items"): "what goes with these items" --
// the n_top items most related to a SET of items, read off the rows of the RecommenderSim CSR.  No user, no ratings: a cart, an
// anonymous session, "more like this".  For a query (basket) q the records are, for each basket position p in order whose member
// b = b_item[p] is an item of the matrix, each entry e of row b in storage order: (item = col[e], v = fl(b_weight[p] * sim[e]));
// without weights v = sim[e], nothing is multiplied.  An item's score is taken over its records in record order: the sum from 0.0
// left to right, that sum / (double)support, or the largest v (the first occurrence's bits among equals, NaN if any v is one).
// Built as the user-kNN top-N is ("sort, don't hash", sorted_runs.h), one slot = one basket position:
//   k_rf_check   : (rec_filter.h) b_ptr / ex_ptr: [0] == 0, non-decreasing, the first bad position; nothing is read through a table
//                  before it passed
//   k_rl_count   : records per slot = the eligible entries of the member's row (rl_eligible: the mask, the query's exclusion
//                  list) + one MARKER for the member itself unless KEEP_MEMBERS, one wave per slot -> scan
//   k_rl_expand  : one wave per slot of the chunk: the marker, then the row compacted in storage order by ballot / prefix:
//                  key = (q - q0) << item_bits | item, value = the record's index (-1: the marker), v beside it
//   pr_run_tables : (sorted_runs.h, as are the chunk plan pr_plan_chunks and the walk pr_each_chunk) the stable sort -- the records
//                  of one (q, item) stay in position order, then storage order --, the runs, per query of the chunk its first run
//   k_rl_reduce  : one lane per run: a marker in the run = the item is a member: not a candidate (rule 2 without a second walk);
//                  support (markers do not count), min_support, the score left to right, finite, the floor
//   pr_select    : au_select_segment over the runs of a query; position in the segment ascends with the item
// No floating-point atomic, no lock: the bits depend on neither the grid nor the chunking.
#include <vector>

#include "common.h"
#include "au_select.h"
#include "predict_rows.h"
#include "rec_filter.h"
#include "sorted_runs.h"

namespace xmap {

// A record takes 64 B of temporaries: the default chunk (PR_MAX_RECORDS) 268 MB.

// The ONE statement of "a record of item `it` is written for query q" that the count pass and the expansion both call: an item of
// the matrix, allowed by the mask, not in the query's exclusion list ex_id[x0 .. x1).  Every lane of a wave runs the same list.
__device__ __forceinline__ bool rl_eligible(int it, int I, const unsigned int *allow, const int *ex_id, long long x0, long long x1) {
    if (it < 0 || it >= I) return false;
    if (allow && !bit_allowed(allow, it)) return false;
    bool on = true;
    for (long long x = x0; x < x1 && on; x++) on = ex_id[x] != it;
    return on;
}

// slot e = a basket position: its query, the member's row [p0, p1) (empty for a member without a row) and its exclusion list
__device__ __forceinline__ int rl_slot(long long e, long long n_query, const long long *b_ptr, const int *b_item, int I,
                                       const long long *row_ptr, const long long *ex_ptr, long long &q, long long &p0, long long &p1,
                                       long long &x0, long long &x1) {
    q = pr_last_le(b_ptr, 0, n_query, e);       // the last q with b_ptr[q] <= e: the empty baskets in front of it are passed over
    p0 = p1 = x0 = x1 = 0;
    if (ex_ptr) { x0 = ex_ptr[q]; x1 = ex_ptr[q + 1]; }
    const int b = b_item[e];
    if (b < 0 || b >= I) return -1;
    p0 = row_ptr[b]; p1 = row_ptr[b + 1];
    return b;
}

// cnt[e] = the records of slot e, the marker included; n_real += the records without the markers
__global__ __launch_bounds__(256) void k_rl_count(long long base, long long n_slots, long long n_query, const long long *b_ptr,
                                                  const int *b_item, int I, const long long *row_ptr, const int *col, int keep,
                                                  const unsigned int *allow, const long long *ex_ptr, const int *ex_id, int *cnt,
                                                  unsigned long long *n_real) {
    const long long e = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (e >= n_slots) return;                   // (wave-uniform)
    const int lane = lane_id();
    long long q, p0, p1, x0, x1;
    const int b = rl_slot(e, n_query, b_ptr, b_item, I, row_ptr, ex_ptr, q, p0, p1, x0, x1);
    int c = 0;
    for (long long r = p0; r < p1; r += WAVE) {
        const long long p = r + lane;
        const int it = p < p1 ? col[p] : -1;
        c += __popcll(__ballot(rl_eligible(it, I, allow, ex_id, x0, x1)));
    }
    if (lane == 0) {
        cnt[e] = c + ((b >= 0 && !keep) ? 1 : 0);
        if (c) atomicAdd(n_real, (unsigned long long)c);
    }
}

// one wave per slot e of the chunk (slots [e0 + base .. e1)): its records at rec_off[e] - rec0: the marker, then the row compacted
// in storage order
__global__ __launch_bounds__(256) void k_rl_expand(long long e0, long long e1, long long rec0, long long q0, long long n_query,
                                                   const long long *b_ptr, const int *b_item, const double *b_weight, int I,
                                                   const long long *row_ptr, const int *col, const double *sim, int keep,
                                                   const unsigned int *allow, const long long *ex_ptr, const int *ex_id,
                                                   const long long *rec_off, int item_bits, unsigned long long *keys, int *vals,
                                                   double *v) {
    const long long e = e0 + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (e >= e1) return;
    const int lane = lane_id();
    const long long end = rec_off[e + 1] - rec0;
    long long o = rec_off[e] - rec0;
    if (o == end) return;                       // no record
    long long q, p0, p1, x0, x1;
    const int b = rl_slot(e, n_query, b_ptr, b_item, I, row_ptr, ex_ptr, q, p0, p1, x0, x1);
    if (b < 0) return;
    const unsigned long long qk = (unsigned long long)(q - q0) << item_bits;
    if (!keep) {
        if (lane == 0) { keys[o] = qk | (unsigned long long)(unsigned)b; vals[o] = -1; v[o] = 0.0; }
        o++;
    }
    const double w = b_weight ? b_weight[e] : 1.0;
    for (long long r = p0; r < p1; r += WAVE) {
        const long long p = r + lane;
        const int it = p < p1 ? col[p] : -1;
        const bool on = rl_eligible(it, I, allow, ex_id, x0, x1);
        const unsigned long long mask = __ballot(on);
        const long long at = o + __popcll(mask & lanemask_lt());
        if (on && at < end) {                   // (at < end: the count pass saw the same row)
            keys[at] = qk | (unsigned long long)(unsigned)it;
            vals[at] = (int)at;
            v[at] = b_weight ? w * sim[p] : sim[p];
        }
        o += __popcll(mask);
    }
}

// one lane per run, records in sorted (= expansion) order.  cnt: [0] dropped by min_support, [1] non-finite, [2] below the floor
__global__ __launch_bounds__(256) void k_rl_reduce(long long n, const int *vals, const double *v, const long long *run_idx,
                                                   const int *run_start, int how, int min_support, double min_score, int *r_status,
                                                   double *r_score, int *r_support, unsigned long long *cnt) {
    const long long n_runs = run_idx[n];
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_runs; r += step) {
        const int s = run_start[r], e = run_start[r + 1];
        bool member = false, nan = false;
        int sup = 0;
        double sum = 0.0, best = 0.0;
        for (int t = s; t < e; t++) {
            const int k = vals[t];
            if (k < 0) { member = true; continue; }     // the marker: no record
            const double x = v[k];
            sum += x;
            if (x != x) nan = true;
            else if (sup == 0 || x > best) best = x;    // (a NaN in front leaves best unset: the score is NaN then anyway)
            sup++;
        }
        r_support[r] = sup;
        r_score[r] = 0.0;
        if (member) { r_status[r] = PR_NOT_CANDIDATE; continue; }
        if (sup < min_support) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[0], 1ull); continue; }
        const double score = how == XMAP_RELATED_SUM ? sum : how == XMAP_RELATED_MEAN ? sum / (double)sup : best;
        if (nan || !finite_f64(score)) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[1], 1ull); continue; }
        if (score < min_score) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[2], 1ull); continue; }
        r_score[r] = score;
        r_status[r] = 0;
    }
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_related_rows(void *stream, int64_t n_query, const int64_t *b_ptr, const int32_t *b_item, const double *b_weight,
                      int32_t n_items, const int64_t *row_ptr, const int32_t *col, const double *sim, int32_t how, int32_t flags,
                      int32_t n_top, int32_t min_support, int64_t max_records, int32_t *out_cnt, int32_t *out_item, double *out_score,
                      int32_t *out_support, const xmap_rec_filter *F, int64_t *h_stats) {
    // the host checks: before any device work
    XM_ARG(n_top >= 1 && n_top <= AU_MAX_TOP);
    XM_ARG(how == XMAP_RELATED_SUM || how == XMAP_RELATED_MEAN || how == XMAP_RELATED_MAX);
    XM_ARG((flags & ~XMAP_RELATED_KEEP_MEMBERS) == 0);
    XM_ARG(min_support >= 1);
    XM_ARG(n_query >= 0 && n_query <= (1ll << 28) && n_items >= 0 && max_records >= 0);
    XM_ARG(n_query == 0 || (b_ptr && out_cnt && out_item && out_score && out_support));
    XM_ARG(n_query == 0 || n_items == 0 || row_ptr);
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    // ---- the filter (a NaN floor on the host, first), then the two pointer tables on the device: nothing is indexed through one that
    // fails, and no output (h_stats included) is written
    bool filt = false;
    double min_score = 0.0;
    int rc = rf_prepare(st, n_query, F, &filt, &min_score);
    if (rc) return rc;
    if (n_query == 0) {
        if (h_stats) for (int k = 0; k < 6; k++) h_stats[k] = 0;
        return XMAP_OK;
    }
    long long n_slots = 0;
    if ((rc = rf_check_ptr(st, n_query, (const long long *)b_ptr, "xmap_related_rows", "b_ptr", &n_slots))) return rc;
    if (n_slots > 0 && !b_item) {
        set_error("xmap_related_rows: b_ptr lists %lld members, b_item is NULL", n_slots);
        return XMAP_ERR_ARG;
    }
    if (h_stats) for (int k = 0; k < 6; k++) h_stats[k] = 0;
    const unsigned int *allow = filt ? (const unsigned int *)F->allow : nullptr;
    const long long *ex_ptr = filt ? (const long long *)F->ex_ptr : nullptr;
    const int *ex_id = filt ? F->ex_id : nullptr;
    const int I = n_items;
    const int keep = (flags & XMAP_RELATED_KEEP_MEMBERS) ? 1 : 0;
    const size_t nq1 = (size_t)n_query + 1;
    if (n_slots == 0 || I == 0) {               // no member has a row (the matrix arrays may be NULL)
        if ((rc = pr_blank(st, n_query, n_top, out_cnt, out_item, out_score, out_support))) return rc;
        XM_HIP(hipStreamSynchronize(st));
        return XMAP_OK;
    }
    // ---- records per slot (the outputs are first written once the record counts have passed)
    int *rcnt = nullptr;
    long long *rec_off = nullptr, *qrec = nullptr;
    unsigned long long *cnt = nullptr, h[6] = {0, 0, 0, 0, 0, 0};
    XM_HIP(xm_malloc_async((void **)&rcnt, sizeof(int) * (size_t)n_slots, st));
    XM_HIP(xm_malloc_async((void **)&rec_off, sizeof(long long) * ((size_t)n_slots + 1), st));
    XM_HIP(xm_malloc_async((void **)&qrec, sizeof(long long) * nq1, st));
    XM_HIP(xm_malloc_async((void **)&cnt, sizeof(h), st));
    XM_HIP(hipMemsetAsync(cnt, 0, sizeof(h), st));
    rc = for_pair_ranges(n_slots, 4, [&](long long base, long long end, dim3 grid) {
        k_rl_count<<<grid, dim3(256), 0, st>>>(base, end, n_query, (const long long *)b_ptr, b_item, I, (const long long *)row_ptr, col, keep,
                                               allow, ex_ptr, ex_id, rcnt, cnt + 5);
    });
    if (rc) return rc;
    if ((rc = xmap_exclusive_scan_i32_to_i64(st, rcnt, (int64_t *)rec_off, n_slots, nullptr))) return rc;
    k_pr_qrec<<<dim3(blocks_for(n_query + 1, 256)), dim3(256), 0, st>>>(n_query, (const long long *)b_ptr, 0, rec_off, qrec);
    XM_LAUNCH_CHECK();
    RecordChunks C;
    C.rec.resize(nq1);
    std::vector<long long> h_bptr(nq1);
    XM_HIP(hipMemcpyAsync(C.rec.data(), qrec, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(h_bptr.data(), b_ptr, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    // ---- the chunks (the markers count as records), then the first write of the outputs
    if ((rc = pr_plan_chunks("related", n_query, max_records, PR_MAX_RECORDS, &C))) return rc;
    if ((rc = pr_blank(st, n_query, n_top, out_cnt, out_item, out_score, out_support))) return rc;
    if (C.n_max > 0) {
        const int item_bits = bits_for(I);
        const size_t nm = (size_t)C.n_max;
        RunTables T;
        int *r_status = nullptr, *r_support = nullptr;
        double *v = nullptr, *r_score = nullptr;
        if ((rc = pr_alloc_runs(st, C.n_max, C.nq_max, item_bits, true, &T))) return rc;
        XM_HIP(xm_malloc_async((void **)&v, sizeof(double) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_status, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_support, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_score, sizeof(double) * nm, st));
        rc = pr_each_chunk(C, [&](long long q0, long long q1, long long n) {
            const unsigned nb = blocks_for(n, 256);
            const long long e0 = h_bptr[q0];
            int rc = for_pair_ranges(h_bptr[q1] - e0, 4, [&](long long base, long long end, dim3 grid) {   // slots [base, end) of the chunk
                k_rl_expand<<<grid, dim3(256), 0, st>>>(e0 + base, e0 + end, C.rec[q0], q0, n_query, (const long long *)b_ptr, b_item, b_weight,
                                                        I, (const long long *)row_ptr, col, sim, keep, allow, ex_ptr, ex_id, rec_off,
                                                        item_bits, T.keys, T.vals, v);
            });
            if (rc || (rc = pr_run_tables(st, T, n, q1 - q0, item_bits))) return rc;
            k_rl_reduce<<<dim3(nb < 4096u ? nb : 4096u), dim3(256), 0, st>>>(n, T.vals, v, T.run_idx, T.run_start, how, min_support, min_score,
                                                                            r_status, r_score, r_support, cnt);
            XM_LAUNCH_CHECK();
            return pr_select(st, T, q1 - q0, q0, n_top, item_bits, r_status, r_score, r_support, out_cnt, out_item, out_score, out_support, cnt);
        });
        if (rc) return rc;
    }
    XM_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = (int64_t)h[3]; h_stats[1] = (int64_t)h[0]; h_stats[2] = (int64_t)h[1]; h_stats[3] = (int64_t)h[2];
        h_stats[4] = (int64_t)h[4]; h_stats[5] = (int64_t)h[5];
    }
    return XMAP_OK;
}
}
