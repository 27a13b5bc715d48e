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
//   radix_sort_pairs : stable, so the records of one (q, item) stay in position order, then storage order
//   k_pr_heads -> scan -> k_pr_starts, k_pr_first : runs, and per query of the chunk its first run
//   k_rl_reduce  : one lane per run: a marker in the run = the item is a member: not a candidate (rule 2 without a second walk);
//                  support (markers do not count), min_support, the score left to right, finite, the floor
//   k_pr_select  : au_select_segment over the runs of a query; position in the segment ascends with the item
// No floating-point atomic, no lock: the bits depend on neither the grid nor the chunking.  (two_pass.h's count_scan_fill fills in
// one pass; here the fill runs chunk by chunk between host decisions, as in stage_e_uknn.hip, so the passes are spelled out.)
#include <vector>

#include "common.h"
#include "au_select.h"
#include "predict_rows.h"
#include "rec_filter.h"
#include "sorted_runs.h"

namespace xmap {

constexpr long long RL_MAX_RECORDS = 1ll << 22;         // the library's default chunk: 4 M records (64 B each: 268 MB of temporaries)

__device__ __forceinline__ bool rl_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for a NaN

// The ONE statement of "a record of item `it` is written for query q" that the count pass and the expansion both call: an item of
// the matrix, allowed by the mask, not in the query's exclusion list ex_id[x0 .. x1).  Every lane of a wave runs the same list.
__device__ __forceinline__ bool rl_eligible(int it, int I, const unsigned int *allow, const int *ex_id, long long x0, long long x1) {
    if (it < 0 || it >= I) return false;
    if (allow && !((allow[it >> 5] >> (it & 31)) & 1u)) return false;
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

// qrec[q] = records in front of query q = rec_off[b_ptr[q]], q <= n_query
__global__ __launch_bounds__(256) void k_rl_qrec(long long n_query, const long long *b_ptr, const long long *rec_off, long long *qrec) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= n_query) qrec[q] = rec_off[b_ptr[q]];
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
        if (nan || !rl_finite(score)) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[1], 1ull); continue; }
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
    const auto blank = [&]() {
        const unsigned bb = pr_blocks((long long)n_query * n_top, 256);
        k_pr_blank<<<dim3(bb < PR_BLANK_BLOCKS ? bb : PR_BLANK_BLOCKS), dim3(256), 0, st>>>(n_query, n_top, out_cnt, out_item, out_score,
                                                                                            out_support);
    };
    if (n_slots == 0 || I == 0) {               // no member has a row (the matrix arrays may be NULL)
        blank();
        XM_LAUNCH_CHECK();
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
    k_rl_qrec<<<dim3(pr_blocks(n_query + 1, 256)), dim3(256), 0, st>>>(n_query, (const long long *)b_ptr, rec_off, qrec);
    XM_LAUNCH_CHECK();
    std::vector<long long> h_rec(nq1), h_bptr(nq1);
    XM_HIP(hipMemcpyAsync(h_rec.data(), qrec, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(h_bptr.data(), b_ptr, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    // ---- chunks of consecutive queries: [q0, q1) with at most max_records records (markers included), or one query
    if (max_records <= 0) max_records = RL_MAX_RECORDS;
    if (max_records > 2147483646ll) max_records = 2147483646ll;    // a chunk of several queries stays below 2^31 - 1 records: only a
                                                                   // single query can reach the capacity error below
    std::vector<long long> cut;
    cut.push_back(0);
    long long n_max = 0, nq_max = 0;
    for (long long q0 = 0; q0 < n_query;) {
        long long q1 = q0 + 1;
        while (q1 < n_query && h_rec[q1 + 1] - h_rec[q0] <= max_records) q1++;
        const long long n = h_rec[q1] - h_rec[q0];
        if (n >= 2147483647ll) {
            set_error("related: query %lld expands to %lld records, a chunk holds fewer than 2^31", q0, n);
            return XMAP_ERR_CAPACITY;
        }
        n_max = n > n_max ? n : n_max;
        nq_max = q1 - q0 > nq_max ? q1 - q0 : nq_max;
        cut.push_back(q1);
        q0 = q1;
    }
    blank();
    XM_LAUNCH_CHECK();
    if (n_max > 0) {
        const int item_bits = pr_bits_for(I);
        XM_ARG(item_bits + pr_bits_for(nq_max) <= 62);
        const size_t nm = (size_t)n_max;
        unsigned long long *keys = nullptr;
        int *vals = nullptr, *head = nullptr, *run_start = nullptr, *r_status = nullptr, *r_support = nullptr;
        long long *run_idx = nullptr, *first = nullptr;
        double *v = nullptr, *r_score = nullptr;
        XM_HIP(xm_malloc_async((void **)&keys, sizeof(unsigned long long) * 2 * nm, st));
        XM_HIP(xm_malloc_async((void **)&vals, sizeof(int) * 2 * nm, st));
        XM_HIP(xm_malloc_async((void **)&v, sizeof(double) * nm, st));
        XM_HIP(xm_malloc_async((void **)&head, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&run_idx, sizeof(long long) * (nm + 1), st));
        XM_HIP(xm_malloc_async((void **)&run_start, sizeof(int) * (nm + 1), st));
        XM_HIP(xm_malloc_async((void **)&first, sizeof(long long) * ((size_t)nq_max + 1), st));
        XM_HIP(xm_malloc_async((void **)&r_status, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_support, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_score, sizeof(double) * nm, st));
        for (size_t k = 0; k + 1 < cut.size(); k++) {
            const long long q0 = cut[k], q1 = cut[k + 1], nq = q1 - q0;
            const long long n = h_rec[q1] - h_rec[q0];
            if (n == 0) continue;               // (the blank outputs stand)
            const unsigned nb = pr_blocks(n, 256);
            const long long e0 = h_bptr[q0];
            rc = for_pair_ranges(h_bptr[q1] - e0, 4, [&](long long base, long long end, dim3 grid) {       // slots [base, end) of the chunk
                k_rl_expand<<<grid, dim3(256), 0, st>>>(e0 + base, e0 + end, h_rec[q0], q0, n_query, (const long long *)b_ptr, b_item, b_weight,
                                                        I, (const long long *)row_ptr, col, sim, keep, allow, ex_ptr, ex_id, rec_off,
                                                        item_bits, keys, vals, v);
            });
            if (rc) return rc;
            if ((rc = radix_sort_pairs(st, keys, vals, keys + nm, vals + nm, n, item_bits + pr_bits_for(nq)))) return rc;
            k_pr_heads<<<dim3(nb), dim3(256), 0, st>>>(n, keys, head);
            XM_LAUNCH_CHECK();
            if ((rc = xmap_exclusive_scan_i32_to_i64(st, head, (int64_t *)run_idx, n, nullptr))) return rc;
            k_pr_starts<<<dim3(nb), dim3(256), 0, st>>>(n, head, run_idx, run_start);
            XM_LAUNCH_CHECK();
            k_pr_first<<<dim3(pr_blocks(nq + 1, 256)), dim3(256), 0, st>>>(nq, n, keys, item_bits, run_idx, first);
            XM_LAUNCH_CHECK();
            k_rl_reduce<<<dim3(nb < 4096u ? nb : 4096u), dim3(256), 0, st>>>(n, vals, v, run_idx, run_start, how, min_support, min_score,
                                                                            r_status, r_score, r_support, cnt);
            XM_LAUNCH_CHECK();
            rc = n_top <= 256 ? pr_select_ranges<256>(st, nq, q0, n_top, first, keys, run_start, item_bits, r_status, r_score, r_support, out_cnt,
                                                      out_item, out_score, out_support, cnt)
                              : pr_select_ranges<1024>(st, nq, q0, n_top, first, keys, run_start, item_bits, r_status, r_score, r_support,
                                                       out_cnt, out_item, out_score, out_support, cnt);
            if (rc) return rc;
        }
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
