// stage_e_itemfold.hip -- item fold-in: one row of RecommenderSim for an item that arrived after training (a book that enters
// the catalogue), computed against the resident user-major profiles with the frozen norms.  The mirror of the user fold-in
// (stage_c_foldin.hip): the model stays frozen, no resident list or average changes, and once the row exists as a neighbour
// list (xmap_rec_select with n_items = n_new) and an item average, the prediction, top-N, audience and explain kernels take the
// tables of I + n_new items as they are (DESIGN.md 4 "Item fold-in").
//
// The batch is a CSR of raters per new item (ptr, user, rating).  Entry e of item q, crossed with row p of its rater's profile,
// is one RECORD (q, j = prof_item[p], r0 = rating[e], r1 = prof_rating[p]); entries in batch order, rows in profile order.  Row
// q of the result has one entry per partner j with a record: n = records, inner = hi(sum fl(r0 r1)) as a double-double sum in
// record order, sim = weighted(inner / (nx ny), n, cap), ls = the largest leave-one-out distance (tri.h: the operations of the
// pair kernels' LS variant, tri_pairs.hip).
//
// Sort, don't hash: no lock, no floating-point atomic, every output position from counts and scans.  The batch is cut into
// chunks of consecutive items whose records number at most max_records (a single item above that is a chunk of its own):
// the plan and the walk are sorted_runs.h's (pr_plan_chunks, pr_each_chunk; a "query" there is an item of the batch here).
//   k_if_check   : the batch comes from outside: ptr[0] == 0, ptr non-decreasing, ptr[n_new] == nnz, 0 <= user < n_users
//   k_if_len     : records per entry = the rater's profile length -> xmap_exclusive_scan -> rec_off
//   k_if_expand  : one thread per record of the chunk (its entry and item by bisection): key = (q - q0) << item_bits | j,
//                  value = the record's index in the chunk; the fill pass also keeps (r0, r1) per record
//   pr_sort_runs : (sorted_runs.h) the stable sort -- the records of one (q, j) stay in expansion order --, then 1 where a run of
//                  equal keys starts -> scan = the run's index
//   k_if_rows    : per item of the chunk the index of its first run (pr_first_run: bisection of the sorted keys) -> its row count
//   pr_run_starts / k_if_reduce (fill only): one lane per run walks its records twice -- the double-double sum and sim, then the
//                  leave-one-out maximum -- and writes the entry at row_ptr[q] + (run - first run of q)
//   k_if_stats   : avg and norm of a new item, one wave per item: the lane-strided double-double sums and dd_reduce of
//                  item_stats.h
// The count pass and the fill pass both expand and sort (the second sort).  Nothing depends on max_records: a
// run never crosses an item, and the sums of a run are taken by one lane in record order.
#include <vector>

#include "common.h"
#include "sorted_runs.h"
#include "tri.h"

namespace xmap {

// The default chunk (PR_MAX_RECORDS) takes about 200 MB of temporaries.

__global__ __launch_bounds__(256) void k_if_check(long long n_new, long long nnz, const long long *ptr, const int *user,
                                                  long long n_users, unsigned long long *bad) {
    const long long total = n_new + 1 + nnz;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += step) {
        bool b;
        if (k <= n_new) {
            const long long p = ptr[k];
            b = k == 0 ? p != 0 : p < ptr[k - 1];
            if (k == n_new) b = b || p != nnz;
        } else {
            const int u = user[k - n_new - 1];
            b = u < 0 || (long long)u >= n_users;
        }
        if (b) {                        // (bad input only: no need to spare the atomics)
            atomicAdd(&bad[0], 1ull);
            atomicMin(&bad[1], (unsigned long long)k);
        }
    }
}

__global__ __launch_bounds__(256) void k_if_len(long long nnz, const int *user, const long long *pptr, int *len) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int u = user[e];
    len[e] = (int)(pptr[u + 1] - pptr[u]);
}

__global__ __launch_bounds__(256) void k_if_expand(long long n, long long rec0, long long e0, long long e1, long long q0, long long q1,
                                                   const long long *ptr, const int *user, const double *rating, const long long *pptr,
                                                   const int *pitem, const double *prating, const long long *rec_off, int item_bits,
                                                   unsigned long long *keys, int *vals, double *r0, double *r1) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const long long g = rec0 + t;
    const long long e = pr_last_le(rec_off, e0, e1, g);         // entries without records are passed over
    const long long q = pr_last_le(ptr, q0, q1, e);             // items without entries too
    const long long p = pptr[user[e]] + (g - rec_off[e]);
    const unsigned long long j = (unsigned long long)(unsigned)pitem[p] & ((1ull << item_bits) - 1ull);
    keys[t] = ((unsigned long long)(q - q0) << item_bits) | j;
    vals[t] = (int)t;
    if (r0) { r0[t] = rating[e]; r1[t] = prating[p]; }
}

// first run and row count of every item of the chunk (sorted_runs.h: the bisection of k_pr_first)
__global__ __launch_bounds__(256) void k_if_rows(long long nq, long long n, const unsigned long long *keys, int item_bits,
                                                 const long long *run_idx, long long *first, int *cnt) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nq) return;
    const long long a = pr_first_run(n, keys, item_bits, run_idx, (unsigned long long)x);
    const long long b = pr_first_run(n, keys, item_bits, run_idx, (unsigned long long)x + 1ull);
    first[x] = a;
    if (cnt) cnt[x] = (int)(b - a);
}

// one lane per run, records in sorted (= expansion) order
__global__ __launch_bounds__(256) void k_if_reduce(long long n, const unsigned long long *keys, const int *vals, const double *r0v,
                                                   const double *r1v, const long long *run_idx, const int *run_start,
                                                   const long long *first, int item_bits, long long q0, int n_items,
                                                   const double *item_norm, const double *new_norm, int cap, const long long *row_ptr,
                                                   int *col, double *sim_out, double *ls_out, int *nij) {
    const long long n_runs = run_idx[n];
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_runs; r += step) {
        const int s = run_start[r], e = run_start[r + 1];
        const unsigned long long key = keys[s];
        const long long x = (long long)(key >> item_bits);
        const int j = (int)(key & ((1ull << item_bits) - 1ull));
        const long long q = q0 + x;
        const long long o = row_ptr[q] + (r - first[x]);
        if (o >= row_ptr[q + 1]) continue;         // a row_ptr that is not the count pass's: nothing is written outside the row
        const double nx = new_norm[q];
        const double ny = j < n_items ? item_norm[j] : 0.0;
        const int cnt = e - s;
        double inner = 0.0, lo = 0.0;
        for (int t = s; t < e; t++) {
            const int v = vals[t];
            dd_add(inner, lo, r0v[v] * r1v[v]);
        }
        const double np = nx * ny;
        const double sim = weighted((np != 0.0) ? 1.0 * inner / np : 0.0, cnt, cap);    // NaN != 0: divides, like the reference
        unsigned long long best = 0ull;
        for (int t = s; t < e; t++) {               // leave-one-out variants (recommenderSim.py:98-116), as tri_pairs.hip takes them
            const int v = vals[t];
            const double r0 = r0v[v], r1 = r1v[v];
            const double rest = inner - r0 * r1;
            const double m1 = sqrt((nx * nx - r0 * r0) * (ny * ny));
            const double m2 = sqrt((nx * nx) * (ny * ny - r1 * r1));
            const double d1 = fabs(weighted((m1 != 0.0) ? 1.0 * rest / m1 : 0.0, cnt - 1, cap) - sim);
            const double d2 = fabs(weighted((m2 != 0.0) ? 1.0 * rest / m2 : 0.0, cnt - 1, cap) - sim);
            const unsigned long long k1 = ls_key(d1), k2 = ls_key(d2);
            const unsigned long long k = k1 > k2 ? k1 : k2;
            best = k > best ? k : best;
        }
        col[o] = j; sim_out[o] = sim; ls_out[o] = __longlong_as_double((long long)best); nij[o] = cnt;
    }
}

// one wave per new item: what item_stats.h computes for a resident item (exact sums rounded once; average = sum / entries)
__global__ __launch_bounds__(256) void k_if_stats(long long n_new, const long long *ptr, const double *rating, double *avg, double *norm) {
    const long long q = (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    const bool on = q < n_new;
    const int lane = lane_id();
    long long p0 = 0, p1 = 0;
    if (on) { p0 = ptr[q]; p1 = ptr[q + 1]; }
    double s = 0.0, slo = 0.0, sq = 0.0, sqlo = 0.0;
    for (long long p = p0 + lane; p < p1; p += WAVE) {
        const double r = rating[p];
        dd_add(s, slo, r);
        dd_add(sq, sqlo, r * r);
    }
    dd_reduce<WAVE>(s, slo);
    dd_reduce<WAVE>(sq, sqlo);
    if (on && lane == 0) {
        const double nn = (double)(p1 - p0);
        avg[q] = (p1 > p0) ? 1.0 * s / nn : 0.0;
        norm[q] = sqrt(sq);
    }
}

struct IfBatch {
    long long n_new, nnz;
    const long long *ptr; const int *user; const double *rating;
    long long n_users; int n_items;
    const long long *pptr; const int *pitem; const double *prating;
};

// the chunked expand -> sort -> runs pass.  fill == false: cnt [n_new] (zeroed here) gets the row counts.  fill == true: the
// entries are written (new_norm holds the batch's norms).  *h_records = records of the whole batch.
static int itemfold_pass(hipStream_t st, const IfBatch &B, long long max_records, bool fill, int *cnt, const double *item_norm,
                         const double *new_norm, int cap, const long long *row_ptr, int *col, double *sim, double *ls, int *nij,
                         long long *h_records) {
    XM_SCOPE(st);
    if (h_records) *h_records = 0;
    if (!fill && B.n_new > 0) XM_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)B.n_new, st));
    if (B.n_new == 0 || B.nnz == 0) return XMAP_OK;
    const size_t nz = (size_t)B.nnz, nq1 = (size_t)B.n_new + 1;
    int *len = nullptr;
    long long *rec_off = nullptr, *item_rec = nullptr;
    XM_HIP(xm_malloc_async((void **)&len, sizeof(int) * nz, st));
    XM_HIP(xm_malloc_async((void **)&rec_off, sizeof(long long) * (nz + 1), st));
    XM_HIP(xm_malloc_async((void **)&item_rec, sizeof(long long) * nq1, st));
    k_if_len<<<dim3((unsigned)((B.nnz + 255) / 256)), dim3(256), 0, st>>>(B.nnz, B.user, B.pptr, len);
    XM_LAUNCH_CHECK();
    int rc = xmap_exclusive_scan_i32_to_i64(st, len, (int64_t *)rec_off, B.nnz, nullptr);
    if (rc) return rc;
    k_pr_qrec<<<dim3(blocks_for(B.n_new + 1, 256)), dim3(256), 0, st>>>(B.n_new, B.ptr, 0, rec_off, item_rec);
    XM_LAUNCH_CHECK();
    RecordChunks C;
    C.rec.resize(nq1);
    std::vector<long long> h_ptr(nq1);
    XM_HIP(hipMemcpyAsync(h_ptr.data(), B.ptr, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(C.rec.data(), item_rec, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_records) *h_records = C.rec[B.n_new];
    if ((rc = pr_plan_chunks("item fold-in", B.n_new, max_records, PR_MAX_RECORDS, &C))) return rc;    // a query = an item of the batch
    if (C.n_max == 0) return XMAP_OK;           // no rater has a row: every count is 0
    const int item_bits = bits_for(B.n_items);
    RunTables T;
    double *r0 = nullptr, *r1 = nullptr;
    if ((rc = pr_alloc_runs(st, C.n_max, C.nq_max, item_bits, fill, &T))) return rc;
    if (fill) {
        XM_HIP(xm_malloc_async((void **)&r0, sizeof(double) * T.nm, st));
        XM_HIP(xm_malloc_async((void **)&r1, sizeof(double) * T.nm, st));
    }
    return pr_each_chunk(C, [&](long long q0, long long q1, long long n) {
        const long long nq = q1 - q0;
        const unsigned nb = blocks_for(n, 256);
        k_if_expand<<<dim3(nb), dim3(256), 0, st>>>(n, C.rec[q0], h_ptr[q0], h_ptr[q1], q0, q1, B.ptr, B.user, B.rating, B.pptr, B.pitem,
                                                    B.prating, rec_off, item_bits, T.keys, T.vals, r0, r1);
        XM_LAUNCH_CHECK();
        int rc = pr_sort_runs(st, T, n, nq, item_bits);
        if (rc) return rc;
        k_if_rows<<<dim3(blocks_for(nq, 256)), dim3(256), 0, st>>>(nq, n, T.keys, item_bits, T.run_idx, T.first, fill ? nullptr : cnt + q0);
        XM_LAUNCH_CHECK();
        if (fill) {                             // (the count pass needs neither the run starts nor a reduce)
            if ((rc = pr_run_starts(st, T, n))) return rc;
            k_if_reduce<<<dim3(nb < 4096u ? nb : 4096u), dim3(256), 0, st>>>(n, T.keys, T.vals, r0, r1, T.run_idx, T.run_start, T.first, item_bits,
                                                                            q0, B.n_items, item_norm, new_norm, cap, row_ptr, col, sim, ls, nij);
            XM_LAUNCH_CHECK();
        }
        return XMAP_OK;
    });
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_itemfold_count(void *stream, int64_t n_new, int64_t nnz, const int64_t *ptr, const int32_t *user, int64_t n_users,
                        int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item, int64_t max_records, int32_t *cnt,
                        int64_t *row_ptr, int64_t *h_counts) {
    XM_ARG(n_new >= 0 && nnz >= 0 && nnz < 2147483647ll && n_users >= 0 && n_users <= 2147483647ll && n_items >= 0 && max_records >= 0);
    XM_ARG(ptr && row_ptr && h_counts && prof_ptr && (nnz == 0 || (user && prof_item)) && (n_new == 0 || cnt));
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    // ---- the check: nothing below it runs on a batch that fails, and no output is written
    unsigned long long *bad = nullptr, h_bad[2] = {0, 0};
    XM_HIP(xm_malloc_async((void **)&bad, sizeof(h_bad), st));
    XM_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned long long), st));
    XM_HIP(hipMemsetAsync(bad + 1, 0xff, sizeof(unsigned long long), st));
    const long long total = n_new + 1 + nnz;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    k_if_check<<<dim3(blocks), dim3(256), 0, st>>>(n_new, nnz, (const long long *)ptr, user, n_users, bad);
    XM_LAUNCH_CHECK();
    XM_HIP(hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_bad[0]) {
        const long long k = (long long)h_bad[1];
        if (k <= n_new)
            set_error("item fold-in batch: %llu bad entries, the first at ptr[%lld] (ptr[0] = 0, non-decreasing, ptr[n_new] = nnz)", h_bad[0], k);
        else
            set_error("item fold-in batch: %llu bad entries, the first at user[%lld] (outside [0, %lld))", h_bad[0], k - n_new - 1,
                      (long long)n_users);
        return XMAP_ERR_ARG;
    }
    const IfBatch B{n_new, nnz, (const long long *)ptr, user, nullptr, n_users, n_items, (const long long *)prof_ptr, prof_item, nullptr};
    long long records = 0;
    int rc = itemfold_pass(st, B, max_records, false, cnt, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &records);
    if (rc) return rc;
    int64_t pairs = 0;
    rc = xmap_exclusive_scan_i32_to_i64(st, cnt, row_ptr, n_new, &pairs);       // (syncs)
    if (rc) return rc;
    std::vector<int32_t> h_cnt((size_t)n_new);
    if (n_new) XM_HIP(hipMemcpyAsync(h_cnt.data(), cnt, sizeof(int32_t) * (size_t)n_new, hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    int64_t with = 0;
    for (int64_t q = 0; q < n_new; q++) with += h_cnt[(size_t)q] > 0;
    h_counts[0] = pairs; h_counts[1] = records; h_counts[2] = with;
    XM_HIP(xm_free_async(bad, st));
    return XMAP_OK;
}

int xmap_itemfold_fill(void *stream, int64_t n_new, int64_t nnz, const int64_t *ptr, const int32_t *user, const double *rating,
                       int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                       const double *item_norm, int32_t cap, int64_t max_records, const int64_t *row_ptr, int32_t *col, double *sim,
                       double *ls, int32_t *nij, double *new_avg, double *new_norm) {
    XM_ARG(n_new >= 0 && nnz >= 0 && nnz < 2147483647ll && n_users >= 0 && n_items >= 0 && max_records >= 0 && cap > 0);
    XM_ARG(ptr && row_ptr && prof_ptr);
    if (n_new == 0) return XMAP_OK;
    XM_ARG(new_avg && new_norm && (nnz == 0 || (user && rating && prof_item && prof_rating && item_norm && col && sim && ls && nij)));
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    k_if_stats<<<dim3((unsigned)((n_new + 3) / 4)), dim3(256), 0, st>>>(n_new, (const long long *)ptr, rating, new_avg, new_norm);
    XM_LAUNCH_CHECK();
    const IfBatch B{n_new, nnz, (const long long *)ptr, user, rating, n_users, n_items, (const long long *)prof_ptr, prof_item, prof_rating};
    return itemfold_pass(st, B, max_records, true, nullptr, item_norm, new_norm, cap, (const long long *)row_ptr, col, sim, ls, nij, nullptr);
}
}
