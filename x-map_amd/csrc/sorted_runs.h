// sorted_runs.h -- the back half of "sort, don't hash" that the peers (stage_e_peers.hip), the user-kNN top-N (stage_e_uknn.hip),
// the item fold-in (stage_e_itemfold.hip), the related items (stage_e_related.hip), the sorted-runs route of the fused lists
// (stage_e_fuse.hip) and the shelves (stage_e_shelf.hip) share.  The kernels: over the records of a chunk of queries, stably sorted
// on (q - q0) << id_bits | id, the run heads, the run starts, the first run of every query, and the segmented selection
// (au_select.h) over the runs of a query with its outputs (count, id, score, size of the run).  The host half (below the kernels):
// the records in front of each query (k_pr_qrec), the chunk plan (pr_plan_chunks: pure host code), the walk over the chunks
// (pr_each_chunk), the run tables and the launches that fill them (pr_alloc_runs, pr_run_tables = pr_sort_runs + pr_run_starts +
// k_pr_first), the selection (pr_select) and the blank outputs (pr_blank).  A caller keeps its own count, expand and reduce
// kernels: what a record is and what a run is worth -- its status and score -- is the caller's.
#ifndef XMAP_SORTED_RUNS_H
#define XMAP_SORTED_RUNS_H
#include <vector>

#include "common.h"
#include "au_select.h"

namespace xmap {

constexpr int PR_NOT_CANDIDATE = 1, PR_DROPPED = 2;     // status of a run (0: scored and kept)

// the last k in [lo, hi) with a[k] <= x (a non-decreasing, a[lo] <= x)
__device__ __forceinline__ long long pr_last_le(const long long *a, long long lo, long long hi, long long x) {
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

static __global__ __launch_bounds__(256) void k_pr_heads(long long n, const unsigned long long *keys, int *head) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) head[t] = (t == 0 || keys[t] != keys[t - 1]) ? 1 : 0;
}

static __global__ __launch_bounds__(256) void k_pr_starts(long long n, const int *head, const long long *run_idx, int *run_start) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    if (head[t]) run_start[run_idx[t]] = (int)t;
    if (t == 0) run_start[run_idx[n]] = (int)n;
}

// index of the first run of local query x: run_idx at the first sorted position in [0, n] whose query is >= x (run_idx[n] = all runs)
__device__ __forceinline__ long long pr_first_run(long long n, const unsigned long long *keys, int id_bits, const long long *run_idx,
                                                  unsigned long long x) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((keys[mid] >> id_bits) >= x) hi = mid; else lo = mid + 1;
    }
    return run_idx[lo];
}

// first[x] = index of the first run of local query x, x <= nq
static __global__ __launch_bounds__(256) void k_pr_first(long long nq, long long n, const unsigned long long *keys, int id_bits,
                                                         const long long *run_idx, long long *first) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x > nq) return;
    first[x] = pr_first_run(n, keys, id_bits, run_idx, (unsigned long long)x);
}

// qrec[q] = records in front of query q = rec_off[the first slot of q], q <= n_query; the first slot is slot_ptr[q], or q * stride
// where every query has `stride` slots (slot_ptr NULL)
static __global__ __launch_bounds__(256) void k_pr_qrec(long long n_query, const long long *slot_ptr, long long stride,
                                                        const long long *rec_off, long long *qrec) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= n_query) qrec[q] = rec_off[slot_ptr ? slot_ptr[q] : q * stride];
}

// one block per query of the chunk: its runs are the segment [first[x], first[x + 1]), in ascending id
// cnt: [3] candidates (runs whose status is not PR_NOT_CANDIDATE), [4] the largest such count of one query
template <int CAP>
static __global__ __launch_bounds__(AU_SEL_THREADS) void k_pr_select(long long nq, long long q0, int n_top, const long long *first,
                                                                     const unsigned long long *keys, const int *run_start, int id_bits,
                                                                     const int *r_status, const double *r_sim, const int *r_common,
                                                                     int *out_cnt, int *out_user, double *out_sim, int *out_common,
                                                                     unsigned long long *cnt) {
    __shared__ unsigned long long K[2 * CAP];
    __shared__ unsigned P[2 * CAP];
    __shared__ int s_staged, s_have, s_cand;
    const int tid = threadIdx.x;
    const long long x = blockIdx.x;
    if (x >= nq) return;
    const long long a = first[x], b = first[x + 1];
    if (tid == 0) { s_have = 0; s_cand = 0; }
    int dropped = 0, floored = 0, cand = 0;
    for (long long r = a + tid; r < b; r += AU_SEL_THREADS) cand += r_status[r] != PR_NOT_CANDIDATE ? 1 : 0;
    au_select_segment<CAP, false>(a, b, n_top, r_sim, r_status, 0.0, K, P, &s_staged, dropped, floored);
    int have = 0;
    for (int j = tid; j < n_top; j += AU_SEL_THREADS) {
        const size_t o = (size_t)(q0 + x) * n_top + j;
        const unsigned pos = P[j];
        const bool v = pos != AU_NO_POS;
        have += v ? 1 : 0;
        out_user[o] = v ? (int)(keys[run_start[a + pos]] & ((1ull << id_bits) - 1ull)) : -1;
        out_sim[o] = v ? r_sim[a + pos] : 0.0;
        out_common[o] = v ? r_common[a + pos] : 0;
    }
    if (have) atomicAdd(&s_have, have);
    if (cand) atomicAdd(&s_cand, cand);
    __syncthreads();
    if (tid == 0) {
        out_cnt[q0 + x] = s_have;
        if (s_cand) { atomicAdd(&cnt[3], (unsigned long long)s_cand); atomicMax(&cnt[4], (unsigned long long)s_cand); }
    }
}

// the outputs of a query without records: count 0 and the padding
static __global__ __launch_bounds__(256) void k_pr_blank(long long n_query, int n_top, int *out_cnt, int *out_user, double *out_sim,
                                                         int *out_common) {
    const long long total = n_query * n_top, step = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += step) {
        if (k < n_query) out_cnt[k] = 0;
        out_user[k] = -1; out_sim[k] = 0.0; out_common[k] = 0;
    }
}

constexpr long long PR_SELECT_RANGE = 1ll << 23;        // queries (one block of 256 threads each) per launch of the selection
static_assert(PR_SELECT_RANGE * AU_SEL_THREADS < (1ll << 32), "the grid of a range stays below 2^32 threads");
constexpr unsigned PR_BLANK_BLOCKS = 1u << 20;          // blocks of the grid-stride fill of the outputs

template <int CAP, class... A>
static int pr_select_ranges(hipStream_t st, long long nq, long long q0, int n_top, const long long *first, A... a) {
    for (long long x0 = 0; x0 < nq; x0 += PR_SELECT_RANGE) {       // the queries of a range: first + x0, outputs from q0 + x0
        const long long m = nq - x0 < PR_SELECT_RANGE ? nq - x0 : PR_SELECT_RANGE;
        k_pr_select<CAP><<<dim3((unsigned)m), dim3(AU_SEL_THREADS), 0, st>>>(m, q0 + x0, n_top, first + x0, a...);
        XM_LAUNCH_CHECK();
    }
    return XMAP_OK;
}

// ---- the host half: what every caller does between its count pass and its reduce kernel -------------------------------------------

constexpr long long PR_MAX_RECORDS = 1ll << 22;         // the library's default chunk: 4 M records

// The chunk plan.  rec [n_query + 1] = the records in front of each query (read back from k_pr_qrec); cut = the chunk borders
// (chunk k = the queries [cut[k], cut[k + 1])), n_max / nq_max = the most records / queries of one chunk.
struct RecordChunks {
    std::vector<long long> rec, cut;
    long long n_max = 0, nq_max = 0;
};

// Chunks of consecutive queries with at most max_records records (<= 0: dflt), or one query.  Pure host code.  A chunk of several
// queries stays below 2^31 - 1 records, so only a single query can reach the capacity error.
static int pr_plan_chunks(const char *what, long long n_query, long long max_records, long long dflt, RecordChunks *C) {
    if (max_records <= 0) max_records = dflt;
    if (max_records > 2147483646ll) max_records = 2147483646ll;
    const std::vector<long long> &rec = C->rec;
    C->cut.assign(1, 0);
    C->n_max = C->nq_max = 0;
    for (long long q0 = 0; q0 < n_query;) {
        long long q1 = q0 + 1;
        while (q1 < n_query && rec[q1 + 1] - rec[q0] <= max_records) q1++;
        const long long n = rec[q1] - rec[q0];
        if (n >= 2147483647ll) {
            set_error("%s: query %lld expands to %lld records, a chunk holds fewer than 2^31", what, q0, n);
            return XMAP_ERR_CAPACITY;
        }
        C->n_max = n > C->n_max ? n : C->n_max;
        C->nq_max = q1 - q0 > C->nq_max ? q1 - q0 : C->nq_max;
        C->cut.push_back(q1);
        q0 = q1;
    }
    return XMAP_OK;
}

// body(q0, q1, n) for every chunk with records, in order; the first code that is not XMAP_OK ends the walk
template <class Body>
static int pr_each_chunk(const RecordChunks &C, Body body) {
    for (size_t k = 0; k + 1 < C.cut.size(); k++) {
        const long long q0 = C.cut[k], q1 = C.cut[k + 1], n = C.rec[q1] - C.rec[q0];
        if (n == 0) continue;                   // (the blank outputs stand)
        const int rc = body(q0, q1, n);
        if (rc) return rc;
    }
    return XMAP_OK;
}

// The run tables of the largest chunk: keys / vals [2 nm] (the second halves are the sort's), head [nm], run_idx / run_start
// [nm + 1], first [nq_max + 1].
struct RunTables {
    unsigned long long *keys;
    int *vals, *head, *run_start;
    long long *run_idx, *first;
    size_t nm;
};

// starts == false: a caller that never takes pr_run_starts (the count pass of the item fold-in) goes without run_start
static int pr_alloc_runs(hipStream_t st, long long n_max, long long nq_max, int id_bits, bool starts, RunTables *T) {
    XM_ARG(id_bits + bits_for(nq_max) <= 62);
    const size_t nm = (size_t)n_max;
    *T = RunTables{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nm};
    XM_HIP(xm_malloc_async((void **)&T->keys, sizeof(unsigned long long) * 2 * nm, st));
    XM_HIP(xm_malloc_async((void **)&T->vals, sizeof(int) * 2 * nm, st));
    XM_HIP(xm_malloc_async((void **)&T->head, sizeof(int) * nm, st));
    XM_HIP(xm_malloc_async((void **)&T->run_idx, sizeof(long long) * (nm + 1), st));
    if (starts) XM_HIP(xm_malloc_async((void **)&T->run_start, sizeof(int) * (nm + 1), st));
    XM_HIP(xm_malloc_async((void **)&T->first, sizeof(long long) * ((size_t)nq_max + 1), st));
    return XMAP_OK;
}

// the n expanded records of a chunk of nq queries: the stable sort, then run_idx = the run of every sorted position
static int pr_sort_runs(hipStream_t st, const RunTables &T, long long n, long long nq, int id_bits) {
    int rc = radix_sort_pairs(st, T.keys, T.vals, T.keys + T.nm, T.vals + T.nm, n, id_bits + bits_for(nq));
    if (rc) return rc;
    k_pr_heads<<<dim3(blocks_for(n, 256)), dim3(256), 0, st>>>(n, T.keys, T.head);
    XM_LAUNCH_CHECK();
    return xmap_exclusive_scan_i32_to_i64(st, T.head, (int64_t *)T.run_idx, n, nullptr);
}

static int pr_run_starts(hipStream_t st, const RunTables &T, long long n) {
    k_pr_starts<<<dim3(blocks_for(n, 256)), dim3(256), 0, st>>>(n, T.head, T.run_idx, T.run_start);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

// sort -> k_pr_heads -> scan -> k_pr_starts -> k_pr_first: everything between a caller's expansion and its reduce kernel
static int pr_run_tables(hipStream_t st, const RunTables &T, long long n, long long nq, int id_bits) {
    int rc = pr_sort_runs(st, T, n, nq, id_bits);
    if (rc || (rc = pr_run_starts(st, T, n))) return rc;
    k_pr_first<<<dim3(blocks_for(nq + 1, 256)), dim3(256), 0, st>>>(nq, n, T.keys, id_bits, T.run_idx, T.first);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

// k_pr_select over the runs of the nq queries from q0; r_int / out_int: the int that travels with a run (its size, a mask)
static int pr_select(hipStream_t st, const RunTables &T, long long nq, long long q0, int n_top, int id_bits, const int *r_status,
                     const double *r_score, const int *r_int, int *out_cnt, int *out_id, double *out_score, int *out_int,
                     unsigned long long *cnt) {
    return n_top <= 256 ? pr_select_ranges<256>(st, nq, q0, n_top, T.first, T.keys, T.run_start, id_bits, r_status, r_score, r_int, out_cnt,
                                                out_id, out_score, out_int, cnt)
                        : pr_select_ranges<1024>(st, nq, q0, n_top, T.first, T.keys, T.run_start, id_bits, r_status, r_score, r_int, out_cnt,
                                                 out_id, out_score, out_int, cnt);
}

static int pr_blank(hipStream_t st, long long n_query, int n_top, int *out_cnt, int *out_id, double *out_score, int *out_int) {
    const unsigned bb = blocks_for(n_query * n_top, 256);
    k_pr_blank<<<dim3(bb < PR_BLANK_BLOCKS ? bb : PR_BLANK_BLOCKS), dim3(256), 0, st>>>(n_query, n_top, out_cnt, out_id, out_score, out_int);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

}  // namespace xmap
#endif
