// sorted_runs.h -- the back half of "sort, don't hash" that the peers (stage_e_peers.hip), the user-kNN top-N (stage_e_uknn.hip) and
// the item fold-in (stage_e_itemfold.hip) share: over the records of a chunk of queries, stably sorted on
// (q - q0) << id_bits | id, the run heads, the run starts, the first run of every query, and -- for the first two -- the segmented
// selection (au_select.h) over the runs of a query with its outputs (count, id, score, size of the run).  What a run is worth --
// its status and score -- is the caller's own reduce kernel.
#ifndef XMAP_SORTED_RUNS_H
#define XMAP_SORTED_RUNS_H
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

static int pr_bits_for(long long v) {   // bits that hold 0 .. v - 1, at least one
    int b = 1;
    while (b < 62 && (1ll << b) < v) b++;
    return b;
}

static unsigned pr_blocks(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

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

}  // namespace xmap
#endif
