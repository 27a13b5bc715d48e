// stage_e_fuse.hip -- fused lists on the device (DESIGN.md 4 "Fused lists"): several top-N lists of the same queries (item-kNN,
// user-kNN, related items, one list per source domain ...) become one list per query, by rank (reciprocal rank fusion) or by
// score (weighted sum / weighted mean).  The records of query q are, for l = 0 .. n_lists - 1, for r = 0 .. m - 1 with
// m = min(max(cnt_l[q], 0), width_l), every (id = item_l[q][r], l, r) whose id lies in [0, n_ids).  A record's term is
// w_l / (rrf_c + (double)(r + 1)) or fl(w_l * score_l[q][r]); an id's num / den / mask run over its records in record order
// (l ascending, then r ascending) from 0.0, left to right.  Two routes, chosen from W = the sum of the widths alone:
//   W <= XMAP_FUSE_BLOCK_RECORDS : k_fu_block, one workgroup per query, the query's records in LDS from the first load to the
//                  selected list: keys id << 14 | l << 10 | r (distinct, so the bitonic network sorts them stably), run heads by
//                  comparing neighbours, the head lane walks its run, au_sort on (au_key(score), position).  No global temporary.
//   otherwise    : "sort, don't hash" with the host half of sorted_runs.h (pr_plan_chunks, pr_each_chunk), one slot = one (query, list):
//     k_fu_count  : records per slot, one wave per slot -> scan
//     k_fu_expand : one wave per slot of the chunk compacts the valid ids in r order: key = (q - q0) << id_bits | id,
//                   value = l << 10 | r
//     pr_run_tables : the stable sort -- the records of one (q, id) stay in (l, r) order --, the runs, per query its first run
//     k_fu_reduce : one lane per run: the same walk (fu_walk) as the block route's head lane
//     pr_select   : au_select_segment over the runs of a query; its int slot carries the mask
// Both routes compute a run's score with the one fu_walk and select on (au_key, position ascending with id): the same bytes.
#include <vector>

#include "common.h"
#include "au_select.h"
#include "predict_rows.h"
#include "sorted_runs.h"

namespace xmap {

constexpr unsigned long long FU_PAD = ~0ull;            // behind every record key (an id stays below 2^31)

// the lists of a call, by value in the kernel arguments
struct FuseLists {
    const int *cnt[XMAP_FUSE_MAX_LISTS];
    const int *item[XMAP_FUSE_MAX_LISTS];
    const double *score[XMAP_FUSE_MAX_LISTS];
    double weight[XMAP_FUSE_MAX_LISTS];
    int width[XMAP_FUSE_MAX_LISTS];
    int n;
};

// The kernels index the lists by a list number that differs from lane to lane: the arguments are copied into LDS once per block,
// with constant indices, so that no lane-indexed copy of them is made in private memory.  Ends with a barrier.
__device__ __forceinline__ void fu_stage(const FuseLists &A, FuseLists *s) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < XMAP_FUSE_MAX_LISTS; l++) {
            s->cnt[l] = A.cnt[l]; s->item[l] = A.item[l]; s->score[l] = A.score[l]; s->weight[l] = A.weight[l]; s->width[l] = A.width[l];
        }
        s->n = A.n;
    }
    __syncthreads();
}

// entries of list l that query q offers: min(max(cnt, 0), width)
__device__ __forceinline__ int fu_len(const FuseLists *L, int l, long long q) {
    const int c = L->cnt[l][q], w = L->width[l];
    return c < 0 ? 0 : c < w ? c : w;
}

// The ONE statement of an id's score, for both routes: the records [s, e) of a run in record order, code(t) = l << 10 | r.
// Returns the status of the run (0, or PR_DROPPED with *why = 0: min_lists, 1: not finite).
template <class Code>
__device__ __forceinline__ int fu_walk(const FuseLists *L, long long q, int how, double rrf_c, int min_lists, int s, int e, Code code,
                                       double *score, int *mask, int *why) {
    double num = 0.0, den = 0.0;
    int m = 0;
    for (int t = s; t < e; t++) {
        const int c = code(t), l = (c >> 10) & 15, r = c & 1023;
        const double w = L->weight[l];
        const double term = how == XMAP_FUSE_RRF ? w / (rrf_c + (double)(r + 1)) : w * L->score[l][(size_t)q * L->width[l] + r];
        num += term;
        den += w;
        m |= 1 << l;
    }
    *mask = m;
    *score = 0.0;
    if (__popc(m) < min_lists) { *why = 0; return PR_DROPPED; }
    const double x = how == XMAP_FUSE_MEAN ? num / den : num;
    if (!finite_f64(x)) { *why = 1; return PR_DROPPED; }
    *score = x;
    return 0;
}

// ---- the block route --------------------------------------------------------------------------------------------------------

constexpr int FU_MIN_NET = 128;                 // the smallest network: two 64-wide lists

// ascending bitonic sort of K[0 .. n), n a power of two and the same in every thread; all threads of the block
__device__ __forceinline__ void fu_sort(unsigned long long *K, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += AU_SEL_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = K[i], b = K[l];
                if ((a > b) == ((i & k) == 0)) { K[i] = b; K[l] = a; }
            }
            __syncthreads();
        }
    }
}

// au_sort (au_select.h) over (K, P)[0 .. n), n one of FU_MIN_NET, 2 FU_MIN_NET, ... N and the same in every thread
template <int N>
__device__ __forceinline__ void fu_au_sort(unsigned long long *K, unsigned *P, int n) {
    if (n == N) { au_sort<N / 2>(K, P); return; }
    if constexpr (N > FU_MIN_NET) fu_au_sort<N / 2>(K, P, n);
}

// One block per query q = q_base + blockIdx.x; N >= the sum of the widths, a power of two.  LDS: 32 B per record slot
// (R 8, S 8, M 4, K 8, P 4) + the lists.  The two networks run over n = the power of two at or above the records the query
// OFFERS (at least FU_MIN_NET, at most N; the counts are read alike by every thread), not over N: a query with 100 entries in
// lists 1 088 wide sorts 128 slots, not 2 048.  cnt: [0] dropped by min_lists, [1] not finite, [3] candidates, [4] the largest
// candidate count of one query, [5] records.
template <int N>
__global__ __launch_bounds__(AU_SEL_THREADS) void k_fu_block(long long q_base, FuseLists A, int n_ids, int how, double rrf_c, int min_lists,
                                                             int n_top, int *out_cnt, int *out_id, double *out_score, int *out_lists,
                                                             unsigned long long *cnt) {
    static_assert(N >= AU_SEL_THREADS && (N & (N - 1)) == 0 && N <= XMAP_FUSE_BLOCK_RECORDS, "bitonic sizes");
    __shared__ FuseLists sL;
    __shared__ unsigned long long R[N];         // the record keys id << 14 | l << 10 | r, FU_PAD behind them
    __shared__ double S[N];                     // at a run's head: its score
    __shared__ int M[N];                        //                  its mask
    __shared__ unsigned long long K[N];         // the selection: au_key of a kept head, AU_NO_KEY elsewhere
    __shared__ unsigned P[N];                   //                its position in R (ascends with the id)
    __shared__ int s_c[5];
    const int tid = threadIdx.x;
    const long long q = q_base + blockIdx.x;
    if (tid < 5) s_c[tid] = 0;
    fu_stage(A, &sL);
    // ---- load: list after list, the entries the query offers; an id outside [0, n_ids) leaves a pad
    int off = 0;
    for (int l = 0; l < sL.n; l++) {
        const int m = fu_len(&sL, l, q);
        const int *it = sL.item[l] + (size_t)q * sL.width[l];
        for (int r = tid; r < m; r += AU_SEL_THREADS) {
            const int id = it[r];
            R[off + r] = (id >= 0 && id < n_ids) ? ((unsigned long long)(unsigned)id << 14) | (unsigned long long)((l << 10) | r) : FU_PAD;
        }
        off += m;                               // (the same in every thread; at most the sum of the widths <= N)
    }
    int n = FU_MIN_NET;
    while (n < off) n <<= 1;
    for (int k = off + tid; k < n; k += AU_SEL_THREADS) R[k] = FU_PAD;
    __syncthreads();
    fu_sort(R, n);
    // ---- run heads; the head lane walks its run
    int n_rec = 0, n_cand = 0, n_min = 0, n_inf = 0, n_kept = 0;
    for (int i = tid; i < n; i += AU_SEL_THREADS) {
        const unsigned long long k = R[i];
        unsigned long long key = AU_NO_KEY;
        unsigned pos = AU_NO_POS;
        if (k != FU_PAD) {
            n_rec++;
            if (i == 0 || (R[i - 1] >> 14) != (k >> 14)) {
                int e = i + 1;
                while (e < n && (R[e] >> 14) == (k >> 14)) e++;
                double score;
                int mask, why = 0;
                const int st = fu_walk(&sL, q, how, rrf_c, min_lists, i, e, [&](int t) { return (int)(R[t] & 0x3fffull); }, &score, &mask, &why);
                n_cand++;
                if (st == 0) { key = au_key(score); pos = (unsigned)i; S[i] = score; M[i] = mask; n_kept++; }
                else if (why == 0) n_min++;
                else n_inf++;
            }
        }
        K[i] = key; P[i] = pos;
    }
    if (n_rec) atomicAdd(&s_c[0], n_rec);
    if (n_cand) atomicAdd(&s_c[1], n_cand);
    if (n_min) atomicAdd(&s_c[2], n_min);
    if (n_inf) atomicAdd(&s_c[3], n_inf);
    if (n_kept) atomicAdd(&s_c[4], n_kept);
    __syncthreads();
    // ---- selection: score descending as numbers, position (= id) ascending on equal scores
    fu_au_sort<N>(K, P, n);
    for (int j = tid; j < n_top; j += AU_SEL_THREADS) {
        const size_t o = (size_t)q * n_top + j;
        const unsigned pos = j < n ? P[j] : AU_NO_POS;
        const bool v = pos != AU_NO_POS;
        out_id[o] = v ? (int)(R[v ? pos : 0] >> 14) : -1;
        out_score[o] = v ? S[pos] : 0.0;
        out_lists[o] = v ? M[pos] : 0;
    }
    if (tid == 0) {
        out_cnt[q] = s_c[4] < n_top ? s_c[4] : n_top;
        if (s_c[0]) atomicAdd(&cnt[5], (unsigned long long)s_c[0]);
        if (s_c[1]) { atomicAdd(&cnt[3], (unsigned long long)s_c[1]); atomicMax(&cnt[4], (unsigned long long)s_c[1]); }
        if (s_c[2]) atomicAdd(&cnt[0], (unsigned long long)s_c[2]);
        if (s_c[3]) atomicAdd(&cnt[1], (unsigned long long)s_c[3]);
    }
}

template <int N>
static int fu_block_ranges(hipStream_t st, long long n_query, const FuseLists &A, int n_ids, int how, double rrf_c, int min_lists, int n_top,
                           int *out_cnt, int *out_id, double *out_score, int *out_lists, unsigned long long *cnt) {
    for (long long q0 = 0; q0 < n_query; q0 += PR_SELECT_RANGE) {          // one block of 256 threads per query: below 2^32 threads
        const long long m = n_query - q0 < PR_SELECT_RANGE ? n_query - q0 : PR_SELECT_RANGE;
        k_fu_block<N><<<dim3((unsigned)m), dim3(AU_SEL_THREADS), 0, st>>>(q0, A, n_ids, how, rrf_c, min_lists, n_top, out_cnt, out_id, out_score,
                                                                           out_lists, cnt);
        XM_LAUNCH_CHECK();
    }
    return XMAP_OK;
}

// ---- the sorted-runs route --------------------------------------------------------------------------------------------------

// rcnt[e] = the records of slot e = q * n_lists + l, one wave per slot; n_rec += them
__global__ __launch_bounds__(256) void k_fu_count(long long base, long long n_slots, FuseLists A, int n_ids, int *rcnt,
                                                  unsigned long long *n_rec) {
    __shared__ FuseLists sL;
    fu_stage(A, &sL);
    const long long e = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (e >= n_slots) return;                   // (wave-uniform)
    const int lane = lane_id();
    const long long q = e / sL.n;
    const int l = (int)(e - q * sL.n);
    const int m = fu_len(&sL, l, q);
    const int *it = sL.item[l] + (size_t)q * sL.width[l];
    int c = 0;
    for (int r0 = 0; r0 < m; r0 += WAVE) {
        const int r = r0 + lane;
        const int id = r < m ? it[r] : -1;
        c += __popcll(__ballot(id >= 0 && id < n_ids));
    }
    if (lane == 0) {
        rcnt[e] = c;
        if (c) atomicAdd(n_rec, (unsigned long long)c);
    }
}

// one wave per slot e in [e0, e1) of the chunk: its records at rec_off[e] - rec0, the valid ids compacted in r order
__global__ __launch_bounds__(256) void k_fu_expand(long long e0, long long e1, long long rec0, long long q0, FuseLists A, int n_ids,
                                                   const long long *rec_off, int id_bits, unsigned long long *keys, int *vals) {
    __shared__ FuseLists sL;
    fu_stage(A, &sL);
    const long long e = e0 + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (e >= e1) return;
    const int lane = lane_id();
    const long long end = rec_off[e + 1] - rec0;
    long long o = rec_off[e] - rec0;
    if (o == end) return;                       // no record
    const long long q = e / sL.n;
    const int l = (int)(e - q * sL.n);
    const int m = fu_len(&sL, l, q);
    const int *it = sL.item[l] + (size_t)q * sL.width[l];
    const unsigned long long qk = (unsigned long long)(q - q0) << id_bits;
    for (int r0 = 0; r0 < m; r0 += WAVE) {
        const int r = r0 + lane;
        const int id = r < m ? it[r] : -1;
        const bool on = id >= 0 && id < n_ids;
        const unsigned long long mask = __ballot(on);
        const long long at = o + __popcll(mask & lanemask_lt());
        if (on && at < end) {                   // (at < end: the count pass saw the same row)
            keys[at] = qk | (unsigned long long)(unsigned)id;
            vals[at] = (l << 10) | r;
        }
        o += __popcll(mask);
    }
}

// one lane per run, records in sorted (= expansion) order.  cnt: [0] dropped by min_lists, [1] not finite
__global__ __launch_bounds__(256) void k_fu_reduce(long long n, long long q0, FuseLists A, const unsigned long long *keys, const int *vals,
                                                   int id_bits, const long long *run_idx, const int *run_start, int how, double rrf_c,
                                                   int min_lists, int *r_status, double *r_score, int *r_mask, unsigned long long *cnt) {
    __shared__ FuseLists sL;
    fu_stage(A, &sL);
    const long long n_runs = run_idx[n];
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_runs; r += step) {
        const int s = run_start[r], e = run_start[r + 1];
        const long long q = q0 + (long long)(keys[s] >> id_bits);
        double score;
        int mask, why = 0;
        const int st = fu_walk(&sL, q, how, rrf_c, min_lists, s, e, [&](int t) { return vals[t]; }, &score, &mask, &why);
        r_status[r] = st;
        r_score[r] = score;
        r_mask[r] = mask;
        if (st) atomicAdd(&cnt[why], 1ull);
    }
}

// The host checks of xmap_fuse_rows and xmap_ctx_fuse, each naming its argument; nothing is written and no device is touched.
int fuse_check(const char *who, int64_t n_query, int32_t n_lists, const xmap_fuse_list *lists, int32_t n_ids, int32_t how, double rrf_c,
               int32_t min_lists, int32_t n_top, int64_t max_records, const void *out_cnt, const void *out_id, const void *out_score,
               const void *out_lists) {
#define FU_CHECK(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return XMAP_ERR_ARG; } } while (0)
    FU_CHECK(n_lists >= 1 && n_lists <= XMAP_FUSE_MAX_LISTS, "%s: n_lists = %d, not in 1 .. %d", who, n_lists, XMAP_FUSE_MAX_LISTS);
    FU_CHECK(lists, "%s: lists is NULL", who);
    FU_CHECK(how == XMAP_FUSE_RRF || how == XMAP_FUSE_SUM || how == XMAP_FUSE_MEAN, "%s: how = %d", who, how);
    for (int l = 0; l < n_lists; l++) {
        FU_CHECK(lists[l].width >= 1 && lists[l].width <= AU_MAX_TOP, "%s: lists[%d].width = %d, not in 1 .. 1024", who, l, lists[l].width);
        FU_CHECK(finite_f64(lists[l].weight), "%s: lists[%d].weight is not finite", who, l);
        FU_CHECK(lists[l].score || how == XMAP_FUSE_RRF, "%s: lists[%d].score is NULL, how is not XMAP_FUSE_RRF", who, l);
    }
    FU_CHECK(finite_f64(rrf_c) && rrf_c >= 0.0, "%s: rrf_c is not finite and >= 0", who);
    FU_CHECK(min_lists >= 1 && min_lists <= n_lists, "%s: min_lists = %d, not in 1 .. n_lists = %d", who, min_lists, n_lists);
    FU_CHECK(n_top >= 1 && n_top <= AU_MAX_TOP, "%s: n_top = %d, not in 1 .. 1024", who, n_top);
    FU_CHECK(n_ids >= 0, "%s: n_ids = %d is negative", who, n_ids);
    FU_CHECK(max_records >= 0, "%s: max_records = %lld is negative", who, (long long)max_records);
    FU_CHECK(n_query >= 0 && n_query <= (1ll << 28), "%s: n_query = %lld, not in 0 .. 2^28", who, (long long)n_query);
    if (n_query > 0) {
        for (int l = 0; l < n_lists; l++) {
            FU_CHECK(lists[l].cnt, "%s: lists[%d].cnt is NULL", who, l);
            FU_CHECK(lists[l].item, "%s: lists[%d].item is NULL", who, l);
        }
        FU_CHECK(out_cnt, "%s: out_cnt is NULL", who);
        FU_CHECK(out_id, "%s: out_id is NULL", who);
        FU_CHECK(out_score, "%s: out_score is NULL", who);
        FU_CHECK(out_lists, "%s: out_lists is NULL", who);
    }
#undef FU_CHECK
    return XMAP_OK;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_fuse_rows(void *stream, int64_t n_query, int32_t n_lists, const xmap_fuse_list *lists, int32_t n_ids, int32_t how, double rrf_c,
                   int32_t min_lists, int32_t n_top, int64_t max_records, int32_t *out_cnt, int32_t *out_id, double *out_score,
                   int32_t *out_lists, int64_t *h_stats) {
    // the host checks: before any device work
    int rc = fuse_check("xmap_fuse_rows", n_query, n_lists, lists, n_ids, how, rrf_c, min_lists, n_top, max_records, out_cnt, out_id, out_score,
                        out_lists);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    if (h_stats) for (int k = 0; k < 5; k++) h_stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    FuseLists A;
    memset(&A, 0, sizeof(A));
    long long W = 0;
    for (int l = 0; l < n_lists; l++) {
        A.cnt[l] = lists[l].cnt; A.item[l] = lists[l].item; A.score[l] = lists[l].score; A.weight[l] = lists[l].weight;
        A.width[l] = lists[l].width;
        W += lists[l].width;
    }
    A.n = n_lists;
    unsigned long long *cnt = nullptr, h[6] = {0, 0, 0, 0, 0, 0};
    XM_HIP(xm_malloc_async((void **)&cnt, sizeof(h), st));
    XM_HIP(hipMemsetAsync(cnt, 0, sizeof(h), st));
    const auto finish = [&]() -> int {
        XM_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
        if (h_stats) {
            h_stats[0] = (int64_t)h[3]; h_stats[1] = (int64_t)h[0]; h_stats[2] = (int64_t)h[1]; h_stats[3] = (int64_t)h[4];
            h_stats[4] = (int64_t)h[5];
        }
        return XMAP_OK;
    };
    // ---- the block route: the sum of the widths decides, nothing else
    if (W <= XMAP_FUSE_BLOCK_RECORDS) {
        rc = W <= 256    ? fu_block_ranges<256>(st, n_query, A, n_ids, how, rrf_c, min_lists, n_top, out_cnt, out_id, out_score, out_lists, cnt)
             : W <= 512  ? fu_block_ranges<512>(st, n_query, A, n_ids, how, rrf_c, min_lists, n_top, out_cnt, out_id, out_score, out_lists, cnt)
             : W <= 1024 ? fu_block_ranges<1024>(st, n_query, A, n_ids, how, rrf_c, min_lists, n_top, out_cnt, out_id, out_score, out_lists, cnt)
                         : fu_block_ranges<2048>(st, n_query, A, n_ids, how, rrf_c, min_lists, n_top, out_cnt, out_id, out_score, out_lists, cnt);
        if (rc) return rc;
        return finish();
    }
    // ---- the sorted-runs route: records per slot
    const long long n_slots = (long long)n_query * n_lists;
    const size_t nq1 = (size_t)n_query + 1;
    int *rcnt = nullptr;
    long long *rec_off = nullptr, *qrec = nullptr;
    XM_HIP(xm_malloc_async((void **)&rcnt, sizeof(int) * (size_t)n_slots, st));
    XM_HIP(xm_malloc_async((void **)&rec_off, sizeof(long long) * ((size_t)n_slots + 1), st));
    XM_HIP(xm_malloc_async((void **)&qrec, sizeof(long long) * nq1, st));
    rc = for_pair_ranges(n_slots, 4, [&](long long base, long long end, dim3 grid) {
        k_fu_count<<<grid, dim3(256), 0, st>>>(base, end, A, n_ids, rcnt, cnt + 5);
    });
    if (rc) return rc;
    if ((rc = xmap_exclusive_scan_i32_to_i64(st, rcnt, (int64_t *)rec_off, n_slots, nullptr))) return rc;
    k_pr_qrec<<<dim3(blocks_for(n_query + 1, 256)), dim3(256), 0, st>>>(n_query, nullptr, n_lists, rec_off, qrec);
    XM_LAUNCH_CHECK();
    RecordChunks C;
    C.rec.resize(nq1);
    XM_HIP(hipMemcpyAsync(C.rec.data(), qrec, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    // ---- the chunks (a query has at most 16 * 1024 records: the capacity error of the plan is out of reach), then the outputs
    if ((rc = pr_plan_chunks("fuse", n_query, max_records, PR_MAX_RECORDS, &C))) return rc;
    if ((rc = pr_blank(st, n_query, n_top, out_cnt, out_id, out_score, out_lists))) return rc;
    if (C.n_max > 0) {
        const int id_bits = bits_for(n_ids);
        const size_t nm = (size_t)C.n_max;
        RunTables T;
        int *r_status = nullptr, *r_mask = nullptr;
        double *r_score = nullptr;
        if ((rc = pr_alloc_runs(st, C.n_max, C.nq_max, id_bits, true, &T))) return rc;
        XM_HIP(xm_malloc_async((void **)&r_status, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_mask, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_score, sizeof(double) * nm, st));
        rc = pr_each_chunk(C, [&](long long q0, long long q1, long long n) {
            const unsigned nb = blocks_for(n, 256);
            const long long e0 = q0 * n_lists;
            int rc = for_pair_ranges((q1 - q0) * n_lists, 4, [&](long long base, long long end, dim3 grid) {       // slots [base, end) of the chunk
                k_fu_expand<<<grid, dim3(256), 0, st>>>(e0 + base, e0 + end, C.rec[q0], q0, A, n_ids, rec_off, id_bits, T.keys, T.vals);
            });
            if (rc || (rc = pr_run_tables(st, T, n, q1 - q0, id_bits))) return rc;
            k_fu_reduce<<<dim3(nb < 4096u ? nb : 4096u), dim3(256), 0, st>>>(n, q0, A, T.keys, T.vals, id_bits, T.run_idx, T.run_start, how, rrf_c,
                                                                            min_lists, r_status, r_score, r_mask, cnt);
            XM_LAUNCH_CHECK();
            return pr_select(st, T, q1 - q0, q0, n_top, id_bits, r_status, r_score, r_mask, out_cnt, out_id, out_score, out_lists, cnt);
        });
        if (rc) return rc;
    }
    return finish();
}
}
