// stage_e_topn.hip -- top-N recommendation on the device: for every query user the N best items the user's own rows give
// evidence for, ranked by the unrounded prediction (DESIGN.md 4 "Top-N").  Everything it reads is what the tail leaves
// resident: user-major profiles, neighbour lists [I][keep], item averages.
//
//   k_tn_rev<count | fill> : (topn_pass.h) the reverse of the neighbour lists -- for neighbour n the items whose first
//                     min(cnt, keep) entries hold n -- by count -> xmap_exclusive_scan -> fill.  One entry per list position
//                     (a repeated neighbour repeats its owner); the order inside a row is whatever the atomics give: the
//                     candidate pass de-duplicates through a bitmap and emits in index order.
//   k_tn_candidates : one block per query user, run twice (count, then fill into buffers of exactly the counted size).  The
//                     item space is walked in windows of TN_WINDOW items; an LDS bitmap of the window takes the union of
//                     rev[p] over the profile items p (16 lanes per profile row), the held items are cleared again unless
//                     XMAP_TOPN_KEEP_HELD, and the marked items leave in ascending index.  A second-level bitmap (one bit per
//                     bitmap word that was touched) is all the emit pass scans, and it zeroes exactly the words it visits:
//                     the window is cleared once per block, never per user.
//   scoring         : k_predict_rows<., RAW = true> (predict_rows.h) over the (user, item) candidate list: the pair body of the
//                     prediction itself, the values before bound_rating.  More than PR_CAP evidence entries: its arena launch.
//   k_tn_select     : segmented top-N, one wave per query: lane j holds the j-th best (score desc, item asc) seen so far; the
//                     segment streams through 64 candidates at a time, a candidate that beats the current N-th is inserted by
//                     a ballot count and a one-lane shift.  Candidates with status 2 are dropped and counted.
// xmap_topn_rows_filtered (rec_filter.h; DESIGN.md 4 "Eligibility"): the FILT instantiation of k_tn_candidates clears the query's
// exclusion ids in the bitmap and ANDs every emitted word with the item mask -- before anything is scored -- and k_tn_select
// drops and counts the candidates below the score floor.
// The call is two halves: tn_score_candidates (reverse lists, candidates, scores; declared in topn_pass.h, which also holds k_tn_rev,
// tn_block_scan and the window geometry) and the selection.  The group lists (stage_e_group.hip) run the first half over their
// flattened member list.
// Every output position follows from the scans, so the result does not depend on the grid or on the order of the atomics.
#include "common.h"
#include "predict_rows.h"
#include "rec_filter.h"
#include "topn_pass.h"

namespace xmap {

constexpr int TN_WINDOW = 1 << 19;              // items per bitmap pass (64 KB of LDS; two blocks per CU)
static_assert(TN_WINDOW == 1 << TN_WINDOW_LOG2, "the window of topn_pass.h, which stage_e_group.hip shares");
static_assert(TN_WINDOW % 32 == 0, "a window starts at a word of the mask");

// FILT (rec_filter.h): the query's exclusion ids are cleared behind the held items, and a touched word meets its word of the
// mask where it is emitted; the count pass adds what the two removed to *removed.  FILT = false is the unfiltered kernel.
template <bool FILL, bool FILT>
__global__ __launch_bounds__(TN_THREADS) void k_tn_candidates(long long n_query, const int *query_user, long long U, int I, int keep_held,
                                                              const long long *rptr, const int *ritem, const long long *pptr,
                                                              const int *pitem, int *cand_cnt, const long long *cand_ptr,
                                                              int *cand_user, int *cand_item, const unsigned int *allow,
                                                              const long long *ex_ptr, const int *ex_id, unsigned long long *removed) {
    extern __shared__ unsigned int tn_lds[];    // [TN_WORDS] bitmap of the window, [TN_SUMMARY] touched words (zero between users),
    unsigned int *bits = tn_lds, *summ = tn_lds + TN_WORDS;                                      // [TN_THREADS / 64] scan scratch
    int *s_scan = (int *)(tn_lds + TN_WORDS + TN_SUMMARY);
    const int tid = threadIdx.x;
    for (int k = tid; k < TN_WORDS + TN_SUMMARY; k += TN_THREADS) tn_lds[k] = 0u;
    __syncthreads();
    [[maybe_unused]] unsigned int gone = 0;     // FILT, count pass: candidates of this thread's words and ids that the rules removed
    for (long long q = blockIdx.x; q < n_query; q += gridDim.x) {
        const int u = query_user[q];
        long long a = 0, b = 0;
        if (u >= 0 && u < U) { a = pptr[u]; b = pptr[u + 1]; }
        long long total = 0;
        const long long out0 = FILL ? cand_ptr[q] : 0;
        for (long long lo = 0; lo < I && b > a; lo += TN_WINDOW) {
            // mark: 16 lanes per profile row walk the reverse row of its item
            for (long long p = a + (tid >> 4); p < b; p += TN_THREADS / 16) {
                const int it = pitem[p];
                if (it < 0 || it >= I) continue;
                const long long r1 = rptr[it + 1];
                for (long long r = rptr[it] + (tid & 15); r < r1; r += 16) {
                    const long long x = (long long)ritem[r] - lo;
                    if (x < 0 || x >= TN_WINDOW) continue;
                    const int w = (int)(x >> 5);
                    const unsigned int old = atomicOr(&bits[w], 1u << (x & 31));
                    if (old == 0u) atomicOr(&summ[w >> 5], 1u << (w & 31));
                }
            }
            __syncthreads();
            if (!keep_held) {                   // an item the user holds is no candidate (its word stays listed as touched)
                for (long long p = a + tid; p < b; p += TN_THREADS) {
                    const long long x = (long long)pitem[p] - lo;
                    if (x >= 0 && x < TN_WINDOW) atomicAnd(&bits[x >> 5], ~(1u << (x & 31)));
                }
                __syncthreads();
            }
            if constexpr (FILT) {               // the query's exclusions: a bit that was still set is a candidate removed, once
                if (ex_ptr) {
                    const long long e1 = ex_ptr[q + 1];
                    for (long long e = ex_ptr[q] + tid; e < e1; e += TN_THREADS) {
                        const long long id = ex_id[e], x = id - lo;
                        if (id < 0 || id >= I || x < 0 || x >= TN_WINDOW) continue;
                        const unsigned int bit = 1u << (x & 31);
                        const unsigned int old = atomicAnd(&bits[x >> 5], ~bit);
                        if constexpr (!FILL) gone += (old & bit) ? 1u : 0u;
                    }
                    __syncthreads();
                }
            }
            // emit in ascending index: count per thread, scan over the block, write; the visited words are zeroed on the way
            int c = 0;
#pragma unroll
            for (int k = 0; k < TN_PER; k++) {
                unsigned int sw = summ[tid * TN_PER + k];
                while (sw) {
                    const int w = (tid * TN_PER + k) * 32 + __ffs(sw) - 1;
                    sw &= sw - 1;
                    const unsigned int raw = bits[w], bw = rf_eligible<FILT>(raw, allow, (lo >> 5) + w);
                    c += __popc(bw);
                    if constexpr (FILT && !FILL) gone += __popc(raw) - __popc(bw);
                }
            }
            int tot;
            const int ex = tn_block_scan(c, &tot, s_scan);
            long long o = out0 + total + ex;
#pragma unroll
            for (int k = 0; k < TN_PER; k++) {
                const int s = tid * TN_PER + k;
                unsigned int sw = summ[s];
                if (sw == 0u) continue;
                summ[s] = 0u;
                while (sw) {
                    const int w = s * 32 + __ffs(sw) - 1;
                    sw &= sw - 1;
                    unsigned int bw = bits[w];
                    bits[w] = 0u;
                    if constexpr (FILL) {
                        bw = rf_eligible<FILT>(bw, allow, (lo >> 5) + w);
                        while (bw) {
                            const int bit = __ffs(bw) - 1;
                            bw &= bw - 1;
                            cand_user[o] = u;
                            cand_item[o] = (int)(lo + (long long)w * 32 + bit);
                            o++;
                        }
                    }
                }
            }
            total += tot;
            __syncthreads();
        }
        if constexpr (!FILL) {
            if (tid == 0) cand_cnt[q] = (int)total;
        }
    }
    if constexpr (FILT && !FILL) {
        if (gone) atomicAdd(removed, (unsigned long long)gone);
    }
}

// lane j < have holds the j-th best candidate so far; keys are distinct (a segment holds an item once).  FLOOR: a scored candidate
// below min_score is dropped and counted; FLOOR = false is the selection of the unfiltered call (min_score is not read)
template <bool FLOOR>
__global__ __launch_bounds__(256) void k_tn_select(long long n_query, int n_top, int rank_by, const long long *cand_ptr, const int *cand_item,
                                                   const double *plain, const double *decay, const int *status, int *out_cnt,
                                                   int *out_item, double *out_plain, double *out_decay,
                                                   unsigned long long *stats /*[0] dropped candidates, [1] largest segment,
                                                                               [2] candidates below the floor*/,
                                                   double min_score) {
    const int lane = lane_id();
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_query) return;
    const long long a = cand_ptr[q], b = cand_ptr[q + 1];
    double ks = 0.0, kp = 0.0, kd = 0.0;
    int ki = -1, have = 0, dropped = 0, floored = 0;
    for (long long p = a; p < b; p += 64) {
        const bool in = p + lane < b;
        const bool scored = in && status[p + lane] == 0;
        dropped += __popcll(__ballot(in && !scored));
        const int xi = scored ? cand_item[p + lane] : 0;
        const double xp = scored ? plain[p + lane] : 0.0, xd = scored ? decay[p + lane] : 0.0;
        const double xs = rank_by ? xd : xp;
        bool ok = scored;
        if constexpr (FLOOR) {                          // the floor: kept iff score >= min_score
            ok = scored && !(xs < min_score);
            floored += __popcll(__ballot(scored && !ok));
        }
        const double ws = rld(ks, n_top - 1);
        const int wi = rl32(ki, n_top - 1);
        unsigned long long m = __ballot(ok && (have < n_top || xs > ws || (xs == ws && xi < wi)));
        while (m) {
            const int j = __ffsll((long long)m) - 1;
            m &= m - 1;
            const double es = rld(xs, j), ep = rld(xp, j), ed = rld(xd, j);
            const int ei = rl32(xi, j);
            const int pos = __popcll(__ballot(lane < have && (ks > es || (ks == es && ki < ei))));
            if (pos >= n_top) continue;
            const double us = __shfl_up(ks, 1, 64), up = __shfl_up(kp, 1, 64), ud = __shfl_up(kd, 1, 64);
            const int ui = __shfl_up(ki, 1, 64);
            if (lane > pos) { ks = us; kp = up; kd = ud; ki = ui; }
            else if (lane == pos) { ks = es; kp = ep; kd = ed; ki = ei; }
            have = have < n_top ? have + 1 : n_top;
        }
    }
    if (lane < n_top) {
        const size_t o = (size_t)q * n_top + lane;
        const bool v = lane < have;
        out_item[o] = v ? ki : -1;
        out_plain[o] = v ? kp : 0.0;
        out_decay[o] = v ? kd : 0.0;
    }
    if (lane == 0) {
        out_cnt[q] = have;
        if (dropped) atomicAdd(&stats[0], (unsigned long long)dropped);
        if constexpr (FLOOR) {
            if (floored) atomicAdd(&stats[2], (unsigned long long)floored);
        }
        atomicMax(&stats[1], (unsigned long long)(b - a));
    }
}

// the two passes of the candidate kernel and the selection, by the rules a call carries: one statement per launch
template <bool FILL, bool FILT, class... A>
static void tn_candidates_launch(hipStream_t st, unsigned blocks, size_t lds, A... a) {
    k_tn_candidates<FILL, FILT><<<dim3(blocks), dim3(TN_THREADS), lds, st>>>(a...);
}
template <bool FILL, class... A>
static hipError_t tn_candidates(bool filt, hipStream_t st, unsigned blocks, size_t lds, A... a) {
    const void *f = filt ? (const void *)k_tn_candidates<FILL, true> : (const void *)k_tn_candidates<FILL, false>;
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (filt) tn_candidates_launch<FILL, true>(st, blocks, lds, a...);
    else tn_candidates_launch<FILL, false>(st, blocks, lds, a...);
    return hipGetLastError();
}

// topn_pass.h: the candidate-and-scoring half, shared with the member pass of the group lists (stage_e_group.hip)
int tn_score_candidates(hipStream_t st, int64_t n_query, const int32_t *query_user, int32_t flags, int64_t n_users, int32_t n_items,
                        int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim, const int64_t *prof_ptr,
                        const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time, const double *item_avg,
                        const double *wtab, int32_t n_w, bool filt, const unsigned int *allow, const long long *ex_ptr, const int *ex_id,
                        unsigned long long *removed, TnScored *out) {
    const int I = n_items;
    const size_t i1 = (size_t)(I ? I : 1);
    // ---- reverse neighbour lists
    int *rcnt = nullptr, *ritem = nullptr;
    long long *rptr = nullptr;
    int64_t n_rev = 0;
    XM_HIP(xm_malloc_async((void **)&rcnt, sizeof(int) * i1, st));
    XM_HIP(xm_malloc_async((void **)&rptr, sizeof(long long) * (i1 + 1), st));
    XM_HIP(hipMemsetAsync(rcnt, 0, sizeof(int) * i1, st));
    const unsigned rev_blocks = (unsigned)(((long long)I * keep + 255) / 256);
    if (I > 0) {
        k_tn_rev<false><<<dim3(rev_blocks), dim3(256), 0, st>>>(I, keep, nb_cnt, nb_col, rcnt, nullptr, nullptr);
        XM_LAUNCH_CHECK();
    }
    int rc = xmap_exclusive_scan_i32_to_i64(st, rcnt, (int64_t *)rptr, I, &n_rev);
    if (rc) return rc;
    XM_HIP(xm_malloc_async((void **)&ritem, sizeof(int) * (size_t)(n_rev ? n_rev : 1), st));
    if (n_rev > 0) {
        XM_HIP(hipMemsetAsync(rcnt, 0, sizeof(int) * i1, st));
        k_tn_rev<true><<<dim3(rev_blocks), dim3(256), 0, st>>>(I, keep, nb_cnt, nb_col, rcnt, rptr, ritem);
        XM_LAUNCH_CHECK();
    }
    // ---- candidates: count, scan, fill
    int *cand_cnt = nullptr, *cand_user = nullptr;
    XM_HIP(xm_malloc_async((void **)&cand_cnt, sizeof(int) * (size_t)n_query, st));
    XM_HIP(xm_malloc_async((void **)&out->cand_ptr, sizeof(long long) * ((size_t)n_query + 1), st));
    const size_t lds = TN_LDS_BYTES;
    const unsigned cblocks = (unsigned)(n_query < TN_MAX_BLOCKS ? n_query : TN_MAX_BLOCKS);
    XM_HIP(tn_candidates<false>(filt, st, cblocks, lds, (long long)n_query, query_user, (long long)n_users, I, flags & XMAP_TOPN_KEEP_HELD,
                                (const long long *)rptr, (const int *)ritem, (const long long *)prof_ptr, prof_item, cand_cnt,
                                (const long long *)nullptr, (int *)nullptr, (int *)nullptr, allow, ex_ptr, ex_id, removed));
    rc = xmap_exclusive_scan_i32_to_i64(st, cand_cnt, (int64_t *)out->cand_ptr, n_query, &out->n_pairs);
    if (rc) return rc;
    if (out->n_pairs > 0) {
        const size_t np = (size_t)out->n_pairs;
        XM_HIP(xm_malloc_async((void **)&cand_user, sizeof(int) * np, st));
        XM_HIP(xm_malloc_async((void **)&out->cand_item, sizeof(int) * np, st));
        XM_HIP(xm_malloc_async((void **)&out->plain, sizeof(double) * np, st));
        XM_HIP(xm_malloc_async((void **)&out->decay, sizeof(double) * np, st));
        XM_HIP(xm_malloc_async((void **)&out->status, sizeof(int) * np, st));
        XM_HIP(tn_candidates<true>(filt, st, cblocks, lds, (long long)n_query, query_user, (long long)n_users, I, flags & XMAP_TOPN_KEEP_HELD,
                                   (const long long *)rptr, (const int *)ritem, (const long long *)prof_ptr, prof_item, (int *)nullptr,
                                   (const long long *)out->cand_ptr, cand_user, out->cand_item, allow, ex_ptr, ex_id,
                                   (unsigned long long *)nullptr));
        // ---- scores: the pair body of the prediction, unrounded
        rc = predict_rows_run<true>(st, out->n_pairs, cand_user, out->cand_item, n_users, I, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item,
                                    prof_rating, prof_time, item_avg, wtab, n_w, out->plain, out->decay, out->status, &out->max_now);
        if (rc) return rc;
    }
    return XMAP_OK;
}

}  // namespace xmap
using namespace xmap;

// xmap_topn_rows (F == NULL, n_stats = 4) and xmap_topn_rows_filtered (n_stats = 6)
static int topn_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                     int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                     const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                     const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *out_cnt,
                     int32_t *out_item, double *out_plain, double *out_decay, const xmap_rec_filter *F, int64_t *h_stats, int n_stats) {
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    XM_ARG(n_top >= 1 && n_top <= TN_MAX_TOP);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query >= 0 && n_users >= 0 && n_items >= 0 && keep >= 1 && keep <= 64 && prof_ptr);
    XM_ARG(n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay));
    XM_ARG(n_items == 0 || (nb_cnt && nb_col && nb_sim && item_avg));
    XM_ARG(n_users == 0 || (prof_item && prof_rating && prof_time));
    if (h_stats) for (int k = 0; k < n_stats; k++) h_stats[k] = 0;
    bool filt = false;
    double min_score = 0.0;
    int rc = rf_prepare(st, n_query, F, &filt, &min_score);     // before any candidate work
    if (rc) return rc;
    if (n_query == 0) return XMAP_OK;
    // [0] dropped candidates, [1] largest segment, [2] below the floor, [3] removed by the mask or the exclusion lists
    unsigned long long *stats = nullptr;
    XM_HIP(xm_malloc_async((void **)&stats, sizeof(unsigned long long) * 4, st));
    XM_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long) * 4, st));
    TnScored S;
    rc = tn_score_candidates(st, n_query, query_user, flags, n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating,
                             prof_time, item_avg, wtab, n_w, filt, filt ? (const unsigned int *)F->allow : nullptr,
                             filt ? (const long long *)F->ex_ptr : nullptr, filt ? F->ex_id : nullptr, stats + 3, &S);
    if (rc) return rc;
    // ---- selection (n_pairs == 0: every segment is empty, the counts and the padding are still written)
    const bool floor = min_score > -__builtin_inf();   // no floor: the selection of the unfiltered call
    (floor ? k_tn_select<true> : k_tn_select<false>)<<<dim3((unsigned)((n_query + 3) / 4)), dim3(256), 0, st>>>(
        n_query, n_top, rank_by, S.cand_ptr, S.cand_item, S.plain, S.decay, S.status, out_cnt, out_item, out_plain, out_decay, stats, min_score);
    XM_LAUNCH_CHECK();
    unsigned long long h[4] = {0, 0, 0, 0};
    XM_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = S.n_pairs; h_stats[1] = (int64_t)h[0]; h_stats[2] = S.max_now; h_stats[3] = (int64_t)h[1];
        if (n_stats == 6) { h_stats[4] = (int64_t)h[2]; h_stats[5] = (int64_t)h[3]; }
    }
    return XMAP_OK;
}

extern "C" {

int xmap_topn_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                   int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                   const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                   const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *out_cnt,
                   int32_t *out_item, double *out_plain, double *out_decay, int64_t *h_stats) {
    return topn_rows(stream, n_query, query_user, n_top, rank_by, flags, n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item,
                     prof_rating, prof_time, item_avg, wtab, n_w, out_cnt, out_item, out_plain, out_decay, nullptr, h_stats, 4);
}

int xmap_topn_rows_filtered(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                            int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                            const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                            const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *out_cnt,
                            int32_t *out_item, double *out_plain, double *out_decay, const xmap_rec_filter *F, int64_t *h_stats) {
    return topn_rows(stream, n_query, query_user, n_top, rank_by, flags, n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item,
                     prof_rating, prof_time, item_avg, wtab, n_w, out_cnt, out_item, out_plain, out_decay, F, h_stats, 6);
}
}
