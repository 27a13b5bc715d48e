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
//                     XMAP_TOPN_KEEP_HELD, and the marked items leave in ascending index.  The bitmap, its summary level, the
//                     exclusion clear and the two-pass emit are IdBitmap (id_bitmap.h), shared with the audience and the group
//                     lists; the kernel holds its query loop, its mark loop, the un-mark of the held items and its writer.
//   scoring         : k_predict_rows<., RAW = true> (predict_rows.h) over the (user, item) candidate list: the pair body of the
//                     prediction itself, the values before bound_rating.  More than PR_CAP evidence entries: its arena launch.
//   k_tn_select     : segmented top-N, one wave per query: lane j holds the j-th best (score desc, item asc) seen so far; the
//                     segment streams through 64 candidates at a time, a candidate that beats the current N-th is inserted by
//                     a ballot count and a one-lane shift.  Candidates with status 2 are dropped and counted.
// xmap_topn_rows_filtered (rec_filter.h; DESIGN.md 4 "Eligibility"): the FILT instantiation of k_tn_candidates clears the query's
// exclusion ids in the bitmap and ANDs every emitted word with the item mask -- before anything is scored -- and k_tn_select
// drops and counts the candidates below the score floor.
// The call is two halves: tn_score_candidates (reverse lists, candidates, scores; declared in topn_pass.h, which also holds k_tn_rev
// and the window geometry) and the selection.  The group lists (stage_e_group.hip) run the first half over their flattened
// member list.  Both sizing passes go through count_scan_fill (two_pass.h); the model travels as a RecModel (rec_model.h).
// Every output position follows from the scans, so the result does not depend on the grid or on the order of the atomics.
#include "common.h"
#include "predict_rows.h"
#include "rec_filter.h"
#include "topn_pass.h"
#include "two_pass.h"

namespace xmap {

constexpr int TN_WINDOW = 1 << 19;              // items per bitmap pass (64 KB of LDS; two blocks per CU)
static_assert(TN_WINDOW == 1 << TN_WINDOW_LOG2, "the window of topn_pass.h, which stage_e_group.hip shares");
static_assert(TN_WINDOW % 32 == 0, "a window starts at a word of the mask");

// FILT (rec_filter.h): the query's exclusion ids are cleared behind the held items, and a touched word meets its word of the
// mask where it is emitted; the count pass adds what the two removed to *removed.  FILT = false is the unfiltered kernel: it
// reads none of allow, ex_ptr, ex_id.
template <bool FILL, bool FILT>
__global__ __launch_bounds__(TN_THREADS) void k_tn_candidates(long long n_query, const int *query_user, long long U, int I, int keep_held,
                                                              const long long *rptr, const int *ritem, const long long *pptr,
                                                              const int *pitem, int *cand_cnt, const long long *cand_ptr,
                                                              int *cand_user, int *cand_item, const unsigned int *allow,
                                                              const long long *ex_ptr, const int *ex_id, unsigned long long *removed) {
    extern __shared__ unsigned int tn_lds[];
    TnBitmap bm(tn_lds);
    const int tid = threadIdx.x;
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
                for (long long r = rptr[it] + (tid & 15); r < r1; r += 16) bm.mark((long long)ritem[r] - lo);
            }
            __syncthreads();
            if (!keep_held) {                   // an item the user holds is no candidate
                for (long long p = a + tid; p < b; p += TN_THREADS) bm.unmark((long long)pitem[p] - lo);
                __syncthreads();
            }
            if constexpr (FILT) bm.template exclude<!FILL>(ex_ptr, ex_id, q, I, lo);
            total += bm.template emit<FILL, FILT, FILT>(lo, allow, out0 + total, [&](long long o, long long item) {
                cand_user[o] = u;
                cand_item[o] = (int)item;
            });
        }
        if constexpr (!FILL) {
            if (tid == 0) cand_cnt[q] = (int)total;
        }
    }
    if constexpr (FILT && !FILL) bm.add_gone(removed);
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

// topn_pass.h: the candidate-and-scoring half, shared with the member pass of the group lists (stage_e_group.hip)
int tn_score_candidates(hipStream_t st, int64_t n_query, const int32_t *query_user, int32_t flags, const RecModel &M, bool filt,
                        const unsigned int *allow, const long long *ex_ptr, const int *ex_id, unsigned long long *removed, TnScored *out) {
    const int I = M.n_items, keep = M.keep;
    // ---- reverse neighbour lists
    int *ritem = nullptr;
    long long *rptr = nullptr;
    int64_t n_rev = 0;
    const unsigned rev_blocks = (unsigned)(((long long)I * keep + 255) / 256);
    int rc = count_scan_fill<true>(
        st, I, &rptr, &n_rev,
        [&](bool fill, int *rcnt, const long long *ptr) {
            if (I > 0) (fill ? k_tn_rev<true> : k_tn_rev<false>)<<<dim3(rev_blocks), dim3(256), 0, st>>>(I, keep, M.nb_cnt, M.nb_col, rcnt, ptr, ritem);
            return hipGetLastError();
        },
        [&](int64_t n) -> int {
            XM_HIP(xm_malloc_async((void **)&ritem, sizeof(int) * (size_t)(n ? n : 1), st));
            return XMAP_OK;
        });
    if (rc) return rc;
    // ---- candidates: count, scan, fill
    int *cand_user = nullptr;
    const unsigned cblocks = (unsigned)(n_query < TN_MAX_BLOCKS ? n_query : TN_MAX_BLOCKS);
    rc = count_scan_fill<false>(
        st, n_query, &out->cand_ptr, &out->n_pairs,
        [&](bool fill, int *cand_cnt, const long long *cand_ptr) {
            const auto k = fill ? (filt ? k_tn_candidates<true, true> : k_tn_candidates<true, false>)
                                : (filt ? k_tn_candidates<false, true> : k_tn_candidates<false, false>);
            return launch_dyn_lds(k, cblocks, TN_THREADS, TnBitmap::LDS_BYTES, st, n_query, query_user, M.n_users, I, flags & XMAP_TOPN_KEEP_HELD,
                                  rptr, ritem, (const long long *)M.prof_ptr, M.prof_item, cand_cnt, cand_ptr, cand_user, out->cand_item, allow,
                                  ex_ptr, ex_id, removed);
        },
        [&](int64_t n) -> int {
            if (n == 0) return XMAP_OK;
            const size_t np = (size_t)n;
            XM_HIP(xm_malloc_async((void **)&cand_user, sizeof(int) * np, st));
            XM_HIP(xm_malloc_async((void **)&out->cand_item, sizeof(int) * np, st));
            XM_HIP(xm_malloc_async((void **)&out->plain, sizeof(double) * np, st));
            XM_HIP(xm_malloc_async((void **)&out->decay, sizeof(double) * np, st));
            XM_HIP(xm_malloc_async((void **)&out->status, sizeof(int) * np, st));
            return XMAP_OK;
        });
    if (rc || out->n_pairs == 0) return rc;
    // ---- scores: the pair body of the prediction, unrounded
    return predict_rows_run<true>(st, out->n_pairs, cand_user, out->cand_item, M, out->plain, out->decay, out->status, &out->max_now);
}

// rec_model.h: xmap_topn_rows (F == NULL, n_stats = 4) and xmap_topn_rows_filtered (n_stats = 6)
int topn_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags, const RecModel &M,
              int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, const xmap_rec_filter *F, int64_t *h_stats,
              int n_stats) {
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    XM_ARG(n_top >= 1 && n_top <= TN_MAX_TOP);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    int rc = rec_model_check(M);
    if (rc) return rc;
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay)));
    if (h_stats) for (int k = 0; k < n_stats; k++) h_stats[k] = 0;
    bool filt = false;
    double min_score = 0.0;
    rc = rf_prepare(st, n_query, F, &filt, &min_score);         // before any candidate work
    if (rc) return rc;
    if (n_query == 0) return XMAP_OK;
    // [0] dropped candidates, [1] largest segment, [2] below the floor, [3] removed by the mask or the exclusion lists
    unsigned long long *stats = nullptr;
    XM_HIP(xm_malloc_async((void **)&stats, sizeof(unsigned long long) * 4, st));
    XM_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long) * 4, st));
    TnScored S;
    rc = tn_score_candidates(st, n_query, query_user, flags, M, filt, filt ? (const unsigned int *)F->allow : nullptr,
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

}  // namespace xmap
using namespace xmap;

extern "C" {

int xmap_topn_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                   int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                   const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                   const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *out_cnt,
                   int32_t *out_item, double *out_plain, double *out_decay, int64_t *h_stats) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    return topn_rows(stream, n_query, query_user, n_top, rank_by, flags, M, out_cnt, out_item, out_plain, out_decay, nullptr, h_stats, 4);
}

int xmap_topn_rows_filtered(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                            int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                            const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                            const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *out_cnt,
                            int32_t *out_item, double *out_plain, double *out_decay, const xmap_rec_filter *F, int64_t *h_stats) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    return topn_rows(stream, n_query, query_user, n_top, rank_by, flags, M, out_cnt, out_item, out_plain, out_decay, F, h_stats, 6);
}
}
