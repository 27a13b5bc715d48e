// stage_e_audience.hip -- the audience of an item on the device: for every query item the N best users among those whose own
// rows give evidence for it, ranked by the unrounded prediction (DESIGN.md 4 "Audience").  The top-N recommendation seen from
// the item: (u, i) is a candidate pair here iff i is a candidate of u in stage_e_topn.hip, and its two scores are the same
// kernel's.  Everything it reads is what the tail leaves resident: user-major profiles, neighbour lists [I][keep], item averages.
//
//   k_au_holders<count | fill> : the item-major transposition of the profiles -- for item n the users whose profile holds n, one
//                     entry per profile row (a user who holds an item twice appears twice) -- by count -> xmap_exclusive_scan ->
//                     fill.  One thread per profile row (its user by bisection of prof_ptr); rows with an item outside [0, I)
//                     are skipped; the order inside a row is whatever the atomics give: the candidate pass de-duplicates
//                     through a bitmap and emits in index order.
//   k_au_candidates : one block per query item, run twice (count, then fill into buffers of exactly the counted size).  The user
//                     space is walked in windows of AU_WINDOW users; an LDS bitmap of the window takes the union of hold[n] over
//                     the item's first min(cnt, keep) neighbours n -- at most 64 rows, each as long as the neighbour is popular,
//                     so the whole block strides one row after the other, coalesced -- the holders of the item itself are
//                     cleared again unless XMAP_AUDIENCE_KEEP_HOLDERS, and the marked users leave in ascending index.  The
//                     bitmap, its summary level, the exclusion clear and the two-pass emit are IdBitmap (id_bitmap.h), shared
//                     with the top-N and the group lists, here with 1024 threads over 2^20 ids: one summary word per thread.
//   scoring         : k_predict_rows<., RAW = true> (predict_rows.h) over the (user, item) candidate list, unchanged.
//   k_au_select     : segmented top-N, one block per query, for segments of up to a million candidates and N up to 1024:
//                     au_select_segment of au_select.h (shared with stage_e_peers.hip) -- the best CAP >= n_top keys sorted in
//                     LDS, the segment streamed through in tiles, survivors staged and re-sorted by a bitonic network.  A key is
//                     (score as an ordered integer, position in the segment): the positions ascend with the user index, keys
//                     are distinct, and the sorted prefix is the same whatever order the survivors were staged in.  Status 2:
//                     dropped and counted.
// Items of an item fold-in (stage_e_itemfold.hip; query items >= n_resident of xmap_itemfold_audience_rows): no profile holds them, their
// holders are the batch's raters -- a second, optional holder CSR that the clear pass of k_au_candidates reads for them.
// xmap_audience_rows_filtered (rec_filter.h; DESIGN.md 4 "Eligibility"): the FILT instantiation of k_au_candidates clears the
// query's exclusion ids in the bitmap and ANDs every emitted word with the user mask -- before anything is scored -- and
// k_au_select drops and counts the candidates below the score floor.
// Every output position follows from the scans, so the result does not depend on the grid or on the order of the atomics.
#include "common.h"
#include "au_select.h"
#include "id_bitmap.h"
#include "predict_rows.h"
#include "rec_filter.h"
#include "two_pass.h"

namespace xmap {

constexpr int AU_WINDOW = 1 << 20;              // users per bitmap pass (128 KB of LDS + 4 KB of summary: one block per CU)
static_assert(AU_WINDOW % 32 == 0, "a window starts at a word of the mask");
constexpr int AU_THREADS = 1024;                // 16 waves stride a holder row; thread t emits summary word t (thread order = user order)
using AuBitmap = IdBitmap<AU_THREADS, 20>;
static_assert(AuBitmap::WINDOW == AU_WINDOW && AuBitmap::PER == 1, "one summary word per thread");
constexpr int AU_MAX_BLOCKS = 512;              // blocks of the candidate pass (grid-stride over the queries: the window is zeroed once per block)
constexpr int AU_ROW_BLOCKS = 2048;             // blocks of the holders pass (grid-stride over the profile rows)

template <bool FILL>
__global__ __launch_bounds__(256) void k_au_holders(long long U, int I, const long long *pptr, const int *pitem, int *hcnt,
                                                    const long long *hptr, int *huser) {
    const long long n_rows = pptr[U];
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (long long)gridDim.x * blockDim.x) {
        const int it = pitem[r];
        if (it < 0 || it >= I) continue;
        long long lo = 0, hi = U;               // the user of row r: the last u with pptr[u] <= r (users without rows are passed over)
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (pptr[mid] <= r) lo = mid; else hi = mid;
        }
        const int at = atomicAdd(&hcnt[it], 1);
        if constexpr (FILL) huser[hptr[it] + at] = (int)lo;
    }
}

// FILT (rec_filter.h): the query's exclusion ids are cleared behind the holders, and a touched word meets its word of the mask
// where it is emitted; the count pass adds what the two removed to *removed.  FILT = false is the unfiltered kernel: it reads
// none of allow, ex_ptr, ex_id.
template <bool FILL, bool FILT>
__global__ __launch_bounds__(AU_THREADS) void k_au_candidates(long long n_query, const int *query_item, long long U, int I, int keep,
                                                              int keep_holders, const int *nb_cnt, const int *nb_col,
                                                              const long long *hptr, const int *huser, int n_resident,
                                                              const long long *new_ptr, const int *new_user, int *cand_cnt,
                                                              const long long *cand_ptr, int *cand_user, int *cand_item,
                                                              const unsigned int *allow, const long long *ex_ptr, const int *ex_id,
                                                              unsigned long long *removed) {
    extern __shared__ unsigned int au_lds[];
    AuBitmap bm(au_lds);
    const int tid = threadIdx.x;
    for (long long q = blockIdx.x; q < n_query; q += gridDim.x) {
        const int it = query_item[q];
        int cnt = (it >= 0 && it < I) ? nb_cnt[it] : 0;
        cnt = cnt < keep ? cnt : keep;
        long long total = 0;
        const long long out0 = FILL ? cand_ptr[q] : 0;
        for (long long lo = 0; lo < U && cnt > 0; lo += AU_WINDOW) {
            // mark: the block strides the holders of one neighbour after the other
            for (int l = 0; l < cnt; l++) {
                const int nb = nb_col[(size_t)it * keep + l];
                if (nb < 0 || nb >= I) continue;        // ignored, as in the prediction
                const long long r1 = hptr[nb + 1];      // (an item of a fold-in batch: no profile holds it, the row is empty)
                for (long long r = hptr[nb] + tid; r < r1; r += AU_THREADS) bm.mark((long long)huser[r] - lo);
            }
            __syncthreads();
            if (!keep_holders) {                // a user who holds the item is no candidate
                const bool nw = new_ptr && it >= n_resident;         // a batch item: its holders are its raters
                const int *hu = nw ? new_user : huser;
                const long long r1 = nw ? new_ptr[it - n_resident + 1] : hptr[it + 1];
                for (long long r = (nw ? new_ptr[it - n_resident] : hptr[it]) + tid; r < r1; r += AU_THREADS) bm.unmark((long long)hu[r] - lo);
                __syncthreads();
            }
            if constexpr (FILT) bm.template exclude<!FILL>(ex_ptr, ex_id, q, U, lo);
            total += bm.template emit<FILL, FILT, FILT>(lo, allow, out0 + total, [&](long long o, long long user) {
                cand_user[o] = (int)user;
                cand_item[o] = it;
            });
        }
        if constexpr (!FILL) {
            if (tid == 0) cand_cnt[q] = (int)total;
        }
    }
    if constexpr (FILT && !FILL) bm.add_gone(removed);
}

// the selection itself is au_select_segment (au_select.h, shared with stage_e_peers.hip); this kernel writes the audience's outputs
// FLOOR: a scored candidate below min_score is dropped and counted; FLOOR = false is the selection of the unfiltered call
template <int CAP, bool FLOOR>
__global__ __launch_bounds__(AU_SEL_THREADS) void k_au_select(long long n_query, int n_top, int rank_by, const long long *cand_ptr,
                                                              const int *cand_user, const double *plain, const double *decay,
                                                              const int *status, int *out_cnt, int *out_user, double *out_plain,
                                                              double *out_decay,
                                                              unsigned long long *stats /*[0] dropped candidates, [1] largest segment,
                                                                                          [2] candidates below the floor*/,
                                                              double min_score) {
    __shared__ unsigned long long K[2 * CAP];
    __shared__ unsigned P[2 * CAP];
    __shared__ int s_staged, s_dropped, s_floored, s_have;
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    if (q >= n_query) return;
    const long long a = cand_ptr[q], b = cand_ptr[q + 1];
    if (tid == 0) { s_dropped = 0; s_floored = 0; s_have = 0; }
    int dropped = 0, floored = 0;
    au_select_segment<CAP, FLOOR>(a, b, n_top, rank_by ? decay : plain, status, min_score, K, P, &s_staged, dropped, floored);
    int have = 0;
    for (int j = tid; j < n_top; j += AU_SEL_THREADS) {
        const size_t o = (size_t)q * n_top + j;
        const unsigned pos = P[j];
        const bool v = pos != AU_NO_POS;
        have += v ? 1 : 0;
        out_user[o] = v ? cand_user[a + pos] : -1;
        out_plain[o] = v ? plain[a + pos] : 0.0;
        out_decay[o] = v ? decay[a + pos] : 0.0;
    }
    if (dropped) atomicAdd(&s_dropped, dropped);
    if constexpr (FLOOR) {
        if (floored) atomicAdd(&s_floored, floored);
    }
    if (have) atomicAdd(&s_have, have);
    __syncthreads();
    if (tid == 0) {
        out_cnt[q] = s_have;
        if (s_dropped) atomicAdd(&stats[0], (unsigned long long)s_dropped);
        if constexpr (FLOOR) {
            if (s_floored) atomicAdd(&stats[2], (unsigned long long)s_floored);
        }
        atomicMax(&stats[1], (unsigned long long)(b - a));
    }
}

template <int CAP>
static void au_select_launch(hipStream_t st, long long n_query, int n_top, int rank_by, const long long *cand_ptr, const int *cand_user,
                             const double *plain, const double *decay, const int *status, int *out_cnt, int *out_user,
                             double *out_plain, double *out_decay, unsigned long long *stats, double min_score) {
    const bool floor = min_score > -__builtin_inf();   // no floor: the selection of the unfiltered call
    (floor ? k_au_select<CAP, true> : k_au_select<CAP, false>)<<<dim3((unsigned)n_query), dim3(AU_SEL_THREADS), 0, st>>>(
        n_query, n_top, rank_by, cand_ptr, cand_user, plain, decay, status, out_cnt, out_user, out_plain, out_decay, stats, min_score);
}

// rec_model.h: xmap_audience_rows (new_ptr == NULL), xmap_itemfold_audience_rows and xmap_audience_rows_filtered (n_stats = 6): the
// items >= n_resident take their holders from the CSR (new_ptr, new_user) -- the raters of a fold-in batch, which no profile holds
int audience_rows(void *stream, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags, const RecModel &M,
                  int32_t *out_cnt, int32_t *out_user, double *out_plain, double *out_decay, int64_t *h_stats, int32_t n_resident,
                  const int64_t *new_ptr, const int32_t *new_user, const xmap_rec_filter *F, int n_stats) {
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    XM_ARG(n_top >= 1 && n_top <= AU_MAX_TOP);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_AUDIENCE_KEEP_HOLDERS) == 0);
    int rc = rec_model_check(M);
    if (rc) return rc;
    XM_ARG(n_query >= 0 && n_query <= 2147483647ll && M.n_users <= 2147483647ll);
    XM_ARG(n_query == 0 || (query_item && out_cnt && out_user && out_plain && out_decay));
    if (h_stats) for (int k = 0; k < n_stats; k++) h_stats[k] = 0;
    bool filt = false;
    double min_score = 0.0;
    rc = rf_prepare(st, n_query, F, &filt, &min_score);         // before any candidate work
    if (rc) return rc;
    if (n_query == 0) return XMAP_OK;
    const int I = M.n_items;
    const long long *pptr = (const long long *)M.prof_ptr;
    // ---- holders: the profiles by item
    int *huser = nullptr;
    long long *hptr = nullptr;
    int64_t n_hold = 0;
    rc = count_scan_fill<true>(
        st, I, &hptr, &n_hold,
        [&](bool fill, int *hcnt, const long long *ptr) {
            if (I > 0 && M.n_users > 0)
                (fill ? k_au_holders<true> : k_au_holders<false>)<<<dim3(AU_ROW_BLOCKS), dim3(256), 0, st>>>(M.n_users, I, pptr, M.prof_item, hcnt,
                                                                                                           ptr, huser);
            return hipGetLastError();
        },
        [&](int64_t n) -> int {
            XM_HIP(xm_malloc_async((void **)&huser, sizeof(int) * (size_t)(n ? n : 1), st));
            return XMAP_OK;
        });
    if (rc) return rc;
    // [0] dropped candidates, [1] largest segment, [2] below the floor, [3] removed by the mask or the exclusion lists
    unsigned long long *stats = nullptr;
    XM_HIP(xm_malloc_async((void **)&stats, sizeof(unsigned long long) * 4, st));
    XM_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long) * 4, st));
    // ---- candidates: count, scan, fill
    int *cand_user = nullptr, *cand_item = nullptr, *status = nullptr;
    long long *cand_ptr = nullptr;
    double *plain = nullptr, *decay = nullptr;
    int64_t n_pairs = 0;
    const unsigned cblocks = (unsigned)(n_query < AU_MAX_BLOCKS ? n_query : AU_MAX_BLOCKS);
    const unsigned int *allow = filt ? (const unsigned int *)F->allow : nullptr;
    const long long *ex_ptr = filt ? (const long long *)F->ex_ptr : nullptr;
    const int *ex_id = filt ? F->ex_id : nullptr;
    rc = count_scan_fill<false>(
        st, n_query, &cand_ptr, &n_pairs,
        [&](bool fill, int *cand_cnt, const long long *ptr) {
            const auto k = fill ? (filt ? k_au_candidates<true, true> : k_au_candidates<true, false>)
                                : (filt ? k_au_candidates<false, true> : k_au_candidates<false, false>);
            return launch_dyn_lds(k, cblocks, AU_THREADS, AuBitmap::LDS_BYTES, st, n_query, query_item, M.n_users, I, M.keep,
                                  flags & XMAP_AUDIENCE_KEEP_HOLDERS, M.nb_cnt, M.nb_col, hptr, huser, n_resident, (const long long *)new_ptr,
                                  new_user, cand_cnt, ptr, cand_user, cand_item, allow, ex_ptr, ex_id, stats + 3);
        },
        [&](int64_t n) -> int {
            if (n == 0) return XMAP_OK;
            const size_t np = (size_t)n;
            XM_HIP(xm_malloc_async((void **)&cand_user, sizeof(int) * np, st));
            XM_HIP(xm_malloc_async((void **)&cand_item, sizeof(int) * np, st));
            XM_HIP(xm_malloc_async((void **)&plain, sizeof(double) * np, st));
            XM_HIP(xm_malloc_async((void **)&decay, sizeof(double) * np, st));
            XM_HIP(xm_malloc_async((void **)&status, sizeof(int) * np, st));
            return XMAP_OK;
        });
    if (rc) return rc;
    // ---- scores: the pair body of the prediction, unrounded
    int32_t max_now = 0;
    if (n_pairs > 0 && (rc = predict_rows_run<true>(st, n_pairs, cand_user, cand_item, M, plain, decay, status, &max_now))) return rc;
    // ---- selection (n_pairs == 0: every segment is empty, the counts and the padding are still written)
    if (n_top <= 256)
        au_select_launch<256>(st, n_query, n_top, rank_by, cand_ptr, cand_user, plain, decay, status, out_cnt, out_user, out_plain, out_decay,
                              stats, min_score);
    else
        au_select_launch<1024>(st, n_query, n_top, rank_by, cand_ptr, cand_user, plain, decay, status, out_cnt, out_user, out_plain,
                               out_decay, stats, min_score);
    XM_LAUNCH_CHECK();
    unsigned long long h[4] = {0, 0, 0, 0};
    XM_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = n_pairs; h_stats[1] = (int64_t)h[0]; h_stats[2] = max_now; h_stats[3] = (int64_t)h[1];
        if (n_stats == 6) { h_stats[4] = (int64_t)h[2]; h_stats[5] = (int64_t)h[3]; }
    }
    return XMAP_OK;
}

}  // namespace xmap
using namespace xmap;

extern "C" {

int xmap_audience_rows(void *stream, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags,
                       int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                       const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                       const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *out_cnt,
                       int32_t *out_user, double *out_plain, double *out_decay, int64_t *h_stats) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    return audience_rows(stream, n_query, query_item, n_top, rank_by, flags, M, out_cnt, out_user, out_plain, out_decay, h_stats, n_items,
                         nullptr, nullptr, nullptr, 4);
}

int xmap_itemfold_audience_rows(void *stream, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags,
                                int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                                const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                                const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *out_cnt,
                                int32_t *out_user, double *out_plain, double *out_decay, int64_t *h_stats, int32_t n_resident,
                                const int64_t *new_ptr, const int32_t *new_user) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    XM_ARG(n_resident >= 0 && n_resident <= n_items && (n_resident == n_items || new_ptr));
    return audience_rows(stream, n_query, query_item, n_top, rank_by, flags, M, out_cnt, out_user, out_plain, out_decay, h_stats, n_resident,
                         new_ptr, new_user, nullptr, 4);
}

int xmap_audience_rows_filtered(void *stream, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags,
                                int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                                const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                                const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *out_cnt,
                                int32_t *out_user, double *out_plain, double *out_decay, int32_t n_resident, const int64_t *new_ptr,
                                const int32_t *new_user, const xmap_rec_filter *F, int64_t *h_stats) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    if (!new_ptr) n_resident = n_items;         // resident items only
    XM_ARG(n_resident >= 0 && n_resident <= n_items);
    return audience_rows(stream, n_query, query_item, n_top, rank_by, flags, M, out_cnt, out_user, out_plain, out_decay, h_stats, n_resident,
                         new_ptr, new_user, F, 6);
}
}
