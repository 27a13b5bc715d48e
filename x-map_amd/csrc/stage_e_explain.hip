// stage_e_explain.hip -- why an item is recommended: for (user, item) pairs, typically the lists of xmap_topn_rows, the
// strongest evidence entries of the score and, for each of those AlterEgo rows, the raw ratings stage C made it from
// (DESIGN.md 4 "Explain").  Everything it reads is resident after generate and rec_select.
//
//   k_explain_rows    : predict_pair<., RAW, EXPLAIN> (predict_rows.h) -- the pair body of the prediction itself with its explain
//                       mode on: the evidence list, p1, d1, now, the time ranks and the status are the prediction's own, not a
//                       copy; on top of them the share of every entry and n_ev rounds of a wave-wide arg-max.  One wave per
//                       pair, four waves per block (7.5 KB of LDS per wave); more than PR_CAP entries: the arena launch, 8
//                       doubles per entry.
//   k_explain_sources : one wave per (pair, reported entry): the user's RAW profile streams through the wave 64 entries at a
//                       time; a ballot of the matches and the running count give src_total and the first n_src positions.  A
//                       pass-through row (its offset in the profile is below cnt_t[u]) is the same walk with the test
//                       `flags & 2` and a target rank.  No atomics: every output position follows from the counts.
//                       One wave rather than a 16-lane group per entry: the work items are pairs x n_ev, far more than the
//                       device holds waves, so nothing idles for want of items, and the wave form has one path for every
//                       profile length (a group form needs a second kernel or a serial tail for profiles beyond 16 entries).
#include "common.h"
#include "predict_rows.h"

namespace xmap {

template <bool ARENA>
__global__ __launch_bounds__(64 * PR_WAVES) void k_explain_rows(
    long long w_base, long long n_work, const int *tu, const int *ti, long long U, int I, int keep, const int *nb_cnt, const int *nb_col,
    const double *nb_sim, const long long *pptr, const int *pitem, const double *prating, const long long *ptime,
    const double *avg, const double *wtab, int n_w, int *status, int *max_now, unsigned long long *ovf, long long *ovf_list,
    double *arena, ExplainOut X) {
    predict_pair<ARENA, true, true>(w_base, n_work, tu, ti, U, I, keep, nb_cnt, nb_col, nb_sim, pptr, pitem, prating, ptime, avg, wtab, n_w,
                                    nullptr, nullptr, status, max_now, ovf, ovf_list, arena, X);
}

constexpr int XS_WAVES = 4;

__global__ __launch_bounds__(64 * XS_WAVES) void k_explain_sources(
    long long w_base, long long n_work, const int *pair_user, int n_ev, const int *ex_cnt, const long long *ex_row, long long U, int I,
    const long long *pptr, const int *pitem, const int *cnt_t, const long long *off_t, const long long *rptr, const int *ritem,
    const uint8_t *flags, const int *map, int n_src, int *src_total, long long *src_pos) {
    const int lane = lane_id();
    const long long w = w_base + (long long)blockIdx.x * XS_WAVES + (threadIdx.x >> 6);     // the launch covers [w_base, n_work)
    if (w >= n_work) return;
    const long long t = w / n_ev;
    const int e = (int)(w - t * n_ev);
    long long *pos = src_pos + (size_t)w * n_src;
    int total = 0, written = 0;
    if (e < ex_cnt[t]) {
        const int u = pair_user[t];
        const long long p = ex_row[w];
        total = -1;
        if (u >= 0 && u < U && p >= pptr[u] && p < pptr[u + 1]) {
            const long long k = p - pptr[u];
            const long long ct = cnt_t ? (long long)cnt_t[u] : off_t[u + 1] - off_t[u];
            const bool pass = k < ct;               // a pass-through row: the k-th raw entry of a target item
            const int tgt = pitem[p];
            const long long ra = rptr[u], rb = rptr[u + 1];
            long long seen = 0;                     // matches before this chunk
            for (long long r = ra; r < rb; r += 64) {
                int it = -1;
                if (r + lane < rb) it = ritem[r + lane];
                bool hit = false;
                if (it >= 0 && it < I) hit = pass ? (flags[it] & 2) != 0 : map[it] == tgt;
                const unsigned long long hm = __ballot(hit);
                const long long rank = seen + __popcll(hm & lanemask_lt());
                if (pass) {
                    if (hit && rank == k && n_src > 0) pos[0] = r + lane;
                } else if (hit && rank < n_src) {
                    pos[rank] = r + lane;
                }
                seen += __popcll(hm);
                if (pass && seen > k) break;
            }
            total = pass ? (seen > k ? 1 : 0) : (int)(seen < 2147483647ll ? seen : 2147483647ll);
            written = total < n_src ? total : n_src;
        }
    }
    if (lane == 0) src_total[w] = total;
    if (lane >= written && lane < n_src) pos[lane] = -1;
}

// rec_model.h: the body of xmap_explain_rows.  The tables are asked for only when there is a pair to explain.
int explain_rows(void *stream, int64_t n_pairs, const int32_t *pair_user, const int32_t *pair_item, int32_t rank_by, int32_t n_ev,
                 const RecModel &M, int32_t *ex_status, int32_t *ex_total, int32_t *ex_cnt, double *ex_score, int64_t *ex_row,
                 int32_t *ex_slot, double *ex_share, int32_t *h_max_now) {
    XM_ARG(n_ev >= 1 && n_ev <= EX_MAX_EV);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG(n_pairs >= 0 && M.n_users >= 0 && M.n_items >= 0 && M.keep >= 1 && M.keep <= 64 && M.n_w >= 1 && M.wtab && M.prof_ptr);
    XM_ARG(n_pairs == 0 || (pair_user && pair_item && M.nb_cnt && M.nb_col && M.nb_sim && M.item_avg));
    XM_ARG(n_pairs == 0 || (ex_status && ex_total && ex_cnt && ex_score && ex_row && ex_slot && ex_share));
    XM_ARG(M.n_users == 0 || (M.prof_item && M.prof_rating && M.prof_time));
    hipStream_t st = (hipStream_t)stream;
    ExplainOut X;
    X.rank_by = rank_by; X.n_ev = n_ev; X.total = ex_total; X.cnt = ex_cnt; X.score = ex_score; X.row = (long long *)ex_row;
    X.slot = ex_slot; X.share = ex_share;
    return pair_rows_run(st, n_pairs, 8, h_max_now, [&](bool in_arena, dim3 grid, long long w_base, long long n_work, int *max_now,
                                                        unsigned long long *ctl, long long *ovf_list, double *arena) {
        auto k = in_arena ? k_explain_rows<true> : k_explain_rows<false>;
        k<<<grid, dim3(64 * PR_WAVES), 0, st>>>(w_base, n_work, pair_user, pair_item, M.n_users, M.n_items, M.keep, M.nb_cnt, M.nb_col,
                                                M.nb_sim, (const long long *)M.prof_ptr, M.prof_item, M.prof_rating,
                                                (const long long *)M.prof_time, M.item_avg, M.wtab, M.n_w, ex_status, max_now, ctl,
                                                ovf_list, arena, X);
    });
}

}  // namespace xmap
using namespace xmap;

extern "C" {

int xmap_explain_rows(void *stream, int64_t n_pairs, const int32_t *pair_user, const int32_t *pair_item, int32_t rank_by,
                      int32_t n_ev, int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                      const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                      const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *ex_status,
                      int32_t *ex_total, int32_t *ex_cnt, double *ex_score, int64_t *ex_row, int32_t *ex_slot, double *ex_share,
                      int32_t *h_max_now) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    return explain_rows(stream, n_pairs, pair_user, pair_item, rank_by, n_ev, M, ex_status, ex_total, ex_cnt, ex_score, ex_row, ex_slot,
                        ex_share, h_max_now);
}

int xmap_explain_sources(void *stream, int64_t n_pairs, const int32_t *pair_user, int32_t n_ev, const int32_t *ex_cnt,
                         const int64_t *ex_row, int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                         const int32_t *cnt_t, const int64_t *off_t, const int64_t *raw_ptr, const int32_t *raw_item,
                         const uint8_t *flags, const int32_t *map_src2tgt, int32_t n_src, int32_t *src_total, int64_t *src_pos) {
    XM_ARG(n_ev >= 1 && n_ev <= EX_MAX_EV);
    XM_ARG(n_src >= 1 && n_src <= EX_MAX_SRC);
    XM_ARG(n_pairs >= 0 && n_users >= 0 && n_items >= 0 && prof_ptr && raw_ptr);
    XM_ARG((cnt_t != nullptr) != (off_t != nullptr));          // exactly one of the two
    XM_ARG(n_pairs == 0 || (pair_user && ex_cnt && ex_row && src_total && src_pos));
    XM_ARG(n_users == 0 || n_pairs == 0 || (prof_item && raw_item && flags && map_src2tgt));
    if (n_pairs == 0) return XMAP_OK;
    const long long n_work = (long long)n_pairs * n_ev;
    return for_pair_ranges(n_work, XS_WAVES, [&](long long base, long long end, dim3 grid) {      // one wave per (pair, entry): in ranges
        k_explain_sources<<<grid, dim3(64 * XS_WAVES), 0, (hipStream_t)stream>>>(
            base, end, pair_user, n_ev, ex_cnt, (const long long *)ex_row, n_users, n_items, (const long long *)prof_ptr, prof_item, cnt_t,
            (const long long *)off_t, (const long long *)raw_ptr, raw_item, flags, map_src2tgt, n_src, src_total, (long long *)src_pos);
    });
}
}
