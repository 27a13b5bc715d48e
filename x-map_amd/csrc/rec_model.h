// rec_model.h -- the model the recommender tail reads, as ONE value inside the library: user-major profiles, neighbour lists
// [n_items][keep], item averages and the decay table.  The fine-grained extern "C" entries (include/xmap_hip.h) take these as
// 13 separate arguments; each builds a RecModel from them on its first line -- the fields stand in the order of those
// arguments -- and everything below an entry takes the struct, as do the coarse calls of api_tail.hip and api_lists.hip,
// which build it once per call from their profiles and tables (ctx.h).  Host code only: the kernels keep their parameter lists.
#ifndef XMAP_REC_MODEL_H
#define XMAP_REC_MODEL_H
#include "common.h"

namespace xmap {

struct RecModel {
    int64_t n_users;
    int32_t n_items, keep;
    const int32_t *nb_cnt, *nb_col;     // [n_items], [n_items][keep]
    const double *nb_sim;               // [n_items][keep]
    const int64_t *prof_ptr;            // [n_users + 1]
    const int32_t *prof_item;
    const double *prof_rating;
    const int64_t *prof_time;
    const double *item_avg;             // [n_items]
    const double *wtab;                 // [n_w]
    int32_t n_w;
};

// what the ranking calls (top-N, audience, group lists) ask of a model before any device work
static inline int rec_model_check(const RecModel &M) {
    XM_ARG(M.n_w >= 1 && M.wtab);
    XM_ARG(M.n_users >= 0 && M.n_items >= 0 && M.keep >= 1 && M.keep <= 64 && M.prof_ptr);
    XM_ARG(M.n_items == 0 || (M.nb_cnt && M.nb_col && M.nb_sim && M.item_avg));
    XM_ARG(M.n_users == 0 || (M.prof_item && M.prof_rating && M.prof_time));
    return XMAP_OK;
}

// The bodies of the fine-grained entries, which the coarse calls of api_tail.hip and api_lists.hip share.  Pointers are device
// pointers; the arguments, outputs, h_stats and sync points are those of the entry of the same name in include/xmap_hip.h.
// stage_e_rows.hip: xmap_predict_rows
int predict_rows(void *stream, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const RecModel &M, double *out_plain,
                 double *out_decay, int32_t *status, int32_t *h_max_now);
// stage_e_topn.hip: xmap_topn_rows (F == NULL, n_stats = 4) and xmap_topn_rows_filtered (n_stats = 6)
int topn_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags, const RecModel &M,
              int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, const xmap_rec_filter *F, int64_t *h_stats,
              int n_stats);
// stage_e_audience.hip: xmap_audience_rows (new_ptr == NULL, n_resident = n_items), xmap_itemfold_audience_rows and
// xmap_audience_rows_filtered (n_stats = 6): the items >= n_resident take their holders from the CSR (new_ptr, new_user) -- the
// raters of a fold-in batch, which no profile holds
int audience_rows(void *stream, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags, const RecModel &M,
                  int32_t *out_cnt, int32_t *out_user, double *out_plain, double *out_decay, int64_t *h_stats, int32_t n_resident,
                  const int64_t *new_ptr, const int32_t *new_user, const xmap_rec_filter *F, int n_stats);
// stage_e_group.hip: xmap_group_topn_rows
int group_topn_rows(void *stream, int64_t n_groups, const int64_t *grp_ptr, const int32_t *grp_user, int32_t n_top, int32_t rank_by,
                    int32_t flags, int32_t how, double veto, const RecModel &M, int32_t *out_cnt, int32_t *out_item, double *out_plain,
                    double *out_decay, int32_t *out_low, const xmap_rec_filter *F, int64_t *h_stats);
// stage_e_explain.hip: xmap_explain_rows
int explain_rows(void *stream, int64_t n_pairs, const int32_t *pair_user, const int32_t *pair_item, int32_t rank_by, int32_t n_ev,
                 const RecModel &M, int32_t *ex_status, int32_t *ex_total, int32_t *ex_cnt, double *ex_score, int64_t *ex_row,
                 int32_t *ex_slot, double *ex_share, int32_t *h_max_now);

// stage_e_shelf.hip: xmap_shelf_rows; the label table and the outputs of a shelf call travel as two values (device pointers)
struct ShelfLabels {
    int32_t n_labels;
    const int64_t *lab_ptr;             // [n_items + 1]
    const int32_t *lab_id;
    const uint32_t *lab_allow;          // (n_labels + 31) / 32 words, or NULL
};
struct ShelfOut {
    int32_t *nshelf, *label;            // [Q], [Q][n_shelf]
    double *sscore;                     // [Q][n_shelf]
    int32_t *size, *cnt, *item;         // [Q][n_shelf] twice, [Q][n_shelf][n_top]
    double *plain, *decay;              // [Q][n_shelf][n_top]
};
int shelf_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags, const RecModel &M,
               const ShelfLabels &L, int32_t n_shelf, int32_t shelf_by, int32_t min_fill, int64_t max_records, const ShelfOut &O,
               const xmap_rec_filter *F, int64_t *h_stats);
// the host checks of the shelf calls, shared with xmap_ctx_recommend_shelves: each names its argument; nothing is written
int shelf_check_args(const char *who, int64_t n_query, int32_t n_shelf, int32_t n_top, int32_t rank_by, int32_t flags, int32_t shelf_by,
                     int32_t min_fill, int32_t n_labels, int64_t max_records);
// the device check of a label table over n_items items (lab_ptr[0] == 0, non-decreasing; ids in range, strictly ascending inside an
// item), shared with xmap_ctx_set_labels; *n_lab = lab_ptr[n_items].  Synchronises.
int shelf_check_labels(hipStream_t st, const char *who, int32_t n_items, int32_t n_labels, const int64_t *lab_ptr, const int32_t *lab_id,
                       int64_t *n_lab);

// stage_e_quota.hip: xmap_quota_rows; the mode arguments and the outputs of a quota call travel as two values (device pointers)
struct QuotaRule {
    int32_t mode, cap;
    const int32_t *lab_cap;             // [n_labels], or NULL
    const uint32_t *lab_weight;         // [n_labels], or NULL
};
struct QuotaOut {
    int32_t *cnt, *item;                // [Q], [Q][n_top]
    double *plain, *decay;              // [Q][n_top]
    int32_t *pos, *label;               // [Q][n_top]
};
int quota_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t n_top, int32_t rank_by, int32_t flags,
               const RecModel &M, const QuotaRule &R, const ShelfLabels &L, const QuotaOut &O, const xmap_rec_filter *F, int64_t *h_stats);
// the host checks of the quota calls, shared with xmap_ctx_recommend_quota: each names its argument; nothing is written
int quota_check_args(const char *who, int64_t n_query, int32_t n_pool, int32_t n_top, int32_t rank_by, int32_t flags, int32_t mode,
                     int32_t cap, bool has_lab_cap, int32_t n_labels);

// stage_e_allot.hip: xmap_allot_rows; the outputs of an allot call travel as one value (device pointers)
struct AllotOut {
    int32_t *cnt, *item;                // [Q], [Q][n_top]
    double *plain, *decay;              // [Q][n_top]
    int32_t *pos, *taken;               // [Q][n_top], [n_items] or NULL
};
int allot_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t n_top, int32_t rank_by, int32_t flags,
               const RecModel &M, int32_t cap, const int32_t *item_cap, const AllotOut &O, const xmap_rec_filter *F, int64_t *h_stats);
// the host checks of the allot calls, shared with xmap_ctx_recommend_allot: each names its argument; nothing is written
int allot_check_args(const char *who, int64_t n_query, int32_t n_pool, int32_t max_pool, int32_t n_top, int32_t rank_by, int32_t flags,
                     int32_t cap, bool has_item_cap);

}  // namespace xmap
#endif
