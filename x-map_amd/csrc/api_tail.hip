// api_tail.hip -- the coarse ABI of the recommender tail (api.hip has the map of the calls): the neighbour lists over the
// RecommenderSim rows, then predictions, top-N lists and audiences over the three sources (the resident AlterEgo profiles, a
// fold-in batch of users, the extended tables of an item fold-in), the two fold-ins themselves, explanations, the union of
// other contexts' rows and the hold-out evaluation of top-N.  The lists that re-rank or combine these are api_lists.hip's.
#include <vector>

#include "ctx.h"

extern "C" {

static int alloc_neighbors(xmap_ctx *c, int keep) {
    drop_ifold(c);              // the extended tables copy the lists
    c->p_nb.release();
    c->have_nb = false;
    const size_t m = (size_t)(c->R.n_items ? c->R.n_items : 1) * keep;
    XM_ALLOCZ(c->p_nb, c->nb_cnt, c->R.n_items ? c->R.n_items : 1);
    XM_ALLOCZ(c->p_nb, c->nb_col, m); XM_ALLOCZ(c->p_nb, c->nb_sim, m); XM_ALLOCZ(c->p_nb, c->nb_ls, m);
    c->keep = keep;
    return XMAP_OK;
}

int xmap_ctx_rec_select(xmap_ctx *c, int keep) {
    XM_ARG(c && c->have_rec && keep >= 1 && keep <= 64);
    XM_HIP(hipSetDevice(c->device));
    XM_TRY(alloc_neighbors(c, keep));
    if (c->rec_pairs > 0)
        XM_TRY(xmap_rec_select(c->st, c->R.n_items, c->rs_row_ptr, c->rs_col, c->rs_sim, c->rs_ls, keep, c->nb_cnt, c->nb_col, c->nb_sim,
                               c->nb_ls));
    XM_HIP(hipStreamSynchronize(c->st));
    c->have_nb = true;
    return XMAP_OK;
}

int xmap_ctx_rec_set_neighbors(xmap_ctx *c, int keep, const int32_t *cnt, const int32_t *col, const double *sim) {
    XM_ARG(c && c->have_rec && keep >= 1 && keep <= 64 && cnt && col && sim);
    XM_HIP(hipSetDevice(c->device));
    const int I = c->R.n_items;
    for (int i = 0; i < I; i++) {
        XM_ARG(cnt[i] <= keep);
        for (int t = 0; t < cnt[i]; t++) XM_ARG(col[(size_t)i * keep + t] >= 0 && col[(size_t)i * keep + t] < I);
    }
    XM_TRY(alloc_neighbors(c, keep));
    const size_t m = (size_t)I * keep;
    if (I) {
        XM_HIP(hipMemcpyAsync(c->nb_cnt, cnt, sizeof(int32_t) * (size_t)I, hipMemcpyHostToDevice, c->st));
        XM_HIP(hipMemcpyAsync(c->nb_col, col, sizeof(int32_t) * m, hipMemcpyHostToDevice, c->st));
        XM_HIP(hipMemcpyAsync(c->nb_sim, sim, sizeof(double) * m, hipMemcpyHostToDevice, c->st));
    }
    XM_HIP(hipStreamSynchronize(c->st));
    c->have_nb = true;
    return XMAP_OK;
}

int xmap_ctx_rec_neighbors_download(xmap_ctx *c, int32_t *cnt, int32_t *col, double *sim, double *ls) {
    XM_ARG(c && c->have_rec && c->have_nb);
    XM_HIP(hipSetDevice(c->device));
    const size_t I = (size_t)c->R.n_items, m = I * (size_t)c->keep;
    if (cnt) XM_TRY(d2h(cnt, (const int32_t *)c->nb_cnt, I, c->st));
    if (col) XM_TRY(d2h(col, (const int32_t *)c->nb_col, m, c->st));
    if (sim) XM_TRY(d2h(sim, (const double *)c->nb_sim, m, c->st));
    if (ls) XM_TRY(d2h(ls, (const double *)c->nb_ls, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

static int predict_over(xmap_ctx *c, const Profiles &P, const Tables &T, int64_t n_test, const int32_t *test_user, const int32_t *test_item,
                        const double *test_rating, const double *wtab, int32_t n_w, double *out_plain, double *out_decay,
                        int32_t *status, double *mae, int32_t *max_now) {
    XM_ARG(n_test >= 0 && wtab && n_w >= 1 && (n_test == 0 || (test_user && test_item && out_plain && out_decay && status)));
    XM_ARG(!mae || test_rating || n_test == 0);
    XM_HIP(hipSetDevice(c->device));
    if (max_now) *max_now = 0;
    if (mae) mae[0] = mae[1] = mae[2] = 0.0;
    if (n_test == 0) return XMAP_OK;
    CoarseCall io(c);
    int32_t *d_user, *d_item, *d_status;
    double *d_real = nullptr, *d_w, *d_plain, *d_decay, *d_mae;
    const size_t n = (size_t)n_test;
    XM_TRY(io.in(&d_user, test_user, n)); XM_TRY(io.in(&d_item, test_item, n));
    XM_TRY(io.in(&d_w, wtab, (size_t)n_w));
    if (test_rating) XM_TRY(io.in(&d_real, test_rating, n));
    XM_TRY(io.out(&d_plain, out_plain, n, true)); XM_TRY(io.out(&d_decay, out_decay, n, true));
    XM_TRY(io.out(&d_status, status, n, true)); XM_TRY(io.scratch(&d_mae, 3, true));
    XM_TRY(predict_rows(c->st, n_test, d_user, d_item, rec_model(P, T, d_w, n_w), d_plain, d_decay, d_status, max_now));
    if (mae) {
        XM_TRY(xmap_mae(c->st, n_test, d_status, d_real, d_plain, d_decay, d_mae));
        io.back(mae, d_mae, 3);
    }
    return io.finish();
}

// n_stats = 4: the unfiltered entry (F is NULL); 6: the filtered one
static int recommend_over(xmap_ctx *c, const Profiles &P, const Tables &T, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by,
                          int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_item, double *out_plain,
                          double *out_decay, int64_t *stats, const xmap_rec_filter *F = nullptr, int n_stats = 4) {
    XM_ARG(n_top >= 1 && n_top <= 64);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay)));
    XM_TRY(check_filter(F, n_query));
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < n_stats; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    CoarseCall io(c);
    TopnLists L;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(filtered_topn(io, P, T, n_query, query_user, n_top, rank_by, flags, wtab, n_w, F, stats, n_stats, &L));
    io.back(out_cnt, L.cnt, n); io.back(out_item, L.item, m); io.back(out_plain, L.plain, m); io.back(out_decay, L.decay, m);
    return io.finish();
}

static int audience_over(xmap_ctx *c, const Profiles &P, const Tables &T, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by,
                         int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user, double *out_plain,
                         double *out_decay, int64_t *stats, const xmap_rec_filter *F = nullptr, int n_stats = 4) {
    XM_ARG(n_top >= 1 && n_top <= 1024);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_AUDIENCE_KEEP_HOLDERS) == 0);
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_item && out_cnt && out_user && out_plain && out_decay)));
    XM_TRY(check_filter(F, n_query));
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < n_stats; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    CoarseCall io(c);
    int32_t *d_item, *d_cnt, *d_user;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(io.in(&d_item, query_item, n));
    XM_TRY(io.in(&d_w, wtab, (size_t)n_w));
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_user, out_user, m));
    XM_TRY(io.out(&d_plain, out_plain, m)); XM_TRY(io.out(&d_decay, out_decay, m));
    xmap_rec_filter D;
    if (n_stats == 6) XM_TRY(upload_filter(io, F, n_query, P.n_users, &D));
    XM_TRY(audience_rows(c->st, n_query, d_item, n_top, rank_by, flags, rec_model(P, T, d_w, n_w), d_cnt, d_user, d_plain, d_decay, stats,
                         T.n_resident, T.new_ptr, T.new_user, n_stats == 6 ? &D : nullptr, n_stats));
    return io.finish();
}

int xmap_ctx_predict(xmap_ctx *c, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const double *test_rating,
                     const double *wtab, int32_t n_w, double *out_plain, double *out_decay, int32_t *status, double *mae,
                     int32_t *max_now) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    return predict_over(c, resident_profiles(c), resident_tables(c),
                        n_test, test_user, test_item, test_rating, wtab, n_w, out_plain, out_decay, status, mae,
                        max_now);
}

int xmap_ctx_recommend(xmap_ctx *c, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                       const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay,
                       int64_t *stats) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    return recommend_over(c, resident_profiles(c), resident_tables(c),
                          n_query, query_user, n_top, rank_by, flags, wtab, n_w, out_cnt, out_item, out_plain,
                          out_decay, stats);
}

int xmap_ctx_audience(xmap_ctx *c, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags,
                      const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user, double *out_plain, double *out_decay,
                      int64_t *stats) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    return audience_over(c, resident_profiles(c), resident_tables(c),
                         n_query, query_item, n_top, rank_by, flags, wtab, n_w, out_cnt, out_user, out_plain,
                         out_decay, stats);
}

// ---- fold-in ------------------------------------------------------------------------------------------------------------

int xmap_ctx_foldin(xmap_ctx *c, int64_t n_new, const int64_t *ptr, const int32_t *item, const float *rating, const int64_t *time,
                    int64_t *counts) {
    XM_ARG(c && c->have_gen && !c->is_union && n_new >= 0 && ptr);
    // the batch is checked here, on the host: bad input starts no device work (xmap_foldin_count's own check then passes)
    if (ptr[0] != 0) { set_error("fold-in batch: ptr[0] = %lld, not 0", (long long)ptr[0]); return XMAP_ERR_ARG; }
    for (int64_t u = 0; u < n_new; u++)
        if (ptr[u + 1] < ptr[u]) { set_error("fold-in batch: ptr[%lld] < ptr[%lld]", (long long)u + 1, (long long)u); return XMAP_ERR_ARG; }
    const int64_t nnz = ptr[n_new];
    XM_ARG(nnz < 2147483647ll && (nnz == 0 || (item && rating && time)));
    const int I = c->R.n_items;
    for (int64_t e = 0; e < nnz; e++)
        if (item[e] < 0 || item[e] >= I) {
            set_error("fold-in batch: item[%lld] = %d outside [0, %d)", (long long)e, (int)item[e], I);
            return XMAP_ERR_ARG;
        }
    XM_HIP(hipSetDevice(c->device));
    // built beside the previous batch, which is replaced only when everything has succeeded
    ScratchPool tmp, fresh;
    int64_t *d_ptr, *d_time, *f_ptr, *f_time, h[3] = {0, 0, 0};
    int32_t *d_item, *cnt_t, *cnt_m, *f_item;
    float *d_rating;
    double *f_rating;
    // the raw ptr / item and the pass-through counts stay with the batch: the sources of an explanation walk them
    XM_TRY(h2d(fresh, &d_ptr, ptr, (size_t)n_new + 1, c->st));
    XM_TRY(h2d(fresh, &d_item, item, (size_t)nnz, c->st));
    XM_TRY(h2d(tmp, &d_rating, rating, (size_t)nnz, c->st));
    XM_TRY(h2d(tmp, &d_time, time, (size_t)nnz, c->st));
    XM_TRY(dalloc(fresh, &cnt_t, (size_t)n_new, c->st)); XM_TRY(dalloc(tmp, &cnt_m, (size_t)n_new, c->st));
    XM_TRY(dalloc(fresh, &f_ptr, (size_t)n_new + 1, c->st));
    XM_TRY(xmap_foldin_count(c->st, n_new, nnz, d_ptr, d_item, I, c->R.flags, c->g_map, cnt_t, cnt_m, f_ptr, h));
    XM_TRY(dalloc(fresh, &f_item, (size_t)h[0], c->st)); XM_TRY(dalloc(fresh, &f_rating, (size_t)h[0], c->st));
    XM_TRY(dalloc(fresh, &f_time, (size_t)h[0], c->st));
    XM_TRY(xmap_foldin_fill(c->st, n_new, nnz, d_ptr, d_item, d_rating, d_time, I, c->R.flags, c->g_map, cnt_t, f_ptr, f_item, f_rating,
                            f_time));
    XM_HIP(hipStreamSynchronize(c->st));
    drop_fold(c);
    c->p_fold.ptrs.swap(fresh.ptrs);
    c->f_users = n_new; c->f_rows = h[0];
    c->f_ptr = f_ptr; c->f_item = f_item; c->f_rating = f_rating; c->f_time = f_time;
    c->f_raw_ptr = d_ptr; c->f_raw_item = d_item; c->f_cnt_t = cnt_t;
    c->have_fold = true;
    if (counts) { counts[0] = h[0]; counts[1] = h[1]; counts[2] = h[2]; }
    return XMAP_OK;
}

int xmap_ctx_foldin_download(xmap_ctx *c, int64_t *prof_ptr, int32_t *prof_item, double *prof_rating, int64_t *prof_time) {
    XM_ARG(c && c->have_fold);
    XM_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)c->f_rows;
    if (prof_ptr) XM_TRY(d2h(prof_ptr, (const int64_t *)c->f_ptr, (size_t)c->f_users + 1, c->st));
    if (prof_item) XM_TRY(d2h(prof_item, (const int32_t *)c->f_item, n, c->st));
    if (prof_rating) XM_TRY(d2h(prof_rating, (const double *)c->f_rating, n, c->st));
    if (prof_time) XM_TRY(d2h(prof_time, (const int64_t *)c->f_time, n, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

int xmap_ctx_foldin_recommend(xmap_ctx *c, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                              const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_item, double *out_plain,
                              double *out_decay, int64_t *stats) {
    XM_ARG(c && c->have_gen && c->have_fold && c->have_rec && c->have_nb);
    return recommend_over(c, foldin_profiles(c), resident_tables(c),
                          n_query, query_user, n_top, rank_by, flags, wtab, n_w, out_cnt, out_item, out_plain,
                          out_decay, stats);
}

int xmap_ctx_foldin_audience(xmap_ctx *c, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags,
                             const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user, double *out_plain,
                             double *out_decay, int64_t *stats) {
    XM_ARG(c && c->have_gen && c->have_fold && c->have_rec && c->have_nb);
    return audience_over(c, foldin_profiles(c), resident_tables(c),
                         n_query, query_item, n_top, rank_by, flags, wtab, n_w, out_cnt, out_user, out_plain,
                         out_decay, stats);
}

int xmap_ctx_foldin_predict(xmap_ctx *c, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const double *test_rating,
                            const double *wtab, int32_t n_w, double *out_plain, double *out_decay, int32_t *status, double *mae,
                            int32_t *max_now) {
    XM_ARG(c && c->have_gen && c->have_fold && c->have_rec && c->have_nb);
    return predict_over(c, foldin_profiles(c), resident_tables(c),
                        n_test, test_user, test_item, test_rating, wtab, n_w, out_plain, out_decay, status, mae,
                        max_now);
}

// ---- item fold-in -------------------------------------------------------------------------------------------------------

int xmap_ctx_item_foldin(xmap_ctx *c, int64_t n_new, const int64_t *ptr, const int32_t *user, const double *rating, int64_t *counts) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb && n_new >= 0 && ptr);
    // the batch is checked here, on the host: bad input starts no device work (xmap_itemfold_count's own check then passes)
    if (ptr[0] != 0) { set_error("item fold-in batch: ptr[0] = %lld, not 0", (long long)ptr[0]); return XMAP_ERR_ARG; }
    for (int64_t q = 0; q < n_new; q++)
        if (ptr[q + 1] < ptr[q]) { set_error("item fold-in batch: ptr[%lld] < ptr[%lld]", (long long)q + 1, (long long)q); return XMAP_ERR_ARG; }
    const int64_t nnz = ptr[n_new];
    const int I = c->R.n_items;
    const int64_t U = c->R.n_users;
    XM_ARG(nnz < 2147483647ll && (nnz == 0 || (user && rating)) && (int64_t)I + n_new <= 2147483647ll);
    for (int64_t e = 0; e < nnz; e++)
        if (user[e] < 0 || user[e] >= U) {
            set_error("item fold-in batch: user[%lld] = %d outside [0, %lld)", (long long)e, (int)user[e], (long long)U);
            return XMAP_ERR_ARG;
        }
    XM_HIP(hipSetDevice(c->device));
    // built beside the previous batch, which is replaced only when everything has succeeded
    ScratchPool tmp, fresh;
    const int keep = c->keep;
    const size_t n1 = (size_t)n_new, x1 = (size_t)I + n1;
    int64_t *d_ptr, *row_ptr, h[3] = {0, 0, 0};
    int32_t *d_user, *cnt, *col, *nij, *x_cnt, *x_col;
    double *d_rating, *sim, *ls, *norm, *x_sim, *x_ls, *x_avg;
    XM_TRY(h2d(fresh, &d_ptr, ptr, n1 + 1, c->st));
    XM_TRY(h2d(fresh, &d_user, user, (size_t)nnz, c->st));
    XM_TRY(h2d(tmp, &d_rating, rating, (size_t)nnz, c->st));
    XM_TRY(dalloc(tmp, &cnt, n1, c->st));
    XM_TRY(dalloc(fresh, &row_ptr, n1 + 1, c->st));
    XM_TRY(xmap_itemfold_count(c->st, n_new, nnz, d_ptr, d_user, U, I, c->pf_ptr, c->pf_item, 0, cnt, row_ptr, h));
    const size_t np = (size_t)h[0];
    XM_TRY(dalloc(fresh, &col, np, c->st)); XM_TRY(dalloc(fresh, &sim, np, c->st)); XM_TRY(dalloc(fresh, &ls, np, c->st));
    XM_TRY(dalloc(fresh, &nij, np, c->st)); XM_TRY(dalloc(fresh, &norm, n1, c->st));
    // the extended tables: the resident rows, then the batch's (the fill pass and the selection write them in place)
    XM_TRY(dalloc(fresh, &x_cnt, x1, c->st, true)); XM_TRY(dalloc(fresh, &x_col, x1 * keep, c->st, true));
    XM_TRY(dalloc(fresh, &x_sim, x1 * keep, c->st, true)); XM_TRY(dalloc(fresh, &x_ls, x1 * keep, c->st, true));
    XM_TRY(dalloc(fresh, &x_avg, x1, c->st, true));
    if (I) {
        const size_t m = (size_t)I * keep;
        XM_HIP(hipMemcpyAsync(x_cnt, c->nb_cnt, sizeof(int32_t) * (size_t)I, hipMemcpyDeviceToDevice, c->st));
        XM_HIP(hipMemcpyAsync(x_col, c->nb_col, sizeof(int32_t) * m, hipMemcpyDeviceToDevice, c->st));
        XM_HIP(hipMemcpyAsync(x_sim, c->nb_sim, sizeof(double) * m, hipMemcpyDeviceToDevice, c->st));
        XM_HIP(hipMemcpyAsync(x_ls, c->nb_ls, sizeof(double) * m, hipMemcpyDeviceToDevice, c->st));
        XM_HIP(hipMemcpyAsync(x_avg, c->rs_avg, sizeof(double) * (size_t)I, hipMemcpyDeviceToDevice, c->st));
    }
    XM_TRY(xmap_itemfold_fill(c->st, n_new, nnz, d_ptr, d_user, d_rating, U, I, c->pf_ptr, c->pf_item, c->pf_rating, c->rs_norm, c->rec_cap, 0,
                              row_ptr, col, sim, ls, nij, x_avg + I, norm));
    if (h[0] > 0)
        XM_TRY(xmap_rec_select(c->st, (int32_t)n_new, row_ptr, col, sim, ls, keep, x_cnt + I, x_col + (size_t)I * keep,
                               x_sim + (size_t)I * keep, x_ls + (size_t)I * keep));
    XM_HIP(hipStreamSynchronize(c->st));
    drop_ifold(c);
    c->p_ifold.ptrs.swap(fresh.ptrs);
    c->if_new = n_new; c->if_pairs = h[0];
    c->if_ptr = d_ptr; c->if_user = d_user; c->if_row_ptr = row_ptr;
    c->if_col = col; c->if_sim = sim; c->if_ls = ls; c->if_nij = nij; c->if_norm = norm;
    c->x_cnt = x_cnt; c->x_col = x_col; c->x_sim = x_sim; c->x_ls = x_ls; c->x_avg = x_avg;
    c->have_ifold = true;
    if (counts) { counts[0] = h[0]; counts[1] = h[1]; counts[2] = h[2]; }
    return XMAP_OK;
}

int xmap_ctx_item_foldin_download(xmap_ctx *c, int64_t *row_ptr, int32_t *col, double *sim, double *ls, int32_t *nij, double *avg,
                                  double *norm, int32_t *nb_cnt, int32_t *nb_col, double *nb_sim, double *nb_ls) {
    XM_ARG(c && c->have_ifold);
    XM_HIP(hipSetDevice(c->device));
    const size_t I = (size_t)c->R.n_items, n1 = (size_t)c->if_new, np = (size_t)c->if_pairs, m = n1 * (size_t)c->keep, o = I * (size_t)c->keep;
    if (row_ptr) XM_TRY(d2h(row_ptr, (const int64_t *)c->if_row_ptr, n1 + 1, c->st));
    if (col) XM_TRY(d2h(col, (const int32_t *)c->if_col, np, c->st));
    if (sim) XM_TRY(d2h(sim, (const double *)c->if_sim, np, c->st));
    if (ls) XM_TRY(d2h(ls, (const double *)c->if_ls, np, c->st));
    if (nij) XM_TRY(d2h(nij, (const int32_t *)c->if_nij, np, c->st));
    if (avg) XM_TRY(d2h(avg, (const double *)(c->x_avg + I), n1, c->st));
    if (norm) XM_TRY(d2h(norm, (const double *)c->if_norm, n1, c->st));
    if (nb_cnt) XM_TRY(d2h(nb_cnt, (const int32_t *)(c->x_cnt + I), n1, c->st));
    if (nb_col) XM_TRY(d2h(nb_col, (const int32_t *)(c->x_col + o), m, c->st));
    if (nb_sim) XM_TRY(d2h(nb_sim, (const double *)(c->x_sim + o), m, c->st));
    if (nb_ls) XM_TRY(d2h(nb_ls, (const double *)(c->x_ls + o), m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

// indices into the batch -> items of the extended tables (I + q); an index outside the batch -> -1, an item without a list
static std::vector<int32_t> batch_items(const xmap_ctx *c, int64_t n, const int32_t *item) {
    std::vector<int32_t> out((size_t)(item ? n : 0));
    for (size_t k = 0; k < out.size(); k++) out[k] = (item[k] >= 0 && item[k] < c->if_new) ? c->R.n_items + item[k] : -1;
    return out;
}

int xmap_ctx_item_foldin_audience(xmap_ctx *c, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags,
                                  const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user, double *out_plain,
                                  double *out_decay, int64_t *stats) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb && c->have_ifold && n_query >= 0);
    const std::vector<int32_t> q = batch_items(c, n_query, query_item);
    return audience_over(c, resident_profiles(c), itemfold_tables(c), n_query, query_item ? q.data() : nullptr, n_top, rank_by, flags, wtab,
                         n_w, out_cnt, out_user, out_plain, out_decay, stats);
}

int xmap_ctx_item_foldin_predict(xmap_ctx *c, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const double *test_rating,
                                 const double *wtab, int32_t n_w, double *out_plain, double *out_decay, int32_t *status, double *mae,
                                 int32_t *max_now) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb && c->have_ifold && n_test >= 0);
    const std::vector<int32_t> t = batch_items(c, n_test, test_item);
    return predict_over(c, resident_profiles(c), itemfold_tables(c), n_test, test_user, test_item ? t.data() : nullptr, test_rating, wtab,
                        n_w, out_plain, out_decay, status, mae, max_now);
}

int xmap_ctx_item_foldin_recommend(xmap_ctx *c, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                                   const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_item, double *out_plain,
                                   double *out_decay, int64_t *stats) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb && c->have_ifold);
    return recommend_over(c, resident_profiles(c), itemfold_tables(c), n_query, query_user, n_top, rank_by, flags, wtab, n_w, out_cnt,
                          out_item, out_plain, out_decay, stats);
}

// ---- eligibility: one filtered entry per direction, over the three sources ------------------------------------------------

int xmap_ctx_recommend_filtered(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by,
                                int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_item, double *out_plain,
                                double *out_decay, const xmap_rec_filter *F, int64_t *stats) {
    Source S;
    XM_TRY(check_source("xmap_ctx_recommend_filtered", source, true));
    XM_TRY(resolve_source("xmap_ctx_recommend_filtered", c, source, true, &S));
    return recommend_over(c, S.P, S.T, n_query, query_user, n_top, rank_by, flags, wtab, n_w, out_cnt, out_item, out_plain, out_decay, stats,
                          F, 6);
}

int xmap_ctx_audience_filtered(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by,
                               int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user, double *out_plain,
                               double *out_decay, const xmap_rec_filter *F, int64_t *stats) {
    Source S;
    XM_TRY(check_source("xmap_ctx_audience_filtered", source, true));
    XM_TRY(resolve_source("xmap_ctx_audience_filtered", c, source, true, &S));
    std::vector<int32_t> q;
    if (source == XMAP_SRC_ITEM_FOLDIN) {       // query_item = indices into the batch
        XM_ARG(n_query >= 0);
        q = batch_items(c, n_query, query_item);
        if (query_item) query_item = q.data();
    }
    return audience_over(c, S.P, S.T, n_query, query_item, n_top, rank_by, flags, wtab, n_w, out_cnt, out_user, out_plain, out_decay, stats,
                         F, 6);
}

// ---- explanations -------------------------------------------------------------------------------------------------------

// the raw profiles a set of AlterEgo profiles was made from, with the count (or the scan) of each profile's pass-through rows
struct RawProfiles {
    const int64_t *ptr;
    const int32_t *item, *cnt_t;
    const int64_t *off_t;
};

static int explain_over(xmap_ctx *c, const Profiles &P, const RawProfiles &W, int64_t n_pairs, const int32_t *pair_user,
                        const int32_t *pair_item, int32_t rank_by, int32_t n_ev, int32_t n_src, const double *wtab, int32_t n_w,
                        int32_t *ex_status, int32_t *ex_total, int32_t *ex_cnt, double *ex_score, int64_t *ex_row, int32_t *ex_slot,
                        double *ex_share, int32_t *src_total, int64_t *src_pos, int32_t *max_now) {
    XM_ARG(n_ev >= 1 && n_ev <= 16);
    XM_ARG(n_src >= 0 && n_src <= 8);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_pairs >= 0 && (n_pairs == 0 || (pair_user && pair_item)));
    XM_ARG(n_pairs == 0 || (ex_status && ex_total && ex_cnt && ex_score && ex_row && ex_slot && ex_share));
    XM_ARG(n_pairs == 0 || n_src == 0 || (src_total && src_pos));
    if (n_src > 0 && c->is_union) {
        set_error("explain with n_src > 0 on a union context: a union of AlterEgo rows has one replacement map and one raw profile "
                  "per part, so a row has no single source; call with n_src = 0 (evidence only)");
        return XMAP_ERR_ARG;
    }
    XM_HIP(hipSetDevice(c->device));
    if (max_now) *max_now = 0;
    if (n_pairs == 0) return XMAP_OK;
    CoarseCall io(c);
    int32_t *d_user, *d_item, *d_status, *d_total, *d_cnt, *d_slot, *d_stotal = nullptr;
    int64_t *d_row, *d_spos = nullptr;
    double *d_w, *d_score, *d_share;
    const size_t n = (size_t)n_pairs, m = n * (size_t)n_ev;
    XM_TRY(io.in(&d_user, pair_user, n)); XM_TRY(io.in(&d_item, pair_item, n));
    XM_TRY(io.in(&d_w, wtab, (size_t)n_w));
    XM_TRY(io.out(&d_status, ex_status, n)); XM_TRY(io.out(&d_total, ex_total, n)); XM_TRY(io.out(&d_cnt, ex_cnt, n));
    XM_TRY(io.out(&d_score, ex_score, n));
    XM_TRY(io.out(&d_row, ex_row, m)); XM_TRY(io.out(&d_slot, ex_slot, m)); XM_TRY(io.out(&d_share, ex_share, m));
    XM_TRY(explain_rows(c->st, n_pairs, d_user, d_item, rank_by, n_ev, rec_model(P, resident_tables(c), d_w, n_w), d_status, d_total, d_cnt,
                        d_score, d_row, d_slot, d_share, max_now));
    if (n_src > 0) {
        XM_TRY(io.out(&d_stotal, src_total, m)); XM_TRY(io.out(&d_spos, src_pos, m * (size_t)n_src));
        XM_TRY(xmap_explain_sources(c->st, n_pairs, d_user, n_ev, d_cnt, d_row, P.n_users, c->R.n_items, P.ptr, P.item, W.cnt_t, W.off_t,
                                    W.ptr, W.item, c->R.flags, c->g_map, n_src, d_stotal, d_spos));
    }
    return io.finish();
}

int xmap_ctx_explain(xmap_ctx *c, int64_t n_pairs, const int32_t *pair_user, const int32_t *pair_item, int32_t rank_by, int32_t n_ev,
                     int32_t n_src, const double *wtab, int32_t n_w, int32_t *ex_status, int32_t *ex_total, int32_t *ex_cnt,
                     double *ex_score, int64_t *ex_row, int32_t *ex_slot, double *ex_share, int32_t *src_total, int64_t *src_pos,
                     int32_t *max_now) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    const RawProfiles W = c->is_union ? RawProfiles{nullptr, nullptr, nullptr, nullptr}
                                      : RawProfiles{c->R.user_ptr, c->R.user_item, nullptr, c->g_off_t};
    return explain_over(c, resident_profiles(c), W, n_pairs, pair_user, pair_item, rank_by, n_ev, n_src, wtab, n_w, ex_status, ex_total,
                        ex_cnt, ex_score, ex_row, ex_slot, ex_share, src_total, src_pos, max_now);
}

int xmap_ctx_foldin_explain(xmap_ctx *c, int64_t n_pairs, const int32_t *pair_user, const int32_t *pair_item, int32_t rank_by,
                            int32_t n_ev, int32_t n_src, const double *wtab, int32_t n_w, int32_t *ex_status, int32_t *ex_total,
                            int32_t *ex_cnt, double *ex_score, int64_t *ex_row, int32_t *ex_slot, double *ex_share, int32_t *src_total,
                            int64_t *src_pos, int32_t *max_now) {
    XM_ARG(c && c->have_gen && c->have_fold && c->have_rec && c->have_nb);
    const RawProfiles W{c->f_raw_ptr, c->f_raw_item, c->f_cnt_t, nullptr};
    return explain_over(c, foldin_profiles(c), W, n_pairs, pair_user, pair_item, rank_by, n_ev, n_src, wtab, n_w, ex_status, ex_total,
                        ex_cnt, ex_score, ex_row, ex_slot, ex_share, src_total, src_pos, max_now);
}

// ---- multi-domain: the union of other contexts' AlterEgo rows ----------------------------------------------------------

int xmap_ctx_union(xmap_ctx *c, int n_parts, xmap_ctx *const *src, const int32_t *const *user_map, const int32_t *const *item_map,
                   int64_t n_users, int32_t n_items, int flags, int64_t *counts) {
    XM_ARG(c && src && user_map && item_map && n_parts >= 1 && n_parts <= 16 && n_users >= 0 && n_items >= 0);
    XM_ARG((flags & ~XMAP_UNION_DISTINCT) == 0);
    for (int d = 0; d < n_parts; d++) {
        const xmap_ctx *s = src[d];
        if (!s || s == c || !s->have_gen || s->is_union || s->device != c->device) {
            set_error("xmap_ctx_union: source %d must be another context on device %d that holds generated rows", d, c->device);
            return XMAP_ERR_ARG;
        }
        XM_ARG((s->R.n_users == 0 || user_map[d]) && (s->R.n_items == 0 || item_map[d]));
    }
    XM_HIP(hipSetDevice(c->device));
    // built beside whatever dst holds, which is replaced only when everything has succeeded
    ScratchPool tmp, fresh;
    xmap_union_part parts[16];
    memset(parts, 0, sizeof(parts));
    for (int d = 0; d < n_parts; d++) {
        const xmap_ctx *s = src[d];
        int32_t *d_umap, *d_imap;
        XM_TRY(h2d(tmp, &d_umap, user_map[d], (size_t)s->R.n_users, c->st));
        XM_TRY(h2d(tmp, &d_imap, item_map[d], (size_t)s->R.n_items, c->st));
        xmap_union_part &p = parts[d];
        p.n_users = s->R.n_users; p.n_items = s->R.n_items; p.n_rows = s->n_rows; p.n_target_rows = s->n_target_rows;
        p.user = s->g_user; p.item = s->g_item; p.rating = s->g_rating; p.time = s->g_time;
        p.off_t = s->g_off_t; p.off_m = s->g_off_m; p.user_map = d_umap; p.item_map = d_imap;
    }
    int64_t *un_ptr, *un_time, h[4] = {0, 0, 0, 0};
    int32_t *un_item, *d_pre, *d_suf;
    uint32_t *d_mask;
    uint8_t *d_flags;
    double *un_rating;
    const size_t i1 = (size_t)(n_items ? n_items : 1);
    XM_TRY(dalloc(fresh, &un_ptr, (size_t)n_users + 1, c->st, true));
    XM_TRY(xmap_union_count(c->st, n_parts, parts, n_users, n_items, flags, un_ptr, h));
    XM_TRY(dalloc(fresh, &un_item, (size_t)h[0], c->st)); XM_TRY(dalloc(fresh, &un_rating, (size_t)h[0], c->st));
    XM_TRY(dalloc(fresh, &un_time, (size_t)h[0], c->st));
    XM_TRY(xmap_union_fill(c->st, n_parts, parts, n_users, n_items, flags, un_ptr, h[0], un_item, un_rating, un_time));
    // every union item is a target item ("T:" in iid); the other predicates are never asked of a tail-only context
    XM_TRY(dalloc(fresh, &d_pre, i1, c->st, true)); XM_TRY(dalloc(fresh, &d_suf, i1, c->st, true));
    XM_TRY(dalloc(fresh, &d_mask, i1, c->st, true)); XM_TRY(dalloc(fresh, &d_flags, i1, c->st));
    XM_HIP(hipMemsetAsync(d_flags, 2, i1, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    drop_tail(c);
    drop_fold(c);
    drop_union(c);
    drop_labels(c);             // the labels go with the item space
    c->p_gen.release(); c->p_ext.release(); c->p_sim.release(); c->p_ratings.release();
    c->have_ratings = c->have_sim = c->have_ext = false;
    c->p_union.ptrs.swap(fresh.ptrs);
    memset(&c->R, 0, sizeof(c->R));
    c->R.n_users = n_users; c->R.n_items = n_items;
    c->R.prefix_cls = d_pre; c->R.suffix_cls = d_suf; c->R.contains_mask = d_mask; c->R.flags = d_flags;
    c->un_ptr = un_ptr; c->un_item = un_item; c->un_rating = un_rating; c->un_time = un_time;
    c->n_rows = c->n_target_rows = h[0];
    c->g_user = c->g_item = nullptr; c->g_rating = nullptr; c->g_time = nullptr; c->g_off_t = c->g_off_m = nullptr; c->g_map = nullptr;
    c->is_union = true;
    c->have_gen = true;
    if (counts) memcpy(counts, h, sizeof(h));
    return XMAP_OK;
}

int xmap_ctx_evaluate_topn(xmap_ctx *c, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const double *test_rating,
                           double rel_min, int32_t n_top, int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t n_cut,
                           const int32_t *cut, const double *dtab, double *agg, int64_t *cover, int32_t *user_nrel, uint64_t *user_mask,
                           int64_t *stats) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(n_top >= 1 && n_top <= 64);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_cut >= 1 && n_cut <= 8 && cut && dtab && agg && cover);
    for (int k = 0; k < n_cut; k++) XM_ARG(cut[k] >= 1 && cut[k] <= n_top && (k == 0 || cut[k] > cut[k - 1]));
    XM_ARG(rel_min == rel_min);
    XM_ARG(n_test >= 0 && (n_test == 0 || (test_user && test_item && test_rating)));
    XM_HIP(hipSetDevice(c->device));
    const size_t U = (size_t)c->R.n_users;
    for (int k = 0; k < n_cut * 8; k++) agg[k] = 0.0;
    for (int k = 0; k < n_cut; k++) cover[k] = 0;
    if (user_nrel) memset(user_nrel, 0, sizeof(int32_t) * U);
    if (user_mask) memset(user_mask, 0, sizeof(uint64_t) * U);
    if (stats) memset(stats, 0, sizeof(int64_t) * 8);
    if (n_test == 0 || U == 0) return XMAP_OK;
    CoarseCall io(c);
    int32_t *d_tu, *d_ti, *d_nrel, *d_eval;
    double *d_tr;
    const size_t n = (size_t)n_test;
    XM_TRY(io.in(&d_tu, test_user, n)); XM_TRY(io.in(&d_ti, test_item, n)); XM_TRY(io.in(&d_tr, test_rating, n));
    XM_TRY(io.scratch(&d_nrel, U)); XM_TRY(io.scratch(&d_eval, U));
    int64_t counts[4] = {0, 0, 0, 0};
    XM_TRY(xmap_eval_users(c->st, n_test, d_tu, d_ti, d_tr, rel_min, c->R.n_users, c->R.n_items, d_nrel, d_eval, counts));
    if (stats) memcpy(stats, counts, sizeof(counts));
    if (user_nrel) io.back(user_nrel, d_nrel, U);
    const size_t Q = (size_t)counts[0], m = Q * (size_t)n_top;
    if (Q == 0) return io.finish();
    // ---- the lists of the users with relevant pairs: they stay on the device (the queries are there already: not filtered_topn)
    int32_t *d_cnt, *d_item;
    double *d_w, *d_dtab, *d_plain, *d_decay, *d_agg;
    uint64_t *d_mask;
    int64_t *d_cover;
    XM_TRY(io.in(&d_w, wtab, (size_t)n_w)); XM_TRY(io.in(&d_dtab, dtab, (size_t)n_top));
    XM_TRY(io.scratch(&d_cnt, Q)); XM_TRY(io.scratch(&d_item, m));
    XM_TRY(io.scratch(&d_plain, m)); XM_TRY(io.scratch(&d_decay, m));
    XM_TRY(io.scratch(&d_mask, Q)); XM_TRY(io.out(&d_agg, agg, (size_t)n_cut * 8));
    XM_TRY(io.out(&d_cover, cover, (size_t)n_cut));
    XM_TRY(topn_rows(c->st, (int64_t)Q, d_eval, n_top, rank_by, flags, rec_model(resident_profiles(c), resident_tables(c), d_w, n_w), d_cnt,
                     d_item, d_plain, d_decay, nullptr, stats ? stats + 4 : nullptr, 4));
    XM_TRY(xmap_topn_eval(c->st, n_test, d_tu, d_ti, d_tr, rel_min, c->R.n_users, c->R.n_items, d_nrel, (int64_t)Q, d_eval, n_top, d_cnt,
                          d_item, n_cut, cut, d_dtab, d_mask, nullptr, d_agg, d_cover));
    if (user_mask) {                // per user, from the per-query masks
        std::vector<uint64_t> h_mask(Q);
        std::vector<int32_t> h_eval(Q);
        XM_TRY(d2h(h_mask.data(), (const uint64_t *)d_mask, Q, c->st));
        XM_TRY(d2h(h_eval.data(), (const int32_t *)d_eval, Q, c->st));
        XM_HIP(hipStreamSynchronize(c->st));
        for (size_t q = 0; q < Q; q++) user_mask[h_eval[q]] = h_mask[q];
    }
    return io.finish();
}
}
