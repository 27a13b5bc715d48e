// api_lists.hip -- the coarse ABI of the calls that re-rank or combine lists (api.hip has the map of the calls): group lists,
// diversified lists, peers and the user-kNN calls over them, related items, the popularity ranking and lists completed with it,
// the label table with shelves and quotas over it, allotment under item capacities, and fused and hybrid lists.  Each entry is
// host checks, one CoarseCall of transfers and the bodies of stage_e_*.hip; the sources are ctx.h's (check_source / resolve_source).
#include <algorithm>
#include <vector>

#include "ctx.h"

extern "C" {

// ---- group lists: one list for several users, over the three sources --------------------------------------------------------------

int xmap_ctx_recommend_group(xmap_ctx *c, int32_t source, int64_t n_groups, const int64_t *grp_ptr, const int32_t *grp_user, int32_t n_top,
                             int32_t rank_by, int32_t flags, int32_t how, double veto, const double *wtab, int32_t n_w, int32_t *out_cnt,
                             int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_low, const xmap_rec_filter *F,
                             int64_t *stats) {
    // the host checks: before any device work, the outputs untouched, the context as it was
    XM_ARG(how == XMAP_GROUP_MEAN || how == XMAP_GROUP_MIN || how == XMAP_GROUP_MAX);
    XM_ARG(veto == veto);                       // NaN
    XM_ARG(n_top >= 1 && n_top <= 64);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_groups >= 0 && (n_groups == 0 || (grp_ptr && out_cnt && out_item && out_plain && out_decay && out_low)));
    if (n_groups > 0 && grp_ptr[0] != 0) { set_error("groups: grp_ptr[0] = %lld, not 0", (long long)grp_ptr[0]); return XMAP_ERR_ARG; }
    for (int64_t g = 0; g < n_groups; g++) {
        const int64_t m = grp_ptr[g + 1] - grp_ptr[g];
        if (m < 0) { set_error("groups: grp_ptr[%lld] < grp_ptr[%lld]", (long long)g + 1, (long long)g); return XMAP_ERR_ARG; }
        if (m > XMAP_GROUP_MAX_MEMBERS) {
            set_error("groups: group %lld has %lld members, more than %d", (long long)g, (long long)m, XMAP_GROUP_MAX_MEMBERS);
            return XMAP_ERR_ARG;
        }
    }
    const int64_t n_mem = n_groups > 0 ? grp_ptr[n_groups] : 0;
    if (n_mem > 0 && !grp_user) { set_error("groups: grp_ptr lists %lld members, grp_user is NULL", (long long)n_mem); return XMAP_ERR_ARG; }
    XM_TRY(check_source("xmap_ctx_recommend_group", source, true));
    XM_TRY(check_filter(F, n_groups));
    Source S;
    XM_TRY(resolve_source("xmap_ctx_recommend_group", c, source, true, &S));
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 8; k++) stats[k] = 0;
    if (n_groups == 0) return XMAP_OK;
    CoarseCall io(c);
    int64_t *d_ptr;
    int32_t *d_user = nullptr, *d_cnt, *d_item, *d_low;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_groups, m = n * (size_t)n_top;
    XM_TRY(io.in(&d_ptr, grp_ptr, n + 1));
    if (n_mem > 0) XM_TRY(io.in(&d_user, grp_user, (size_t)n_mem));
    XM_TRY(io.in(&d_w, wtab, (size_t)n_w));
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_item, out_item, m)); XM_TRY(io.out(&d_plain, out_plain, m));
    XM_TRY(io.out(&d_decay, out_decay, m)); XM_TRY(io.out(&d_low, out_low, m));
    xmap_rec_filter D;
    XM_TRY(upload_filter(io, F, n_groups, S.T.n_items, &D));
    XM_TRY(group_topn_rows(c->st, n_groups, d_ptr, d_user, n_top, rank_by, flags, how, veto, rec_model(S.P, S.T, d_w, n_w), d_cnt, d_item,
                           d_plain, d_decay, d_low, &D, stats));
    return io.finish();
}

// ---- diversified lists: the filtered top-N with n_top = n_pool into device temporaries, then the re-ranking ----------------------

int xmap_ctx_recommend_diverse(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t n_top,
                               int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, double weight, const xmap_rec_filter *F,
                               int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, double *out_pen,
                               double *out_ils, int64_t *stats) {
    // the host checks: before any device work, the outputs untouched, the context as it was
    XM_ARG(weight >= 0.0 && weight <= 1.7976931348623157e308);      // finite and >= 0 (a NaN fails both)
    XM_ARG(n_pool >= 1 && n_pool <= 64);
    XM_ARG(n_top >= 1 && n_top <= n_pool);
    XM_TRY(check_source("xmap_ctx_recommend_diverse", source, false));      // the rows of batch items are not part of the index
    Source S;
    XM_TRY(resolve_source("xmap_ctx_recommend_diverse", c, source, true, &S));
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay && out_pen && out_ils)));
    XM_TRY(check_filter(F, n_query));
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 8; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    const int32_t I = c->R.n_items;
    if (!c->have_div) {
        c->p_div.release();
        XM_ALLOC(c->p_div, c->dv_col, c->rec_pairs); XM_ALLOC(c->p_div, c->dv_abs, c->rec_pairs);
        int64_t dups = 0;
        XM_TRY(xmap_div_index(c->st, I, c->rec_pairs, c->rs_row_ptr, c->rs_col, c->rs_sim, c->dv_col, c->dv_abs, &dups));
        c->have_div = true;
    }
    CoarseCall io(c);
    TopnLists L;                // the pool
    int32_t *d_cnt, *d_item, *d_pos;
    double *d_plain, *d_decay, *d_pen, *d_ils;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_item, out_item, m)); XM_TRY(io.scratch(&d_pos, m));
    XM_TRY(io.out(&d_plain, out_plain, m)); XM_TRY(io.out(&d_decay, out_decay, m));
    XM_TRY(io.out(&d_pen, out_pen, m)); XM_TRY(io.out(&d_ils, out_ils, n));
    int64_t h6[6] = {0, 0, 0, 0, 0, 0}, h2[2] = {0, 0};
    XM_TRY(filtered_topn(io, S.P, S.T, n_query, query_user, n_pool, rank_by, flags, wtab, n_w, F, h6, 6, &L));
    XM_TRY(xmap_diversify_rows(c->st, n_query, n_pool, L.cnt, L.item, L.plain, L.decay, rank_by, weight, n_top, I, c->rs_row_ptr,
                               c->dv_col, c->dv_abs, d_cnt, d_item, d_plain, d_decay, d_pos, d_pen, d_ils, h2));
    XM_TRY(io.finish());
    if (stats) { for (int k = 0; k < 6; k++) stats[k] = h6[k]; stats[6] = h2[0]; stats[7] = h2[1]; }
    return XMAP_OK;
}

// ---- peers: the users most like a query user, over the resident profiles or a fold-in batch ---------------------------------------

// the context's peer index of centring z (0 raw ratings, 1 centred by rs_avg): built on first use
static int peer_index_of(xmap_ctx *c, int z) {
    if (c->have_peer[z]) return XMAP_OK;
    const int32_t I = c->R.n_items;
    const int64_t U = c->R.n_users;
    c->p_peer[z].release();
    XM_ALLOC(c->p_peer[z], c->pr_hd_ptr[z], I + 1); XM_ALLOC(c->p_peer[z], c->pr_hd_user[z], c->n_rows);
    XM_ALLOC(c->p_peer[z], c->pr_hd_x[z], c->n_rows); XM_ALLOC(c->p_peer[z], c->pr_nrm[z], U);
    XM_TRY(xmap_peer_index(c->st, U, I, c->pf_ptr, c->pf_item, c->pf_rating, z ? c->rs_avg : nullptr, c->pr_hd_ptr[z], c->pr_hd_user[z],
                           c->pr_hd_x[z], c->pr_nrm[z], nullptr));
    c->have_peer[z] = true;
    return XMAP_OK;
}

// xmap_ctx_peers (with_ls = false, out_ls unused) and xmap_ctx_peers_ls
static int ctx_peers_run(xmap_ctx *c, bool with_ls, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t flags,
                         int32_t cap, int32_t min_common, int32_t *out_cnt, int32_t *out_user, double *out_sim, int32_t *out_common,
                         double *out_ls, const xmap_rec_filter *F, int64_t *stats) {
    // the host checks: before any device work, the outputs untouched, the context as it was
    XM_ARG(n_top >= 1 && n_top <= 1024);
    XM_ARG(cap >= 1);
    XM_ARG(min_common >= 1);
    XM_ARG((flags & ~(XMAP_PEERS_KEEP_SELF | XMAP_PEERS_CENTRED)) == 0);
    XM_TRY(check_source(with_ls ? "xmap_ctx_peers_ls" : "xmap_ctx_peers", source, false));      // an item fold-in adds items, not users
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_user && out_cnt && out_user && out_sim && out_common)));
    XM_ARG(!with_ls || out_ls);
    XM_TRY(check_filter(F, n_query));
    Source S;
    XM_TRY(resolve_source(with_ls ? "xmap_ctx_peers_ls" : "xmap_ctx_peers", c, source, false, &S));
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 6; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    const int32_t I = c->R.n_items;
    const int64_t U = c->R.n_users;
    const int z = (flags & XMAP_PEERS_CENTRED) ? 1 : 0;
    const double *centre = z ? c->rs_avg : nullptr;
    XM_TRY(peer_index_of(c, z));
    const int32_t fl = (flags & XMAP_PEERS_KEEP_SELF) | (source == XMAP_SRC_RESIDENT ? XMAP_PEERS_SAME : 0);
    CoarseCall io(c);
    int32_t *d_query, *d_cnt, *d_user, *d_common;
    double *d_sim;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(io.in(&d_query, query_user, n));
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_user, out_user, m));
    XM_TRY(io.out(&d_sim, out_sim, m)); XM_TRY(io.out(&d_common, out_common, m));
    xmap_rec_filter D;
    XM_TRY(upload_filter(io, F, n_query, U, &D));
    double *d_ls = nullptr;
    if (with_ls) {
        XM_TRY(io.out(&d_ls, out_ls, m));
        XM_TRY(xmap_peer_rows_ls(c->st, n_query, d_query, S.P.n_users, S.P.ptr, S.P.item, S.P.rating, fl, n_top, cap, min_common, U, I, centre,
                                 c->pr_hd_ptr[z], c->pr_hd_user[z], c->pr_hd_x[z], c->pr_nrm[z], 0, d_cnt, d_user, d_sim, d_common, d_ls,
                                 &D, stats));
    } else
        XM_TRY(xmap_peer_rows(c->st, n_query, d_query, S.P.n_users, S.P.ptr, S.P.item, S.P.rating, fl, n_top, cap, min_common, U, I, centre,
                              c->pr_hd_ptr[z], c->pr_hd_user[z], c->pr_hd_x[z], c->pr_nrm[z], 0, d_cnt, d_user, d_sim, d_common, &D, stats));
    return io.finish();
}

int xmap_ctx_peers(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t flags, int32_t cap,
                   int32_t min_common, int32_t *out_cnt, int32_t *out_user, double *out_sim, int32_t *out_common, const xmap_rec_filter *F,
                   int64_t *stats) {
    return ctx_peers_run(c, false, source, n_query, query_user, n_top, flags, cap, min_common, out_cnt, out_user, out_sim, out_common,
                         nullptr, F, stats);
}

int xmap_ctx_peers_ls(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t flags, int32_t cap,
                      int32_t min_common, int32_t *out_cnt, int32_t *out_user, double *out_sim, int32_t *out_common, double *out_ls,
                      const xmap_rec_filter *F, int64_t *stats) {
    return ctx_peers_run(c, true, source, n_query, query_user, n_top, flags, cap, min_common, out_cnt, out_user, out_sim, out_common,
                         out_ls, F, stats);
}

// ---- user-kNN: predictions and top-N from the peer lists ----------------------------------------------------------------------------

// what the two user-kNN calls share, on the device: the n_nb peers of the queries (xmap_peer_rows without rules), the resident
// means and the queries' own means
struct UknnLists {
    int32_t *query, *cnt, *user;
    double *sim, *user_avg, *query_avg;
    Profiles Q;
};

static int uknn_lists(xmap_ctx *c, CoarseCall &io, int32_t source, const Profiles &Q, int64_t n_query, const int32_t *query_user, int32_t n_nb,
                      int32_t peer_flags, int32_t cap, int32_t min_common, UknnLists *L) {
    const int32_t I = c->R.n_items;
    const int64_t U = c->R.n_users;
    const int z = (peer_flags & XMAP_PEERS_CENTRED) ? 1 : 0;
    XM_TRY(peer_index_of(c, z));
    L->Q = Q;
    const int32_t fl = (peer_flags & XMAP_PEERS_KEEP_SELF) | (source == XMAP_SRC_RESIDENT ? XMAP_PEERS_SAME : 0);
    const size_t n = (size_t)n_query, m = n * (size_t)n_nb;
    int32_t *d_common, *d_ucnt, *d_qcnt;
    XM_TRY(io.in(&L->query, query_user, n));
    XM_TRY(io.scratch(&L->cnt, n)); XM_TRY(io.scratch(&L->user, m));
    XM_TRY(io.scratch(&L->sim, m)); XM_TRY(io.scratch(&d_common, m));
    XM_TRY(xmap_peer_rows(c->st, n_query, L->query, L->Q.n_users, L->Q.ptr, L->Q.item, L->Q.rating, fl, n_nb, cap, min_common, U, I,
                          z ? c->rs_avg : nullptr, c->pr_hd_ptr[z], c->pr_hd_user[z], c->pr_hd_x[z], c->pr_nrm[z], 0, L->cnt, L->user,
                          L->sim, d_common, nullptr, nullptr));
    XM_TRY(io.scratch(&L->user_avg, (size_t)U)); XM_TRY(io.scratch(&d_ucnt, (size_t)U));
    XM_TRY(xmap_uknn_means(c->st, U, I, c->pf_ptr, c->pf_item, c->pf_rating, L->user_avg, d_ucnt));
    const double *src = L->user_avg;
    if (source == XMAP_SRC_FOLDIN) {
        double *d_qavg;
        XM_TRY(io.scratch(&d_qavg, (size_t)L->Q.n_users)); XM_TRY(io.scratch(&d_qcnt, (size_t)L->Q.n_users));
        XM_TRY(xmap_uknn_means(c->st, L->Q.n_users, I, L->Q.ptr, L->Q.item, L->Q.rating, d_qavg, d_qcnt));
        src = d_qavg;
    }
    XM_TRY(io.scratch(&L->query_avg, n));
    XM_TRY(uknn_gather(c->st, n_query, L->query, L->Q.n_users, src, L->query_avg));
    return XMAP_OK;
}

int xmap_ctx_uknn_predict(xmap_ctx *c, int32_t source, int64_t n_test, const int32_t *test_user, const int32_t *test_item,
                          const double *test_rating, int32_t n_nb, int32_t peer_flags, int32_t cap, int32_t min_common, int32_t flags,
                          double *out_score, double *out_bound, int32_t *out_n, int32_t *status, double *mae) {
    // the host checks: before any device work, the outputs untouched, the context as it was
    XM_ARG(n_nb >= 1 && n_nb <= 1024);
    XM_ARG(cap >= 1);
    XM_ARG(min_common >= 1);
    XM_ARG((peer_flags & ~(XMAP_PEERS_KEEP_SELF | XMAP_PEERS_CENTRED)) == 0);
    XM_ARG((flags & ~XMAP_UKNN_OWN_MEAN) == 0);
    XM_TRY(check_source("xmap_ctx_uknn_predict", source, false));       // an item fold-in adds items, not users
    XM_ARG(n_test >= 0 && (n_test == 0 || (test_user && test_item && out_score && out_bound && out_n && status)));
    XM_ARG(!mae || test_rating || n_test == 0);
    Source S;
    XM_TRY(resolve_source("xmap_ctx_uknn_predict", c, source, false, &S));
    XM_HIP(hipSetDevice(c->device));
    if (mae) mae[0] = mae[1] = 0.0;
    if (n_test == 0) return XMAP_OK;
    // the distinct users of the pairs are the queries (ascending); test_q = the pair's position among them
    std::vector<int32_t> users(test_user, test_user + n_test);
    std::sort(users.begin(), users.end());
    users.erase(std::unique(users.begin(), users.end()), users.end());
    std::vector<int32_t> tq((size_t)n_test);
    for (int64_t t = 0; t < n_test; t++) tq[(size_t)t] = (int32_t)(std::lower_bound(users.begin(), users.end(), test_user[t]) - users.begin());
    CoarseCall io(c);
    UknnLists L;
    XM_TRY(uknn_lists(c, io, source, S.P, (int64_t)users.size(), users.data(), n_nb, peer_flags, cap, min_common, &L));
    int32_t *d_q, *d_item, *d_n, *d_status;
    double *d_real = nullptr, *d_score, *d_bound, *d_mae;
    const size_t n = (size_t)n_test;
    XM_TRY(io.in(&d_q, tq.data(), n));
    XM_TRY(io.in(&d_item, test_item, n));
    if (test_rating) XM_TRY(io.in(&d_real, test_rating, n));
    XM_TRY(io.out(&d_score, out_score, n)); XM_TRY(io.out(&d_bound, out_bound, n));
    XM_TRY(io.out(&d_n, out_n, n)); XM_TRY(io.out(&d_status, status, n)); XM_TRY(io.scratch(&d_mae, 3, true));
    XM_TRY(xmap_uknn_predict_rows(c->st, n_test, d_q, d_item, (int64_t)users.size(), L.query_avg, n_nb, L.cnt, L.user, L.sim, c->R.n_users,
                                  c->R.n_items, c->pf_ptr, c->pf_item, c->pf_rating, L.user_avg, flags, d_score, d_bound, d_n, d_status));
    double h_mae[3] = {0.0, 0.0, 0.0};
    if (mae) {
        XM_TRY(xmap_mae(c->st, n_test, d_status, d_real, d_bound, d_bound, d_mae));
        io.back(h_mae, d_mae, 3);
    }
    XM_TRY(io.finish());
    if (mae) { mae[0] = h_mae[0]; mae[1] = h_mae[1]; }
    return XMAP_OK;
}

int xmap_ctx_uknn_recommend(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_nb, int32_t peer_flags,
                            int32_t cap, int32_t min_common, int32_t flags, int32_t n_top, int32_t min_support, int32_t *out_cnt,
                            int32_t *out_item, double *out_score, int32_t *out_support, const xmap_rec_filter *F, int64_t *stats) {
    // the host checks: before any device work, the outputs untouched, the context as it was
    XM_ARG(n_nb >= 1 && n_nb <= 1024);
    XM_ARG(n_top >= 1 && n_top <= 1024);
    XM_ARG(min_support >= 1);
    XM_ARG(cap >= 1);
    XM_ARG(min_common >= 1);
    XM_ARG((peer_flags & ~(XMAP_PEERS_KEEP_SELF | XMAP_PEERS_CENTRED)) == 0);
    XM_ARG((flags & ~(XMAP_UKNN_OWN_MEAN | XMAP_UKNN_KEEP_HELD)) == 0);
    XM_TRY(check_source("xmap_ctx_uknn_recommend", source, false));     // an item fold-in adds items, not users
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_user && out_cnt && out_item && out_score && out_support)));
    XM_ARG(n_query * (int64_t)n_nb < 2147483647ll);
    XM_TRY(check_filter(F, n_query));
    Source S;
    XM_TRY(resolve_source("xmap_ctx_uknn_recommend", c, source, false, &S));
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 6; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    CoarseCall io(c);
    UknnLists L;
    XM_TRY(uknn_lists(c, io, source, S.P, n_query, query_user, n_nb, peer_flags, cap, min_common, &L));
    int32_t *d_cnt, *d_item, *d_support;
    double *d_score;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_item, out_item, m));
    XM_TRY(io.out(&d_score, out_score, m)); XM_TRY(io.out(&d_support, out_support, m));
    xmap_rec_filter D;
    XM_TRY(upload_filter(io, F, n_query, c->R.n_items, &D));
    XM_TRY(xmap_uknn_topn_rows(c->st, n_query, L.query, L.Q.n_users, L.Q.ptr, L.Q.item, L.query_avg, n_nb, L.cnt, L.user, L.sim, c->R.n_users,
                               c->R.n_items, c->pf_ptr, c->pf_item, c->pf_rating, L.user_avg, flags, n_top, min_support, 0, d_cnt, d_item,
                               d_score, d_support, &D, stats));
    return io.finish();
}

// ---- related items: the top-N over the RecommenderSim rows of a basket's members -----------------------------------------------------

int xmap_ctx_related(xmap_ctx *c, int64_t n_query, const int64_t *b_ptr, const int32_t *b_item, const double *b_weight, int32_t how,
                     int32_t flags, int32_t n_top, int32_t min_support, int64_t max_records, int32_t *out_cnt, int32_t *out_item,
                     double *out_score, int32_t *out_support, const xmap_rec_filter *F, int64_t *stats) {
    // the host checks: before any device work, the outputs untouched, the context as it was
    XM_ARG(n_top >= 1 && n_top <= 1024);
    XM_ARG(how == XMAP_RELATED_SUM || how == XMAP_RELATED_MEAN || how == XMAP_RELATED_MAX);
    XM_ARG((flags & ~XMAP_RELATED_KEEP_MEMBERS) == 0);
    XM_ARG(min_support >= 1);
    XM_ARG(max_records >= 0);
    XM_ARG(n_query >= 0 && n_query <= (1ll << 28) && (n_query == 0 || (b_ptr && out_cnt && out_item && out_score && out_support)));
    if (n_query > 0) {
        if (b_ptr[0] != 0) { set_error("related: b_ptr[0] = %lld, not 0", (long long)b_ptr[0]); return XMAP_ERR_ARG; }
        for (int64_t q = 0; q < n_query; q++)
            if (b_ptr[q + 1] < b_ptr[q]) { set_error("related: b_ptr[%lld] < b_ptr[%lld]", (long long)q + 1, (long long)q); return XMAP_ERR_ARG; }
        if (b_ptr[n_query] > 0 && !b_item) { set_error("related: b_ptr lists %lld members, b_item is NULL", (long long)b_ptr[n_query]); return XMAP_ERR_ARG; }
    }
    XM_TRY(check_filter(F, n_query));
    XM_ARG(c && c->have_rec);
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 6; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    CoarseCall io(c);
    int64_t *d_ptr;
    int32_t *d_member, *d_cnt, *d_item, *d_support;
    double *d_weight = nullptr, *d_score;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top, nb = (size_t)b_ptr[n_query];
    XM_TRY(io.in(&d_ptr, b_ptr, n + 1));
    XM_TRY(io.in(&d_member, b_item, nb));
    if (b_weight) XM_TRY(io.in(&d_weight, b_weight, nb));
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_item, out_item, m));
    XM_TRY(io.out(&d_score, out_score, m)); XM_TRY(io.out(&d_support, out_support, m));
    xmap_rec_filter D;
    XM_TRY(upload_filter(io, F, n_query, c->R.n_items, &D));
    XM_TRY(xmap_related_rows(c->st, n_query, d_ptr, d_member, d_weight, c->R.n_items, c->rs_row_ptr, c->rs_col, c->rs_sim, how, flags, n_top,
                             min_support, max_records, d_cnt, d_item, d_score, d_support, &D, stats));
    return io.finish();
}

// ---- popularity fill: the ranking over the peer index of the raw ratings, and short lists completed with its head ------------------

// the context's ranking for (how, damping, min_count): built on first use, rebuilt when the three differ (one ranking per context)
static int pop_index_of(xmap_ctx *c, int32_t how, double damping, int32_t min_count) {
    if (c->have_pop && c->pop_how == how && c->pop_damping == damping && c->pop_min == min_count) return XMAP_OK;
    XM_TRY(peer_index_of(c, 0));
    const int32_t I = c->R.n_items;
    c->p_pop.release();
    c->have_pop = false;
    XM_ALLOC(c->p_pop, c->pp_item, I); XM_ALLOC(c->p_pop, c->pp_pos, I); XM_ALLOC(c->p_pop, c->pp_score, I);
    int64_t h[3] = {0, 0, 0};
    XM_TRY(xmap_pop_index(c->st, I, c->pr_hd_ptr[0], c->pr_hd_x[0], how, damping, min_count, c->pp_item, c->pp_score, c->pp_pos, h));
    c->pop_how = how; c->pop_damping = damping; c->pop_min = min_count; c->pop_ranked = h[0];
    c->have_pop = true;
    return XMAP_OK;
}

int xmap_ctx_popular(xmap_ctx *c, int32_t how, double damping, int32_t min_count, int64_t n_max, int32_t *out_item, double *out_score,
                     int64_t *n_ranked) {
    // the host checks: before any device work, the outputs untouched, the context as it was
    XM_ARG(how == XMAP_POP_COUNT || how == XMAP_POP_MEAN);
    XM_ARG(damping >= 0.0 && damping <= 1.7976931348623157e308);      // finite and >= 0 (a NaN fails both)
    XM_ARG(min_count >= 1);
    XM_ARG(n_max >= 0 && (n_max == 0 || (out_item && out_score)));
    XM_ARG(c && c->have_gen && c->have_rec);
    XM_HIP(hipSetDevice(c->device));
    XM_TRY(pop_index_of(c, how, damping, min_count));
    const int64_t I = c->R.n_items, n = n_max < I ? n_max : I;
    XM_TRY(d2h(out_item, (const int32_t *)c->pp_item, (size_t)n, c->st));
    XM_TRY(d2h(out_score, (const double *)c->pp_score, (size_t)n, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    for (int64_t k = n; k < n_max; k++) { out_item[k] = -1; out_score[k] = 0.0; }
    if (n_ranked) *n_ranked = c->pop_ranked;
    return XMAP_OK;
}

int xmap_ctx_recommend_filled(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by,
                              int32_t flags, const double *wtab, int32_t n_w, int32_t how, double damping, int32_t min_count,
                              int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_src,
                              const xmap_rec_filter *F, int64_t *stats) {
    // the host checks: before any device work, the outputs untouched, the context as it was
    XM_ARG(n_top >= 1 && n_top <= 64);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    XM_ARG(how == XMAP_POP_COUNT || how == XMAP_POP_MEAN);
    XM_ARG(damping >= 0.0 && damping <= 1.7976931348623157e308);      // finite and >= 0 (a NaN fails both)
    XM_ARG(min_count >= 1);
    XM_TRY(check_source("xmap_ctx_recommend_filled", source, true));
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay && out_src)));
    XM_TRY(check_filter(F, n_query));
    Source S;
    XM_TRY(resolve_source("xmap_ctx_recommend_filled", c, source, true, &S));
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 10; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    XM_TRY(pop_index_of(c, how, damping, min_count));
    CoarseCall io(c);
    TopnLists L;                // completed in place
    int32_t *d_src;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(io.out(&d_src, out_src, m));
    int64_t h6[6] = {0, 0, 0, 0, 0, 0}, h4[4] = {0, 0, 0, 0};
    XM_TRY(filtered_topn(io, S.P, S.T, n_query, query_user, n_top, rank_by, flags, wtab, n_w, F, h6, 6, &L));
    XM_TRY(xmap_topn_fill_rows(c->st, n_query, L.user, n_top, flags, S.P.n_users, S.T.n_items, S.P.ptr, S.P.item, S.T.avg, (int32_t)c->pop_ranked,
                               c->pp_item, c->pp_pos, c->R.n_items, L.cnt, L.item, L.plain, L.decay, d_src, &L.D, h4));
    io.back(out_cnt, L.cnt, n); io.back(out_item, L.item, m); io.back(out_plain, L.plain, m); io.back(out_decay, L.decay, m);
    XM_TRY(io.finish());
    if (stats) { for (int k = 0; k < 6; k++) stats[k] = h6[k]; for (int k = 0; k < 4; k++) stats[6 + k] = h4[k]; }
    return XMAP_OK;
}

// ---- shelves: the label table of the item space, and xmap_shelf_rows over the three sources ------------------------------------------

int xmap_ctx_set_labels(xmap_ctx *c, int32_t n_labels, const int64_t *lab_ptr, const int32_t *lab_id) {
    // the host checks: before the context is read
    if (n_labels < 0 || n_labels > XMAP_SHELF_MAX_LABELS) {
        set_error("xmap_ctx_set_labels: n_labels = %d, not in 0 .. 2^24", n_labels);
        return XMAP_ERR_ARG;
    }
    if (n_labels > 0 && !lab_ptr) { set_error("xmap_ctx_set_labels: lab_ptr is NULL"); return XMAP_ERR_ARG; }
    XM_ARG(c && (c->have_ratings || c->is_union));
    XM_HIP(hipSetDevice(c->device));
    if (n_labels == 0) { drop_labels(c); return XMAP_OK; }
    const size_t I1 = (size_t)c->R.n_items + 1;
    // the table's own check first needs lab_ptr[n_items] entries of lab_id: read on the host only where lab_ptr is sane so far
    int64_t n_ids = 0;
    bool sane = lab_ptr[0] == 0;
    for (size_t i = 1; i < I1 && sane; i++) sane = lab_ptr[i] >= lab_ptr[i - 1];
    if (sane) n_ids = lab_ptr[I1 - 1];
    if (n_ids > 0 && !lab_id) { set_error("xmap_ctx_set_labels: lab_ptr lists %lld labels, lab_id is NULL", (long long)n_ids); return XMAP_ERR_ARG; }
    ScratchPool fresh;          // (a table that fails leaves the earlier one in place)
    int64_t *d_ptr;
    int32_t *d_id;
    XM_TRY(h2d(fresh, &d_ptr, lab_ptr, I1, c->st));
    XM_TRY(h2d(fresh, &d_id, lab_id, (size_t)n_ids, c->st));
    int64_t n_lab = 0;
    XM_TRY(shelf_check_labels(c->st, "xmap_ctx_set_labels", c->R.n_items, n_labels, d_ptr, d_id, &n_lab));
    drop_labels(c);
    c->p_lab.ptrs.swap(fresh.ptrs);
    c->have_lab = true;
    c->n_labels = n_labels; c->n_lab = n_lab;
    c->lb_ptr = d_ptr; c->lb_id = d_id;
    c->h_lab_ptr.assign(lab_ptr, lab_ptr + I1);
    return XMAP_OK;
}

// The labels of a call over the tables T: the context's table, and the call's lab_allow on the device.  The batch items of an
// item fold-in carry no label: for its tables lab_ptr is extended by its last value.
static int call_labels(xmap_ctx *c, CoarseCall &io, const Tables &T, const uint32_t *lab_allow, ShelfLabels *L) {
    const int64_t *d_lab_ptr = c->lb_ptr;
    if (T.n_items > c->R.n_items) {
        std::vector<int64_t> ext(c->h_lab_ptr);
        ext.resize((size_t)T.n_items + 1, c->h_lab_ptr.back());
        int64_t *d_ext;
        XM_TRY(io.in(&d_ext, (const int64_t *)ext.data(), ext.size()));
        XM_HIP(hipStreamSynchronize(c->st));    // (ext leaves with this block)
        d_lab_ptr = d_ext;
    }
    uint32_t *d_allow = nullptr;
    if (lab_allow) XM_TRY(io.in(&d_allow, lab_allow, (size_t)((c->n_labels + 31) / 32)));
    *L = ShelfLabels{c->n_labels, d_lab_ptr, c->lb_id, d_allow};
    return XMAP_OK;
}

int xmap_ctx_recommend_shelves(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_shelf, int32_t n_top,
                               int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t shelf_by, int32_t min_fill,
                               const uint32_t *lab_allow, int32_t *out_nshelf, int32_t *out_label, double *out_sscore, int32_t *out_size,
                               int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, const xmap_rec_filter *F,
                               int64_t *stats) {
    // the host checks: before the context is read, the outputs untouched, the context as it was
    const char *who = "xmap_ctx_recommend_shelves";
    XM_TRY(shelf_check_args(who, n_query, n_shelf, n_top, rank_by, flags, shelf_by, min_fill, 1, 0));
    XM_TRY(check_source(who, source, true));
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query == 0 || (query_user && out_nshelf && out_label && out_sscore && out_size && out_cnt && out_item && out_plain && out_decay));
    XM_TRY(check_filter(F, n_query));
    Source S;
    XM_TRY(resolve_source(who, c, source, true, &S));
    if (!c->have_lab) { set_error("%s: the context has no labels (xmap_ctx_set_labels)", who); return XMAP_ERR_ARG; }
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 10; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    CoarseCall io(c);
    ShelfLabels B;
    XM_TRY(call_labels(c, io, S.T, lab_allow, &B));
    int32_t *d_user, *d_nshelf, *d_label, *d_size, *d_cnt, *d_item;
    double *d_w, *d_sscore, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, ns = n * (size_t)n_shelf, m = ns * (size_t)n_top;
    XM_TRY(io.in(&d_user, query_user, n));
    XM_TRY(io.in(&d_w, wtab, (size_t)n_w));
    XM_TRY(io.out(&d_nshelf, out_nshelf, n)); XM_TRY(io.out(&d_label, out_label, ns)); XM_TRY(io.out(&d_sscore, out_sscore, ns));
    XM_TRY(io.out(&d_size, out_size, ns)); XM_TRY(io.out(&d_cnt, out_cnt, ns)); XM_TRY(io.out(&d_item, out_item, m));
    XM_TRY(io.out(&d_plain, out_plain, m)); XM_TRY(io.out(&d_decay, out_decay, m));
    xmap_rec_filter D;
    XM_TRY(upload_filter(io, F, n_query, S.T.n_items, &D));
    XM_TRY(shelf_rows(c->st, n_query, d_user, n_top, rank_by, flags, rec_model(S.P, S.T, d_w, n_w), B, n_shelf, shelf_by, min_fill, 0,
                      ShelfOut{d_nshelf, d_label, d_sscore, d_size, d_cnt, d_item, d_plain, d_decay}, &D, stats));
    return io.finish();
}

// ---- quotas and calibrated lists: xmap_quota_rows over the three sources and the context's labels ------------------------------------

int xmap_ctx_recommend_quota(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t n_top,
                             int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t mode, int32_t cap,
                             const int32_t *lab_cap, const uint32_t *lab_weight, const uint32_t *lab_allow, int32_t *out_cnt,
                             int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos, int32_t *out_label,
                             const xmap_rec_filter *F, int64_t *stats) {
    // the host checks: before the context is read, the outputs untouched, the context as it was
    const char *who = "xmap_ctx_recommend_quota";
    XM_TRY(quota_check_args(who, n_query, n_pool, n_top, rank_by, flags, mode, cap, lab_cap != nullptr, 1));
    XM_TRY(check_source(who, source, true));
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay && out_pos && out_label));
    XM_TRY(check_filter(F, n_query));
    Source S;
    XM_TRY(resolve_source(who, c, source, true, &S));
    if (!c->have_lab) { set_error("%s: the context has no labels (xmap_ctx_set_labels)", who); return XMAP_ERR_ARG; }
    XM_HIP(hipSetDevice(c->device));
    if (n_query == 0) {
        if (stats) for (int k = 0; k < 10; k++) stats[k] = 0;
        return XMAP_OK;
    }
    CoarseCall io(c);
    ShelfLabels B;
    XM_TRY(call_labels(c, io, S.T, lab_allow, &B));
    uint32_t *d_weight = nullptr;
    int32_t *d_cap = nullptr;
    if (lab_cap) XM_TRY(io.in(&d_cap, lab_cap, (size_t)c->n_labels));
    if (lab_weight) XM_TRY(io.in(&d_weight, lab_weight, (size_t)c->n_labels));
    int32_t *d_user, *d_cnt, *d_item, *d_pos, *d_label;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(io.in(&d_user, query_user, n));
    XM_TRY(io.in(&d_w, wtab, (size_t)n_w));
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_item, out_item, m)); XM_TRY(io.out(&d_plain, out_plain, m));
    XM_TRY(io.out(&d_decay, out_decay, m)); XM_TRY(io.out(&d_pos, out_pos, m)); XM_TRY(io.out(&d_label, out_label, m));
    xmap_rec_filter D;
    XM_TRY(upload_filter(io, F, n_query, S.T.n_items, &D));
    int64_t h10[10];
    XM_TRY(quota_rows(c->st, n_query, d_user, n_pool, n_top, rank_by, flags, rec_model(S.P, S.T, d_w, n_w), QuotaRule{mode, cap, d_cap, d_weight},
                      B, QuotaOut{d_cnt, d_item, d_plain, d_decay, d_pos, d_label}, &D, h10));
    XM_TRY(io.finish());
    if (stats) for (int k = 0; k < 10; k++) stats[k] = h10[k];
    return XMAP_OK;
}

// ---- allotment: xmap_allot_rows over the three sources --------------------------------------------------------------------------------

int xmap_ctx_recommend_allot(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t n_top,
                             int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t cap, const int32_t *item_cap,
                             int32_t n_cap, int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos,
                             int32_t *item_taken, const xmap_rec_filter *F, int64_t *stats) {
    // the host checks: before the context is read, the outputs untouched, the context as it was
    const char *who = "xmap_ctx_recommend_allot";
    XM_TRY(allot_check_args(who, n_query, n_pool, 64, n_top, rank_by, flags, cap, item_cap != nullptr));
    if (item_cap) {
        if (n_cap < 0) { set_error("%s: n_cap = %d, not >= 0", who, n_cap); return XMAP_ERR_ARG; }
        for (int32_t i = 0; i < n_cap; i++)
            if (item_cap[i] < 0) {
                set_error("%s: item_cap is negative: the first at item_cap[%d] (0 bars an item, INT32_MAX is no cap)", who, i);
                return XMAP_ERR_ARG;
            }
    }
    XM_TRY(check_source(who, source, true));
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay && out_pos));
    XM_TRY(check_filter(F, n_query));
    Source S;
    XM_TRY(resolve_source(who, c, source, true, &S));
    XM_HIP(hipSetDevice(c->device));
    if (item_cap && n_cap != S.T.n_items) {
        set_error("%s: n_cap = %d, the tables of the source hold %d items", who, n_cap, S.T.n_items);
        return XMAP_ERR_ARG;
    }
    CoarseCall io(c);
    int32_t *d_cap = nullptr, *d_taken = nullptr, *d_user, *d_cnt, *d_item, *d_pos;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top, I = (size_t)S.T.n_items;
    if (item_cap) XM_TRY(io.in(&d_cap, item_cap, I));
    if (item_taken) XM_TRY(io.out(&d_taken, item_taken, I));
    XM_TRY(io.in(&d_user, query_user, n));
    XM_TRY(io.in(&d_w, wtab, (size_t)n_w));
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_item, out_item, m)); XM_TRY(io.out(&d_plain, out_plain, m));
    XM_TRY(io.out(&d_decay, out_decay, m)); XM_TRY(io.out(&d_pos, out_pos, m));
    xmap_rec_filter D;
    XM_TRY(upload_filter(io, F, n_query, S.T.n_items, &D));
    int64_t h12[12];
    XM_TRY(allot_rows(c->st, n_query, d_user, n_pool, n_top, rank_by, flags, rec_model(S.P, S.T, d_w, n_w), cap, d_cap,
                      AllotOut{d_cnt, d_item, d_plain, d_decay, d_pos, d_taken}, &D, h12));
    XM_TRY(io.finish());
    if (stats) for (int k = 0; k < 12; k++) stats[k] = h12[k];
    return XMAP_OK;
}

// ---- fused lists: xmap_fuse_rows over uploaded lists, and the item-based and user-based lists of the same users fused -------------

int xmap_ctx_fuse(xmap_ctx *c, int64_t n_query, int32_t n_lists, const xmap_fuse_list *lists, int32_t n_ids, int32_t how, double rrf_c,
                  int32_t min_lists, int32_t n_top, int32_t *out_cnt, int32_t *out_id, double *out_score, int32_t *out_lists,
                  int64_t *stats) {
    // the host checks: before the context is read, the outputs untouched
    XM_TRY(fuse_check("xmap_ctx_fuse", n_query, n_lists, lists, n_ids, how, rrf_c, min_lists, n_top, 0, out_cnt, out_id, out_score, out_lists));
    XM_ARG(c);
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 5; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    CoarseCall io(c);
    xmap_fuse_list D[XMAP_FUSE_MAX_LISTS];
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    for (int l = 0; l < n_lists; l++) {
        const size_t ml = n * (size_t)lists[l].width;
        int32_t *d_c, *d_i;
        double *d_s = nullptr;
        XM_TRY(io.in(&d_c, lists[l].cnt, n));
        XM_TRY(io.in(&d_i, lists[l].item, ml));
        if (lists[l].score) XM_TRY(io.in(&d_s, lists[l].score, ml));
        D[l].cnt = d_c; D[l].item = d_i; D[l].score = d_s; D[l].width = lists[l].width; D[l].weight = lists[l].weight;
    }
    int32_t *d_cnt, *d_id, *d_lists;
    double *d_score;
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_id, out_id, m));
    XM_TRY(io.out(&d_score, out_score, m)); XM_TRY(io.out(&d_lists, out_lists, m));
    XM_TRY(xmap_fuse_rows(c->st, n_query, n_lists, D, n_ids, how, rrf_c, min_lists, n_top, 0, d_cnt, d_id, d_score, d_lists, stats));
    return io.finish();
}

int xmap_ctx_recommend_hybrid(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t n_pool_items,
                              int32_t rank_by, int32_t topn_flags, const double *wtab, int32_t n_w, int32_t n_pool_users, int32_t n_nb,
                              int32_t peer_flags, int32_t cap, int32_t min_common, int32_t uknn_flags, int32_t min_support, double w_items,
                              double w_users, int32_t how, double rrf_c, int32_t min_lists, const xmap_rec_filter *F, int32_t *out_cnt,
                              int32_t *out_item, double *out_score, int32_t *out_lists, int64_t *stats) {
    // the host checks: before the context is read or any device work is done, the outputs untouched
    XM_ARG(n_top >= 1 && n_top <= 1024);
    XM_ARG(n_pool_items >= 1 && n_pool_items <= 64);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((topn_flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_pool_users >= 1 && n_pool_users <= 1024);
    XM_ARG(n_nb >= 1 && n_nb <= 1024);
    XM_ARG((peer_flags & ~(XMAP_PEERS_KEEP_SELF | XMAP_PEERS_CENTRED)) == 0);
    XM_ARG(cap >= 1);
    XM_ARG(min_common >= 1);
    XM_ARG((uknn_flags & ~(XMAP_UKNN_OWN_MEAN | XMAP_UKNN_KEEP_HELD)) == 0);
    XM_ARG(min_support >= 1);
    XM_ARG(w_items >= -1.7976931348623157e308 && w_items <= 1.7976931348623157e308);       // finite (a NaN fails both)
    XM_ARG(w_users >= -1.7976931348623157e308 && w_users <= 1.7976931348623157e308);
    XM_ARG(how == XMAP_FUSE_RRF || how == XMAP_FUSE_SUM || how == XMAP_FUSE_MEAN);
    XM_ARG(rrf_c >= 0.0 && rrf_c <= 1.7976931348623157e308);        // finite and >= 0
    XM_ARG(min_lists >= 1 && min_lists <= 2);
    XM_TRY(check_source("xmap_ctx_recommend_hybrid", source, false));       // an item fold-in adds items, not users
    XM_ARG(n_query >= 0 && n_query <= (1ll << 28) && (n_query == 0 || (query_user && out_cnt && out_item && out_score && out_lists)));
    XM_ARG(n_query * (int64_t)n_nb < 2147483647ll);
    XM_TRY(check_filter(F, n_query));
    Source S;
    XM_TRY(resolve_source("xmap_ctx_recommend_hybrid", c, source, true, &S));
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 17; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    CoarseCall io(c);
    const size_t n = (size_t)n_query, mu = n * (size_t)n_pool_users, m = n * (size_t)n_top;
    int64_t h6[6] = {0, 0, 0, 0, 0, 0}, u6[6] = {0, 0, 0, 0, 0, 0}, f5[5] = {0, 0, 0, 0, 0};
    // ---- list 0: the filtered item-kNN top-N, as xmap_ctx_recommend_filtered runs it
    TopnLists A;
    XM_TRY(filtered_topn(io, S.P, S.T, n_query, query_user, n_pool_items, rank_by, topn_flags, wtab, n_w, F, h6, 6, &A));
    // ---- list 1: the user-kNN top-N, as xmap_ctx_uknn_recommend runs it
    UknnLists L;
    XM_TRY(uknn_lists(c, io, source, S.P, n_query, query_user, n_nb, peer_flags, cap, min_common, &L));
    int32_t *u_cnt, *u_item, *u_support;
    double *u_score;
    XM_TRY(io.scratch(&u_cnt, n)); XM_TRY(io.scratch(&u_item, mu));
    XM_TRY(io.scratch(&u_score, mu)); XM_TRY(io.scratch(&u_support, mu));
    XM_TRY(xmap_uknn_topn_rows(c->st, n_query, L.query, L.Q.n_users, L.Q.ptr, L.Q.item, L.query_avg, n_nb, L.cnt, L.user, L.sim, c->R.n_users,
                               c->R.n_items, c->pf_ptr, c->pf_item, c->pf_rating, L.user_avg, uknn_flags, n_pool_users, min_support, 0, u_cnt,
                               u_item, u_score, u_support, &A.D, u6));
    // ---- the fuse
    const xmap_fuse_list lists[2] = {{A.cnt, A.item, rank_by ? A.decay : A.plain, n_pool_items, w_items},
                                     {u_cnt, u_item, u_score, n_pool_users, w_users}};
    int32_t *d_cnt, *d_id, *d_lists;
    double *d_score;
    XM_TRY(io.out(&d_cnt, out_cnt, n)); XM_TRY(io.out(&d_id, out_item, m));
    XM_TRY(io.out(&d_score, out_score, m)); XM_TRY(io.out(&d_lists, out_lists, m));
    XM_TRY(xmap_fuse_rows(c->st, n_query, 2, lists, c->R.n_items, how, rrf_c, min_lists, n_top, 0, d_cnt, d_id, d_score, d_lists, f5));
    XM_TRY(io.finish());
    if (stats) {
        for (int k = 0; k < 6; k++) { stats[k] = h6[k]; stats[6 + k] = u6[k]; }
        for (int k = 0; k < 5; k++) stats[12 + k] = f5[k];
    }
    return XMAP_OK;
}
}
