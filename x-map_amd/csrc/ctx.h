// ctx.h -- the context of the coarse ABI (xmap_ctx_*), private to the files that implement it (api.hip, api_tail.hip,
// api_lists.hip): the pools and the resident state of a context, the transfers of one coarse call (CoarseCall), the
// sources a tail call reads its profiles and tables from, and the filtered top-N the list calls start from.  Host code only.
#ifndef XMAP_CTX_H
#define XMAP_CTX_H
#include <vector>

#include "common.h"
#include "rec_model.h"

namespace xmap {

struct Pool {
    std::vector<void *> ptrs;
    void release() {
        for (void *p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};
struct ScratchPool : Pool { ~ScratchPool() { release(); } };       // a stage's temporaries: released when the call returns

}  // namespace xmap

using namespace xmap;

struct xmap_ctx {
    int device = 0;
    hipStream_t st = nullptr;
    Pool p_ratings, p_sim, p_ext, p_gen, p_rows;
    // ratings
    xmap_ratings R;
    bool have_ratings = false;
    bool plain_exact = true;        // cosine may use the plain fp64 sums (plain_sums_exact)
    // stage A
    bool have_sim = false;
    xmap_sim S;
    double *u_avg = nullptr, *u_norm = nullptr, *info = nullptr;
    int64_t n_kept = 0, n_eval = 0, n_contrib = 0;
    int64_t half_contrib = 0;       // sum over the users of d (d - 1) / 2: sizes the pair buffers (known from user_ptr)
    // stage B
    bool have_ext = false;
    int top_k = 0;
    xmap_ext_tables T;
    xmap_path_units Un;
    int32_t *n_cand = nullptr, *top_end = nullptr;
    double *top_val = nullptr;
    int64_t n_out = 0, n_paths = 0;
    // accumulator rows (kernels return them zeroed: kept across passes)
    double *acc = nullptr, *hacc = nullptr;
    int32_t *touched = nullptr, *htouched = nullptr;
    int64_t acc_slots = 0, acc_len = 0, hacc_rows = 0, hacc_len = 0;
    int32_t n_slots = 0;
    int32_t fast_div = 0;
    // stage C
    bool have_gen = false;
    int32_t *g_user = nullptr, *g_item = nullptr;
    double *g_rating = nullptr;
    int64_t *g_time = nullptr;
    int64_t n_rows = 0, n_target_rows = 0;
    int64_t *g_off_t = nullptr, *g_off_m = nullptr;     // per-user offsets of the two row segments (exclusive scans, [U+1])
                                                        // (g_off_t also tells an explanation which rows of a profile are pass-through rows)
    int32_t *g_map = nullptr;                           // the replacement map (source item -> target item, -1: none) in p_gen
    // the recommender tail: profiles of the AlterEgo rows, RecommenderSim over them, neighbour lists
    Pool p_rec, p_nb;
    bool have_rec = false, have_nb = false;
    int64_t *pf_ptr = nullptr, *pf_time = nullptr;
    int32_t *pf_item = nullptr;
    double *pf_rating = nullptr;
    int64_t *rs_row_ptr = nullptr;
    int32_t *rs_col = nullptr, *rs_nij = nullptr;
    double *rs_sim = nullptr, *rs_ls = nullptr, *rs_avg = nullptr, *rs_norm = nullptr;
    int64_t rec_pairs = 0;
    int keep = 0;
    int rec_cap = 0;                // the num_atleast of the resident RecommenderSim (an item fold-in weights with the same)
    int32_t *nb_cnt = nullptr, *nb_col = nullptr;
    double *nb_sim = nullptr, *nb_ls = nullptr;
    // the diversity index of the RecommenderSim CSR (xmap_div_index; rs_row_ptr is shared): built by the first
    // xmap_ctx_recommend_diverse, dropped with the matrix, kept when the neighbour lists change
    Pool p_div;
    bool have_div = false;
    int32_t *dv_col = nullptr;
    double *dv_abs = nullptr;
    // the peer index of the resident profiles (xmap_peer_index), one per centring ([0] raw ratings, [1] centred by rs_avg): built
    // by the first xmap_ctx_peers that needs it, dropped with the profiles and the averages (drop_tail)
    Pool p_peer[2];
    bool have_peer[2] = {false, false};
    int64_t *pr_hd_ptr[2] = {nullptr, nullptr};
    int32_t *pr_hd_user[2] = {nullptr, nullptr};
    double *pr_hd_x[2] = {nullptr, nullptr}, *pr_nrm[2] = {nullptr, nullptr};
    // the popularity ranking over the peer index [0] (xmap_pop_index), with what it was built for: built by the first
    // xmap_ctx_popular / xmap_ctx_recommend_filled, rebuilt when (how, damping, min_count) differ, dropped with the tail
    Pool p_pop;
    bool have_pop = false;
    int32_t pop_how = 0, pop_min = 0;
    double pop_damping = 0.0;
    int64_t pop_ranked = 0;
    int32_t *pp_item = nullptr, *pp_pos = nullptr;
    double *pp_score = nullptr;
    // item fold-in: the RecommenderSim rows of the last batch of new items (if_*), the batch's rater CSR, and the EXTENDED tables
    // of I + if_new items (x_*: rows [0, I) copies of nb_* / rs_avg, row I + q the list and the average of batch item q); hangs
    // on the tail and the neighbour lists: dropped with them
    Pool p_ifold;
    bool have_ifold = false;
    int64_t if_new = 0, if_pairs = 0;
    int64_t *if_row_ptr = nullptr, *if_ptr = nullptr;
    int32_t *if_col = nullptr, *if_nij = nullptr, *if_user = nullptr;
    double *if_sim = nullptr, *if_ls = nullptr, *if_norm = nullptr;
    int32_t *x_cnt = nullptr, *x_col = nullptr;
    double *x_sim = nullptr, *x_ls = nullptr, *x_avg = nullptr;
    // fold-in: the AlterEgo profiles of the last batch (user-major, as pf_*), built with g_map: dropped with the map
    Pool p_fold;
    bool have_fold = false;
    int64_t f_users = 0, f_rows = 0;
    int64_t *f_ptr = nullptr, *f_time = nullptr;
    int32_t *f_item = nullptr;
    double *f_rating = nullptr;
    // the batch's raw CSR and pass-through counts, for the sources of an explanation (xmap_ctx_foldin_explain)
    int64_t *f_raw_ptr = nullptr;
    int32_t *f_raw_item = nullptr, *f_cnt_t = nullptr;
    // the label table of the item space (xmap_ctx_set_labels): lab_ptr [n_items + 1] and lab_id on the device, lab_ptr also on the
    // host (an item fold-in extends it); survives the tail, dropped with the item space (an upload, a union) and the context
    Pool p_lab;
    bool have_lab = false;
    int32_t n_labels = 0;
    int64_t n_lab = 0;
    int64_t *lb_ptr = nullptr;
    int32_t *lb_id = nullptr;
    std::vector<int64_t> h_lab_ptr;
    // multi-domain: this context holds the union of other contexts' AlterEgo rows as user-major profiles (xmap_ctx_union) and
    // nothing of the stages; have_gen is set, n_rows = the union's rows, R carries the union's sizes and all-target flags
    Pool p_union;
    bool is_union = false;
    int64_t *un_ptr = nullptr, *un_time = nullptr;
    int32_t *un_item = nullptr;
    double *un_rating = nullptr;
};

namespace xmap {

template <typename T>
static inline int dalloc(Pool &pool, T **out, size_t n, hipStream_t st, bool zero = false) {
    void *p = nullptr;
    const size_t bytes = sizeof(T) * (n ? n : 1);
    XM_HIP(hipMalloc(&p, bytes));
    pool.ptrs.push_back(p);
    if (zero) XM_HIP(hipMemsetAsync(p, 0, bytes, st));
    *out = (T *)p;
    return XMAP_OK;
}
#define XM_TRY(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)
#define XM_ALLOC(pool, ptr, n) XM_TRY(dalloc(pool, &(ptr), (size_t)(n), c->st))
#define XM_ALLOCZ(pool, ptr, n) XM_TRY(dalloc(pool, &(ptr), (size_t)(n), c->st, true))

template <typename T>
static inline int h2d(Pool &pool, T **out, const T *host, size_t n, hipStream_t st) {
    XM_TRY(dalloc(pool, out, n, st));
    if (n) XM_HIP(hipMemcpyAsync(*out, host, sizeof(T) * n, hipMemcpyHostToDevice, st));
    return XMAP_OK;
}
template <typename T>
static inline int d2h(T *host, const T *dev, size_t n, hipStream_t st) {
    if (n) XM_HIP(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, st));
    return XMAP_OK;
}

// The transfers of one coarse call: host arrays in, device temporaries, host arrays out.  The temporaries are released when
// the call returns, whichever way; the copies to the caller's buffers are only recorded and go out in finish(), in the order
// they were recorded and in front of the call's one wait, so a call that fails on the way has written to none of them.
// An optional array stays the caller's `if`: a pointer left NULL is how the bodies are told "absent".
struct CoarseCall {
    hipStream_t st;
    ScratchPool tmp;
    struct Back { void *host; const void *dev; size_t bytes; };
    std::vector<Back> backs;
    explicit CoarseCall(const xmap_ctx *c) : st(c->st) {}
    template <typename T>
    int in(T **d, const T *host, size_t n) { return h2d(tmp, d, host, n, st); }
    template <typename T>
    int scratch(T **d, size_t n, bool zero = false) { return dalloc(tmp, d, n, st, zero); }
    // a device buffer of the call (an output, or a temporary that is also read back) -> host[n] at finish()
    template <typename T>
    void back(T *host, const T *dev, size_t n) { backs.push_back(Back{host, dev, sizeof(T) * n}); }
    template <typename T>
    int out(T **d, T *host, size_t n, bool zero = false) {
        XM_TRY(scratch(d, n, zero));
        back(host, *d, n);
        return XMAP_OK;
    }
    int finish() {
        for (const Back &b : backs)
            if (b.bytes) XM_HIP(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
        return XMAP_OK;
    }
};

// any earlier stage run again invalidates the recommender tail (as the stages invalidate each other)
static inline void drop_ifold(xmap_ctx *c) {
    c->p_ifold.release();
    c->have_ifold = false;
    c->if_new = c->if_pairs = 0;
}

static inline void drop_tail(xmap_ctx *c) {
    drop_ifold(c);
    c->p_nb.release(); c->p_rec.release(); c->p_div.release();
    c->have_rec = c->have_nb = c->have_div = false;
    for (int k = 0; k < 2; k++) { c->p_peer[k].release(); c->have_peer[k] = false; }
    c->p_pop.release(); c->have_pop = false;
}

// the fold-in batch hangs on the replacement map: upload, item_sim, extend and generate drop it; the tail calls leave it
// the union of other contexts' rows goes with whatever replaces it: an upload, or the next union
static inline void drop_union(xmap_ctx *c) {
    c->p_union.release();
    if (c->is_union) c->have_gen = false;
    c->is_union = false;
}

static inline void drop_labels(xmap_ctx *c) {
    c->p_lab.release();
    c->have_lab = false;
    c->n_labels = 0; c->n_lab = 0;
    c->h_lab_ptr.clear();
}

static inline void drop_fold(xmap_ctx *c) {
    c->p_fold.release();
    c->have_fold = false;
    c->f_users = c->f_rows = 0;
}

// user-major profiles the prediction and ranking kernels read: the resident AlterEgo rows, or a fold-in batch
struct Profiles {
    int64_t n_users;
    const int64_t *ptr, *time;
    const int32_t *item;
    const double *rating;
};
static inline Profiles resident_profiles(const xmap_ctx *c) { return Profiles{c->R.n_users, c->pf_ptr, c->pf_time, c->pf_item, c->pf_rating}; }
static inline Profiles foldin_profiles(const xmap_ctx *c) { return Profiles{c->f_users, c->f_ptr, c->f_time, c->f_item, c->f_rating}; }

// the tables the same kernels read: neighbour lists [n_items][keep], item averages [n_items]; the resident ones, or the extended
// ones of an item fold-in (items >= n_resident are the batch's; their holders are the batch's raters, new_ptr / new_user)
struct Tables {
    int32_t n_items, keep;
    const int32_t *cnt, *col;
    const double *sim, *avg;
    int32_t n_resident;
    const int64_t *new_ptr;
    const int32_t *new_user;
};
static inline Tables resident_tables(const xmap_ctx *c) {
    return Tables{c->R.n_items, c->keep, c->nb_cnt, c->nb_col, c->nb_sim, c->rs_avg, c->R.n_items, nullptr, nullptr};
}
static inline Tables itemfold_tables(const xmap_ctx *c) {
    return Tables{(int32_t)(c->R.n_items + c->if_new), c->keep, c->x_cnt, c->x_col, c->x_sim, c->x_avg, c->R.n_items, c->if_ptr, c->if_user};
}
// the model of one coarse call (rec_model.h): profiles, tables and the call's decay table on the device
static inline RecModel rec_model(const Profiles &P, const Tables &T, const double *d_w, int32_t n_w) {
    return RecModel{P.n_users, T.n_items, T.keep, T.cnt, T.col, T.sim, P.ptr, P.item, P.rating, P.time, T.avg, d_w, n_w};
}

// The source of a tail call (XMAP_SRC_*) in two steps.  check_source is an argument check: it does not read the context and
// names the call in its message; item_foldin = false where the batch of an item fold-in is no source of the call.
static inline int check_source(const char *who, int32_t source, bool item_foldin) {
    if (source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN || (item_foldin && source == XMAP_SRC_ITEM_FOLDIN)) return XMAP_OK;
    set_error("%s: bad argument: source = %d, not XMAP_SRC_RESIDENT%s", who, source, item_foldin ? ", _FOLDIN or _ITEM_FOLDIN" : " or _FOLDIN");
    return XMAP_ERR_ARG;
}
// resolve_source runs after the argument checks: what the context must hold for a checked source (need_nb = false: a call that
// reads no neighbour lists), then the profiles and the tables of that source.  A refusal names the entry and the condition.
struct Source { Profiles P; Tables T; };
#define XM_CTX(cond) do { if (!(cond)) { set_error("%s: bad argument: %s", who, #cond); return XMAP_ERR_ARG; } } while (0)
static inline int resolve_source(const char *who, const xmap_ctx *c, int32_t source, bool need_nb, Source *S) {
    if (need_nb) XM_CTX(c && c->have_gen && c->have_rec && c->have_nb);
    else XM_CTX(c && c->have_gen && c->have_rec);
    XM_CTX(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_CTX(source != XMAP_SRC_ITEM_FOLDIN || c->have_ifold);
    S->P = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    S->T = source == XMAP_SRC_ITEM_FOLDIN ? itemfold_tables(c) : resident_tables(c);
    return XMAP_OK;
}
#undef XM_CTX

// The eligibility rules of a coarse call (xmap_rec_filter with HOST pointers), checked on the host before any device work, as
// xmap_ctx_foldin checks its batch
static inline int check_filter(const xmap_rec_filter *F, int64_t n_query) {
    if (!F) return XMAP_OK;
    if (F->min_score != F->min_score) { set_error("filter: min_score is NaN"); return XMAP_ERR_ARG; }
    if (!F->ex_ptr || n_query <= 0) return XMAP_OK;
    if (F->ex_ptr[0] != 0) { set_error("filter: ex_ptr[0] = %lld, not 0", (long long)F->ex_ptr[0]); return XMAP_ERR_ARG; }
    for (int64_t q = 0; q < n_query; q++)
        if (F->ex_ptr[q + 1] < F->ex_ptr[q]) { set_error("filter: ex_ptr[%lld] < ex_ptr[%lld]", (long long)q + 1, (long long)q); return XMAP_ERR_ARG; }
    if (F->ex_ptr[n_query] > 0 && !F->ex_id) { set_error("filter: ex_ptr lists %lld ids, ex_id is NULL", (long long)F->ex_ptr[n_query]); return XMAP_ERR_ARG; }
    return XMAP_OK;
}

// the device copy of a checked host filter over an id space of n ids (n_query > 0)
static inline int upload_filter(CoarseCall &io, const xmap_rec_filter *F, int64_t n_query, int64_t n, xmap_rec_filter *D) {
    D->allow = nullptr; D->ex_ptr = nullptr; D->ex_id = nullptr;
    D->min_score = F ? F->min_score : -__builtin_inf();
    if (!F) return XMAP_OK;
    if (F->allow) {
        uint32_t *d_allow;
        XM_TRY(io.in(&d_allow, F->allow, (size_t)((n + 31) / 32)));
        D->allow = d_allow;
    }
    if (F->ex_ptr) {
        int64_t *d_ptr;
        int32_t *d_id;
        XM_TRY(io.in(&d_ptr, F->ex_ptr, (size_t)n_query + 1));
        XM_TRY(io.in(&d_id, F->ex_id, (size_t)F->ex_ptr[n_query]));
        D->ex_ptr = d_ptr; D->ex_id = d_id;
    }
    return XMAP_OK;
}

// The top-N of n_query users into device temporaries of the call, as xmap_ctx_recommend_filtered ranks them (n_stats = 6:
// the filter F, or none, uploaded as L->D) or xmap_ctx_recommend does (F == NULL, n_stats = 4: L->D is not set): the queries
// and the decay table go up, the four columns stay on the device for whatever re-ranks, completes or returns them.
struct TopnLists {
    int32_t *user, *cnt, *item;         // the queries [Q]; counts [Q], items [Q][n_top]
    double *w, *plain, *decay;          // the decay table [n_w]; scores [Q][n_top]
    xmap_rec_filter D;                  // device pointers: the later passes of the call filter by the same rules
};
static inline int filtered_topn(CoarseCall &io, const Profiles &P, const Tables &T, int64_t n_query, const int32_t *query_user,
                                int32_t n_top, int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, const xmap_rec_filter *F,
                                int64_t *h_stats, int n_stats, TopnLists *L) {
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(io.in(&L->user, query_user, n));
    XM_TRY(io.in(&L->w, wtab, (size_t)n_w));
    XM_TRY(io.scratch(&L->cnt, n)); XM_TRY(io.scratch(&L->item, m));
    XM_TRY(io.scratch(&L->plain, m)); XM_TRY(io.scratch(&L->decay, m));
    if (n_stats == 6) XM_TRY(upload_filter(io, F, n_query, T.n_items, &L->D));
    return topn_rows(io.st, n_query, L->user, n_top, rank_by, flags, rec_model(P, T, L->w, n_w), L->cnt, L->item, L->plain, L->decay,
                     n_stats == 6 ? &L->D : nullptr, h_stats, n_stats);
}

}  // namespace xmap
#endif
