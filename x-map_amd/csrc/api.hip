// api.hip -- the coarse, handle-based C ABI of the hot path: a host in any language drives the three
// pipelines with plain host buffers and never sees a device pointer, a scan or a work-unit plan.
//
//   xmap_ctx_create -> xmap_ctx_upload_ratings -> xmap_ctx_item_sim     (baseliner_calculate_sim_pipeline, assist.py:66-77)
//                                              -> xmap_ctx_extend       (extender_pipeline, assist.py:80-102; lazy lists)
//                                              -> xmap_ctx_generate     (generator_pipeline, assist.py:136-150)
//   the recommender tail over the AlterEgo rows, device-resident:   -> xmap_ctx_rec_sim (assist.py:153-177)
//                     -> xmap_ctx_rec_select | xmap_ctx_rec_set_neighbors (assist.py:179-192) -> xmap_ctx_predict (assist.py:195-207)
//                                                                                  | xmap_ctx_recommend (top-N per query user)
//                                                                                  | xmap_ctx_audience (top-N users per query item)
//                                                                                  | xmap_ctx_evaluate_topn (top-N against held-out pairs)
//   fold-in, for profiles that were not rows of the upload:  xmap_ctx_generate -> xmap_ctx_foldin (the batch's AlterEgo profiles)
//                     -> [rec_sim -> rec_select] -> xmap_ctx_foldin_predict | xmap_ctx_foldin_recommend (the same kernels, the batch's rows)
//   item fold-in, for items that were not in the upload:  rec_sim -> rec_select -> xmap_ctx_item_foldin (rows, lists, extended tables)
//                     -> xmap_ctx_item_foldin_audience | _predict | _recommend (the same kernels, tables of I + n_new items)
//   related items for a basket:  rec_sim -> xmap_ctx_related (the top-N over the RecommenderSim rows of the basket's members; no lists)
//   explanations of (user, item) pairs: xmap_ctx_explain | xmap_ctx_foldin_explain, wherever xmap_ctx_predict | xmap_ctx_foldin_predict work
//   xmap_ctx_*_download copy results into caller-allocated host buffers whose sizes the stage call reported.
//
// Everything below is orchestration of the kernels' own entry points (include/xmap_hip.h): buffer sizes, prefix sums,
// overflow retries and unit planning that xmap/engine/device.py does for the Python host.  No torch, no other library.
#include <math.h>
#include <stdlib.h>
#include <algorithm>
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
static int dalloc(Pool &pool, T **out, size_t n, hipStream_t st, bool zero = false) {
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
static int h2d(Pool &pool, T **out, const T *host, size_t n, hipStream_t st) {
    XM_TRY(dalloc(pool, out, n, st));
    if (n) XM_HIP(hipMemcpyAsync(*out, host, sizeof(T) * n, hipMemcpyHostToDevice, st));
    return XMAP_OK;
}
template <typename T>
static int d2h(T *host, const T *dev, size_t n, hipStream_t st) {
    if (n) XM_HIP(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, st));
    return XMAP_OK;
}

// any earlier stage run again invalidates the recommender tail (as the stages invalidate each other)
static void drop_ifold(xmap_ctx *c) {
    c->p_ifold.release();
    c->have_ifold = false;
    c->if_new = c->if_pairs = 0;
}

static void drop_tail(xmap_ctx *c) {
    drop_ifold(c);
    c->p_nb.release(); c->p_rec.release(); c->p_div.release();
    c->have_rec = c->have_nb = c->have_div = false;
    for (int k = 0; k < 2; k++) { c->p_peer[k].release(); c->have_peer[k] = false; }
    c->p_pop.release(); c->have_pop = false;
}

// the fold-in batch hangs on the replacement map: upload, item_sim, extend and generate drop it; the tail calls leave it
// the union of other contexts' rows goes with whatever replaces it: an upload, or the next union
static void drop_union(xmap_ctx *c) {
    c->p_union.release();
    if (c->is_union) c->have_gen = false;
    c->is_union = false;
}

static void drop_labels(xmap_ctx *c) {
    c->p_lab.release();
    c->have_lab = false;
    c->n_labels = 0; c->n_lab = 0;
    c->h_lab_ptr.clear();
}

static void drop_fold(xmap_ctx *c) {
    c->p_fold.release();
    c->have_fold = false;
    c->f_users = c->f_rows = 0;
}

// one reverse adjacency: count -> scan -> fill
static int reverse_list(xmap_ctx *c, int mode, const uint8_t *bb, const int64_t *attach_ptr, const void *thr, int32_t *long_rows,
                        uint8_t *eflag, int32_t *counted /*the list's counts where a fused pass left them, or NULL*/,
                        const int64_t **rptr, const int32_t **ridx, const double **rval, const uint8_t **rflag) {
    const int I = c->R.n_items, k = c->top_k;
    int32_t *rcnt = counted;
    int64_t *ptr;
    XM_ALLOCZ(c->p_ext, ptr, I + 1);
    if (!counted) {
        XM_ALLOCZ(c->p_ext, rcnt, I);
        XM_TRY(xmap_reverse_count(c->st, &c->S, mode, k, bb, c->T.cls, c->T.kcnt, c->T.kcol, c->T.kval, c->R.suffix_cls,
                                  c->R.contains_mask, c->R.flags, attach_ptr, thr, long_rows, eflag, rcnt, 0, I));
    }
    int64_t n = 0;
    XM_TRY(xmap_exclusive_scan_i32_to_i64(c->st, rcnt, ptr, I, &n));
    int32_t *idx;
    double *val;
    uint8_t *flag;
    XM_ALLOC(c->p_ext, idx, n);
    XM_ALLOC(c->p_ext, val, 3 * (size_t)(n ? n : 1));
    XM_ALLOCZ(c->p_ext, flag, n);
    XM_TRY(xmap_reverse_fill(c->st, &c->S, mode, k, bb, c->T.cls, c->T.kcnt, c->T.kcol, c->T.kval, c->R.suffix_cls,
                             c->R.contains_mask, c->R.flags, attach_ptr, thr, long_rows, eflag, ptr, idx, val, flag, 0, I));
    *rptr = ptr; *ridx = idx; *rval = val; *rflag = flag;
    return XMAP_OK;
}

// accumulator rows of the enumeration: zero-filled once, reused while large enough
static int ensure_rows(xmap_ctx *c, int64_t slots, int64_t len, int64_t hrows) {
    if (c->acc == nullptr || c->acc_slots < slots || c->acc_len != len || c->hacc_rows < hrows) {
        c->p_rows.release();
        c->acc = nullptr; c->hacc = nullptr;
        XM_ALLOCZ(c->p_rows, c->acc, (size_t)slots * len * 4);
        XM_ALLOC(c->p_rows, c->touched, (size_t)slots * len);
        if (hrows) {
            XM_ALLOCZ(c->p_rows, c->hacc, (size_t)hrows * len * 4);
            XM_ALLOC(c->p_rows, c->htouched, (size_t)hrows * len);
        }
        c->acc_slots = slots; c->acc_len = len; c->hacc_rows = hrows;
    }
    return XMAP_OK;
}

static int run_enumeration(xmap_ctx *c, int64_t xs_cap, int64_t *xs_off, int32_t *xs_end, double *xs_val) {
    const int I = c->R.n_items;
    xmap_path_rows Rw;
    Rw.n_slots = c->n_slots; Rw.acc = c->acc; Rw.touched = c->touched; Rw.hacc = c->hacc; Rw.htouched = c->htouched;
    xmap_path_out O;
    O.n_cand = c->n_cand; O.top_end = c->top_end; O.top_val = c->top_val;
    O.xs_cap = xs_cap; O.xs_off = xs_off; O.xs_end = xs_end; O.xs_val = xs_val;
    XM_HIP(hipMemsetAsync(c->n_cand, 0, sizeof(int32_t) * (size_t)I, c->st));
    XM_HIP(hipMemsetAsync(c->top_end, 0xff, sizeof(int32_t) * (size_t)I * XMAP_TOPC, c->st));
    XM_HIP(hipMemsetAsync(c->top_val, 0, sizeof(double) * (size_t)I * XMAP_TOPC, c->st));
    int64_t *d_cnt;
    XM_ALLOCZ(c->p_ext, d_cnt, 8);
    int64_t h_cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int rc;
    // n_nb == 0 (nothing joint): the per-path kernel over item-indexed rows (the same row buffers, U = I)
    if (c->T.n_nb > 0) rc = xmap_extend_cols(c->st, &c->T, &c->Un, &Rw, &O, c->fast_div, d_cnt, h_cnt);
    else rc = xmap_extend_paths(c->st, &c->T, &c->Un, &Rw, &O, d_cnt, h_cnt);
    if (rc && rc != XMAP_ERR_CAPACITY) {     // a failed pass may leave partial sums in the rows
        c->p_rows.release();
        c->acc = nullptr;
    }
    c->n_out = h_cnt[0]; c->n_paths = h_cnt[1];
    return rc;
}

// ---- stage A of the coarse ABI.  What differs between xmap_ctx_item_sim (BaselinerSim over the ratings) and xmap_ctx_rec_sim
// (RecommenderSim over the AlterEgo profiles); scratch, sizing, retries and the order of the fine-grained calls are tri_pass's.
struct TriPass {
    const xmap_ratings *R;      // the ratings view (its item_ptr is written by the layout)
    const double *rating64;     // fp64 ratings (wide profile entries, rater records and sort records), or NULL: R->user_rating
    int ch_min, dups, method, cap;
    bool heavy;                 // run the rows of H (false: the layout has none)
    bool aux, skip_self;        // a sixth COO / CSR column (the pairs' local sensitivities); a row may pair with itself (no mirrored entry)
    int64_t half_contrib;       // sum over the users of d (d - 1) / 2: sizes the unit lists and the half COO
    Pool *stats_pool, *csr_pool, *mutu_pool;    // where u_avg / u_norm / info, the CSR columns and the mutu column are kept
    int64_t *row_ptr;           // [I + 1], zeroed: the CSR's row pointers
};
struct TriResult {
    double *u_avg, *u_norm /*NULL with rating64*/, *info, *norms /*in tmp*/, *sim, *aux;
    int32_t *col, *mutu, *nij;
    int64_t n, n_unordered, kept;   // kept / evaluated unordered pairs; room of the CSR columns (2 n: a self pair uses one of its two)
};

// layout -> plan(slot_target) -> pairs (again with smaller partitions after a table overflow, with more slack after a COO
// overflow; one host wait per attempt) -> mirrored counts -> mirror.  tmp: the pass's scratch, the caller's to release.
// The two host waits do not drain the stream (the order of Engine.item_sim_tri, xmap/engine/device.py): the profile copy's flag
// pass is queued behind the first plan's read-back, the mirrored counts behind the read-back of the pair kernels' counters.
static int tri_pass(hipStream_t st, const TriPass &J, Pool &tmp, TriResult &O) {
#define T_ALLOC(ptr, n) XM_TRY(dalloc(tmp, &(ptr), (size_t)(n), st))
#define T_ALLOCZ(ptr, n) XM_TRY(dalloc(tmp, &(ptr), (size_t)(n), st, true))
    const xmap_ratings &R = *J.R;
    const int I = R.n_items;
    const int64_t U = R.n_users, nnz = R.nnz;
    const bool wide = J.rating64 != nullptr;
    const size_t n1 = (size_t)(nnz ? nnz : 1), i1 = (size_t)(I ? I : 1);
    const size_t rw = wide ? 3 : 2;         // 64-bit words of a sort record
    // A2 / A3 + layout of the "tri" formulation: one transposition (xmap_sim3_layout); the CSC arrays stay unbuilt
    int32_t *cnt, *hist, *ctl, *hid, *hlist;
    int64_t *pre;
    uint64_t *ub_key, *ub, *rcrec, *Wp, *srec, *buf_a, *buf_b;
    O.u_norm = nullptr; O.aux = nullptr;
    XM_TRY(dalloc(*J.stats_pool, &O.u_avg, (size_t)U, st, wide));       // (fp64 ratings: the user averages are zero by construction)
    if (!wide) XM_TRY(dalloc(*J.stats_pool, &O.u_norm, (size_t)U, st));
    XM_TRY(dalloc(*J.stats_pool, &O.info, i1 * 4, st, true));
    T_ALLOCZ(O.norms, 2 * i1);
    T_ALLOC(cnt, i1);
    T_ALLOC(hist, U + 2); T_ALLOC(pre, U + 3); T_ALLOC(ctl, 4); T_ALLOC(hid, i1); T_ALLOCZ(hlist, 1024);
    T_ALLOC(ub_key, n1); T_ALLOC(ub, (wide ? 2 : 1) * n1); T_ALLOC(rcrec, 2 * n1); T_ALLOC(Wp, i1);
    T_ALLOC(srec, rw * n1); T_ALLOC(buf_a, rw * n1); T_ALLOC(buf_b, rw * n1);
    XM_TRY(xmap_sim3_layout(st, &R, (int64_t *)R.item_ptr, J.rating64, J.ch_min, XMAP_LAYOUT_RECORDS | XMAP_LAYOUT_STATS,
                            0, I, cnt, O.u_avg, O.u_norm, hist, pre, ctl, hid, hlist, ub_key, ub, srec, buf_a, buf_b, rcrec, Wp, O.info,
                            O.norms, nullptr));
    int32_t *Q, *Cc, *Qcat, *uq_item = nullptr, *uq_q = nullptr, *uc_item = nullptr, *uc_c = nullptr;
    uint8_t *small;
    int64_t *uq_ptr, *uc_ptr;
    T_ALLOCZ(Q, i1); T_ALLOCZ(Cc, i1); T_ALLOCZ(small, i1); T_ALLOC(Qcat, 5 * i1); T_ALLOCZ(uq_ptr, (size_t)5 * I + 1);
    T_ALLOCZ(uc_ptr, I + 1);
    int slot_target = 768;          // (75 % load of the 1024-slot tables; device.py: SLOT_TARGET / CH_MIN)
    double coo_slack = 1.0;
    int64_t hc[10];
    auto plan = [&](int target, bool ub_flags) -> int {
        const int64_t cap_light = J.half_contrib / target + I + 1, cap_heavy = nnz / J.ch_min + 1025;
        T_ALLOC(uq_item, cap_light); T_ALLOC(uq_q, 4 * cap_light); T_ALLOC(uc_item, cap_heavy); T_ALLOC(uc_c, cap_heavy);
        XM_TRY(xmap_sim3_plan_begin(st, &R, target, pre, hid, ctl, Q, Cc, small, Wp, Qcat, uq_ptr, uc_ptr, J.dups, uq_item, uq_q, uc_item, uc_c,
                                    cap_light, cap_heavy));
        // the profile copy's flags (the plan reads none of them): once, under the first plan's wait
        if (ub_flags && !wide)
            XM_TRY(xmap_sim3_layout(st, &R, (int64_t *)R.item_ptr, J.rating64, J.ch_min, XMAP_LAYOUT_UB_FLAGS, 0, I, cnt, O.u_avg, O.u_norm, hist,
                                    pre, ctl, hid, hlist, ub_key, ub, srec, buf_a, buf_b, rcrec, Wp, O.info, O.norms, nullptr));
        return xmap_sim3_plan_wait(cap_light, cap_heavy, hc);
    };
    XM_TRY(plan(slot_target, true));
    // all phases in one call: the heavy rows run on a side stream next to the class launches of the light rows; own and
    // mirrored row counts apart (mir), kept / evaluated pairs summed on the device
    const int phases = XMAP_PAIRS_RESET | XMAP_PAIRS_LIGHT | XMAP_PAIRS_MIRCOUNT | XMAP_PAIRS_SHARD_SUMS | XMAP_PAIRS_NO_MARKS |
                       (J.heavy ? XMAP_PAIRS_HEAVY | XMAP_PAIRS_HEAVY_MERGE : 0);
    int32_t *coo_i = nullptr, *coo_j = nullptr, *coo_mutu = nullptr, *coo_nij = nullptr, *own = nullptr, *mir = nullptr;
    double *coo_sim = nullptr, *coo_aux = nullptr;
    int64_t *d_shards = nullptr;
    int64_t cap_coo = 0;
    for (;;) {
        const int64_t n_light = hc[0], n_hu = J.heavy ? hc[1] : 0, n_heavy = J.heavy ? hc[9] : 0;
        cap_coo = ((int64_t)((double)(J.half_contrib > 0 ? J.half_contrib : 1) * coo_slack) / 4096 + 1100) * 4096;
        double *hp_hi, *hp_lo;
        int32_t *hp_cnt, *hp_mut;
        int64_t *d_cnt;
        T_ALLOC(coo_i, cap_coo); T_ALLOC(coo_j, cap_coo); T_ALLOC(coo_sim, cap_coo); T_ALLOC(coo_mutu, cap_coo); T_ALLOC(coo_nij, cap_coo);
        if (J.aux) T_ALLOC(coo_aux, cap_coo);
        T_ALLOC(own, i1); T_ALLOC(mir, i1);
        const size_t hp = (size_t)(n_hu ? n_hu : 1) * 1024;
        T_ALLOC(hp_hi, hp); T_ALLOC(hp_lo, hp); T_ALLOC(hp_cnt, hp); T_ALLOC(hp_mut, hp);
        T_ALLOCZ(d_cnt, 6); T_ALLOC(d_shards, 2 * 4096);
        XM_TRY(xmap_sim2_pairs(st, &R, J.method, J.cap, O.u_avg, O.norms, rcrec, ub, Q, small, uq_item, uq_q, hc + 2, 0, n_light, hid, hlist,
                               ctl, Cc, uc_ptr, uc_item, uc_c, (int32_t)n_hu, (int32_t)n_heavy, phases, hp_hi, hp_lo, hp_cnt, hp_mut, cap_coo, coo_i,
                               coo_j, coo_sim, coo_mutu, coo_nij, coo_aux, own, d_shards, d_cnt, mir));
        int64_t h_cnt[6];
        int32_t *mir_part;
        T_ALLOC(mir_part, cap_coo);
        XM_TRY(xmap_sim3_counters_begin(st, d_cnt));
        XM_TRY(xmap_sim3_mircount(st, I, cap_coo, coo_i, coo_j, d_shards, cap_coo, J.skip_self ? 1 : 0, mir_part, mir));
        XM_TRY(xmap_sim3_counters_wait(h_cnt));
        if (h_cnt[2]) {                 // an LDS pair table overflowed: smaller partitions
            if (slot_target <= 32) { set_error("pair-table overflow"); return XMAP_ERR_OVERFLOW; }
            slot_target /= 2;
            XM_TRY(plan(slot_target, false));
            continue;
        }
        if (h_cnt[3]) {                 // a half-COO shard overflowed: more slack
            if (coo_slack > 64) { set_error("half-COO overflow"); return XMAP_ERR_CAPACITY; }
            coo_slack *= 2;
            continue;
        }
        O.n = h_cnt[4]; O.n_unordered = h_cnt[5];
        break;
    }
    // mirror the half COO into the CSR (row = [own | mirrored], tile sort by the heavier item); a sixth column travels along
    const int64_t n = O.n;
    const size_t nn = (size_t)(n ? n : 1);
    O.kept = 2 * n;
    int64_t *mptr;
    int32_t *fill, *tot;
    uint64_t *mir_a, *mir_b;
    T_ALLOCZ(mptr, I + 1);
    XM_TRY(dalloc(*J.csr_pool, &O.col, (size_t)O.kept, st)); XM_TRY(dalloc(*J.csr_pool, &O.sim, (size_t)O.kept, st));
    XM_TRY(dalloc(*J.mutu_pool, &O.mutu, (size_t)O.kept, st)); XM_TRY(dalloc(*J.csr_pool, &O.nij, (size_t)O.kept, st));
    if (J.aux) XM_TRY(dalloc(*J.csr_pool, &O.aux, (size_t)O.kept, st));
    T_ALLOC(fill, i1); T_ALLOC(tot, i1); T_ALLOC(mir_a, (J.aux ? 4 : 3) * nn); T_ALLOC(mir_b, (J.aux ? 4 : 3) * nn);
    return xmap_sim3_mirror(st, I, cap_coo, coo_i, coo_j, coo_sim, coo_mutu, coo_nij, d_shards, n, own, mir, tot, J.row_ptr, mptr, fill, mir_a,
                            mir_b, O.col, O.sim, O.mutu, O.nij, coo_aux, O.aux, 0, I);
#undef T_ALLOC
#undef T_ALLOCZ
}

}  // namespace xmap

extern "C" {

int xmap_ctx_create(int device, xmap_ctx **out) {
    XM_ARG(out);
    *out = nullptr;
    XM_HIP(hipSetDevice(device));
    xmap_ctx *c = new xmap_ctx();
    c->device = device;
    memset(&c->R, 0, sizeof(c->R)); memset(&c->S, 0, sizeof(c->S)); memset(&c->T, 0, sizeof(c->T)); memset(&c->Un, 0, sizeof(c->Un));
    hipError_t e = hipStreamCreate(&c->st);
    if (e != hipSuccess) { delete c; set_error("hipStreamCreate -> %s", hipGetErrorString(e)); return XMAP_ERR_HIP; }
    *out = c;
    return XMAP_OK;
}

void xmap_ctx_destroy(xmap_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    drop_tail(c);
    drop_fold(c);
    drop_union(c);
    drop_labels(c);
    c->p_gen.release(); c->p_ext.release(); c->p_sim.release(); c->p_rows.release(); c->p_ratings.release();
    if (c->st) (void)hipStreamDestroy(c->st);
    delete c;
}

// The plain fp64 sums of cosine mode (an item's sums of r and r^2, a pair's dot product) are exact in any order when every
// rating is a multiple of 2^-e and U M^2 2^2e <= 2^53 (M = max |r|, U = users: no sum has more terms).  Otherwise cosine
// runs as XMAP_COSINE_EXACT; XMAP_EXACT_COSINE=1 in the environment forces that route.  (xmap/engine/exactness.py is the
// same rule for the Python host.)
static bool plain_sums_exact(int64_t U, int64_t nnz, const float *rating) {
    const char *force = getenv("XMAP_EXACT_COSINE");
    if (force && force[0] == '1') return false;
    double M = 0.0;
    int e = 0;
    for (int64_t k = 0; k < nnz; k++) {
        const double r = fabs((double)rating[k]);
        if (!(r <= 1e300)) return false;                   // inf, nan
        if (r > M) M = r;
        while (e <= 26 && ldexp(r, e) != floor(ldexp(r, e))) e++;
        if (e > 26) return false;
    }
    if (M == 0.0) return true;
    const double Mi = ldexp(M, e);                         // an integer
    if (Mi > 134217728.0) return false;                    // Mi^2 > 2^54
    const uint64_t m2 = (uint64_t)Mi * (uint64_t)Mi;
    return (uint64_t)U <= (1ull << 53) / m2;
}

/* What the stages assume of an upload and never test themselves (host code, O(nnz), no device call): profile lengths are
 * differences of user_ptr, stage A sizes its tables for profiles without a repeated item (dups = 0; only RecommenderSim's
 * AlterEgo profiles may hold one: allow_repeats), suffix_cls is a shift count of stage B.  The first offending position is
 * named in xmap_last_error().  stamp[i] = the last position of item i: a repeat is a stamp inside the running profile. */
int xmap_check_ratings(int64_t n_users, int32_t n_items, const int64_t *user_ptr, const int32_t *item, const int32_t *prefix_cls,
                       const int32_t *suffix_cls, int32_t allow_repeats) {
    XM_ARG(user_ptr && n_users >= 0 && n_items >= 0);
    if (user_ptr[0] != 0) { set_error("ratings: user_ptr[0] = %lld, not 0", (long long)user_ptr[0]); return XMAP_ERR_ARG; }
    for (int64_t u = 0; u < n_users; u++)
        if (user_ptr[u + 1] < user_ptr[u]) {
            set_error("ratings: user_ptr[%lld] < user_ptr[%lld]", (long long)u + 1, (long long)u);
            return XMAP_ERR_ARG;
        }
    const int64_t nnz = user_ptr[n_users];
    if (nnz >= 2147483647ll) { set_error("ratings: user_ptr[%lld] = %lld does not fit int32", (long long)n_users, (long long)nnz); return XMAP_ERR_ARG; }
    XM_ARG(nnz == 0 || item);
    for (int64_t e = 0; e < nnz; e++)
        if (item[e] < 0 || item[e] >= n_items) {
            set_error("ratings: item[%lld] = %d outside [0, %d)", (long long)e, (int)item[e], (int)n_items);
            return XMAP_ERR_ARG;
        }
    if (!allow_repeats && nnz > 0) {
        std::vector<int64_t> stamp;
        try { stamp.assign((size_t)n_items, -1); }
        catch (const std::bad_alloc &) { set_error("ratings: out of host memory for %d stamps", (int)n_items); return XMAP_ERR_CAPACITY; }
        for (int64_t u = 0; u < n_users; u++)
            for (int64_t e = user_ptr[u]; e < user_ptr[u + 1]; e++) {
                int64_t &s = stamp[item[e]];
                if (s >= user_ptr[u]) {
                    set_error("ratings: user %lld holds item %d twice (item[%lld] and item[%lld])", (long long)u, (int)item[e],
                              (long long)s, (long long)e);
                    return XMAP_ERR_ARG;
                }
                s = e;
            }
    }
    for (int32_t i = 0; suffix_cls && i < n_items; i++)
        if (suffix_cls[i] < 0 || suffix_cls[i] >= 32) {
            set_error("ratings: suffix_cls[%d] = %d outside [0, 32)", (int)i, (int)suffix_cls[i]);
            return XMAP_ERR_ARG;
        }
    for (int32_t i = 0; prefix_cls && i < n_items; i++)
        if (prefix_cls[i] < 0) { set_error("ratings: prefix_cls[%d] = %d is negative", (int)i, (int)prefix_cls[i]); return XMAP_ERR_ARG; }
    return XMAP_OK;
}

int xmap_ctx_upload_ratings(xmap_ctx *c, int64_t n_users, int32_t n_items, const int64_t *user_ptr, const int32_t *item,
                            const float *rating, const int64_t *time, const int32_t *prefix_cls, const int32_t *suffix_cls,
                            const uint32_t *contains_mask, const uint8_t *flags) {
    XM_ARG(c && user_ptr && prefix_cls && suffix_cls && contains_mask && flags && n_users >= 0 && n_items >= 0);
    // a refused upload leaves the context as it was: nothing is dropped, allocated or launched before the input has passed
    XM_TRY(xmap_check_ratings(n_users, n_items, user_ptr, item, prefix_cls, suffix_cls, 0));
    XM_ARG(user_ptr[n_users] == 0 || (rating && time));
    XM_HIP(hipSetDevice(c->device));
    drop_tail(c);
    drop_fold(c);
    drop_union(c);
    drop_labels(c);             // the labels go with the item space
    c->p_gen.release(); c->p_ext.release(); c->p_sim.release(); c->p_ratings.release();
    c->have_sim = c->have_ext = c->have_gen = false;
    const int64_t nnz = user_ptr[n_users];
    xmap_ratings &R = c->R;
    memset(&R, 0, sizeof(R));
    R.n_users = n_users; R.n_items = n_items; R.nnz = nnz;
    c->half_contrib = 0;
    for (int64_t u = 0; u < n_users; u++) { const int64_t d = user_ptr[u + 1] - user_ptr[u]; c->half_contrib += d * (d - 1) / 2; }
    int64_t *d_ptr, *d_time, *d_iptr;
    int32_t *d_item, *d_iuser, *d_pre, *d_suf;
    float *d_rating, *d_irating;
    uint32_t *d_mask;
    uint8_t *d_flags;
    XM_TRY(h2d(c->p_ratings, &d_ptr, user_ptr, (size_t)n_users + 1, c->st));
    XM_TRY(h2d(c->p_ratings, &d_item, item, (size_t)nnz, c->st));
    XM_TRY(h2d(c->p_ratings, &d_rating, rating, (size_t)nnz, c->st));
    XM_TRY(h2d(c->p_ratings, &d_time, time, (size_t)nnz, c->st));
    XM_TRY(h2d(c->p_ratings, &d_pre, prefix_cls, (size_t)n_items, c->st));
    XM_TRY(h2d(c->p_ratings, &d_suf, suffix_cls, (size_t)n_items, c->st));
    XM_TRY(h2d(c->p_ratings, &d_mask, contains_mask, (size_t)n_items, c->st));
    XM_TRY(h2d(c->p_ratings, &d_flags, flags, (size_t)n_items, c->st));
    XM_ALLOCZ(c->p_ratings, d_iptr, n_items + 1);
    XM_ALLOCZ(c->p_ratings, d_iuser, nnz);
    XM_ALLOCZ(c->p_ratings, d_irating, nnz);
    R.user_ptr = d_ptr; R.user_item = d_item; R.user_rating = d_rating; R.user_time = d_time;
    R.item_ptr = d_iptr; R.item_user = d_iuser; R.item_rating = d_irating;
    R.prefix_cls = d_pre; R.suffix_cls = d_suf; R.contains_mask = d_mask; R.flags = d_flags;
    c->plain_exact = plain_sums_exact(n_users, nnz, rating);
    XM_HIP(hipStreamSynchronize(c->st));
    c->have_ratings = true;
    return XMAP_OK;
}

int xmap_ctx_item_sim(xmap_ctx *c, int method, int cap, int64_t *n_kept, int64_t *n_evaluated) {
    XM_ARG(c && c->have_ratings && (method == XMAP_COSINE || method == XMAP_ADJUST_COSINE) && cap > 0);
    XM_HIP(hipSetDevice(c->device));
    drop_tail(c);
    drop_fold(c);
    c->p_gen.release(); c->p_ext.release(); c->p_sim.release();
    c->have_sim = c->have_ext = c->have_gen = false;
    xmap_ratings &R = c->R;
    const int I = R.n_items;
    const int pair_method = (method == XMAP_COSINE && !c->plain_exact) ? XMAP_COSINE_EXACT : method;
    ScratchPool tmp;                       // layout / plan / half COO: released at the end of the stage
    int64_t *row_ptr;
    XM_ALLOCZ(c->p_sim, row_ptr, I + 1);
    TriPass J;
    J.R = &R; J.rating64 = nullptr; J.ch_min = 2048; J.dups = 0; J.method = pair_method; J.cap = cap;
    J.heavy = true; J.aux = false; J.skip_self = false; J.half_contrib = c->half_contrib;
    J.stats_pool = J.csr_pool = J.mutu_pool = &c->p_sim; J.row_ptr = row_ptr;
    TriResult O;
    XM_TRY(tri_pass(c->st, J, tmp, O));
    XM_HIP(hipStreamSynchronize(c->st));
    c->u_avg = O.u_avg; c->u_norm = O.u_norm; c->info = O.info;
    c->S.n_items = I; c->S.row_ptr = row_ptr; c->S.col = O.col; c->S.sim = O.sim; c->S.mutu = O.mutu; c->S.nij = O.nij; c->S.info = c->info;
    c->S.frac = nullptr;
    c->n_kept = O.kept; c->n_eval = 2 * O.n_unordered; c->n_contrib = 2 * c->half_contrib;
    c->have_sim = true;
    if (n_kept) *n_kept = c->n_kept;
    if (n_evaluated) *n_evaluated = c->n_eval;
    return XMAP_OK;
}

int xmap_ctx_sim_download(xmap_ctx *c, int64_t *row_ptr, int32_t *col, double *sim, int32_t *mutu, int32_t *nij, double *info,
                          double *user_avg) {
    XM_ARG(c && c->have_sim);
    XM_HIP(hipSetDevice(c->device));
    const int I = c->R.n_items;
    if (row_ptr) XM_TRY(d2h(row_ptr, c->S.row_ptr, (size_t)I + 1, c->st));
    if (col) XM_TRY(d2h(col, c->S.col, (size_t)c->n_kept, c->st));
    if (sim) XM_TRY(d2h(sim, c->S.sim, (size_t)c->n_kept, c->st));
    if (mutu) XM_TRY(d2h(mutu, c->S.mutu, (size_t)c->n_kept, c->st));
    if (nij) XM_TRY(d2h(nij, c->S.nij, (size_t)c->n_kept, c->st));
    if (info) XM_TRY(d2h(info, (const double *)c->info, (size_t)I * 4, c->st));
    if (user_avg) XM_TRY(d2h(user_avg, (const double *)c->u_avg, (size_t)c->R.n_users, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

int xmap_ctx_extend(xmap_ctx *c, int top_k, int64_t *n_out, int64_t *n_paths) {
    XM_ARG(c && c->have_sim && top_k >= 1);
    XM_HIP(hipSetDevice(c->device));
    drop_tail(c);
    drop_fold(c);
    c->p_gen.release(); c->p_ext.release();
    c->have_ext = c->have_gen = false;
    const int I = c->R.n_items, k = top_k;
    c->top_k = k;
    xmap_ext_tables &T = c->T;
    memset(&T, 0, sizeof(T));
    T.n_items = I; T.top_k = k; T.flags = c->R.flags;
    XM_ALLOCZ(c->p_ext, c->n_cand, I);
    XM_ALLOC(c->p_ext, c->top_end, (size_t)I * XMAP_TOPC);
    XM_ALLOCZ(c->p_ext, c->top_val, (size_t)I * XMAP_TOPC);
    c->n_out = c->n_paths = 0;
    if (I == 0) { c->have_ext = true; if (n_out) *n_out = 0; if (n_paths) *n_paths = 0; return XMAP_OK; }
    // B1-B4: bridge flags, classified top-k lists
    uint8_t *bb, *cls;
    int32_t *kcnt, *kcol;
    double *kval;
    XM_ALLOCZ(c->p_ext, bb, I); XM_ALLOC(c->p_ext, cls, I); XM_ALLOC(c->p_ext, kcnt, (size_t)I * 2);       // (xmap_knn_classify writes
    XM_ALLOC(c->p_ext, kcol, (size_t)I * 2 * k); XM_ALLOC(c->p_ext, kval, (size_t)I * 2 * k * 3);          //  every entry of its rows)
    XM_TRY(xmap_bridge_flags(c->st, &c->S, c->R.prefix_cls, bb));
    XM_TRY(xmap_knn_classify(c->st, &c->S, k, bb, c->R.suffix_cls, c->R.contains_mask, cls, kcnt, kcol, kval, 0, I));
    T.cls = cls; T.kcnt = kcnt; T.kcol = kcol; T.kval = kval;
    XM_TRY(xmap_edge_ranges(c->st, &c->S, &c->fast_div));
    // B5a/b: reverse adjacencies
    double *thr;
    int32_t *long_rows;
    XM_ALLOC(c->p_ext, thr, (size_t)I * 4);
    XM_ALLOC(c->p_ext, long_rows, I + 1);
    uint8_t *eflag;                         // one byte per entry of the matrix: what a count pass found, for its fill pass
    XM_ALLOC(c->p_ext, eflag, (size_t)(c->n_kept > 0 ? c->n_kept : 1));
    XM_TRY(xmap_knn_thresholds(c->st, I, k, kcnt, kcol, kval, thr));
    const uint8_t *dummy;
    // attach and rnn lists: ONE count pass over the matrix for both, then their fill passes; then the src lists (whose
    // predicate reads the attach offsets)
    int32_t *cnt_att, *cnt_rnn;
    XM_ALLOCZ(c->p_ext, cnt_att, I);
    XM_ALLOCZ(c->p_ext, cnt_rnn, I);
    XM_TRY(xmap_reverse_count_att_rnn(c->st, &c->S, k, bb, cls, kcnt, kcol, kval, c->R.suffix_cls, c->R.contains_mask, c->R.flags,
                                      thr, long_rows, eflag, cnt_att, cnt_rnn, 0, I));
    XM_TRY(reverse_list(c, 0, bb, nullptr, thr, long_rows, eflag, cnt_att, &T.att_ptr, &T.att_idx, &T.att_val, &dummy));
    XM_TRY(reverse_list(c, 2, bb, nullptr, thr, long_rows, eflag, cnt_rnn, &T.rnn_ptr, &T.rnn_idx, &T.rnn_val, &dummy));
    XM_TRY(reverse_list(c, 1, bb, T.att_ptr, thr, long_rows, eflag, nullptr, &T.src_ptr, &T.src_idx, &T.src_val, &T.src_flag));
    // exact per-start path counts -> work units
    int64_t *wtmp, *P;
    XM_ALLOCZ(c->p_ext, wtmp, (size_t)4 * I); XM_ALLOCZ(c->p_ext, P, I);
    XM_TRY(xmap_path_weights(c->st, &T, wtmp, P));
    // middle lists of the joint paths (row-wise construction)
    int32_t *nb_list, *nb_id;
    int64_t n_nb = 0;
    XM_ALLOC(c->p_ext, nb_list, I); XM_ALLOC(c->p_ext, nb_id, I);
    XM_TRY(xmap_nb_index(c->st, I, cls, nb_list, nb_id, &n_nb));
    T.n_nb = (int32_t)n_nb; T.nb_list = nb_list; T.nb_id = nb_id;
    if (n_nb > 0) {
        int32_t *ng;
        int64_t *nrec, *dir_ptr, *rec_ptr, n_tiles = 0, n_records = 0;
        void *dir, *midX;
        XM_ALLOC(c->p_ext, ng, n_nb); XM_ALLOC(c->p_ext, nrec, n_nb); XM_ALLOCZ(c->p_ext, dir_ptr, n_nb + 1); XM_ALLOCZ(c->p_ext, rec_ptr, n_nb + 1);
        XM_TRY(xmap_mid_rows_count(c->st, &T, ng, nrec));
        XM_TRY(xmap_exclusive_scan_i32_to_i64(c->st, ng, dir_ptr, n_nb, &n_tiles));
        XM_TRY(xmap_exclusive_scan_i64(c->st, nrec, rec_ptr, n_nb, &n_records));
        char *dir_c, *mid_c;
        XM_ALLOC(c->p_ext, dir_c, (size_t)(n_tiles ? n_tiles : 1) * 24);
        XM_ALLOC(c->p_ext, mid_c, (size_t)(n_records ? n_records : 1) * 64);
        dir = dir_c; midX = mid_c;
        T.dir_ptr = dir_ptr;
        XM_TRY(xmap_mid_rows_place(c->st, &T, rec_ptr, dir, midX));
        T.dir = dir; T.midX = midX;
    }
    // end universe (rows are indexed by end rank, in column order)
    int64_t len = I;
    if (n_nb > 0) {
        int32_t *mark, *urank, *uitem;
        int64_t *rank, n_ends = 0;
        XM_ALLOC(c->p_ext, mark, I); XM_ALLOC(c->p_ext, rank, I + 1); XM_ALLOC(c->p_ext, urank, I); XM_ALLOC(c->p_ext, uitem, I);
        XM_TRY(xmap_end_universe(c->st, &T, mark, rank, urank, uitem, &n_ends));
        XM_TRY(xmap_end_order(c->st, I, k, (int32_t)n_nb, nb_list, kcnt, kcol, (int32_t)n_ends, urank, uitem));
        T.n_ends = (int32_t)n_ends; T.urank = urank; T.uitem = uitem;
        len = n_ends > 0 ? n_ends : 1;
    }
    // work units; accumulator rows: one per resident wavefront (xmap_extend_cols_slots), capped by 24 GB
    int32_t resident = 0;
    XM_TRY(xmap_extend_cols_slots(&resident));
    int64_t n_slots = resident;
    const int64_t slot_cap = ((int64_t)24 << 30) / (36 * len);
    if (n_slots > slot_cap) n_slots = slot_cap > 4 ? slot_cap : 4;
    const int64_t max_rows = ((int64_t)16 << 30) / (36 * len) > 2 ? ((int64_t)16 << 30) / (36 * len) : 2;
    const int64_t cap_units = (int64_t)I + max_rows;
    int32_t *unit_start, *unit_c, *unit_G, *unit_row, *unit_nt, *heavy_unit0;
    XM_ALLOC(c->p_ext, unit_start, cap_units); XM_ALLOC(c->p_ext, unit_c, cap_units); XM_ALLOC(c->p_ext, unit_G, cap_units);
    XM_ALLOC(c->p_ext, unit_row, cap_units); XM_ALLOC(c->p_ext, heavy_unit0, I);
    int64_t hp[5];
    XM_TRY(xmap_path_plan(c->st, I, P, 0, I, 0, 8192, max_rows, cap_units, unit_start, unit_c, unit_G, unit_row, heavy_unit0, hp));
    XM_ALLOCZ(c->p_ext, unit_nt, hp[0]);
    xmap_path_units &Un = c->Un;
    Un.n_units = (int32_t)hp[0]; Un.unit_start = unit_start; Un.unit_c = unit_c; Un.unit_G = unit_G; Un.unit_row = unit_row;
    Un.unit_nt = unit_nt; Un.n_heavy = (int32_t)hp[1]; Un.heavy_unit0 = heavy_unit0;
    if (n_slots > hp[0]) n_slots = hp[0] > 4 ? hp[0] : 4;
    c->n_slots = (int32_t)n_slots;
    XM_TRY(ensure_rows(c, n_slots, len, hp[2]));
    XM_TRY(run_enumeration(c, 0, nullptr, nullptr, nullptr));
    c->have_ext = true;
    if (n_out) *n_out = c->n_out;
    if (n_paths) *n_paths = c->n_paths;
    return XMAP_OK;
}

int xmap_ctx_ext_download(xmap_ctx *c, int32_t *n_cand, int32_t *top_end, double *top_val) {
    XM_ARG(c && c->have_ext);
    XM_HIP(hipSetDevice(c->device));
    const size_t I = (size_t)c->R.n_items;
    if (n_cand) XM_TRY(d2h(n_cand, (const int32_t *)c->n_cand, I, c->st));
    if (top_end) XM_TRY(d2h(top_end, (const int32_t *)c->top_end, I * XMAP_TOPC, c->st));
    if (top_val) XM_TRY(d2h(top_val, (const double *)c->top_val, I * XMAP_TOPC, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

int xmap_ctx_ext_lists(xmap_ctx *c, int64_t *xs_off, int32_t *xs_end, double *xs_val) {
    XM_ARG(c && c->have_ext && xs_off && (c->n_out == 0 || (xs_end && xs_val)));
    XM_HIP(hipSetDevice(c->device));
    const int I = c->R.n_items;
    if (I == 0) return XMAP_OK;
    const int64_t cap = c->n_out > 0 ? c->n_out : 1;      // exact: the candidate counts of the first pass
    ScratchPool tmp;
    int64_t *d_off;
    int32_t *d_end;
    double *d_val;
    XM_TRY(dalloc(tmp, &d_off, (size_t)I, c->st, true));
    XM_TRY(dalloc(tmp, &d_end, (size_t)cap, c->st));
    XM_TRY(dalloc(tmp, &d_val, (size_t)cap, c->st));
    XM_TRY(run_enumeration(c, cap, d_off, d_end, d_val));
    XM_TRY(d2h(xs_off, (const int64_t *)d_off, (size_t)I, c->st));
    XM_TRY(d2h(xs_end, (const int32_t *)d_end, (size_t)c->n_out, c->st));
    XM_TRY(d2h(xs_val, (const double *)d_val, (size_t)c->n_out, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

int xmap_ctx_candidates(xmap_ctx *c, int32_t *n_top) {
    XM_ARG(c && c->have_ext && n_top);
    XM_HIP(hipSetDevice(c->device));
    const int I = c->R.n_items;
    if (I == 0) return XMAP_OK;
    ScratchPool tmp;
    int32_t *d_top, *d_choice, *d_map;
    XM_TRY(dalloc(tmp, &d_top, (size_t)I, c->st, true));
    XM_TRY(dalloc(tmp, &d_choice, (size_t)I, c->st, true));
    XM_TRY(dalloc(tmp, &d_map, (size_t)I, c->st, true));
    XM_TRY(xmap_select_map(c->st, I, 0, c->n_cand, c->top_end, nullptr, d_top, d_choice, d_map));
    XM_TRY(d2h(n_top, (const int32_t *)d_top, (size_t)I, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

int xmap_ctx_generate(xmap_ctx *c, int private_flag, const int32_t *picks, int32_t *choice, int64_t *n_rows, int64_t *n_target_rows) {
    XM_ARG(c && c->have_ext);
    XM_HIP(hipSetDevice(c->device));
    drop_tail(c);
    drop_fold(c);
    c->p_gen.release();
    c->have_gen = false;
    const int I = c->R.n_items;
    const int64_t U = c->R.n_users;
    int32_t *d_top, *d_choice, *d_map, *d_picks = nullptr;
    XM_ALLOCZ(c->p_gen, d_top, I); XM_ALLOCZ(c->p_gen, d_choice, I); XM_ALLOCZ(c->p_gen, d_map, I);
    if (picks) XM_TRY(h2d(c->p_gen, &d_picks, picks, (size_t)I, c->st));
    XM_TRY(xmap_select_map(c->st, I, private_flag ? 1 : 0, c->n_cand, c->top_end, d_picks, d_top, d_choice, d_map));
    if (choice) XM_TRY(d2h(choice, (const int32_t *)d_choice, (size_t)I, c->st));
    int32_t *cnt_t, *cnt_m;
    int64_t *off_t, *off_m, nt = 0, nm = 0;
    XM_ALLOCZ(c->p_gen, cnt_t, U); XM_ALLOCZ(c->p_gen, cnt_m, U); XM_ALLOCZ(c->p_gen, off_t, U + 1); XM_ALLOCZ(c->p_gen, off_m, U + 1);
    XM_TRY(xmap_alterego_count(c->st, &c->R, d_map, cnt_t, cnt_m, nullptr));
    XM_TRY(xmap_exclusive_scan_i32_to_i64(c->st, cnt_t, off_t, U, &nt));
    XM_TRY(xmap_exclusive_scan_i32_to_i64(c->st, cnt_m, off_m, U, &nm));
    const int64_t n = nt + nm;
    XM_ALLOC(c->p_gen, c->g_user, n); XM_ALLOC(c->p_gen, c->g_item, n); XM_ALLOC(c->p_gen, c->g_rating, n); XM_ALLOC(c->p_gen, c->g_time, n);
    XM_TRY(xmap_alterego_fill(c->st, &c->R, d_map, off_t, off_m, nt, c->g_user, c->g_item, c->g_rating, c->g_time));
    XM_HIP(hipStreamSynchronize(c->st));
    c->n_rows = n; c->n_target_rows = nt;
    c->g_off_t = off_t; c->g_off_m = off_m;
    c->g_map = d_map;
    c->have_gen = true;
    if (n_rows) *n_rows = n;
    if (n_target_rows) *n_target_rows = nt;
    return XMAP_OK;
}

int xmap_ctx_gen_download(xmap_ctx *c, int32_t *user, int32_t *item, double *rating, int64_t *time) {
    XM_ARG(c && c->have_gen && !c->is_union);
    XM_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)c->n_rows;
    if (user) XM_TRY(d2h(user, (const int32_t *)c->g_user, n, c->st));
    if (item) XM_TRY(d2h(item, (const int32_t *)c->g_item, n, c->st));
    if (rating) XM_TRY(d2h(rating, (const double *)c->g_rating, n, c->st));
    if (time) XM_TRY(d2h(time, (const int64_t *)c->g_time, n, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

// ---- the recommender tail ---------------------------------------------------------------------------------------------

int xmap_ctx_rec_sim(xmap_ctx *c, int cap, int64_t *n_pairs) {
    XM_ARG(c && c->have_gen && cap > 0);
    XM_HIP(hipSetDevice(c->device));
    drop_tail(c);
    const int I = c->R.n_items;
    const int64_t U = c->R.n_users, nnz = c->n_rows;
    XM_ARG(nnz < 2147483647ll);
    const size_t n1 = (size_t)(nnz ? nnz : 1), i1 = (size_t)(I ? I : 1);
    // (a) user-major profiles in stage-C row order
    XM_ALLOCZ(c->p_rec, c->pf_ptr, U + 1);
    XM_ALLOC(c->p_rec, c->pf_item, n1); XM_ALLOC(c->p_rec, c->pf_rating, n1); XM_ALLOC(c->p_rec, c->pf_time, n1);
    if (c->is_union) {              // the union's rows are profiles already
        XM_HIP(hipMemcpyAsync(c->pf_ptr, c->un_ptr, sizeof(int64_t) * (size_t)(U + 1), hipMemcpyDeviceToDevice, c->st));
        if (nnz) {
            XM_HIP(hipMemcpyAsync(c->pf_item, c->un_item, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToDevice, c->st));
            XM_HIP(hipMemcpyAsync(c->pf_rating, c->un_rating, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, c->st));
            XM_HIP(hipMemcpyAsync(c->pf_time, c->un_time, sizeof(int64_t) * (size_t)nnz, hipMemcpyDeviceToDevice, c->st));
        }
    } else {
        XM_TRY(xmap_rec_profiles(c->st, U, nnz, c->n_target_rows, c->g_off_t, c->g_off_m, c->g_user, c->g_item, c->g_rating, c->g_time,
                                 c->pf_ptr, c->pf_item, c->pf_rating, c->pf_time));
    }
    XM_ALLOCZ(c->p_rec, c->rs_row_ptr, I + 1);
    XM_ALLOCZ(c->p_rec, c->rs_avg, i1); XM_ALLOCZ(c->p_rec, c->rs_norm, i1);
    c->rec_pairs = 0;
    c->rec_cap = cap;
    if (I == 0 || nnz == 0) {
        XM_HIP(hipStreamSynchronize(c->st));
        c->have_rec = true;
        if (n_pairs) *n_pairs = 0;
        return XMAP_OK;
    }
    std::vector<int64_t> h_ptr((size_t)U + 1);
    XM_TRY(d2h(h_ptr.data(), (const int64_t *)c->pf_ptr, (size_t)U + 1, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    int64_t half_contrib = 0;
    for (int64_t u = 0; u < U; u++) { const int64_t d = h_ptr[u + 1] - h_ptr[u]; half_contrib += d * (d - 1) / 2; }
    ScratchPool tmp;
    // the profiles as the ratings of the pair machinery: fp64 ratings (wide records), zero user average, no heavy set
    xmap_ratings P = c->R;
    float *f_dummy, *f_irating;
    int64_t *item_ptr;
    int32_t *i_user;
    XM_ALLOCZ(tmp, f_dummy, n1); XM_ALLOCZ(tmp, f_irating, n1); XM_ALLOCZ(tmp, item_ptr, I + 1); XM_ALLOCZ(tmp, i_user, n1);
    P.nnz = nnz; P.user_ptr = c->pf_ptr; P.user_item = c->pf_item; P.user_rating = f_dummy; P.user_time = c->pf_time;
    P.item_ptr = item_ptr; P.item_user = i_user; P.item_rating = f_irating;
    // the RecommenderSim variant of the pair kernels: exact sums, nothing filtered, self pairs, local sensitivities
    TriPass J;
    J.R = &P; J.rating64 = c->pf_rating; J.dups = 1; J.method = XMAP_ADJUST_COSINE; J.cap = cap;
    J.ch_min = (int)((U + 2 > 64) ? U + 2 : 64);        // more raters than users: no item is heavy
    J.heavy = false; J.aux = true; J.skip_self = true; J.half_contrib = half_contrib;
    J.stats_pool = J.mutu_pool = &tmp; J.csr_pool = &c->p_rec; J.row_ptr = c->rs_row_ptr;
    TriResult O;
    XM_TRY(tri_pass(c->st, J, tmp, O));
    c->rec_cap = cap;
    c->rs_col = O.col; c->rs_sim = O.sim; c->rs_nij = O.nij; c->rs_ls = O.aux;
    // the item averages the prediction reads are the layout's (exact sum / n), the norms its adjusted norms (zero user average)
    XM_HIP(hipMemcpy2DAsync(c->rs_avg, sizeof(double), O.info, 4 * sizeof(double), sizeof(double), (size_t)I, hipMemcpyDeviceToDevice, c->st));
    XM_HIP(hipMemcpyAsync(c->rs_norm, O.norms + I, sizeof(double) * (size_t)I, hipMemcpyDeviceToDevice, c->st));
    int64_t kept = 0;           // a self pair is one entry: the CSR's length is its last row pointer
    XM_TRY(d2h(&kept, (const int64_t *)(c->rs_row_ptr + I), 1, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    c->rec_pairs = kept;
    c->have_rec = true;
    if (n_pairs) *n_pairs = kept;
    return XMAP_OK;
}

int xmap_ctx_rec_profiles_download(xmap_ctx *c, int64_t *prof_ptr, int32_t *prof_item, double *prof_rating, int64_t *prof_time) {
    XM_ARG(c && c->have_rec);
    XM_HIP(hipSetDevice(c->device));
    const size_t n = (size_t)c->n_rows;
    if (prof_ptr) XM_TRY(d2h(prof_ptr, (const int64_t *)c->pf_ptr, (size_t)c->R.n_users + 1, c->st));
    if (prof_item) XM_TRY(d2h(prof_item, (const int32_t *)c->pf_item, n, c->st));
    if (prof_rating) XM_TRY(d2h(prof_rating, (const double *)c->pf_rating, n, c->st));
    if (prof_time) XM_TRY(d2h(prof_time, (const int64_t *)c->pf_time, n, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

int xmap_ctx_rec_download(xmap_ctx *c, int64_t *row_ptr, int32_t *col, double *sim, double *ls, int32_t *nij, double *item_avg,
                          double *item_norm) {
    XM_ARG(c && c->have_rec);
    XM_HIP(hipSetDevice(c->device));
    const size_t I = (size_t)c->R.n_items, n = (size_t)c->rec_pairs;
    if (row_ptr) XM_TRY(d2h(row_ptr, (const int64_t *)c->rs_row_ptr, I + 1, c->st));
    if (col) XM_TRY(d2h(col, (const int32_t *)c->rs_col, n, c->st));
    if (sim) XM_TRY(d2h(sim, (const double *)c->rs_sim, n, c->st));
    if (ls) XM_TRY(d2h(ls, (const double *)c->rs_ls, n, c->st));
    if (nij) XM_TRY(d2h(nij, (const int32_t *)c->rs_nij, n, c->st));
    if (item_avg) XM_TRY(d2h(item_avg, (const double *)c->rs_avg, I, c->st));
    if (item_norm) XM_TRY(d2h(item_norm, (const double *)c->rs_norm, I, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

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

// user-major profiles the prediction and ranking kernels read: the resident AlterEgo rows, or a fold-in batch
struct Profiles {
    int64_t n_users;
    const int64_t *ptr, *time;
    const int32_t *item;
    const double *rating;
};
static Profiles resident_profiles(const xmap_ctx *c) { return Profiles{c->R.n_users, c->pf_ptr, c->pf_time, c->pf_item, c->pf_rating}; }
static Profiles foldin_profiles(const xmap_ctx *c) { return Profiles{c->f_users, c->f_ptr, c->f_time, c->f_item, c->f_rating}; }

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
static Tables resident_tables(const xmap_ctx *c) {
    return Tables{c->R.n_items, c->keep, c->nb_cnt, c->nb_col, c->nb_sim, c->rs_avg, c->R.n_items, nullptr, nullptr};
}
static Tables itemfold_tables(const xmap_ctx *c) {
    return Tables{(int32_t)(c->R.n_items + c->if_new), c->keep, c->x_cnt, c->x_col, c->x_sim, c->x_avg, c->R.n_items, c->if_ptr, c->if_user};
}
// the model of one coarse call (rec_model.h): profiles, tables and the call's decay table on the device
static RecModel rec_model(const Profiles &P, const Tables &T, const double *d_w, int32_t n_w) {
    return RecModel{P.n_users, T.n_items, T.keep, T.cnt, T.col, T.sim, P.ptr, P.item, P.rating, P.time, T.avg, d_w, n_w};
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
    ScratchPool tmp;
    int32_t *d_user, *d_item, *d_status;
    double *d_real = nullptr, *d_w, *d_plain, *d_decay, *d_mae;
    const size_t n = (size_t)n_test;
    XM_TRY(h2d(tmp, &d_user, test_user, n, c->st));
    XM_TRY(h2d(tmp, &d_item, test_item, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    if (test_rating) XM_TRY(h2d(tmp, &d_real, test_rating, n, c->st));
    XM_TRY(dalloc(tmp, &d_plain, n, c->st, true)); XM_TRY(dalloc(tmp, &d_decay, n, c->st, true));
    XM_TRY(dalloc(tmp, &d_status, n, c->st, true)); XM_TRY(dalloc(tmp, &d_mae, 3, c->st, true));
    XM_TRY(predict_rows(c->st, n_test, d_user, d_item, rec_model(P, T, d_w, n_w), d_plain, d_decay, d_status, max_now));
    if (mae) {
        XM_TRY(xmap_mae(c->st, n_test, d_status, d_real, d_plain, d_decay, d_mae));
        XM_TRY(d2h(mae, (const double *)d_mae, 3, c->st));
    }
    XM_TRY(d2h(out_plain, (const double *)d_plain, n, c->st));
    XM_TRY(d2h(out_decay, (const double *)d_decay, n, c->st));
    XM_TRY(d2h(status, (const int32_t *)d_status, n, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}

// The eligibility rules of a coarse call (xmap_rec_filter with HOST pointers), checked on the host before any device work, as
// xmap_ctx_foldin checks its batch
static int check_filter(const xmap_rec_filter *F, int64_t n_query) {
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
static int upload_filter(xmap_ctx *c, ScratchPool &tmp, const xmap_rec_filter *F, int64_t n_query, int64_t n, xmap_rec_filter *D) {
    D->allow = nullptr; D->ex_ptr = nullptr; D->ex_id = nullptr;
    D->min_score = F ? F->min_score : -__builtin_inf();
    if (!F) return XMAP_OK;
    if (F->allow) {
        uint32_t *d_allow;
        XM_TRY(h2d(tmp, &d_allow, F->allow, (size_t)((n + 31) / 32), c->st));
        D->allow = d_allow;
    }
    if (F->ex_ptr) {
        int64_t *d_ptr;
        int32_t *d_id;
        XM_TRY(h2d(tmp, &d_ptr, F->ex_ptr, (size_t)n_query + 1, c->st));
        XM_TRY(h2d(tmp, &d_id, F->ex_id, (size_t)F->ex_ptr[n_query], c->st));
        D->ex_ptr = d_ptr; D->ex_id = d_id;
    }
    return XMAP_OK;
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
    ScratchPool tmp;
    int32_t *d_user, *d_cnt, *d_item;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(h2d(tmp, &d_user, query_user, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_item, m, c->st));
    XM_TRY(dalloc(tmp, &d_plain, m, c->st)); XM_TRY(dalloc(tmp, &d_decay, m, c->st));
    xmap_rec_filter D;
    if (n_stats == 6) XM_TRY(upload_filter(c, tmp, F, n_query, T.n_items, &D));
    XM_TRY(topn_rows(c->st, n_query, d_user, n_top, rank_by, flags, rec_model(P, T, d_w, n_w), d_cnt, d_item, d_plain, d_decay,
                     n_stats == 6 ? &D : nullptr, stats, n_stats));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_item, m, c->st));
    XM_TRY(d2h(out_plain, (const double *)d_plain, m, c->st));
    XM_TRY(d2h(out_decay, (const double *)d_decay, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
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
    ScratchPool tmp;
    int32_t *d_item, *d_cnt, *d_user;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(h2d(tmp, &d_item, query_item, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_user, m, c->st));
    XM_TRY(dalloc(tmp, &d_plain, m, c->st)); XM_TRY(dalloc(tmp, &d_decay, m, c->st));
    xmap_rec_filter D;
    if (n_stats == 6) XM_TRY(upload_filter(c, tmp, F, n_query, P.n_users, &D));
    XM_TRY(audience_rows(c->st, n_query, d_item, n_top, rank_by, flags, rec_model(P, T, d_w, n_w), d_cnt, d_user, d_plain, d_decay, stats,
                         T.n_resident, T.new_ptr, T.new_user, n_stats == 6 ? &D : nullptr, n_stats));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_user, (const int32_t *)d_user, m, c->st));
    XM_TRY(d2h(out_plain, (const double *)d_plain, m, c->st));
    XM_TRY(d2h(out_decay, (const double *)d_decay, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
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
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN || source == XMAP_SRC_ITEM_FOLDIN);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_ARG(source != XMAP_SRC_ITEM_FOLDIN || c->have_ifold);
    return recommend_over(c, source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c),
                          source == XMAP_SRC_ITEM_FOLDIN ? itemfold_tables(c) : resident_tables(c), n_query, query_user, n_top, rank_by, flags,
                          wtab, n_w, out_cnt, out_item, out_plain, out_decay, stats, F, 6);
}

int xmap_ctx_audience_filtered(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by,
                               int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user, double *out_plain,
                               double *out_decay, const xmap_rec_filter *F, int64_t *stats) {
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN || source == XMAP_SRC_ITEM_FOLDIN);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_ARG(source != XMAP_SRC_ITEM_FOLDIN || (c->have_ifold && n_query >= 0));
    if (source == XMAP_SRC_ITEM_FOLDIN) {       // query_item = indices into the batch
        const std::vector<int32_t> q = batch_items(c, n_query, query_item);
        return audience_over(c, resident_profiles(c), itemfold_tables(c), n_query, query_item ? q.data() : nullptr, n_top, rank_by, flags,
                             wtab, n_w, out_cnt, out_user, out_plain, out_decay, stats, F, 6);
    }
    return audience_over(c, source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c), resident_tables(c), n_query, query_item,
                         n_top, rank_by, flags, wtab, n_w, out_cnt, out_user, out_plain, out_decay, stats, F, 6);
}

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
    XM_TRY(check_filter(F, n_groups));
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN || source == XMAP_SRC_ITEM_FOLDIN);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_ARG(source != XMAP_SRC_ITEM_FOLDIN || c->have_ifold);
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 8; k++) stats[k] = 0;
    if (n_groups == 0) return XMAP_OK;
    const Profiles P = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    const Tables T = source == XMAP_SRC_ITEM_FOLDIN ? itemfold_tables(c) : resident_tables(c);
    ScratchPool tmp;
    int64_t *d_ptr;
    int32_t *d_user = nullptr, *d_cnt, *d_item, *d_low;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_groups, m = n * (size_t)n_top;
    XM_TRY(h2d(tmp, &d_ptr, grp_ptr, n + 1, c->st));
    if (n_mem > 0) XM_TRY(h2d(tmp, &d_user, grp_user, (size_t)n_mem, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_item, m, c->st)); XM_TRY(dalloc(tmp, &d_low, m, c->st));
    XM_TRY(dalloc(tmp, &d_plain, m, c->st)); XM_TRY(dalloc(tmp, &d_decay, m, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_groups, T.n_items, &D));
    XM_TRY(group_topn_rows(c->st, n_groups, d_ptr, d_user, n_top, rank_by, flags, how, veto, rec_model(P, T, d_w, n_w), d_cnt, d_item, d_plain,
                           d_decay, d_low, &D, stats));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_item, m, c->st));
    XM_TRY(d2h(out_plain, (const double *)d_plain, m, c->st));
    XM_TRY(d2h(out_decay, (const double *)d_decay, m, c->st));
    XM_TRY(d2h(out_low, (const int32_t *)d_low, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
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
    XM_ARG(source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN);       // the rows of batch items are not part of the index
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
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
    const Profiles P = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    const Tables T = resident_tables(c);
    ScratchPool tmp;
    int32_t *d_user, *p_cnt, *p_item, *d_cnt, *d_item, *d_pos;
    double *d_w, *p_plain, *p_decay, *d_plain, *d_decay, *d_pen, *d_ils;
    const size_t n = (size_t)n_query, mp = n * (size_t)n_pool, m = n * (size_t)n_top;
    XM_TRY(h2d(tmp, &d_user, query_user, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &p_cnt, n, c->st)); XM_TRY(dalloc(tmp, &p_item, mp, c->st));
    XM_TRY(dalloc(tmp, &p_plain, mp, c->st)); XM_TRY(dalloc(tmp, &p_decay, mp, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_item, m, c->st)); XM_TRY(dalloc(tmp, &d_pos, m, c->st));
    XM_TRY(dalloc(tmp, &d_plain, m, c->st)); XM_TRY(dalloc(tmp, &d_decay, m, c->st));
    XM_TRY(dalloc(tmp, &d_pen, m, c->st)); XM_TRY(dalloc(tmp, &d_ils, n, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_query, T.n_items, &D));
    int64_t h6[6] = {0, 0, 0, 0, 0, 0}, h2[2] = {0, 0};
    XM_TRY(topn_rows(c->st, n_query, d_user, n_pool, rank_by, flags, rec_model(P, T, d_w, n_w), p_cnt, p_item, p_plain, p_decay, &D, h6, 6));
    XM_TRY(xmap_diversify_rows(c->st, n_query, n_pool, p_cnt, p_item, p_plain, p_decay, rank_by, weight, n_top, I, c->rs_row_ptr,
                               c->dv_col, c->dv_abs, d_cnt, d_item, d_plain, d_decay, d_pos, d_pen, d_ils, h2));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_item, m, c->st));
    XM_TRY(d2h(out_plain, (const double *)d_plain, m, c->st));
    XM_TRY(d2h(out_decay, (const double *)d_decay, m, c->st));
    XM_TRY(d2h(out_pen, (const double *)d_pen, m, c->st));
    XM_TRY(d2h(out_ils, (const double *)d_ils, n, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
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
    XM_ARG(source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN);       // an item fold-in adds items, not users
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_user && out_cnt && out_user && out_sim && out_common)));
    XM_ARG(!with_ls || out_ls);
    XM_TRY(check_filter(F, n_query));
    XM_ARG(c && c->have_gen && c->have_rec);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 6; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    const int32_t I = c->R.n_items;
    const int64_t U = c->R.n_users;
    const int z = (flags & XMAP_PEERS_CENTRED) ? 1 : 0;
    const double *centre = z ? c->rs_avg : nullptr;
    XM_TRY(peer_index_of(c, z));
    const Profiles Q = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    const int32_t fl = (flags & XMAP_PEERS_KEEP_SELF) | (source == XMAP_SRC_RESIDENT ? XMAP_PEERS_SAME : 0);
    ScratchPool tmp;
    int32_t *d_query, *d_cnt, *d_user, *d_common;
    double *d_sim;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(h2d(tmp, &d_query, query_user, n, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_user, m, c->st));
    XM_TRY(dalloc(tmp, &d_sim, m, c->st)); XM_TRY(dalloc(tmp, &d_common, m, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_query, U, &D));
    double *d_ls = nullptr;
    if (with_ls) {
        XM_TRY(dalloc(tmp, &d_ls, m, c->st));
        XM_TRY(xmap_peer_rows_ls(c->st, n_query, d_query, Q.n_users, Q.ptr, Q.item, Q.rating, fl, n_top, cap, min_common, U, I, centre,
                                 c->pr_hd_ptr[z], c->pr_hd_user[z], c->pr_hd_x[z], c->pr_nrm[z], 0, d_cnt, d_user, d_sim, d_common, d_ls,
                                 &D, stats));
    } else
        XM_TRY(xmap_peer_rows(c->st, n_query, d_query, Q.n_users, Q.ptr, Q.item, Q.rating, fl, n_top, cap, min_common, U, I, centre,
                              c->pr_hd_ptr[z], c->pr_hd_user[z], c->pr_hd_x[z], c->pr_nrm[z], 0, d_cnt, d_user, d_sim, d_common, &D, stats));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_user, (const int32_t *)d_user, m, c->st));
    XM_TRY(d2h(out_sim, (const double *)d_sim, m, c->st));
    XM_TRY(d2h(out_common, (const int32_t *)d_common, m, c->st));
    if (with_ls) XM_TRY(d2h(out_ls, (const double *)d_ls, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
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

static int uknn_lists(xmap_ctx *c, ScratchPool &tmp, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_nb,
                      int32_t peer_flags, int32_t cap, int32_t min_common, UknnLists *L) {
    const int32_t I = c->R.n_items;
    const int64_t U = c->R.n_users;
    const int z = (peer_flags & XMAP_PEERS_CENTRED) ? 1 : 0;
    XM_TRY(peer_index_of(c, z));
    L->Q = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    const int32_t fl = (peer_flags & XMAP_PEERS_KEEP_SELF) | (source == XMAP_SRC_RESIDENT ? XMAP_PEERS_SAME : 0);
    const size_t n = (size_t)n_query, m = n * (size_t)n_nb;
    int32_t *d_common, *d_ucnt, *d_qcnt;
    XM_TRY(h2d(tmp, &L->query, query_user, n, c->st));
    XM_TRY(dalloc(tmp, &L->cnt, n, c->st)); XM_TRY(dalloc(tmp, &L->user, m, c->st));
    XM_TRY(dalloc(tmp, &L->sim, m, c->st)); XM_TRY(dalloc(tmp, &d_common, m, c->st));
    XM_TRY(xmap_peer_rows(c->st, n_query, L->query, L->Q.n_users, L->Q.ptr, L->Q.item, L->Q.rating, fl, n_nb, cap, min_common, U, I,
                          z ? c->rs_avg : nullptr, c->pr_hd_ptr[z], c->pr_hd_user[z], c->pr_hd_x[z], c->pr_nrm[z], 0, L->cnt, L->user,
                          L->sim, d_common, nullptr, nullptr));
    XM_TRY(dalloc(tmp, &L->user_avg, (size_t)U, c->st)); XM_TRY(dalloc(tmp, &d_ucnt, (size_t)U, c->st));
    XM_TRY(xmap_uknn_means(c->st, U, I, c->pf_ptr, c->pf_item, c->pf_rating, L->user_avg, d_ucnt));
    const double *src = L->user_avg;
    if (source == XMAP_SRC_FOLDIN) {
        double *d_qavg;
        XM_TRY(dalloc(tmp, &d_qavg, (size_t)L->Q.n_users, c->st)); XM_TRY(dalloc(tmp, &d_qcnt, (size_t)L->Q.n_users, c->st));
        XM_TRY(xmap_uknn_means(c->st, L->Q.n_users, I, L->Q.ptr, L->Q.item, L->Q.rating, d_qavg, d_qcnt));
        src = d_qavg;
    }
    XM_TRY(dalloc(tmp, &L->query_avg, n, c->st));
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
    XM_ARG(source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN);       // an item fold-in adds items, not users
    XM_ARG(n_test >= 0 && (n_test == 0 || (test_user && test_item && out_score && out_bound && out_n && status)));
    XM_ARG(!mae || test_rating || n_test == 0);
    XM_ARG(c && c->have_gen && c->have_rec);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_HIP(hipSetDevice(c->device));
    if (mae) mae[0] = mae[1] = 0.0;
    if (n_test == 0) return XMAP_OK;
    // the distinct users of the pairs are the queries (ascending); test_q = the pair's position among them
    std::vector<int32_t> users(test_user, test_user + n_test);
    std::sort(users.begin(), users.end());
    users.erase(std::unique(users.begin(), users.end()), users.end());
    std::vector<int32_t> tq((size_t)n_test);
    for (int64_t t = 0; t < n_test; t++) tq[(size_t)t] = (int32_t)(std::lower_bound(users.begin(), users.end(), test_user[t]) - users.begin());
    ScratchPool tmp;
    UknnLists L;
    XM_TRY(uknn_lists(c, tmp, source, (int64_t)users.size(), users.data(), n_nb, peer_flags, cap, min_common, &L));
    int32_t *d_q, *d_item, *d_n, *d_status;
    double *d_real = nullptr, *d_score, *d_bound, *d_mae;
    const size_t n = (size_t)n_test;
    XM_TRY(h2d(tmp, &d_q, (const int32_t *)tq.data(), n, c->st));
    XM_TRY(h2d(tmp, &d_item, test_item, n, c->st));
    if (test_rating) XM_TRY(h2d(tmp, &d_real, test_rating, n, c->st));
    XM_TRY(dalloc(tmp, &d_score, n, c->st)); XM_TRY(dalloc(tmp, &d_bound, n, c->st));
    XM_TRY(dalloc(tmp, &d_n, n, c->st)); XM_TRY(dalloc(tmp, &d_status, n, c->st)); XM_TRY(dalloc(tmp, &d_mae, 3, c->st, true));
    XM_TRY(xmap_uknn_predict_rows(c->st, n_test, d_q, d_item, (int64_t)users.size(), L.query_avg, n_nb, L.cnt, L.user, L.sim, c->R.n_users,
                                  c->R.n_items, c->pf_ptr, c->pf_item, c->pf_rating, L.user_avg, flags, d_score, d_bound, d_n, d_status));
    double h_mae[3] = {0.0, 0.0, 0.0};
    if (mae) {
        XM_TRY(xmap_mae(c->st, n_test, d_status, d_real, d_bound, d_bound, d_mae));
        XM_TRY(d2h(h_mae, (const double *)d_mae, 3, c->st));
    }
    XM_TRY(d2h(out_score, (const double *)d_score, n, c->st));
    XM_TRY(d2h(out_bound, (const double *)d_bound, n, c->st));
    XM_TRY(d2h(out_n, (const int32_t *)d_n, n, c->st));
    XM_TRY(d2h(status, (const int32_t *)d_status, n, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
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
    XM_ARG(source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN);       // an item fold-in adds items, not users
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_user && out_cnt && out_item && out_score && out_support)));
    XM_ARG(n_query * (int64_t)n_nb < 2147483647ll);
    XM_TRY(check_filter(F, n_query));
    XM_ARG(c && c->have_gen && c->have_rec);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 6; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    ScratchPool tmp;
    UknnLists L;
    XM_TRY(uknn_lists(c, tmp, source, n_query, query_user, n_nb, peer_flags, cap, min_common, &L));
    int32_t *d_cnt, *d_item, *d_support;
    double *d_score;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_item, m, c->st));
    XM_TRY(dalloc(tmp, &d_score, m, c->st)); XM_TRY(dalloc(tmp, &d_support, m, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_query, c->R.n_items, &D));
    XM_TRY(xmap_uknn_topn_rows(c->st, n_query, L.query, L.Q.n_users, L.Q.ptr, L.Q.item, L.query_avg, n_nb, L.cnt, L.user, L.sim, c->R.n_users,
                               c->R.n_items, c->pf_ptr, c->pf_item, c->pf_rating, L.user_avg, flags, n_top, min_support, 0, d_cnt, d_item,
                               d_score, d_support, &D, stats));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_item, m, c->st));
    XM_TRY(d2h(out_score, (const double *)d_score, m, c->st));
    XM_TRY(d2h(out_support, (const int32_t *)d_support, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
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
    ScratchPool tmp;
    int64_t *d_ptr;
    int32_t *d_member, *d_cnt, *d_item, *d_support;
    double *d_weight = nullptr, *d_score;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top, nb = (size_t)b_ptr[n_query];
    XM_TRY(h2d(tmp, &d_ptr, b_ptr, n + 1, c->st));
    XM_TRY(h2d(tmp, &d_member, b_item, nb, c->st));
    if (b_weight) XM_TRY(h2d(tmp, &d_weight, b_weight, nb, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_item, m, c->st));
    XM_TRY(dalloc(tmp, &d_score, m, c->st)); XM_TRY(dalloc(tmp, &d_support, m, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_query, c->R.n_items, &D));
    XM_TRY(xmap_related_rows(c->st, n_query, d_ptr, d_member, d_weight, c->R.n_items, c->rs_row_ptr, c->rs_col, c->rs_sim, how, flags, n_top,
                             min_support, max_records, d_cnt, d_item, d_score, d_support, &D, stats));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_item, m, c->st));
    XM_TRY(d2h(out_score, (const double *)d_score, m, c->st));
    XM_TRY(d2h(out_support, (const int32_t *)d_support, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
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
    XM_ARG(source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN || source == XMAP_SRC_ITEM_FOLDIN);
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query >= 0 && (n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay && out_src)));
    XM_TRY(check_filter(F, n_query));
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_ARG(source != XMAP_SRC_ITEM_FOLDIN || c->have_ifold);
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 10; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    XM_TRY(pop_index_of(c, how, damping, min_count));
    const Profiles P = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    const Tables T = source == XMAP_SRC_ITEM_FOLDIN ? itemfold_tables(c) : resident_tables(c);
    ScratchPool tmp;
    int32_t *d_user, *d_cnt, *d_item, *d_src;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(h2d(tmp, &d_user, query_user, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_item, m, c->st)); XM_TRY(dalloc(tmp, &d_src, m, c->st));
    XM_TRY(dalloc(tmp, &d_plain, m, c->st)); XM_TRY(dalloc(tmp, &d_decay, m, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_query, T.n_items, &D));
    int64_t h6[6] = {0, 0, 0, 0, 0, 0}, h4[4] = {0, 0, 0, 0};
    XM_TRY(topn_rows(c->st, n_query, d_user, n_top, rank_by, flags, rec_model(P, T, d_w, n_w), d_cnt, d_item, d_plain, d_decay, &D, h6, 6));
    XM_TRY(xmap_topn_fill_rows(c->st, n_query, d_user, n_top, flags, P.n_users, T.n_items, P.ptr, P.item, T.avg, (int32_t)c->pop_ranked,
                               c->pp_item, c->pp_pos, c->R.n_items, d_cnt, d_item, d_plain, d_decay, d_src, &D, h4));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_item, m, c->st));
    XM_TRY(d2h(out_plain, (const double *)d_plain, m, c->st));
    XM_TRY(d2h(out_decay, (const double *)d_decay, m, c->st));
    XM_TRY(d2h(out_src, (const int32_t *)d_src, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
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

int xmap_ctx_recommend_shelves(xmap_ctx *c, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_shelf, int32_t n_top,
                               int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t shelf_by, int32_t min_fill,
                               const uint32_t *lab_allow, int32_t *out_nshelf, int32_t *out_label, double *out_sscore, int32_t *out_size,
                               int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, const xmap_rec_filter *F,
                               int64_t *stats) {
    // the host checks: before the context is read, the outputs untouched, the context as it was
    const char *who = "xmap_ctx_recommend_shelves";
    XM_TRY(shelf_check_args(who, n_query, n_shelf, n_top, rank_by, flags, shelf_by, min_fill, 1, 0));
    if (source != XMAP_SRC_RESIDENT && source != XMAP_SRC_FOLDIN && source != XMAP_SRC_ITEM_FOLDIN) {
        set_error("%s: source = %d, not XMAP_SRC_RESIDENT, _FOLDIN or _ITEM_FOLDIN", who, source);
        return XMAP_ERR_ARG;
    }
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query == 0 || (query_user && out_nshelf && out_label && out_sscore && out_size && out_cnt && out_item && out_plain && out_decay));
    XM_TRY(check_filter(F, n_query));
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_ARG(source != XMAP_SRC_ITEM_FOLDIN || c->have_ifold);
    if (!c->have_lab) { set_error("%s: the context has no labels (xmap_ctx_set_labels)", who); return XMAP_ERR_ARG; }
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 10; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    const Profiles P = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    const Tables T = source == XMAP_SRC_ITEM_FOLDIN ? itemfold_tables(c) : resident_tables(c);
    ScratchPool tmp;
    const int64_t *d_lab_ptr = c->lb_ptr;
    if (T.n_items > c->R.n_items) {             // the batch items carry no label: lab_ptr extended by its last value
        std::vector<int64_t> ext(c->h_lab_ptr);
        ext.resize((size_t)T.n_items + 1, c->h_lab_ptr.back());
        int64_t *d_ext;
        XM_TRY(h2d(tmp, &d_ext, (const int64_t *)ext.data(), ext.size(), c->st));
        XM_HIP(hipStreamSynchronize(c->st));    // (ext leaves with this block)
        d_lab_ptr = d_ext;
    }
    uint32_t *d_allow = nullptr;
    if (lab_allow) XM_TRY(h2d(tmp, &d_allow, lab_allow, (size_t)((c->n_labels + 31) / 32), c->st));
    int32_t *d_user, *d_nshelf, *d_label, *d_size, *d_cnt, *d_item;
    double *d_w, *d_sscore, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, ns = n * (size_t)n_shelf, m = ns * (size_t)n_top;
    XM_TRY(h2d(tmp, &d_user, query_user, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &d_nshelf, n, c->st)); XM_TRY(dalloc(tmp, &d_label, ns, c->st)); XM_TRY(dalloc(tmp, &d_sscore, ns, c->st));
    XM_TRY(dalloc(tmp, &d_size, ns, c->st)); XM_TRY(dalloc(tmp, &d_cnt, ns, c->st)); XM_TRY(dalloc(tmp, &d_item, m, c->st));
    XM_TRY(dalloc(tmp, &d_plain, m, c->st)); XM_TRY(dalloc(tmp, &d_decay, m, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_query, T.n_items, &D));
    XM_TRY(shelf_rows(c->st, n_query, d_user, n_top, rank_by, flags, rec_model(P, T, d_w, n_w),
                      ShelfLabels{c->n_labels, d_lab_ptr, c->lb_id, d_allow}, n_shelf, shelf_by, min_fill, 0,
                      ShelfOut{d_nshelf, d_label, d_sscore, d_size, d_cnt, d_item, d_plain, d_decay}, &D, stats));
    XM_TRY(d2h(out_nshelf, (const int32_t *)d_nshelf, n, c->st));
    XM_TRY(d2h(out_label, (const int32_t *)d_label, ns, c->st));
    XM_TRY(d2h(out_sscore, (const double *)d_sscore, ns, c->st));
    XM_TRY(d2h(out_size, (const int32_t *)d_size, ns, c->st));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, ns, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_item, m, c->st));
    XM_TRY(d2h(out_plain, (const double *)d_plain, m, c->st));
    XM_TRY(d2h(out_decay, (const double *)d_decay, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
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
    if (source != XMAP_SRC_RESIDENT && source != XMAP_SRC_FOLDIN && source != XMAP_SRC_ITEM_FOLDIN) {
        set_error("%s: source = %d, not XMAP_SRC_RESIDENT, _FOLDIN or _ITEM_FOLDIN", who, source);
        return XMAP_ERR_ARG;
    }
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay && out_pos && out_label));
    XM_TRY(check_filter(F, n_query));
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_ARG(source != XMAP_SRC_ITEM_FOLDIN || c->have_ifold);
    if (!c->have_lab) { set_error("%s: the context has no labels (xmap_ctx_set_labels)", who); return XMAP_ERR_ARG; }
    XM_HIP(hipSetDevice(c->device));
    if (n_query == 0) {
        if (stats) for (int k = 0; k < 10; k++) stats[k] = 0;
        return XMAP_OK;
    }
    const Profiles P = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    const Tables T = source == XMAP_SRC_ITEM_FOLDIN ? itemfold_tables(c) : resident_tables(c);
    ScratchPool tmp;
    const int64_t *d_lab_ptr = c->lb_ptr;
    if (T.n_items > c->R.n_items) {             // the batch items carry no label: lab_ptr extended by its last value
        std::vector<int64_t> ext(c->h_lab_ptr);
        ext.resize((size_t)T.n_items + 1, c->h_lab_ptr.back());
        int64_t *d_ext;
        XM_TRY(h2d(tmp, &d_ext, (const int64_t *)ext.data(), ext.size(), c->st));
        XM_HIP(hipStreamSynchronize(c->st));    // (ext leaves with this block)
        d_lab_ptr = d_ext;
    }
    uint32_t *d_allow = nullptr, *d_weight = nullptr;
    int32_t *d_cap = nullptr;
    if (lab_allow) XM_TRY(h2d(tmp, &d_allow, lab_allow, (size_t)((c->n_labels + 31) / 32), c->st));
    if (lab_cap) XM_TRY(h2d(tmp, &d_cap, lab_cap, (size_t)c->n_labels, c->st));
    if (lab_weight) XM_TRY(h2d(tmp, &d_weight, lab_weight, (size_t)c->n_labels, c->st));
    int32_t *d_user, *d_cnt, *d_item, *d_pos, *d_label;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    XM_TRY(h2d(tmp, &d_user, query_user, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_item, m, c->st)); XM_TRY(dalloc(tmp, &d_plain, m, c->st));
    XM_TRY(dalloc(tmp, &d_decay, m, c->st)); XM_TRY(dalloc(tmp, &d_pos, m, c->st)); XM_TRY(dalloc(tmp, &d_label, m, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_query, T.n_items, &D));
    int64_t h10[10];
    XM_TRY(quota_rows(c->st, n_query, d_user, n_pool, n_top, rank_by, flags, rec_model(P, T, d_w, n_w), QuotaRule{mode, cap, d_cap, d_weight},
                      ShelfLabels{c->n_labels, d_lab_ptr, c->lb_id, d_allow}, QuotaOut{d_cnt, d_item, d_plain, d_decay, d_pos, d_label}, &D,
                      h10));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_item, m, c->st));
    XM_TRY(d2h(out_plain, (const double *)d_plain, m, c->st));
    XM_TRY(d2h(out_decay, (const double *)d_decay, m, c->st));
    XM_TRY(d2h(out_pos, (const int32_t *)d_pos, m, c->st));
    XM_TRY(d2h(out_label, (const int32_t *)d_label, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
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
    if (source != XMAP_SRC_RESIDENT && source != XMAP_SRC_FOLDIN && source != XMAP_SRC_ITEM_FOLDIN) {
        set_error("%s: source = %d, not XMAP_SRC_RESIDENT, _FOLDIN or _ITEM_FOLDIN", who, source);
        return XMAP_ERR_ARG;
    }
    XM_ARG(n_w >= 1 && wtab);
    XM_ARG(n_query == 0 || (query_user && out_cnt && out_item && out_plain && out_decay && out_pos));
    XM_TRY(check_filter(F, n_query));
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_ARG(source != XMAP_SRC_ITEM_FOLDIN || c->have_ifold);
    XM_HIP(hipSetDevice(c->device));
    const Profiles P = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    const Tables T = source == XMAP_SRC_ITEM_FOLDIN ? itemfold_tables(c) : resident_tables(c);
    if (item_cap && n_cap != T.n_items) {
        set_error("%s: n_cap = %d, the tables of the source hold %d items", who, n_cap, T.n_items);
        return XMAP_ERR_ARG;
    }
    ScratchPool tmp;
    int32_t *d_cap = nullptr, *d_taken = nullptr, *d_user, *d_cnt, *d_item, *d_pos;
    double *d_w, *d_plain, *d_decay;
    const size_t n = (size_t)n_query, m = n * (size_t)n_top, I = (size_t)T.n_items;
    if (item_cap) XM_TRY(h2d(tmp, &d_cap, item_cap, I, c->st));
    if (item_taken) XM_TRY(dalloc(tmp, &d_taken, I ? I : 1, c->st));
    XM_TRY(h2d(tmp, &d_user, query_user, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, n ? n : 1, c->st)); XM_TRY(dalloc(tmp, &d_item, m ? m : 1, c->st)); XM_TRY(dalloc(tmp, &d_plain, m ? m : 1, c->st));
    XM_TRY(dalloc(tmp, &d_decay, m ? m : 1, c->st)); XM_TRY(dalloc(tmp, &d_pos, m ? m : 1, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_query, T.n_items, &D));
    int64_t h12[12];
    XM_TRY(allot_rows(c->st, n_query, d_user, n_pool, n_top, rank_by, flags, rec_model(P, T, d_w, n_w), cap, d_cap,
                      AllotOut{d_cnt, d_item, d_plain, d_decay, d_pos, d_taken}, &D, h12));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_item, m, c->st));
    XM_TRY(d2h(out_plain, (const double *)d_plain, m, c->st));
    XM_TRY(d2h(out_decay, (const double *)d_decay, m, c->st));
    XM_TRY(d2h(out_pos, (const int32_t *)d_pos, m, c->st));
    if (item_taken) XM_TRY(d2h(item_taken, (const int32_t *)d_taken, I, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
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
    ScratchPool tmp;
    xmap_fuse_list D[XMAP_FUSE_MAX_LISTS];
    const size_t n = (size_t)n_query, m = n * (size_t)n_top;
    for (int l = 0; l < n_lists; l++) {
        const size_t ml = n * (size_t)lists[l].width;
        int32_t *d_c, *d_i;
        double *d_s = nullptr;
        XM_TRY(h2d(tmp, &d_c, lists[l].cnt, n, c->st));
        XM_TRY(h2d(tmp, &d_i, lists[l].item, ml, c->st));
        if (lists[l].score) XM_TRY(h2d(tmp, &d_s, lists[l].score, ml, c->st));
        D[l].cnt = d_c; D[l].item = d_i; D[l].score = d_s; D[l].width = lists[l].width; D[l].weight = lists[l].weight;
    }
    int32_t *d_cnt, *d_id, *d_lists;
    double *d_score;
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_id, m, c->st));
    XM_TRY(dalloc(tmp, &d_score, m, c->st)); XM_TRY(dalloc(tmp, &d_lists, m, c->st));
    XM_TRY(xmap_fuse_rows(c->st, n_query, n_lists, D, n_ids, how, rrf_c, min_lists, n_top, 0, d_cnt, d_id, d_score, d_lists, stats));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_id, (const int32_t *)d_id, m, c->st));
    XM_TRY(d2h(out_score, (const double *)d_score, m, c->st));
    XM_TRY(d2h(out_lists, (const int32_t *)d_lists, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
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
    XM_ARG(source == XMAP_SRC_RESIDENT || source == XMAP_SRC_FOLDIN);       // an item fold-in adds items, not users
    XM_ARG(n_query >= 0 && n_query <= (1ll << 28) && (n_query == 0 || (query_user && out_cnt && out_item && out_score && out_lists)));
    XM_ARG(n_query * (int64_t)n_nb < 2147483647ll);
    XM_TRY(check_filter(F, n_query));
    XM_ARG(c && c->have_gen && c->have_rec && c->have_nb);
    XM_ARG(source != XMAP_SRC_FOLDIN || c->have_fold);
    XM_HIP(hipSetDevice(c->device));
    if (stats) for (int k = 0; k < 17; k++) stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    const Profiles P = source == XMAP_SRC_FOLDIN ? foldin_profiles(c) : resident_profiles(c);
    const Tables T = resident_tables(c);
    ScratchPool tmp;
    const size_t n = (size_t)n_query, mi = n * (size_t)n_pool_items, mu = n * (size_t)n_pool_users, m = n * (size_t)n_top;
    // ---- list 0: the filtered item-kNN top-N, as xmap_ctx_recommend_filtered runs it
    int32_t *d_user, *i_cnt, *i_item;
    double *d_w, *i_plain, *i_decay;
    XM_TRY(h2d(tmp, &d_user, query_user, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &i_cnt, n, c->st)); XM_TRY(dalloc(tmp, &i_item, mi, c->st));
    XM_TRY(dalloc(tmp, &i_plain, mi, c->st)); XM_TRY(dalloc(tmp, &i_decay, mi, c->st));
    xmap_rec_filter D;
    XM_TRY(upload_filter(c, tmp, F, n_query, T.n_items, &D));
    int64_t h6[6] = {0, 0, 0, 0, 0, 0}, u6[6] = {0, 0, 0, 0, 0, 0}, f5[5] = {0, 0, 0, 0, 0};
    XM_TRY(topn_rows(c->st, n_query, d_user, n_pool_items, rank_by, topn_flags, rec_model(P, T, d_w, n_w), i_cnt, i_item, i_plain, i_decay, &D,
                     h6, 6));
    // ---- list 1: the user-kNN top-N, as xmap_ctx_uknn_recommend runs it
    UknnLists L;
    XM_TRY(uknn_lists(c, tmp, source, n_query, query_user, n_nb, peer_flags, cap, min_common, &L));
    int32_t *u_cnt, *u_item, *u_support;
    double *u_score;
    XM_TRY(dalloc(tmp, &u_cnt, n, c->st)); XM_TRY(dalloc(tmp, &u_item, mu, c->st));
    XM_TRY(dalloc(tmp, &u_score, mu, c->st)); XM_TRY(dalloc(tmp, &u_support, mu, c->st));
    XM_TRY(xmap_uknn_topn_rows(c->st, n_query, L.query, L.Q.n_users, L.Q.ptr, L.Q.item, L.query_avg, n_nb, L.cnt, L.user, L.sim, c->R.n_users,
                               c->R.n_items, c->pf_ptr, c->pf_item, c->pf_rating, L.user_avg, uknn_flags, n_pool_users, min_support, 0, u_cnt,
                               u_item, u_score, u_support, &D, u6));
    // ---- the fuse
    const xmap_fuse_list lists[2] = {{i_cnt, i_item, rank_by ? i_decay : i_plain, n_pool_items, w_items},
                                     {u_cnt, u_item, u_score, n_pool_users, w_users}};
    int32_t *d_cnt, *d_id, *d_lists;
    double *d_score;
    XM_TRY(dalloc(tmp, &d_cnt, n, c->st)); XM_TRY(dalloc(tmp, &d_id, m, c->st));
    XM_TRY(dalloc(tmp, &d_score, m, c->st)); XM_TRY(dalloc(tmp, &d_lists, m, c->st));
    XM_TRY(xmap_fuse_rows(c->st, n_query, 2, lists, c->R.n_items, how, rrf_c, min_lists, n_top, 0, d_cnt, d_id, d_score, d_lists, f5));
    XM_TRY(d2h(out_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(out_item, (const int32_t *)d_id, m, c->st));
    XM_TRY(d2h(out_score, (const double *)d_score, m, c->st));
    XM_TRY(d2h(out_lists, (const int32_t *)d_lists, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    if (stats) {
        for (int k = 0; k < 6; k++) { stats[k] = h6[k]; stats[6 + k] = u6[k]; }
        for (int k = 0; k < 5; k++) stats[12 + k] = f5[k];
    }
    return XMAP_OK;
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
    ScratchPool tmp;
    int32_t *d_user, *d_item, *d_status, *d_total, *d_cnt, *d_slot, *d_stotal = nullptr;
    int64_t *d_row, *d_spos = nullptr;
    double *d_w, *d_score, *d_share;
    const size_t n = (size_t)n_pairs, m = n * (size_t)n_ev;
    XM_TRY(h2d(tmp, &d_user, pair_user, n, c->st));
    XM_TRY(h2d(tmp, &d_item, pair_item, n, c->st));
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(dalloc(tmp, &d_status, n, c->st)); XM_TRY(dalloc(tmp, &d_total, n, c->st)); XM_TRY(dalloc(tmp, &d_cnt, n, c->st));
    XM_TRY(dalloc(tmp, &d_score, n, c->st));
    XM_TRY(dalloc(tmp, &d_row, m, c->st)); XM_TRY(dalloc(tmp, &d_slot, m, c->st)); XM_TRY(dalloc(tmp, &d_share, m, c->st));
    XM_TRY(explain_rows(c->st, n_pairs, d_user, d_item, rank_by, n_ev, rec_model(P, resident_tables(c), d_w, n_w), d_status, d_total, d_cnt,
                        d_score, d_row, d_slot, d_share, max_now));
    if (n_src > 0) {
        XM_TRY(dalloc(tmp, &d_stotal, m, c->st)); XM_TRY(dalloc(tmp, &d_spos, m * (size_t)n_src, c->st));
        XM_TRY(xmap_explain_sources(c->st, n_pairs, d_user, n_ev, d_cnt, d_row, P.n_users, c->R.n_items, P.ptr, P.item, W.cnt_t, W.off_t,
                                    W.ptr, W.item, c->R.flags, c->g_map, n_src, d_stotal, d_spos));
        XM_TRY(d2h(src_total, (const int32_t *)d_stotal, m, c->st));
        XM_TRY(d2h(src_pos, (const int64_t *)d_spos, m * (size_t)n_src, c->st));
    }
    XM_TRY(d2h(ex_status, (const int32_t *)d_status, n, c->st));
    XM_TRY(d2h(ex_total, (const int32_t *)d_total, n, c->st));
    XM_TRY(d2h(ex_cnt, (const int32_t *)d_cnt, n, c->st));
    XM_TRY(d2h(ex_score, (const double *)d_score, n, c->st));
    XM_TRY(d2h(ex_row, (const int64_t *)d_row, m, c->st));
    XM_TRY(d2h(ex_slot, (const int32_t *)d_slot, m, c->st));
    XM_TRY(d2h(ex_share, (const double *)d_share, m, c->st));
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
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
    ScratchPool tmp;
    int32_t *d_tu, *d_ti, *d_nrel, *d_eval;
    double *d_tr;
    const size_t n = (size_t)n_test;
    XM_TRY(h2d(tmp, &d_tu, test_user, n, c->st));
    XM_TRY(h2d(tmp, &d_ti, test_item, n, c->st));
    XM_TRY(h2d(tmp, &d_tr, test_rating, n, c->st));
    XM_TRY(dalloc(tmp, &d_nrel, U, c->st)); XM_TRY(dalloc(tmp, &d_eval, U, c->st));
    int64_t counts[4] = {0, 0, 0, 0};
    XM_TRY(xmap_eval_users(c->st, n_test, d_tu, d_ti, d_tr, rel_min, c->R.n_users, c->R.n_items, d_nrel, d_eval, counts));
    if (stats) memcpy(stats, counts, sizeof(counts));
    if (user_nrel) XM_TRY(d2h(user_nrel, (const int32_t *)d_nrel, U, c->st));
    const size_t Q = (size_t)counts[0], m = Q * (size_t)n_top;
    if (Q == 0) {
        XM_HIP(hipStreamSynchronize(c->st));
        return XMAP_OK;
    }
    // ---- the lists of the users with relevant pairs: they stay on the device
    int32_t *d_cnt, *d_item;
    double *d_w, *d_dtab, *d_plain, *d_decay, *d_agg;
    uint64_t *d_mask;
    int64_t *d_cover;
    XM_TRY(h2d(tmp, &d_w, wtab, (size_t)n_w, c->st));
    XM_TRY(h2d(tmp, &d_dtab, dtab, (size_t)n_top, c->st));
    XM_TRY(dalloc(tmp, &d_cnt, Q, c->st)); XM_TRY(dalloc(tmp, &d_item, m, c->st));
    XM_TRY(dalloc(tmp, &d_plain, m, c->st)); XM_TRY(dalloc(tmp, &d_decay, m, c->st));
    XM_TRY(dalloc(tmp, &d_mask, Q, c->st)); XM_TRY(dalloc(tmp, &d_agg, (size_t)n_cut * 8, c->st));
    XM_TRY(dalloc(tmp, &d_cover, (size_t)n_cut, c->st));
    XM_TRY(topn_rows(c->st, (int64_t)Q, d_eval, n_top, rank_by, flags, rec_model(resident_profiles(c), resident_tables(c), d_w, n_w), d_cnt,
                     d_item, d_plain, d_decay, nullptr, stats ? stats + 4 : nullptr, 4));
    XM_TRY(xmap_topn_eval(c->st, n_test, d_tu, d_ti, d_tr, rel_min, c->R.n_users, c->R.n_items, d_nrel, (int64_t)Q, d_eval, n_top, d_cnt,
                          d_item, n_cut, cut, d_dtab, d_mask, nullptr, d_agg, d_cover));
    XM_TRY(d2h(agg, (const double *)d_agg, (size_t)n_cut * 8, c->st));
    XM_TRY(d2h(cover, (const int64_t *)d_cover, (size_t)n_cut, c->st));
    if (user_mask) {                // per user, from the per-query masks
        std::vector<uint64_t> h_mask(Q);
        std::vector<int32_t> h_eval(Q);
        XM_TRY(d2h(h_mask.data(), (const uint64_t *)d_mask, Q, c->st));
        XM_TRY(d2h(h_eval.data(), (const int32_t *)d_eval, Q, c->st));
        XM_HIP(hipStreamSynchronize(c->st));
        for (size_t q = 0; q < Q; q++) user_mask[h_eval[q]] = h_mask[q];
    }
    XM_HIP(hipStreamSynchronize(c->st));
    return XMAP_OK;
}
}
