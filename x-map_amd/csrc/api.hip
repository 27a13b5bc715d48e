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
//
// The coarse ABI by file:
//   ctx.h          the context (struct xmap_ctx, its pools, what drops what), the transfers of one call (CoarseCall), the
//                  sources of a tail call (check_source / resolve_source), the filter and the filtered top-N on the device
//   api.hip        this file: create / destroy, upload and its check, the stages (item_sim, extend, candidates, generate) with
//                  their downloads, and rec_sim, which is stage A's pass (tri_pass) over the AlterEgo profiles
//   api_tail.hip   the tail over its three sources: rec_select / rec_set_neighbors, predict / recommend / audience and the
//                  filtered entries, fold-in and item fold-in, explain, union, evaluate_topn
//   api_lists.hip  what re-ranks or combines lists: group, diverse, peers, uknn, related, popular / filled, set_labels,
//                  shelves, quota, allot, fuse, hybrid
#include <math.h>
#include <stdlib.h>
#include <vector>

#include "ctx.h"

namespace xmap {

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
    CoarseCall io(c);
    int64_t *d_off;
    int32_t *d_end;
    double *d_val;
    XM_TRY(io.out(&d_off, xs_off, (size_t)I, true));
    XM_TRY(io.scratch(&d_end, (size_t)cap)); XM_TRY(io.scratch(&d_val, (size_t)cap));
    XM_TRY(run_enumeration(c, cap, d_off, d_end, d_val));
    io.back(xs_end, d_end, (size_t)c->n_out); io.back(xs_val, d_val, (size_t)c->n_out);       // (n_out, as the pass has just counted it)
    return io.finish();
}

int xmap_ctx_candidates(xmap_ctx *c, int32_t *n_top) {
    XM_ARG(c && c->have_ext && n_top);
    XM_HIP(hipSetDevice(c->device));
    const int I = c->R.n_items;
    if (I == 0) return XMAP_OK;
    CoarseCall io(c);
    int32_t *d_top, *d_choice, *d_map;
    XM_TRY(io.out(&d_top, n_top, (size_t)I, true));
    XM_TRY(io.scratch(&d_choice, (size_t)I, true)); XM_TRY(io.scratch(&d_map, (size_t)I, true));
    XM_TRY(xmap_select_map(c->st, I, 0, c->n_cand, c->top_end, nullptr, d_top, d_choice, d_map));
    return io.finish();
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
}
