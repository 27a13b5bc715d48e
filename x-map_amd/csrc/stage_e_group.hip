// stage_e_group.hip -- group lists on the device: ONE top-N list for several users, by aggregating the members' unrounded
// predictions (mean, least misery, most pleasure; a veto) -- xmap_group_topn_rows (include/xmap_hip.h carries the statement in
// full; DESIGN.md 4 "Group lists").  Groups are a CSR over the flattened member list grp_user.
//
//   k_gr_check      : grp_ptr[0] == 0, non-decreasing, every size <= XMAP_GROUP_MAX_MEMBERS; on the device, before any other
//                     work; nothing is read through a table that fails.
//   member pass     : tn_score_candidates (topn_pass.h; the candidate-and-scoring half of xmap_topn_rows) with the flattened
//                     members as the queries: per member a segment of (item ascending, plain, decayed, status), pairs with evidence
//                     only -- a member without evidence for an item predicts the item average (predict_pair, n == 0), which costs
//                     no wave.  The mask acts here: a masked item is never scored.  The exclusion lists belong to groups, not to
//                     members, so an excluded item may be scored; exclusion lists are short.  The pass takes the call's flags: an
//                     item a member holds leaves the group's candidates without XMAP_TOPN_KEEP_HELD whoever else has evidence
//                     for it, so that member's pair is never needed -- and a group of one scores exactly what xmap_topn_rows scores.
//   k_gr_candidates : one block per group (grid-stride), run twice (count, then fill into a buffer of exactly the counted size).
//                     The windowed LDS bitmap of k_tn_candidates (IdBitmap, id_bitmap.h; the geometry of topn_pass.h): the union
//                     of the members' segments is marked, every member's held items are cleared unless KEEP_HELD, the group's
//                     exclusion ids are cleared (a bit that was still set is counted, once), and the marked items leave in
//                     ascending index through the shared emit, which applies the mask without counting what it removes.
//   k_gr_select     : one wave per group, four per block.  The group's candidates stream through 64 at a time; a lane owns one
//                     candidate and walks the members in list order: the item is found in the member's segment by bisection
//                     (one entry or none: a segment holds an item once) and gives that entry's scores and status, or the item
//                     average.  Status 2, then the veto, then the floor; the aggregate and the least-happy member; insertion by
//                     the ballot count and one-lane shift of k_tn_select with (aggregate plain, aggregate decayed, item, low).
// Every output position follows from the scans, so the result does not depend on the grid or on the order of the atomics.
#include "common.h"
#include "rec_filter.h"
#include "topn_pass.h"
#include "two_pass.h"

namespace xmap {

constexpr int GR_WINDOW = 1 << TN_WINDOW_LOG2;  // items per bitmap pass: the window of k_tn_candidates
constexpr int GR_MAX_MEMBERS = XMAP_GROUP_MAX_MEMBERS;
static_assert(GR_MAX_MEMBERS == 64, "a lane of the selection wave holds one member's segment");

// grp_ptr[0 .. n_groups]: bad[0] += positions k with ptr[k] < ptr[k - 1] (k = 0: ptr[0] != 0), bad[1] += groups of more than
// GR_MAX_MEMBERS members, bad[2] = ptr[n_groups].  Bounded by n_groups alone.
static __global__ __launch_bounds__(256) void k_gr_check(long long n_groups, const long long *grp_ptr, unsigned long long *bad) {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k <= n_groups; k += step) {
        const bool b = k == 0 ? grp_ptr[0] != 0 : grp_ptr[k] < grp_ptr[k - 1];
        if (b) atomicAdd(&bad[0], 1ull);        // (bad input only: no need to spare the atomics)
        if (k > 0 && grp_ptr[k] - grp_ptr[k - 1] > GR_MAX_MEMBERS) atomicAdd(&bad[1], 1ull);
        if (k == n_groups) bad[2] = (unsigned long long)grp_ptr[k];
    }
}

// mem_ptr / mem_item: the members' candidate segments (member pass), indexed by the position in grp_user.  The mask is always
// applied (allow may be NULL), ex_ptr is tested at run time, and *excluded counts the bits the exclusion lists cleared -- not
// what the mask removed, which the member pass has counted.
template <bool FILL>
__global__ __launch_bounds__(TN_THREADS) void k_gr_candidates(long long n_groups, const long long *grp_ptr, const int *grp_user, long long U, int I,
                                                              int keep_held, const long long *mem_ptr, const int *mem_item,
                                                              const long long *pptr, const int *pitem, int *gc_cnt, const long long *gc_ptr,
                                                              int *gc_item, const unsigned int *allow, const long long *ex_ptr,
                                                              const int *ex_id, unsigned long long *excluded) {
    extern __shared__ unsigned int gr_lds[];
    TnBitmap bm(gr_lds);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (long long g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const long long a = grp_ptr[g], b = grp_ptr[g + 1];
        long long total = 0;
        const long long out0 = FILL ? gc_ptr[g] : 0;
        for (long long lo = 0; lo < I && b > a; lo += GR_WINDOW) {
            // mark: one wave per member walks the member's segment
            for (long long p = a + wv; p < b; p += TN_THREADS / 64) {
                const long long r1 = mem_ptr[p + 1];
                for (long long r = mem_ptr[p] + lane; r < r1; r += 64) bm.mark((long long)mem_item[r] - lo);
            }
            __syncthreads();
            if (!keep_held) {                   // an item any member holds is no candidate
                for (long long p = a + wv; p < b; p += TN_THREADS / 64) {
                    const int u = grp_user[p];
                    if (u < 0 || u >= U) continue;
                    const long long r1 = pptr[u + 1];
                    for (long long r = pptr[u] + lane; r < r1; r += 64) bm.unmark((long long)pitem[r] - lo);
                }
                __syncthreads();
            }
            bm.template exclude<!FILL>(ex_ptr, ex_id, g, I, lo);
            total += bm.template emit<FILL, true, false>(lo, allow, out0 + total, [&](long long o, long long item) { gc_item[o] = (int)item; });
        }
        if constexpr (!FILL) {
            if (tid == 0) gc_cnt[g] = (int)total;
        }
    }
    if constexpr (!FILL) bm.add_gone(excluded);
}

// lane j < have holds the j-th best candidate so far; keys are distinct (the candidate list holds an item once).
// HOW: XMAP_GROUP_MEAN / _MIN / _MAX.  veto = -inf and min_score = -inf compare false against every number: no veto, no floor.
template <int HOW>
__global__ __launch_bounds__(256) void k_gr_select(long long n_groups, int n_top, int rank_by, const long long *grp_ptr, const long long *mem_ptr,
                                                   const int *mem_item, const double *mem_plain, const double *mem_decay,
                                                   const int *mem_status, const long long *gc_ptr, const int *gc_item, const double *avg,
                                                   double veto, double min_score, int *out_cnt, int *out_item, double *out_plain,
                                                   double *out_decay, int *out_low,
                                                   unsigned long long *stats /*[0] dropped (status 2), [1] largest candidate count,
                                                                               [2] below the floor, [4] vetoed*/) {
    const int lane = lane_id();
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const long long ma = grp_ptr[g];
    const int m = (int)(grp_ptr[g + 1] - ma);   // <= 64 (k_gr_check)
    long long seg_a = 0, seg_b = 0;             // lane j < m: the segment of member j
    if (lane < m) { seg_a = mem_ptr[ma + lane]; seg_b = mem_ptr[ma + lane + 1]; }
    const long long a = gc_ptr[g], b = gc_ptr[g + 1];
    double ks = 0.0, kp = 0.0, kd = 0.0;
    int ki = -1, kl = -1, have = 0, dropped = 0, vetoed = 0, floored = 0;
    for (long long p = a; p < b; p += 64) {
        const bool in = p + lane < b;
        const int xi = in ? gc_item[p + lane] : 0;
        const double base = in ? avg[xi] : 0.0;
        bool bad = false, veto_hit = false;
        double xp = 0.0, xd = 0.0, lows = 0.0;
        int xl = 0;
        for (int j = 0; j < m; j++) {           // the members in list order
            const long long s0 = rl64(seg_a, j), s1 = rl64(seg_b, j);
            long long lo = s0, hi = s1;
            while (lo < hi) {                   // the first entry with an item >= xi
                const long long mid = lo + ((hi - lo) >> 1);
                if (mem_item[mid] < xi) lo = mid + 1;
                else hi = mid;
            }
            double sp = base, sd = base;
            if (in && lo < s1 && mem_item[lo] == xi) {
                sp = mem_plain[lo]; sd = mem_decay[lo];
                bad |= mem_status[lo] != 0;
            } else
                bad |= !isfinite(base);         // a member without evidence predicts the item average
            const double rs = rank_by ? sd : sp;
            veto_hit |= rs < veto;
            if (j == 0) { xp = sp; xd = sd; lows = rs; }
            else {
                if constexpr (HOW == XMAP_GROUP_MEAN) { xp += sp; xd += sd; }
                else if constexpr (HOW == XMAP_GROUP_MIN) { xp = sp < xp ? sp : xp; xd = sd < xd ? sd : xd; }
                else { xp = sp > xp ? sp : xp; xd = sd > xd ? sd : xd; }
                if (rs < lows) { lows = rs; xl = j; }
            }
        }
        if constexpr (HOW == XMAP_GROUP_MEAN) { xp = xp / (double)m; xd = xd / (double)m; }
        const double xs = rank_by ? xd : xp;
        const bool scored = in && !bad;                         // order of the drops: status 2, the veto, the floor
        dropped += __popcll(__ballot(in && bad));
        const bool liked = scored && !veto_hit;
        vetoed += __popcll(__ballot(scored && veto_hit));
        const bool ok = liked && !(xs < min_score);
        floored += __popcll(__ballot(liked && !ok));
        const double ws = rld(ks, n_top - 1);
        const int wi = rl32(ki, n_top - 1);
        unsigned long long mask = __ballot(ok && (have < n_top || xs > ws || (xs == ws && xi < wi)));
        while (mask) {
            const int j = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const double es = rld(xs, j), ep = rld(xp, j), ed = rld(xd, j);
            const int ei = rl32(xi, j), el = rl32(xl, j);
            const int pos = __popcll(__ballot(lane < have && (ks > es || (ks == es && ki < ei))));
            if (pos >= n_top) continue;
            const double us = __shfl_up(ks, 1, 64), up = __shfl_up(kp, 1, 64), ud = __shfl_up(kd, 1, 64);
            const int ui = __shfl_up(ki, 1, 64), ul = __shfl_up(kl, 1, 64);
            if (lane > pos) { ks = us; kp = up; kd = ud; ki = ui; kl = ul; }
            else if (lane == pos) { ks = es; kp = ep; kd = ed; ki = ei; kl = el; }
            have = have < n_top ? have + 1 : n_top;
        }
    }
    if (lane < n_top) {
        const size_t o = (size_t)g * n_top + lane;
        const bool v = lane < have;
        out_item[o] = v ? ki : -1;
        out_plain[o] = v ? kp : 0.0;
        out_decay[o] = v ? kd : 0.0;
        out_low[o] = v ? kl : -1;
    }
    if (lane == 0) {
        out_cnt[g] = have;
        if (dropped) atomicAdd(&stats[0], (unsigned long long)dropped);
        if (floored) atomicAdd(&stats[2], (unsigned long long)floored);
        if (vetoed) atomicAdd(&stats[4], (unsigned long long)vetoed);
        atomicMax(&stats[1], (unsigned long long)(b - a));
    }
}

// rec_model.h: the body of xmap_group_topn_rows
int group_topn_rows(void *stream, int64_t n_groups, const int64_t *grp_ptr, const int32_t *grp_user, int32_t n_top, int32_t rank_by,
                    int32_t flags, int32_t how, double veto, const RecModel &M, int32_t *out_cnt, int32_t *out_item, double *out_plain,
                    double *out_decay, int32_t *out_low, const xmap_rec_filter *F, int64_t *h_stats) {
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    XM_ARG(how == XMAP_GROUP_MEAN || how == XMAP_GROUP_MIN || how == XMAP_GROUP_MAX);
    XM_ARG(veto == veto);                       // NaN
    XM_ARG(n_top >= 1 && n_top <= TN_MAX_TOP);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG((flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    int rc = rec_model_check(M);
    if (rc) return rc;
    XM_ARG(n_groups >= 0 && (n_groups == 0 || (grp_ptr && out_cnt && out_item && out_plain && out_decay && out_low)));
    if (h_stats) for (int k = 0; k < 8; k++) h_stats[k] = 0;
    if (n_groups == 0) {
        bool f0 = false;
        double m0 = 0.0;
        return rf_prepare(st, 0, F, &f0, &m0);  // (the floor is still checked)
    }
    // ---- the groups, before any other work
    unsigned long long *bad = nullptr, h_bad[3] = {0, 0, 0};
    XM_HIP(xm_malloc_async((void **)&bad, sizeof(h_bad), st));
    XM_HIP(hipMemsetAsync(bad, 0, sizeof(h_bad), st));
    {
        const long long total = n_groups + 1;
        const unsigned blocks = (unsigned)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
        k_gr_check<<<dim3(blocks), dim3(256), 0, st>>>(n_groups, (const long long *)grp_ptr, bad);
        XM_LAUNCH_CHECK();
    }
    XM_HIP(hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_bad[0]) {
        set_error("xmap_group_topn_rows: grp_ptr has %llu bad entries (grp_ptr[0] = 0, non-decreasing)", h_bad[0]);
        return XMAP_ERR_ARG;
    }
    if (h_bad[1]) {
        set_error("xmap_group_topn_rows: %llu groups of more than %d members", h_bad[1], GR_MAX_MEMBERS);
        return XMAP_ERR_ARG;
    }
    const int64_t n_mem = (int64_t)h_bad[2];
    if (n_mem > 0 && !grp_user) {
        set_error("xmap_group_topn_rows: grp_ptr lists %lld members, grp_user is NULL", (long long)n_mem);
        return XMAP_ERR_ARG;
    }
    bool filt = false;
    double min_score = 0.0;
    rc = rf_prepare(st, n_groups, F, &filt, &min_score);
    if (rc) return rc;
    const unsigned int *allow = F ? (const unsigned int *)F->allow : nullptr;
    const long long *ex_ptr = F ? (const long long *)F->ex_ptr : nullptr;
    const int *ex_id = F ? F->ex_id : nullptr;
    // [0] dropped (status 2), [1] largest candidate count, [2] below the floor, [3] removed by the exclusion lists, [4] vetoed,
    // [5] what the mask removed from the members' candidates (not reported)
    unsigned long long *stats = nullptr;
    XM_HIP(xm_malloc_async((void **)&stats, sizeof(unsigned long long) * 6, st));
    XM_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long) * 6, st));
    // ---- member pass: the flattened members as the queries of a top-N call; the mask, not the exclusions
    TnScored S;
    if (n_mem > 0 && (rc = tn_score_candidates(st, n_mem, grp_user, flags, M, allow != nullptr, allow, nullptr, nullptr, stats + 5, &S))) return rc;
    // ---- the groups' candidates: count, scan, fill
    int *gc_item = nullptr;
    long long *gc_ptr = nullptr;
    int64_t n_gc = 0;
    const unsigned cblocks = (unsigned)(n_groups < TN_MAX_BLOCKS ? n_groups : TN_MAX_BLOCKS);
    rc = count_scan_fill<false>(
        st, n_groups, &gc_ptr, &n_gc,
        [&](bool fill, int *gc_cnt, const long long *ptr) {
            return launch_dyn_lds(fill ? k_gr_candidates<true> : k_gr_candidates<false>, cblocks, TN_THREADS, TnBitmap::LDS_BYTES, st, n_groups,
                                  (const long long *)grp_ptr, grp_user, M.n_users, M.n_items, flags & XMAP_TOPN_KEEP_HELD, S.cand_ptr,
                                  S.cand_item, (const long long *)M.prof_ptr, M.prof_item, gc_cnt, ptr, gc_item, allow, ex_ptr, ex_id, stats + 3);
        },
        [&](int64_t n) -> int {
            if (n > 0) XM_HIP(xm_malloc_async((void **)&gc_item, sizeof(int) * (size_t)n, st));
            return XMAP_OK;
        });
    if (rc) return rc;
    // ---- aggregate and select (n_gc == 0: every list is empty, the counts and the padding are still written)
    auto sel = how == XMAP_GROUP_MEAN ? k_gr_select<XMAP_GROUP_MEAN> : how == XMAP_GROUP_MIN ? k_gr_select<XMAP_GROUP_MIN> : k_gr_select<XMAP_GROUP_MAX>;
    sel<<<dim3((unsigned)((n_groups + 3) / 4)), dim3(256), 0, st>>>(
        (long long)n_groups, n_top, rank_by, (const long long *)grp_ptr, (const long long *)S.cand_ptr, (const int *)S.cand_item,
        (const double *)S.plain, (const double *)S.decay, (const int *)S.status, (const long long *)gc_ptr, (const int *)gc_item, M.item_avg, veto,
        min_score, out_cnt, out_item, out_plain, out_decay, out_low, stats);
    XM_LAUNCH_CHECK();
    unsigned long long h[6] = {0, 0, 0, 0, 0, 0};
    XM_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = S.n_pairs; h_stats[1] = (int64_t)h[0]; h_stats[2] = S.max_now; h_stats[3] = (int64_t)h[1];
        h_stats[4] = (int64_t)h[2]; h_stats[5] = (int64_t)h[3]; h_stats[6] = (int64_t)h[4]; h_stats[7] = n_gc;
    }
    return XMAP_OK;
}

}  // namespace xmap
using namespace xmap;

extern "C" {

int xmap_group_topn_rows(void *stream, int64_t n_groups, const int64_t *grp_ptr, const int32_t *grp_user, int32_t n_top, int32_t rank_by,
                         int32_t flags, int32_t how, double veto, int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt,
                         const int32_t *nb_col, const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item,
                         const double *prof_rating, const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w,
                         int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_low,
                         const xmap_rec_filter *F, int64_t *h_stats) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    return group_topn_rows(stream, n_groups, grp_ptr, grp_user, n_top, rank_by, flags, how, veto, M, out_cnt, out_item, out_plain, out_decay,
                           out_low, F, h_stats);
}
}
