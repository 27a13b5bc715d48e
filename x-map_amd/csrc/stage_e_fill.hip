// stage_e_fill.hip -- the popularity fill (DESIGN.md 4 "Popularity fill"): a ranking of the items by how many resident profiles
// hold them (or by their damped mean rating), and the completion of short top-N lists with the head of that ranking under the
// eligibility rules of the lists -- what a user holds, what the list already contains, what the query excludes, what the mask
// forbids.  The only member of the recommender tail that answers when there is no evidence at all.
//
// The ranking (xmap_pop_index) over the item-major transposition xmap_peer_index leaves (centre == NULL: raw ratings):
//   k_fl_sums  : one wave per item: n_i, and the double-double sum of its holders' ratings (lane-strided, the fixed butterfly of
//                dd_reduce) -- exactly what k_pr_centre has before its division; (hi, lo) are kept for the total
//   k_fl_total : ONE block: thread t adds the (hi, lo) of the items t, t + 1024, ... in ascending order, dd_reduce per wave, lane 0
//                of wave 0 adds the 16 wave sums in order: a fixed shape, the bits of G depend on no grid.  mu = G / T
//   k_fl_keys  : one thread per item: the score (fp64, one rounded operation per step, no fused multiply-add), ranked iff
//                n_i >= min_count and the score is finite; key = the complement of the order-preserving 64-bit image of the score
//                (-0.0 as +0.0), all ones for an unranked item (no finite score maps there); pop_pos = -1
//   radix_sort_pairs : stable over the items in ascending order = the tie rule
//   k_fl_rank  : one thread per position: pop_item / pop_score, and pop_pos through the item
// The fill (xmap_topn_fill_rows), one wave per query, XMAP_FILL_WINDOW rank positions at a time: the skip ids (the list, the user's
// rows, the exclusion list) are looked up once each in pop_pos and those that fall into the window are marked in an LDS bitmap
// (integer OR: order-free); then the wave walks the window 64 positions at a time, one lane per position, a ballot of the clear
// bits hands out the slots in position order.  With a mask the ranking is compacted once per call to its allowed positions
// (flag -> scan -> fill), so a 1 % mask costs one pass over the items, not a hundred windows per query.
// No floating-point atomic, no inline assembly: plain C++ and vector stores.
#include "common.h"
#include "predict_rows.h"
#include "rec_filter.h"

namespace xmap {

constexpr int FL_WORDS = XMAP_FILL_WINDOW / 32;         // LDS words of one wave's window
constexpr int FL_WAVES = 4;
constexpr int FL_TOTAL_THREADS = 1024;
static_assert(XMAP_FILL_WINDOW % (2 * WAVE) == 0, "a lane zeroes whole words, a walk step covers 64 positions");

__global__ __launch_bounds__(256) void k_fl_sums(long long base, long long I, const long long *hd_ptr, const double *hd_x, double *s_hi,
                                                 double *s_lo) {
    const long long i = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    const bool on = i < I;
    const int lane = lane_id();
    long long p0 = 0, p1 = 0;
    if (on) { p0 = hd_ptr[i]; p1 = hd_ptr[i + 1]; }
    double s = 0.0, slo = 0.0;
    for (long long p = p0 + lane; p < p1; p += WAVE) dd_add(s, slo, hd_x[p]);
    dd_reduce<WAVE>(s, slo);
    if (on && lane == 0) { s_hi[i] = s; s_lo[i] = slo; }
}

// tot[0] = G, tot[1] = mu
__global__ __launch_bounds__(FL_TOTAL_THREADS) void k_fl_total(long long I, const long long *hd_ptr, const double *s_hi, const double *s_lo,
                                                               double *tot) {
    __shared__ double w_hi[FL_TOTAL_THREADS / WAVE], w_lo[FL_TOTAL_THREADS / WAVE];
    double s = 0.0, slo = 0.0;
    for (long long i = threadIdx.x; i < I; i += FL_TOTAL_THREADS) {
        dd_add(s, slo, s_hi[i]);
        dd_add(s, slo, s_lo[i]);
    }
    dd_reduce<WAVE>(s, slo);
    if (lane_id() == 0) { w_hi[threadIdx.x >> 6] = s; w_lo[threadIdx.x >> 6] = slo; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double g = 0.0, glo = 0.0;
        for (int w = 0; w < FL_TOTAL_THREADS / WAVE; w++) {
            dd_add(g, glo, w_hi[w]);
            dd_add(g, glo, w_lo[w]);
        }
        const long long T = hd_ptr[I];
        tot[0] = g;
        tot[1] = T > 0 ? g / (double)T : 0.0;
    }
}

// cnt: [0] ranked, [1] below min_count, [2] a non-finite score (of those at or above min_count)
__global__ __launch_bounds__(256) void k_fl_keys(int I, const long long *hd_ptr, const double *s_hi, const double *tot, int how,
                                                 double damping, int min_count, unsigned long long *keys, int *vals, double *score,
                                                 int *pop_pos, unsigned long long *cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I) return;
    const long long n = hd_ptr[i + 1] - hd_ptr[i];
    double sc;
    if (how == XMAP_POP_COUNT) sc = (double)n;
    else {
        const double a = damping * tot[1];
        const double num = s_hi[i] + a;
        const double den = (double)n + damping;
        sc = num / den;
    }
    unsigned long long key = ~0ull;
    if (n < (long long)min_count) atomicAdd(&cnt[1], 1ull);
    else if (!finite_f64(sc)) atomicAdd(&cnt[2], 1ull);
    else {
        atomicAdd(&cnt[0], 1ull);
        unsigned long long u = (unsigned long long)__double_as_longlong(sc + 0.0);      // (-0.0 + 0.0 = +0.0)
        u ^= (u >> 63) ? ~0ull : (1ull << 63);       // ascends with the number
        key = ~u;                                    // descends with it; never all ones for a finite score
    }
    keys[i] = key;
    vals[i] = i;
    score[i] = sc;
    pop_pos[i] = -1;                            // (k_fl_rank gives the ranked items their positions)
}

// position r of the sorted items: the ranked ones stand in front (n_ranked of them)
__global__ __launch_bounds__(256) void k_fl_rank(int I, const unsigned long long *cnt, const int *vals, const double *score, int *pop_item,
                                                 double *pop_score, int *pop_pos) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= I) return;
    const long long n_ranked = (long long)cnt[0];
    if (r < n_ranked) {
        const int i = vals[r];
        pop_item[r] = i;
        pop_score[r] = score[i];
        pop_pos[i] = r;
    } else {
        pop_item[r] = -1;
        pop_score[r] = 0.0;
    }
}

// ---- the mask: the ranking compacted to its allowed positions ---------------------------------------------------------------

__global__ __launch_bounds__(256) void k_fl_flag(int n_ranked, int n_pop, const int *pop_item, const unsigned int *allow, int *flag) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_ranked) return;
    const int i = pop_item[r];
    flag[r] = (i >= 0 && i < n_pop && bit_allowed(allow, i)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_fl_compact_item(int n_ranked, const int *pop_item, const int *flag, const long long *off, int *c_item) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_ranked && flag[r]) c_item[off[r]] = pop_item[r];
}

__global__ __launch_bounds__(256) void k_fl_compact_pos(int n_pop, int n_ranked, const int *pop_pos, const int *flag, const long long *off,
                                                        int *c_pos) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pop) return;
    const int p = pop_pos[i];
    c_pos[i] = (p >= 0 && p < n_ranked && flag[p]) ? (int)off[p] : -1;
}

// ---- the fill ---------------------------------------------------------------------------------------------------------------------

// the position of id in the window [w0, w0 + XMAP_FILL_WINDOW) is marked; an id without a position marks nothing
__device__ __forceinline__ void fl_mark(unsigned int *win, int id, int n_pop, const int *pos, long long w0) {
    if (id < 0 || id >= n_pop) return;
    const long long p = (long long)pos[id] - w0;
    if (p >= 0 && p < XMAP_FILL_WINDOW) atomicOr(&win[p >> 5], 1u << (p & 31));
}

// one wave per query.  st: [0] queries short on entry, [1] of those filled to n_top, [2] fill entries written, [3] still short
__global__ __launch_bounds__(FL_WAVES * WAVE) void k_fl_fill(long long base, long long end, const int *query_user, int n_top, int keep,
                                                             long long n_users, const long long *prof_ptr, const int *prof_item,
                                                             const double *item_avg, int n_ranked, const int *rk_item, const int *rk_pos,
                                                             int n_pop, int *cnt, int *item, double *plain, double *decay, int *out_src,
                                                             const long long *ex_ptr, const int *ex_id, unsigned long long *st) {
    __shared__ unsigned int lds[FL_WAVES][FL_WORDS];
    const long long q = base + (long long)blockIdx.x * FL_WAVES + (threadIdx.x >> 6);
    if (q >= end) return;                       // (wave-uniform)
    const int lane = lane_id();
    unsigned int *win = lds[threadIdx.x >> 6];
    int c0 = cnt[q];
    c0 = c0 < 0 ? 0 : (c0 > n_top ? n_top : c0);
    const size_t o = (size_t)q * n_top;
    if (c0 == n_top) {                          // full on entry: the list keeps every byte
        if (lane < n_top) out_src[o + lane] = 0;
        return;
    }
    const int u = query_user[q];
    long long r0 = 0, r1 = 0, x0 = 0, x1 = 0;
    if (!keep && u >= 0 && u < n_users) { r0 = prof_ptr[u]; r1 = prof_ptr[u + 1]; }
    if (ex_ptr) { x0 = ex_ptr[q]; x1 = ex_ptr[q + 1]; }
    int c = c0;
    for (long long w0 = 0; w0 < n_ranked && c < n_top; w0 += XMAP_FILL_WINDOW) {
        for (int k = lane; k < FL_WORDS; k += WAVE) win[k] = 0u;
        wave_sync<false>();
        // the entries a fill appended stand at positions below w0: only the list as it came can fall into this window
        if (lane < c0) fl_mark(win, item[o + lane], n_pop, rk_pos, w0);
        for (long long p = r0 + lane; p < r1; p += WAVE) fl_mark(win, prof_item[p], n_pop, rk_pos, w0);
        for (long long p = x0 + lane; p < x1; p += WAVE) fl_mark(win, ex_id[p], n_pop, rk_pos, w0);
        wave_sync<false>();
        for (int k = 0; k < XMAP_FILL_WINDOW && c < n_top; k += WAVE) {      // (c is wave-uniform)
            const long long r = w0 + k + lane;
            int i = -1;
            if (r < n_ranked && !((win[(k + lane) >> 5] >> (lane & 31)) & 1u)) i = rk_item[r];
            const bool on = i >= 0 && i < n_pop;
            const unsigned long long m = __ballot(on);
            const int at = c + __popcll(m & lanemask_lt());
            if (on && at < n_top) {
                const double a = item_avg[i];
                item[o + at] = i; plain[o + at] = a; decay[o + at] = a; out_src[o + at] = 1;
            }
            c += __popcll(m);
            if (w0 + k + WAVE >= n_ranked) break;
        }
        c = c > n_top ? n_top : c;
        wave_sync<false>();                     // the walk's reads are done before the next window is zeroed
    }
    if (lane < c0) out_src[o + lane] = 0;
    else if (lane >= c && lane < n_top) out_src[o + lane] = -1;
    if (lane == 0) {
        cnt[q] = c;
        atomicAdd(&st[0], 1ull);
        if (c == n_top) atomicAdd(&st[1], 1ull);
        else atomicAdd(&st[3], 1ull);
        if (c > c0) atomicAdd(&st[2], (unsigned long long)(c - c0));
    }
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_pop_index(void *stream, int32_t n_items, const int64_t *hd_ptr, const double *hd_x, int32_t how, double damping,
                   int32_t min_count, int32_t *pop_item, double *pop_score, int32_t *pop_pos, int64_t *h_counts) {
    // the host checks: before any device work
    XM_ARG(how == XMAP_POP_COUNT || how == XMAP_POP_MEAN);
    XM_ARG(damping >= 0.0 && damping <= 1.7976931348623157e308);      // finite and >= 0 (a NaN fails both)
    XM_ARG(min_count >= 1);
    XM_ARG(n_items >= 0 && (n_items == 0 || (hd_ptr && pop_item && pop_score && pop_pos)));
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    if (h_counts) h_counts[0] = h_counts[1] = h_counts[2] = 0;
    if (n_items == 0) return XMAP_OK;
    const int I = n_items;
    const size_t n = (size_t)I;
    double *s_hi = nullptr, *s_lo = nullptr, *tot = nullptr, *score = nullptr;
    unsigned long long *keys = nullptr, *cnt = nullptr, h[3] = {0, 0, 0};
    int *vals = nullptr;
    XM_HIP(xm_malloc_async((void **)&s_hi, sizeof(double) * n, st));
    XM_HIP(xm_malloc_async((void **)&s_lo, sizeof(double) * n, st));
    XM_HIP(xm_malloc_async((void **)&score, sizeof(double) * n, st));
    XM_HIP(xm_malloc_async((void **)&tot, sizeof(double) * 2, st));
    XM_HIP(xm_malloc_async((void **)&keys, sizeof(unsigned long long) * 2 * n, st));
    XM_HIP(xm_malloc_async((void **)&vals, sizeof(int) * 2 * n, st));
    XM_HIP(xm_malloc_async((void **)&cnt, sizeof(h), st));
    XM_HIP(hipMemsetAsync(cnt, 0, sizeof(h), st));
    int rc = for_pair_ranges(I, 4, [&](long long base, long long, dim3 grid) {
        k_fl_sums<<<grid, dim3(256), 0, st>>>(base, I, (const long long *)hd_ptr, hd_x, s_hi, s_lo);
    });
    if (rc) return rc;
    k_fl_total<<<dim3(1), dim3(FL_TOTAL_THREADS), 0, st>>>(I, (const long long *)hd_ptr, s_hi, s_lo, tot);
    XM_LAUNCH_CHECK();
    const unsigned nb = blocks_for(I, 256);
    k_fl_keys<<<dim3(nb), dim3(256), 0, st>>>(I, (const long long *)hd_ptr, s_hi, tot, how, damping, min_count, keys, vals, score, pop_pos,
                                         cnt);
    XM_LAUNCH_CHECK();
    if ((rc = radix_sort_pairs(st, keys, vals, keys + n, vals + n, I, 64))) return rc;
    k_fl_rank<<<dim3(nb), dim3(256), 0, st>>>(I, cnt, vals, score, pop_item, pop_score, pop_pos);
    XM_LAUNCH_CHECK();
    XM_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_counts) for (int k = 0; k < 3; k++) h_counts[k] = (int64_t)h[k];
    return XMAP_OK;
}

int xmap_topn_fill_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t flags, int64_t n_users,
                        int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item, const double *item_avg, int32_t n_ranked,
                        const int32_t *pop_item, const int32_t *pop_pos, int32_t n_pop_items, int32_t *cnt, int32_t *item, double *plain,
                        double *decay, int32_t *out_src, const xmap_rec_filter *F, int64_t *h_stats) {
    // the host checks: before any device work
    XM_ARG(n_top >= 1 && n_top <= 64);
    XM_ARG((flags & ~XMAP_TOPN_KEEP_HELD) == 0);
    XM_ARG(n_query >= 0 && n_users >= 0 && n_items >= 0);
    XM_ARG(n_pop_items >= 0 && n_pop_items <= n_items && n_ranked >= 0 && n_ranked <= n_pop_items);
    XM_ARG(n_query == 0 || (query_user && cnt && item && plain && decay && out_src));
    XM_ARG(n_ranked == 0 || (pop_item && pop_pos && item_avg));
    XM_ARG(n_query == 0 || n_users == 0 || (flags & XMAP_TOPN_KEEP_HELD) || prof_ptr);
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    // the filter: a NaN floor on the host, then ex_ptr on the device; nothing is indexed through a table that fails and no output
    // (h_stats included) is written.  The floor itself is a floor on predictions: it does not apply to a fill.
    bool filt = false;
    double min_score = 0.0;
    int rc = rf_prepare(st, n_query, F, &filt, &min_score);
    if (rc) return rc;
    if (h_stats) for (int k = 0; k < 4; k++) h_stats[k] = 0;
    if (n_query == 0) return XMAP_OK;
    const unsigned int *allow = filt ? (const unsigned int *)F->allow : nullptr;
    const long long *ex_ptr = filt ? (const long long *)F->ex_ptr : nullptr;
    const int *ex_id = filt ? F->ex_id : nullptr;
    const int *rk_item = pop_item, *rk_pos = pop_pos;
    int n_rk = n_ranked;
    if (allow && n_ranked > 0) {                // the ranking's allowed positions, compacted once per call
        int *flag = nullptr, *c_item = nullptr, *c_pos = nullptr;
        long long *off = nullptr;
        XM_HIP(xm_malloc_async((void **)&flag, sizeof(int) * (size_t)n_ranked, st));
        XM_HIP(xm_malloc_async((void **)&off, sizeof(long long) * ((size_t)n_ranked + 1), st));
        XM_HIP(xm_malloc_async((void **)&c_item, sizeof(int) * (size_t)n_ranked, st));
        XM_HIP(xm_malloc_async((void **)&c_pos, sizeof(int) * (size_t)n_pop_items, st));
        k_fl_flag<<<dim3(blocks_for(n_ranked, 256)), dim3(256), 0, st>>>(n_ranked, n_pop_items, pop_item, allow, flag);
        XM_LAUNCH_CHECK();
        int64_t total = 0;
        if ((rc = xmap_exclusive_scan_i32_to_i64(st, flag, (int64_t *)off, n_ranked, &total))) return rc;
        k_fl_compact_item<<<dim3(blocks_for(n_ranked, 256)), dim3(256), 0, st>>>(n_ranked, pop_item, flag, off, c_item);
        XM_LAUNCH_CHECK();
        k_fl_compact_pos<<<dim3(blocks_for(n_pop_items, 256)), dim3(256), 0, st>>>(n_pop_items, n_ranked, pop_pos, flag, off, c_pos);
        XM_LAUNCH_CHECK();
        rk_item = c_item; rk_pos = c_pos; n_rk = (int)total;
    }
    unsigned long long *d_st = nullptr, h[4] = {0, 0, 0, 0};
    XM_HIP(xm_malloc_async((void **)&d_st, sizeof(h), st));
    XM_HIP(hipMemsetAsync(d_st, 0, sizeof(h), st));
    const int keep = (flags & XMAP_TOPN_KEEP_HELD) ? 1 : 0;
    rc = for_pair_ranges(n_query, FL_WAVES, [&](long long base, long long end, dim3 grid) {
        k_fl_fill<<<grid, dim3(FL_WAVES * WAVE), 0, st>>>(base, end, query_user, n_top, keep, n_users, (const long long *)prof_ptr, prof_item,
                                                          item_avg, n_rk, rk_item, rk_pos, n_pop_items, cnt, item, plain, decay, out_src,
                                                          ex_ptr, ex_id, d_st);
    });
    if (rc) return rc;
    XM_HIP(hipMemcpyAsync(h, d_st, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_stats) for (int k = 0; k < 4; k++) h_stats[k] = (int64_t)h[k];
    return XMAP_OK;
}
}
