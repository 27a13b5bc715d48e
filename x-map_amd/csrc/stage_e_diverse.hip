// stage_e_diverse.hip -- diversified top-N on the device: a greedy maximal-marginal-relevance re-ranking of a top-M pool into a
// top-N list by item similarity, with the intra-list similarity of every returned list out of the same pass (DESIGN.md 4
// "Diversified lists").  What it reads is what xmap_topn_rows writes (the pool) and the RecommenderSim CSR the tail leaves resident.
//
//   xmap_div_index  : the diversity index of a RecommenderSim CSR -- every row's entries by column ascending, |sim| beside them:
//     k_dv_keys     : one thread per entry: its row by bisection of row_ptr -> key = row << bits(I) | col, value = entry index;
//                     a column outside [0, I) would not fit its field: counted, XMAP_ERR_ARG
//     radix_sort_pairs (plan.hip) over the bits(I) + bits(I) key bits
//     k_dv_gather   : dv_col / dv_abs through the sorted entry indices; adjacent equal keys (a row holding a column twice) are
//                     counted (integer atomics: the count does not depend on their order)
//   k_dv_rerank     : one wave per query, four per block; lane j is pool position j and keeps score, penalty and similarity sum
//                     of its item in registers.  Per pick: obj = score - w * pen (two operations), a butterfly arg-max over (obj
//                     descending, lane ascending), then every live lane bisects the pick's sorted row -- a wave-uniform range --
//                     for its own item with a wave-uniform trip count: 64 lanes descend the same row, so the first levels read the
//                     same lines and only the last ones spread (~5 cycles per distinct 128-byte line per
//                     vector-memory instruction).  No search after the last pick, no LDS.
// Every output follows from the registers of one wave and the sorted rows, so the result does not depend on the grid or on the
// order of the atomics (which only add integers).
#include <math.h>

#include "common.h"

namespace xmap {

constexpr int DV_MAX_POOL = 64;

__global__ __launch_bounds__(256) void k_dv_keys(int I, long long nnz, int col_bits, const long long *row_ptr, const int *col,
                                                 unsigned long long *keys, int *vals, unsigned long long *bad) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    int lo = 0, n = I;                      // the last row r of [0, I) with row_ptr[r] <= e (empty rows in front of it are skipped)
    while (n > 1) {
        const int half = n >> 1;
        if (row_ptr[lo + half] <= e) lo += half;
        n -= half;
    }
    const int c = col[e];
    const bool ok = c >= 0 && c < I;
    keys[e] = ((unsigned long long)lo << col_bits) | (unsigned long long)(ok ? c : 0);
    vals[e] = (int)e;
    if (!ok) atomicAdd(bad, 1ull);
}

__global__ __launch_bounds__(256) void k_dv_gather(long long nnz, int col_bits, const unsigned long long *keys, const int *vals,
                                                   const double *sim, int *dv_col, double *dv_abs, unsigned long long *dups) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = k < nnz;
    bool dup = false;
    if (in) {
        const unsigned long long key = keys[k];
        dv_col[k] = (int)(key & ((1ull << col_bits) - 1ull));
        dv_abs[k] = fabs(sim[vals[k]]);
        dup = k > 0 && keys[k - 1] == key;
    }
    const int n = __popcll(__ballot(dup));
    if (n && lane_id() == 0) atomicAdd(dups, (unsigned long long)n);
}

// a beats b: a live position (l < 64) over none, then the larger obj as numbers, then the smaller position
__device__ __forceinline__ bool dv_beats(double ao, int al, double bo, int bl) {
    return al < 64 && (bl >= 64 || ao > bo || (ao == bo && al < bl));
}

__global__ __launch_bounds__(256) void k_dv_rerank(long long n_query, int n_pool, const int *in_cnt, const int *in_item,
                                                   const double *in_plain, const double *in_decay, int rank_by, double w, int n_top,
                                                   int I, const long long *row_ptr, const int *dv_col, const double *dv_abs,
                                                   int *out_cnt, int *out_item, double *out_plain, double *out_decay, int *out_pos,
                                                   double *out_pen, double *out_ils, unsigned long long *stats) {
    const int lane = lane_id();
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_query) return;
    int cnt = uniform(in_cnt[q]);
    cnt = cnt < 0 ? 0 : (cnt > n_pool ? n_pool : cnt);
    bool live = lane < cnt;
    const size_t at = (size_t)q * n_pool + lane;
    const int item = live ? in_item[at] : -1;
    const double plain = live ? in_plain[at] : 0.0, decay = live ? in_decay[at] : 0.0;
    const double score = rank_by ? decay : plain;
    double pen = 0.0, sum = 0.0, pairsum = 0.0;
    const int n = cnt < n_top ? cnt : n_top;
    int oi = -1, opos = -1, moved = 0;      // lane r keeps output r
    double op = 0.0, od = 0.0, open = 0.0;
    for (int r = 0; r < n; r++) {
        const double t = w * pen;           // (-ffp-contract=off: a multiply, then a subtract)
        double bo = score - t;
        int bl = live ? lane : 64;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double xo = __shfl_xor(bo, m, 64);
            const int xl = __shfl_xor(bl, m, 64);
            if (dv_beats(xo, xl, bo, bl)) { bo = xo; bl = xl; }
        }
        const int js = uniform(bl);         // live holds n - r >= 1 positions: js < 64
        const int pi = rl32(item, js);
        const double pp = rld(plain, js), pd = rld(decay, js), ppen = rld(pen, js);
        pairsum = pairsum + rld(sum, js);
        if (lane == r) { oi = pi; op = pp; od = pd; opos = js; open = ppen; }
        moved |= js != r;
        if (lane == js) live = false;
        if (r + 1 < n && pi >= 0 && pi < I) {
            const long long a = row_ptr[pi], b = row_ptr[pi + 1];      // wave-uniform
            if (live && b > a) {
                long long lo = a, len = b - a;
                while (len > 1) {           // the last entry <= item, if the row has one: the same trip count in every lane
                    const long long half = len >> 1;
                    if (dv_col[lo + half] <= item) lo += half;
                    len -= half;
                }
                if (dv_col[lo] == item) {
                    const double v = dv_abs[lo];
                    if (v > pen) pen = v;   // a NaN never raises a penalty
                    sum = sum + v;
                }
            }
        }
    }
    if (lane < n_top) {
        const size_t o = (size_t)q * n_top + lane;
        out_item[o] = oi; out_plain[o] = op; out_decay[o] = od; out_pos[o] = opos; out_pen[o] = open;
    }
    if (lane == 0) {
        out_cnt[q] = n;
        out_ils[q] = n >= 2 ? pairsum / (double)(n * (n - 1) / 2) : 0.0;
        if (stats) {
            if (moved) atomicAdd(&stats[0], 1ull);
            if (n) atomicAdd(&stats[1], (unsigned long long)n);
        }
    }
}

}  // namespace xmap
using namespace xmap;

extern "C" {

int xmap_div_index(void *stream, int32_t n_items, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const double *sim,
                   int32_t *dv_col, double *dv_abs, int64_t *h_dups) {
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    XM_ARG(n_items >= 0 && nnz >= 0 && nnz < (1ll << 31));      // the sort carries entry indices as int
    XM_ARG(nnz == 0 || (n_items > 0 && row_ptr && col && sim && dv_col && dv_abs));
    if (h_dups) *h_dups = 0;
    if (nnz == 0) return XMAP_OK;
    const int col_bits = bits_for(n_items), row_bits = bits_for(n_items);
    const size_t n = (size_t)nnz;
    unsigned long long *keys = nullptr, *cnt = nullptr;
    int *vals = nullptr;
    XM_HIP(xm_malloc_async((void **)&keys, sizeof(unsigned long long) * 2 * n, st));
    XM_HIP(xm_malloc_async((void **)&vals, sizeof(int) * 2 * n, st));
    XM_HIP(xm_malloc_async((void **)&cnt, sizeof(unsigned long long) * 2, st));     // [0] repeated (row, column), [1] columns outside [0, I)
    XM_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * 2, st));
    const dim3 grid((unsigned)((nnz + 255) / 256)), block(256);
    k_dv_keys<<<grid, block, 0, st>>>(n_items, nnz, col_bits, (const long long *)row_ptr, col, keys, vals, cnt + 1);
    XM_LAUNCH_CHECK();
    int rc = radix_sort_pairs(st, keys, vals, keys + n, vals + n, nnz, col_bits + row_bits);
    if (rc) return rc;
    k_dv_gather<<<grid, block, 0, st>>>(nnz, col_bits, keys, vals, sim, dv_col, dv_abs, cnt);
    XM_LAUNCH_CHECK();
    unsigned long long h[2] = {0, 0};
    XM_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_dups) *h_dups = (int64_t)h[0];
    if (h[1]) { set_error("xmap_div_index: %llu columns outside [0, %d)", h[1], (int)n_items); return XMAP_ERR_ARG; }
    if (h[0]) { set_error("xmap_div_index: %llu repeated (row, column) entries", h[0]); return XMAP_ERR_ARG; }
    return XMAP_OK;
}

int xmap_diversify_rows(void *stream, int64_t n_query, int32_t n_pool, const int32_t *in_cnt, const int32_t *in_item,
                        const double *in_plain, const double *in_decay, int32_t rank_by, double weight, int32_t n_top,
                        int32_t n_items, const int64_t *row_ptr, const int32_t *dv_col, const double *dv_abs,
                        int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos,
                        double *out_pen, double *out_ils, int64_t *h_stats) {
    XM_ARG(weight >= 0.0 && weight <= 1.7976931348623157e308);      // finite and >= 0 (a NaN fails both)
    XM_ARG(n_pool >= 1 && n_pool <= DV_MAX_POOL);
    XM_ARG(n_top >= 1 && n_top <= n_pool);
    XM_ARG(rank_by == 0 || rank_by == 1);
    XM_ARG(n_query >= 0 && n_items >= 0);
    XM_ARG(n_query == 0 || (in_cnt && in_item && in_plain && in_decay && out_cnt && out_item && out_plain && out_decay && out_pos &&
                            out_pen && out_ils));
    XM_ARG(n_items == 0 || row_ptr);
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    if (h_stats) h_stats[0] = h_stats[1] = 0;
    if (n_query == 0) return XMAP_OK;
    unsigned long long *stats = nullptr;
    if (h_stats) {
        XM_HIP(xm_malloc_async((void **)&stats, sizeof(unsigned long long) * 2, st));
        XM_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long) * 2, st));
    }
    k_dv_rerank<<<dim3((unsigned)((n_query + 3) / 4)), dim3(256), 0, st>>>(
        n_query, n_pool, in_cnt, in_item, in_plain, in_decay, rank_by, weight, n_top, n_items, (const long long *)row_ptr, dv_col, dv_abs,
        out_cnt, out_item, out_plain, out_decay, out_pos, out_pen, out_ils, stats);
    XM_LAUNCH_CHECK();
    if (h_stats) {
        unsigned long long h[2] = {0, 0};
        XM_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
        h_stats[0] = (int64_t)h[0]; h_stats[1] = (int64_t)h[1];
    }
    return XMAP_OK;
}
}
