// stage_e_eval.hip -- hold-out evaluation of the top-N lists on the device (DESIGN.md 4 "Top-N evaluation"): what xmap_mae is to
// xmap_predict_rows.  The lists xmap_topn_rows left in HBM and the held-out (user, item, rating) pairs are read where they are;
// hit rate, precision, recall, NDCG, MAP, MRR and catalogue coverage at up to 8 cutoffs come back as a few numbers.
//
//   k_ev_count      : one thread per pair classifies it (ignored / relevant / below rel_min) and counts the relevant pairs of its
//                     user in n_rel.  Global integer atomics: the users of a batch of pairs are spread over the whole table, an
//                     LDS cache of it would hold nothing twice.  The one case that piles onto an address -- a wave whose relevant
//                     pairs all belong to one user (pairs usually arrive user by user) -- is one atomic of the lane count.  The
//                     three counters are summed per block first.
//   k_ev_flag / k_ev_compact : n_rel > 0 -> xmap_exclusive_scan -> eval_user, ascending.
//   k_te_map / k_te_verify   : user -> query table (atomicMax of the query index, then every query checks it is the one listed:
//                     a user listed twice is found here).
//   k_te_mark       : one thread per relevant pair compares its item with the list of its user's query and ORs the positions
//                     into the query's 64-bit mask.  The OR is idempotent: the mask is a pure function of the inputs.
//   k_te_idcg       : prefix sums of the discount table, left to right (the ideal DCG of min(c, n) relevant items).
//   k_te_metric     : grid (queries, cutoffs); mask -> the five metrics of the statement in the header, in its order of operations,
//                     -> q_metric and double-double block partials; k_te_final folds the partials in block order.
//   k_te_cover_mark / k_te_cover_count : position r of a list marks its item in the bitmap of the first cutoff above r (a word
//                     that already shows the bit is left alone: the lists name the same popular items over and over);
//                     cover[k] = popcount of the OR of the bitmaps 0 .. k.
// Every loop is grid-stride; integer atomics and ORs only, so the results do not depend on the grid or on the order.
#include "common.h"

namespace xmap {

constexpr int EV_THREADS = 256;
constexpr int EV_MAX_BLOCKS = 512;               // 8 waves per CU: these passes wait on memory, they are not the time of the tail
constexpr int EV_MAX_CUT = 8;
constexpr int EV_MAX_TOP = 64;
constexpr int EV_PART_BLOCKS = 256;             // blocks (per cutoff) of the metric pass
constexpr int EV_PART = 13;                     // 5 x (hi, lo) + evaluated, queries with a hit, hits

struct EvCuts { int n; int c[EV_MAX_CUT]; };

static unsigned ev_blocks(long long n, int cap = EV_MAX_BLOCKS) {
    const long long b = (n + EV_THREADS - 1) / EV_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// 0 ignored, 1 relevant, 2 below rel_min
__device__ __forceinline__ int ev_class(int u, int i, double r, double rel_min, long long U, int I) {
    if (u < 0 || u >= U || i < 0 || i >= I || r != r) return 0;
    return r >= rel_min ? 1 : 2;
}

__global__ __launch_bounds__(EV_THREADS) void k_ev_count(long long n, const int *tu, const int *ti, const double *tr, double rel_min,
                                                         long long U, int I, int *n_rel, unsigned long long *counters /*[3]*/) {
    long long c_rel = 0, c_ign = 0, c_low = 0;
    const long long stride = (long long)gridDim.x * EV_THREADS;
    for (long long base = (long long)blockIdx.x * EV_THREADS; base < n; base += stride) {
        const long long p = base + threadIdx.x;
        int cls = -1, u = 0;
        if (p < n) { u = tu[p]; cls = ev_class(u, ti[p], tr[p], rel_min, U, I); }
        c_rel += cls == 1; c_ign += cls == 0; c_low += cls == 2;
        const bool rel = cls == 1;
        const unsigned long long m = __ballot(rel);
        if (m == 0ull) continue;
        const int first = __ffsll((long long)m) - 1;
        const int u0 = rl32(u, first);
        if (__ballot(rel && u != u0) == 0ull) {             // one user: one atomic for the wave
            if (lane_id() == first) atomicAdd(&n_rel[u0], __popcll(m));
        } else if (rel) {
            atomicAdd(&n_rel[u], 1);
        }
    }
    c_rel = wave_sum_ll(c_rel); c_ign = wave_sum_ll(c_ign); c_low = wave_sum_ll(c_low);
    __shared__ long long sh[EV_THREADS / 64][3];
    if (lane_id() == 0) { sh[threadIdx.x >> 6][0] = c_rel; sh[threadIdx.x >> 6][1] = c_ign; sh[threadIdx.x >> 6][2] = c_low; }
    __syncthreads();
    if (threadIdx.x < 3) {
        long long s = 0;
        for (int w = 0; w < EV_THREADS / 64; w++) s += sh[w][threadIdx.x];
        if (s) atomicAdd(&counters[threadIdx.x], (unsigned long long)s);
    }
}

__global__ __launch_bounds__(EV_THREADS) void k_ev_flag(long long U, const int *n_rel, int *flag) {
    for (long long u = (long long)blockIdx.x * EV_THREADS + threadIdx.x; u < U; u += (long long)gridDim.x * EV_THREADS)
        flag[u] = n_rel[u] > 0;
}

__global__ __launch_bounds__(EV_THREADS) void k_ev_compact(long long U, const int *n_rel, const long long *pos, int *eval_user) {
    for (long long u = (long long)blockIdx.x * EV_THREADS + threadIdx.x; u < U; u += (long long)gridDim.x * EV_THREADS)
        if (n_rel[u] > 0) eval_user[pos[u]] = (int)u;
}

__global__ __launch_bounds__(EV_THREADS) void k_te_map(long long Q, const int *query_user, long long U, int *u2q) {
    for (long long q = (long long)blockIdx.x * EV_THREADS + threadIdx.x; q < Q; q += (long long)gridDim.x * EV_THREADS) {
        const int u = query_user[q];
        if (u >= 0 && u < U) atomicMax(&u2q[u], (int)q);
    }
}

__global__ __launch_bounds__(EV_THREADS) void k_te_verify(long long Q, const int *query_user, long long U, const int *u2q, int *dup) {
    for (long long q = (long long)blockIdx.x * EV_THREADS + threadIdx.x; q < Q; q += (long long)gridDim.x * EV_THREADS) {
        const int u = query_user[q];
        if (u >= 0 && u < U && u2q[u] != (int)q) *dup = 1;
    }
}

__global__ __launch_bounds__(EV_THREADS) void k_te_mark(long long n, const int *tu, const int *ti, const double *tr, double rel_min,
                                                        long long U, int I, const int *u2q, int n_top, const int *out_cnt,
                                                        const int *out_item, unsigned long long *q_mask) {
    for (long long p = (long long)blockIdx.x * EV_THREADS + threadIdx.x; p < n; p += (long long)gridDim.x * EV_THREADS) {
        const int u = tu[p], it = ti[p];
        if (ev_class(u, it, tr[p], rel_min, U, I) != 1) continue;
        const int q = u2q[u];
        if (q < 0) continue;
        int cnt = out_cnt[q];
        cnt = cnt < 0 ? 0 : (cnt > n_top ? n_top : cnt);
        const int *l = out_item + (size_t)q * n_top;
        unsigned long long bits = 0ull;
        for (int r = 0; r < cnt; r++)
            if (l[r] == it) bits |= 1ull << r;
        if (bits) atomicOr(&q_mask[q], bits);
    }
}

__global__ __launch_bounds__(64) void k_te_idcg(int n_top, const double *dtab, double *pre /*[n_top + 1]*/) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    pre[0] = s;
    for (int r = 0; r < n_top; r++) { s = s + dtab[r]; pre[r + 1] = s; }
}

// blockIdx.y = cutoff.  The statement of include/xmap_hip.h: only the ranks that hit add anything, so the loop visits the
// set bits of the mask in ascending order -- the same operations in the same order.
__global__ __launch_bounds__(EV_THREADS) void k_te_metric(long long Q, const int *query_user, long long U, const int *n_rel, int n_top,
                                                          const int *out_cnt, EvCuts cuts, const double *dtab, const double *pre,
                                                          unsigned long long *q_mask, double *q_metric, double *part) {
    const int k = blockIdx.y, c = cuts.c[k];
    double sh_[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, sl_[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double n_ev = 0.0, n_hitq = 0.0, n_hits = 0.0;
    const long long stride = (long long)gridDim.x * EV_THREADS;
    for (long long q = (long long)blockIdx.x * EV_THREADS + threadIdx.x; q < Q; q += stride) {
        const int u = query_user[q];
        const int n = (u >= 0 && u < U) ? n_rel[u] : 0;
        double m5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (n > 0) {
            int L = out_cnt[q];
            L = L < 0 ? 0 : (L > n_top ? n_top : L);
            const int lim = c < L ? c : L;
            unsigned long long mm = q_mask[q];
            if (lim < 64) mm &= (1ull << lim) - 1ull;
            int h = 0;
            double dcg = 0.0, ap = 0.0, rr = 0.0;
            while (mm) {
                const int r = __ffsll((long long)mm) - 1;
                mm &= mm - 1ull;
                h++;
                dcg = dcg + dtab[r];
                ap = ap + (double)h / (double)(r + 1);
                if (rr == 0.0) rr = 1.0 / (double)(r + 1);
            }
            const int cn = c < n ? c : n;
            m5[0] = (double)h / (double)c;
            m5[1] = (double)h / (double)n;
            m5[2] = dcg / pre[cn];
            m5[3] = ap / (double)cn;
            m5[4] = rr;
            n_ev += 1.0; n_hitq += h > 0 ? 1.0 : 0.0; n_hits += (double)h;
#pragma unroll
            for (int x = 0; x < 5; x++) dd_add(sh_[x], sl_[x], m5[x]);
        } else if (k == 0) {
            q_mask[q] = 0ull;                   // not evaluated (no other cutoff's blocks read the mask of such a query)
        }
        if (q_metric) {
            double *o = q_metric + ((size_t)q * cuts.n + k) * 5;
#pragma unroll
            for (int x = 0; x < 5; x++) o[x] = m5[x];
        }
    }
#pragma unroll
    for (int x = 0; x < 5; x++) dd_reduce<64>(sh_[x], sl_[x]);
    n_ev = wave_sum(n_ev); n_hitq = wave_sum(n_hitq); n_hits = wave_sum(n_hits);    // integers below 2^53: exact
    __shared__ double sh[EV_THREADS / 64][EV_PART];
    const int wv = threadIdx.x >> 6;
    if (lane_id() == 0) {
#pragma unroll
        for (int x = 0; x < 5; x++) { sh[wv][2 * x] = sh_[x]; sh[wv][2 * x + 1] = sl_[x]; }
        sh[wv][10] = n_ev; sh[wv][11] = n_hitq; sh[wv][12] = n_hits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = part + ((size_t)blockIdx.x * cuts.n + k) * EV_PART;
        for (int x = 0; x < 5; x++) {
            double a = 0.0, al = 0.0;
            for (int w = 0; w < EV_THREADS / 64; w++) { dd_add(a, al, sh[w][2 * x]); dd_add(a, al, sh[w][2 * x + 1]); }
            o[2 * x] = a; o[2 * x + 1] = al;
        }
        for (int x = 10; x < EV_PART; x++) {
            double a = 0.0;
            for (int w = 0; w < EV_THREADS / 64; w++) a += sh[w][x];
            o[x] = a;
        }
    }
}

__global__ __launch_bounds__(64) void k_te_final(int n_blocks, int n_cut, const double *part, const unsigned long long *cover_cnt,
                                                 double *agg /*[n_cut][8]*/, long long *cover /*[n_cut]*/) {
    const int k = threadIdx.x;
    if (k >= n_cut) return;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, l[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, cnt[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < n_blocks; b++) {
        const double *p = part + ((size_t)b * n_cut + k) * EV_PART;
        for (int x = 0; x < 5; x++) { dd_add(s[x], l[x], p[2 * x]); dd_add(s[x], l[x], p[2 * x + 1]); }
        for (int x = 0; x < 3; x++) cnt[x] += p[10 + x];
    }
    double *o = agg + (size_t)k * 8;
    for (int x = 0; x < 3; x++) o[x] = cnt[x];
    for (int x = 0; x < 5; x++) o[3 + x] = s[x];
    cover[k] = (long long)cover_cnt[k];
}

__global__ __launch_bounds__(EV_THREADS) void k_te_cover_mark(long long Q, int n_top, int I, const int *out_cnt, const int *out_item,
                                                              EvCuts cuts, long long words, unsigned int *bitmap /*[n_cut][words]*/) {
    const long long total = Q * n_top;
    const int c_last = cuts.c[cuts.n - 1];
    for (long long e = (long long)blockIdx.x * EV_THREADS + threadIdx.x; e < total; e += (long long)gridDim.x * EV_THREADS) {
        const long long q = e / n_top;
        const int r = (int)(e - q * n_top);
        if (r >= c_last) continue;
        int cnt = out_cnt[q];
        cnt = cnt > n_top ? n_top : cnt;
        if (r >= cnt) continue;
        const int it = out_item[e];
        if (it < 0 || it >= I) continue;
        int k = 0;
        while (r >= cuts.c[k]) k++;             // r < c_last: ends inside the table
        unsigned int *w = bitmap + (size_t)k * words + (it >> 5);
        const unsigned int bit = 1u << (it & 31);
        if ((*w & bit) == 0u) atomicOr(w, bit);
    }
}

__global__ __launch_bounds__(EV_THREADS) void k_te_cover_count(long long words, EvCuts cuts, const unsigned int *bitmap,
                                                               unsigned long long *cover_cnt /*[EV_MAX_CUT]*/) {
    long long cnt[EV_MAX_CUT];
#pragma unroll
    for (int k = 0; k < EV_MAX_CUT; k++) cnt[k] = 0;
    for (long long w = (long long)blockIdx.x * EV_THREADS + threadIdx.x; w < words; w += (long long)gridDim.x * EV_THREADS) {
        unsigned int acc = 0u;
#pragma unroll
        for (int k = 0; k < EV_MAX_CUT; k++) {
            if (k < cuts.n) { acc |= bitmap[(size_t)k * words + w]; cnt[k] += __popc(acc); }
        }
    }
    __shared__ long long sh[EV_THREADS / 64][EV_MAX_CUT];
#pragma unroll
    for (int k = 0; k < EV_MAX_CUT; k++) {
        const long long s = wave_sum_ll(cnt[k]);
        if (lane_id() == 0) sh[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < cuts.n) {
        long long s = 0;
        for (int w = 0; w < EV_THREADS / 64; w++) s += sh[w][threadIdx.x];
        if (s) atomicAdd(&cover_cnt[threadIdx.x], (unsigned long long)s);
    }
}

}  // namespace xmap
using namespace xmap;

extern "C" {

int xmap_eval_users(void *stream, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const double *test_rating,
                    double rel_min, int64_t n_users, int32_t n_items, int32_t *n_rel, int32_t *eval_user, int64_t *h_counts) {
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    XM_ARG(h_counts && rel_min == rel_min);
    XM_ARG(n_test >= 0 && n_users >= 0 && n_users <= INT32_MAX && n_items >= 0);
    XM_ARG(n_test == 0 || (test_user && test_item && test_rating));
    XM_ARG(n_users == 0 || (n_rel && eval_user));
    h_counts[0] = h_counts[1] = h_counts[2] = h_counts[3] = 0;
    const long long U = n_users;
    unsigned long long *counters = nullptr;
    XM_HIP(xm_malloc_async((void **)&counters, sizeof(unsigned long long) * 4, st));
    XM_HIP(hipMemsetAsync(counters, 0, sizeof(unsigned long long) * 4, st));
    if (U > 0) XM_HIP(hipMemsetAsync(n_rel, 0, sizeof(int) * (size_t)U, st));
    if (n_test > 0) {
        // with no user every pair is ignored: the kernel then never touches n_rel
        k_ev_count<<<dim3(ev_blocks(n_test)), dim3(EV_THREADS), 0, st>>>(n_test, test_user, test_item, test_rating, rel_min, U, n_items, n_rel,
                                                                         counters);
        XM_LAUNCH_CHECK();
    }
    int64_t n_eval = 0;
    if (U > 0) {
        int *flag = nullptr;
        long long *pos = nullptr;
        XM_HIP(xm_malloc_async((void **)&flag, sizeof(int) * (size_t)U, st));
        XM_HIP(xm_malloc_async((void **)&pos, sizeof(long long) * ((size_t)U + 1), st));
        k_ev_flag<<<dim3(ev_blocks(U)), dim3(EV_THREADS), 0, st>>>(U, n_rel, flag);
        XM_LAUNCH_CHECK();
        const int rc = xmap_exclusive_scan_i32_to_i64(st, flag, (int64_t *)pos, U, &n_eval);
        if (rc) return rc;
        if (n_eval > 0) {
            k_ev_compact<<<dim3(ev_blocks(U)), dim3(EV_THREADS), 0, st>>>(U, n_rel, pos, eval_user);
            XM_LAUNCH_CHECK();
        }
    }
    unsigned long long h[4] = {0, 0, 0, 0};
    XM_HIP(hipMemcpyAsync(h, counters, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    h_counts[0] = n_eval; h_counts[1] = (int64_t)h[0]; h_counts[2] = (int64_t)h[1]; h_counts[3] = (int64_t)h[2];
    return XMAP_OK;
}

int xmap_topn_eval(void *stream, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const double *test_rating,
                   double rel_min, int64_t n_users, int32_t n_items, const int32_t *n_rel, int64_t n_query, const int32_t *query_user,
                   int32_t n_top, const int32_t *out_cnt, const int32_t *out_item, int32_t n_cut, const int32_t *h_cut, const double *dtab,
                   uint64_t *q_mask, double *q_metric, double *agg, int64_t *cover) {
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    XM_ARG(n_top >= 1 && n_top <= EV_MAX_TOP);
    XM_ARG(n_cut >= 1 && n_cut <= EV_MAX_CUT && h_cut);
    EvCuts cuts;
    cuts.n = n_cut;
    for (int k = 0; k < EV_MAX_CUT; k++) cuts.c[k] = k < n_cut ? h_cut[k] : INT32_MAX;
    for (int k = 0; k < n_cut; k++) XM_ARG(cuts.c[k] >= 1 && cuts.c[k] <= n_top && (k == 0 || cuts.c[k] > cuts.c[k - 1]));
    XM_ARG(rel_min == rel_min && dtab && agg && cover);
    XM_ARG(n_test >= 0 && n_users >= 0 && n_users <= INT32_MAX && n_items >= 0 && n_query >= 0 && n_query <= INT32_MAX);
    XM_ARG(n_test == 0 || (test_user && test_item && test_rating));
    XM_ARG(n_users == 0 || n_rel);
    XM_ARG(n_query == 0 || (query_user && out_cnt && out_item && q_mask));
    const long long U = n_users, Q = n_query;
    const int I = n_items;
    // ---- user -> query, and the check that no user is listed twice
    int *u2q = nullptr, *dup = nullptr;
    XM_HIP(xm_malloc_async((void **)&u2q, sizeof(int) * (size_t)(U ? U : 1), st));
    XM_HIP(xm_malloc_async((void **)&dup, sizeof(int), st));
    XM_HIP(hipMemsetAsync(u2q, 0xff, sizeof(int) * (size_t)(U ? U : 1), st));
    XM_HIP(hipMemsetAsync(dup, 0, sizeof(int), st));
    if (Q > 0) {
        k_te_map<<<dim3(ev_blocks(Q)), dim3(EV_THREADS), 0, st>>>(Q, query_user, U, u2q);
        XM_LAUNCH_CHECK();
        k_te_verify<<<dim3(ev_blocks(Q)), dim3(EV_THREADS), 0, st>>>(Q, query_user, U, u2q, dup);
        XM_LAUNCH_CHECK();
        int h_dup = 0;
        XM_HIP(hipMemcpyAsync(&h_dup, dup, sizeof(int), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
        if (h_dup) {
            set_error("%s:%d bad argument: a user is listed more than once in query_user", __FILE__, __LINE__);
            return XMAP_ERR_ARG;
        }
    }
    // ---- hit masks
    if (Q > 0) XM_HIP(hipMemsetAsync(q_mask, 0, sizeof(uint64_t) * (size_t)Q, st));
    if (Q > 0 && n_test > 0) {
        k_te_mark<<<dim3(ev_blocks(n_test)), dim3(EV_THREADS), 0, st>>>(n_test, test_user, test_item, test_rating, rel_min, U, I, u2q, n_top,
                                                                        out_cnt, out_item, (unsigned long long *)q_mask);
        XM_LAUNCH_CHECK();
    }
    // ---- coverage
    const long long words = ((long long)I + 31) / 32;
    unsigned int *bitmap = nullptr;
    unsigned long long *cover_cnt = nullptr;
    const size_t bm_bytes = sizeof(unsigned int) * (size_t)n_cut * (size_t)(words ? words : 1);
    XM_HIP(xm_malloc_async((void **)&bitmap, bm_bytes, st));
    XM_HIP(xm_malloc_async((void **)&cover_cnt, sizeof(unsigned long long) * EV_MAX_CUT, st));
    XM_HIP(hipMemsetAsync(cover_cnt, 0, sizeof(unsigned long long) * EV_MAX_CUT, st));
    if (Q > 0 && words > 0) {
        XM_HIP(hipMemsetAsync(bitmap, 0, bm_bytes, st));
        k_te_cover_mark<<<dim3(ev_blocks(Q * n_top)), dim3(EV_THREADS), 0, st>>>(Q, n_top, I, out_cnt, out_item, cuts, words, bitmap);
        XM_LAUNCH_CHECK();
        k_te_cover_count<<<dim3(ev_blocks(words)), dim3(EV_THREADS), 0, st>>>(words, cuts, bitmap, cover_cnt);
        XM_LAUNCH_CHECK();
    }
    // ---- metrics and aggregates
    double *pre = nullptr, *part = nullptr;
    const unsigned mblocks = Q > 0 ? ev_blocks(Q, EV_PART_BLOCKS) : 0;
    XM_HIP(xm_malloc_async((void **)&pre, sizeof(double) * (EV_MAX_TOP + 1), st));
    XM_HIP(xm_malloc_async((void **)&part, sizeof(double) * EV_PART * EV_MAX_CUT * EV_PART_BLOCKS, st));
    if (Q > 0) {
        k_te_idcg<<<dim3(1), dim3(64), 0, st>>>(n_top, dtab, pre);
        XM_LAUNCH_CHECK();
        k_te_metric<<<dim3(mblocks, (unsigned)n_cut), dim3(EV_THREADS), 0, st>>>(Q, query_user, U, n_rel, n_top, out_cnt, cuts, dtab, pre,
                                                                                 (unsigned long long *)q_mask, q_metric, part);
        XM_LAUNCH_CHECK();
    }
    k_te_final<<<dim3(1), dim3(64), 0, st>>>((int)mblocks, n_cut, part, cover_cnt, agg, (long long *)cover);
    XM_LAUNCH_CHECK();
    XM_HIP(hipStreamSynchronize(st));
    return XMAP_OK;
}
}
