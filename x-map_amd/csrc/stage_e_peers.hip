// stage_e_peers.hip -- similar users on the device: for every query user the N resident users whose profiles are most alike
// (DESIGN.md 4 "Peers").  The transpose of the item fold-in (stage_e_itemfold.hip): there one new item against the items of its
// raters' profiles, here one user against the holders of the items of its own profile; the same "sort, don't hash" -- expand
// records, stable radix_sort_pairs, run heads, one lane per run -- and no floating-point atomic, so the bits depend on neither
// the grid nor the chunking.
//
// x(p) = prof_rating[p] - centre[prof_item[p]] (centre == NULL: the rating itself); a row is VALID iff 0 <= prof_item[p] < I.
// The index (xmap_peer_index): the item-major transposition of the valid resident rows in HOLDER ORDER (ascending row index = user
// ascending, then profile order), x beside the user, and nrm(u) = sqrt(the bilinear form of u with itself) of every user.
//   k_pr_item_keys : key = the row's item (invalid: I, sorted behind everything), value = the row -> radix_sort_pairs (stable)
//   k_pr_hd_ptr    : hd_ptr[i] = the first sorted position whose key is >= i (bisection), i <= I
//   k_pr_hd_fill   : hd_user (bisection of prof_ptr) and hd_x per sorted position
//   k_pr_norm      : one wave per user; the wave finds the rows r with the item of row p by ballot, every lane runs the same
//                    double-double chain in record order (p in profile order, r in profile order)
// The rows (xmap_peer_rows): the queries are cut into chunks of consecutive queries whose records number at most max_records
// (sorted_runs.h: the plan pr_plan_chunks, the walk pr_each_chunk).
//   k_pr_qlen / k_pr_count : rows per query -> scan; records per query row = holders of its item (under a mask: the ELIGIBLE
//                    holders, one wave per row counting ballots) -> scan = rec_off
//   k_pr_expand    : one thread per record (its row and query by bisection): key = (q - q0) << user_bits | v, value = the record's
//                    index, t = fl(x(p) x(h)).  k_pr_expand_masked: one wave per query row walks the holders and compacts the
//                    eligible ones in holder order -- no record of an ineligible user is written
//   pr_run_tables  : (sorted_runs.h) the stable sort -- the records of one (q, v) stay in expansion order --, the runs, per query
//                    of the chunk its first run
//   k_pr_reduce    : one lane per run: self rule, exclusion list, min_common, dot = the double-double chain, sim, the floor
//   pr_select      : au_select_segment (au_select.h) over the runs of a query; position in the segment ascends with the user
// With the local sensitivity (xmap_peer_rows_ls; LS = true of the templates below -- xmap_peer_rows is the LS = false code): the
// expansion writes the two factors of a record instead of their product, the reduce multiplies them (the same bits) and keeps the
// dot of every run, and after the selection
//   k_pr_ls        : one wave per returned entry: its run by bisection among the runs of the query (they ascend with the user),
//                    the leave-one-out distances of the records lane-strided, the largest as an integer (ls_key of tri.h: a
//                    maximum of integers, so the order of the lanes does not matter)
#include <vector>

#include "common.h"
#include "au_select.h"
#include "predict_rows.h"
#include "rec_filter.h"
#include "sorted_runs.h"
#include "tri.h"

namespace xmap {

// A record takes 64 B of temporaries (80 B with the local sensitivity): the default chunk (PR_MAX_RECORDS) 270 MB.

__device__ __forceinline__ double pr_x(const int *item, const double *rating, const double *centre, long long p) {
    return centre ? rating[p] - centre[item[p]] : rating[p];
}

__global__ __launch_bounds__(256) void k_pr_item_keys(long long n_rows, int I, const int *pitem, unsigned long long *keys, int *vals) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int it = pitem[r];
    keys[r] = (it < 0 || it >= I) ? (unsigned long long)I : (unsigned long long)it;
    vals[r] = (int)r;
}

__global__ __launch_bounds__(256) void k_pr_hd_ptr(int I, long long n_rows, const unsigned long long *keys, long long *hd_ptr) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > I) return;
    long long lo = 0, hi = n_rows;              // first position in [0, n_rows] with key >= i
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] >= (unsigned long long)i) hi = mid; else lo = mid + 1;
    }
    hd_ptr[i] = lo;
}

__global__ __launch_bounds__(256) void k_pr_hd_fill(long long n_rows, long long U, int I, const unsigned long long *keys, const int *vals,
                                                    const long long *pptr, const int *pitem, const double *prating, const double *centre,
                                                    int *hd_user, double *hd_x) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows) return;
    if (keys[t] >= (unsigned long long)I) { hd_user[t] = -1; hd_x[t] = 0.0; return; }   // behind hd_ptr[I]: never read
    const long long r = vals[t];
    hd_user[t] = (int)pr_last_le(pptr, 0, U, r);        // users without rows are passed over
    hd_x[t] = pr_x(pitem, prating, centre, r);
}

// one wave per entry k of the list: user u = sel ? sel[k] : k; out[k] = nrm(u), 0.0 for a user outside [0, U)
// (base: the first entry of this launch -- for_pair_ranges of predict_rows.h keeps every grid below 2^32 threads)
__global__ __launch_bounds__(256) void k_pr_norm(long long base, long long n, const int *sel, long long U, int I, const long long *pptr, const int *pitem,
                                                 const double *prating, const double *centre, double *out) {
    const long long k = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (k >= n) return;                         // (wave-uniform)
    const int lane = lane_id();
    const long long u = sel ? (long long)sel[k] : k;
    long long p0 = 0, p1 = 0;
    if (u >= 0 && u < U) { p0 = pptr[u]; p1 = pptr[u + 1]; }
    double hi = 0.0, lo = 0.0;
    for (long long p = p0; p < p1; p++) {
        const int ip = pitem[p];
        if (ip < 0 || ip >= I) continue;        // (wave-uniform)
        const double xp = pr_x(pitem, prating, centre, p);
        for (long long base = p0; base < p1; base += WAVE) {
            const long long r = base + lane;
            const bool m = r < p1 && pitem[r] == ip;
            const double xr = m ? pr_x(pitem, prating, centre, r) : 0.0;
            unsigned long long mask = __ballot(m);
            while (mask) {                      // every lane runs the same chain
                const int l = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                dd_add(hi, lo, xp * __shfl(xr, l, WAVE));
            }
        }
    }
    if (lane == 0) out[k] = sqrt(hi);           // a negative or NaN sum: NaN
}

// rows of query q in the query CSR: 0 for a query user outside it
__global__ __launch_bounds__(256) void k_pr_qlen(long long n_query, const int *query_user, long long n_q_users, const long long *qptr, int *qlen) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_query) return;
    const long long a = query_user[q];
    qlen[q] = (a >= 0 && a < n_q_users) ? (int)(qptr[a + 1] - qptr[a]) : 0;
}

// records of flattened query row e (one wave per row): the holders of its item, under a mask the eligible ones
__global__ __launch_bounds__(256) void k_pr_count(long long base, long long n_qrows, long long n_query, const long long *qrow_off, const int *query_user,
                                                  const long long *qptr, const int *qitem, int I, const long long *hd_ptr, const int *hd_user,
                                                  const unsigned int *allow, int *cnt) {
    const long long e = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (e >= n_qrows) return;
    const int lane = lane_id();
    const long long q = pr_last_le(qrow_off, 0, n_query, e);
    const long long p = qptr[query_user[q]] + (e - qrow_off[q]);
    const int it = qitem[p];
    int c = 0;
    if (it >= 0 && it < I) {
        const long long h0 = hd_ptr[it], h1 = hd_ptr[it + 1];
        if (!allow) c = (int)(h1 - h0);
        else
            for (long long base = h0; base < h1; base += WAVE) {
                const long long h = base + lane;
                c += __popcll(__ballot(h < h1 && bit_allowed(allow, hd_user[h])));
            }
    }
    if (lane == 0) cnt[e] = c;
}

template <bool LS>
__global__ __launch_bounds__(256) void k_pr_expand(long long n, long long rec0, long long e0, long long e1, long long q0, long long q1,
                                                   const long long *qrow_off, const long long *rec_off, const int *query_user,
                                                   const long long *qptr, const int *qitem, const double *qrating, const double *centre,
                                                   const long long *hd_ptr, const int *hd_user, const double *hd_x, int user_bits,
                                                   unsigned long long *keys, int *vals, double *tv, double *tb) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const long long g = rec0 + t;
    const long long e = pr_last_le(rec_off, e0, e1, g);         // rows without records are passed over
    const long long q = pr_last_le(qrow_off, q0, q1, e);        // queries without rows too
    const long long p = qptr[query_user[q]] + (e - qrow_off[q]);
    const long long h = hd_ptr[qitem[p]] + (g - rec_off[e]);    // (a row with records has a valid item)
    keys[t] = ((unsigned long long)(q - q0) << user_bits) | (unsigned long long)(unsigned)hd_user[h];
    vals[t] = (int)t;
    if constexpr (LS) { tv[t] = pr_x(qitem, qrating, centre, p); tb[t] = hd_x[h]; }     // the factors: the query's x, the holder's x
    else tv[t] = pr_x(qitem, qrating, centre, p) * hd_x[h];
}

// under a mask: one wave per query row of the chunk, the eligible holders compacted in holder order at rec_off[e] - rec0
template <bool LS>
__global__ __launch_bounds__(256) void k_pr_expand_masked(long long rec0, long long e0, long long e1, long long q0, long long q1,
                                                          const long long *qrow_off, const long long *rec_off, const int *query_user,
                                                          const long long *qptr, const int *qitem, const double *qrating,
                                                          const double *centre, int I, const long long *hd_ptr, const int *hd_user,
                                                          const double *hd_x, const unsigned int *allow, int user_bits,
                                                          unsigned long long *keys, int *vals, double *tv, double *tb) {
    const long long e = e0 + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (e >= e1) return;
    const int lane = lane_id();
    const long long end = rec_off[e + 1] - rec0;
    long long o = rec_off[e] - rec0;
    if (o == end) return;                       // no eligible holder (or an invalid item)
    const long long q = pr_last_le(qrow_off, q0, q1, e);
    const long long p = qptr[query_user[q]] + (e - qrow_off[q]);
    const int it = qitem[p];
    if (it < 0 || it >= I) return;
    const double xp = pr_x(qitem, qrating, centre, p);
    const long long h1 = hd_ptr[it + 1];
    for (long long base = hd_ptr[it]; base < h1; base += WAVE) {
        const long long h = base + lane;
        const int v = h < h1 ? hd_user[h] : 0;
        const bool m = h < h1 && bit_allowed(allow, v);
        const unsigned long long mask = __ballot(m);
        const long long at = o + __popcll(mask & lanemask_lt());
        if (m && at < end) {                    // (at < end: the count pass saw the same mask)
            keys[at] = ((unsigned long long)(q - q0) << user_bits) | (unsigned long long)(unsigned)v;
            vals[at] = (int)at;
            if constexpr (LS) { tv[at] = xp; tb[at] = hd_x[h]; }
            else tv[at] = xp * hd_x[h];
        }
        o += __popcll(mask);
    }
}

// one lane per run, records in sorted (= expansion) order.  cnt: [0] dropped by min_common, [1] non-finite, [2] below the floor
// LS: tv / tb are the factors, r_dot[r] = the dot of a kept run
template <bool LS>
__global__ __launch_bounds__(256) void k_pr_reduce(long long n, const unsigned long long *keys, const int *vals, const double *tv,
                                                   const double *tb, double *r_dot, const long long *run_idx, const int *run_start,
                                                   int user_bits, long long q0, const int *query_user, int same, int keep_self, const long long *ex_ptr,
                                                   const int *ex_id, int min_common, int cap, double min_score, const double *qnrm,
                                                   const double *nrm, int *r_status, double *r_sim, int *r_common,
                                                   unsigned long long *cnt) {
    const long long n_runs = run_idx[n];
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_runs; r += step) {
        const int s = run_start[r], e = run_start[r + 1];
        const unsigned long long key = keys[s];
        const long long q = q0 + (long long)(key >> user_bits);
        const int v = (int)(key & ((1ull << user_bits) - 1ull));
        const int nc = e - s;
        r_common[r] = nc;
        r_sim[r] = 0.0;
        bool out = same && !keep_self && v == query_user[q];
        if (!out && ex_ptr) {
            const long long x1 = ex_ptr[q + 1];
            for (long long x = ex_ptr[q]; x < x1 && !out; x++) out = ex_id[x] == v;
        }
        if (out) { r_status[r] = PR_NOT_CANDIDATE; continue; }
        if (nc < min_common) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[0], 1ull); continue; }
        double dot = 0.0, lo = 0.0;
        if constexpr (LS) {
            for (int t = s; t < e; t++) { const int i = vals[t]; dd_add(dot, lo, tv[i] * tb[i]); }
            r_dot[r] = dot;
        } else
            for (int t = s; t < e; t++) dd_add(dot, lo, tv[vals[t]]);
        const double np = qnrm[q] * nrm[v];
        const double sim = weighted((np != 0.0) ? dot / np : 0.0, nc, cap);     // NaN != 0: divides
        if (!finite_f64(sim)) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[1], 1ull); continue; }
        if (sim < min_score) { r_status[r] = PR_DROPPED; atomicAdd(&cnt[2], 1ull); continue; }
        r_sim[r] = sim;
        r_status[r] = 0;
    }
}

// k_pr_select (cnt [3] candidates after the self rule, the exclusions and the mask, [4] the largest such count of one query)
// and k_pr_blank: sorted_runs.h

// The local sensitivity of the returned entries of a chunk, one wave per cell c = x * n_top + j of its nq queries (base: the first
// cell of this launch).  Entry j of query q0 + x is user v; its run is the one of v among the runs [first[x], first[x + 1]) of the
// query, which ascend with the user.  Per record, with a / b the query's and the holder's x (recommenderSim.py:98-116 between
// users, as k_if_reduce takes it between items): rest = inner - a b; the two norms with the record left out of one side;
// d = |weighted(rest / m, n - 1, cap) - sim|.  ls = the largest d, NaN above everything.
__global__ __launch_bounds__(256) void k_pr_ls(long long base, long long n_cells, long long q0, int n_top, const long long *first,
                                               const unsigned long long *keys, const int *vals, const double *ta, const double *tb,
                                               const int *run_start, int user_bits, const double *r_dot, int cap, const double *qnrm,
                                               const double *nrm, const int *out_cnt, const int *out_user, const double *out_sim,
                                               double *out_ls) {
    const long long c = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (c >= n_cells) return;                   // (wave-uniform)
    const long long x = c / n_top;
    const int j = (int)(c - x * n_top);
    const long long q = q0 + x;
    if (j >= out_cnt[q]) return;                // behind the count: the blank 0.0 stands
    const size_t o = (size_t)q * n_top + j;
    const int v = out_user[o];
    const unsigned long long umask = (1ull << user_bits) - 1ull;
    long long lo = first[x], hi = first[x + 1];         // the first run of the query whose user is >= v
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)(keys[run_start[mid]] & umask) >= (long long)v) hi = mid; else lo = mid + 1;
    }
    if (lo >= first[x + 1] || (int)(keys[run_start[lo]] & umask) != v) return;      // (every returned entry has its run)
    const int s = run_start[lo], e = run_start[lo + 1];
    const int nc = e - s;
    const double inner = r_dot[lo], sim = out_sim[o];
    const double nx = qnrm[q], ny = nrm[v];
    long long best = 0ll;                       // ls_key: the bits of a non-negative double, below 2^63
    for (int t = s + lane_id(); t < e; t += WAVE) {
        const int i = vals[t];
        const double a = ta[i], b = tb[i];
        const double rest = inner - a * b;
        const double m1 = sqrt((nx * nx - a * a) * (ny * ny));
        const double m2 = sqrt((nx * nx) * (ny * ny - b * b));
        const double d1 = fabs(weighted((m1 != 0.0) ? 1.0 * rest / m1 : 0.0, nc - 1, cap) - sim);
        const double d2 = fabs(weighted((m2 != 0.0) ? 1.0 * rest / m2 : 0.0, nc - 1, cap) - sim);
        const long long k1 = (long long)ls_key(d1), k2 = (long long)ls_key(d2);
        const long long k = k1 > k2 ? k1 : k2;
        best = k > best ? k : best;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const long long other = __shfl_xor(best, m, WAVE);
        best = other > best ? other : best;
    }
    if (lane_id() == 0) out_ls[o] = __longlong_as_double(best);
}

// avg[i] of the x of item i's holders: the exact double-double sum rounded once, divided by the entries -- what item_stats.h
// computes for an item of RecommenderSim (lane-strided sums, the fixed butterfly of dd_reduce); one wave per item
__global__ __launch_bounds__(256) void k_pr_centre(long long base, long long I, const long long *hd_ptr, const double *hd_x, double *avg) {
    const long long i = base + (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    const bool on = i < I;
    const int lane = lane_id();
    long long p0 = 0, p1 = 0;
    if (on) { p0 = hd_ptr[i]; p1 = hd_ptr[i + 1]; }
    double s = 0.0, slo = 0.0;
    for (long long p = p0 + lane; p < p1; p += WAVE) dd_add(s, slo, hd_x[p]);
    dd_reduce<WAVE>(s, slo);
    if (on && lane == 0) avg[i] = (p1 > p0) ? 1.0 * s / (double)(p1 - p0) : 0.0;
}

static int pr_norms(hipStream_t st, long long n, const int *sel, long long U, int I, const long long *pptr, const int *pitem,
                    const double *prating, const double *centre, double *out) {
    return for_pair_ranges(n, 4, [&](long long base, long long end, dim3 grid) {
        k_pr_norm<<<grid, dim3(256), 0, st>>>(base, end, sel, U, I, pptr, pitem, prating, centre, out);
    });
}

}  // namespace xmap

using namespace xmap;

// xmap_peer_rows (LS = false, out_ls unused) and xmap_peer_rows_ls (LS = true)
template <bool LS>
static int peer_rows_run(void *stream, int64_t n_query, const int32_t *query_user, int64_t n_q_users, const int64_t *q_ptr, const int32_t *q_item,
                         const double *q_rating, int32_t flags, int32_t n_top, int32_t cap, int32_t min_common, int64_t n_users, int32_t n_items,
                         const double *centre, const int64_t *hd_ptr, const int32_t *hd_user, const double *hd_x, const double *nrm,
                         int64_t max_records, int32_t *out_cnt, int32_t *out_user, double *out_sim, int32_t *out_common, double *out_ls,
                         const xmap_rec_filter *F, int64_t *h_stats);

extern "C" {

int xmap_peer_index(void *stream, int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                    const double *prof_rating, const double *centre, int64_t *hd_ptr, int32_t *hd_user, double *hd_x, double *nrm,
                    int64_t *h_rows) {
    XM_ARG(n_users >= 0 && n_users < 2147483647ll && n_items >= 0 && prof_ptr && hd_ptr && (n_users == 0 || nrm));
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    if (h_rows) *h_rows = 0;
    const int I = n_items;
    long long n_rows = 0;
    XM_HIP(hipMemcpyAsync(&n_rows, prof_ptr + n_users, sizeof(long long), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    XM_ARG(n_rows >= 0 && n_rows < 2147483647ll);
    XM_ARG(n_rows == 0 || (prof_item && prof_rating && hd_user && hd_x));
    if (n_rows == 0) {
        XM_HIP(hipMemsetAsync(hd_ptr, 0, sizeof(int64_t) * ((size_t)I + 1), st));
    } else {
        const size_t nr = (size_t)n_rows;
        unsigned long long *keys = nullptr;
        int *vals = nullptr;
        XM_HIP(xm_malloc_async((void **)&keys, sizeof(unsigned long long) * 2 * nr, st));
        XM_HIP(xm_malloc_async((void **)&vals, sizeof(int) * 2 * nr, st));
        const unsigned nb = blocks_for(n_rows, 256);
        k_pr_item_keys<<<dim3(nb), dim3(256), 0, st>>>(n_rows, I, prof_item, keys, vals);
        XM_LAUNCH_CHECK();
        int rc = radix_sort_pairs(st, keys, vals, keys + nr, vals + nr, n_rows, bits_for((long long)I + 1));
        if (rc) return rc;
        k_pr_hd_ptr<<<dim3(blocks_for((long long)I + 1, 256)), dim3(256), 0, st>>>(I, n_rows, keys, (long long *)hd_ptr);
        XM_LAUNCH_CHECK();
        k_pr_hd_fill<<<dim3(nb), dim3(256), 0, st>>>(n_rows, n_users, I, keys, vals, (const long long *)prof_ptr, prof_item, prof_rating,
                                                     centre, hd_user, hd_x);
        XM_LAUNCH_CHECK();
    }
    if (n_users > 0) {
        const int rc = pr_norms(st, n_users, nullptr, n_users, I, (const long long *)prof_ptr, prof_item, prof_rating, centre, nrm);
        if (rc) return rc;
    }
    long long rows = 0;
    XM_HIP(hipMemcpyAsync(&rows, hd_ptr + I, sizeof(long long), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_rows) *h_rows = rows;
    return XMAP_OK;
}

int xmap_peer_centre(void *stream, int32_t n_items, const int64_t *hd_ptr, const double *hd_x, double *centre) {
    XM_ARG(n_items >= 0 && (n_items == 0 || (hd_ptr && centre)));
    hipStream_t st = (hipStream_t)stream;
    return for_pair_ranges(n_items, 4, [&](long long base, long long, dim3 grid) {
        k_pr_centre<<<grid, dim3(256), 0, st>>>(base, n_items, (const long long *)hd_ptr, hd_x, centre);
    });
}

int xmap_peer_rows(void *stream, int64_t n_query, const int32_t *query_user, int64_t n_q_users, const int64_t *q_ptr, const int32_t *q_item,
                   const double *q_rating, int32_t flags, int32_t n_top, int32_t cap, int32_t min_common, int64_t n_users, int32_t n_items,
                   const double *centre, const int64_t *hd_ptr, const int32_t *hd_user, const double *hd_x, const double *nrm,
                   int64_t max_records, int32_t *out_cnt, int32_t *out_user, double *out_sim, int32_t *out_common, const xmap_rec_filter *F,
                   int64_t *h_stats) {
    return peer_rows_run<false>(stream, n_query, query_user, n_q_users, q_ptr, q_item, q_rating, flags, n_top, cap, min_common, n_users,
                                n_items, centre, hd_ptr, hd_user, hd_x, nrm, max_records, out_cnt, out_user, out_sim, out_common, nullptr,
                                F, h_stats);
}

int xmap_peer_rows_ls(void *stream, int64_t n_query, const int32_t *query_user, int64_t n_q_users, const int64_t *q_ptr,
                      const int32_t *q_item, const double *q_rating, int32_t flags, int32_t n_top, int32_t cap, int32_t min_common,
                      int64_t n_users, int32_t n_items, const double *centre, const int64_t *hd_ptr, const int32_t *hd_user,
                      const double *hd_x, const double *nrm, int64_t max_records, int32_t *out_cnt, int32_t *out_user, double *out_sim,
                      int32_t *out_common, double *out_ls, const xmap_rec_filter *F, int64_t *h_stats) {
    XM_ARG(out_ls);                             // also with n_query == 0
    return peer_rows_run<true>(stream, n_query, query_user, n_q_users, q_ptr, q_item, q_rating, flags, n_top, cap, min_common, n_users,
                               n_items, centre, hd_ptr, hd_user, hd_x, nrm, max_records, out_cnt, out_user, out_sim, out_common, out_ls, F,
                               h_stats);
}
}

template <bool LS>
static int peer_rows_run(void *stream, int64_t n_query, const int32_t *query_user, int64_t n_q_users, const int64_t *q_ptr, const int32_t *q_item,
                         const double *q_rating, int32_t flags, int32_t n_top, int32_t cap, int32_t min_common, int64_t n_users, int32_t n_items,
                         const double *centre, const int64_t *hd_ptr, const int32_t *hd_user, const double *hd_x, const double *nrm,
                         int64_t max_records, int32_t *out_cnt, int32_t *out_user, double *out_sim, int32_t *out_common, double *out_ls,
                         const xmap_rec_filter *F, int64_t *h_stats) {
    // the host checks: before any device work
    XM_ARG(n_top >= 1 && n_top <= AU_MAX_TOP);
    XM_ARG(cap >= 1);
    XM_ARG(min_common >= 1);
    XM_ARG((flags & ~(XMAP_PEERS_SAME | XMAP_PEERS_KEEP_SELF)) == 0);
    XM_ARG(n_query >= 0 && n_query <= (1ll << 28) && n_q_users >= 0 && n_users >= 0 && n_users < 2147483647ll && n_items >= 0 &&
           max_records >= 0);
    XM_ARG(n_query == 0 || (query_user && q_ptr && hd_ptr && out_cnt && out_user && out_sim && out_common));
    XM_ARG(n_query == 0 || n_users == 0 || n_items == 0 || (q_item && q_rating && hd_user && hd_x && nrm));
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    if (h_stats) for (int k = 0; k < 6; k++) h_stats[k] = 0;
    bool filt = false;
    double min_score = 0.0;
    int rc = rf_prepare(st, n_query, F, &filt, &min_score);     // a NaN floor; ex_ptr, on the device
    if (rc) return rc;
    if (n_query == 0) return XMAP_OK;
    const unsigned int *allow = filt ? (const unsigned int *)F->allow : nullptr;
    const long long *ex_ptr = filt ? (const long long *)F->ex_ptr : nullptr;
    const int *ex_id = filt ? F->ex_id : nullptr;
    const int I = n_items;
    const size_t nq1 = (size_t)n_query + 1;
    // ---- rows per query, records per row (the outputs are first written once the row count has passed)
    int *qlen = nullptr;
    long long *qrow_off = nullptr;
    int64_t n_qrows = 0;
    XM_HIP(xm_malloc_async((void **)&qlen, sizeof(int) * (size_t)n_query, st));
    XM_HIP(xm_malloc_async((void **)&qrow_off, sizeof(long long) * nq1, st));
    k_pr_qlen<<<dim3(blocks_for(n_query, 256)), dim3(256), 0, st>>>(n_query, query_user, n_q_users, (const long long *)q_ptr, qlen);
    XM_LAUNCH_CHECK();
    if ((rc = xmap_exclusive_scan_i32_to_i64(st, qlen, (int64_t *)qrow_off, n_query, &n_qrows))) return rc;
    XM_ARG(n_qrows < 2147483647ll);
    if ((rc = pr_blank(st, n_query, n_top, out_cnt, out_user, out_sim, out_common))) return rc;
    if constexpr (LS) XM_HIP(hipMemsetAsync(out_ls, 0, sizeof(double) * (size_t)n_query * n_top, st));  // 0.0 behind the count
    if (n_qrows == 0 || n_users == 0 || I == 0) { XM_HIP(hipStreamSynchronize(st)); return XMAP_OK; }
    const size_t ne = (size_t)n_qrows;
    int *rcnt = nullptr;
    long long *rec_off = nullptr, *qrec = nullptr;
    double *qnrm = nullptr;
    XM_HIP(xm_malloc_async((void **)&rcnt, sizeof(int) * ne, st));
    XM_HIP(xm_malloc_async((void **)&rec_off, sizeof(long long) * (ne + 1), st));
    XM_HIP(xm_malloc_async((void **)&qrec, sizeof(long long) * nq1, st));
    XM_HIP(xm_malloc_async((void **)&qnrm, sizeof(double) * (size_t)n_query, st));
    rc = for_pair_ranges(n_qrows, 4, [&](long long base, long long end, dim3 grid) {
        k_pr_count<<<grid, dim3(256), 0, st>>>(base, end, n_query, qrow_off, query_user, (const long long *)q_ptr, q_item, I,
                                               (const long long *)hd_ptr, hd_user, allow, rcnt);
    });
    if (rc) return rc;
    if ((rc = xmap_exclusive_scan_i32_to_i64(st, rcnt, (int64_t *)rec_off, n_qrows, nullptr))) return rc;
    k_pr_qrec<<<dim3(blocks_for(n_query + 1, 256)), dim3(256), 0, st>>>(n_query, qrow_off, 0, rec_off, qrec);
    XM_LAUNCH_CHECK();
    if ((rc = pr_norms(st, n_query, query_user, n_q_users, I, (const long long *)q_ptr, q_item, q_rating, centre, qnrm))) return rc;
    RecordChunks C;
    C.rec.resize(nq1);
    std::vector<long long> h_row(nq1);
    XM_HIP(hipMemcpyAsync(h_row.data(), qrow_off, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(C.rec.data(), qrec, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if ((rc = pr_plan_chunks("peers", n_query, max_records, PR_MAX_RECORDS, &C))) return rc;
    unsigned long long *cnt = nullptr, h[5] = {0, 0, 0, 0, 0};
    XM_HIP(xm_malloc_async((void **)&cnt, sizeof(h), st));
    XM_HIP(hipMemsetAsync(cnt, 0, sizeof(h), st));
    if (C.n_max > 0) {
        const int user_bits = bits_for(n_users);
        const size_t nm = (size_t)C.n_max;
        RunTables T;
        int *r_status = nullptr, *r_common = nullptr;
        double *tv = nullptr, *r_sim = nullptr, *tb = nullptr, *r_dot = nullptr;
        if ((rc = pr_alloc_runs(st, C.n_max, C.nq_max, user_bits, true, &T))) return rc;
        XM_HIP(xm_malloc_async((void **)&tv, sizeof(double) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_status, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_common, sizeof(int) * nm, st));
        XM_HIP(xm_malloc_async((void **)&r_sim, sizeof(double) * nm, st));
        if constexpr (LS) {
            XM_HIP(xm_malloc_async((void **)&tb, sizeof(double) * nm, st));
            XM_HIP(xm_malloc_async((void **)&r_dot, sizeof(double) * nm, st));
        }
        const int same = (flags & XMAP_PEERS_SAME) ? 1 : 0, keep_self = (flags & XMAP_PEERS_KEEP_SELF) ? 1 : 0;
        rc = pr_each_chunk(C, [&](long long q0, long long q1, long long n) {
            const long long nq = q1 - q0;
            const unsigned nb = blocks_for(n, 256);
            int rc = XMAP_OK;
            if (allow) {
                rc = for_pair_ranges(h_row[q1] - h_row[q0], 4, [&](long long base, long long end, dim3 grid) {      // rows [base, end) of the chunk
                    k_pr_expand_masked<LS><<<grid, dim3(256), 0, st>>>(C.rec[q0], h_row[q0] + base, h_row[q0] + end, q0, q1, qrow_off, rec_off,
                                                                   query_user, (const long long *)q_ptr, q_item, q_rating, centre, I,
                                                                   (const long long *)hd_ptr, hd_user, hd_x, allow, user_bits, T.keys, T.vals, tv, tb);
                });
                if (rc) return rc;
            } else
                k_pr_expand<LS><<<dim3(nb), dim3(256), 0, st>>>(n, C.rec[q0], h_row[q0], h_row[q1], q0, q1, qrow_off, rec_off, query_user,
                                                            (const long long *)q_ptr, q_item, q_rating, centre, (const long long *)hd_ptr,
                                                            hd_user, hd_x, user_bits, T.keys, T.vals, tv, tb);
            XM_LAUNCH_CHECK();
            if ((rc = pr_run_tables(st, T, n, nq, user_bits))) return rc;
            k_pr_reduce<LS><<<dim3(nb < 4096u ? nb : 4096u), dim3(256), 0, st>>>(n, T.keys, T.vals, tv, tb, r_dot, T.run_idx, T.run_start, user_bits, q0,
                                                                            query_user, same, keep_self, ex_ptr, ex_id, min_common, cap, min_score,
                                                                            qnrm, nrm, r_status, r_sim, r_common, cnt);
            XM_LAUNCH_CHECK();
            rc = pr_select(st, T, nq, q0, n_top, user_bits, r_status, r_sim, r_common, out_cnt, out_user, out_sim, out_common, cnt);
            if constexpr (LS) {
                if (rc) return rc;
                rc = for_pair_ranges(nq * n_top, 4, [&](long long base, long long end, dim3 grid) {
                    k_pr_ls<<<grid, dim3(256), 0, st>>>(base, end, q0, n_top, T.first, T.keys, T.vals, tv, tb, T.run_start, user_bits, r_dot, cap,
                                                        qnrm, nrm, out_cnt, out_user, out_sim, out_ls);
                });
            }
            return rc;
        });
        if (rc) return rc;
    }
    XM_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = (int64_t)h[3]; h_stats[1] = (int64_t)h[0]; h_stats[2] = (int64_t)h[1]; h_stats[3] = (int64_t)h[2];
        h_stats[4] = (int64_t)h[4]; h_stats[5] = C.rec[(size_t)n_query];
    }
    return XMAP_OK;
}
