// tri_records.hip -- stage A, "tri" formulation (tri.h): the records a sharded step exchanges between ranks.
//   k_pack_partials / k_partial_keys / k_partial_gather / k_merge_partials : user-sharded input -- the raw half COO of a
//                     rank's users as 32-byte partial records, grouped by owner (before the exchange) or by pair key
//                     (after it), the shares of a pair added up exactly, finished and appended to a half COO
//   k_pack_pairs / k_unpack_pairs : the kept pairs of a rank as 24-byte records for the all-gather before stage B, and back
#include "tri.h"

namespace xmap {

// ---- user-sharded input ("each GPU produces partial (dot, n, mutu) for all pairs touched by its users") ------
// A partial record is 32 bytes: key = lower item index << 32 | higher index, the dot product as an exact (value, error)
// pair, n_ij | mutuality << 32.  A rank has at most one record per pair (every unordered pair belongs to one work unit).
__global__ __launch_bounds__(256) void k_pack_partials(long long n_coo, const int *coo_i, const int *coo_j, const double *coo_hi,
                                                       const double *coo_lo, const int *coo_mutu, const int *coo_nij,
                                                       unsigned long long *cursor, long long *rec) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool v = e < n_coo && coo_i[e] >= 0;
    const unsigned long long m = __ballot(v);
    if (!m) return;
    unsigned long long base = 0;
    if (lane_id() == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
    base = ((unsigned long long)(unsigned)rl32((int)(base >> 32), 0) << 32) | (unsigned)rl32((int)(base & 0xffffffffull), 0);
    if (!v) return;
    const long long p = (long long)base + __popcll(m & lanemask_lt());
    const int i = coo_i[e], j = coo_j[e];
    const int a = i < j ? i : j, b = i < j ? j : i;
    rec[p * 4 + 0] = ((long long)a << 32) | (long long)(unsigned)b;
    rec[p * 4 + 1] = __double_as_longlong(coo_hi[e]);
    rec[p * 4 + 2] = __double_as_longlong(coo_lo[e]);
    rec[p * 4 + 3] = (long long)(unsigned)coo_nij[e] | ((long long)coo_mutu[e] << 32);
}

// sort key of a record: the pair key squeezed to 2 * bits_b bits (same order), or -- n_owners > 0, before the exchange --
// the rank that owns the lower item (items [I r / n_owners, I (r + 1) / n_owners) belong to rank r)
// the kept pairs of a rank for the stage-B exchange: valid COO entries -> 24-byte records (i | j << 32, sim bits,
// mutu | n_ij << 32), and back
__global__ __launch_bounds__(256) void k_pack_pairs(long long n_coo, const int *coo_i, const int *coo_j, const double *coo_sim,
                                                    const int *coo_mutu, const int *coo_nij, unsigned long long *cursor,
                                                    long long *rec) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool v = e < n_coo && coo_i[e] >= 0;
    const unsigned long long m = __ballot(v);
    if (!m) return;
    unsigned long long base = 0;
    if (lane_id() == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
    base = ((unsigned long long)(unsigned)rl32((int)(base >> 32), 0) << 32) | (unsigned)rl32((int)(base & 0xffffffffull), 0);
    if (!v) return;
    const long long p = (long long)base + __popcll(m & lanemask_lt());
    rec[p * 3 + 0] = (long long)(unsigned)coo_i[e] | ((long long)coo_j[e] << 32);
    rec[p * 3 + 1] = __double_as_longlong(coo_sim[e]);
    rec[p * 3 + 2] = (long long)(unsigned)coo_mutu[e] | ((long long)coo_nij[e] << 32);
}

__global__ __launch_bounds__(256) void k_unpack_pairs(long long n, const long long *rec, int *coo_i, int *coo_j, double *coo_sim,
                                                      int *coo_mutu, int *coo_nij) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const long long a = rec[t * 3], c = rec[t * 3 + 2];
    coo_i[t] = (int)(a & 0xffffffffll); coo_j[t] = (int)(a >> 32);
    coo_sim[t] = __longlong_as_double(rec[t * 3 + 1]);
    coo_mutu[t] = (int)(c & 0xffffffffll); coo_nij[t] = (int)(c >> 32);
}

__global__ __launch_bounds__(256) void k_partial_keys(long long n, const long long *rec, int bits_b, int n_items, int n_owners,
                                                      unsigned long long *keys, int *vals) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const unsigned long long k = (unsigned long long)rec[t * 4];
    const long long a = (long long)(k >> 32), b = (long long)(k & 0xffffffffull);
    if (n_owners > 0) {
        long long r = a * n_owners / n_items;
        while (r + 1 < n_owners && (long long)n_items * (r + 1) / n_owners <= a) r++;
        while (r > 0 && (long long)n_items * r / n_owners > a) r--;
        keys[t] = (unsigned long long)r;
    } else {
        keys[t] = ((unsigned long long)a << bits_b) | (unsigned long long)b;
    }
    vals[t] = (int)t;
}

__global__ __launch_bounds__(256) void k_partial_gather(long long n, const long long *rec, const int *vals, long long *out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const long long s = vals[t];
    const longlong2 a = *(const longlong2 *)(rec + s * 4), b = *(const longlong2 *)(rec + s * 4 + 2);
    *(longlong2 *)(out + t * 4) = a;
    *(longlong2 *)(out + t * 4 + 2) = b;
}

// records sorted by key, equal keys in rank order: the thread at the head of a run adds the run up (the dot product
// exactly: the shares are exact (value, error) pairs), finishes the pair like finish_pair and appends it to the half COO
template <int METHOD>
__global__ __launch_bounds__(256) void k_merge_partials(long long n, const long long *rec, const double *nrm, int cap,
                                                        unsigned long long *counters /*[0] kept, [1] evaluated*/, int *coo_i,
                                                        int *coo_j, double *coo_sim, int *coo_mutu, int *coo_nij, int *rowcnt) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool head = false, keep = false;
    int i = 0, j = 0, nn = 0, mm = 0;
    double simv = 0.0;
    if (t < n) {
        const long long key = rec[t * 4];
        head = t == 0 || rec[(t - 1) * 4] != key;
        if (head) {
            double hi = 0.0, lo = 0.0;
            for (long long u = t; u < n && rec[u * 4] == key; u++) {
                const double ph = __longlong_as_double(rec[u * 4 + 1]), pl = __longlong_as_double(rec[u * 4 + 2]);
                if (METHOD == XMAP_COSINE) hi += ph;          // integer-exact
                else { dd_add(hi, lo, ph); dd_add(hi, lo, pl); }
                const unsigned long long c = (unsigned long long)rec[u * 4 + 3];
                nn += (int)(c & 0xffffffffull); mm += (int)(c >> 32);
            }
            i = (int)(key >> 32); j = (int)(key & 0xffffffffll);
            const double np = nrm[i] * nrm[j];                 // finish_pair
            const double cs = (np != 0.0) ? 1.0 * hi / np : 0.0;
            const int mn = nn < cap ? nn : cap;
            simv = 1.0 * cs * (double)mn / (double)cap;
            keep = (simv != 0.0) && (mm != 0);
        }
    }
    const unsigned long long hm = __ballot(head), km = __ballot(keep);
    if (!hm) return;
    unsigned long long base = 0;
    if (lane_id() == 0) {
        atomicAdd(&counters[1], (unsigned long long)__popcll(hm));
        if (km) base = atomicAdd(&counters[0], (unsigned long long)__popcll(km));
    }
    base = ((unsigned long long)(unsigned)rl32((int)(base >> 32), 0) << 32) | (unsigned)rl32((int)(base & 0xffffffffull), 0);
    if (!keep) return;
    const long long p = (long long)base + __popcll(km & lanemask_lt());
    coo_i[p] = i; coo_j[p] = j; coo_sim[p] = simv; coo_mutu[p] = mm; coo_nij[p] = nn;
    atomicAdd(&rowcnt[i], 1);
    atomicAdd(&rowcnt[j], 1);
}

}  // namespace xmap

using namespace xmap;

namespace {

// the kernels here append through device counters: N of them zeroed, handed to `launch`, read back into h_count (synchronises)
template <int N, typename Launch>
int with_counters(hipStream_t st, int64_t *h_count, Launch launch) {
    unsigned long long *cur = nullptr;
    XM_HIP(xm_malloc_async((void **)&cur, N * sizeof(unsigned long long), st));
    XM_HIP(hipMemsetAsync(cur, 0, N * sizeof(unsigned long long), st));
    launch(cur);
    XM_LAUNCH_CHECK();
    XM_HIP(hipMemcpyAsync(h_count, cur, N * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    XM_HIP(xm_free_async(cur, st));
    return XMAP_OK;
}

}  // namespace

extern "C" {

int xmap_sim2_pack_partials(void *stream, int64_t n_coo, const int32_t *coo_i, const int32_t *coo_j, const double *coo_hi,
                            const double *coo_lo, const int32_t *coo_mutu, const int32_t *coo_nij, int64_t *rec /*[n_coo][4]*/,
                            int64_t *h_count) {
    XM_SCOPE(stream);
    XM_ARG(coo_i && coo_j && coo_hi && coo_lo && coo_mutu && coo_nij && rec && h_count && n_coo >= 0);
    hipStream_t st = (hipStream_t)stream;
    return with_counters<1>(st, h_count, [&](unsigned long long *cur) {
        if (n_coo > 0)
            k_pack_partials<<<dim3((unsigned)((n_coo + 255) / 256)), dim3(256), 0, st>>>(n_coo, coo_i, coo_j, coo_hi, coo_lo, coo_mutu,
                                                                                         coo_nij, cur, (long long *)rec);
    });
}

int xmap_sim2_pack_pairs(void *stream, int64_t n_coo, const int32_t *coo_i, const int32_t *coo_j, const double *coo_sim,
                         const int32_t *coo_mutu, const int32_t *coo_nij, int64_t *rec /*[n_coo][3]*/, int64_t *h_count) {
    XM_SCOPE(stream);
    XM_ARG(coo_i && coo_j && coo_sim && coo_mutu && coo_nij && rec && h_count && n_coo >= 0);
    hipStream_t st = (hipStream_t)stream;
    return with_counters<1>(st, h_count, [&](unsigned long long *cur) {
        if (n_coo > 0)
            k_pack_pairs<<<dim3((unsigned)((n_coo + 255) / 256)), dim3(256), 0, st>>>(n_coo, coo_i, coo_j, coo_sim, coo_mutu, coo_nij, cur,
                                                                                      (long long *)rec);
    });
}

int xmap_sim2_unpack_pairs(void *stream, int64_t n, const int64_t *rec /*[n][3]*/, int32_t *coo_i, int32_t *coo_j, double *coo_sim,
                           int32_t *coo_mutu, int32_t *coo_nij) {
    XM_ARG(rec && coo_i && coo_j && coo_sim && coo_mutu && coo_nij && n >= 0);
    if (n > 0) {
        k_unpack_pairs<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(n, (const long long *)rec, coo_i, coo_j,
                                                                                                 coo_sim, coo_mutu, coo_nij);
        XM_LAUNCH_CHECK();
    }
    return XMAP_OK;
}

int xmap_sim2_sort_partials(void *stream, int64_t n, const int64_t *rec, int64_t *rec_sorted, int32_t n_items, int32_t n_owners) {
    XM_SCOPE(stream);
    XM_ARG(rec && rec_sorted && n >= 0 && n < 0x7fffffffLL && n_items > 0 && n_owners >= 0 && n_owners <= 65536);
    if (n == 0) return XMAP_OK;
    int bits_b = 1;
    while ((1ll << bits_b) < (long long)n_items) bits_b++;
    int bits = 2 * bits_b;
    if (n_owners > 0) { bits = 1; while ((1 << bits) < n_owners) bits++; }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *keys = nullptr;
    int *vals = nullptr;
    XM_HIP(xm_malloc_async((void **)&keys, sizeof(unsigned long long) * 2 * (size_t)n, st));
    XM_HIP(xm_malloc_async((void **)&vals, sizeof(int) * 2 * (size_t)n, st));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    k_partial_keys<<<grid, block, 0, st>>>(n, (const long long *)rec, bits_b, n_items, n_owners, keys, vals);
    XM_LAUNCH_CHECK();
    int rc = radix_sort_pairs(st, keys, vals, keys + n, vals + n, n, bits);
    if (rc) return rc;
    k_partial_gather<<<grid, block, 0, st>>>(n, (const long long *)rec, vals, (long long *)rec_sorted);
    XM_LAUNCH_CHECK();
    XM_HIP(xm_free_async(vals, st));
    XM_HIP(xm_free_async(keys, st));
    return XMAP_OK;
}

int xmap_sim2_merge_partials(void *stream, int method, int cap, int32_t n_items, int64_t n, const int64_t *rec_sorted,
                             const double *norms, int32_t *coo_i, int32_t *coo_j, double *coo_sim, int32_t *coo_mutu,
                             int32_t *coo_nij, int32_t *rowcnt, int64_t *h_counts /*[2]: kept, evaluated (unordered pairs)*/) {
    XM_SCOPE(stream);
    XM_ARG(rec_sorted && norms && coo_i && coo_j && coo_sim && coo_mutu && coo_nij && rowcnt && h_counts && n >= 0 && cap > 0);
    XM_ARG(method == XMAP_COSINE || method == XMAP_ADJUST_COSINE || method == XMAP_COSINE_EXACT);
    hipStream_t st = (hipStream_t)stream;
    XM_HIP(hipMemsetAsync(rowcnt, 0, sizeof(int32_t) * (size_t)(n_items > 0 ? n_items : 1), st));
    return with_counters<2>(st, h_counts, [&](unsigned long long *cnt) {
        if (n <= 0) return;
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        // exact cosine: the records hold the dot products as (value, error) pairs; added up exactly, over the plain norms
        const double *nrm = norms + (method == XMAP_ADJUST_COSINE ? (size_t)n_items : 0);
        (method == XMAP_COSINE ? k_merge_partials<XMAP_COSINE> : k_merge_partials<XMAP_ADJUST_COSINE>)<<<grid, block, 0, st>>>(
            n, (const long long *)rec_sorted, nrm, cap, cnt, coo_i, coo_j, coo_sim, coo_mutu, coo_nij, rowcnt);
    });
}
}
