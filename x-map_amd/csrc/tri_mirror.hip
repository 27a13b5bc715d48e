// tri_mirror.hip -- stage A, "tri" formulation (tri.h): the half COO of the pair kernels becomes the CSR, both directions
// of every kept pair.
//   k_scatter       : round 2 (xmap_sim2_scatter: the user-sharded step, cross-checks) -- atomic row cursors
//   k_cbs_hist / k_cb_scan / k_cbs_scatter / k_cb_count : mirror_counts -- occurrences of every item in a column with no
//                     atomic per entry (xmap_sim3_mircount; the layout's raters per item)
//   k_coo_chunks, CooLoaderT, MirFin, k_mir_tiles : round 3 (xmap_sim3_mirror) -- row = [own | mirrored]: the own half
//                     written in runs from the COO, the mirrored half routed by the tile sort keyed by the heavier item
//   k_ts_plan / k_ts_chunks, ts_geometry, ts_prepare : the host side of the tile sort (tilesort.h), shared with the layout
#include "tri.h"

namespace xmap {

// Mirror the half COO into the CSR.  Records of one unit are contiguous and share the lighter item i, so the
// i-side cursor is bumped once per run of equal i inside a wave and those writes are coalesced; the j-side
// (heavier item) writes are scattered.
// SC_U groups of 64 COO slots per wave, their loads, cursor atomics and row-pointer gathers issued together (a slot is a
// chain of four dependent round trips: coo_i -> the rest of the record -> cursors / row pointers -> writes): 2.65 -> 2.53 ms.
// Neither the latency nor the cursor atomics bound the kernel (removing the j-side atomic altogether: 2.3 ms); what is
// left is its traffic, 7.2 GB for 1.7 GB of records (four partial-sector writes per mirrored entry).
constexpr int SC_U = 4;
__global__ __launch_bounds__(256) void k_scatter(long long n, const int *coo_i, const int *coo_j, const double *coo_sim,
                                                 const int *coo_mutu, const int *coo_nij, const double *coo_aux,
                                                 const long long *row_ptr, int *fill, int *col, double *sim, int *mutu,
                                                 int *nij, double *aux) {
    const int lane = lane_id();
    const long long r0 = ((long long)blockIdx.x * (blockDim.x >> 6) + uniform((int)(threadIdx.x >> 6))) * (64 * SC_U) + lane;
    int i[SC_U], j[SC_U], m[SC_U], nn[SC_U];
    double s[SC_U], x[SC_U];
    bool valid[SC_U];
#pragma unroll
    for (int u = 0; u < SC_U; u++) {
        const long long r = r0 + 64 * u;
        i[u] = (r < n) ? coo_i[r] : -1;
    }
#pragma unroll
    for (int u = 0; u < SC_U; u++) {
        const long long r = r0 + 64 * u;
        valid[u] = i[u] >= 0;
        j[u] = 0; m[u] = 0; nn[u] = 0; s[u] = 0.0; x[u] = 0.0;
        if (valid[u]) {
            j[u] = coo_j[r]; s[u] = coo_sim[r]; m[u] = coo_mutu[r]; nn[u] = coo_nij[r];
            if (coo_aux) x[u] = coo_aux[r];
        } else {
            i[u] = -1 - lane;   // inactive lanes: unique fake rows
        }
    }
    int base[SC_U], lead[SC_U], bj[SC_U];
    long long rpi[SC_U], rpj[SC_U];
#pragma unroll
    for (int u = 0; u < SC_U; u++) {
        const int prev = __shfl_up(i[u], 1, 64);
        const bool leader = (lane == 0) || (prev != i[u]);
        const unsigned long long lm = __ballot(leader);
        const unsigned long long below = lm & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
        lead[u] = 63 - __clzll((long long)below);
        const unsigned long long above = (lane == 63) ? 0ull : (lm >> (lane + 1));
        // run length as seen by the leader: distance to the next leader
        const int next = above ? lane + 1 + (__ffsll((long long)above) - 1) : 64;
        base[u] = 0; bj[u] = 0; rpi[u] = 0; rpj[u] = 0;
        if (leader && valid[u]) base[u] = atomicAdd(&fill[i[u]], next - lane);
        if (valid[u]) {
            rpi[u] = row_ptr[i[u]];
            if (j[u] != i[u]) {   // (a row paired with itself -- RecommenderSim -- is one entry)
                bj[u] = atomicAdd(&fill[j[u]], 1);
                rpj[u] = row_ptr[j[u]];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < SC_U; u++) {
        const int bs = __shfl(base[u], lead[u], 64);
        if (valid[u]) {
            const long long a = rpi[u] + bs + (lane - lead[u]);
            col[a] = j[u]; sim[a] = s[u]; mutu[a] = m[u]; nij[a] = nn[u];
            if (aux) aux[a] = x[u];
            if (j[u] != i[u]) {
                const long long b = rpj[u] + bj[u];
                col[b] = i[u]; sim[b] = s[u]; mutu[b] = m[u]; nij[b] = nn[u];
                if (aux) aux[b] = x[u];
            }
        }
    }
}

// The same counts for large inputs without a global atomic per rating (k_count3 issues ~0.9 per rating whatever its LDS cache
// catches: a chunk of 8192 ratings holds ~7000 different items; 9.7e6 device-scope atomics are 0.37 ms at BASELINE configs[1]).
// The item column is first partitioned into <= 1024 buckets of 2^sh consecutive items -- bucket histogram, scan, scatter with
// one reservation per (workgroup, bucket) -- and then counted slice by slice of the partitioned column in an LDS window of
// CB_WIN items anchored at the slice's first bucket: a slice of 8192 entries lies in one or two buckets, so its counts leave
// as one atomic per item it holds (~3e6 atomics in all, three coalesced passes over 39 MB).
constexpr int CB_MAX = 1024;          // buckets
constexpr int CB_CHUNK = 8192;        // entries per workgroup of the histogram / scatter / count passes
constexpr int CB_WIN = 8192;          // items of the count pass's LDS window
constexpr int CB_SPB = 4;             // segments (chunks) per workgroup
constexpr int CB_T = 1024;            // threads per workgroup of the three passes

// exclusive scan of the bucket counts (one workgroup of CB_MAX threads); clears the scatter cursors
__global__ __launch_bounds__(CB_MAX) void k_cb_scan(const unsigned *bcnt, long long *bptr, unsigned *bcur) {
    __shared__ long long ws[CB_MAX / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long c = bcnt[t];
    long long inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const long long o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    long long base = 0;
    for (int x = 0; x < w; x++) base += ws[x];
    bptr[t] = base + inc - c;
    if (t == CB_MAX - 1) bptr[CB_MAX] = base + inc;
    bcur[t] = 0u;
}

__global__ __launch_bounds__(CB_T) void k_cb_count(long long nnz, const int *part, int sh, const long long *bptr, int n_items, int *cnt) {
    __shared__ unsigned win[CB_WIN];
    __shared__ int s_b;
    if (nnz < 0) nnz = bptr[CB_MAX];       // (the partitioned column's length is only known on the device)
    const long long p0 = (long long)blockIdx.x * (CB_CHUNK * CB_SPB);
    if (p0 >= nnz) return;
    if (threadIdx.x == 0) {       // the bucket that holds position p0: the last b with bptr[b] <= p0
        int lo = 0, hi = CB_MAX;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (bptr[mid] <= p0) lo = mid; else hi = mid; }
        s_b = lo;
    }
    for (int t = threadIdx.x; t < CB_WIN; t += CB_T) win[t] = 0u;
    __syncthreads();
    const int item0 = s_b << sh;
#pragma unroll 4
    for (int q = threadIdx.x; q < CB_CHUNK * CB_SPB; q += CB_T) {
        const long long p = p0 + q;
        if (p >= nnz) break;
        const int it = part[p];
        const unsigned d = (unsigned)(it - item0);
        if (d < (unsigned)CB_WIN) atomicAdd(&win[d], 1u); else atomicAdd(&cnt[it], 1);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < CB_WIN; t += CB_T)
        if (win[t] && item0 + t < n_items) atomicAdd(&cnt[item0 + t], (int)win[t]);
}

// The same three passes over the partner column of the half COO (shard s = entries [s shard_cap, s shard_cap + cur[s])): the
// mirrored row counts.  Round 2 / 3 counted them with one device-scope atomic per kept pair inside the pair kernels
// (2.65e7 per pass at BASELINE configs[1], replicas for the heavy partners): taken out, the class launches are 31 % shorter
// (2.77 -> 1.91 ms summed; profiles/r03e_pair_mirsep.txt) -- the atomics, not the walk, were what the kernels waited for.
// SELF: an entry may pair a row with itself (RecommenderSim) and then has no mirrored entry.
// A workgroup of 1024 threads takes CB_SPB segments (a segment = chunk c of range r, listed chunk-major: with a sharded COO
// consecutive segments are the same chunk of consecutive shards, each a quarter full) into ONE LDS histogram: the global
// atomics of these passes are one per (workgroup, bucket), so the more entries a workgroup holds the fewer there are.
template <bool SELF>
__global__ __launch_bounds__(CB_T) void k_cbs_hist(long long range_cap, int n_ranges, const unsigned long long *cur, const int *coo_i,
                                                   const int *coo_j, int sh, unsigned *bcnt) {
    __shared__ unsigned h[CB_MAX];
    for (int t = threadIdx.x; t < CB_MAX; t += CB_T) h[t] = 0u;
    __syncthreads();
    const long long cpr = (range_cap + CB_CHUNK - 1) / CB_CHUNK;        // chunks per range
#pragma unroll
    for (int sg = 0; sg < CB_SPB; sg++) {
        const long long g = (long long)blockIdx.x * CB_SPB + sg;
        const long long c = g / n_ranges;
        const int r = (int)(g - c * n_ranges);
        if (c >= cpr) break;
        const long long n = (cur && (long long)cur[r] < range_cap) ? (long long)cur[r] : range_cap;       // (no cursors: all valid)
        const long long b = (long long)r * range_cap;
#pragma unroll
        for (int q = 0; q < CB_CHUNK / CB_T; q++) {
            const long long e = c * CB_CHUNK + q * CB_T + threadIdx.x;
            if (e < n) {
                const int j = coo_j[b + e];
                if (!SELF || j != coo_i[b + e]) atomicAdd(&h[j >> sh], 1u);
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < CB_MAX; t += CB_T)
        if (h[t]) atomicAdd(&bcnt[t], h[t]);
}

// The workgroup's entries are staged in LDS in bucket order and leave as runs (consecutive lanes write consecutive words
// of a bucket's range): written straight from the registers every lane hits another bucket, a 4-byte transaction each
// (0.25 ms for the 2.65e7 partners of a pass against 0.06 ms for the histogram pass over the same data).
template <bool SELF>
__global__ __launch_bounds__(CB_T) void k_cbs_scatter(long long range_cap, int n_ranges, const unsigned long long *cur, const int *coo_i,
                                                      const int *coo_j, int sh, const long long *bptr, unsigned *bcur, int *out) {
    static_assert(CB_T == CB_MAX, "one thread per bucket in the scan");
    __shared__ unsigned h[CB_MAX], off[CB_MAX + 1], wsum[CB_T / 64];
    __shared__ long long base[CB_MAX];
    __shared__ int stage[CB_CHUNK * CB_SPB];
    const int tid = threadIdx.x;
    h[tid] = 0u;
    __syncthreads();
    constexpr int EPT = CB_CHUNK / CB_T;
    const long long cpr = (range_cap + CB_CHUNK - 1) / CB_CHUNK;
    int it[CB_SPB][EPT];
    unsigned rk[CB_SPB][EPT];
#pragma unroll
    for (int sg = 0; sg < CB_SPB; sg++) {
        const long long g = (long long)blockIdx.x * CB_SPB + sg;
        const long long c = g / n_ranges;
        const int r = (int)(g - c * n_ranges);
        const long long n = (c < cpr) ? ((cur && (long long)cur[r] < range_cap) ? (long long)cur[r] : range_cap) : 0;
        const long long b = (long long)r * range_cap;
#pragma unroll
        for (int q = 0; q < EPT; q++) {
            const long long e = c * CB_CHUNK + q * CB_T + tid;
            it[sg][q] = -1;
            if (e < n) {
                const int j = coo_j[b + e];
                if (!SELF || j != coo_i[b + e]) it[sg][q] = j;
            }
        }
    }
#pragma unroll
    for (int sg = 0; sg < CB_SPB; sg++)
#pragma unroll
        for (int q = 0; q < EPT; q++) rk[sg][q] = it[sg][q] >= 0 ? atomicAdd(&h[it[sg][q] >> sh], 1u) : 0u;
    __syncthreads();
    {   // exclusive scan of the bucket counts (one bucket per thread), and the workgroup's place in every bucket's range
        const unsigned c = h[tid];
        const int lane = tid & 63, w = tid >> 6;
        unsigned inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        unsigned bs = 0;
        for (int x = 0; x < w; x++) bs += wsum[x];
        off[tid] = bs + inc - c;
        if (tid == CB_T - 1) off[CB_MAX] = bs + inc;
        if (c) base[tid] = bptr[tid] + (long long)atomicAdd(&bcur[tid], c);
    }
    __syncthreads();
#pragma unroll
    for (int sg = 0; sg < CB_SPB; sg++)
#pragma unroll
        for (int q = 0; q < EPT; q++)
            if (it[sg][q] >= 0) stage[off[it[sg][q] >> sh] + rk[sg][q]] = it[sg][q];
    __syncthreads();
    const int total = (int)off[CB_MAX];
    for (int x = tid; x < total; x += CB_T) {
        const int v = stage[x];
        const int bk = v >> sh;
        out[base[bk] + (x - (int)off[bk])] = v;
    }
}

// ---- the mirror (round 3): own half written in runs, mirrored half through the tile sort --------------------------------------
// Row i of the CSR = [the pairs row i computed itself (own[i]) | the pairs computed in lighter rows (mir[i])]; the row totals
// own + mir are added up inside the scan that makes row_ptr (xmap_exclusive_scan2_i32_to_i64).

// level-A loader of the mirror: the half COO (SoA, cut into shards that are filled from their start) as 24-byte records
// keyed by the heavier item; its chunks are listed from the shard cursors (k_coo_chunks), so every slot of a chunk is a
// record.  The same workgroup writes the OWN half of its chunk (extra): the records of one unit are contiguous in the
// COO and share the lighter item i -- one cursor bump per run, coalesced writes, the chunk still in the caches.
// AUX: a sixth COO column travels along (RecommenderSim: the pair's local sensitivity; 32-byte records), and a row may pair
// with itself -- such a record has an own entry and no mirrored one (k_ts_bin does not route it)
template <bool AUX, bool SHARE>      // SHARE: only the rows [row_lo, row_hi) are built
struct CooLoaderT {
    static constexpr int RW = AUX ? 4 : 3;
    const int *__restrict__ coo_i; const int *__restrict__ coo_j; const double *__restrict__ coo_sim;
    const int *__restrict__ coo_mutu; const int *__restrict__ coo_nij; const double *__restrict__ coo_aux;
    const longlong2 *chunks; const unsigned *n_chunks;
    const long long *row_ptr; int *fill; int *col; double *sim; int *mutu; int *nij; double *aux;
    int row_lo, row_hi;       // the rows this call builds (an item-sharded rank: its share; the counts outside it are zero)
    __device__ __forceinline__ bool chunk(long long, long long &i0, long long &i1) const {
        if (blockIdx.x >= *n_chunks) return false;
        const longlong2 c = chunks[blockIdx.x];
        i0 = c.x; i1 = c.x + c.y;
        return true;
    }
    __device__ __forceinline__ void load(long long idx, unsigned long long (&w)[RW]) const {
        w[0] = (unsigned long long)(unsigned)coo_j[idx] | ((unsigned long long)(unsigned)coo_i[idx] << 32);
        w[1] = (unsigned long long)__double_as_longlong(coo_sim[idx]);
        w[2] = (unsigned long long)(unsigned)coo_mutu[idx] | ((unsigned long long)(unsigned)coo_nij[idx] << 32);
        if (AUX) w[RW - 1] = (unsigned long long)__double_as_longlong(coo_aux[idx]);
    }
    __device__ __forceinline__ bool keep(const unsigned long long (&w)[RW]) const {
        const int j = (int)(unsigned)w[0];
        return (!AUX || j != (int)(w[0] >> 32)) && (!SHARE || (j >= row_lo && j < row_hi));
    }
    // own half of the chunk: for a fixed r the lanes of a wave hold consecutive COO slots
    __device__ __forceinline__ void extra(long long, const unsigned long long (&w)[ts::Chunk<RW>::EPT][RW],
                                          const bool (&on)[ts::Chunk<RW>::EPT]) const {
        constexpr int E = ts::Chunk<RW>::EPT;
        const int lane = lane_id();
        int lead[E], base[E];
        long long rp[E];
#pragma unroll
        for (int r = 0; r < E; r++) {
            const int iw = (int)(w[r][0] >> 32);
            const bool mine = on[r] && (!SHARE || (iw >= row_lo && iw < row_hi));
            const int iu = mine ? iw : -1 - lane;                           // inactive lanes: unique fake rows
            const int prev = __shfl_up(iu, 1, 64);
            const bool leader = (lane == 0) || (prev != iu);
            const unsigned long long lm = __ballot(leader);
            const unsigned long long below = lm & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
            lead[r] = 63 - __clzll((long long)below);
            const unsigned long long above = (lane == 63) ? 0ull : (lm >> (lane + 1));
            const int next = above ? lane + 1 + (__ffsll((long long)above) - 1) : 64;
            base[r] = 0; rp[r] = -1;
            if (leader && mine) base[r] = atomicAdd(&fill[iu], next - lane);
            if (mine) rp[r] = row_ptr[iu];
        }
#pragma unroll
        for (int r = 0; r < E; r++) {
            const int bs = __shfl(base[r], lead[r], 64);
            if (rp[r] >= 0) {
                const long long a = rp[r] + bs + (lane - lead[r]);
                col[a] = (int)(unsigned)w[r][0]; sim[a] = __longlong_as_double((long long)w[r][1]);
                mutu[a] = (int)(unsigned)w[r][2]; nij[a] = (int)(w[r][2] >> 32);
                if (AUX) aux[a] = __longlong_as_double((long long)w[r][RW - 1]);
            }
        }
    }
};

// chunks of CH records of the COO's shards: shard s holds its records in slots [s shard_cap, s shard_cap + fill[s])
// (cur == NULL: one range of n_fill records)
__global__ __launch_bounds__(256) void k_coo_chunks(int n_shards, long long shard_cap, const unsigned long long *cur, long long n_fill,
                                                    longlong2 *chunks, unsigned *n_chunks, long long cap) {
    constexpr int CH = ts::Chunk<3>::CH;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_shards) return;
    long long f = cur ? (long long)cur[s] : n_fill;
    if (f > shard_cap) f = shard_cap;
    const int nch = (int)((f + CH - 1) / CH);
    if (nch == 0) return;
    const unsigned base = atomicAdd(n_chunks, (unsigned)nch);
    for (int x = 0; x < nch; x++)
        if ((long long)base + x < cap) {
            longlong2 c;
            c.x = (long long)s * shard_cap + (long long)x * CH;
            c.y = min((long long)CH, f - (long long)x * CH);
            chunks[base + x] = c;
        }
}

// level C of the mirror: the small keys of a tile, laid out as CSR columns in LDS, leave as whole row segments
template <bool AUX>
__global__ __launch_bounds__(ts::CT) void k_mir_tiles(ts::Geo G, const unsigned long long *bufB, const long long *row_ptr,
                                                      const int *own, int *col, double *sim, int *mutu, int *nij, double *aux) {
    constexpr int RW = AUX ? 4 : 3;
    constexpr int CAPX = AUX ? 2048 : ts::CAP;      // (with the sixth column: 68 KB of LDS, two workgroups per CU still)
    __shared__ unsigned cur[ts::NK_MAX], kst[ts::NK_MAX];
    __shared__ long long gsh[ts::NK_MAX];
    __shared__ double lsim[CAPX];
    __shared__ double laux[AUX ? CAPX : 1];
    __shared__ int lcol[CAPX], lmutu[CAPX], lnij[CAPX];
    __shared__ unsigned short lkk[CAPX];
    const ts::TileHead h = ts::tile_head(G, blockIdx.x);
    if (h.nk <= 0 || h.n <= 0) return;
    for (int x = threadIdx.x; x < h.nk; x += ts::CT) {
        const int k = h.k0 + x;
        cur[x] = 0u;
        kst[x] = (unsigned)(G.ptr[k] - h.pos0);
        gsh[x] = row_ptr[k] + own[k] - G.ptr[k];        // mirrored position -> CSR position of key k
    }
    __syncthreads();
    const bool in_lds = h.n <= CAPX;
    constexpr int UN = 4;
    for (int base = 0; base < h.n; base += ts::CT * UN) {
        unsigned long long w[UN][RW];
        bool on[UN];
#pragma unroll
        for (int t = 0; t < UN; t++) {
            const int idx = base + t * ts::CT + threadIdx.x;
            on[t] = idx < h.n;
            const size_t o = (size_t)(h.pos0 + (on[t] ? idx : 0)) * RW;
#pragma unroll
            for (int x = 0; x < RW; x++) w[t][x] = bufB[o + x];
        }
#pragma unroll
        for (int t = 0; t < UN; t++) {
            if (!on[t]) continue;
            const int kk = (int)((unsigned)w[t][0]) - h.k0;
            const unsigned q = kst[kk] + atomicAdd(&cur[kk], 1u);
            const int ci = (int)(w[t][0] >> 32), cm = (int)(unsigned)w[t][2], cn = (int)(w[t][2] >> 32);
            const double cs = __longlong_as_double((long long)w[t][1]);
            const double ca = AUX ? __longlong_as_double((long long)w[t][RW - 1]) : 0.0;
            if (in_lds) {
                lcol[q] = ci; lsim[q] = cs; lmutu[q] = cm; lnij[q] = cn; lkk[q] = (unsigned short)kk;
                if (AUX) laux[q] = ca;
            } else {
                const long long P = h.pos0 + q + gsh[kk];
                col[P] = ci; sim[P] = cs; mutu[P] = cm; nij[P] = cn;
                if (AUX) aux[P] = ca;
            }
        }
    }
    if (!in_lds) return;
    __syncthreads();
    for (int q = threadIdx.x; q < h.n; q += ts::CT) {
        const long long P = h.pos0 + q + gsh[lkk[q]];
        col[P] = lcol[q]; sim[P] = lsim[q]; mutu[P] = lmutu[q]; nij[P] = lnij[q];
        if (AUX) aux[P] = laux[q];
    }
}

// the large keys' mirrored halves, written by level B (tilesort.h: the finisher): record w at position p of the sort goes to
// the CSR columns at p + row_ptr[k] + own[k] - ptr[k]
template <bool AUX>
struct MirFin {
    static constexpr int RW = AUX ? 4 : 3;
    static constexpr bool STATE = true, WSUM = false;
    const long long *__restrict__ row_ptr; const int *__restrict__ own;
    int *__restrict__ col; double *__restrict__ sim; int *__restrict__ mutu; int *__restrict__ nij; double *__restrict__ aux;
    __device__ __forceinline__ long long state(const ts::Geo &G, int k) const { return row_ptr[k] + (long long)own[k] - G.ptr[k]; }
    __device__ __forceinline__ unsigned gather(const unsigned long long (&)[RW]) const { return 0u; }
    __device__ __forceinline__ unsigned long long store(long long sh, long long p, const unsigned long long (&w)[RW], unsigned) const {
        const long long P = p + sh;
        col[P] = (int)(w[0] >> 32); sim[P] = __longlong_as_double((long long)w[1]);
        mutu[P] = (int)(unsigned)w[2]; nij[P] = (int)(w[2] >> 32);
        if (AUX) aux[P] = __longlong_as_double((long long)w[RW - 1]);
        return 0ull;
    }
    __device__ __forceinline__ void flush(int, unsigned long long) const {}
};

namespace ts {

// one thread per key: tile, tile boundaries, large keys
__global__ __launch_bounds__(256) void k_ts_plan(Geo G) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= G.K) return;
    const long long p = G.ptr[k], cnt = G.ptr[k + 1] - p;
    const int t = (int)(measure(G, k, p) >> G.ts_log);
    const bool large = cnt >= (1ll << G.ts_log);
    const int tp = k > 0 ? (int)(measure(G, k - 1, G.ptr[k - 1]) >> G.ts_log) : -1;
    for (int x = tp + 1; x <= t; x++) { G.tile_key0[x] = k; G.tile_pos0[x] = p; }
    if (k == G.K - 1)
        for (int x = t + 1; x <= G.T; x++) { G.tile_key0[x] = G.K; G.tile_pos0[x] = G.ptr[G.K]; }
    if (large) G.tile_large[t] = k;
}

// one thread per level-A bucket: its chunks of CH records for level B
__global__ __launch_bounds__(256) void k_ts_chunks(Geo G) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= G.NA) return;
    const int t0 = a << NB_LOG, t1 = min(G.T, (a + 1) << NB_LOG);
    const long long size = G.tile_pos0[t1] - G.tile_pos0[t0];
    const int nch = (int)((size + G.ch - 1) / G.ch);
    if (nch == 0) return;
    const unsigned base = atomicAdd(&G.counters[0], (unsigned)nch);
    for (int x = 0; x < nch; x++)
        if ((long long)base + x < G.clist_cap) G.clist[base + x] = make_int2(a, x);
}

}  // namespace ts

// ---- tile sort: host side (tri.h) ----
void ts_geometry(int K, long long M, int ch, ts::Geo &G) {
    G.K = K; G.M = M; G.ch = ch;
    G.ts_log = 11;
    for (;;) {
        const long long TS = 1ll << G.ts_log;
        long long kw = M / (4 * (long long)(K > 0 ? K : 1));
        const long long kw_min = TS / (ts::NK_MAX - 2) + 1;          // keys of a tile <= TS / KW + 1 <= NK_MAX
        if (kw < kw_min) kw = kw_min;
        if (kw < 4) kw = 4;
        const long long tiles = ((M + (long long)K * kw) >> G.ts_log) + 1;
        if (tiles <= (long long)ts::NA_MAX * ts::NB || G.ts_log >= 30) {
            G.KW = (int)kw;
            G.NA = (int)((tiles + ts::NB - 1) / ts::NB);
            if (G.NA < 1) G.NA = 1;
            if (G.NA > ts::NA_MAX) G.NA = ts::NA_MAX;
            G.T = G.NA * ts::NB;
            return;
        }
        G.ts_log++;
    }
}

int ts_prepare(hipStream_t st, ts::Geo &G, const long long *ptr, FillList *fills) {
    G.ptr = ptr;
    G.clist_cap = G.M / G.ch + G.NA + 1;
    XM_HIP(xm_malloc_async((void **)&G.tile_key0, sizeof(int) * ((size_t)G.T + 1), st));
    XM_HIP(xm_malloc_async((void **)&G.tile_pos0, sizeof(long long) * ((size_t)G.T + 1), st));
    XM_HIP(xm_malloc_async((void **)&G.tile_large, sizeof(int) * (size_t)G.T, st));
    // cursors and the chunk counter in one zeroed block: curA [NA], curB [2 T], counters [8 B]
    unsigned long long *z = nullptr;
    const size_t nz = (size_t)G.NA + 2 * (size_t)G.T + 1;
    XM_HIP(xm_malloc_async((void **)&z, sizeof(unsigned long long) * nz, st));
    G.curA = z; G.curB = z + G.NA; G.counters = (unsigned *)(z + G.NA + 2 * (size_t)G.T);
    XM_HIP(xm_malloc_async((void **)&G.clist, sizeof(int2) * (size_t)G.clist_cap, st));
    FillList own;
    FillList &F = fills ? *fills : own;
    F.add(z, sizeof(unsigned long long) * nz);
    F.add(G.tile_large, sizeof(int) * (size_t)G.T, 0xffffffffu);
    int rcode = fill_multi(st, F);
    if (rcode) return rcode;
    ts::k_ts_plan<<<dim3((unsigned)((G.K + 255) / 256)), dim3(256), 0, st>>>(G);
    XM_LAUNCH_CHECK();
    ts::k_ts_chunks<<<dim3((unsigned)((G.NA + 255) / 256)), dim3(256), 0, st>>>(G);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

namespace {
template <bool AUX, bool SHARE>
int mirror_levels(hipStream_t st, const ts::Geo &G, int64_t coo_cap, const int32_t *coo_i, const int32_t *coo_j, const double *coo_sim,
                  const int32_t *coo_mutu, const int32_t *coo_nij, const double *coo_aux, const longlong2 *chunks, const unsigned *n_chunks,
                  long long chunk_cap, int64_t n_pairs, const int32_t *own, const int64_t *row_ptr, int32_t *fill, void *bufA, void *bufB,
                  int32_t *col, double *sim, int32_t *mutu, int32_t *nij, double *aux, int row_lo, int row_hi) {
    constexpr int RW = AUX ? 4 : 3;
    CooLoaderT<AUX, SHARE> LA{coo_i, coo_j, coo_sim, coo_mutu, coo_nij, coo_aux, chunks, n_chunks, (const long long *)row_ptr, fill,
                              col, sim, mutu, nij, aux, row_lo, row_hi};
    ts::RecLoader<RW> LB{(const unsigned long long *)bufA};
    MirFin<AUX> FB{(const long long *)row_ptr, own, col, sim, mutu, nij, aux};
    ts::k_ts_bin<RW, false, CooLoaderT<AUX, SHARE>, ts::NoFin><<<dim3((unsigned)chunk_cap), dim3(ts::BT), 0, st>>>(
        G, LA, coo_cap, (unsigned long long *)bufA, ts::NoFin{});
    XM_LAUNCH_CHECK();
    // level B: the tiles' small parts to bufB, the large keys' records to the CSR
    ts::k_ts_bin<RW, true, ts::RecLoader<RW>, MirFin<AUX>><<<dim3((unsigned)G.clist_cap), dim3(ts::BT), 0, st>>>(
        G, LB, n_pairs, (unsigned long long *)bufB, FB);
    XM_LAUNCH_CHECK();
    k_mir_tiles<AUX><<<dim3((unsigned)G.T), dim3(ts::CT), 0, st>>>(G, (const unsigned long long *)bufB, (const long long *)row_ptr, own, col,
                                                                   sim, mutu, nij, aux);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}
}  // namespace

int mirror_counts(hipStream_t st, int n_items, long long range_cap, int n_ranges, const unsigned long long *cur, const int *coo_i,
                  const int *coo_j, bool skip_self, int *part, int *counts, FillList *fills) {
    FillList own;
    FillList &F = fills ? *fills : own;
    if (n_items <= 0 || range_cap <= 0 || n_ranges <= 0) return fill_multi(st, F);
    int sh = 0;
    while (((long long)(n_items - 1) >> sh) >= CB_MAX) sh++;
    unsigned *bcnt = nullptr, *bcur = nullptr;
    long long *bptr = nullptr;
    XM_HIP(xm_malloc_async((void **)&bcnt, sizeof(unsigned) * CB_MAX, st));
    XM_HIP(xm_malloc_async((void **)&bcur, sizeof(unsigned) * CB_MAX, st));
    XM_HIP(xm_malloc_async((void **)&bptr, sizeof(long long) * (CB_MAX + 1), st));
    F.add(bcnt, sizeof(unsigned) * CB_MAX);
    int rcode = fill_multi(st, F);
    if (rcode) return rcode;
    const long long segs = (long long)n_ranges * ((range_cap + CB_CHUNK - 1) / CB_CHUNK);
    const dim3 g((unsigned)((segs + CB_SPB - 1) / CB_SPB));
    (skip_self ? k_cbs_hist<true> : k_cbs_hist<false>)<<<g, dim3(CB_T), 0, st>>>(range_cap, n_ranges, cur, coo_i, coo_j, sh, bcnt);
    XM_LAUNCH_CHECK();
    k_cb_scan<<<dim3(1), dim3(CB_MAX), 0, st>>>(bcnt, bptr, bcur);
    XM_LAUNCH_CHECK();
    (skip_self ? k_cbs_scatter<true> : k_cbs_scatter<false>)<<<g, dim3(CB_T), 0, st>>>(range_cap, n_ranges, cur, coo_i, coo_j, sh, bptr, bcur,
                                                                                        part);
    XM_LAUNCH_CHECK();
    const long long cap = range_cap * n_ranges;
    k_cb_count<<<dim3((unsigned)((cap + (long long)CB_CHUNK * CB_SPB - 1) / ((long long)CB_CHUNK * CB_SPB))), dim3(CB_T), 0, st>>>(
        -1, part, sh, bptr, n_items, counts);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_sim2_scatter(void *stream, int32_t n_items, int64_t n_coo, const int32_t *coo_i, const int32_t *coo_j,
                      const double *coo_sim, const int32_t *coo_mutu, const int32_t *coo_nij, const double *coo_ls /*or NULL*/,
                      const int64_t *row_ptr, int32_t *fill /*[I] scratch*/, const int32_t *hid, const int32_t *hlist,
                      int32_t *col, double *sim, int32_t *mutu, int32_t *nij, double *ls /*or NULL*/) {
    XM_ARG(coo_i && coo_j && coo_sim && coo_mutu && coo_nij && row_ptr && fill && hid && hlist && col && sim && mutu && nij);
    XM_ARG((coo_ls != nullptr) == (ls != nullptr));
    hipStream_t st = (hipStream_t)stream;
    XM_HIP(hipMemsetAsync(fill, 0, sizeof(int32_t) * (size_t)(n_items > 0 ? n_items : 1), st));
    if (n_coo > 0) {
        // the kernel is bound by its partial-sector writes (PMC: 7.2 GB moved for 1.7 GB), not by the cursor atomics:
        // an LDS histogram bumping the heavy items' cursors once per workgroup was slower (2.9 vs 2.4 ms), 64
        // replicated cursors per heavy item changed nothing
        k_scatter<<<dim3((unsigned)((n_coo + 256 * SC_U - 1) / (256 * SC_U))), dim3(256), 0, st>>>(
            n_coo, coo_i, coo_j, coo_sim, coo_mutu, coo_nij, coo_ls, (const long long *)row_ptr, fill, col, sim, mutu, nij, ls);
        XM_LAUNCH_CHECK();
    }
    return XMAP_OK;
}

int xmap_sim3_mircount(void *stream, int32_t n_items, int64_t coo_cap, const int32_t *coo_i, const int32_t *coo_j,
                       const int64_t *d_shards, int64_t n_pairs, int32_t skip_self, void *scratch, int32_t *mir) {
    XM_SCOPE(stream);
    XM_ARG(coo_i && coo_j && scratch && mir && n_items >= 0 && coo_cap >= 0 && n_pairs >= 0);
    XM_ARG(d_shards ? (coo_cap >= COO_SHARDS) : (n_pairs <= coo_cap));
    hipStream_t st = (hipStream_t)stream;
    if (n_items == 0) return XMAP_OK;
    FillList F;            // the counts and the bucket counters are cleared in one launch
    F.add(mir, sizeof(int32_t) * (size_t)n_items);
    if (n_pairs == 0 || coo_cap == 0) return fill_multi(st, F);
    return mirror_counts(st, n_items, d_shards ? coo_cap / COO_SHARDS : n_pairs, d_shards ? COO_SHARDS : 1,
                         (const unsigned long long *)d_shards, coo_i, coo_j, skip_self != 0, (int *)scratch, mir, &F);
}

int xmap_sim3_mirror(void *stream, int32_t n_items, int64_t coo_cap, const int32_t *coo_i, const int32_t *coo_j,
                     const double *coo_sim, const int32_t *coo_mutu, const int32_t *coo_nij, const int64_t *d_shards, int64_t n_pairs,
                     const int32_t *own, const int32_t *mir, int32_t *tot, int64_t *row_ptr, int64_t *mptr, int32_t *fill,
                     void *bufA, void *bufB, int32_t *col, double *sim, int32_t *mutu, int32_t *nij, const double *coo_aux, double *aux,
                     int32_t row_lo, int32_t row_hi) {
    XM_SCOPE(stream);
    XM_ARG(row_lo >= 0 && row_lo <= row_hi && row_hi <= n_items);
    XM_ARG(coo_i && coo_j && coo_sim && coo_mutu && coo_nij && own && mir && tot && row_ptr && mptr && fill && bufA && bufB);
    XM_ARG(col && sim && mutu && nij && n_items >= 0 && coo_cap >= 0 && n_pairs >= 0 && n_pairs < 0x7fffffffLL);
    XM_ARG(d_shards ? (coo_cap >= COO_SHARDS) : (n_pairs <= coo_cap));
    XM_ARG((coo_aux != nullptr) == (aux != nullptr));
    hipStream_t st = (hipStream_t)stream;
    const int I = n_items;
    // row_ptr = scan of own + mir (the row totals are added up inside the scan: tot stays unused), mptr = scan of mir: one pass
    int rcode = xmap_exclusive_scan2_i32_to_i64(stream, own, mir, 1, row_ptr, mptr, I, nullptr);
    if (rcode) return rcode;
    if (n_pairs == 0 || I == 0 || coo_cap == 0) return XMAP_OK;
    ts::Geo G;
    ts_geometry(I, n_pairs, coo_aux ? ts::Chunk<4>::CH : ts::Chunk<3>::CH, G);      // (n_pairs bounds the mirrored records: a self pair has none)
    // the COO's chunks: from the shard cursors of the pair kernels, or one range of n_pairs records
    static_assert(ts::Chunk<3>::CH <= ts::Chunk<4>::CH && ts::Chunk<4>::CH % ts::Chunk<3>::CH == 0, "chunk lists by the narrow record width");
    const int n_shards = d_shards ? COO_SHARDS : 1;
    const long long shard_cap = d_shards ? coo_cap / COO_SHARDS : coo_cap;
    const long long chunk_cap = n_pairs / ts::Chunk<3>::CH + n_shards + 1;
    longlong2 *chunks = nullptr;
    unsigned *n_chunks = nullptr;
    XM_HIP(xm_malloc_async((void **)&chunks, sizeof(longlong2) * (size_t)chunk_cap, st));
    XM_HIP(xm_malloc_async((void **)&n_chunks, sizeof(unsigned), st));
    FillList F;            // the row cursors, the chunk counter and the sort's tables are cleared in one launch
    F.add(fill, sizeof(int32_t) * (size_t)I);
    F.add(n_chunks, sizeof(unsigned));
    rcode = ts_prepare(st, G, (const long long *)mptr, &F);
    if (rcode) return rcode;
    k_coo_chunks<<<dim3((unsigned)((n_shards + 255) / 256)), dim3(256), 0, st>>>(n_shards, shard_cap, (const unsigned long long *)d_shards,
                                                                                 n_pairs, chunks, n_chunks, chunk_cap);
    XM_LAUNCH_CHECK();
    const bool share = row_lo > 0 || row_hi < I;        // (four instances of the levels: sixth column or not, all rows or a share)
    auto levels = coo_aux ? (share ? mirror_levels<true, true> : mirror_levels<true, false>)
                          : (share ? mirror_levels<false, true> : mirror_levels<false, false>);
    return levels(st, G, coo_cap, coo_i, coo_j, coo_sim, coo_mutu, coo_nij, coo_aux, chunks, n_chunks, chunk_cap, n_pairs, own, row_ptr, fill,
                  bufA, bufB, col, sim, mutu, nij, aux, row_lo, row_hi);
}
}
