// tilesort.h -- transposition of sparse records by key when every key's count is known in advance.
//
// Stage A transposes twice: the ratings by item (the rater records of the pair kernel) and the kept pairs by their
// heavier item (the mirrored half of item2item_simRDD; reference core/baselinerSim.py:182-183 emits both directions).
// Round 1 / 2 placed every record with a returning atomic on its key's cursor and a scattered write: both run at the
// memory system's rate of random 64-byte transactions (~1e10 / s), 4x the bytes they carry.  Here the final position
// space is known before a record moves (prefix sum of the per-key counts), so the records are routed towards it in two
// binning levels whose writes are runs of records, and placed exactly in LDS:
//
//   measure of key k   m[k] = ptr[k] + k * KW        (its first position + a weight per key, so that a tile bounds both
//                                                      the records and the keys it holds)
//   tile of key k      m[k] >> ts_log                  (T tiles, a level-A bucket = 2^NB_LOG consecutive tiles)
//   large key          count >= tile measure: always the last key of its tile, at most one per tile; its records are
//                      routed straight to its own position range at level B, which writes them in their final form
//                      (the level's finisher: they sit in LDS in final order when the chunk leaves)
//   level A / B        a workgroup bins a chunk of CH records: the records are loaded whole (coalesced) into registers,
//                      bucket histogram and ranks by LDS atomics, one returning global atomic per occupied bucket for the
//                      fragment's place in the bucket's range, the records staged in LDS in bucket order and copied out
//                      as flat words (consecutive lanes write consecutive words of a fragment); level B's large keys:
//                      a lane per record, consecutive lanes consecutive positions of the key's range
//   level C            one workgroup per tile: the small keys' records get their rank from LDS cursors, are laid out in
//                      final order in LDS and leave as whole rows
//
// Any order inside a key is a correct result (every consumer sums exactly or re-sorts), which is what makes ranks by
// atomics admissible.  No host synchronisation: the chunk list is built on the device, grids are upper bounds.
#pragma once
#include "common.h"

namespace xmap {
namespace ts {

constexpr int BT = 256;          // threads of a binning workgroup
// records per workgroup of a binning level: the chunk is staged in LDS in bucket order (16-byte records: 64 KB, 24-byte
// records: 48 KB, 32-byte records: 64 KB; two workgroups per CU either way)
template <int RW> struct Chunk { static constexpr int CH = RW == 2 ? 4096 : 2048; static constexpr int EPT = CH / BT; };
constexpr int NB_LOG = 7;
constexpr int NB = 1 << NB_LOG;   // fine tiles per level-A bucket
constexpr int NA_MAX = 256;       // level-A buckets (LDS histogram; two staged chunks of 16-byte records per CU need the rest)
constexpr int CAP = 3072;         // records of a tile's small part that are laid out in LDS (more: placed directly)
constexpr int CT = 512;           // threads of a level-C workgroup
constexpr int NK_MAX = 520;       // keys of a tile's small part (the host chooses KW so that tile measure / KW + 1 fits)

struct Geo {
    int K;                        // keys
    long long M;                  // records (= ptr[K])
    int KW, ts_log, T, NA;
    int ch;                       // records per chunk of the binning levels (Chunk<RW>::CH)
    const long long *ptr;         // [K + 1] first position of every key
    int *tile_key0;               // [T + 1] first key of a tile
    long long *tile_pos0;         // [T + 1] = ptr[tile_key0]
    int *tile_large;              // [T] the tile's large key, or -1
    unsigned long long *curA;     // [NA] fragment cursors of the level-A buckets
    unsigned long long *curB;     // [2 T] ... of the tiles' small parts, then of their large keys
    unsigned *counters;           // [0] level-B chunks listed
    int2 *clist;                  // level-B chunks (bucket, chunk)
    long long clist_cap;
};

__device__ __forceinline__ long long measure(const Geo &G, int k, long long p) { return p + (long long)k * G.KW; }

// (k_ts_plan / k_ts_chunks, which fill these tables: with their only caller, ts_prepare in tri_mirror.hip)
// exclusive scan of cnt[0 .. n) (n <= 2 * BT) into off[0 .. n], all BT threads call
__device__ __forceinline__ void block_scan_2(const unsigned *cnt, unsigned *off, int n, unsigned *wsum) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned a = (2 * tid < n) ? cnt[2 * tid] : 0u, b = (2 * tid + 1 < n) ? cnt[2 * tid + 1] : 0u;
    unsigned inc = a + b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned base = 0;
    for (int x = 0; x < w; x++) base += wsum[x];
    const unsigned ex = base + inc - (a + b);
    if (2 * tid < n) off[2 * tid] = ex;
    if (2 * tid + 1 < n) off[2 * tid + 1] = ex + a;
    if (tid == BT - 1) off[n] = base + inc;
    __syncthreads();
}

// records of RW 64-bit words, key = low 32 bits of word 0
template <int RW>
struct RecLoader {
    const unsigned long long *__restrict__ in;
    // level A: chunk c = records [c CH, (c + 1) CH)
    __device__ __forceinline__ bool chunk(long long n_in, long long &i0, long long &i1) const {
        i0 = (long long)blockIdx.x * Chunk<RW>::CH;
        i1 = min(n_in, i0 + Chunk<RW>::CH);
        return true;
    }
    __device__ __forceinline__ void load(long long idx, unsigned long long (&w)[RW]) const {
#pragma unroll
        for (int x = 0; x < RW; x++) w[x] = in[idx * RW + x];
    }
    // a record the level does not route (it still reaches extra): none here
    __device__ __forceinline__ bool keep(const unsigned long long (&)[RW]) const { return true; }
    // what else the workgroup does with its chunk (w[r] = record i0 + r BT + tid, on[r]: there is one)
    __device__ __forceinline__ void extra(long long, const unsigned long long (&)[Chunk<RW>::EPT][RW], const bool (&)[Chunk<RW>::EPT]) const {}
};

// What level B does with the records of the large keys (the finisher of k_ts_bin): they are staged in final order, so they
// leave in their final form instead of going through `out`.
//   STATE / state(G, k)   a 64-bit value per occupied large bucket, computed once by the thread that reserves its fragment
//   gather(w)             what a record's final form needs from memory: issued for FU records of a lane before any is stored
//   store(state, p, w, g) record w at position p of the sort's position space; returns its share of the key's sum (WSUM)
//   WSUM / flush(k, sum)  the sum over the workgroup's records of large key k: one call per (workgroup, occupied bucket)
// NoFin: level A, which has no large buckets.
struct NoFin {
    static constexpr bool STATE = false, WSUM = false;
    __device__ __forceinline__ long long state(const Geo &, int) const { return 0; }
    template <int RW> __device__ __forceinline__ unsigned gather(const unsigned long long (&)[RW]) const { return 0u; }
    template <int RW> __device__ __forceinline__ unsigned long long store(long long, long long, const unsigned long long (&)[RW], unsigned) const { return 0ull; }
    __device__ __forceinline__ void flush(int, unsigned long long) const {}
};
constexpr int FU = 4;             // records of a large key per lane whose gathers are in flight together

// One binning level.  LEVEL_B = false: a chunk of the loader's index space (L.chunk), buckets = level-A buckets.
// LEVEL_B = true: a listed chunk of a level-A bucket's range in the input (position space), buckets = the bucket's fine
// tiles (small part, to `out`) + their large keys (to their final place through the finisher F).
template <int RW, bool LEVEL_B, typename Loader, typename Fin>
__global__ __launch_bounds__(BT) void k_ts_bin(Geo G, Loader L, long long n_in, unsigned long long *__restrict__ out, Fin F) {
    constexpr int CH = Chunk<RW>::CH, EPT = Chunk<RW>::EPT;
    constexpr int NBK = LEVEL_B ? 2 * NB : NA_MAX;
    __shared__ unsigned hist[NBK];
    __shared__ unsigned off[NBK + 1];
    __shared__ long long gbase[NBK];
    __shared__ unsigned wsum[BT / 64];
    __shared__ __attribute__((aligned(16))) unsigned long long stage[CH * RW];
    __shared__ unsigned short sbk[CH];
    constexpr int NKB = LEVEL_B ? NB : NA_MAX;      // buckets by key: level B's large keys share their tile's
    __shared__ int bkey0[NKB], blarge[LEVEL_B ? NB : 1];
    __shared__ long long fstate[LEVEL_B && Fin::STATE ? NB : 1];             // the finisher's: per large bucket
    __shared__ unsigned long long fsum[LEVEL_B && Fin::WSUM ? NB : 1];
    const int tid = threadIdx.x;
    long long i0, i1;
    int a = 0;
    if (LEVEL_B) {
        if (blockIdx.x >= G.counters[0]) return;
        const int2 c = G.clist[blockIdx.x];
        a = c.x;
        const int t0 = a << NB_LOG, t1 = min(G.T, (a + 1) << NB_LOG);
        i0 = G.tile_pos0[t0] + (long long)c.y * CH;
        i1 = min(G.tile_pos0[t1], i0 + CH);
    } else {
        if (!L.chunk(n_in, i0, i1)) return;
    }
    const int nbk = LEVEL_B ? 2 * NB : G.NA;
    for (int b = tid; b < nbk; b += BT) hist[b] = 0u;
    if (LEVEL_B && Fin::WSUM)
        for (int b = tid; b < NB; b += BT) fsum[b] = 0ull;
    // the first key of every bucket: level A (no key reaches the buckets past NA), level B (the tiles of bucket a and
    // their large keys)
    if (LEVEL_B) {
        for (int b = tid; b < NB; b += BT) { bkey0[b] = G.tile_key0[(a << NB_LOG) + b]; blarge[b] = G.tile_large[(a << NB_LOG) + b]; }
    } else {
        for (int b = tid; b < NA_MAX; b += BT) bkey0[b] = b < G.NA ? G.tile_key0[b << NB_LOG] : 0x7fffffff;
    }
    __syncthreads();
    unsigned long long w[EPT][RW];
    bool on[EPT], rt[EPT];  // there is a record; it is routed
    unsigned br[EPT];       // bucket, then bucket << 16 | rank
#pragma unroll
    for (int r = 0; r < EPT; r++) {
        const long long idx = i0 + r * BT + tid;
        on[r] = idx < i1;
        if (on[r]) L.load(idx, w[r]);
        else {
#pragma unroll
            for (int x = 0; x < RW; x++) w[r][x] = 0ull;
        }
        rt[r] = on[r] && L.keep(w[r]);
    }
    // the bucket is monotone in the key: the last b with bkey0[b] <= key (the last of a run of equal ones: buckets
    // without keys), by bisection in LDS (a table of every key's tile was a gather, at level A over the whole key range)
#pragma unroll
    for (int r = 0; r < EPT; r++) br[r] = 0u;
#pragma unroll
    for (int d = NKB / 2; d > 0; d >>= 1)
#pragma unroll
        for (int r = 0; r < EPT; r++)
            if (bkey0[br[r] + d] <= (int)(unsigned)w[r][0]) br[r] += d;
    if (LEVEL_B) {
#pragma unroll
        for (int r = 0; r < EPT; r++)
            if (blarge[br[r]] == (int)(unsigned)w[r][0]) br[r] |= NB;
    }
#pragma unroll
    for (int r = 0; r < EPT; r++)
        if (rt[r]) br[r] = (br[r] << 16) | atomicAdd(&hist[br[r]], 1u);
    __syncthreads();
    block_scan_2(hist, off, nbk, wsum);
    for (int b = tid; b < nbk; b += BT) {
        const unsigned c = hist[b];
        if (!c) continue;
        long long start;
        unsigned long long *cur;
        if (LEVEL_B) {
            const int t = (a << NB_LOG) | (b & (NB - 1));
            if (b >= NB) { start = G.ptr[G.tile_large[t]]; cur = &G.curB[(size_t)G.T + t]; }
            else { start = G.tile_pos0[t]; cur = &G.curB[t]; }
        } else {
            start = G.tile_pos0[b << NB_LOG];
            cur = &G.curA[b];
        }
        // word 0 of the staged chunk -> its word of `out`, as if the whole chunk went where this fragment goes (a large
        // key's fragment: slot 0 -> its position, for the finisher)
        const long long pos = start + (long long)atomicAdd(cur, (unsigned long long)c) - (long long)off[b];
        if (LEVEL_B && b >= NB) {
            gbase[b] = pos;
            if (Fin::STATE) fstate[b - NB] = F.state(G, blarge[b - NB]);
        } else {
            gbase[b] = pos * RW;
        }
    }
#pragma unroll
    for (int r = 0; r < EPT; r++) {
        if (!rt[r]) continue;
        const unsigned b = br[r] >> 16, s = off[b] + (br[r] & 0xffffu);
#pragma unroll
        for (int x = 0; x < RW; x++) stage[s * RW + x] = w[r][x];
        sbk[s] = (unsigned short)b;
    }
    L.extra(i0, w, on);
    __syncthreads();
    // the staged chunk leaves as flat words, VW per lane (16 bytes where a record is a whole number of them): consecutive
    // lanes write consecutive words of a fragment, so a store instruction covers every line it touches and no line of a
    // fragment is stored twice (a lane per 24-byte record touched each of its lines with both of its stores)
    // (level B: the small parts, slots [0, off[NB]); the large keys' records are the tail of the staging area)
    constexpr int VW = RW % 2 == 0 ? 2 : 1;
    const int nw = (int)off[LEVEL_B ? NB : nbk] * RW;
#pragma unroll 4
    for (int q = tid * VW; q < nw; q += BT * VW) {
        unsigned long long *o = out + (gbase[sbk[q / RW]] + q);
#pragma unroll
        for (int x = 0; x < VW; x++) o[x] = stage[q + x];
    }
    if (!LEVEL_B) return;
    // the large keys' records in their final form: a lane per record, consecutive lanes take consecutive slots = consecutive
    // positions of a fragment, so every column store of a wave covers runs of whole lines (but for the fragment's ends).
    // No chunk without such records enters the loop or meets the barrier behind it.
    const int s0 = (int)off[NB], s1 = (int)off[2 * NB];
    for (int sw = s0 + (tid & ~63); sw < s1; sw += BT * FU) {        // (wave-uniform: the sums below run over whole waves)
        const int sb = sw + (tid & 63);
        unsigned long long v[FU][RW];
        unsigned g[FU];
        int bk[FU];
#pragma unroll
        for (int t = 0; t < FU; t++) {      // (past the end: the last record again, not stored)
            const int s = min(sb + t * BT, s1 - 1);
            bk[t] = sbk[s];
#pragma unroll
            for (int x = 0; x < RW; x++) v[t][x] = stage[s * RW + x];
        }
#pragma unroll
        for (int t = 0; t < FU; t++) g[t] = F.gather(v[t]);
#pragma unroll
        for (int t = 0; t < FU; t++) {
            if (sw + t * BT >= s1) break;
            const int s = sb + t * BT;
            unsigned long long add = 0ull;
            if (s < s1) add = F.store(Fin::STATE ? fstate[bk[t] - NB] : 0ll, gbase[bk[t]] + s, v[t], g[t]);
            if (Fin::WSUM) {
                // the lanes of a wave hold consecutive slots: one bucket as a rule, and then one LDS atomic for all of them
                if (__all(bk[t] == __builtin_amdgcn_readfirstlane(bk[t]))) {
                    add = (unsigned long long)wave_sum_ll((long long)add);
                    if (lane_id() == 0 && add) atomicAdd(&fsum[bk[t] - NB], add);
                } else if (add) {
                    atomicAdd(&fsum[bk[t] - NB], add);
                }
            }
        }
    }
    if (Fin::WSUM && s1 > s0) {
        __syncthreads();
        for (int b = tid; b < NB; b += BT)
            if (hist[NB + b]) F.flush(blarge[b], fsum[b]);
    }
}

// what a level-C workgroup knows about its tile
struct TileHead { int k0, nk, large; long long pos0; int n; };
__device__ __forceinline__ TileHead tile_head(const Geo &G, int t) {
    TileHead h;
    h.k0 = G.tile_key0[t];
    const int k1 = G.tile_key0[t + 1];
    h.large = G.tile_large[t];
    const int ks1 = h.large >= 0 ? h.large : k1;
    h.nk = ks1 - h.k0;
    h.pos0 = G.tile_pos0[t];
    const long long pos1 = h.large >= 0 ? G.ptr[h.large] : G.tile_pos0[t + 1];
    h.n = (int)(pos1 - h.pos0);
    return h;
}

}  // namespace ts
}  // namespace xmap
