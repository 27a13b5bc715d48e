// tri_pairs.hip -- stage A, "tri" formulation (tri.h): the pair kernels; the kept pairs go to a half COO (-> tri_mirror.hip)
//   k_pair_tri      : light rows, one launch per table class (on forked streams); LDS hash table sized to the row's
//                     partner bound and shared by 1 / 2 / 4 / 16 waves, rater records instead of a dependent row_ptr
//                     hop, prefix-only profile reads; appends kept pairs to a half-COO.  LS = true is the
//                     RecommenderSim variant (core/recommenderSim.py:65-133): no filter, self pairs, second walk for
//                     the leave-one-out local sensitivity
//   k_pair_pack     : the light rows of the 128- and 256-slot classes, G consecutive units per wave: 8-byte slots, the
//                     double-double sums by rank within the slot (no claim, no turn), finalised by the co-rating of rank 0
//   k_pair_heavy    : rows of H, raters in chunks (one rater per lane), DENSE LDS table over H, partial tables to HBM
//   k_heavy_merge   : double-double merge of the chunk partials (4 waves per row), finalise, append
//   k_shard_sums    : kept / evaluated pairs summed over the shard cursors, for the host's single read-back
#include <type_traits>

#include "tri.h"

namespace xmap {

constexpr uint32_t T_EMPTY = 0xFFFFFFFFu;

struct TriArgs {
    const long long *iptr;
    const RaterRec *rc;      // [nnz] rater records in CSC order
    const int2 *ub;          // [nnz] weight-sorted profiles: (item | flag, rating bits)
    const double *u_avg; const double *nrm;   // nrm: dense [I] norm of the method (norm2 | adjnorm2)
    int cap;
    // light
    const int *Q; const uint8_t *small; const int *uq_item; const int *uq_q; long long unit_lo, unit_hi;
    // heavy
    const int *hid; const int *hlist; const int *CH; const int *uc_item; const int *uc_c;
    const long long *uc_ptr; const int *C;
    double *hp_hi; double *hp_lo; int *hp_cnt; int *hp_mut;    // [heavy units][HMAX]
    // output: half COO + per-row counts
    long long shard_cap;            // COO entries per shard
    unsigned long long *shard_cur;  // [COO_SHARDS] cursors
    unsigned long long *shard_occ;  // [COO_SHARDS] unordered pairs evaluated
    int *coo_i; int *coo_j; double *coo_sim; int *coo_mutu; int *coo_nij;
    double *coo_aux;                // optional 6th column (RecommenderSim: local sensitivity)
    int *rowcnt;                    // pairs a row computed itself
    int *mircnt;                    // (host side only: NULL = the mirrored counts are added to rowcnt after the kernels)
    unsigned long long *counters;   // [2] table overflow, [3] COO overflow
    int heavy_mod, heavy_rem;       // the rows of H this call computes: item index % heavy_mod == heavy_rem (item-sharded ranks
                                    // deal the heavy rows round-robin; 1, 0: all of them)
    int raw;                        // user-sharded input: emit every pair's partial sums (dot as (value, error) in coo_sim /
                                    // coo_aux, n_ij, mutuality) unfinished and unfiltered -- xmap_sim2_merge finishes them
};

// cosine (:91-95), significance weighting (:84-89), zero filter (:198,:207) for one accumulated pair
template <int METHOD>
__device__ __forceinline__ bool finish_pair(const TriArgs &A, int i, int j, int n, int m, double dot, double &simv) {
    const double np = A.nrm[i] * A.nrm[j];
    const double cs = (np != 0.0) ? 1.0 * dot / np : 0.0;
    const int mn = n < A.cap ? n : A.cap;
    simv = 1.0 * cs * (double)mn / (double)A.cap;
    return (simv != 0.0) && (m != 0);
}

// append the kept pairs of one wave's table (callback gives slot -> pair) to the half COO (cut into COO_SHARDS segments
// with a cursor each: tri.h)
// (the mirrored row counts are not taken here any more -- one device atomic per kept pair, with HEAVY_SHARDS replicas for
// the heavy partners, was what the pair kernels waited for: xmap_sim3_mircount / mirror_counts take them from the COO)

// finalise(s, j, n, m, sim, occupied) -> keep.  Pass 1 finalises every slot once (the result is parked by `park`),
// pass 2 writes the kept ones.
template <typename Fin, typename Park, typename Get, typename Aux>
__device__ __forceinline__ void append_pairs(const TriArgs &A, int i, int s_begin, int n_slots, Fin fin, Park park, Get get,
                                             Aux aux) {
    const int lane = lane_id();
    const int shard = (blockIdx.x * (blockDim.x >> 6) + uniform((int)(threadIdx.x >> 6))) & (COO_SHARDS - 1);
    int kept = 0, occ = 0;
    for (int s0 = s_begin; s0 < n_slots; s0 += 64) {
        int j, n, m; double sv; bool o;
        bool keep = fin(s0 + lane, j, n, m, sv, o);
        park(s0 + lane, o, keep, sv);
        kept += __popcll(__ballot(keep));
        occ += __popcll(__ballot(o));
    }
    if (lane == 0 && occ) atomicAdd(&A.shard_occ[shard], (unsigned long long)occ);
    if (!kept) return;
    unsigned long long base = 0;
    if (lane == 0) {
        base = atomicAdd(&A.shard_cur[shard], (unsigned long long)kept);
        atomicAdd(&A.rowcnt[i], kept);
    }
    base = ((unsigned long long)(unsigned)rl32((int)(base >> 32), 0) << 32) | (unsigned)rl32((int)(base & 0xffffffffull), 0);
    if ((long long)(base + kept) > A.shard_cap) {
        if (lane == 0) atomicOr(&A.counters[3], 1ull);
        return;
    }
    base += (unsigned long long)shard * (unsigned long long)A.shard_cap;
    for (int s0 = s_begin; s0 < n_slots; s0 += 64) {
        int j, n, m; double sv;
        bool keep = get(s0 + lane, j, n, m, sv);
        unsigned long long km = __ballot(keep);
        if (keep) {
            long long p = (long long)base + __popcll(km & lanemask_lt());
            A.coo_i[p] = i; A.coo_j[p] = j;
            A.coo_sim[p] = sv; A.coo_mutu[p] = m; A.coo_nij[p] = n;
            if (A.coo_aux) A.coo_aux[p] = aux(s0 + lane);
        }
        base += __popcll(km);
    }
}

// sums of the shard cursors (kept pairs) and of the evaluated-pair counters -> counters[4], counters[5]: what the host reads
// after the pair kernels, in one copy with the overflow flags
__global__ __launch_bounds__(256) void k_shard_sums(const unsigned long long *shards, unsigned long long *counters) {
    unsigned long long a = 0ull, b = 0ull;
    for (int s = threadIdx.x; s < COO_SHARDS; s += 256) { a += shards[s]; b += shards[COO_SHARDS + s]; }
    a = (unsigned long long)wave_sum_ll((long long)a);
    b = (unsigned long long)wave_sum_ll((long long)b);
    if (lane_id() == 0) { atomicAdd(&counters[4], a); atomicAdd(&counters[5], b); }
}

// Light rows.  The co-ratings of a block of raters are walked as one flat list, one per lane (k_pair_tri: walk).  Lanes
// of different raters may meet on one partner: the counters use LDS atomics, the fp64 sum is either an LDS atomic add
// (cosine over ratings the host found exact: order irrelevant) or, for the double-double sum, serialised per slot
// (conflicts are rare): through a claim word inside one wave, through a lock bit in the slot's key when several waves
// share the table.

// The table size is a template parameter: rows whose partner bound is <= SMALL_BOUND (the vast majority: items
// with a handful of raters) run with 128 slots (3.5 KB of LDS, full occupancy, 8x cheaper init/finalise), rows up
// to 2 SMALL_BOUND with 256, up to MID_BOUND with 512, the others with 1024.  The units are listed class-major, one
// launch per class.  The big tables are few per CU (5 of 1024 slots fit in LDS) and their rows have the most
// raters (158 on average at BASELINE configs[1], against 6 in the smallest class): NW waves share one table there
// (4 for 1024 slots, 2 for 512), each taking every NW-th block of 64 raters, which keeps 20 waves per CU in flight
// instead of 5.
// LS (RecommenderSim, core/recommenderSim.py:90-133): nothing is filtered, a row may pair with itself (an item twice
// in one profile), and every pair also gets its leave-one-out local sensitivity, which needs the FINAL inner product
// and count of the pair: after the accumulation pass the slots are finalised in LDS and the raters are walked a
// second time, each co-rating looking its slot up and raising the slot's maximum (bit pattern of a non-negative
// double, NaN above everything: np.max propagates NaN).  (weighted, ls_key: tri.h -- the item fold-in takes the same steps.)

// Per-unit time stamps (round 3, profiles/r03c_pair_trace.txt): a unit of the smallest class lives ~14 us -- 2.0 us
// until its item / partition / rater range are read, 3.4 us until the first rater records and prefixes are in, 9.7 us
// until its (single) step of 8 raters is in the table, 4.3 us of finalisation and appends -- and holds its LDS table
// all that time; LDS capacity x unit lifetime (79 GB us over 41 MB of LDS = 1.9 ms) is what bounds the class launches.
// A field of the kernel's argument struct, read from the kernarg segment where it is used (a volatile scalar load: it stays
// at that place).  The finalisation needs seventeen pointers the walk never touches; as plain uses of A they are all loaded
// at the kernel's entry and kept -- 101 SGPRs, i.e. 7 waves per SIMD, or ~100 v_writelane / v_readlane spill moves per unit
// (a sixth of its vector instructions) when the kernel is held to 8.
// KARG reads at offsetof(TriArgs, field) from the kernarg base: correct only while the struct is the kernel's FIRST and ONLY
// parameter (k_pair_tri(TriArgs A), k_pair_heavy(TriArgs A)): keep it so.
static_assert(std::is_standard_layout<TriArgs>::value, "KARG() addresses TriArgs fields by offsetof");
#define KARG(field) (*(decltype(TriArgs::field) const volatile __attribute__((address_space(4))) *)( \
    (const char __attribute__((address_space(4))) *)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(TriArgs, field)))
template <int METHOD, int LOG_SLOTS, int NW, bool LS>
__global__ __launch_bounds__(64 * NW, (LOG_SLOTS == 7 && !LS) ? 8 : 1) void k_pair_tri(TriArgs A) {   // (128 slots: 8 waves per SIMD fit, keep the SGPRs below the limit for that)
    constexpr int SLOTS_ = 1 << LOG_SLOTS;
    constexpr bool ADJ = METHOD == XMAP_ADJUST_COSINE;
    using RT = typename std::conditional<LS, double, float>::type;      // rating type of the profile copy and the rater records
    // one slot = key 4 B (item; bit 31 = the slot's lock while several waves share the table) + counters + sum: 24 B (adjusted
    // cosine: (value, error) sum) for the rows below WIDE_MIN raters -- n_ij and the mutuality count in 16 bits each -- so six
    // 1024-slot tables fit one CU (round 2: 32 KB + 8 B each with 64-bit counters and a lock word: four)
    // (profiles hold an item once there: n_ij <= n_i < WIDE_MIN; the AlterEgo rows of LS may repeat items: 32-bit halves)
    using CM = typename std::conditional<NW == 16 || LS, unsigned long long, unsigned>::type;
    constexpr int MSH = (NW == 16 || LS) ? 32 : 16;
    constexpr CM NMASK = (CM)(((CM)1 << MSH) - 1);
    constexpr uint32_t LOCKBIT = 0x80000000u;
    __shared__ uint32_t key[SLOTS_];
    __shared__ CM cm[SLOTS_];                     // n_ij (low half) | mutuality (high half)
    __shared__ double dot[SLOTS_];
    __shared__ double dlo[ADJ ? SLOTS_ : 1];
    __shared__ unsigned short claim[ADJ && NW == 1 ? SLOTS_ : 1];   // (lane ids; NW > 1 locks the key word)
    __shared__ double s_ny[LS ? SLOTS_ : 1];              // LS: norm of the partner
    __shared__ unsigned long long s_ls[LS ? SLOTS_ : 1];  // LS: running maximum (ls_key)
    __shared__ int s_ovf;
    static_assert(!LS || ADJ, "the local-sensitivity pass keeps the similarity in dlo[]");

    const int lane = lane_id();
    const long long unit = A.unit_lo + blockIdx.x;
    if (unit >= A.unit_hi) return;
    // the unit's record in one round trip: item; (partition, first rater, end of raters, partitions of the row)
    const int i = uniform(A.uq_item[unit]);
    const int4 ud = ((const int4 *)A.uq_q)[unit];
    const int q = uniform(ud.x), p0 = uniform(ud.y), p1 = uniform(ud.z), Qi = uniform(ud.w);
    const int w = uniform((int)uniform((int)(threadIdx.x >> 6)));      // (a scalar: the block loop of the walk is a scalar loop)
    for (int s = threadIdx.x; s < SLOTS_; s += 64 * NW) {
        key[s] = T_EMPTY; cm[s] = (CM)0; dot[s] = 0.0;
        if (ADJ) dlo[s] = 0.0;
    }
    if (NW > 1) {
        if (threadIdx.x == 0) s_ovf = 0;
        __syncthreads();
    }
    const double nx = A.nrm[i];     // (for the finalisation: in flight during the walk)
    int ovf = 0;

    // walk(body): every co-rating of this unit's raters (those of hash partition q); body(act, j, jw, rj, ri, a, gei)
    // runs once per lane and 64 co-ratings.  Wave w takes every NW-th block of RB raters, one rater record per lane
    // (RB = 64 when the wave is alone or the row is very long; the rows of the shared 1024 / 512-slot tables have 158 / 33
    // raters on average: blocks of 16 deal them out evenly -- a unit lives as long as its busiest wave, and holds its table
    // that long).  The prefixes of a block are walked as ONE flat list (round 2 gave each rater 8 lanes: half of the
    // lanes idle, one dependent load per 8 entries of the longest of eight prefixes, 10-18 us per unit of which the
    // table work was a fraction -- profiles/r03c_pair_trace.txt): an inclusive scan of the prefix lengths over the lanes, then
    // lane l of round t takes co-rating 64 t + l, finds its rater by binary search over the scan (log2 RB permutes) and loads
    // its entry; all loads of WU rounds are in flight together and every lane of every round but the last is busy.
    constexpr int RB = (NW == 1 || NW == 16) ? 64 : 16;
    constexpr int WU = 2;
    // Loads of the walk: every one is unconditional (a clamped index for a lane that has nothing to load) and nothing is
    // done with a loaded value before the loads that can go out with it are out -- a load under `if (act)`, or a select on a
    // freshly prefetched record, is waited for on the spot, which had put a block's record prefetch, the user averages and the
    // two rounds' entries one round trip after the other.  The user average is read per co-rating next to the profile entry
    // (the lanes of one rater read one address), not per rater ahead of the rounds.
    struct RawRec { int e0, pw, usr; RT r; };
    auto rater = [&](int p) {
        const int pc = (lane < RB && p < p1) ? p : p0;
        RawRec o;
        if (LS) {       // fp64 ratings, user average 0 by construction
            const RaterRecWide rr = ((const RaterRecWide *)A.rc)[pc];
            o.e0 = rr.e0; o.pw = rr.pos_ge; o.r = (RT)rr.rating; o.usr = 0;
        } else {
            const RaterRec rr = A.rc[pc];
            o.e0 = rr.e0; o.pw = rr.pos_ge; o.r = (RT)rr.rating; o.usr = rr.user;
        }
        return o;
    };
    auto entry = [&](int e, int &jw_, RT &rj_) {        // one entry of a sorted profile
        if (LS) { const UbWide v = ((const UbWide *)A.ub)[e]; jw_ = v.item_ge; rj_ = (RT)v.rating; }
        else { const int2 v = A.ub[e]; jw_ = v.x; rj_ = (RT)__int_as_float(v.y); }
    };
    auto walk = [&](auto &&body) {
        int base = p0 + RB * w;
        if (base >= p1) return;
        RawRec cur = rater(base + lane);
        for (; base < p1; base += RB * NW) {
            RawRec nxt = cur;
            if (base + RB * NW < p1) nxt = rater(base + RB * NW + lane);      // this wave's next block (a scalar branch)
            const bool ok = lane < RB && base + lane < p1;
            const int e0 = cur.e0, pw = cur.pw, usr = cur.usr;
            const RT r = cur.r;
            const int len = ok ? (pw & 0x7fffffff) : 0;       // the rater's prefix: entries [e0, e0 + len) of its profile
            int end = len;
#pragma unroll
            for (int d = 1; d < RB; d <<= 1) { const int v = __shfl_up(end, d, 64); if (lane >= d) end += v; }
            const int total = rl32(end, RB - 1);
            const int start = end - len;
            for (int f0 = 0; f0 < total; f0 += 64 * WU) {
                int jw[WU]; RT rj[WU]; bool act[WU]; double ri[WU], a[WU]; unsigned gei[WU];
                int tt[WU], ee[WU], uu[WU];
#pragma unroll
                for (int u = 0; u < WU; u++) {
                    const int f = f0 + u * 64 + lane;
                    act[u] = f < total;
                    int t = 0;                                // the rater of co-rating f: #{k : end[k] <= f}
#pragma unroll
                    for (int step = RB / 2; step >= 1; step >>= 1) { const int v = __shfl(end, t + step - 1, 64); if (v <= f) t += step; }
                    const int eb = __shfl(e0, t, 64), sb = __shfl(start, t, 64), ut = __shfl(usr, t, 64);
                    tt[u] = t;
                    ee[u] = act[u] ? eb + (f - sb) : 0;
                    uu[u] = act[u] ? ut : 0;
                }
#pragma unroll
                for (int u = 0; u < WU; u++) {
                    entry(ee[u], jw[u], rj[u]);
                    a[u] = 0.0;
                    if (ADJ && !LS) a[u] = A.u_avg[uu[u]];
                }
#pragma unroll
                for (int u = 0; u < WU; u++) {
                    const int pwt = __shfl(pw, tt[u], 64);
                    ri[u] = (double)__shfl(r, tt[u], 64);
                    gei[u] = ((unsigned)pwt) >> 31;
                }
#pragma unroll
                for (int u = 0; u < WU; u++) {
                    if (u && f0 + u * 64 >= total) continue;  // (uniform)
                    const int j = jw[u] & 0x7fffffff;
                    bool ac = act[u];
                    if (ac && Qi > 1) ac = (int)__umulhi(mix32((uint32_t)j), (uint32_t)Qi) == q;
                    body(ac, j, jw[u], rj[u], ri[u], a[u], gei[u]);
                }
            }
            cur = nxt;
        }
    };

    // pass 1: accumulate n_ij, mutuality and the dot product per partner
    walk([&](bool act, int j, int jw, RT rj, double ri, double a, unsigned gei) {
        uint32_t h = 0;
        if (act) {
            h = ((uint32_t)j * 0x9E3779B1u) >> (32 - LOG_SLOTS);
            int probes = 0;
            for (;;) {
                uint32_t prev = atomicCAS(&key[h], T_EMPTY, (uint32_t)j);
                if (prev == T_EMPTY || (prev & ~LOCKBIT) == (uint32_t)j) break;
                h = (h + 1) & (SLOTS_ - 1);
                if (++probes >= SLOTS_) { act = false; ovf = 1; break; }
            }
        }
        if (act) {
            const CM inc = (CM)1 | (((((unsigned)jw) >> 31) == gei) ? ((CM)1 << MSH) : (CM)0);
            atomicAdd(&cm[h], inc);
            if (METHOD == XMAP_COSINE) atomicAdd(&dot[h], (1.0 * ri) * (double)rj);   // integer-exact
        }
        if (ADJ) {
            const double term = (ri - a) * ((double)rj - a);
            // volatile: the sums are shared between lanes (and waves); the compiler must neither forward the
            // claim / lock store to the load nor hoist the sum loads out of the loop
            // (LDS-qualified: through a generic volatile pointer these become flat_load / flat_store, which also count on
            // vmcnt -- every turn then waited for the prefix loads in flight as well)
            typedef __attribute__((address_space(3))) volatile double lds_vf64;
            typedef __attribute__((address_space(3))) volatile unsigned short lds_vu16;
            lds_vf64 *vhi = (lds_vf64 *)dot, *vlo = (lds_vf64 *)dlo;
            bool pending = act;
            if (NW == 1) {
                lds_vu16 *vclaim = (lds_vu16 *)claim;
                while (__ballot(pending)) {       // lanes that share a slot take turns
                    if (pending) vclaim[h] = (unsigned short)lane;
                    if (pending && vclaim[h] == (unsigned short)lane) {
                        double hi = vhi[h], lo = vlo[h];
                        dd_add(hi, lo, term);
                        vhi[h] = hi; vlo[h] = lo;
                        pending = false;
                    }
                }
            } else {
                while (__ballot(pending)) {       // a lock per slot (bit 31 of its key): the holder releases in the same pass
                    if (pending && !(atomicOr(&key[h], LOCKBIT) & LOCKBIT)) {
                        double hi = vhi[h], lo = vlo[h];
                        dd_add(hi, lo, term);
                        vhi[h] = hi; vlo[h] = lo;
                        __threadfence_block();
                        atomicAnd(&key[h], ~LOCKBIT);
                        pending = false;
                    }
                }
            }
        }
    });
    if (NW > 1) {
        if (ovf) s_ovf = 1;
        __syncthreads();          // all raters are in the table (and every lock bit is clear again)
        ovf = s_ovf;
    }
    if (__ballot(ovf)) {
        if (threadIdx.x == 0) atomicOr(&A.counters[2], 1ull);
        return;
    }
    if (LS) {
        // finalise the slots: an item paired with itself was met once per user holding it twice, the reference lists
        // both orders (recommenderSim.py:71-72): count and inner product double (exactly)
        const double nx = A.nrm[i];
        for (int s = threadIdx.x; s < SLOTS_; s += 64 * NW) {
            const uint32_t kj = key[s];
            if (kj == T_EMPTY) continue;
            int n = (int)(cm[s] & NMASK);
            double inner = dot[s];
            if ((int)kj == i) { n *= 2; inner *= 2.0; }
            const double ny = A.nrm[kj];
            const double np = nx * ny;
            cm[s] = (CM)(unsigned)n;
            dot[s] = inner;
            dlo[s] = weighted((np != 0.0) ? 1.0 * inner / np : 0.0, n, A.cap);   // NaN != 0: divides, like the reference
            s_ny[s] = ny;
            s_ls[s] = 0ull;
        }
        if (NW > 1) __syncthreads();
        // pass 2: leave-one-out variants (recommenderSim.py:98-116)
        walk([&](bool act, int j, int jw, RT rj, double ri, double a, unsigned gei) {
            if (!act) return;
            uint32_t h = ((uint32_t)j * 0x9E3779B1u) >> (32 - LOG_SLOTS);
            while (key[h] != (uint32_t)j) h = (h + 1) & (SLOTS_ - 1);
            const double inner = dot[h], sim = dlo[h], ny = s_ny[h];
            const int n = (int)cm[h];
            const double r0 = ri, r1 = (double)rj;
            const double rest = inner - r0 * r1;
            const double m1 = sqrt((nx * nx - r0 * r0) * (ny * ny));
            const double m2 = sqrt((nx * nx) * (ny * ny - r1 * r1));
            const double d1 = fabs(weighted((m1 != 0.0) ? 1.0 * rest / m1 : 0.0, n - 1, A.cap) - sim);
            const double d2 = fabs(weighted((m2 != 0.0) ? 1.0 * rest / m2 : 0.0, n - 1, A.cap) - sim);
            const unsigned long long k1 = ls_key(d1), k2 = ls_key(d2);
            atomicMax(&s_ls[h], k1 > k2 ? k1 : k2);
        });
        if (NW > 1) __syncthreads();
        append_pairs(A, i, w * (SLOTS_ / NW), (w + 1) * (SLOTS_ / NW),
            [&](int s, int &j, int &n, int &m, double &sv, bool &o) {
                const uint32_t kj = key[s];
                o = kj != T_EMPTY;
                if (!o) return false;
                j = (int)kj; n = (int)cm[s]; m = 0; sv = dlo[s];
                return true;
            },
            [&](int s, bool o, bool keep, double sv) {},
            [&](int s, int &j, int &n, int &m, double &sv) {
                const uint32_t kj = key[s];
                if (kj == T_EMPTY) return false;
                j = (int)kj; n = (int)cm[s]; m = 0; sv = dlo[s];
                return true;
            },
            [&](int s) { return __longlong_as_double((long long)s_ls[s]); });
        return;
    }
    // finalisation: this wave's share of the slots stays in registers (NIT rounds of 64); the norms of all partners are
    // gathered in one go (round 2: norm gather -> cursor atomic -> heavy-id gather, three dependent round trips and the slots
    // read twice from LDS), then one returning atomic on the shard cursor, then the stores.  The mirrored row counts are
    // not taken here (one device atomic per kept pair): xmap_sim2_pairs counts them from the COO afterwards (k_cbs_*)
    // (the argument fields of this part: see KARG)
    const auto k_coo_i = KARG(coo_i);
    const auto k_coo_j = KARG(coo_j);
    const auto k_coo_sim = KARG(coo_sim);
    const auto k_coo_mutu = KARG(coo_mutu);
    const auto k_coo_nij = KARG(coo_nij);
    const auto k_coo_aux = KARG(coo_aux);
    const auto k_nrm = KARG(nrm);
    const auto k_rowcnt = KARG(rowcnt);
    const auto k_shard_cur = KARG(shard_cur);
    const auto k_shard_occ = KARG(shard_occ);
    const auto k_shard_cap = KARG(shard_cap);
    const auto k_cap = KARG(cap);
    const auto k_raw = KARG(raw);
    const auto k_counters = KARG(counters);
    constexpr int NIT = SLOTS_ / NW / 64;
    const int sb0 = w * (SLOTS_ / NW);
    int fj[NIT], fn[NIT], fm[NIT];
    double fs[NIT], fy[NIT], fa[NIT];
    bool fo[NIT], fk[NIT];
#pragma unroll
    for (int t = 0; t < NIT; t++) {
        const int sl = sb0 + t * 64 + lane;
        const uint32_t kj = key[sl];
        fo[t] = kj != T_EMPTY;
        fj[t] = (int)kj;
        const CM c = cm[sl];
        fn[t] = (int)(c & NMASK); fm[t] = (int)(c >> MSH);
        fs[t] = dot[sl];
        fa[t] = (ADJ && k_raw) ? dlo[sl] : 0.0;
        fy[t] = 0.0;
        if (fo[t]) {
            if (!k_raw) fy[t] = k_nrm[kj];
        }
    }
    int kept = 0, occ = 0;
#pragma unroll
    for (int t = 0; t < NIT; t++) {
        bool keep = fo[t];
        if (keep && !k_raw) {          // cosine (:91-95), significance weighting (:84-89), zero filter (:198,:207): finish_pair
            const double np = nx * fy[t];
            const double cs = (np != 0.0) ? 1.0 * fs[t] / np : 0.0;
            const int mn = fn[t] < k_cap ? fn[t] : k_cap;
            fs[t] = 1.0 * cs * (double)mn / (double)k_cap;
            keep = (fs[t] != 0.0) && (fm[t] != 0);
        }
        fk[t] = keep;
        kept += __popcll(__ballot(keep));
        occ += __popcll(__ballot(fo[t]));
    }
    const int shard = (blockIdx.x * NW + w) & (COO_SHARDS - 1);
    if (lane == 0 && occ) atomicAdd(&k_shard_occ[shard], (unsigned long long)occ);
    if (!kept) return;
    unsigned long long cbase = 0;
    if (lane == 0) {
        cbase = atomicAdd(&k_shard_cur[shard], (unsigned long long)kept);
        atomicAdd(&k_rowcnt[i], kept);
    }
    cbase = ((unsigned long long)(unsigned)rl32((int)(cbase >> 32), 0) << 32) | (unsigned)rl32((int)(cbase & 0xffffffffull), 0);
    if ((long long)(cbase + kept) > k_shard_cap) {
        if (lane == 0) atomicOr(&k_counters[3], 1ull);
        return;
    }
    cbase += (unsigned long long)shard * (unsigned long long)k_shard_cap;
#pragma unroll
    for (int t = 0; t < NIT; t++) {
        const unsigned long long km = __ballot(fk[t]);
        if (fk[t]) {
            const long long pp = (long long)cbase + __popcll(km & lanemask_lt());
            const int j = fj[t];
            k_coo_i[pp] = i; k_coo_j[pp] = j;
            k_coo_sim[pp] = fs[t]; k_coo_mutu[pp] = fm[t]; k_coo_nij[pp] = fn[t];
            if (k_coo_aux) k_coo_aux[pp] = fa[t];
        }
        cbase += __popcll(km);
    }
}

// Packed light rows: the 128- and 256-slot classes (one partition per row by construction: plan_item files a row there only
// with q == 1).  A row of the smallest class has 6 raters and 63 co-ratings on average -- a single round of 64 lanes -- and
// k_pair_tri holds a wave and a table for five dependent round trips to do it.  Here one wave takes G consecutive units of
// its class range and computes them in ONE pass: the G unit records in one round trip, the members' raters as one list (the
// table of a co-rating is its member's region of the wave's LDS), all rounds of the flat list in flight together, one
// finalisation, one returning atomic on the shard cursor.
// The sums take no lock and no turn: the returning atomicAdd on a slot's count word gives every co-rating its RANK within
// its slot; a lane keeps (slot, rank, term) of its co-ratings in registers; after the walk a wave scan of the slot counts
// gives every slot an offset, the terms go to an LDS buffer at offset + rank, and the lane whose co-rating has rank 0 sums
// its slot with dd_add in registers (exact, hence order-independent) and finalises the pair there: it knows the partner, and
// the partner's norm has been in flight since the walk.  So the finalisation runs over the rounds of the walk (two for the
// average pack of the 128-slot class), not over the slots of G tables at half load, and in the order of the flat list,
// which is member by member.  LDS per slot: key + count word, 8 B (k_pair_tri: 26 B), + 8 B per co-rating.
// A pack the wave cannot hold that way -- more than 64 raters, or more than 64 E co-ratings (the partner bound of a row
// is min(W+, heavier items): on a small catalogue a 128-slot row may have thousands of co-ratings) -- runs its members one
// after the other through one table with the per-slot serialised sum of k_pair_tri (the same LDS bytes, laid out anew) and
// append_pairs.  Correct for any row of the class; not what the class launches spend their time in.
// E: the rounds of 64 co-ratings a wave holds in registers.  G and E per class: launch_pack.
constexpr int pack_lds(int log_slots, int g, int e) {
    return 8 * (g << log_slots) + 512 * e > (26 << log_slots) ? 8 * (g << log_slots) + 512 * e : (26 << log_slots);
}
constexpr int pack_waves(int lds) { return 160 * 1024 / lds / 4 > 8 ? 8 : 160 * 1024 / lds / 4; }    // per SIMD, as the LDS admits
template <int METHOD, int LOG_SLOTS, int G, int PACK_E>
__global__ __launch_bounds__(64, pack_waves(pack_lds(LOG_SLOTS, G, PACK_E))) void k_pair_pack(TriArgs A) {
    constexpr int S = 1 << LOG_SLOTS, GS = G * S;
    constexpr int NIT = GS / 64;            // rounds of 64 slots
    constexpr bool ADJ = METHOD == XMAP_ADJUST_COSINE;
    constexpr int CAP = 64 * PACK_E;
    static_assert(GS % 256 == 0 && GS <= 65536 && CAP <= 32768, "16-byte fills; (slot, rank) in one word");
    __shared__ __align__(16) unsigned char lds[pack_lds(LOG_SLOTS, G, PACK_E)];
    // the pack: key[GS] | count word[GS] (n_ij low half, mutuality high half: n_ij < WIDE_MIN) | terms[CAP]
    uint32_t *key = (uint32_t *)lds;
    uint32_t *cm = key + GS;
    double *terms = (double *)(cm + GS);
    // one member at a time: key[S] | count word[S] | sum[S] | error[S] | claim[S]
    uint32_t *key1 = (uint32_t *)lds;
    uint32_t *cm1 = key1 + S;
    double *dot1 = (double *)(cm1 + S);
    double *dlo1 = dot1 + S;
    unsigned short *claim1 = (unsigned short *)(dlo1 + S);

    const int lane = lane_id();
    const long long u0 = A.unit_lo + (long long)blockIdx.x * G;
    if (u0 >= A.unit_hi) return;
    const int nm = (A.unit_hi - u0 < G) ? (int)(A.unit_hi - u0) : G;     // members of this pack
    // the unit records of the pack in one round trip (lane m: member m)
    const long long um = u0 + (lane < nm ? lane : 0);
    const int it_l = A.uq_item[um];
    const int4 ud = ((const int4 *)A.uq_q)[um];
    const int nr_l = lane < nm ? ud.z - ud.y : 0;
    int im[G], pm[G], ro[G + 1];          // item, first rater, position in the pack's rater list (scalars)
    ro[0] = 0;
#pragma unroll
    for (int m = 0; m < G; m++) {
        im[m] = rl32(it_l, m); pm[m] = rl32(ud.y, m);
        ro[m + 1] = ro[m] + rl32(nr_l, m);
    }
    const int R = ro[G];

    // the pack's raters, one per lane
    bool packed = R <= 64;
    int eoff = 0, usrf = 0, end = 0, total = 0;
    float r = 0.f;
    if (packed) {
        int p = pm[0] + lane;
#pragma unroll
        for (int m = 1; m < G; m++)
            if (lane >= ro[m]) p = pm[m] + (lane - ro[m]);
        const bool ok = lane < R;
        const RaterRec rr = A.rc[ok ? p : pm[0]];
        {
            const uint4 e4 = make_uint4(T_EMPTY, T_EMPTY, T_EMPTY, T_EMPTY), z4 = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int x = 0; x < GS / 256; x++) { ((uint4 *)key)[x * 64 + lane] = e4; ((uint4 *)cm)[x * 64 + lane] = z4; }
        }
        r = rr.rating;
        usrf = rr.user | (rr.pos_ge & (int)0x80000000);   // the rater's side of its item's average travels with the user
        const int len = ok ? (rr.pos_ge & 0x7fffffff) : 0;       // the rater's prefix: entries [e0, e0 + len) of its profile
        end = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(end, d, 64); if (lane >= d) end += v; }
        total = rl32(end, 63);
        eoff = rr.e0 - (end - len);           // co-rating f of the flat list is entry eoff + f
        packed = total <= CAP;
    }
    if (!packed) {
        for (int m = 0; m < nm; m++) {
            const int i = rl32(it_l, m), p0 = rl32(ud.y, m), p1 = rl32(ud.z, m);
            int ovf = 0;
            __syncthreads();          // (one wave: orders the LDS phases)
            for (int s = lane; s < S; s += 64) { key1[s] = T_EMPTY; cm1[s] = 0u; dot1[s] = 0.0; dlo1[s] = 0.0; }
            __syncthreads();
            // the walk of k_pair_tri in blocks of 64 raters, one round at a time
            for (int base = p0; base < p1; base += 64) {
                const bool ok = base + lane < p1;
                const RaterRec rr = A.rc[ok ? base + lane : p0];
                const int len = ok ? (rr.pos_ge & 0x7fffffff) : 0;
                int en = len;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(en, d, 64); if (lane >= d) en += v; }
                const int tot = rl32(en, 63);
                const int st = en - len;
                for (int f0 = 0; f0 < tot; f0 += 64) {
                    const int f = f0 + lane;
                    bool act = f < tot;
                    int t = 0;
#pragma unroll
                    for (int step = 32; step >= 1; step >>= 1) { const int v = __shfl(en, t + step - 1, 64); if (v <= f) t += step; }
                    const int eb = __shfl(rr.e0, t, 64), sb = __shfl(st, t, 64), ut = __shfl(rr.user, t, 64);
                    const int pwt = __shfl(rr.pos_ge, t, 64);
                    const double ri = (double)__shfl(rr.rating, t, 64);
                    const int2 v = A.ub[act ? eb + (f - sb) : 0];
                    const double a = ADJ ? A.u_avg[act ? ut : 0] : 0.0;
                    const int j = v.x & 0x7fffffff;
                    const double rjd = (double)__int_as_float(v.y);
                    uint32_t h = 0;
                    if (act) {
                        h = ((uint32_t)j * 0x9E3779B1u) >> (32 - LOG_SLOTS);
                        int probes = 0;
                        for (;;) {
                            const uint32_t prev = atomicCAS(&key1[h], T_EMPTY, (uint32_t)j);
                            if (prev == T_EMPTY || prev == (uint32_t)j) break;
                            h = (h + 1) & (S - 1);
                            if (++probes >= S) { act = false; ovf = 1; break; }
                        }
                    }
                    if (act) atomicAdd(&cm1[h], 1u | (((((unsigned)v.x) >> 31) == (((unsigned)pwt) >> 31)) ? (1u << 16) : 0u));
                    const double tm = ADJ ? (ri - a) * (rjd - a) : (1.0 * ri) * rjd;
                    // (LDS-qualified volatile accesses, as in k_pair_tri)
                    typedef __attribute__((address_space(3))) volatile double lds_vf64;
                    typedef __attribute__((address_space(3))) volatile unsigned short lds_vu16;
                    lds_vf64 *vhi = (lds_vf64 *)dot1, *vlo = (lds_vf64 *)dlo1;
                    lds_vu16 *vclaim = (lds_vu16 *)claim1;
                    bool pending = act;
                    while (__ballot(pending)) {       // lanes that share a slot take turns
                        if (pending) vclaim[h] = (unsigned short)lane;
                        if (pending && vclaim[h] == (unsigned short)lane) {
                            double hi = vhi[h], lo = vlo[h];
                            dd_add(hi, lo, tm);
                            vhi[h] = hi; vlo[h] = lo;
                            pending = false;
                        }
                    }
                }
            }
            __syncthreads();
            if (__ballot(ovf)) {
                if (lane == 0) atomicOr(&A.counters[2], 1ull);
                return;
            }
            append_pairs(A, i, 0, S,
                [&](int s, int &j, int &n, int &mu, double &sv, bool &o) {
                    const uint32_t kj = key1[s];
                    o = kj != T_EMPTY;
                    if (!o) return false;
                    j = (int)kj; n = (int)(cm1[s] & 0xffffu); mu = (int)(cm1[s] >> 16);
                    return finish_pair<METHOD>(A, i, j, n, mu, dot1[s], sv);
                },
                [&](int s, bool o, bool keep, double sv) {
                    if (o) { if (keep) dot1[s] = sv; else key1[s] = T_EMPTY; }
                },
                [&](int s, int &j, int &n, int &mu, double &sv) {
                    const uint32_t kj = key1[s];
                    if (kj == T_EMPTY) return false;
                    j = (int)kj; n = (int)(cm1[s] & 0xffffu); mu = (int)(cm1[s] >> 16); sv = dot1[s];
                    return true;
                },
                [&](int s) { return 0.0; });
        }
        return;
    }
    double nxm[G];                        // (for the finalisation: in flight during the walk)
#pragma unroll
    for (int m = 0; m < G; m++) nxm[m] = A.nrm[im[m]];
    // the walk: co-rating f = 64 u + lane of the pack's flat list, all rounds' loads in flight together (k_pair_tri: walk)
    int jw[PACK_E], tt[PACK_E], ee[PACK_E], uu[PACK_E], sr[PACK_E];
    float rj[PACK_E];
    double term[PACK_E], ny[PACK_E];
    int ovf = 0;
#pragma unroll
    for (int u = 0; u < PACK_E; u++) {
        if (u * 64 >= total) break;           // (uniform)
        const int f = u * 64 + lane;
        const bool act = f < total;
        int t = 0;                            // the rater of co-rating f: #{k : end[k] <= f}
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) { const int v = __shfl(end, t + step - 1, 64); if (v <= f) t += step; }
        const int eo = __shfl(eoff, t, 64), uf = __shfl(usrf, t, 64);
        tt[u] = t;
        ee[u] = act ? eo + f : 0;
        uu[u] = act ? uf : 0;
    }
#pragma unroll
    for (int u = 0; u < PACK_E; u++) {
        if (u * 64 >= total) break;
        const int2 v = A.ub[ee[u]];
        jw[u] = v.x; rj[u] = __int_as_float(v.y);
        term[u] = ADJ ? A.u_avg[uu[u] & 0x7fffffff] : 0.0;       // (the rater's average, until the term is formed)
    }
#pragma unroll
    for (int u = 0; u < PACK_E; u++) {
        sr[u] = -1;
        if (u * 64 >= total) continue;
        const double ri = (double)__shfl(r, tt[u], 64);
        int mt = 0;                           // the member of the rater
#pragma unroll
        for (int m = 1; m < G; m++) mt += (tt[u] >= ro[m]) ? 1 : 0;
        const int j = jw[u] & 0x7fffffff;
        bool act = u * 64 + lane < total;
        ny[u] = act ? A.nrm[j] : 0.0;         // (for the finalisation)
        uint32_t h = 0;
        if (act) {
            const uint32_t tb = (uint32_t)mt << LOG_SLOTS;
            h = ((uint32_t)j * 0x9E3779B1u) >> (32 - LOG_SLOTS);
            int probes = 0;
            for (;;) {
                const uint32_t prev = atomicCAS(&key[tb + h], T_EMPTY, (uint32_t)j);
                if (prev == T_EMPTY || prev == (uint32_t)j) break;
                h = (h + 1) & (S - 1);
                if (++probes >= S) { act = false; ovf = 1; break; }
            }
            h += tb;
        }
        if (act) {
            const uint32_t inc = 1u | (((((unsigned)jw[u]) >> 31) == (((unsigned)uu[u]) >> 31)) ? (1u << 16) : 0u);
            const uint32_t rank = atomicAdd(&cm[h], inc) & 0xffffu;
            sr[u] = (int)(h | (rank << 16));
            const double a = term[u];
            term[u] = ADJ ? (ri - a) * ((double)rj[u] - a) : (1.0 * ri) * (double)rj[u];
        }
    }
    if (__ballot(ovf)) {
        if (lane == 0) atomicOr(&A.counters[2], 1ull);
        return;
    }
    __syncthreads();          // (one wave: orders the LDS phases)
    // offsets of the slots' terms (lane-major: the slots 64 k + lane of a lane follow one another); they replace the keys
    {
        int cnt[NIT], mine = 0;
#pragma unroll
        for (int k = 0; k < NIT; k++) { cnt[k] = (int)(cm[k * 64 + lane] & 0xffffu); mine += cnt[k]; }
        int off = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(off, d, 64); if (lane >= d) off += v; }
        off -= mine;
#pragma unroll
        for (int k = 0; k < NIT; k++) { key[k * 64 + lane] = (uint32_t)off; off += cnt[k]; }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PACK_E; u++)
        if (sr[u] >= 0) terms[key[sr[u] & 0xffff] + (uint32_t)(sr[u] >> 16)] = term[u];
    __syncthreads();
    // finalisation (k_pair_tri's, for G rows, by the lanes of rank 0): one returning atomic on the shard cursor for the pack's
    // kept pairs, the appends in the order of the flat list -- a row's records stay contiguous in its shard --, a row-count
    // add per member
    const auto k_coo_i = KARG(coo_i);
    const auto k_coo_j = KARG(coo_j);
    const auto k_coo_sim = KARG(coo_sim);
    const auto k_coo_mutu = KARG(coo_mutu);
    const auto k_coo_nij = KARG(coo_nij);
    const auto k_rowcnt = KARG(rowcnt);
    const auto k_shard_cur = KARG(shard_cur);
    const auto k_shard_occ = KARG(shard_occ);
    const auto k_shard_cap = KARG(shard_cap);
    const auto k_cap = KARG(cap);
    const auto k_counters = KARG(counters);
    unsigned long long fk[PACK_E];        // ballots of the kept pairs
    uint32_t fc[PACK_E];
    int kept = 0, occ = 0, mkept = 0;     // mkept: lane m holds member m's kept pairs
#pragma unroll
    for (int u = 0; u < PACK_E; u++) {
        fk[u] = 0ull;
        if (u * 64 >= total) continue;
        const bool own = sr[u] >= 0 && (sr[u] >> 16) == 0;
        const int slot = own ? (sr[u] & 0xffff) : 0;
        const int mt = slot >> LOG_SLOTS;
        const uint32_t c = cm[slot];
        const int n = own ? (int)(c & 0xffffu) : 0, mu = (int)(c >> 16);
        const int off = (int)key[slot];
        double hi = 0.0, lo = 0.0;
        for (int x = 0; __ballot(x < n); x++)
            if (x < n) dd_add(hi, lo, terms[off + x]);
        bool keep = own;
        if (own) {                        // cosine (:91-95), significance weighting (:84-89), zero filter (:198,:207): finish_pair
            double nx = nxm[0];
#pragma unroll
            for (int m = 1; m < G; m++) nx = (mt == m) ? nxm[m] : nx;
            const double np = nx * ny[u];
            const double cs = (np != 0.0) ? 1.0 * hi / np : 0.0;
            const int mn = n < k_cap ? n : k_cap;
            hi = 1.0 * cs * (double)mn / (double)k_cap;
            keep = (hi != 0.0) && (mu != 0);
        }
        term[u] = hi;
        fc[u] = c;
        fk[u] = __ballot(keep);
        kept += __popcll(fk[u]);
        occ += __popcll(__ballot(own));
#pragma unroll
        for (int m = 0; m < G; m++) {
            const int cm_ = __popcll(__ballot(keep && mt == m));
            if (lane == m) mkept += cm_;
        }
    }
    const int shard = blockIdx.x & (COO_SHARDS - 1);
    if (lane == 0 && occ) atomicAdd(&k_shard_occ[shard], (unsigned long long)occ);
    if (!kept) return;
    unsigned long long cbase = 0;
    if (lane == 0) cbase = atomicAdd(&k_shard_cur[shard], (unsigned long long)kept);
    if (mkept) atomicAdd(&k_rowcnt[it_l], mkept);
    cbase = ((unsigned long long)(unsigned)rl32((int)(cbase >> 32), 0) << 32) | (unsigned)rl32((int)(cbase & 0xffffffffull), 0);
    if ((long long)(cbase + kept) > k_shard_cap) {
        if (lane == 0) atomicOr(&k_counters[3], 1ull);
        return;
    }
    cbase += (unsigned long long)shard * (unsigned long long)k_shard_cap;
#pragma unroll
    for (int u = 0; u < PACK_E; u++) {
        if ((fk[u] >> lane) & 1ull) {
            const long long pp = (long long)cbase + __popcll(fk[u] & lanemask_lt());
            const int mt = (sr[u] & 0xffff) >> LOG_SLOTS;
            int i = im[0];
#pragma unroll
            for (int m = 1; m < G; m++) i = (mt == m) ? im[m] : i;
            k_coo_i[pp] = i; k_coo_j[pp] = jw[u] & 0x7fffffff;
            k_coo_sim[pp] = term[u]; k_coo_mutu[pp] = (int)(fc[u] >> 16); k_coo_nij[pp] = (int)(fc[u] & 0xffffu);
        }
        cbase += __popcll(fk[u]);
    }
}

// rows of H: chunk c of the raters, dense table over H (partners of a heavy row are heavier, hence in H)
// HEAVY_WAVES waves share the unit's dense table (each takes every HEAVY_WAVES-th block of 64 raters): a unit is a chain
// of dependent gathers (rater record -> prefix entry -> heavy id) and one wave per 26 KB table left 6 waves on a CU.
constexpr int HEAVY_WAVES = 4;
template <int METHOD>
__global__ __launch_bounds__(64 * HEAVY_WAVES) void k_pair_heavy(TriArgs A) {
    __shared__ uint32_t cnt[HMAX];
    __shared__ uint32_t mut[HMAX];
    __shared__ double dot[HMAX];
    __shared__ double dlo[METHOD == XMAP_ADJUST_COSINE ? HMAX : 1];
    __shared__ unsigned lockw[METHOD == XMAP_ADJUST_COSINE ? HMAX : 1];
    const int lane = lane_id(), w = uniform((int)(threadIdx.x >> 6));
    const int unit = blockIdx.x;
    for (int s = threadIdx.x; s < HMAX; s += 64 * HEAVY_WAVES) {
        cnt[s] = 0; mut[s] = 0; dot[s] = 0.0;
        if (METHOD == XMAP_ADJUST_COSINE) { dlo[s] = 0.0; lockw[s] = 0u; }
    }
    __syncthreads();
    const int i = uniform(A.uc_item[unit]);
    if (A.heavy_mod > 1 && (i % A.heavy_mod) != A.heavy_rem) return;      // another rank's heavy row (by ITEM index: the dense
                                                                          // heavy ids are handed out by atomics and differ between ranks)
    const int c = uniform(A.uc_c[unit]);
    const int CH = uniform(*A.CH);
    const int base0 = uniform((int)A.iptr[i]);
    const int p0 = base0 + c * CH;
    int p1 = uniform((int)A.iptr[i + 1]);
    if (p0 + CH < p1) p1 = p0 + CH;
    for (int base = p0 + 64 * w; base < p1; base += 64 * HEAVY_WAVES) {
        const int p = base + lane;
        int e0 = 0, pw = 0;
        float r = 0.f;
        double au = 0.0;
        if (p < p1) {
            const RaterRec rr = A.rc[p];
            e0 = rr.e0; pw = rr.pos_ge; r = rr.rating;
            if (METHOD == XMAP_ADJUST_COSINE) au = A.u_avg[rr.user];
        }
        // one rater per lane: within H a rater's prefix is short (0.8 entries on average at BASELINE configs[1]), so
        // every lane walks its own; lanes that meet on a partner use LDS atomics / a lock word per slot
        const int b1 = (p < p1) ? e0 + (pw & 0x7fffffff) : e0;
        const unsigned gei = ((unsigned)pw) >> 31;
        const double ri = (double)r;
        for (int e = e0; __ballot(e < b1); e++) {
            const bool act = e < b1;
            int h = 0;
            double term = 0.0;
            if (act) {
                const int2 v = A.ub[e];
                const int jw = v.x;
                const float rj = __int_as_float(v.y);
                h = A.hid[jw & 0x7fffffff];
                atomicAdd(&cnt[h], 1u);
                if ((((unsigned)jw) >> 31) == gei) atomicAdd(&mut[h], 1u);
                if (METHOD == XMAP_COSINE) atomicAdd(&dot[h], (1.0 * ri) * (double)rj);   // integer-exact
                else term = (ri - au) * ((double)rj - au);
            }
            if (METHOD == XMAP_ADJUST_COSINE) {
                volatile double *vhi = dot, *vlo = dlo;
                bool pending = act;
                while (__ballot(pending)) {       // a lock per slot: the holder releases in the same pass
                    if (pending && atomicCAS(&lockw[h], 0u, 1u) == 0u) {
                        double hi = vhi[h], lo = vlo[h];
                        dd_add(hi, lo, term);
                        vhi[h] = hi; vlo[h] = lo;
                        __threadfence_block();
                        atomicExch(&lockw[h], 0u);
                        pending = false;
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < HMAX; s += 64 * HEAVY_WAVES) {
        size_t o = (size_t)unit * HMAX + s;
        A.hp_cnt[o] = (int)cnt[s];
        A.hp_mut[o] = (int)mut[s];
        A.hp_hi[o] = dot[s];
        A.hp_lo[o] = (METHOD == XMAP_ADJUST_COSINE) ? dlo[s] : 0.0;
    }
}

template <int METHOD>
__global__ __launch_bounds__(256) void k_heavy_merge(TriArgs A, int n_heavy) {
    __shared__ uint32_t cnt[HMAX];
    __shared__ uint32_t mut[HMAX];
    __shared__ double dot[HMAX];
    const int h = blockIdx.x;
    if (h >= n_heavy) return;
    const int i = A.hlist[h];
    if (A.heavy_mod > 1 && (i % A.heavy_mod) != A.heavy_rem) return;
    const int nc = A.C[i];
    const long long u0 = A.uc_ptr[i];
    // four waves per row: the most popular item has ~80 chunks of partials to fold
    for (int s = threadIdx.x; s < HMAX; s += 256) {
        unsigned cn = 0, mu = 0;
        double hi = 0.0, lo = 0.0;
        for (int c = 0; c < nc; c++) {
            size_t o = (size_t)(u0 + c) * HMAX + s;
            cn += (unsigned)A.hp_cnt[o];
            mu += (unsigned)A.hp_mut[o];
            if (METHOD == XMAP_COSINE) {
                hi += A.hp_hi[o];
            } else {
                dd_add(hi, lo, A.hp_hi[o]);
                dd_add(hi, lo, A.hp_lo[o]);
            }
        }
        cnt[s] = cn; mut[s] = mu; dot[s] = hi;
    }
    if (nc == 0) return;
    __syncthreads();
    const int w = uniform((int)(threadIdx.x >> 6));
    append_pairs(A, i, w * (HMAX / 4), (w + 1) * (HMAX / 4),
        [&](int s, int &j, int &n, int &m, double &sv, bool &o) {
            o = cnt[s] != 0;
            if (!o) return false;
            j = A.hlist[s]; n = (int)cnt[s]; m = (int)mut[s];
            return finish_pair<METHOD>(A, i, j, n, m, dot[s], sv);
        },
        [&](int s, bool o, bool keep, double sv) {
            if (o) { if (keep) dot[s] = sv; else cnt[s] = 0; }
        },
        [&](int s, int &j, int &n, int &m, double &sv) {
            if (cnt[s] == 0) return false;
            j = A.hlist[s]; n = (int)cnt[s]; m = (int)mut[s]; sv = dot[s];
            return true;
        },
        [&](int s) { return 0.0; });
}

}  // namespace xmap

using namespace xmap;

// forked streams for the per-class pair kernels (created once per process and device; never destroyed)
struct SideStreams { hipStream_t s[N_CLASSES + 1]; hipEvent_t fork, done[N_CLASSES + 1]; int dev; };   // + one for the heavy rows
static SideStreams *side_streams() {
    static thread_local SideStreams *cur[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { set_error("hipGetDevice failed"); return nullptr; }
    if (cur[dev]) return cur[dev];
    SideStreams *p = new SideStreams();
    p->dev = dev;
    bool ok = hipEventCreateWithFlags(&p->fork, hipEventDisableTiming) == hipSuccess;
    for (int c = 0; c <= N_CLASSES && ok; c++)
        ok = hipStreamCreateWithFlags(&p->s[c], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&p->done[c], hipEventDisableTiming) == hipSuccess;
    if (!ok) { set_error("could not create the side streams"); delete p; return nullptr; }
    cur[dev] = p;
    return p;
}

namespace {

// the light rows of the table class of rank c (class_rank): the one table of {LOG_SLOTS, waves sharing the LDS table} per class
template <int METHOD, bool LS>
int launch_tri(int c, dim3 grid, hipStream_t st, const TriArgs &A) {
#define XM_TRI(LOG_SLOTS, NW) k_pair_tri<METHOD, LOG_SLOTS, NW, LS><<<grid, dim3(64 * NW), 0, st>>>(A)
    switch (c) {
    case 0: XM_TRI(10, 16); break;        // class 4: light rows with >= WIDE_MIN raters
    case 1: XM_TRI(10, 4); break;         // class 0
    case 2: XM_TRI(9, 2); break;          // class 2
    case 3: XM_TRI(8, 1); break;          // class 3
    default: XM_TRI(7, 1); break;         // class 1
    }
#undef XM_TRI
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

// rows per wave (G) and rounds of co-ratings held (E) of the packed classes (profiles/r10_pair_packs.txt: the sweep).  Two
// rows: at BASELINE configs[1] two rows of the 128-slot class have at most 192 co-ratings, two of the 256-slot class at most
// 383; four rows per wave (E = 6) ran 8 % longer in the 128-slot class, eight 70 % longer: what a wave does for its rows it does
// one round after the other, and a pack lives as long as that takes
constexpr int PACK_G128 = 2, PACK_E128 = 3, PACK_G256 = 2, PACK_E256 = 6;
// the packed classes (k_pair_pack): rank 4 = the 128-slot class, rank 3 = the 256-slot class -> the units of a pack
int pack_units(int c) { return c == 4 ? PACK_G128 : (c == 3 ? PACK_G256 : 0); }
template <int METHOD>
int launch_pack(int c, long long n_units, hipStream_t st, const TriArgs &A) {
    const int g = pack_units(c);
    const dim3 grid((unsigned)((n_units + g - 1) / g));
    if (c == 4) k_pair_pack<METHOD, 7, PACK_G128, PACK_E128><<<grid, dim3(64), 0, st>>>(A);
    else k_pair_pack<METHOD, 8, PACK_G256, PACK_E256><<<grid, dim3(64), 0, st>>>(A);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

// the rows of H: chunk partials of n_units heavy units (0: none), then the merge of n_heavy rows (0: none)
int launch_heavy(int method, hipStream_t st, const TriArgs &A, int n_units, int n_heavy) {
    const bool cos = method == XMAP_COSINE;         // (else the double-double kernels; exact cosine arrives as adjusted cosine)
    if (n_units > 0) {
        (cos ? k_pair_heavy<XMAP_COSINE> : k_pair_heavy<XMAP_ADJUST_COSINE>)<<<dim3((unsigned)n_units), dim3(64 * HEAVY_WAVES), 0, st>>>(A);
        XM_LAUNCH_CHECK();
    }
    if (n_heavy > 0) {
        (cos ? k_heavy_merge<XMAP_COSINE> : k_heavy_merge<XMAP_ADJUST_COSINE>)<<<dim3((unsigned)n_heavy), dim3(256), 0, st>>>(A, n_heavy);
        XM_LAUNCH_CHECK();
    }
    return XMAP_OK;
}

}  // namespace

extern "C" {

int xmap_sim2_pairs(void *stream, const xmap_ratings *R, int method, int cap, const double *u_avg, const double *norms, const void *rc,
                    const void *ub, const int32_t *Q, const uint8_t *small, const int32_t *uq_item, const int32_t *uq_q,
                    const int64_t *cls_ptr /*host [6]*/, int64_t unit_lo, int64_t unit_hi, const int32_t *hid, const int32_t *hlist,
                    const int32_t *ctl, const int32_t *C, const int64_t *uc_ptr, const int32_t *uc_item, const int32_t *uc_c,
                    int32_t n_heavy_units, int32_t n_heavy, int phases, double *hp_hi, double *hp_lo, int32_t *hp_cnt, int32_t *hp_mut,
                    int64_t coo_cap, int32_t *coo_i, int32_t *coo_j, double *coo_sim, int32_t *coo_mutu, int32_t *coo_nij,
                    double *coo_ls /*or NULL*/, int32_t *rowcnt, int64_t *d_shards /*[2][4096]*/, int64_t *d_counters /*[4]*/,
                    int32_t *mircnt /*[I] or NULL*/) {
    XM_SCOPE(stream);
    XM_ARG(R && u_avg && norms && rc && ub);
    XM_ARG(Q && small && uq_item && uq_q && cls_ptr && hid && hlist && ctl && C && uc_ptr && uc_item && uc_c);
    XM_ARG(coo_i && coo_j && coo_sim && coo_mutu && coo_nij && rowcnt && d_shards && d_counters);
    XM_ARG(coo_cap >= COO_SHARDS);
    XM_ARG(method == XMAP_COSINE || method == XMAP_ADJUST_COSINE || method == XMAP_COSINE_EXACT);
    XM_ARG(n_heavy_units == 0 || !(phases & (XMAP_PAIRS_HEAVY | XMAP_PAIRS_HEAVY_MERGE)) || (hp_hi && hp_lo && hp_cnt && hp_mut));
    hipStream_t st = (hipStream_t)stream;
    // exact cosine: the adjusted-cosine kernels (double-double dot product) with a zero user average and the plain norms
    const bool exact_cos = method == XMAP_COSINE_EXACT;
    const double *nrm = norms + (method == XMAP_ADJUST_COSINE ? (size_t)R->n_items : 0);
    FillList F;             // the small fills of the call leave in one launch
    if (exact_cos) {
        double *zero_avg = nullptr;
        const size_t ub = sizeof(double) * (size_t)(R->n_users > 0 ? R->n_users : 1);
        XM_HIP(xm_malloc_async((void **)&zero_avg, ub, st));
        F.add(zero_avg, ub);
        u_avg = zero_avg;
        method = XMAP_ADJUST_COSINE;
    }
    // coo_ls selects the RecommenderSim variant: exact (double-double) sums, no filter, local sensitivity; its layout
    // has no heavy rows
    const bool raw = (phases & XMAP_PAIRS_RAW) != 0;      // partial sums of a user share: coo_ls is then the error column of the dot
    XM_ARG(!coo_ls || ((raw || method == XMAP_ADJUST_COSINE) && n_heavy_units == 0));
    XM_ARG(!raw || (coo_ls && n_heavy_units == 0 && n_heavy == 0));
    const size_t In = (size_t)(R->n_items > 0 ? R->n_items : 1);
    // with RESET the shard sums' two words are cleared along with the counters; without, in front of k_shard_sums
    const bool sums_cleared = (phases & XMAP_PAIRS_RESET) && (phases & XMAP_PAIRS_SHARD_SUMS);
    if (phases & XMAP_PAIRS_RESET) {   // reset the COO cursor / counters / row counts
        F.add(d_counters, (sums_cleared ? 6 : 4) * sizeof(int64_t));
        F.add(d_shards, 2 * COO_SHARDS * sizeof(int64_t));
        // -1 = unused entry (NO_MARKS: the caller reads the COO through the shard cursors only: 0.4 GB less to write)
        if (!(phases & XMAP_PAIRS_NO_MARKS)) XM_HIP(hipMemsetAsync(coo_i, 0xff, sizeof(int32_t) * (size_t)coo_cap, st));
        F.add(rowcnt, sizeof(int32_t) * In);
        if (mircnt) F.add(mircnt, sizeof(int32_t) * In);
    }
    {
        int rc_fill = fill_multi(st, F);
        if (rc_fill) return rc_fill;
    }
    TriArgs A;
    memset(&A, 0, sizeof(A));
    A.iptr = (const long long *)R->item_ptr; A.rc = (const RaterRec *)rc; A.ub = (const int2 *)ub;
    A.u_avg = u_avg; A.nrm = nrm; A.cap = cap;
    A.Q = Q; A.small = small; A.uq_item = uq_item; A.uq_q = uq_q; A.unit_lo = unit_lo; A.unit_hi = unit_hi;
    A.hid = hid; A.hlist = hlist; A.CH = ctl; A.uc_item = uc_item; A.uc_c = uc_c;
    A.uc_ptr = (const long long *)uc_ptr; A.C = C;
    A.hp_hi = hp_hi; A.hp_lo = hp_lo; A.hp_cnt = hp_cnt; A.hp_mut = hp_mut;
    A.shard_cap = coo_cap / COO_SHARDS; A.shard_cur = (unsigned long long *)d_shards;
    A.shard_occ = (unsigned long long *)d_shards + COO_SHARDS;
    A.coo_i = coo_i; A.coo_j = coo_j; A.coo_sim = coo_sim; A.coo_mutu = coo_mutu; A.coo_nij = coo_nij; A.coo_aux = coo_ls; A.raw = raw ? 1 : 0;
    A.heavy_mod = XMAP_PAIRS_DEAL_MOD(phases); A.heavy_rem = XMAP_PAIRS_DEAL_REM(phases);
    if (A.heavy_mod < 1) A.heavy_mod = 1;
    A.rowcnt = rowcnt; A.mircnt = mircnt; A.counters = (unsigned long long *)d_counters;
    // HEAVY | LIGHT | HEAVY_MERGE in one call: the heavy rows (chunk partials, then their merge) run on a side stream of their
    // own, next to the class launches of the light rows -- they share nothing but the atomic COO cursors and counters
    const int all_rows = XMAP_PAIRS_HEAVY | XMAP_PAIRS_LIGHT | XMAP_PAIRS_HEAVY_MERGE;
    const bool light = (phases & XMAP_PAIRS_LIGHT) && unit_hi > unit_lo;
    const bool heavy_aside = (phases & all_rows) == all_rows && n_heavy_units > 0 && unit_hi > unit_lo;
    hipStream_t hs = st;
    SideStreams *side = nullptr;
    if (light || heavy_aside) {
        side = side_streams();
        if (!side) return XMAP_ERR_HIP;
        XM_HIP(hipEventRecord(side->fork, st));
    }
    if (heavy_aside) {
        hs = side->s[N_CLASSES];
        XM_HIP(hipStreamWaitEvent(hs, side->fork, 0));
    }
    int rcode = launch_heavy(method, hs, A, (phases & XMAP_PAIRS_HEAVY) ? n_heavy_units : 0, heavy_aside ? n_heavy : 0);
    if (rcode) return rcode;
    if (heavy_aside) {
        XM_HIP(hipEventRecord(side->done[N_CLASSES], hs));
        XM_HIP(hipStreamWaitEvent(st, side->done[N_CLASSES], 0));
    }
    if (light) {
        // one launch per table class: the class's units within [unit_lo, unit_hi).  The classes are independent (they
        // only share the COO cursors, which are atomic) and each ends in a tail of long rows at low occupancy: they
        // run side by side on forked streams and the caller's stream joins them.
        // the 128- and 256-slot classes go through k_pair_pack, several rows per wave; the raw step and RecommenderSim keep
        // k_pair_tri there.  XMAP_PAIR_PACKS=0 (tests, A/B runs): every class through k_pair_tri
        const char *pk_env = getenv("XMAP_PAIR_PACKS");
        const bool packs = !raw && !coo_ls && !(pk_env && atoi(pk_env) == 0);
        for (int c = 0; c < N_CLASSES; c++) {
            const long long lo = unit_lo > cls_ptr[c] ? unit_lo : cls_ptr[c];
            const long long hi = unit_hi < cls_ptr[c + 1] ? unit_hi : cls_ptr[c + 1];
            if (hi <= lo) continue;
            A.unit_lo = lo; A.unit_hi = hi;
            const dim3 grid((unsigned)(hi - lo));
            hipStream_t cs = side->s[c];
            XM_HIP(hipStreamWaitEvent(cs, side->fork, 0));
            if (packs && pack_units(c))
                rcode = method == XMAP_COSINE ? launch_pack<XMAP_COSINE>(c, hi - lo, cs, A) : launch_pack<XMAP_ADJUST_COSINE>(c, hi - lo, cs, A);
            else if (coo_ls && !raw) rcode = launch_tri<XMAP_ADJUST_COSINE, true>(c, grid, cs, A);
            else if (method == XMAP_COSINE) rcode = launch_tri<XMAP_COSINE, false>(c, grid, cs, A);
            else rcode = launch_tri<XMAP_ADJUST_COSINE, false>(c, grid, cs, A);
            if (rcode) return rcode;
            XM_HIP(hipEventRecord(side->done[c], cs));
            XM_HIP(hipStreamWaitEvent(st, side->done[c], 0));
        }
        A.unit_lo = unit_lo; A.unit_hi = unit_hi;
    }
    if ((phases & XMAP_PAIRS_HEAVY_MERGE) && !heavy_aside && n_heavy_units > 0) {
        rcode = launch_heavy(method, st, A, 0, n_heavy);
        if (rcode) return rcode;
    }
    if (phases & XMAP_PAIRS_SHARD_SUMS) {      // d_counters is [6]: [4] = kept pairs, [5] = unordered pairs evaluated (sums over the shards)
        if (!sums_cleared) XM_HIP(hipMemsetAsync(d_counters + 4, 0, 2 * sizeof(int64_t), st));
        k_shard_sums<<<dim3(1), dim3(256), 0, st>>>((const unsigned long long *)d_shards, (unsigned long long *)d_counters);
        XM_LAUNCH_CHECK();
    }
    if ((phases & XMAP_PAIRS_MIRCOUNT) && !raw && !mircnt && R->n_items > 0) {
        // the round-2 sequence / cross-checks (one combined count per row): the mirrored counts on top of the own ones, from
        // the partner column of the COO.  The round-3 caller (mircnt given) counts in xmap_sim3_mircount, where it has scratch.
        int *part = nullptr;
        XM_HIP(xm_malloc_async((void **)&part, sizeof(int) * (size_t)coo_cap, st));
        return mirror_counts(st, R->n_items, coo_cap / COO_SHARDS, COO_SHARDS, (const unsigned long long *)d_shards, coo_i, coo_j,
                             coo_ls != nullptr, part, rowcnt);
    }
    return XMAP_OK;
}

/* The host's read of the pair kernels' counters without draining the stream (include/xmap_hip.h): begin queues the copy into
 * pinned memory and an event behind it, wait takes the event. */
int xmap_sim3_counters_begin(void *stream, const int64_t *d_counters) {
    XM_ARG(d_counters);
    return host_wait_post((hipStream_t)stream, HW_PAIRS, d_counters, 6);
}
int xmap_sim3_counters_wait(int64_t *h_out) {
    XM_ARG(h_out);
    const int64_t *h = nullptr;
    int rcode = host_wait_take(HW_PAIRS, &h);
    if (rcode) return rcode;
    for (int c = 0; c < 6; c++) h_out[c] = h[c];
    return XMAP_OK;
}
}
