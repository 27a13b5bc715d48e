// tri_layout.hip -- stage A, "tri" formulation (tri.h): everything the pair kernels read, and the list of their work units.
//   k_hist / k_threshold / k_mark_heavy : rater-count histogram -> #items at least as heavy (bound on a row's
//                                         distinct partners) and the set H of at most HMAX items with more
//                                         than CH raters (dense ids)
//   k_sort_profiles : per-user sort by weight (4 short profiles per wave)
//   k_rater_records : the rater records of every item; W+_i = number of contributions of row i (k_plan2)
//   k_plan2 / k_fill_units2 : light units (item, hash partition) listed by LDS table class, heavy units (item in H,
//                     chunk of CH raters)
//   round 3 (one transposition per pass, below): k_count3, k_sort_profiles3, k_rc_tiles / RcFin through the tile sort,
//                     k_item_stats3 .. k_item_big_flags, k_rc_flags / k_ub_flags
#include "tri.h"
#include "item_stats.h"

namespace xmap {

__device__ __forceinline__ unsigned long long wkey(int n, int item) {
    return ((unsigned long long)(unsigned)n << 32) | (unsigned)item;
}

// ---------------------------------------------------------------------------------------------
// most items have a handful of raters: the low bins are counted per workgroup in LDS first
constexpr int HIST_LDS = 2048;
constexpr int HIST_PER = 16;   // items per thread
__global__ __launch_bounds__(256) void k_hist(int I, const long long *iptr, int HB, int *hist) {
    __shared__ int loc[HIST_LDS];
    for (int t = threadIdx.x; t < HIST_LDS; t += 256) loc[t] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * 256 * HIST_PER;
    for (int q = 0; q < HIST_PER; q++) {
        const long long i = base + (long long)q * 256 + threadIdx.x;
        if (i < I) {
            long long n = iptr[i + 1] - iptr[i];
            int bin = n < HB - 1 ? (int)n : HB - 1;
            if (bin < HIST_LDS) atomicAdd(&loc[bin], 1); else atomicAdd(&hist[bin], 1);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < HIST_LDS && t < HB; t += 256)
        if (loc[t]) atomicAdd(&hist[t], loc[t]);
}

// pre[v] = #{items with n < v}.  CH = smallest v >= ch_min with #{n > v} <= HMAX.
__global__ __launch_bounds__(256) void k_threshold(int I, int HB, const long long *pre, int ch_min, int *CH) {
    int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= HB - 1 || v < ch_min) return;
    long long gt_v = I - pre[v + 1];
    long long gt_prev = (v == ch_min) ? (long long)HMAX + 1 : I - pre[v];
    if (gt_v <= HMAX && (v == ch_min || gt_prev > HMAX)) atomicMin(CH, v);
}

__global__ __launch_bounds__(256) void k_mark_heavy(int I, const long long *iptr, const int *CH, int *hid, int *hlist,
                                                    int *n_heavy) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I) return;
    long long n = iptr[i + 1] - iptr[i];
    int h = -1;
    if (n > *CH) {
        h = atomicAdd(n_heavy, 1);
        if (h < HMAX) hlist[h] = i;
    }
    hid[i] = h;
}

// private copy of every profile sorted heaviest first, (index | flag, rating) interleaved.  One wave per 4 users:
// profiles of up to 16 ratings (90 % at BASELINE configs[1]) are sorted four at a time, one per 16-lane group, by a
// bitonic network cut off at the longest of the four (the xor-shuffles never leave a group); the others follow one
// by one on the whole wave (network cut off at the profile's length), profiles above 64 ratings by counting ranks.
__device__ __forceinline__ void sort_entry(const int *uitem, const float *urating, const long long *iptr,
                                           const double *info, long long e, unsigned long long &key, int &px, int &py) {
    const int it = uitem[e];
    const float r = urating[e];
    const double2 an = *(const double2 *)(info + (size_t)it * 4), nn = *(const double2 *)(info + (size_t)it * 4 + 2);
    key = wkey((int)nn.y, it);                                      // info[it] = (avg, norm, adjnorm, n): one 32-B record
    const unsigned ge = ((double)r >= an.x) ? 0x80000000u : 0u;   // rating >= item average
    px = (int)((unsigned)it | ge);
    py = __float_as_int(r);
}

// descending bitonic network over groups of `width` lanes (width a power of two <= 64, uniform); pos = lane in group
__device__ __forceinline__ void bitonic_desc(int width, int pos, unsigned long long &key, int &px, int &py) {
#pragma unroll
    for (int k2 = 2; k2 <= 64; k2 <<= 1) {
        if (k2 <= width)
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const unsigned long long ok = __shfl_xor(key, j, 64);
            const int ox = __shfl_xor(px, j, 64), oy = __shfl_xor(py, j, 64);
            const bool desc = (pos & k2) == 0;
            const bool lower = (pos & j) == 0;
            const bool take_other = (lower == desc) ? (ok > key) : (ok < key);
            if (take_other) { key = ok; px = ox; py = oy; }
        }
    }
}

constexpr int SORT_LDS = 256;    // keys of a long profile staged in LDS (2 KB per wave: 8 KB per block leaves the kernel its full occupancy; 1024 had held it to 5 waves per SIMD for the sake of the few profiles of 257..1024 ratings, which now rank from the global scratch)

__device__ __forceinline__ int pow2_at_least(int d) {
    int w = 2;
    while (w < d) w <<= 1;
    return w;
}

__global__ __launch_bounds__(256) void k_sort_profiles(long long U, const long long *uptr, const int *uitem,
                                                       const float *urating, const long long *iptr, const double *info,
                                                       unsigned long long *ub_key, int2 *ub) {
    __shared__ unsigned long long lkeys[4][SORT_LDS];
    const long long u0 = ((long long)blockIdx.x * 4 + uniform((int)(threadIdx.x >> 6))) * 4;
    if (u0 >= U) return;
    const int lane = lane_id();
    const int g = lane >> 4, gl = lane & 15;
    {   // the short profiles, one per 16-lane group
        const long long u = u0 + g;
        long long a = 0;
        int d = 0;
        if (u < U) { a = uptr[u]; d = (int)(uptr[u + 1] - a); }
        const bool small = d <= 16;
        int wmax = small ? d : 0;
#pragma unroll
        for (int m = 32; m >= 16; m >>= 1) wmax = max(wmax, __shfl_xor(wmax, m, 64));
        wmax = rl32(wmax, 0);
        if (wmax > 0) {
            unsigned long long key = 0ull;   // pads sort last
            int px = 0, py = 0;
            if (small && gl < d) sort_entry(uitem, urating, iptr, info, a + gl, key, px, py);
            bitonic_desc(pow2_at_least(wmax), gl, key, px, py);
            if (small && gl < d) ub[a + gl] = make_int2(px, py);
        }
    }
    for (int q = 0; q < 4; q++) {   // the longer ones on the whole wave
        const long long u = u0 + q;
        if (u >= U) break;
        const long long a = uptr[u];
        const int d = (int)(uptr[u + 1] - a);
        if (d <= 16) continue;
        if (d <= 64) {
            unsigned long long key = 0ull;
            int px = 0, py = 0;
            if (lane < d) sort_entry(uitem, urating, iptr, info, a + lane, key, px, py);
            bitonic_desc(pow2_at_least(d), lane, key, px, py);
            if (lane < d) ub[a + lane] = make_int2(px, py);
            continue;
        }
        // longer than a wave: rank by counting.  The keys are staged in LDS
        // (or, past SORT_LDS of them, in the ub_key scratch) and every entry counts the heavier ones.
        unsigned long long *keys = d <= SORT_LDS ? lkeys[uniform((int)(threadIdx.x >> 6))] : ub_key + a;
        for (int p = lane; p < d; p += 64) {
            unsigned long long key;
            int px, py;
            sort_entry(uitem, urating, iptr, info, a + p, key, px, py);
            keys[p] = key;
        }
        __threadfence_block();
        for (int p = lane; p < d; p += 64) {
            unsigned long long key;
            int px, py;
            sort_entry(uitem, urating, iptr, info, a + p, key, px, py);
            int rank = 0;   // equal keys (an item twice in one profile: AlterEgo rows) keep their order
            for (int o = 0; o < d; o++) rank += (keys[o] > key) || (keys[o] == key && o < p);
            ub[a + rank] = make_int2(px, py);
        }
    }
}

// one thread per CSC entry (item i, its p-th rater u): position of i in u's sorted profile = number of heavier
// co-rated items = length of the prefix this rater contributes.  No atomics; raters stay in ascending user order.
__global__ __launch_bounds__(256) void k_rater_records(int I, long long nnz, const long long *iptr, const int *iuser,
                                                       const long long *uptr, const int2 *ub, RaterRec *rc, int *taken,
                                                       unsigned long long *Wp) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = p < nnz;
    int i = -1;
    long long pos_sum = 0;
    if (valid) {
        // item of CSC entry p: binary search in iptr
        int lo = 0, hi = I;
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (iptr[mid] <= p) lo = mid; else hi = mid;
        }
        i = lo;
        const int u = iuser[p];
        const long long a = uptr[u], b = uptr[u + 1];
        RaterRec r;
        r.e0 = (int)a; r.pos_ge = 0; r.rating = 0.f; r.user = u;
        for (long long e = a; e < b; e++) {
            int2 v = ub[e];
            if ((v.x & 0x7fffffff) == i) {
                // A profile may hold the item more than once (AlterEgo rows: a pass-through and a mapped rating); the
                // copies are adjacent in the sorted profile and the item then has as many CSC entries for this user:
                // each takes one copy (`taken`, zeroed, non-NULL only when the caller allows duplicates).
                if (taken && e + 1 < b && (ub[e + 1].x & 0x7fffffff) == i) {
                    e += atomicAdd(&taken[e], 1);
                    v = ub[e];
                }
                const int pos = (b - a >= 2) ? (int)(e - a) : 0;   // users with >= 2 ratings only (baselinerSim.py:184-185)
                r.pos_ge = (int)((unsigned)pos | ((unsigned)v.x & 0x80000000u));
                r.rating = __int_as_float(v.y);
                pos_sum = pos;
                break;
            }
        }
        rc[p] = r;
    }
    // W+ of the item = sum of its raters' prefix lengths (the contributions of its row): the entries of an item are
    // consecutive, so a wave adds up its runs and issues one atomic per run (exact integers: order does not matter).
    // k_plan2 had walked the rater records of every item for this sum, the popular items' 1e5 records with one wave.
    const int lane = lane_id();
    const int i_prev = __shfl_up(i, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || i != i_prev);
    long long incl = pos_sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const long long t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
    const bool seg_end = (lane == 63) || ((heads >> (lane + 1)) & 1ull);
    const int h = 63 - __clzll((long long)(heads & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull))));
    const long long before = __shfl(incl, h > 0 ? h - 1 : 0, 64);
    if (seg_end && i >= 0) {
        const long long seg = incl - (h > 0 ? before : 0);
        if (seg) atomicAdd(&Wp[i], (unsigned long long)seg);
    }
}
__device__ __forceinline__ void plan_item(int i, long long w, int I, const long long *iptr, const long long *pre, int HB,
                                          const int *hid, const int *CH, int target, int dups, int *Q, int *C,
                                          uint8_t *small, unsigned long long *Wp, int *Qcat) {
    const long long n = iptr[i + 1] - iptr[i];
    long long ge = I - pre[n < HB - 1 ? n : HB - 1];   // #{items with at least as many raters}
    const long long others = ge - 1 + (dups ? 1 : 0);   // with duplicate items a row can pair with itself
    long long bound = w < others ? w : others;
    int q = 0, c = 0;
    if (w > 0) {
        if (hid[i] >= 0) c = (int)((n + *CH - 1) / *CH);
        else q = (int)((bound + target - 1) / target);
    }
    Q[i] = q;
    C[i] = c;
    // rows with very many raters (popular items below the heavy threshold, or every popular item when there is no
    // heavy set: RecommenderSim) are bound by the walk over their raters, not by the table: class 4
    const int cls = (q >= 1 && n >= WIDE_MIN) ? 4
                    : ((q != 1) ? 0 : (bound <= SMALL_BOUND ? 1 : (bound <= 2 * SMALL_BOUND ? 3 : (bound <= MID_BOUND ? 2 : 0))));
    small[i] = (uint8_t)cls;
    Wp[i] = (unsigned long long)w;
    // the light units are listed class-major (largest tables first: their units run longest), so that each table
    // class is one contiguous range of units: Qcat[rank][i] (zero in the other classes) is what the unit scan runs over
    const int rank = class_rank(cls);
#pragma unroll
    for (int r = 0; r < N_CLASSES; r++) Qcat[(size_t)r * I + i] = (r == rank) ? q : 0;
}

__global__ __launch_bounds__(256) void k_plan2(int I, const long long *iptr, const RaterRec *rc, const long long *pre,
                                               int HB, const int *hid, const int *CH, int target, int dups, int *Q, int *C,
                                               uint8_t *small, unsigned long long *Wp, int *Qcat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;     // W+ comes summed from k_rater_records
    if (i >= I) return;
    plan_item(i, (long long)Wp[i], I, iptr, pre, HB, hid, CH, target, dups, Q, C, small, Wp, Qcat);
}

// light unit u: uq_item[u] and the record uq_q[4 u ..] = (partition, first rater, end of raters, partitions of the row) --
// what k_pair_tri needs to start, in one round trip
__global__ __launch_bounds__(256) void k_fill_units2(int I, const long long *iptr, const int *Qcat, const long long *uq_ptr,
                                                     int *uq_item, int *uq_q, const int *C, const long long *uc_ptr, int *uc_item,
                                                     int *uc_c, long long cap_light, long long cap_heavy, const int *ctl,
                                                     long long *counts) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    // what the host reads back, in one block: {light units, heavy units, first unit of class rank 0..4, light units, CH, |H|}
    // (both scans are complete: they ran in earlier launches)
    if (counts && x == 0) {
        for (int c = 0; c <= N_CLASSES; c++) counts[2 + c] = uq_ptr[(long long)c * I];
        counts[0] = uq_ptr[(long long)N_CLASSES * I];
        counts[1] = uc_ptr[I];
        counts[8] = ctl[0]; counts[9] = ctl[1];
    }
    if (x >= (long long)N_CLASSES * I) return;
    const int i = (int)(x % I);
    long long b = uq_ptr[x];
    const int nq = Qcat[x];
    if (nq > 0) {
        const int p0 = (int)iptr[i], p1 = (int)iptr[i + 1];
        for (int k = 0; k < nq && b + k < cap_light; k++) {
            uq_item[b + k] = i;
            ((int4 *)uq_q)[b + k] = make_int4(k, p0, p1, nq);
        }
    }
    if (x >= I) return;
    b = uc_ptr[i];
    for (int k = 0; k < C[i] && b + k < cap_heavy; k++) { uc_item[b + k] = i; uc_c[b + k] = k; }
}

// =================================================================================================================
// Round 3: ONE transposition per pass.  Round 2 built the CSC (count + scan + fill with returning cursor atomics), read
// it for the item statistics, and transposed a second time in k_rater_records; the mirror of the kept pairs was a third
// scatter with cursor atomics.  Now: item counts and rating sums in one pass over the CSR (k_count3) -> profiles sorted
// by weight, each entry leaving as a 16-byte sort record keyed by its item (k_sort_profiles3) -> the records moved to
// item order by the two-level tile sort (tilesort.h), where the rater records get their final form and W+ is summed ->
// item statistics from the rater records (k_item_stats3).  The CSC arrays are not built at all.
// =================================================================================================================
constexpr int CNT_SLOTS = 4096;
constexpr int CNT_CHUNK = 8192;
__device__ __forceinline__ int cnt_slot(int it) { return (int)(mix32((uint32_t)it) & (CNT_SLOTS - 1)); }

// raters per item.  Popular items (8e4 raters at BASELINE configs[1]) would serialise that many atomics on one word:
// every workgroup counts its entries in a direct-mapped LDS cache of (item, count) slots first and goes to memory once
// per occupied slot; entries whose slot is taken by another item use the global word directly.
__global__ __launch_bounds__(256) void k_count3(long long nnz, const int *uitem, int *cnt) {
    __shared__ int tag[CNT_SLOTS], loc[CNT_SLOTS];
    for (int t = threadIdx.x; t < CNT_SLOTS; t += 256) { tag[t] = -1; loc[t] = 0; }
    __syncthreads();
    const long long e0 = (long long)blockIdx.x * CNT_CHUNK;
    for (int q = threadIdx.x; q < CNT_CHUNK; q += 256) {
        const long long e = e0 + q;
        if (e >= nnz) break;
        const int it = uitem[e];
        const int sl = cnt_slot(it);
        const int old = atomicCAS(&tag[sl], -1, it);
        if (old == -1 || old == it) atomicAdd(&loc[sl], 1); else atomicAdd(&cnt[it], 1);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < CNT_SLOTS; t += 256)
        if (loc[t]) atomicAdd(&cnt[tag[t]], loc[t]);
}

// Sort records (tilesort.h: key = low 32 bits of word 0).  Narrow (float ratings): {item, pos | flag << 31, rating bits,
// user}.  Wide (fp64 ratings -- RecommenderSim over AlterEgo means, core/recommenderSim.py:64-133 takes np.float64): {item,
// pos | flag, rating (8 B), user, -}.

// The mutuality flag (rating >= item average) needs the item averages, which come out of the rater records this sort
// feeds: the profile copy and the sort records leave without it, k_item_stats3 sets it in the rater records and
// k_ub_flags in the profile copy.
template <bool WIDE>
__device__ __forceinline__ void sort_entry3(const int *uitem, const float *ur32, const double *ur64, const int *cnt,
                                            long long e, unsigned long long &key, int &px, long long &py) {
    const int it = uitem[e];
    key = wkey(cnt[it], it);
    px = it;
    py = WIDE ? __double_as_longlong(ur64[e]) : (long long)(unsigned)__float_as_int(ur32[e]);
}

// v of lane ^ J.  Partners inside a row of 16 lanes come through the data-parallel lane selects of the vector unit, which
// cost no LDS turn and no wait: quad permutations for 1 and 2, half-row mirror then quad reversal for 4 (7 ^ 3), a row
// rotation by 8 for 8.  All 64 lanes are active wherever the networks run.
template <int J>
__device__ __forceinline__ int xor_lane(int v) {
    if constexpr (J == 1) return __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, true);            // quad_perm:[1,0,3,2]
    else if constexpr (J == 2) return __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, true);       // quad_perm:[2,3,0,1]
    else if constexpr (J == 4) {
        const int h = __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, true);                     // row_half_mirror
        return __builtin_amdgcn_update_dpp(h, h, 0x1B, 0xF, 0xF, true);                             // quad_perm:[3,2,1,0]
    } else if constexpr (J == 8) return __builtin_amdgcn_update_dpp(v, v, 0x128, 0xF, 0xF, true);    // row_ror:8
    else return __shfl_xor(v, J, 64);
}

// the compare-exchange steps J, J / 2 .. 1 of merge level K2: the lane keeps the larger of the two keys where the network wants
// the larger one, the smaller where it wants the smaller one, its own on a tie.  The key's low word is the item, so the rating is
// all that travels with it.
template <bool WIDE, int K2, int J>
__device__ __forceinline__ void bitonic_steps3(int pos, unsigned long long &key, long long &py) {
    if constexpr (J > 0) {
        const unsigned long long ok = (unsigned long long)(unsigned)xor_lane<J>((int)(unsigned)key) |
                                      ((unsigned long long)(unsigned)xor_lane<J>((int)(key >> 32)) << 32);
        long long oy = (long long)(unsigned)xor_lane<J>((int)(unsigned long long)py);
        if (WIDE) oy |= (long long)((unsigned long long)(unsigned)xor_lane<J>((int)((unsigned long long)py >> 32)) << 32);
        const bool desc = (pos & K2) == 0;
        const bool lower = (pos & J) == 0;
        const bool take_other = (lower == desc) ? (ok > key) : (ok < key);
        key = take_other ? ok : key;
        py = take_other ? oy : py;
        bitonic_steps3<WIDE, K2, J / 2>(pos, key, py);
    }
}

// descending bitonic network over groups of `width` lanes (width a power of two <= 64, uniform); pos = lane in group
template <bool WIDE, int K2 = 2>
__device__ __forceinline__ void bitonic_desc3(int width, int pos, unsigned long long &key, long long &py) {
    if constexpr (K2 <= 64) {
        if (K2 > width) return;
        bitonic_steps3<WIDE, K2, K2 / 2>(pos, key, py);
        bitonic_desc3<WIDE, K2 * 2>(width, pos, key, py);
    }
}

// one sorted entry at position `rank` of user u's profile [a, a + d): the profile copy the pair kernel walks and the sort
// record that becomes the item's rater record
template <bool WIDE>
__device__ __forceinline__ void emit_entry3(long long a, int d, int rank, long long u, int px, long long py, void *ub,
                                            unsigned long long *srec) {
    const long long e = a + rank;
    const unsigned pos_ge = (unsigned)(d >= 2 ? rank : 0) | ((unsigned)px & 0x80000000u);   // users with >= 2 ratings only (:184-185)
    const unsigned long long w0 = (unsigned long long)((unsigned)px & 0x7fffffffu) | ((unsigned long long)pos_ge << 32);
    if (WIDE) {
        UbWide v; v.item_ge = px; v.pad = 0; v.rating = __longlong_as_double(py);
        ((UbWide *)ub)[e] = v;
        srec[e * 3 + 0] = w0; srec[e * 3 + 1] = (unsigned long long)py; srec[e * 3 + 2] = (unsigned long long)(unsigned)u;
    } else {
        ((int2 *)ub)[e] = make_int2(px, (int)py);
        ulonglong2 w; w.x = w0; w.y = (unsigned long long)(unsigned)py | ((unsigned long long)(unsigned)u << 32);
        *(ulonglong2 *)(srec + e * 2) = w;
    }
}

// The round-3 sort.  A wave takes SORT_NB consecutive users and asks for everything it will need before it uses any of
// it: the SORT_NB + 1 profile starts in one load; the entries of its short profiles (up to 16 ratings; SORT_NB / 4 rounds of
// four, one profile per 16-lane group) and of the first SORT_MB profiles of 17..64 ratings (one per wave) with clamped,
// unconditional loads; then every rater-count gather; then the networks, which are independent chains; then the stores.
// The network of a round is cut off at the round's longest profile, that of a whole-wave profile at its length, as in
// k_sort_profiles; profiles above 64 ratings follow one by one, ranked by counting.
constexpr int SORT_NB = 16;
constexpr int SORT_MB = 4;

template <bool WIDE>
__device__ __forceinline__ void entry_load3(const int *uitem, const float *ur32, const double *ur64, long long e, int &it,
                                            long long &py) {
    it = uitem[e];
    py = WIDE ? __double_as_longlong(ur64[e]) : (long long)(unsigned)__float_as_int(ur32[e]);
}

// up to SORT_MB profiles of 17..64 ratings, one per wave-wide network: k[m] = the user's place in the batch or -1
struct MidGroup {
    int k[SORT_MB], a[SORT_MB], d[SORT_MB];     // uniform
    int it[SORT_MB], c[SORT_MB];
    long long py[SORT_MB];
};

template <bool WIDE>
__global__ __launch_bounds__(256) void k_sort_profiles3(long long U, const long long *uptr, const int *uitem, const float *ur32,
                                                        const double *ur64, const int *cnt, unsigned long long *ub_key,
                                                        void *ub, unsigned long long *srec) {
    __shared__ unsigned long long lkeys[4][SORT_LDS];
    constexpr int ROUNDS = SORT_NB / 4;
    const int wv = uniform((int)(threadIdx.x >> 6));
    const long long u0 = ((long long)blockIdx.x * 4 + wv) * SORT_NB;
    if (u0 >= U) return;
    const int lane = lane_id();
    const int g = lane >> 4, gl = lane & 15;
    // lane k: start and length of user u0 + k (an empty profile past the last user).  nnz < 2^31 (xmap_sim3_layout)
    const long long ul = u0 + lane;
    const int pa = (int)uptr[ul < U ? ul : U];
    const int dl = __shfl_down(pa, 1, 64) - pa;
    unsigned midm = (unsigned)__ballot(lane < SORT_NB && dl > 16 && dl <= 64);
    const unsigned longm = (unsigned)__ballot(lane < SORT_NB && dl > 64);

    MidGroup M;
    auto mid_request = [&]() {
#pragma unroll
        for (int m = 0; m < SORT_MB; m++) {
            M.k[m] = midm ? __ffs(midm) - 1 : -1;
            midm &= midm - 1;
            const int k = M.k[m] >= 0 ? M.k[m] : 0;
            M.a[m] = rl32(pa, k);
            M.d[m] = M.k[m] >= 0 ? rl32(dl, k) : 0;
            entry_load3<WIDE>(uitem, ur32, ur64, lane < M.d[m] ? (long long)M.a[m] + lane : 0ll, M.it[m], M.py[m]);
        }
    };
    auto mid_gather = [&]() {
#pragma unroll
        for (int m = 0; m < SORT_MB; m++) M.c[m] = cnt[M.it[m]];
    };
    auto mid_finish = [&]() {
#pragma unroll
        for (int m = 0; m < SORT_MB; m++) {
            if (M.k[m] < 0) continue;
            const int d = M.d[m];
            const long long a = M.a[m], u = u0 + M.k[m];
            const bool on = lane < d;
            unsigned long long key = on ? wkey(M.c[m], M.it[m]) : 0ull;   // pads sort last
            long long py = on ? M.py[m] : 0ll;
            bitonic_desc3<WIDE>(pow2_at_least(d), lane, key, py);
            if (on) emit_entry3<WIDE>(a, d, lane, u, (int)(unsigned)key, py, ub, srec);
        }
    };

    // requests: the short profiles' entries, the first whole-wave profiles' entries
    int sa[ROUNDS], sd[ROUNDS], sit[ROUNDS], sc[ROUNDS];
    long long spy[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        sa[r] = __shfl(pa, r * 4 + g, 64);
        sd[r] = __shfl(dl, r * 4 + g, 64);
        const bool on = sd[r] <= 16 && gl < sd[r];
        entry_load3<WIDE>(uitem, ur32, ur64, on ? (long long)sa[r] + gl : 0ll, sit[r], spy[r]);
    }
    mid_request();
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) sc[r] = cnt[sit[r]];
    mid_gather();

#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        const long long u = u0 + r * 4 + g;
        const int d = sd[r];
        const bool small = d <= 16, on = small && gl < d;
        int wmax = 0;                       // the longest short profile of the round (uniform)
#pragma unroll
        for (int x = 0; x < 4; x++) {
            const int dx = rl32(dl, r * 4 + x);
            wmax = max(wmax, dx <= 16 ? dx : 0);
        }
        if (wmax > 0) {
            unsigned long long key = on ? wkey(sc[r], sit[r]) : 0ull;   // pads sort last
            long long py = on ? spy[r] : 0ll;
            bitonic_desc3<WIDE>(pow2_at_least(wmax), gl, key, py);
            if (on) emit_entry3<WIDE>(sa[r], d, gl, u, (int)(unsigned)key, py, ub, srec);
        }
    }
    for (;;) {
        mid_finish();
        if (!midm) break;
        mid_request();
        mid_gather();
    }

    // longer than a wave: rank by counting.  The keys are staged in LDS (or, past SORT_LDS of them, in the ub_key scratch) and
    // every entry counts the heavier ones.
    for (unsigned lm = longm; lm; lm &= lm - 1) {
        const int k = __ffs(lm) - 1;
        const long long a = rl32(pa, k), u = u0 + k;
        const int d = rl32(dl, k);
        unsigned long long *keys = d <= SORT_LDS ? lkeys[wv] : ub_key + a;
        for (int p = lane; p < d; p += 64) {
            unsigned long long key;
            int px;
            long long py;
            sort_entry3<WIDE>(uitem, ur32, ur64, cnt, a + p, key, px, py);
            keys[p] = key;
        }
        __threadfence_block();
        for (int p = lane; p < d; p += 64) {
            unsigned long long key;
            int px;
            long long py;
            sort_entry3<WIDE>(uitem, ur32, ur64, cnt, a + p, key, px, py);
            int rank = 0;   // equal keys (an item twice in one profile: AlterEgo rows) keep their order
            for (int o = 0; o < d; o++) rank += (keys[o] > key) || (keys[o] == key && o < p);
            emit_entry3<WIDE>(a, d, rank, u, px, py, ub, srec);
        }
    }
}

// final form of a rater record from its sort record: e0 = first entry of the user's profile
template <bool WIDE>
__device__ __forceinline__ unsigned rater_user(const unsigned long long *w) { return WIDE ? (unsigned)w[2] : (unsigned)(w[1] >> 32); }
template <bool WIDE>
__device__ __forceinline__ ulonglong2 rater_record_at(const unsigned long long *w, unsigned e0) {
    ulonglong2 o;
    o.x = (unsigned long long)e0 | (w[0] & 0xffffffff00000000ull);     // {e0, pos | flag}
    o.y = w[1];                                                        // narrow: {rating bits, user}; wide: the fp64 rating
    return o;
}
template <bool WIDE>
__device__ __forceinline__ ulonglong2 rater_record(const unsigned long long *w, const long long *uptr) {
    return rater_record_at<WIDE>(w, (unsigned)uptr[rater_user<WIDE>(w)]);
}

// level C of the rater records: one workgroup per tile.  The small keys' records are ranked by LDS cursors, converted,
// laid out in final order in LDS and written as whole rows; W+ of every small key (sum of its raters' prefix lengths = the
// contributions of its row) is summed on the way.
template <bool WIDE>
__global__ __launch_bounds__(ts::CT) void k_rc_tiles(ts::Geo G, const unsigned long long *bufB, const long long *uptr,
                                                     ulonglong2 *rc, unsigned long long *Wp) {
    constexpr int RW = WIDE ? 3 : 2;
    __shared__ unsigned cur[ts::NK_MAX], kst[ts::NK_MAX];
    __shared__ unsigned long long wsum[ts::NK_MAX];
    __shared__ ulonglong2 lrec[ts::CAP];
    const ts::TileHead h = ts::tile_head(G, blockIdx.x);
    if (h.nk <= 0) return;
    for (int x = threadIdx.x; x < h.nk; x += ts::CT) {
        cur[x] = 0u; wsum[x] = 0ull;
        kst[x] = (unsigned)(G.ptr[h.k0 + x] - h.pos0);
    }
    __syncthreads();
    const bool in_lds = h.n <= ts::CAP;
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
            atomicAdd(&wsum[kk], (unsigned long long)((unsigned)(w[t][0] >> 32) & 0x7fffffffu));
            const ulonglong2 o = rater_record<WIDE>(w[t], uptr);
            if (in_lds) lrec[q] = o; else rc[h.pos0 + q] = o;
        }
    }
    __syncthreads();
    if (in_lds)
        for (int q = threadIdx.x; q < h.n; q += ts::CT) rc[h.pos0 + q] = lrec[q];
    for (int x = threadIdx.x; x < h.nk; x += ts::CT) Wp[h.k0 + x] = wsum[x];
}

// the large keys' rater records, written by level B (tilesort.h: the finisher) at their final position; W+ of a large key is
// summed per workgroup in LDS and added once (Wp is cleared before the sort, k_rc_tiles stores the small keys' only)
template <bool WIDE>
struct RcFin {
    static constexpr int RW = WIDE ? 3 : 2;
    static constexpr bool STATE = false, WSUM = true;
    const long long *__restrict__ uptr; ulonglong2 *__restrict__ rc; unsigned long long *Wp;
    __device__ __forceinline__ long long state(const ts::Geo &, int) const { return 0; }
    __device__ __forceinline__ unsigned gather(const unsigned long long (&w)[RW]) const { return (unsigned)uptr[rater_user<WIDE>(w)]; }
    __device__ __forceinline__ unsigned long long store(long long, long long p, const unsigned long long (&w)[RW], unsigned e0) const {
        rc[p] = rater_record_at<WIDE>(w, e0);
        return (unsigned long long)((unsigned)(w[0] >> 32) & 0x7fffffffu);
    }
    __device__ __forceinline__ void flush(int k, unsigned long long sum) const { if (sum) atomicAdd(&Wp[k], sum); }
};

// item statistics from the rater records (item_stats.h); the records' mutuality flags are set once the average is known
struct RcSrc {
    RaterRec *rc; const double *u_avg;
    static constexpr bool has_flags = true;
    __device__ __forceinline__ void load(long long p, double &r, int &u) const { const RaterRec x = rc[p]; r = (double)x.rating; u = x.user; }
    __device__ __forceinline__ double uavg(int u) const { return u_avg[u]; }
    __device__ __forceinline__ void set_flag(long long p, bool ge) const { if (ge) rc[p].pos_ge |= (int)0x80000000u; }
    // whole records (item_stats_records): one 16-byte load holds the rating, the user and the flag word
    typedef RaterRec Rec;
    __device__ __forceinline__ Rec rec(long long p) const { return rc[p]; }
    static __device__ __forceinline__ double rating(const Rec &x) { return (double)x.rating; }
    static __device__ __forceinline__ int user(const Rec &x) { return x.user; }
    __device__ __forceinline__ void raise_flag(long long p, const Rec &x) const { rc[p].pos_ge = (int)((unsigned)x.pos_ge | 0x80000000u); }
};
struct RcWideSrc {
    const RaterRecWide *rc;
    static constexpr bool has_flags = false;       // RecommenderSim has no mutuality
    __device__ __forceinline__ void load(long long p, double &r, int &u) const { r = rc[p].rating; u = 0; }
    __device__ __forceinline__ double uavg(int) const { return 0.0; }
    __device__ __forceinline__ void set_flag(long long, bool) const {}
    typedef RaterRecWide Rec;
    __device__ __forceinline__ Rec rec(long long p) const { return rc[p]; }
    static __device__ __forceinline__ double rating(const Rec &x) { return x.rating; }
    static __device__ __forceinline__ int user(const Rec &) { return 0; }
    __device__ __forceinline__ void raise_flag(long long, const Rec &) const {}
};

// Items with more than STAT_BIG raters (up to 1e5 at BASELINE configs[1]: one wave walking them was the kernel's tail, and
// the unrolled walk they need cost every wave of the kernel its registers) are
// cut into chunks of STAT_CHK raters: k_item_stats3 lists them, k_item_chunks sums every chunk on a wave of its own,
// k_item_big adds an item's chunk sums up in chunk order (the adjusted norm exactly) and finishes it, k_item_big_flags sets
// the flags of its rater records.
constexpr int STAT_BIG = 512;
constexpr int STAT_CHK = 2048;
struct BigList {
    unsigned *counters;       // [0] chunks listed, [1] big items listed
    int2 *chunks;             // (item, chunk)
    int4 *items;              // (item, first chunk, chunks, -)
    double *part;             // [chunk][ITEM_PART]
    long long chunk_cap, item_cap;
};

template <typename Src>
__global__ __launch_bounds__(256) void k_item_stats3(int I, int lo, int hi, const long long *iptr, const Src src, double *info,
                                                     double *norms, BigList B) {
    const int i0 = lo + (blockIdx.x * 4 + uniform((int)(threadIdx.x >> 6))) * 4;
    if (i0 >= hi) return;
    const int lane = lane_id();
    // lane k: where the records of item i0 + k start and how many there are (none past the range); one load for the wave
    const long long pl = iptr[min(i0 + lane, hi)];
    const long long nl = __shfl_down(pl, 1, 64) - pl;
    {   // up to 64 raters: four items at a time, one per 16-lane group, four records a lane
        const int i = i0 + (lane >> 4);
        const long long p0 = __shfl(pl, lane >> 4, 64), n = __shfl(nl, lane >> 4, 64);
        item_stats_records<16, 4, Src>(i < hi && n <= 64, i, lane & 15, I, p0, p0 + n, src, info, norms);
    }
    for (int t = 0; t < 4; t++) {
        const int i = i0 + t;
        if (i >= hi) break;
        const long long n = rl64(nl, t);
        if (n <= 64) continue;
        if (n > STAT_BIG) {
            if (lane == 0) {
                const int nch = (int)((n + STAT_CHK - 1) / STAT_CHK);
                const unsigned base = atomicAdd(&B.counters[0], (unsigned)nch);
                const unsigned slot = atomicAdd(&B.counters[1], 1u);
                if ((long long)slot < B.item_cap) B.items[slot] = make_int4(i, (int)base, nch, 0);
                for (int x = 0; x < nch; x++)
                    if ((long long)base + x < B.chunk_cap) B.chunks[base + x] = make_int2(i, x);
            }
            continue;
        }
        item_stats_group<64, Src, false>(true, i, lane, I, iptr, src, info, norms, nullptr, nullptr);     // 65 .. STAT_BIG: the whole wave walks
    }
}

// one wave per listed chunk: the item's partial sums over raters [c STAT_CHK, (c + 1) STAT_CHK)
template <typename Src>
__global__ __launch_bounds__(256) void k_item_chunks(const long long *iptr, const Src src, BigList B) {
    const unsigned c = blockIdx.x * 4 + uniform((int)(threadIdx.x >> 6));
    if (c >= B.counters[0]) return;
    const int2 d = B.chunks[c];
    const int lane = lane_id();
    const long long p0 = iptr[d.x] + (long long)d.y * STAT_CHK;
    const long long p1 = min(iptr[d.x + 1], p0 + STAT_CHK);
    constexpr int UN = 8;
    double s = 0.0, slo = 0.0, q = 0.0, qlo = 0.0, a2 = 0.0, a2lo = 0.0;
    for (long long p = p0 + lane; p < p1; p += 64 * UN) {
        double rr[UN], av[UN];
        int uu[UN];
#pragma unroll
        for (int t = 0; t < UN; t++) {
            rr[t] = 0.0; uu[t] = -1;
            if (p + 64 * t < p1) src.load(p + 64 * t, rr[t], uu[t]);
        }
#pragma unroll
        for (int t = 0; t < UN; t++) av[t] = uu[t] >= 0 ? src.uavg(uu[t]) : 0.0;
#pragma unroll
        for (int t = 0; t < UN; t++) {
            if (uu[t] < 0) continue;
            const double dlt = rr[t] - av[t];
            dd_add(s, slo, rr[t]);
            dd_add(q, qlo, rr[t] * rr[t]);
            dd_add(a2, a2lo, dlt * dlt);
        }
    }
    dd_reduce<64>(s, slo);
    dd_reduce<64>(q, qlo);
    dd_reduce<64>(a2, a2lo);
    if (lane == 0) {
        double *o = B.part + (size_t)c * ITEM_PART;
        o[0] = s; o[1] = slo; o[2] = q; o[3] = qlo; o[4] = a2; o[5] = a2lo; o[6] = (double)(p1 - p0);
    }
}

__global__ __launch_bounds__(64) void k_item_big(int I, BigList B, double *info, double *norms) {
    const unsigned b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B.counters[1]) return;
    const int4 d = B.items[b];
    double s = 0.0, slo = 0.0, q = 0.0, qlo = 0.0, a2 = 0.0, a2lo = 0.0, n = 0.0;
    for (int x = 0; x < d.z; x++) {
        const double *o = B.part + (size_t)(d.y + x) * ITEM_PART;
        dd_add(s, slo, o[0]);
        dd_add(s, slo, o[1]);
        dd_add(q, qlo, o[2]);
        dd_add(q, qlo, o[3]);
        dd_add(a2, a2lo, o[4]);
        dd_add(a2, a2lo, o[5]);
        n += o[6];
    }
    const int i = d.x;
    info[(size_t)i * 4 + 0] = (n > 0.0) ? 1.0 * s / n : 0.0;
    info[(size_t)i * 4 + 1] = sqrt(q);
    info[(size_t)i * 4 + 2] = sqrt(a2);
    info[(size_t)i * 4 + 3] = 1.0 * n;
    norms[i] = sqrt(q);
    norms[(size_t)I + i] = sqrt(a2);
}

template <typename Src>
__global__ __launch_bounds__(256) void k_item_big_flags(const long long *iptr, const Src src, BigList B, const double *info) {
    const unsigned c = blockIdx.x * 4 + uniform((int)(threadIdx.x >> 6));
    if (c >= B.counters[0]) return;
    const int2 d = B.chunks[c];
    const double avg = info[(size_t)d.x * 4];
    const long long p0 = iptr[d.x] + (long long)d.y * STAT_CHK;
    const long long p1 = min(iptr[d.x + 1], p0 + STAT_CHK);
    for (long long p = p0 + lane_id(); p < p1; p += 64) {
        double r; int u;
        src.load(p, r, u);
        src.set_flag(p, r >= avg);
    }
}

// the rater records' flags from the complete item info (sharded item statistics: a rank's k_item_stats3 flagged the records
// of ITS items only; after the all-gather of the item info every record is done here -- idempotent).  A record knows its
// profile entry (e0 + position), the entry knows its item.
__global__ __launch_bounds__(256) void k_rc_flags(long long nnz, RaterRec *rc, const int2 *ub, const double *info) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const RaterRec r = rc[p];
    const int it = ub[(long long)r.e0 + (r.pos_ge & 0x7fffffff)].x & 0x7fffffff;
    if ((double)r.rating >= info[(size_t)it * 4]) rc[p].pos_ge = (int)((unsigned)r.pos_ge | 0x80000000u);
}

// the profile copy's flags: rating >= average of the entry's item
__global__ __launch_bounds__(256) void k_ub_flags(long long nnz, int2 *ub, const double *info) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int2 v = ub[e];
    if ((double)__int_as_float(v.y) >= info[(size_t)v.x * 4]) ub[e].x = (int)((unsigned)v.x | 0x80000000u);
}

}  // namespace xmap

using namespace xmap;

namespace {

// rater-count histogram -> pre[v] = #items with fewer than v raters (partner bounds), ctl = {CH, |H|, -, -}, the heavy set hid / hlist
void heavy_set_fills(FillList &F, int64_t n_users, int32_t *hist, int32_t *ctl) {
    F.add(hist, sizeof(int32_t) * (size_t)(n_users + 2));
    F.add(ctl, sizeof(int32_t), 0x7f7f7f7fu);                       // CH = 0x7f7f7f7f: "no heavy rows"
    F.add(ctl + 1, 3 * sizeof(int32_t));
}
// filled: the caller has cleared hist and ctl already (heavy_set_fills in a launch of its own)
int heavy_set(void *stream, int I, int64_t n_users, const int64_t *item_ptr, int32_t ch_min, int32_t *hist, int64_t *pre, int32_t *ctl,
              int32_t *hid, int32_t *hlist, bool filled = false) {
    hipStream_t st = (hipStream_t)stream;
    const int HB = (int)n_users + 2;
    if (!filled) {
        FillList F;
        heavy_set_fills(F, n_users, hist, ctl);
        int rc = fill_multi(st, F);
        if (rc) return rc;
    }
    if (I > 0) {
        k_hist<<<dim3((unsigned)((I + 256 * HIST_PER - 1) / (256 * HIST_PER))), dim3(256), 0, st>>>(I, (const long long *)item_ptr, HB, hist);
        XM_LAUNCH_CHECK();
    }
    int rcode = xmap_exclusive_scan_i32_to_i64(stream, hist, pre, HB, nullptr);
    if (rcode) return rcode;
    if (HB - 1 > ch_min) {
        k_threshold<<<dim3((unsigned)((HB + 255) / 256)), dim3(256), 0, st>>>(I, HB, (const long long *)pre, ch_min, ctl);
        XM_LAUNCH_CHECK();
    }
    if (I > 0) {
        k_mark_heavy<<<dim3((unsigned)((I + 255) / 256)), dim3(256), 0, st>>>(I, (const long long *)item_ptr, ctl, hid, hlist, ctl + 1);
        XM_LAUNCH_CHECK();
    }
    return XMAP_OK;
}

// h_ctl (host, [2]) = {CH, |H|}: the copy, the wait for the stream (and whatever else the caller queued on it), the |H| check
int read_heavy_ctl(hipStream_t st, const int32_t *ctl, int32_t *h_ctl) {
    XM_HIP(hipMemcpyAsync(h_ctl, ctl, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_ctl[1] > HMAX) {
        set_error("heavy set larger than %d", HMAX);
        return XMAP_ERR_OVERFLOW;
    }
    return XMAP_OK;
}

// first half of both plan entry points: partitions, chunks and table class of every row (k_plan2), the scans of the light
// (class-major) and the heavy units.  h_light / h_heavy (host, or NULL): their totals -- a scan that reports it synchronises
int plan_rows(void *stream, const xmap_ratings *R, int32_t slot_target, const void *rc, const int64_t *pre, const int32_t *hid,
              const int32_t *ctl, int32_t *Q, int32_t *C, uint8_t *small, uint64_t *Wp, int32_t *Qcat, int64_t *uq_ptr, int64_t *uc_ptr,
              int32_t dups, int64_t *h_light, int64_t *h_heavy) {
    XM_ARG(slot_target > 0 && slot_target <= T_SLOTS);
    hipStream_t st = (hipStream_t)stream;
    const int I = R->n_items;
    if (I > 0) {            // (k_plan2 writes every class slot of every item: no fill of Qcat)
        k_plan2<<<dim3((unsigned)((I + 255) / 256)), dim3(256), 0, st>>>(
            I, (const long long *)R->item_ptr, (const RaterRec *)rc, (const long long *)pre, (int)R->n_users + 2, hid, ctl, slot_target, dups,
            Q, C, small, (unsigned long long *)Wp, Qcat);
        XM_LAUNCH_CHECK();
    }
    int rcode = xmap_exclusive_scan_i32_to_i64(stream, Qcat, uq_ptr, (int64_t)N_CLASSES * I, h_light);
    if (rcode) return rcode;
    return xmap_exclusive_scan_i32_to_i64(stream, C, uc_ptr, I, h_heavy);
}

// sort records (RW words each) -> rater records in item order through the two binning levels of the tile sort, W+ summed
template <int RW>
int sort_rater_records(hipStream_t st, const ts::Geo &G, long long nnz, const void *srec, void *bufA, void *bufB, const int64_t *user_ptr,
                       void *rc, uint64_t *Wp) {
    constexpr bool WIDE = RW == 3;
    const dim3 gridA((unsigned)((nnz + G.ch - 1) / G.ch)), gridB((unsigned)G.clist_cap);
    ts::RecLoader<RW> LA{(const unsigned long long *)srec}, LB{(const unsigned long long *)bufA};
    RcFin<WIDE> FB{(const long long *)user_ptr, (ulonglong2 *)rc, (unsigned long long *)Wp};
    ts::k_ts_bin<RW, false, ts::RecLoader<RW>, ts::NoFin><<<gridA, dim3(ts::BT), 0, st>>>(G, LA, nnz, (unsigned long long *)bufA, ts::NoFin{});
    XM_LAUNCH_CHECK();
    // level B: the tiles' small parts to bufB, the large keys' records to rc (+ their W+)
    ts::k_ts_bin<RW, true, ts::RecLoader<RW>, RcFin<WIDE>><<<gridB, dim3(ts::BT), 0, st>>>(G, LB, nnz, (unsigned long long *)bufB, FB);
    XM_LAUNCH_CHECK();
    k_rc_tiles<WIDE><<<dim3((unsigned)G.T), dim3(ts::CT), 0, st>>>(G, (const unsigned long long *)bufB, (const long long *)user_ptr,
                                                                  (ulonglong2 *)rc, (unsigned long long *)Wp);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

// item statistics of [lo, hi) from the rater records behind src, big items in chunks; the records' flags where they have any
template <typename Src>
int item_stats3(hipStream_t st, int I, int lo, int hi, const int64_t *item_ptr, const Src &src, double *info, double *norms,
                const BigList &B) {
    const long long *iptr = (const long long *)item_ptr;
    const dim3 grid((unsigned)((hi - lo + 15) / 16)), gridC((unsigned)((B.chunk_cap + 3) / 4)), gridI((unsigned)((B.item_cap + 63) / 64));
    k_item_stats3<Src><<<grid, dim3(256), 0, st>>>(I, lo, hi, iptr, src, info, norms, B);
    XM_LAUNCH_CHECK();
    k_item_chunks<Src><<<gridC, dim3(256), 0, st>>>(iptr, src, B);
    XM_LAUNCH_CHECK();
    k_item_big<<<gridI, dim3(64), 0, st>>>(I, B, info, norms);
    XM_LAUNCH_CHECK();
    if constexpr (Src::has_flags) {
        k_item_big_flags<Src><<<gridC, dim3(256), 0, st>>>(iptr, src, B, info);
        XM_LAUNCH_CHECK();
    }
    return XMAP_OK;
}

}  // namespace

extern "C" {

int xmap_sim2_layout(void *stream, const xmap_ratings *R, const double *info, int32_t ch_min, int32_t *hist /*[U+2]*/,
                     int64_t *pre /*[U+3]*/, int32_t *ctl /*[4]: CH, n_heavy*/, int32_t *hid, int32_t *hlist /*[1024]*/,
                     uint64_t *ub_key /*[nnz] scratch*/, void *ub /*[nnz] 8 B*/, void *rc /*[nnz] 16 B*/,
                     uint64_t *Wp /*[I] out*/, int32_t dups, int32_t *h_ctl /*[2]*/) {
    XM_ARG(R && info && hist && pre && ctl && hid && hlist && ub_key && ub && rc && Wp && ch_min >= 64);
    XM_ARG(R->nnz < 0x7fffffffLL && R->n_users < 0x7ffffff0LL);
    hipStream_t st = (hipStream_t)stream;
    const int I = R->n_items;
    int rcode = heavy_set(stream, I, R->n_users, R->item_ptr, ch_min, hist, pre, ctl, hid, hlist);
    if (rcode) return rcode;
    if (R->n_users > 0) {
        k_sort_profiles<<<dim3((unsigned)((R->n_users + 15) / 16)), dim3(256), 0, st>>>(
            R->n_users, (const long long *)R->user_ptr, R->user_item, R->user_rating, (const long long *)R->item_ptr, info,
            (unsigned long long *)ub_key, (int2 *)ub);
        XM_LAUNCH_CHECK();
    }
    XM_HIP(hipMemsetAsync(Wp, 0, sizeof(uint64_t) * (size_t)(I > 0 ? I : 1), st));
    if (R->nnz > 0) {
        // profiles that may hold an item twice: the sort is done with ub_key, which then serves as the (zeroed) copy
        // counters of k_rater_records
        if (dups) XM_HIP(hipMemsetAsync(ub_key, 0, sizeof(int32_t) * (size_t)R->nnz, st));
        k_rater_records<<<dim3((unsigned)((R->nnz + 255) / 256)), dim3(256), 0, st>>>(
            I, R->nnz, (const long long *)R->item_ptr, R->item_user, (const long long *)R->user_ptr, (const int2 *)ub,
            (RaterRec *)rc, dups ? (int *)ub_key : nullptr, (unsigned long long *)Wp);
        XM_LAUNCH_CHECK();
    }
    return h_ctl ? read_heavy_ctl(st, ctl, h_ctl) : XMAP_OK;
}

int xmap_sim2_plan(void *stream, const xmap_ratings *R, int32_t slot_target, const void *rc, const int64_t *pre,
                   const int32_t *hid, const int32_t *ctl, int32_t *Q, int32_t *C, uint8_t *small, uint64_t *Wp /*[I] out*/,
                   int32_t *Qcat /*[4 I]*/, int64_t *uq_ptr /*[4 I + 1]*/, int64_t *uc_ptr, int32_t dups,
                   int64_t *h_counts /*[8]: light units, heavy units, first unit of table class rank 0..4, light units*/) {
    XM_ARG(R && rc && Wp && pre && hid && ctl && Q && C && small && Qcat && uq_ptr && uc_ptr && h_counts);
    hipStream_t st = (hipStream_t)stream;
    const int I = R->n_items;
    int rcode = plan_rows(stream, R, slot_target, rc, pre, hid, ctl, Q, C, small, Wp, Qcat, uq_ptr, uc_ptr, dups, &h_counts[0], &h_counts[1]);
    if (rcode) return rcode;
    // class boundaries uq_ptr[c I], c = 0..4: one strided copy (the scan above has synchronised the stream)
    if (I > 0)
        XM_HIP(hipMemcpy2DAsync(&h_counts[2], sizeof(int64_t), uq_ptr, sizeof(int64_t) * (size_t)I, sizeof(int64_t),
                                N_CLASSES, hipMemcpyDeviceToHost, st));
    else
        for (int c = 0; c < N_CLASSES; c++) h_counts[2 + c] = 0;
    XM_HIP(hipStreamSynchronize(st));
    h_counts[2 + N_CLASSES] = h_counts[0];
    return XMAP_OK;
}

int xmap_sim2_units(void *stream, int32_t n_items, const int64_t *item_ptr, const int32_t *Qcat, const int64_t *uq_ptr,
                    int32_t *uq_item, int32_t *uq_q, const int32_t *C, const int64_t *uc_ptr, int32_t *uc_item, int32_t *uc_c) {
    XM_ARG(item_ptr && Qcat && uq_ptr && uq_item && uq_q && C && uc_ptr && uc_item && uc_c);
    if (n_items == 0) return XMAP_OK;
    k_fill_units2<<<dim3((unsigned)(((long long)N_CLASSES * n_items + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        n_items, (const long long *)item_ptr, Qcat, (const long long *)uq_ptr, uq_item, uq_q, C, (const long long *)uc_ptr, uc_item, uc_c, 0x7fffffffffffffffLL,
        0x7fffffffffffffffLL, nullptr, nullptr);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

/* xmap_sim2_plan + xmap_sim2_units with ONE host wait (include/xmap_hip.h): the scans leave their totals on the device, the unit
 * kernel gathers everything the host reads into one block, and that block travels to pinned memory with an event behind it.
 * begin queues all of it; wait takes the event.  What the caller queues in between runs while the host waits and reads. */
int xmap_sim3_plan_begin(void *stream, const xmap_ratings *R, int32_t slot_target, const int64_t *pre, const int32_t *hid,
                         const int32_t *ctl, int32_t *Q, int32_t *C, uint8_t *small, uint64_t *Wp, int32_t *Qcat, int64_t *uq_ptr,
                         int64_t *uc_ptr, int32_t dups, int32_t *uq_item, int32_t *uq_q, int32_t *uc_item, int32_t *uc_c,
                         int64_t cap_light, int64_t cap_heavy) {
    XM_SCOPE(stream);
    XM_ARG(R && Wp && pre && hid && ctl && Q && C && small && Qcat && uq_ptr && uc_ptr);
    XM_ARG(uq_item && uq_q && uc_item && uc_c && cap_light >= 0 && cap_heavy >= 0);
    hipStream_t st = (hipStream_t)stream;
    const int I = R->n_items;
    int rcode = plan_rows(stream, R, slot_target, nullptr, pre, hid, ctl, Q, C, small, Wp, Qcat, uq_ptr, uc_ptr, dups, nullptr, nullptr);
    if (rcode) return rcode;
    long long *counts = nullptr;
    XM_HIP(xm_malloc_async((void **)&counts, sizeof(long long) * 10, st));
    // (no items: one block that only gathers the counts -- both scans have left their zero totals)
    const long long threads = (long long)N_CLASSES * I > 0 ? (long long)N_CLASSES * I : 1;
    k_fill_units2<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(
        I, (const long long *)R->item_ptr, Qcat, (const long long *)uq_ptr, uq_item, uq_q, C, (const long long *)uc_ptr, uc_item, uc_c,
        cap_light, cap_heavy, ctl, counts);
    XM_LAUNCH_CHECK();
    return host_wait_post(st, HW_PLAN, counts, 10);
}

int xmap_sim3_plan_wait(int64_t cap_light, int64_t cap_heavy, int64_t *h_out) {
    XM_ARG(h_out);
    const int64_t *h = nullptr;
    int rcode = host_wait_take(HW_PLAN, &h);
    if (rcode) return rcode;
    for (int c = 0; c < 10; c++) h_out[c] = h[c];
    if (h_out[9] > HMAX) {
        set_error("heavy set larger than %d", HMAX);
        return XMAP_ERR_OVERFLOW;
    }
    if (h_out[0] > cap_light || h_out[1] > cap_heavy) {
        set_error("unit arrays too small: %lld light / %lld heavy units, room for %lld / %lld", (long long)h_out[0], (long long)h_out[1],
                  (long long)cap_light, (long long)cap_heavy);
        return XMAP_ERR_CAPACITY;
    }
    return XMAP_OK;
}

int xmap_sim3_plan(void *stream, const xmap_ratings *R, int32_t slot_target, const int64_t *pre, const int32_t *hid,
                   const int32_t *ctl, int32_t *Q, int32_t *C, uint8_t *small, uint64_t *Wp, int32_t *Qcat, int64_t *uq_ptr,
                   int64_t *uc_ptr, int32_t dups, int32_t *uq_item, int32_t *uq_q, int32_t *uc_item, int32_t *uc_c,
                   int64_t cap_light, int64_t cap_heavy, int64_t *h_out) {
    XM_ARG(h_out);
    for (int c = 0; c < 10; c++) h_out[c] = 0;
    int rcode = xmap_sim3_plan_begin(stream, R, slot_target, pre, hid, ctl, Q, C, small, Wp, Qcat, uq_ptr, uc_ptr, dups, uq_item, uq_q, uc_item,
                                     uc_c, cap_light, cap_heavy);
    if (rcode) return rcode;
    return xmap_sim3_plan_wait(cap_light, cap_heavy, h_out);
}

/* Round-3 layout of stage A (one transposition per pass): see the declarations in include/xmap_hip.h. */
int xmap_sim3_layout(void *stream, const xmap_ratings *R, int64_t *item_ptr, const double *rating64, int32_t ch_min, int32_t phases,
                     int32_t stats_lo, int32_t stats_hi, int32_t *cnt, double *u_avg, double *u_norm, int32_t *hist, int64_t *pre, int32_t *ctl, int32_t *hid, int32_t *hlist,
                     uint64_t *ub_key, void *ub, void *srec, void *bufA, void *bufB, void *rc, uint64_t *Wp, double *info,
                     double *norms, int32_t *h_ctl) {
    XM_SCOPE(stream);
    XM_ARG(R && item_ptr && (const int64_t *)item_ptr == R->item_ptr && cnt && u_avg && hist && pre && ctl && hid && hlist);
    XM_ARG(ub_key && ub && srec && bufA && bufB && rc && Wp && info && norms && ch_min >= 64);
    XM_ARG(R->nnz < 0x7fffffffLL && R->n_users < 0x7ffffff0LL && R->n_items >= 0);
    XM_ARG(rating64 || u_norm);
    XM_ARG(stats_lo >= 0 && stats_lo <= stats_hi && stats_hi <= R->n_items && (phases & ~XMAP_LAYOUT_ALL) == 0);
    hipStream_t st = (hipStream_t)stream;
    const int I = R->n_items;
    const long long nnz = R->nnz;
    const bool wide = rating64 != nullptr;
    const size_t In = (size_t)(I > 0 ? I : 1);
    int rcode = XMAP_OK;
    // the big items' lists (STATS); taken here so that their counters are cleared with the other fills of the pass
    const bool stats = (phases & XMAP_LAYOUT_STATS) && stats_hi > stats_lo;
    BigList B;
    bool b_cleared = false;
    if (stats) {
        B.chunk_cap = nnz / STAT_CHK + nnz / STAT_BIG + 2;
        B.item_cap = nnz / STAT_BIG + 2;
        XM_HIP(xm_malloc_async((void **)&B.counters, 2 * sizeof(unsigned), st));
        XM_HIP(xm_malloc_async((void **)&B.chunks, sizeof(int2) * (size_t)B.chunk_cap, st));
        XM_HIP(xm_malloc_async((void **)&B.items, sizeof(int4) * (size_t)B.item_cap, st));
        XM_HIP(xm_malloc_async((void **)&B.part, sizeof(double) * ITEM_PART * (size_t)B.chunk_cap, st));
    }
    if (phases & XMAP_LAYOUT_RECORDS) {
        // every small fill of the pass in one launch: the rater counts, the histogram and ctl of the heavy set, W+ (summed by the
        // tile sort's last level), the big items' counters (+ the bucket counters of the partitioned count)
        FillList F;
        F.add(cnt, sizeof(int32_t) * In);
        heavy_set_fills(F, R->n_users, hist, ctl);
        F.add(Wp, sizeof(uint64_t) * In);
        if (stats) { F.add(B.counters, 2 * sizeof(unsigned)); b_cleared = true; }
        // raters per item -> item_ptr
        const char *cb_env = getenv("XMAP_COUNT_PART_MIN");          // (tests force the partitioned count on small inputs)
        const long long cb_min = cb_env ? atoll(cb_env) : 2000000ll;
        if (nnz >= cb_min && I > 0) {         // partitioned count (k_cbs_*, k_cb_count): the item column as one range, through bufA
            rcode = mirror_counts(st, I, nnz, 1, nullptr, nullptr, R->user_item, false, (int *)bufA, cnt, &F);        // (free until the tile sort)
            if (rcode) return rcode;
        } else {
            rcode = fill_multi(st, F);
            if (rcode) return rcode;
            if (nnz > 0) {
                k_count3<<<dim3((unsigned)((nnz + CNT_CHUNK - 1) / CNT_CHUNK)), dim3(256), 0, st>>>(nnz, R->user_item, cnt);
                XM_LAUNCH_CHECK();
            }
        }
        rcode = xmap_exclusive_scan_i32_to_i64(stream, cnt, item_ptr, I, nullptr);
        if (rcode) return rcode;
        if (!wide) {
            rcode = xmap_user_stats(stream, R, u_avg, u_norm);
            if (rcode) return rcode;
        }
        // rater-count histogram -> partner bounds, heavy set (as xmap_sim2_layout)
        rcode = heavy_set(stream, I, R->n_users, item_ptr, ch_min, hist, pre, ctl, hid, hlist, true);
        if (rcode) return rcode;
        // sorted profiles + sort records (no mutuality flags yet)
        if (R->n_users > 0 && nnz > 0) {
            const dim3 grid((unsigned)((R->n_users + 4 * SORT_NB - 1) / (4 * SORT_NB)));
            (wide ? k_sort_profiles3<true> : k_sort_profiles3<false>)<<<grid, dim3(256), 0, st>>>(
                R->n_users, (const long long *)R->user_ptr, R->user_item, wide ? nullptr : R->user_rating, rating64, cnt,
                (unsigned long long *)ub_key, ub, (unsigned long long *)srec);
            XM_LAUNCH_CHECK();
        }
        // sort records -> rater records in item order, W+ (cleared above)
        if (nnz > 0 && I > 0) {
            ts::Geo G;
            ts_geometry(I, nnz, wide ? ts::Chunk<3>::CH : ts::Chunk<2>::CH, G);
            rcode = ts_prepare(st, G, (const long long *)item_ptr);
            if (rcode) return rcode;
            rcode = wide ? sort_rater_records<3>(st, G, nnz, srec, bufA, bufB, R->user_ptr, rc, Wp)
                         : sort_rater_records<2>(st, G, nnz, srec, bufA, bufB, R->user_ptr, rc, Wp);
            if (rcode) return rcode;
        }
    }
    // item statistics of [stats_lo, stats_hi) from the rater records (+ those records' mutuality flags), big items in chunks
    if (stats) {
        if (!b_cleared) XM_HIP(hipMemsetAsync(B.counters, 0, 2 * sizeof(unsigned), st));
        rcode = wide ? item_stats3(st, I, stats_lo, stats_hi, item_ptr, RcWideSrc{(const RaterRecWide *)rc}, info, norms, B)
                     : item_stats3(st, I, stats_lo, stats_hi, item_ptr, RcSrc{(RaterRec *)rc, u_avg}, info, norms, B);
        if (rcode) return rcode;
    }
    // mutuality flags from the COMPLETE item info: the profile copy's, the rater records' of the items another rank's
    // statistics covered
    if (!wide && nnz > 0 && I > 0) {
        if (phases & XMAP_LAYOUT_RC_FLAGS) {
            k_rc_flags<<<dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st>>>(nnz, (RaterRec *)rc, (const int2 *)ub, info);
            XM_LAUNCH_CHECK();
        }
        if (phases & XMAP_LAYOUT_UB_FLAGS) {
            k_ub_flags<<<dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st>>>(nnz, (int2 *)ub, info);
            XM_LAUNCH_CHECK();
        }
    }
    return h_ctl ? read_heavy_ctl(st, ctl, h_ctl) : XMAP_OK;
}
}
