// stage_c_union.hip -- the union of the AlterEgo rows of D independent two-domain problems (the reference's multi-domain
// driver: alterEgo_profile1.union(alterEgo_profile2) ... .distinct(), code/multidomain_demo.py:128) as ONE set of user-major
// profiles in the layout xmap_rec_profiles writes, so that the whole recommender tail (RecommenderSim, selection, prediction,
// top-N, evaluation, MAE) runs over D domains as it does over one.
//
// A part is one domain's stage-C output as xmap_alterego_fill leaves it, plus two maps into the union's index spaces
// (xmap_union_part).  The rows of union user g, in the order of the contract: parts in the order given; within a part the rows
// of the local user u with user_map[u] = g, pass-through rows first, then mapped rows, each in stage-C order -- 2 D segments,
// found through the inverse user maps inv[d][g] the first pass builds.  Rows whose item maps to -1 are dropped; with
// XMAP_UNION_DISTINCT a row equal to an earlier remaining row of the same user (item, time, rating as a number) is removed.
// Equality is transitive (ratings are finite), so "equal to an earlier kept row" is "not the first row of its class".
//
// Passes (count -> scan -> fill; both passes decide a user's class from its row count L, neither carries state to the other):
//   k_union_check  (count only) every map entry, offset and item index against its bounds; inv by compare-and-swap, which
//                  also finds a user_map that is not injective.  The kernels behind it return at once when it found anything.
//   k_union_short  L <= 32 (UN_SHORT): a 32-lane group per user, two users per wave.  Lane s < 2 D owns segment s, lane r row r;
//                  duplicates by broadcasting a 32-bit hash of each row and comparing the fields only where hashes meet.
//                  Users with more rows are appended to the lists of the two classes below (the order of a list decides
//                  nothing but scheduling: positions come from prof_ptr).
//   k_union_block<medium>  32 < L <= 2048 (UN_MED): a block per user; rows staged in LDS (20 B each) with a 4096-slot hash set of
//                  row indices, 56 KB in all, two blocks per CU.  A slot belongs to the class that claimed it and keeps the
//                  least row index of the class (atomicMin): the first occurrence, whatever order the lanes arrive in.
//   k_union_block<large>   L > 2048: the same set in global memory (2 slots per row, from the stream's arena), rows re-read in place.
//   k_union_tally + exclusive scan -> prof_ptr and the four counters.
// One pass over the rows in count and one in fill for short users; medium and large users read their rows twice per pass
// (insert, then select in order).  Two synchronisations in count (the verdict of the check with the list sizes; the totals),
// none in fill.
#include "common.h"

namespace xmap {

constexpr int UN_MAX_PARTS = 16;
constexpr int UN_SHORT = 32;            // rows of a short user (one 32-lane group)
constexpr int UN_MED = 2048;            // rows of a medium user (LDS)
constexpr int UN_SLOTS = 4096;          // hash slots of a medium user
constexpr int UN_EMPTY = 0x7fffffff;

struct UParts { xmap_union_part p[UN_MAX_PARTS]; };
struct URow { int item; double rating; long long time; };      // item: the union item, -1 = dropped

// lists of the users beyond UN_SHORT, built by k_union_short: meta[0] / [1] = medium / large users, [2] = slot cursor of the
// large users' hash sets, [3] = rows of the large users
struct ULists { unsigned long long *meta; int *med; int *big; unsigned long long *big_off; };

// the descriptors to device memory: kernels index them by a part number that differs per lane
__global__ void k_union_parts(UParts H, int D, xmap_union_part *out) {
#pragma unroll
    for (int d = 0; d < UN_MAX_PARTS; d++)
        if ((int)threadIdx.x == d && d < D) out[d] = H.p[d];
}

// Position k of part d: [0, U) user_map, [U, U + I) item_map, then off_t [U + 1], off_m [U + 1], item [n_rows].  bad[0] += bad
// positions, bad[1] = min((d * 8 + kind) << 48 | position).  Bounded by the sizes alone; inv is indexed by checked values only.
__global__ __launch_bounds__(256) void k_union_check(const xmap_union_part *P, long long n_users, int n_items, int *inv,
                                                     unsigned long long *bad) {
    const int d = blockIdx.y;
    const xmap_union_part p = P[d];
    const long long U = p.n_users, I = p.n_items, total = U + I + 2 * (U + 1) + p.n_rows;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += step) {
        long long q = k;
        int kind;
        bool b;
        if (q < U) {
            kind = 0;
            const int g = p.user_map[q];
            b = g < 0 || g >= n_users;
            if (!b && atomicCAS(&inv[(long long)d * n_users + g], -1, (int)q) != -1) { b = true; kind = 5; }
        } else if ((q -= U) < I) {
            kind = 1;
            const int m = p.item_map[q];
            b = m < -1 || m >= n_items;
        } else if ((q -= I) <= U) {
            kind = 2;
            const long long v = p.off_t[q];
            b = q == 0 ? v != 0 : v < p.off_t[q - 1];
            if (q == U) b = b || v != p.n_target_rows;
        } else if ((q -= U + 1) <= U) {
            kind = 3;
            const long long v = p.off_m[q];
            b = q == 0 ? v != 0 : v < p.off_m[q - 1];
            if (q == U) b = b || v != p.n_rows - p.n_target_rows;
        } else {
            q -= U + 1;
            kind = 4;
            const int it = p.item[q];
            b = it < 0 || it >= I;
        }
        if (b) {                        // (bad input only: no need to spare the atomics)
            atomicAdd(&bad[0], 1ull);
            atomicMin(&bad[1], ((unsigned long long)(d * 8 + kind) << 48) | (unsigned long long)q);
        }
    }
}

// the inverse user maps of parts the count pass accepted (fill)
__global__ __launch_bounds__(256) void k_union_inv(const xmap_union_part *P, long long n_users, int *inv) {
    const int d = blockIdx.y;
    const long long U = P[d].n_users;
    const int *user_map = P[d].user_map;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < U; u += step)
        inv[(long long)d * n_users + user_map[u]] = (int)u;
}

// segment s of union user g: part s >> 1; s & 1 = 0: the local user's pass-through rows, 1: its mapped rows
__device__ __forceinline__ void union_seg(const xmap_union_part *P, int D, long long n_users, const int *inv, long long g, int s,
                                          int &beg, int &len) {
    beg = 0; len = 0;
    const int d = s >> 1;
    if (d >= D) return;
    const int lu = inv[(long long)d * n_users + g];
    if (lu < 0) return;
    if (s & 1) {
        const long long b = P[d].off_m[lu];
        beg = (int)(P[d].n_target_rows + b); len = (int)(P[d].off_m[lu + 1] - b);
    } else {
        const long long b = P[d].off_t[lu];
        beg = (int)b; len = (int)(P[d].off_t[lu + 1] - b);
    }
}

__device__ __forceinline__ URow union_row(const xmap_union_part *P, int d, int src) {
    URow r;
    r.item = P[d].item_map[P[d].item[src]];
    r.rating = P[d].rating[src];
    r.time = P[d].time[src];
    return r;
}

__device__ __forceinline__ bool same_row(const URow &a, const URow &b) {
    return a.item == b.item && a.time == b.time && a.rating == b.rating;        // -0.0 == 0.0: equal as numbers
}

__device__ __forceinline__ uint32_t row_hash(const URow &r) {
    const unsigned long long rb = r.rating == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(r.rating);
    uint32_t h = mix32((uint32_t)r.item * 0x9E3779B1u + 0x7F4A7C15u);
    h = mix32(h ^ (uint32_t)r.time);
    h = mix32(h + (uint32_t)((unsigned long long)r.time >> 32));
    h = mix32(h ^ (uint32_t)rb);
    return mix32(h + (uint32_t)(rb >> 32));
}

// ---- short users: a 32-lane group each.  Writes cnt / drp (count) or the rows (fill) of the users with L <= UN_SHORT and
// lists the others.
template <bool FILL>
__global__ __launch_bounds__(256) void k_union_short(const xmap_union_part *P, int D, long long n_users, int distinct, const int *inv,
                                                     const unsigned long long *bad, ULists Ls, int *cnt, int *drp,
                                                     const long long *prof_ptr, int *o_item, double *o_rating, long long *o_time) {
    if (bad && bad[0]) return;
    const int r = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    const long long g = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool user = g < n_users;
    int beg = 0, len = 0;
    if (user) union_seg(P, D, n_users, inv, g, r, beg, len);
    long long inc = len;                        // inclusive scan of the segment lengths over the group
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) {
        const long long o = __shfl_up(inc, m, 32);
        if (r >= m) inc += o;
    }
    const long long L = __shfl(inc, 31, 32);
    const int start = (int)(inc - len);
    if (user && L > UN_SHORT && r == 0) {
        if (L > UN_MED) {
            const unsigned long long k = atomicAdd(&Ls.meta[1], 1ull);
            const unsigned long long slots = 2ull * (unsigned long long)(FILL ? prof_ptr[g + 1] - prof_ptr[g] : L) + 2ull;
            Ls.big[k] = (int)g;
            Ls.big_off[k] = atomicAdd(&Ls.meta[2], slots);
            atomicAdd(&Ls.meta[3], (unsigned long long)L);
        } else {
            Ls.med[atomicAdd(&Ls.meta[0], 1ull)] = (int)g;
        }
    }
    const int n = (user && L <= UN_SHORT) ? (int)L : 0;
    // row r of the user: the segment that holds it
    int part = 0, src = 0;
    for (int s = 0; s < 2 * D; s++) {
        const int st = __shfl(start, s, 32), ln = __shfl(len, s, 32), bg = __shfl(beg, s, 32);
        if (r >= st && r < st + ln) { part = s >> 1; src = bg + (r - st); }
    }
    URow row;
    row.item = -1; row.rating = 0.0; row.time = 0;
    if (r < n) row = union_row(P, part, src);
    const bool valid = r < n && row.item >= 0;
    bool dup = false;
    if (distinct) {
        const int n_other = __shfl_xor(n, 32, 64);
        const int n_max = n > n_other ? n : n_other;
        const uint32_t h = row_hash(row);
        for (int j = 0; j + 1 < n_max; j++) {
            const uint32_t hj = (uint32_t)__shfl((int)h, j, 32);
            if (__any(j < r && valid && hj == h)) {
                URow o;
                o.item = __shfl(row.item, j, 32);
                o.time = __shfl(row.time, j, 32);
                o.rating = __shfl(row.rating, j, 32);
                if (j < r && valid && o.item >= 0 && same_row(o, row)) dup = true;
            }
        }
    }
    const bool keep = valid && !dup;
    const uint32_t mk = (uint32_t)(__ballot(keep) >> (32 * half)), md = (uint32_t)(__ballot(r < n && row.item < 0) >> (32 * half));
    if (!FILL) {
        if (user && L <= UN_SHORT && r == 0) { cnt[g] = __popc(mk); drp[g] = __popc(md); }
    } else if (keep) {
        const long long o = prof_ptr[g] + __popc(mk & ((1u << r) - 1u));
        o_item[o] = row.item; o_rating[o] = row.rating; o_time[o] = row.time;
    }
}

// ---- medium and large users: a block each, over a list
template <bool BIG>
struct URows {                                  // the rows of the block's user by position
    const xmap_union_part *P;
    const int *s_beg, *s_start;                 // segment s: first source row, first position (s_start[32] = L)
    const int *s_item; const long long *s_time; const double *s_rating;
    __device__ __forceinline__ URow global_at(int r) const {
        int s = 0;
        while (r >= s_start[s + 1]) s++;
        return union_row(P, s >> 1, s_beg[s] + (r - s_start[s]));
    }
    __device__ __forceinline__ URow at(int r) const {
        if (BIG) return global_at(r);
        URow o;
        o.item = s_item[r]; o.time = s_time[r]; o.rating = s_rating[r];
        return o;
    }
};

template <bool FILL, bool BIG>
__global__ __launch_bounds__(256) void k_union_block(const xmap_union_part *P, int D, long long n_users, int distinct, const int *inv,
                                                     const int *list, const unsigned long long *n_list,
                                                     const unsigned long long *big_off, int *gtab, int *cnt, int *drp,
                                                     const long long *prof_ptr, int *o_item, double *o_rating, long long *o_time) {
    __shared__ int s_beg[32], s_len[32], s_start[33], s_w[4], s_drop;
    __shared__ int s_item[BIG ? 1 : UN_MED];
    __shared__ long long s_time[BIG ? 1 : UN_MED];
    __shared__ double s_rating[BIG ? 1 : UN_MED];
    __shared__ int s_tab[BIG ? 1 : UN_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long n = *n_list;
    URows<BIG> rows{P, s_beg, s_start, s_item, s_time, s_rating};
    for (unsigned long long k = blockIdx.x; k < n; k += gridDim.x) {
        const long long g = list[k];
        __syncthreads();
        if (tid < 32) union_seg(P, D, n_users, inv, g, tid, s_beg[tid], s_len[tid]);
        if (tid == 0) s_drop = 0;
        __syncthreads();
        if (tid == 0) {
            int a = 0;
            for (int s = 0; s < 32; s++) { s_start[s] = a; a += s_len[s]; }
            s_start[32] = a;
        }
        __syncthreads();
        const int L = s_start[32];
        int *tab = s_tab;
        unsigned long long size = UN_SLOTS;
        if (BIG) {
            tab = gtab + big_off[k];
            size = 2ull * (unsigned long long)(FILL ? prof_ptr[g + 1] - prof_ptr[g] : (long long)L) + 2ull;
        }
        if (distinct)
            for (unsigned long long i = tid; i < size; i += 256) __atomic_store_n(&tab[i], UN_EMPTY, __ATOMIC_RELAXED);
        if (!BIG)
            for (int r = tid; r < L; r += 256) {
                const URow o = rows.global_at(r);
                s_item[r] = o.item; s_time[r] = o.time; s_rating[r] = o.rating;
            }
        __threadfence();
        __syncthreads();
        // the set: a slot belongs to the class that claimed it and ends with the least row index of the class
        if (distinct)
            for (long long r0 = tid; r0 < L; r0 += 256) {
                const int r = (int)r0;
                const URow row = rows.at(r);
                if (row.item < 0) continue;
                unsigned long long slot = row_hash(row) % size;
                for (;;) {
                    int cur = __atomic_load_n(&tab[slot], __ATOMIC_RELAXED);
                    if (cur == UN_EMPTY) {
                        cur = atomicCAS(&tab[slot], UN_EMPTY, r);
                        if (cur == UN_EMPTY) break;
                    }
                    if (same_row(rows.at(cur), row)) { atomicMin(&tab[slot], r); break; }
                    if (++slot == size) slot = 0;
                }
            }
        __threadfence();
        __syncthreads();
        // the kept rows in order
        long long running = 0;
        for (long long base = 0; base < L; base += 256) {
            const long long r0 = base + tid;
            const int r = (int)r0;
            bool keep = false, drop = false;
            URow row;
            row.item = -1; row.rating = 0.0; row.time = 0;
            if (r0 < L) {
                row = rows.at(r);
                if (row.item < 0) drop = true;
                else if (!distinct) keep = true;
                else {
                    unsigned long long slot = row_hash(row) % size;
                    for (;;) {              // (its class was inserted: the walk ends before an empty slot)
                        const int cur = __atomic_load_n(&tab[slot], __ATOMIC_RELAXED);
                        if (cur == r) { keep = true; break; }
                        if (cur == UN_EMPTY || same_row(rows.at(cur), row)) break;
                        if (++slot == size) slot = 0;
                    }
                }
            }
            const unsigned long long bk = __ballot(keep), bd = __ballot(drop);
            if (lane == 0) {
                s_w[w] = __popcll(bk);
                if (bd) atomicAdd(&s_drop, __popcll(bd));
            }
            __syncthreads();
            int pre = 0, tot = 0;
            for (int i = 0; i < 4; i++) { if (i < w) pre += s_w[i]; tot += s_w[i]; }
            if (FILL && keep) {
                const long long o = prof_ptr[g] + running + pre + __popcll(bk & lanemask_lt());
                o_item[o] = row.item; o_rating[o] = row.rating; o_time[o] = row.time;
            }
            running += tot;
            __syncthreads();
        }
        if (!FILL && tid == 0) { cnt[g] = (int)running; drp[g] = s_drop; }
    }
}

// tot[0] += dropped rows, tot[1] += users with a row (integer sums: any order gives the same)
__global__ __launch_bounds__(256) void k_union_tally(long long n_users, const int *cnt, const int *drp, unsigned long long *tot) {
    long long a = 0, b = 0;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_users; g += step) { a += drp[g]; b += cnt[g] > 0; }
    a = wave_sum_ll(a); b = wave_sum_ll(b);
    if (lane_id() == 0) {
        if (a) atomicAdd(&tot[0], (unsigned long long)a);
        if (b) atomicAdd(&tot[1], (unsigned long long)b);
    }
}

static const char *const UN_KIND[6] = {"user_map entry outside [0, n_users)", "item_map entry outside [-1, n_items)",
                                       "off_t (off_t[0] = 0, non-decreasing, off_t[U] = n_target_rows)",
                                       "off_m (off_m[0] = 0, non-decreasing, off_m[U] = n_rows - n_target_rows)",
                                       "row item outside [0, n_items of the part)", "user_map names a union user twice"};

// what both entry points ask of the host-side arguments; *n_total = rows of all parts
static int union_args(int32_t n_parts, const xmap_union_part *parts, int64_t n_users, int32_t n_items, int32_t flags, int64_t *n_total) {
    XM_ARG(parts && n_parts >= 1 && n_parts <= UN_MAX_PARTS);
    XM_ARG(n_users >= 0 && n_users < 2147483647ll && n_items >= 0 && (flags & ~XMAP_UNION_DISTINCT) == 0);
    int64_t total = 0;
    for (int d = 0; d < n_parts; d++) {
        const xmap_union_part &p = parts[d];
        XM_ARG(p.n_users >= 0 && p.n_users < 2147483647ll && p.n_items >= 0);
        XM_ARG(p.n_target_rows >= 0 && p.n_rows >= p.n_target_rows && p.n_rows < 2147483647ll);
        XM_ARG(p.off_t && p.off_m && (p.n_users == 0 || p.user_map) && (p.n_items == 0 || p.item_map));
        XM_ARG(p.n_rows == 0 || (p.item && p.rating && p.time));
        total += p.n_rows;
    }
    XM_ARG(total < 2147483647ll);
    *n_total = total;
    return XMAP_OK;
}

struct UWork {                  // temporaries both passes take
    xmap_union_part *parts; int *inv; ULists Ls; int64_t cap_med, cap_big;
};

static int union_work(hipStream_t st, int32_t n_parts, const xmap_union_part *parts, int64_t n_users, int64_t n_total, UWork &W) {
    W.cap_med = n_total / (UN_SHORT + 1) + 1;
    W.cap_big = n_total / (UN_MED + 1) + 1;
    XM_HIP(xm_malloc_async((void **)&W.parts, sizeof(xmap_union_part) * UN_MAX_PARTS, st));
    XM_HIP(xm_malloc_async((void **)&W.inv, sizeof(int) * (size_t)n_parts * (size_t)(n_users ? n_users : 1), st));
    XM_HIP(xm_malloc_async((void **)&W.Ls.meta, sizeof(unsigned long long) * 8, st));
    XM_HIP(xm_malloc_async((void **)&W.Ls.med, sizeof(int) * (size_t)W.cap_med, st));
    XM_HIP(xm_malloc_async((void **)&W.Ls.big, sizeof(int) * (size_t)W.cap_big, st));
    XM_HIP(xm_malloc_async((void **)&W.Ls.big_off, sizeof(unsigned long long) * (size_t)W.cap_big, st));
    XM_HIP(hipMemsetAsync(W.inv, 0xff, sizeof(int) * (size_t)n_parts * (size_t)(n_users ? n_users : 1), st));
    XM_HIP(hipMemsetAsync(W.Ls.meta, 0, sizeof(unsigned long long) * 8, st));
    UParts H;
    memset(&H, 0, sizeof(H));
    for (int d = 0; d < n_parts; d++) H.p[d] = parts[d];
    k_union_parts<<<dim3(1), dim3(64), 0, st>>>(H, n_parts, W.parts);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

static unsigned grid_for(long long n, unsigned cap) {
    const long long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b < (long long)cap ? b : (long long)cap));
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_union_count(void *stream, int32_t n_parts, const xmap_union_part *parts, int64_t n_users, int32_t n_items, int32_t flags,
                     int64_t *prof_ptr, int64_t *h_counts) {
    int64_t n_total = 0;
    int rc = union_args(n_parts, parts, n_users, n_items, flags, &n_total);
    if (rc) return rc;
    XM_ARG(prof_ptr && h_counts);
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    const int distinct = (flags & XMAP_UNION_DISTINCT) ? 1 : 0;
    UWork W;
    rc = union_work(st, n_parts, parts, n_users, n_total, W);
    if (rc) return rc;
    unsigned long long *bad = nullptr, *tot = nullptr, h_bad[2] = {0, 0}, h_meta[4] = {0, 0, 0, 0}, h_tot[2] = {0, 0};
    int *cnt = nullptr, *drp = nullptr;
    XM_HIP(xm_malloc_async((void **)&bad, sizeof(h_bad), st));
    XM_HIP(xm_malloc_async((void **)&tot, sizeof(h_tot), st));
    XM_HIP(xm_malloc_async((void **)&cnt, sizeof(int) * (size_t)(n_users ? n_users : 1), st));
    XM_HIP(xm_malloc_async((void **)&drp, sizeof(int) * (size_t)(n_users ? n_users : 1), st));
    XM_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned long long), st));
    XM_HIP(hipMemsetAsync(bad + 1, 0xff, sizeof(unsigned long long), st));
    XM_HIP(hipMemsetAsync(tot, 0, sizeof(h_tot), st));
    // ---- the check: nothing behind it indexes anything when it fails, and no output is written
    long long most = 0;
    for (int d = 0; d < n_parts; d++) {
        const long long t = 3 * parts[d].n_users + 2 + parts[d].n_items + parts[d].n_rows;
        if (t > most) most = t;
    }
    k_union_check<<<dim3(grid_for(most, 4096), (unsigned)n_parts), dim3(256), 0, st>>>(W.parts, n_users, n_items, W.inv, bad);
    XM_LAUNCH_CHECK();
    if (n_users > 0) {
        k_union_short<false><<<dim3((unsigned)((n_users + 7) / 8)), dim3(256), 0, st>>>(W.parts, n_parts, n_users, distinct, W.inv, bad, W.Ls,
                                                                                        cnt, drp, nullptr, nullptr, nullptr, nullptr);
        XM_LAUNCH_CHECK();
    }
    XM_HIP(hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(h_meta, W.Ls.meta, sizeof(h_meta), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_bad[0]) {
        const int code = (int)(h_bad[1] >> 48);
        set_error("union: %llu bad entries, the first in part %d at position %llu: %s", h_bad[0], code / 8,
                  h_bad[1] & 0xffffffffffffull, UN_KIND[(code % 8) < 6 ? code % 8 : 0]);
        return XMAP_ERR_ARG;
    }
    // ---- the users beyond a lane group
    if (h_meta[0]) {
        k_union_block<false, false><<<dim3((unsigned)h_meta[0]), dim3(256), 0, st>>>(W.parts, n_parts, n_users, distinct, W.inv, W.Ls.med,
                                                                                    W.Ls.meta + 0, nullptr, nullptr, cnt, drp, nullptr,
                                                                                    nullptr, nullptr, nullptr);
        XM_LAUNCH_CHECK();
    }
    int *gtab = nullptr;
    if (h_meta[1]) {
        XM_HIP(xm_malloc_async((void **)&gtab, sizeof(int) * (size_t)(distinct ? h_meta[2] : 1), st));
        k_union_block<false, true><<<dim3((unsigned)h_meta[1]), dim3(256), 0, st>>>(W.parts, n_parts, n_users, distinct, W.inv, W.Ls.big,
                                                                                   W.Ls.meta + 1, W.Ls.big_off, gtab, cnt, drp, nullptr,
                                                                                   nullptr, nullptr, nullptr);
        XM_LAUNCH_CHECK();
    }
    if (n_users > 0) {
        k_union_tally<<<dim3(grid_for(n_users, 1024)), dim3(256), 0, st>>>(n_users, cnt, drp, tot);
        XM_LAUNCH_CHECK();
    }
    rc = xmap_exclusive_scan_i32_to_i64(st, cnt, prof_ptr, n_users, nullptr);
    if (rc) return rc;
    long long h_rows = 0;
    XM_HIP(hipMemcpyAsync(&h_rows, prof_ptr + n_users, sizeof(long long), hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(h_tot, tot, sizeof(h_tot), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    h_counts[0] = h_rows;
    h_counts[1] = n_total - (int64_t)h_tot[0] - h_rows;         // what is neither kept nor dropped was a duplicate
    h_counts[2] = (int64_t)h_tot[0];
    h_counts[3] = (int64_t)h_tot[1];
    if (gtab) XM_HIP(xm_free_async(gtab, st));
    XM_HIP(xm_free_async(drp, st)); XM_HIP(xm_free_async(cnt, st)); XM_HIP(xm_free_async(tot, st)); XM_HIP(xm_free_async(bad, st));
    XM_HIP(xm_free_async(W.Ls.big_off, st)); XM_HIP(xm_free_async(W.Ls.big, st)); XM_HIP(xm_free_async(W.Ls.med, st));
    XM_HIP(xm_free_async(W.Ls.meta, st)); XM_HIP(xm_free_async(W.inv, st)); XM_HIP(xm_free_async(W.parts, st));
    return XMAP_OK;
}

int xmap_union_fill(void *stream, int32_t n_parts, const xmap_union_part *parts, int64_t n_users, int32_t n_items, int32_t flags,
                    const int64_t *prof_ptr, int64_t n_out, int32_t *prof_item, double *prof_rating, int64_t *prof_time) {
    int64_t n_total = 0;
    int rc = union_args(n_parts, parts, n_users, n_items, flags, &n_total);
    if (rc) return rc;
    XM_ARG(prof_ptr && n_out >= 0 && n_out <= n_total);
    if (n_out == 0 || n_users == 0) return XMAP_OK;             // no row to write
    XM_ARG(prof_item && prof_rating && prof_time);
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    const int distinct = (flags & XMAP_UNION_DISTINCT) ? 1 : 0;
    UWork W;
    rc = union_work(st, n_parts, parts, n_users, n_total, W);
    if (rc) return rc;
    long long most = 0;
    for (int d = 0; d < n_parts; d++) if (parts[d].n_users > most) most = parts[d].n_users;
    k_union_inv<<<dim3(grid_for(most, 4096), (unsigned)n_parts), dim3(256), 0, st>>>(W.parts, n_users, W.inv);
    XM_LAUNCH_CHECK();
    k_union_short<true><<<dim3((unsigned)((n_users + 7) / 8)), dim3(256), 0, st>>>(W.parts, n_parts, n_users, distinct, W.inv, nullptr, W.Ls,
                                                                                   nullptr, nullptr, (const long long *)prof_ptr, prof_item,
                                                                                   prof_rating, (long long *)prof_time);
    XM_LAUNCH_CHECK();
    // the lists' lengths stay on the device: the blocks stride over them.  A user beyond UN_SHORT needs n_total > UN_SHORT.
    if (n_total > UN_SHORT) {
        const unsigned blocks = (unsigned)(W.cap_med < 2048 ? W.cap_med : 2048);
        k_union_block<true, false><<<dim3(blocks), dim3(256), 0, st>>>(W.parts, n_parts, n_users, distinct, W.inv, W.Ls.med, W.Ls.meta + 0,
                                                                      nullptr, nullptr, nullptr, nullptr, (const long long *)prof_ptr,
                                                                      prof_item, prof_rating, (long long *)prof_time);
        XM_LAUNCH_CHECK();
    }
    int *gtab = nullptr;
    if (n_total > UN_MED) {
        // a large user's set has two slots per kept row (+ 2): the kept rows are its classes
        XM_HIP(xm_malloc_async((void **)&gtab, sizeof(int) * (distinct ? 2 * (size_t)n_out + 2 * (size_t)W.cap_big : 1), st));
        const unsigned blocks = (unsigned)(W.cap_big < 256 ? W.cap_big : 256);
        k_union_block<true, true><<<dim3(blocks), dim3(256), 0, st>>>(W.parts, n_parts, n_users, distinct, W.inv, W.Ls.big, W.Ls.meta + 1,
                                                                     W.Ls.big_off, gtab, nullptr, nullptr, (const long long *)prof_ptr,
                                                                     prof_item, prof_rating, (long long *)prof_time);
        XM_LAUNCH_CHECK();
        XM_HIP(xm_free_async(gtab, st));
    }
    XM_HIP(xm_free_async(W.Ls.big_off, st)); XM_HIP(xm_free_async(W.Ls.big, st)); XM_HIP(xm_free_async(W.Ls.med, st));
    XM_HIP(xm_free_async(W.Ls.meta, st)); XM_HIP(xm_free_async(W.inv, st)); XM_HIP(xm_free_async(W.parts, st));
    return XMAP_OK;
}
}
