// stage_e_quota.hip -- label quotas and calibrated lists on the device (DESIGN.md 4 "Quotas and calibrated lists"): ONE list with a
// guaranteed mix of labels, cut from a pool of up to 1 024 ranked positions.  CAP: at most cap(l) entries of label l, greedy in
// pool order.  SHARE: the seats of the list go to the labels by Sainte-Lague quotients of their weights (an editorial mix, or the
// query user's own history), each seat taken by the label's best position still free.  Integers only; the scores are copied.
//   k_qt_capcheck : lab_cap: the first label with a negative entry (before any other work)
//   k_rf_check    : (rec_filter.h) / k_sh_check (stage_e_shelf.hip, through shelf_check_labels): the label table, as the shelves
//   k_qt_maxrow   : the longest label row of the whole table, one integer max-reduction: n_pool x it bounds the records of ANY pool
//   k_qt<PC, ROWS, FLOOR> : one block of 256 threads per query, everything of the query in LDS:
//       pool      : ROWS: au_select_segment (au_select.h) over the query's scored segment, the n_pool best straight into LDS (PC =
//                   its CAP: 256 or 1 024), never written to memory; else the caller's pool, position j = rank j
//       records   : one record per (position, governed label), in position order (poff: a block scan of the row lengths)
//       local ids : the records' labels sorted by a bitonic network and made unique in place: the distinct labels of the pool in
//                   ascending order; a record's local id = its label's index there (bisection).  Caps / weights, counters / seats and
//                   the cursors are arrays over the local ids
//       weights   : lab_weight, or the history: the block walks the user's profile rows, bisects each governed label of a row's
//                   item in the distinct labels and adds with integer LDS atomics (labels outside the pool cannot claim a seat)
//       CAP       : the greedy loop position by position: the block tests the position's labels, a block-wide OR decides
//       SHARE     : the records as (local id, position) keys sorted again: per label its positions ascending, a cursor per label
//                   that skips the positions already taken; per slot a block-wide arg-max of the quotients (64-bit products, the
//                   smaller local id = the smaller label on equality)
//       outputs   : the chosen positions' items and score bits, copied; counts and padding
// LDS: 8 PC + PC / 8 + 136 B, and the larger of the selection's 24 PC B and 18 B per record slot (a power of two >= n_pool x the
// longest label row): 8 KB for a pool of 256 single-label items, 150 KB at the limit of 8 192 records.
#include "au_select.h"
#include "common.h"
#include "rec_filter.h"
#include "rec_model.h"
#include "topn_pass.h"
#include "two_pass.h"

namespace xmap {

constexpr int QT_THREADS = AU_SEL_THREADS;
constexpr unsigned QT_PAD = 0xffffffffu;        // behind every label and every (local id, position) key
constexpr int QT_POS_BITS = 10;
static_assert(XMAP_QUOTA_MAX_POOL == 1 << QT_POS_BITS && XMAP_QUOTA_MAX_POOL <= AU_MAX_TOP, "a position takes 10 bits of a key");
static_assert(XMAP_QUOTA_MAX_RECORDS <= 1 << 13 && XMAP_QUOTA_MAX_RECORDS < 65536, "local ids and record offsets are 16-bit");

// the fixed part of a block's LDS: src [PC] u32, poff [PC + 4] u16, opos [PC] u16, taken [PC / 32] u32, scratch [32] i32
__host__ __device__ constexpr size_t qt_fixed_bytes(int PC) { return (size_t)4 * PC + 2 * (PC + 4) + 2 * PC + PC / 8 + 128; }
__host__ __device__ constexpr size_t qt_back_bytes(int rcap) { return (size_t)18 * rcap + 8; }
static_assert(qt_fixed_bytes(256) % 8 == 0 && qt_fixed_bytes(1024) % 8 == 0, "the union region starts at an 8-byte boundary");

struct QtArgs {
    int n_pool, n_top, rcap, mode, cap, rank_by;
    // the caller's pool (ROWS = false)
    const int *in_cnt, *in_item;
    const double *in_plain, *in_decay;
    // the scored segments (ROWS = true)
    const long long *cand_ptr;
    const int *cand_item;
    const double *plain, *decay;
    const int *status;
    double min_score;
    // the rule
    const int *lab_cap;
    const unsigned *lab_weight;
    const int *query_user;
    long long n_users;
    const long long *prof_ptr;
    const int *prof_item;
    // the labels
    int n_items;
    const long long *lab_ptr;
    const int *lab_id;
    const unsigned *lab_allow;
    // outputs; st: [0..3] the quota counters, [4] dropped candidates, [5] the largest segment, [6] candidates below the floor
    int *out_cnt, *out_item;
    double *out_plain, *out_decay;
    int *out_pos, *out_label;
    unsigned long long *st;
};

// lab_cap: bad[0] = the first label with a negative cap
__global__ __launch_bounds__(256) void k_qt_capcheck(int n_labels, const int *lab_cap, unsigned long long *bad) {
    const int step = gridDim.x * blockDim.x;
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < n_labels; l += step)
        if (lab_cap[l] < 0) atomicMin(&bad[0], (unsigned long long)l);          // (a minimum does not depend on the order)
}

// mx[0] = the longest label row; lab_ptr has passed its check
__global__ __launch_bounds__(256) void k_qt_maxrow(int I, const long long *lab_ptr, unsigned long long *mx) {
    const long long step = (long long)gridDim.x * blockDim.x;
    unsigned long long m = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < I; i += step) {
        const unsigned long long c = (unsigned long long)(lab_ptr[i + 1] - lab_ptr[i]);
        m = c > m ? c : m;
    }
    if (m) atomicMax(&mx[0], m);
}

// block-wide exclusive scan of one int per thread (s4: 4 ints of LDS); two barriers
__device__ __forceinline__ void qt_scan(int v, int *s4, int &excl, int &total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s4[wave] = inc;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < QT_THREADS / 64; w++) {
        const int x = s4[w];
        pre += w < wave ? x : 0;
        tot += x;
    }
    excl = pre + inc - v;
    total = tot;
    __syncthreads();
}

// ascending bitonic sort of X[0 .. N), N a power of two, all threads of the block
__device__ __forceinline__ void qt_sort(unsigned *X, int N) {
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int t = threadIdx.x; t < N / 2; t += QT_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned a = X[i], b = X[l];
                if ((a > b) == ((i & k) == 0)) { X[i] = b; X[l] = a; }
            }
            __syncthreads();
        }
    }
}

// the index of v in the ascending distinct X[0 .. n), -1 if it is not there
__device__ __forceinline__ int qt_find(const unsigned *X, int n, unsigned v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (X[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && X[lo] == v ? lo : -1;
}

// The ONE statement of "the governed labels of item it", in ascending label: the count and the fill both call it.  Returns the count.
template <class Emit>
__device__ __forceinline__ int qt_labels(int it, const QtArgs &A, Emit emit) {
    if (it < 0 || it >= A.n_items) return 0;
    int c = 0;
    const long long b = A.lab_ptr[it + 1];
    for (long long k = A.lab_ptr[it]; k < b; k++) {
        const int l = A.lab_id[k];
        if (A.lab_allow && !bit_allowed(A.lab_allow, l)) continue;
        emit(c, (unsigned)l);
        c++;
    }
    return c;
}

// a beats b in the order of the quotients w / (2 s + 1): exactly, in 64-bit products; the smaller id on equality
__device__ __forceinline__ bool qt_beats(unsigned wa, unsigned sa, int da, unsigned wb, unsigned sb, int db) {
    const unsigned long long x = (unsigned long long)wa * (2ull * sb + 1ull), y = (unsigned long long)wb * (2ull * sa + 1ull);
    return x > y || (x == y && da < db);
}

template <int PC, bool ROWS, bool FLOOR>
__global__ __launch_bounds__(QT_THREADS) void k_qt(const QtArgs A) {
    extern __shared__ unsigned long long qt_lds[];
    unsigned char *base = (unsigned char *)qt_lds;
    unsigned *src = (unsigned *)base;                                   // [PC] position -> candidate of the segment (ROWS)
    unsigned short *poff = (unsigned short *)(base + 4 * PC);          // [PC + 1] position -> its first record
    unsigned short *opos = poff + PC + 4;                              // [PC] slot -> position
    unsigned *taken = (unsigned *)(opos + PC);                          // [PC / 32] SHARE: the positions already seated
    int *scr = (int *)(taken + PC / 32);                                // [32]
    unsigned char *uni = base + qt_fixed_bytes(PC);
    const int rcap = A.rcap;
    unsigned *A32 = (unsigned *)uni, *B32 = A32 + rcap, *W32 = B32 + rcap;      // records / keys; distinct labels; caps or weights
    unsigned short *C16 = (unsigned short *)(W32 + rcap), *N16 = C16 + rcap, *S16 = N16 + rcap;   // local ids; counters; cursors
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const int n_pool = A.n_pool, n_top = A.n_top;
    const bool share = A.mode == XMAP_QUOTA_SHARE;

    // ---- the pool: m positions
    int m = 0;
    long long seg_a = 0, seg_n = 0;
    bool full = false;
    if constexpr (ROWS) {
        seg_a = A.cand_ptr[q];
        seg_n = A.cand_ptr[q + 1] - seg_a;
        unsigned long long *K = (unsigned long long *)uni;
        unsigned *P = (unsigned *)(K + 2 * PC);
        if (tid == 0) { scr[8] = 0; scr[9] = 0; scr[10] = 0; }
        int dropped = 0, floored = 0;
        au_select_segment<PC, FLOOR>(seg_a, seg_a + seg_n, n_pool, A.rank_by ? A.decay : A.plain, A.status, A.min_score, K, P, &scr[11],
                                     dropped, floored);
        unsigned mine[PC / QT_THREADS];
        int have = 0;
#pragma unroll
        for (int i = 0; i < PC / QT_THREADS; i++) {
            const int j = tid + i * QT_THREADS;
            mine[i] = j < n_pool ? P[j] : AU_NO_POS;
            have += mine[i] != AU_NO_POS ? 1 : 0;
        }
        if (have) atomicAdd(&scr[8], have);
        if (dropped) atomicAdd(&scr[9], dropped);
        if (floored) atomicAdd(&scr[10], floored);
        __syncthreads();                        // K / P are read: the records may take their place
#pragma unroll
        for (int i = 0; i < PC / QT_THREADS; i++) src[tid + i * QT_THREADS] = mine[i];
        m = scr[8];
        full = m == n_pool;
    } else {
        const int c = A.in_cnt[q];
        m = c < 0 ? 0 : c < n_pool ? c : n_pool;
        full = c >= n_pool;
        for (int j = tid; j < PC; j += QT_THREADS) src[j] = (unsigned)j;
    }
    for (int k = tid; k < PC / 32; k += QT_THREADS) taken[k] = 0u;
    __syncthreads();
    const auto item_at = [&](int j) -> int {
        return ROWS ? A.cand_item[seg_a + src[j]] : A.in_item[(size_t)q * n_pool + j];
    };

    // ---- records: poff by a scan of the row lengths, the labels in position order
    int n_rec = 0;
    for (int j0 = 0; j0 < m; j0 += QT_THREADS) {
        const int j = j0 + tid;
        const int c = j < m ? qt_labels(item_at(j), A, [](int, unsigned) {}) : 0;
        int excl, total;
        qt_scan(c, scr, excl, total);
        if (j < m) poff[j] = (unsigned short)(n_rec + excl);
        n_rec += total;
    }
    if (tid == 0) poff[m] = (unsigned short)n_rec;
    int n_sort = 2;
    while (n_sort < n_rec) n_sort <<= 1;        // <= rcap: n_rec <= n_pool x the longest row
    __syncthreads();
    for (int j = tid; j < m; j += QT_THREADS) {
        const int o = poff[j], e = poff[j + 1];
        qt_labels(item_at(j), A, [&](int c, unsigned l) {
            if (o + c < e) { A32[o + c] = l; B32[o + c] = l; }          // (the count pass saw the same table)
        });
    }
    for (int t = n_rec + tid; t < n_sort; t += QT_THREADS) B32[t] = QT_PAD;
    __syncthreads();

    // ---- the distinct labels, ascending, in B32[0 .. D)
    int D = 0;
    if (n_rec > 0) {
        qt_sort(B32, n_sort);
        for (int t0 = 0; t0 < n_rec; t0 += QT_THREADS) {
            const int t = t0 + tid;
            const unsigned v = t < n_rec ? B32[t] : 0u;
            const bool head = t < n_rec && (t == 0 || B32[t - 1] != v);
            int excl, total;
            qt_scan(head ? 1 : 0, scr, excl, total);    // (its barriers stand between the reads above and the writes below)
            if (head) B32[D + excl] = v;                // D + excl <= t: a slot this or an earlier pass has read
            D += total;
            __syncthreads();
        }
    }
    for (int r = tid; r < n_rec; r += QT_THREADS) C16[r] = (unsigned short)qt_find(B32, D, A32[r]);
    for (int d = tid; d < D; d += QT_THREADS) {
        N16[d] = 0;
        const unsigned l = B32[d];
        W32[d] = share ? (A.lab_weight ? A.lab_weight[l] : 0u) : (A.lab_cap ? (unsigned)A.lab_cap[l] : (unsigned)A.cap);
    }
    __syncthreads();
    if (share && !A.lab_weight && D > 0) {      // the history: rows of the user's profile per governed label of the pool
        const int u = A.query_user[q];
        if (u >= 0 && u < A.n_users) {
            const long long pb = A.prof_ptr[u + 1];
            for (long long p = A.prof_ptr[u] + tid; p < pb; p += QT_THREADS)
                qt_labels(A.prof_item[p], A, [&](int, unsigned l) {
                    const int d = qt_find(B32, D, l);
                    if (d >= 0) atomicAdd(&W32[d], 1u);
                });
        }
        __syncthreads();
    }

    int r = 0, third = 0;                       // the slots filled; CAP: positions refused, SHARE: fills
    if (!share) {
        // ---- CAP: greedy in pool order; every thread holds r
        for (int j = 0; j < m && r < n_top; j++) {
            const int o = poff[j], e = poff[j + 1];
            int bad = 0;
            for (int k = o + tid; k < e; k += QT_THREADS) {
                const int d = C16[k];
                bad |= (int)N16[d] >= (int)W32[d] ? 1 : 0;
            }
            if (__syncthreads_or(bad)) { third++; continue; }
            for (int k = o + tid; k < e; k += QT_THREADS) N16[C16[k]]++;       // (the labels of one position are distinct)
            if (tid == 0) opos[r] = (unsigned short)j;
            r++;
            __syncthreads();
        }
    } else {
        // ---- SHARE: per label its positions ascending = the keys (local id, position) sorted; S16[d] = the label's cursor
        for (int j = tid; j < m; j += QT_THREADS)
            for (int k = poff[j]; k < poff[j + 1]; k++) A32[k] = ((unsigned)C16[k] << QT_POS_BITS) | (unsigned)j;
        for (int t = n_rec + tid; t < n_sort; t += QT_THREADS) A32[t] = QT_PAD;
        __syncthreads();
        if (n_rec > 0) qt_sort(A32, n_sort);
        for (int t = tid; t < n_rec; t += QT_THREADS) {
            const unsigned d = A32[t] >> QT_POS_BITS;
            if (t == 0 || (A32[t - 1] >> QT_POS_BITS) != d) S16[d] = (unsigned short)t;
        }
        __syncthreads();
        const int n = m < n_top ? m : n_top;
        int fc = 0;                             // the fill cursor: the first position not yet seated
        unsigned *red = (unsigned *)scr + 16;   // [4][3]
        for (; r < n; r++) {
            unsigned bw = 0, bs = 0;
            int bd = -1;
            for (int d = tid; d < D; d += QT_THREADS) {
                const unsigned w = W32[d];
                if (!w) continue;
                int cur = S16[d];
                while (cur < n_rec && (A32[cur] >> QT_POS_BITS) == (unsigned)d &&
                       ((taken[(A32[cur] & (XMAP_QUOTA_MAX_POOL - 1)) >> 5] >> (A32[cur] & 31)) & 1u))
                    cur++;
                S16[d] = (unsigned short)cur;
                if (cur >= n_rec || (A32[cur] >> QT_POS_BITS) != (unsigned)d) continue;     // no position of the label is left
                const unsigned s = N16[d];
                if (bd < 0 || qt_beats(w, s, d, bw, bs, bd)) { bw = w; bs = s; bd = d; }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const unsigned ow = __shfl_xor(bw, o, 64), os = __shfl_xor(bs, o, 64);
                const int od = __shfl_xor(bd, o, 64);
                if (od >= 0 && (bd < 0 || qt_beats(ow, os, od, bw, bs, bd))) { bw = ow; bs = os; bd = od; }
            }
            if (lane_id() == 0) { red[(tid >> 6) * 3] = bw; red[(tid >> 6) * 3 + 1] = bs; red[(tid >> 6) * 3 + 2] = (unsigned)bd; }
            __syncthreads();
            bd = -1;
#pragma unroll
            for (int w = 0; w < QT_THREADS / 64; w++) {
                const unsigned ow = red[w * 3], os = red[w * 3 + 1];
                const int od = (int)red[w * 3 + 2];
                if (od >= 0 && (bd < 0 || qt_beats(ow, os, od, bw, bs, bd))) { bw = ow; bs = os; bd = od; }
            }
            int j;
            if (bd < 0) {                       // off-profile fill, in pool order
                while ((taken[fc >> 5] >> (fc & 31)) & 1u) fc++;
                j = fc;
                third++;
            } else {
                j = (int)(A32[S16[bd]] & (XMAP_QUOTA_MAX_POOL - 1));
            }
            __syncthreads();                    // every thread has read taken / the cursor / the seats of this slot
            if (tid == 0) {
                taken[j >> 5] |= 1u << (j & 31);
                opos[r] = (unsigned short)j;
                A.out_label[(size_t)q * n_top + r] = bd < 0 ? -1 : (int)B32[bd];
            }
            for (int k = poff[j] + tid; k < poff[j + 1]; k += QT_THREADS) N16[C16[k]]++;
            __syncthreads();
        }
    }
    __syncthreads();

    // ---- outputs
    const int want = m < n_top ? m : n_top;
    int differs = r != want ? 1 : 0;
    for (int t = tid; t < n_top; t += QT_THREADS) {
        const size_t o = (size_t)q * n_top + t;
        if (t < r) {
            const int j = opos[t];
            differs |= j != t ? 1 : 0;
            if constexpr (ROWS) {
                const long long p = seg_a + src[j];
                A.out_item[o] = A.cand_item[p]; A.out_plain[o] = A.plain[p]; A.out_decay[o] = A.decay[p];
            } else {
                const size_t p = (size_t)q * n_pool + j;
                A.out_item[o] = A.in_item[p]; A.out_plain[o] = A.in_plain[p]; A.out_decay[o] = A.in_decay[p];
            }
            A.out_pos[o] = j;
            if (!share) A.out_label[o] = poff[j + 1] > poff[j] ? (int)B32[C16[poff[j]]] : -1;   // (a position's labels ascend)
        } else {
            A.out_item[o] = -1; A.out_plain[o] = 0.0; A.out_decay[o] = 0.0; A.out_pos[o] = -1; A.out_label[o] = -1;
        }
    }
    differs = __syncthreads_or(differs);
    if (tid == 0) {
        A.out_cnt[q] = r;
        if (differs) atomicAdd(&A.st[0], 1ull);
        if (r) atomicAdd(&A.st[1], (unsigned long long)r);
        if (third) atomicAdd(&A.st[2], (unsigned long long)third);
        if (!share && r < n_top && full) atomicAdd(&A.st[3], 1ull);
        if constexpr (ROWS) {
            if (scr[9]) atomicAdd(&A.st[4], (unsigned long long)scr[9]);
            if (scr[10]) atomicAdd(&A.st[6], (unsigned long long)scr[10]);
            atomicMax(&A.st[5], (unsigned long long)seg_n);
        }
    }
}

// rec_model.h: the host checks of the quota calls, each naming its argument; nothing is written
int quota_check_args(const char *who, int64_t n_query, int32_t n_pool, int32_t n_top, int32_t rank_by, int32_t flags, int32_t mode,
                     int32_t cap, bool has_lab_cap, int32_t n_labels) {
#define QT_BAD(cond, ...) do { if (cond) { set_error(__VA_ARGS__); return XMAP_ERR_ARG; } } while (0)
    QT_BAD(n_query < 0 || n_query > (1ll << 28), "%s: n_query = %lld, not in 0 .. 2^28", who, (long long)n_query);
    QT_BAD(n_pool < 1 || n_pool > XMAP_QUOTA_MAX_POOL, "%s: n_pool = %d, not in 1 .. %d", who, n_pool, XMAP_QUOTA_MAX_POOL);
    QT_BAD(n_top < 1 || n_top > n_pool, "%s: n_top = %d, not in 1 .. n_pool = %d", who, n_top, n_pool);
    QT_BAD(rank_by != 0 && rank_by != 1, "%s: rank_by = %d, not 0 or 1", who, rank_by);
    QT_BAD((flags & ~XMAP_TOPN_KEEP_HELD) != 0, "%s: flags = %d, only XMAP_TOPN_KEEP_HELD is known", who, flags);
    QT_BAD(mode != XMAP_QUOTA_CAP && mode != XMAP_QUOTA_SHARE, "%s: mode = %d, not XMAP_QUOTA_CAP or XMAP_QUOTA_SHARE", who, mode);
    QT_BAD(mode == XMAP_QUOTA_CAP && !has_lab_cap && cap < 1, "%s: cap = %d, not >= 1 (lab_cap is NULL)", who, cap);
    QT_BAD(n_labels < 1 || n_labels > XMAP_SHELF_MAX_LABELS, "%s: n_labels = %d, not in 1 .. 2^24", who, n_labels);
#undef QT_BAD
    return XMAP_OK;
}

static int quota_check_out(const char *who, int64_t n_query, const QuotaOut &O) {
    if (n_query > 0 && !(O.cnt && O.item && O.plain && O.decay && O.pos && O.label)) {
        set_error("%s: an output is NULL", who);
        return XMAP_ERR_ARG;
    }
    return XMAP_OK;
}

// The device checks of a quota call, in their order: lab_cap, the label table, the longest label row against n_pool.  *rcap = the
// record slots of a block (a power of two).  Synchronises; nothing is written.
static int quota_check_tables(hipStream_t st, const char *who, int32_t n_pool, const QuotaRule &R, int32_t n_items, const ShelfLabels &L,
                              int *rcap) {
    unsigned long long *dv = nullptr, hv[2] = {RF_NO_POS, 0};
    XM_HIP(xm_malloc_async((void **)&dv, sizeof(hv), st));
    XM_HIP(hipMemcpyAsync(dv, hv, sizeof(hv), hipMemcpyHostToDevice, st));
    if (R.mode == XMAP_QUOTA_CAP && R.lab_cap) {
        const unsigned blocks = blocks_for(L.n_labels, 256) < 1024u ? blocks_for(L.n_labels, 256) : 1024u;
        k_qt_capcheck<<<dim3(blocks), dim3(256), 0, st>>>(L.n_labels, R.lab_cap, dv);
        XM_LAUNCH_CHECK();
        XM_HIP(hipMemcpyAsync(hv, dv, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
        if (hv[0] != RF_NO_POS) {
            set_error("%s: lab_cap is negative: the first at lab_cap[%llu] (0 bars a label, INT32_MAX is no cap)", who, hv[0]);
            return XMAP_ERR_ARG;
        }
    }
    int64_t n_lab = 0;
    int rc = shelf_check_labels(st, who, n_items, L.n_labels, L.lab_ptr, L.lab_id, &n_lab);
    if (rc) return rc;
    if (n_items > 0) {
        const unsigned blocks = blocks_for(n_items, 256) < 1024u ? blocks_for(n_items, 256) : 1024u;
        k_qt_maxrow<<<dim3(blocks), dim3(256), 0, st>>>(n_items, (const long long *)L.lab_ptr, dv + 1);
        XM_LAUNCH_CHECK();
        XM_HIP(hipMemcpyAsync(hv + 1, dv + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
    }
    if ((unsigned long long)n_pool * hv[1] > (unsigned long long)XMAP_QUOTA_MAX_RECORDS) {
        set_error("%s: n_pool = %d x the longest label row = %llu is above XMAP_QUOTA_MAX_RECORDS = %d", who, n_pool, hv[1],
                  XMAP_QUOTA_MAX_RECORDS);
        return XMAP_ERR_ARG;
    }
    int c = 256;
    while ((unsigned long long)c < (unsigned long long)n_pool * hv[1]) c <<= 1;
    *rcap = c;
    return XMAP_OK;
}

template <int PC, bool ROWS>
static hipError_t quota_launch_pc(hipStream_t st, int64_t n_query, const QtArgs &A) {
    const size_t sel = ROWS ? (size_t)24 * PC : 0, back = qt_back_bytes(A.rcap);
    const size_t lds = qt_fixed_bytes(PC) + (sel > back ? sel : back);
    const bool floor = ROWS && A.min_score > -__builtin_inf();
    return launch_dyn_lds(floor ? k_qt<PC, ROWS, true> : k_qt<PC, ROWS, false>, (unsigned)n_query, QT_THREADS, lds, st, A);
}

// the back half of n_query > 0 queries; d_st: the seven counters, zeroed
template <bool ROWS>
static int quota_launch(hipStream_t st, int64_t n_query, const QtArgs &A) {
    hipError_t e;
    if (A.n_pool <= 256) e = quota_launch_pc<256, ROWS>(st, n_query, A);
    else e = quota_launch_pc<1024, ROWS>(st, n_query, A);
    XM_HIP(e);
    return XMAP_OK;
}

static int quota_check_share(const char *who, const QuotaRule &R, const int32_t *query_user, int64_t n_users, const int64_t *prof_ptr,
                             const int32_t *prof_item) {
    if (R.mode != XMAP_QUOTA_SHARE || R.lab_weight) return XMAP_OK;
    if (!query_user || n_users < 0 || !prof_ptr || (n_users > 0 && !prof_item)) {
        set_error("%s: XMAP_QUOTA_SHARE without lab_weight reads the history: query_user, n_users >= 0, prof_ptr, prof_item", who);
        return XMAP_ERR_ARG;
    }
    return XMAP_OK;
}

// rec_model.h: xmap_quota_rows
int quota_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t n_top, int32_t rank_by, int32_t flags,
               const RecModel &M, const QuotaRule &R, const ShelfLabels &L, const QuotaOut &O, const xmap_rec_filter *F, int64_t *h_stats) {
    const char *who = "xmap_quota_rows";
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    int rc = quota_check_args(who, n_query, n_pool, n_top, rank_by, flags, R.mode, R.cap, R.lab_cap != nullptr, L.n_labels);
    if (rc) return rc;
    if ((rc = rec_model_check(M))) return rc;
    XM_ARG(n_query == 0 || query_user);
    if ((rc = quota_check_out(who, n_query, O))) return rc;
    bool filt = false;
    double min_score = 0.0;
    if ((rc = rf_prepare(st, n_query, F, &filt, &min_score))) return rc;
    if (n_query == 0) {
        if (h_stats) for (int k = 0; k < 10; k++) h_stats[k] = 0;
        return XMAP_OK;
    }
    int rcap = 0;
    if ((rc = quota_check_tables(st, who, n_pool, R, M.n_items, L, &rcap))) return rc;
    if (h_stats) for (int k = 0; k < 10; k++) h_stats[k] = 0;
    unsigned long long *d_st = nullptr;         // [0..6] the block's counters, [7] removed by the mask or the exclusion lists
    XM_HIP(xm_malloc_async((void **)&d_st, sizeof(unsigned long long) * 8, st));
    XM_HIP(hipMemsetAsync(d_st, 0, sizeof(unsigned long long) * 8, st));
    TnScored S;
    rc = tn_score_candidates(st, n_query, query_user, flags, M, filt, filt ? (const unsigned int *)F->allow : nullptr,
                             filt ? (const long long *)F->ex_ptr : nullptr, filt ? F->ex_id : nullptr, d_st + 7, &S);
    if (rc) return rc;
    QtArgs A{};
    A.n_pool = n_pool; A.n_top = n_top; A.rcap = rcap; A.mode = R.mode; A.cap = R.cap; A.rank_by = rank_by;
    A.cand_ptr = S.cand_ptr; A.cand_item = S.cand_item; A.plain = S.plain; A.decay = S.decay; A.status = S.status; A.min_score = min_score;
    A.lab_cap = R.lab_cap; A.lab_weight = R.lab_weight; A.query_user = query_user; A.n_users = M.n_users;
    A.prof_ptr = (const long long *)M.prof_ptr; A.prof_item = M.prof_item;
    A.n_items = M.n_items; A.lab_ptr = (const long long *)L.lab_ptr; A.lab_id = L.lab_id; A.lab_allow = L.lab_allow;
    A.out_cnt = O.cnt; A.out_item = O.item; A.out_plain = O.plain; A.out_decay = O.decay; A.out_pos = O.pos; A.out_label = O.label;
    A.st = d_st;
    if ((rc = quota_launch<true>(st, n_query, A))) return rc;
    unsigned long long h[8];
    XM_HIP(hipMemcpyAsync(h, d_st, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = S.n_pairs; h_stats[1] = (int64_t)h[4]; h_stats[2] = S.max_now; h_stats[3] = (int64_t)h[5];
        h_stats[4] = (int64_t)h[6]; h_stats[5] = (int64_t)h[7];
        for (int k = 0; k < 4; k++) h_stats[6 + k] = (int64_t)h[k];
    }
    return XMAP_OK;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_quota_pool(void *stream, int64_t n_query, int32_t n_pool, const int32_t *in_cnt, const int32_t *in_item, const double *in_plain,
                    const double *in_decay, int32_t rank_by, int32_t mode, int32_t cap, const int32_t *lab_cap, const uint32_t *lab_weight,
                    const int32_t *query_user, int64_t n_users, const int64_t *prof_ptr, const int32_t *prof_item, int32_t n_items,
                    int32_t n_labels, const int64_t *lab_ptr, const int32_t *lab_id, const uint32_t *lab_allow, int32_t n_top,
                    int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos, int32_t *out_label,
                    int64_t *h_stats) {
    const char *who = "xmap_quota_pool";
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    const QuotaRule R{mode, cap, lab_cap, lab_weight};
    const ShelfLabels L{n_labels, lab_ptr, lab_id, lab_allow};
    const QuotaOut O{out_cnt, out_item, out_plain, out_decay, out_pos, out_label};
    // the host checks: before any device work
    int rc = quota_check_args(who, n_query, n_pool, n_top, rank_by, 0, mode, cap, lab_cap != nullptr, n_labels);
    if (rc) return rc;
    if (n_items < 0) { set_error("%s: n_items = %d, not >= 0", who, n_items); return XMAP_ERR_ARG; }
    if (n_query > 0 && !(in_cnt && in_item && in_plain && in_decay)) { set_error("%s: a column of the pool is NULL", who); return XMAP_ERR_ARG; }
    if ((rc = quota_check_out(who, n_query, O))) return rc;
    if ((rc = quota_check_share(who, R, query_user, n_users, prof_ptr, prof_item))) return rc;
    if (n_query == 0) {
        if (h_stats) for (int k = 0; k < 4; k++) h_stats[k] = 0;
        return XMAP_OK;
    }
    int rcap = 0;
    if ((rc = quota_check_tables(st, who, n_pool, R, n_items, L, &rcap))) return rc;
    unsigned long long *d_st = nullptr;
    XM_HIP(xm_malloc_async((void **)&d_st, sizeof(unsigned long long) * 8, st));
    XM_HIP(hipMemsetAsync(d_st, 0, sizeof(unsigned long long) * 8, st));
    QtArgs A{};
    A.n_pool = n_pool; A.n_top = n_top; A.rcap = rcap; A.mode = mode; A.cap = cap; A.rank_by = rank_by;
    A.in_cnt = in_cnt; A.in_item = in_item; A.in_plain = in_plain; A.in_decay = in_decay;
    A.lab_cap = lab_cap; A.lab_weight = lab_weight; A.query_user = query_user; A.n_users = n_users;
    A.prof_ptr = (const long long *)prof_ptr; A.prof_item = prof_item;
    A.n_items = n_items; A.lab_ptr = (const long long *)lab_ptr; A.lab_id = lab_id; A.lab_allow = lab_allow;
    A.out_cnt = out_cnt; A.out_item = out_item; A.out_plain = out_plain; A.out_decay = out_decay; A.out_pos = out_pos; A.out_label = out_label;
    A.st = d_st;
    if ((rc = quota_launch<false>(st, n_query, A))) return rc;
    if (h_stats) {
        unsigned long long h[4];
        XM_HIP(hipMemcpyAsync(h, d_st, sizeof(h), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
        for (int k = 0; k < 4; k++) h_stats[k] = (int64_t)h[k];
    }
    return XMAP_OK;
}

int xmap_quota_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags, int64_t n_users,
                    int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim,
                    const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time,
                    const double *item_avg, const double *wtab, int32_t n_w, int32_t n_pool, int32_t mode, int32_t cap,
                    const int32_t *lab_cap, const uint32_t *lab_weight, int32_t n_labels, const int64_t *lab_ptr, const int32_t *lab_id,
                    const uint32_t *lab_allow, int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos,
                    int32_t *out_label, const xmap_rec_filter *F, int64_t *h_stats) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    return quota_rows(stream, n_query, query_user, n_pool, n_top, rank_by, flags, M, QuotaRule{mode, cap, lab_cap, lab_weight},
                      ShelfLabels{n_labels, lab_ptr, lab_id, lab_allow},
                      QuotaOut{out_cnt, out_item, out_plain, out_decay, out_pos, out_label}, F, h_stats);
}
}
