// stage_e_allot.hip -- stock limits: top-N for many queries under item capacities (include/xmap_hip.h, "allotment"; DESIGN.md 4
// "Allotment").  Recipient-proposing deferred acceptance over pools in the top-N layout: every query proposes its first n_top
// positions that are neither void nor refused, every item keeps the cap(i) best offers by (au_key(score), q, j) and refuses the
// rest, until a round refuses nothing.  The refused set only grows and is the least fixed point of a monotone operator, so the
// lists are a pure function of the inputs whatever the schedule of rounds.
//   once:      k_al_keys -> radix_sort_pairs (stable, 64 bits; the initial order is (q, j), so ties fall to the smaller q, then the
//              smaller j) -> k_al_rank: rank[q * n_pool + j] = the place of the position among all positions, < 2^31
//              k_al_void: the refused bitmap [Q][ceil(n_pool / 32)], the void positions set
//   per round: k_al_propose (a wave per query: ballot + popcount over the live bits, one record per pick, fixed slots of n_top,
//              blanks keyed behind every item) -> radix_sort_pairs on item << rank_bits | rank -> k_al_refuse (a thread per
//              record: the record `cap` places ahead holds the same item <=> at least cap better offers of the run precede this
//              one; atomicOr of the position's bit, one integer atomicAdd per wave on the call's counter) -> the host reads the
//              counter; a round that adds nothing ends the loop
//   emit:      k_al_taken over the last round's runs (the thread at the tail of a run finds its head by bisection), k_al_emit (a
//              wave per query writes the lists from the bitmap and the pool)
// Integers only after au_key; integer atomics (atomicOr on bitmap words, atomicAdd on counters); no lock.
#include "rec_model.h"
#include "au_select.h"

namespace xmap {
namespace {

constexpr int AL_WAVES = 4;                     // queries (waves) of a block of the propose / emit kernels
constexpr unsigned long long AL_NONE = ~0ull;
// the call's counters on the device: [0..5] h_stats of the statement ([2], [4] are the host's), [6] positions refused so far
constexpr int AL_ST = 8, AL_ST_REFUSED = 6;

struct AlPool {
    int n_pool, n_top, n_items, cap;
    const int *cnt, *item, *item_cap;
    const double *plain, *decay, *score;        // score = the rank_by column
};

__device__ __forceinline__ int al_cap(const AlPool &P, int i) { return P.item_cap ? P.item_cap[i] : P.cap; }

__global__ __launch_bounds__(256) void k_al_capcheck(int n_items, const int *item_cap, unsigned long long *first) {
    unsigned long long bad = AL_NONE;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += (long long)gridDim.x * blockDim.x)
        if (item_cap[i] < 0 && (unsigned long long)i < bad) bad = (unsigned long long)i;
    if (bad != AL_NONE) atomicMin(first, bad);
}

__global__ __launch_bounds__(256) void k_al_keys(long long n, const double *score, unsigned long long *keys, int *vals) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    keys[t] = au_key(score[t]);
    vals[t] = (int)t;
}

__global__ __launch_bounds__(256) void k_al_rank(long long n, const int *vals, int *rank) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) rank[vals[s]] = (int)s;
}

// one thread per word of the bitmap: bit j of query q is set where position (q, j) is void (or behind n_pool)
__global__ __launch_bounds__(256) void k_al_void(long long n_words, int W, AlPool P, unsigned *bm, unsigned long long *st) {
    const long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n_words) return;
    const long long q = x / W;
    const int w = (int)(x - q * W), c = P.cnt[q];
    const int m = c < 0 ? 0 : (c > P.n_pool ? P.n_pool : c);
    unsigned word = 0u;
    int below = 0;
    for (int b = 0; b < 32; b++) {
        const int j = w * 32 + b;
        bool dead = j >= m;
        if (!dead) {
            const int i = P.item[q * P.n_pool + j];
            dead = (unsigned)i >= (unsigned)P.n_items || al_cap(P, i) == 0;
            below += dead ? 1 : 0;
        }
        word |= (dead ? 1u : 0u) << b;
    }
    bm[x] = word;
    if (below) atomicAdd(&st[3], (unsigned long long)below);
}

// The wave of a query walks its bitmap: pick(idx, j) for the first n_top live positions j, idx = 0, 1, ... in ascending j.
// Returns their number (wave-uniform).
template <class Pick>
__device__ __forceinline__ int al_walk(const unsigned *bmq, int n_pool, int n_top, Pick pick) {
    const int lane = lane_id();
    int have = 0;
    for (int c = 0; c < n_pool && have < n_top; c += WAVE) {
        const int j = c + lane;
        const bool live = j < n_pool && !((bmq[j >> 5] >> (j & 31)) & 1u);
        const unsigned long long mask = __ballot(live);
        const int idx = have + __popcll(mask & lanemask_lt());
        if (live && idx < n_top) pick(idx, j);
        have += __popcll(mask);
    }
    return have < n_top ? have : n_top;
}

// records [Q][n_top]: key = item << rb | rank, value = the flat position; the slots behind a query's picks are blank (item = n_items)
__global__ __launch_bounds__(64 * AL_WAVES) void k_al_propose(long long n_query, int W, int rb, AlPool P, const unsigned *bm,
                                                              const int *rank, unsigned long long *keys, int *vals) {
    const long long q = (long long)blockIdx.x * AL_WAVES + (threadIdx.x >> 6);
    if (q >= n_query) return;
    const long long t0 = q * P.n_pool, o0 = q * P.n_top;
    const int have = al_walk(bm + q * W, P.n_pool, P.n_top, [&](int idx, int j) {
        keys[o0 + idx] = ((unsigned long long)(unsigned)P.item[t0 + j] << rb) | (unsigned long long)(unsigned)rank[t0 + j];
        vals[o0 + idx] = (int)(t0 + j);
    });
    for (int k = have + lane_id(); k < P.n_top; k += WAVE) {
        keys[o0 + k] = (unsigned long long)(unsigned)P.n_items << rb;
        vals[o0 + k] = -1;
    }
}

// the sorted records: an item's offers are one run, best first.  Record t is refused iff cap(item) offers of its run precede it.
__global__ __launch_bounds__(256) void k_al_refuse(long long n, int W, int rb, AlPool P, const unsigned long long *keys, const int *vals,
                                                   unsigned *bm, unsigned long long *st) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool refused = false;
    if (t < n) {
        const unsigned long long i = keys[t] >> rb;
        if (i != (unsigned long long)(unsigned)P.n_items) {
            const long long c = al_cap(P, (int)i);
            refused = t >= c && (keys[t - c] >> rb) == i;
        }
        if (refused) {
            const long long pos = vals[t], q = pos / P.n_pool;
            const int j = (int)(pos - q * P.n_pool);
            atomicOr(&bm[q * W + (j >> 5)], 1u << (j & 31));
        }
    }
    const unsigned long long mask = __ballot(refused);
    if (mask && lane_id() == 0) atomicAdd(&st[AL_ST_REFUSED], (unsigned long long)__popcll(mask));
}

// the records of the last round (nothing was refused): taken[item] = the length of its run; taken is zeroed
__global__ __launch_bounds__(256) void k_al_taken(long long n, int rb, int n_items, const unsigned long long *keys, int *taken) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const unsigned long long i = keys[t] >> rb;
    if (i == (unsigned long long)(unsigned)n_items) return;
    if (t + 1 < n && (keys[t + 1] >> rb) == i) return;          // not the tail of its run
    long long lo = 0, hi = t;                   // the first record of item i
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((keys[mid] >> rb) >= i) hi = mid; else lo = mid + 1;
    }
    taken[i] = (int)(t - lo + 1);
}

__global__ __launch_bounds__(64 * AL_WAVES) void k_al_emit(long long n_query, int W, AlPool P, const unsigned *bm, int *out_cnt,
                                                           int *out_item, double *out_plain, double *out_decay, int *out_pos,
                                                           unsigned long long *st) {
    const long long q = (long long)blockIdx.x * AL_WAVES + (threadIdx.x >> 6);
    if (q >= n_query) return;
    const long long t0 = q * P.n_pool, o0 = q * P.n_top;
    bool moved = false;
    const int have = al_walk(bm + q * W, P.n_pool, P.n_top, [&](int idx, int j) {
        out_item[o0 + idx] = P.item[t0 + j];
        out_plain[o0 + idx] = P.plain[t0 + j];
        out_decay[o0 + idx] = P.decay[t0 + j];
        out_pos[o0 + idx] = j;
        moved |= j != idx;
    });
    for (int k = have + lane_id(); k < P.n_top; k += WAVE) {
        out_item[o0 + k] = -1; out_plain[o0 + k] = 0.0; out_decay[o0 + k] = 0.0; out_pos[o0 + k] = -1;
    }
    const bool any_moved = __ballot(moved) != 0ull;
    if (lane_id() == 0) {
        const int c = P.cnt[q], m = c < 0 ? 0 : (c > P.n_pool ? P.n_pool : c);
        out_cnt[q] = have;
        if (any_moved || have != (m < P.n_top ? m : P.n_top)) atomicAdd(&st[0], 1ull);
        if (have) atomicAdd(&st[1], (unsigned long long)have);
        if (have < P.n_top && c >= P.n_pool) atomicAdd(&st[5], 1ull);
    }
}

// the caps on the device, before any other device work: the first negative entry is named, nothing is written
int allot_check_caps(hipStream_t st, const char *who, int n_items, const int *item_cap) {
    if (!item_cap || n_items == 0) return XMAP_OK;
    unsigned long long *dv = nullptr, hv = AL_NONE;
    XM_HIP(xm_malloc_async((void **)&dv, sizeof(hv), st));
    XM_HIP(hipMemcpyAsync(dv, &hv, sizeof(hv), hipMemcpyHostToDevice, st));
    const unsigned blocks = blocks_for(n_items, 256) < 1024u ? blocks_for(n_items, 256) : 1024u;
    k_al_capcheck<<<dim3(blocks), dim3(256), 0, st>>>(n_items, item_cap, dv);
    XM_LAUNCH_CHECK();
    XM_HIP(hipMemcpyAsync(&hv, dv, sizeof(hv), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (hv != AL_NONE) {
        set_error("%s: item_cap is negative: the first at item_cap[%llu] (0 bars an item, INT32_MAX is no cap)", who, hv);
        return XMAP_ERR_ARG;
    }
    return XMAP_OK;
}

// the allotment over n_query > 0 checked pools; h6: the six of the statement
int allot_run(hipStream_t st, long long n_query, const AlPool &P, const AllotOut &O, int64_t *h6) {
    const long long N = n_query * P.n_pool, n_rec = n_query * P.n_top;
    const int W = (P.n_pool + 31) / 32, rb = bits_for(N);
    const long long n_words = n_query * W;
    unsigned long long *keys = nullptr, *d_st = nullptr;
    int *vals = nullptr, *rank = nullptr;
    unsigned *bm = nullptr;
    XM_HIP(xm_malloc_async((void **)&keys, sizeof(unsigned long long) * 2 * (size_t)N, st));
    XM_HIP(xm_malloc_async((void **)&vals, sizeof(int) * 2 * (size_t)N, st));
    XM_HIP(xm_malloc_async((void **)&rank, sizeof(int) * (size_t)N, st));
    XM_HIP(xm_malloc_async((void **)&bm, sizeof(unsigned) * (size_t)n_words, st));
    XM_HIP(xm_malloc_async((void **)&d_st, sizeof(unsigned long long) * AL_ST, st));
    XM_HIP(hipMemsetAsync(d_st, 0, sizeof(unsigned long long) * AL_ST, st));
    // ---- once: the place of every position in the offer order, the void positions
    k_al_keys<<<dim3(blocks_for(N, 256)), dim3(256), 0, st>>>(N, P.score, keys, vals);
    XM_LAUNCH_CHECK();
    int rc = radix_sort_pairs(st, keys, vals, keys + N, vals + N, N, 64);
    if (rc) return rc;
    k_al_rank<<<dim3(blocks_for(N, 256)), dim3(256), 0, st>>>(N, vals, rank);
    XM_LAUNCH_CHECK();
    k_al_void<<<dim3(blocks_for(n_words, 256)), dim3(256), 0, st>>>(n_words, W, P, bm, d_st);
    XM_LAUNCH_CHECK();
    // ---- the rounds: every round but the last adds to the refused set, which holds at most N positions
    const unsigned qblocks = blocks_for(n_query, AL_WAVES);
    const int bits = rb + bits_for((long long)P.n_items + 1);
    unsigned long long refused = 0;
    int64_t rounds = 0;
    for (;;) {
        k_al_propose<<<dim3(qblocks), dim3(64 * AL_WAVES), 0, st>>>(n_query, W, rb, P, bm, rank, keys, vals);
        XM_LAUNCH_CHECK();
        if ((rc = radix_sort_pairs(st, keys, vals, keys + N, vals + N, n_rec, bits))) return rc;
        k_al_refuse<<<dim3(blocks_for(n_rec, 256)), dim3(256), 0, st>>>(n_rec, W, rb, P, keys, vals, bm, d_st);
        XM_LAUNCH_CHECK();
        unsigned long long now = 0;
        XM_HIP(hipMemcpyAsync(&now, d_st + AL_ST_REFUSED, sizeof(now), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
        rounds++;
        if (now == refused) break;
        refused = now;
    }
    // ---- the lists, and the offers every item holds
    if (O.taken && P.n_items > 0) {
        XM_HIP(hipMemsetAsync(O.taken, 0, sizeof(int) * (size_t)P.n_items, st));
        k_al_taken<<<dim3(blocks_for(n_rec, 256)), dim3(256), 0, st>>>(n_rec, rb, P.n_items, keys, O.taken);
        XM_LAUNCH_CHECK();
    }
    k_al_emit<<<dim3(qblocks), dim3(64 * AL_WAVES), 0, st>>>(n_query, W, P, bm, O.cnt, O.item, O.plain, O.decay, O.pos, d_st);
    XM_LAUNCH_CHECK();
    unsigned long long h[AL_ST];
    XM_HIP(hipMemcpyAsync(h, d_st, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h6) {
        h6[0] = (int64_t)h[0]; h6[1] = (int64_t)h[1]; h6[2] = (int64_t)refused; h6[3] = (int64_t)h[3]; h6[4] = rounds;
        h6[5] = (int64_t)h[5];
    }
    return XMAP_OK;
}

int allot_check_out(const char *who, int64_t n_query, const AllotOut &O) {
    if (n_query > 0 && !(O.cnt && O.item && O.plain && O.decay && O.pos)) {
        set_error("%s: an output is NULL", who);
        return XMAP_ERR_ARG;
    }
    return XMAP_OK;
}

}  // namespace

// rec_model.h: the host checks of the allot calls, each naming its argument; nothing is written
int allot_check_args(const char *who, int64_t n_query, int32_t n_pool, int32_t max_pool, int32_t n_top, int32_t rank_by, int32_t flags,
                     int32_t cap, bool has_item_cap) {
#define AL_BAD(cond, ...) do { if (cond) { set_error(__VA_ARGS__); return XMAP_ERR_ARG; } } while (0)
    AL_BAD(n_query < 0, "%s: n_query = %lld, not >= 0", who, (long long)n_query);
    AL_BAD(n_pool < 1 || n_pool > max_pool, "%s: n_pool = %d, not in 1 .. %d", who, n_pool, max_pool);
    AL_BAD(n_query >= (1ll << 31) || n_query * n_pool >= (1ll << 31), "%s: n_query * n_pool = %lld * %d, not below 2^31", who,
           (long long)n_query, n_pool);
    AL_BAD(n_top < 1 || n_top > n_pool, "%s: n_top = %d, not in 1 .. n_pool = %d", who, n_top, n_pool);
    AL_BAD(rank_by != 0 && rank_by != 1, "%s: rank_by = %d, not 0 or 1", who, rank_by);
    AL_BAD((flags & ~XMAP_TOPN_KEEP_HELD) != 0, "%s: flags = %d, only XMAP_TOPN_KEEP_HELD is known", who, flags);
    AL_BAD(!has_item_cap && cap < 1, "%s: cap = %d, not >= 1 (item_cap is NULL)", who, cap);
#undef AL_BAD
    return XMAP_OK;
}

// rec_model.h: xmap_allot_rows
int allot_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t n_top, int32_t rank_by, int32_t flags,
               const RecModel &M, int32_t cap, const int32_t *item_cap, const AllotOut &O, const xmap_rec_filter *F, int64_t *h_stats) {
    const char *who = "xmap_allot_rows";
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    int rc = allot_check_args(who, n_query, n_pool, 64, n_top, rank_by, flags, cap, item_cap != nullptr);
    if (rc) return rc;
    if ((rc = rec_model_check(M))) return rc;
    XM_ARG(n_query == 0 || query_user);
    if ((rc = allot_check_out(who, n_query, O))) return rc;
    if ((rc = allot_check_caps(st, who, M.n_items, item_cap))) return rc;
    int64_t h12[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // the pool: by definition what xmap_topn_rows_filtered returns with n_top = n_pool
    const size_t nq = (size_t)(n_query ? n_query : 1), np = nq * (size_t)n_pool;
    int *p_cnt = nullptr, *p_item = nullptr;
    double *p_plain = nullptr, *p_decay = nullptr;
    XM_HIP(xm_malloc_async((void **)&p_cnt, sizeof(int) * nq, st));
    XM_HIP(xm_malloc_async((void **)&p_item, sizeof(int) * np, st));
    XM_HIP(xm_malloc_async((void **)&p_plain, sizeof(double) * np, st));
    XM_HIP(xm_malloc_async((void **)&p_decay, sizeof(double) * np, st));
    if ((rc = topn_rows(stream, n_query, query_user, n_pool, rank_by, flags, M, p_cnt, p_item, p_plain, p_decay, F, h12, 6))) return rc;
    if (n_query > 0) {
        const AlPool P{n_pool, n_top, M.n_items, cap, p_cnt, p_item, item_cap, p_plain, p_decay, rank_by ? p_decay : p_plain};
        if ((rc = allot_run(st, n_query, P, O, h12 + 6))) return rc;
    } else if (O.taken && M.n_items > 0) {
        XM_HIP(hipMemsetAsync(O.taken, 0, sizeof(int) * (size_t)M.n_items, st));
        XM_HIP(hipStreamSynchronize(st));
    }
    if (h_stats) for (int k = 0; k < 12; k++) h_stats[k] = h12[k];
    return XMAP_OK;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_allot_pool(void *stream, int64_t n_query, int32_t n_pool, const int32_t *in_cnt, const int32_t *in_item, const double *in_plain,
                    const double *in_decay, int32_t rank_by, int32_t n_items, int32_t cap, const int32_t *item_cap, int32_t n_top,
                    int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos, int32_t *item_taken,
                    int64_t *h_stats) {
    const char *who = "xmap_allot_pool";
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    const AllotOut O{out_cnt, out_item, out_plain, out_decay, out_pos, item_taken};
    // the host checks: before any device work
    int rc = allot_check_args(who, n_query, n_pool, XMAP_ALLOT_MAX_POOL, n_top, rank_by, 0, cap, item_cap != nullptr);
    if (rc) return rc;
    if (n_items < 0) { set_error("%s: n_items = %d, not >= 0", who, n_items); return XMAP_ERR_ARG; }
    if (n_query > 0 && !(in_cnt && in_item && in_plain && in_decay)) { set_error("%s: a column of the pool is NULL", who); return XMAP_ERR_ARG; }
    if ((rc = allot_check_out(who, n_query, O))) return rc;
    if ((rc = allot_check_caps(st, who, n_items, item_cap))) return rc;
    if (n_query == 0) {
        if (item_taken && n_items > 0) {
            XM_HIP(hipMemsetAsync(item_taken, 0, sizeof(int) * (size_t)n_items, st));
            XM_HIP(hipStreamSynchronize(st));
        }
        if (h_stats) for (int k = 0; k < 6; k++) h_stats[k] = 0;
        return XMAP_OK;
    }
    const AlPool P{n_pool, n_top, n_items, cap, in_cnt, in_item, item_cap, in_plain, in_decay, rank_by ? in_decay : in_plain};
    return allot_run(st, n_query, P, O, h_stats);
}

int xmap_allot_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t rank_by, int32_t flags,
                    int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim,
                    const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time,
                    const double *item_avg, const double *wtab, int32_t n_w, int32_t n_top, int32_t cap, const int32_t *item_cap,
                    int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos, int32_t *item_taken,
                    const xmap_rec_filter *F, int64_t *h_stats) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    return allot_rows(stream, n_query, query_user, n_pool, n_top, rank_by, flags, M, cap, item_cap,
                      AllotOut{out_cnt, out_item, out_plain, out_decay, out_pos, item_taken}, F, h_stats);
}
}
