// predict_rows.h -- the pair body of the device-resident prediction, shared by k_predict_rows (stage_e_rows.hip: the bounded
// predictions of item_based_prediction) and the scoring pass of the top-N recommendation (stage_e_topn.hip: the same two
// values before bound_rating).  One body with a compile-time switch: the two kernels are the same code.
#pragma once
#include "common.h"

namespace xmap {

constexpr int PR_CAP = 128;        // evidence entries of a pair staged in LDS (6 KB per wave)
constexpr int PR_WAVES = 4;

__device__ __forceinline__ double bound_rating_rows(double r) {
    const double x = r + 0.5;       // max(0, min(int(x), 5)): int() truncates towards zero
    return x >= 5.0 ? 5.0 : (x < 1.0 ? 0.0 : (double)(long long)x);
}

template <bool ARENA>
__device__ __forceinline__ void wave_sync() {
    if constexpr (ARENA) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
    else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ARENA = false: pair = wave index; a pair with more than PR_CAP evidence entries is appended to ovf_list with an arena
// offset (ovf[0] pairs, ovf[1] entries) and left for the second launch.  ARENA = true: wave w takes (pair, offset) =
// ovf_list[2 w ..] and stages its evidence in arena[6 offset ..].
// RAW = false: item_based_prediction (the bounded predictions, status 1 for an item without a list).  RAW = true: the two values
// as they stand before bound_rating (the scores the top-N selection ranks, stage_e_topn.hip); nothing else differs.
template <bool ARENA, bool RAW>
__device__ __forceinline__ void predict_pair(
    long long n_work, const int *tu, const int *ti, long long U, int I, int keep, const int *nb_cnt, const int *nb_col,
    const double *nb_sim, const long long *pptr, const int *pitem, const double *prating, const long long *ptime,
    const double *avg, const double *wtab, int n_w, double *out_plain, double *out_decay, int *status, int *max_now,
    unsigned long long *ovf, long long *ovf_list, double *arena) {
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const long long w = (long long)blockIdx.x * PR_WAVES + wv;
    if (w >= n_work) return;
    const long long t = ARENA ? ovf_list[2 * w] : w;
    const int u = tu[t], it = ti[t];
    int cnt = (it >= 0 && it < I) ? nb_cnt[it] : 0;
    cnt = cnt < keep ? cnt : keep;
    if (cnt <= 0) {       // item without a neighbour list: ()
        if (lane == 0) { status[t] = 1; out_plain[t] = 0.0; out_decay[t] = 0.0; }
        return;
    }
    const double base = avg[it];
    int nb = -1;
    double s = 0.0, navg = 0.0;
    if (lane < cnt) {
        const size_t o = (size_t)it * keep + lane;
        nb = nb_col[o];
        if (nb < 0 || nb >= I) nb = -1;
        else { s = nb_sim[o]; navg = avg[nb]; }
    }
    long long a = 0, b = 0;
    if (u >= 0 && u < U) { a = pptr[u]; b = pptr[u + 1]; }
    // count pass: rows of the user's profile that hold this lane's neighbour
    int c = 0;
    for (long long p = a; p < b; p += 64) {
        const int pit = (p + lane < b) ? pitem[p + lane] : -2;
        const int lim = (int)min(64ll, b - p);
        for (int j = 0; j < lim; j++) c += (rl32(pit, j) == nb) ? 1 : 0;
    }
    int incl = c;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int o = __shfl_up(incl, m, 64);
        if (lane >= m) incl += o;
    }
    const int n = rl32(incl, 63);
    double plain = base, decayed = base;
    bool bad = !isfinite(base);
    if (n > 0) {
        double *e0, *e1, *s0, *s1;
        long long *tm, *st;
        if constexpr (ARENA) {
            double *slice = arena + 6 * (size_t)ovf_list[2 * w + 1];
            e0 = slice; e1 = e0 + n; s0 = e1 + n; s1 = s0 + n;
            tm = (long long *)(s1 + n); st = tm + n;
        } else {
            if (n > PR_CAP) {
                if (lane == 0) {
                    const unsigned long long slot = atomicAdd(&ovf[0], 1ull);
                    const unsigned long long off = atomicAdd(&ovf[1], (unsigned long long)n);
                    ovf_list[2 * slot] = t; ovf_list[2 * slot + 1] = (long long)off;
                    status[t] = 3;       // pending: the arena launch decides it
                }
                return;
            }
            __shared__ double sh_d[PR_WAVES][4 * PR_CAP];
            __shared__ long long sh_t[PR_WAVES][2 * PR_CAP];
            e0 = sh_d[wv]; e1 = e0 + PR_CAP; s0 = e1 + PR_CAP; s1 = s0 + PR_CAP;
            tm = sh_t[wv]; st = tm + PR_CAP;
        }
        // fill pass: evidence order = neighbour-list order, within a neighbour the user's rows in profile order
        int k = incl - c;
        for (long long p = a; p < b; p += 64) {
            const bool in = p + lane < b;
            const int pit = in ? pitem[p + lane] : -2;
            const double pr = in ? prating[p + lane] : 0.0;
            const long long pt = in ? ptime[p + lane] : 0;
            const int lim = (int)min(64ll, b - p);
            for (int j = 0; j < lim; j++) {
                const int ji = rl32(pit, j);
                const double jr = rld(pr, j);
                const long long jt = rl64(pt, j);
                if (ji == nb) { e0[k] = s * (jr - navg); e1[k] = fabs(s); tm[k] = jt; k++; }
            }
        }
        wave_sync<ARENA>();
        double p0 = 0.0, p1 = 0.0;          // Python's sum(): left to right
        for (int q = 0; q < n; q++) { p0 += e0[q]; p1 += e1[q]; }
        plain = base + p0 / p1;
        // stable order by time: position = entries with a smaller time + earlier entries with the same time
        for (int q = lane; q < n; q += 64) {
            const long long tq = tm[q];
            int pos = 0;
            for (int j = 0; j < n; j++) {
                const long long tj = tm[j];
                pos += (tj < tq || (tj == tq && j < q)) ? 1 : 0;
            }
            s0[pos] = e0[q]; s1[pos] = e1[q]; st[pos] = tq;
        }
        wave_sync<ARENA>();
        int ranks = 0;                        // distinct times
        for (int q0 = 0; q0 < n; q0 += 64) {
            const int q = q0 + lane;
            const bool fresh = q < n && (q == 0 || st[q] != st[q - 1]);
            ranks += __popcll(__ballot(fresh));
        }
        const int now = ranks + 1;
        if (lane == 0) atomicMax(max_now, now);
        if (now > n_w) bad = true;            // the decay table is too short
        else {
            double d0 = 0.0, d1 = 0.0;
            int r = 0;
            long long prev = 0;
            for (int q = 0; q < n; q++) {
                const long long tq = st[q];
                if (q == 0 || tq != prev) r++;
                prev = tq;
                const double wt = wtab[now - r];
                d0 += s0[q] * wt; d1 += s1[q] * wt;
            }
            decayed = base + d0 / d1;
            // where Python raises (zero weight sum, int() of an infinity or a NaN): status 2
            if (p1 == 0.0 || d1 == 0.0 || !isfinite(plain) || !isfinite(decayed)) bad = true;
        }
    }
    if (lane == 0) {
        status[t] = bad ? 2 : 0;
        out_plain[t] = bad ? 0.0 : (RAW ? plain : bound_rating_rows(plain));
        out_decay[t] = bad ? 0.0 : (RAW ? decayed : bound_rating_rows(decayed));
    }
}

template <bool ARENA, bool RAW>
__global__ __launch_bounds__(64 * PR_WAVES) void k_predict_rows(
    long long n_work, const int *tu, const int *ti, long long U, int I, int keep, const int *nb_cnt, const int *nb_col,
    const double *nb_sim, const long long *pptr, const int *pitem, const double *prating, const long long *ptime,
    const double *avg, const double *wtab, int n_w, double *out_plain, double *out_decay, int *status, int *max_now,
    unsigned long long *ovf, long long *ovf_list, double *arena) {
    predict_pair<ARENA, RAW>(n_work, tu, ti, U, I, keep, nb_cnt, nb_col, nb_sim, pptr, pitem, prating, ptime, avg, wtab, n_w, out_plain,
                             out_decay, status, max_now, ovf, ovf_list, arena);
}

// The two launches of the pair kernel over n_test pairs (device arrays): the wave-per-pair launch, then -- for the pairs whose
// evidence does not fit the LDS staging -- the same kernel over an arena of exactly the entries the first launch counted.
// One host wait per launch.  *h_max_now (may be NULL) = the largest `now` met.
template <bool RAW>
static int predict_rows_run(hipStream_t st, int64_t n_test, const int32_t *test_user, const int32_t *test_item, int64_t n_users,
                            int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim,
                            const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time,
                            const double *item_avg, const double *wtab, int32_t n_w, double *out_plain, double *out_decay,
                            int32_t *status, int32_t *h_max_now) {
    XM_SCOPE(st);
    if (h_max_now) *h_max_now = 0;
    if (n_test == 0) return XMAP_OK;
    unsigned long long *ctl = nullptr;          // [0], [1]: overflowed pairs, their evidence entries; [2]: largest `now`
    long long *ovf_list = nullptr;
    XM_HIP(xm_malloc_async((void **)&ctl, sizeof(unsigned long long) * 3, st));
    XM_HIP(xm_malloc_async((void **)&ovf_list, sizeof(long long) * 2 * (size_t)n_test, st));
    XM_HIP(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * 3, st));
    int *max_now = (int *)(ctl + 2);
    k_predict_rows<false, RAW><<<dim3((unsigned)((n_test + PR_WAVES - 1) / PR_WAVES)), dim3(64 * PR_WAVES), 0, st>>>(
        n_test, test_user, test_item, n_users, n_items, keep, nb_cnt, nb_col, nb_sim, (const long long *)prof_ptr, prof_item, prof_rating,
        (const long long *)prof_time, item_avg, wtab, n_w, out_plain, out_decay, status, max_now, ctl, ovf_list, nullptr);
    XM_LAUNCH_CHECK();
    unsigned long long h[3] = {0, 0, 0};
    XM_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h[0] > 0) {       // pairs whose evidence does not fit the LDS staging: the same kernel over an arena of exactly h[1] entries
        double *arena = nullptr;
        XM_HIP(xm_malloc_async((void **)&arena, sizeof(double) * 6 * (size_t)h[1], st));
        k_predict_rows<true, RAW><<<dim3((unsigned)((h[0] + PR_WAVES - 1) / PR_WAVES)), dim3(64 * PR_WAVES), 0, st>>>(
            (long long)h[0], test_user, test_item, n_users, n_items, keep, nb_cnt, nb_col, nb_sim, (const long long *)prof_ptr, prof_item,
            prof_rating, (const long long *)prof_time, item_avg, wtab, n_w, out_plain, out_decay, status, max_now, ctl, ovf_list, arena);
        XM_LAUNCH_CHECK();
        XM_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
    }
    if (h_max_now) *h_max_now = (int32_t)(h[2] & 0xffffffffull);
    return XMAP_OK;
}

}  // namespace xmap
