// stage_e_rows.hip -- the device-resident recommender tail: from the AlterEgo rows stage C leaves in HBM to predictions
// and MAE without a host conversion (reference core/recommenderSim.py -> core/recommenderPrivacy.py ->
// core/recommenderPrediction.py:26-139; DESIGN.md 4 "RecommenderSim").
//
//   k_rec_profiles  : stage-C rows (pass-through segment, then mapped segment, both in user order) -> user-major profiles
//                     in stage-C row order; one row per thread, the destination follows from the two per-user offsets.
//   k_predict_rows  : item_based_prediction, one WAVE per test pair, lanes = the neighbours of the test item.  Every lane
//                     looks its neighbour up in the test user's profile (the profile streams through the wave 64 rows at
//                     a time, one readlane per row), a prefix scan over the lanes gives the evidence offsets, the
//                     evidence (sim * (rating - neighbour average), |sim|, time) is staged in evidence order -- in LDS
//                     for up to PR_CAP entries, else in an arena slice sized by this count pass (second launch over the
//                     pairs that overflowed) --, the plain sums run left to right over it, the stable time order is a
//                     rank count per entry, the decayed sums run left to right over the sorted copy.  Same operations in
//                     the same order as RecommenderPrediction._predict_pair; there is no limit on the evidence of a pair.
//   k_mae_*         : count of predicted pairs, sum |real - plain|, sum |real - decayed| as double-double sums rounded once.
#include "common.h"

namespace xmap {

__global__ __launch_bounds__(256) void k_rec_profiles(long long U, long long n, long long n_t, const long long *off_t,
                                                      const long long *off_m, const int *user, const int *item,
                                                      const double *rating, const long long *time, long long *pptr, int *pitem,
                                                      double *prating, long long *ptime) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= U) pptr[q] = off_t[q] + off_m[q];
    if (q >= n) return;
    const long long u = user[q];
    if (u < 0 || u >= U) return;
    const long long ot = off_t[u], om = off_m[u];
    const long long dst = ot + om + (q < n_t ? q - ot : (off_t[u + 1] - ot) + (q - n_t - om));
    if (dst < 0 || dst >= n) return;
    pitem[dst] = item[q]; prating[dst] = rating[q]; ptime[dst] = time[q];
}

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
template <bool ARENA>
__global__ __launch_bounds__(64 * PR_WAVES) void k_predict_rows(
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
        out_plain[t] = bad ? 0.0 : bound_rating_rows(plain);
        out_decay[t] = bad ? 0.0 : bound_rating_rows(decayed);
    }
}

// ---- MAE (calculate_mae, core/recommenderPrediction.py:107-139): exact sums, so the result does not depend on the grid
constexpr int MAE_BLOCKS = 256;
__global__ __launch_bounds__(256) void k_mae_partial(long long n, const int *status, const double *real, const double *plain,
                                                     const double *decay, double *part /*[MAE_BLOCKS][5]*/) {
    double ph = 0.0, pl = 0.0, dh = 0.0, dl = 0.0, cn = 0.0;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
        if (status[q] != 0) continue;
        dd_add(ph, pl, fabs(real[q] - plain[q]));
        dd_add(dh, dl, fabs(real[q] - decay[q]));
        cn += 1.0;
    }
    dd_reduce<64>(ph, pl);
    dd_reduce<64>(dh, dl);
    cn = wave_sum(cn);
    __shared__ double sh[4][5];
    const int wv = threadIdx.x >> 6;
    if (lane_id() == 0) { sh[wv][0] = ph; sh[wv][1] = pl; sh[wv][2] = dh; sh[wv][3] = dl; sh[wv][4] = cn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, al = 0.0, b = 0.0, bl = 0.0, c = 0.0;
        for (int x = 0; x < 4; x++) {
            dd_add(a, al, sh[x][0]); dd_add(a, al, sh[x][1]);
            dd_add(b, bl, sh[x][2]); dd_add(b, bl, sh[x][3]);
            c += sh[x][4];
        }
        double *o = part + (size_t)blockIdx.x * 5;
        o[0] = a; o[1] = al; o[2] = b; o[3] = bl; o[4] = c;
    }
}

__global__ __launch_bounds__(64) void k_mae_final(int n_part, const double *part, double *out /*[3]*/) {
    if (threadIdx.x != 0) return;
    double a = 0.0, al = 0.0, b = 0.0, bl = 0.0, c = 0.0;
    for (int x = 0; x < n_part; x++) {
        const double *p = part + (size_t)x * 5;
        dd_add(a, al, p[0]); dd_add(a, al, p[1]);
        dd_add(b, bl, p[2]); dd_add(b, bl, p[3]);
        c += p[4];             // counts: integers below 2^53, exact
    }
    out[0] = c; out[1] = a; out[2] = b;
}

}  // namespace xmap
using namespace xmap;

extern "C" {

int xmap_rec_profiles(void *stream, int64_t n_users, int64_t n_rows, int64_t n_target_rows, const int64_t *off_t, const int64_t *off_m,
                      const int32_t *user, const int32_t *item, const double *rating, const int64_t *time, int64_t *prof_ptr,
                      int32_t *prof_item, double *prof_rating, int64_t *prof_time) {
    XM_ARG(off_t && off_m && prof_ptr && n_users >= 0 && n_rows >= 0 && n_target_rows >= 0 && n_target_rows <= n_rows);
    XM_ARG(n_rows == 0 || (user && item && rating && time && prof_item && prof_rating && prof_time));
    const long long m = (n_rows > n_users + 1) ? n_rows : n_users + 1;
    k_rec_profiles<<<dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        n_users, n_rows, n_target_rows, (const long long *)off_t, (const long long *)off_m, user, item, rating, (const long long *)time,
        (long long *)prof_ptr, prof_item, prof_rating, (long long *)prof_time);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

int xmap_predict_rows(void *stream, int64_t n_test, const int32_t *test_user, const int32_t *test_item, int64_t n_users,
                      int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim,
                      const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time,
                      const double *item_avg, const double *wtab, int32_t n_w, double *out_plain, double *out_decay,
                      int32_t *status, int32_t *h_max_now) {
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    XM_ARG(n_test >= 0 && n_users >= 0 && n_items >= 0 && keep >= 1 && keep <= 64 && n_w >= 1 && wtab && prof_ptr);
    XM_ARG(n_test == 0 || (test_user && test_item && nb_cnt && nb_col && nb_sim && item_avg && out_plain && out_decay && status));
    XM_ARG(prof_ptr && (n_users == 0 || (prof_item && prof_rating && prof_time)));
    if (h_max_now) *h_max_now = 0;
    if (n_test == 0) return XMAP_OK;
    unsigned long long *ctl = nullptr;          // [0], [1]: overflowed pairs, their evidence entries; [2]: largest `now`
    long long *ovf_list = nullptr;
    XM_HIP(xm_malloc_async((void **)&ctl, sizeof(unsigned long long) * 3, st));
    XM_HIP(xm_malloc_async((void **)&ovf_list, sizeof(long long) * 2 * (size_t)n_test, st));
    XM_HIP(hipMemsetAsync(ctl, 0, sizeof(unsigned long long) * 3, st));
    int *max_now = (int *)(ctl + 2);
    k_predict_rows<false><<<dim3((unsigned)((n_test + PR_WAVES - 1) / PR_WAVES)), dim3(64 * PR_WAVES), 0, st>>>(
        n_test, test_user, test_item, n_users, n_items, keep, nb_cnt, nb_col, nb_sim, (const long long *)prof_ptr, prof_item, prof_rating,
        (const long long *)prof_time, item_avg, wtab, n_w, out_plain, out_decay, status, max_now, ctl, ovf_list, nullptr);
    XM_LAUNCH_CHECK();
    unsigned long long h[3] = {0, 0, 0};
    XM_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h[0] > 0) {       // pairs whose evidence does not fit the LDS staging: the same kernel over an arena of exactly h[1] entries
        double *arena = nullptr;
        XM_HIP(xm_malloc_async((void **)&arena, sizeof(double) * 6 * (size_t)h[1], st));
        k_predict_rows<true><<<dim3((unsigned)((h[0] + PR_WAVES - 1) / PR_WAVES)), dim3(64 * PR_WAVES), 0, st>>>(
            (long long)h[0], test_user, test_item, n_users, n_items, keep, nb_cnt, nb_col, nb_sim, (const long long *)prof_ptr, prof_item,
            prof_rating, (const long long *)prof_time, item_avg, wtab, n_w, out_plain, out_decay, status, max_now, ctl, ovf_list, arena);
        XM_LAUNCH_CHECK();
        XM_HIP(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
    }
    if (h_max_now) *h_max_now = (int32_t)(h[2] & 0xffffffffull);
    return XMAP_OK;
}

int xmap_mae(void *stream, int64_t n_test, const int32_t *status, const double *real, const double *out_plain, const double *out_decay,
             double *mae /*[3] device*/) {
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    XM_ARG(mae && n_test >= 0 && (n_test == 0 || (status && real && out_plain && out_decay)));
    double *part = nullptr;
    XM_HIP(xm_malloc_async((void **)&part, sizeof(double) * 5 * MAE_BLOCKS, st));
    int blocks = (int)((n_test + 255) / 256);
    blocks = blocks < 1 ? 1 : (blocks > MAE_BLOCKS ? MAE_BLOCKS : blocks);
    k_mae_partial<<<dim3(blocks), dim3(256), 0, st>>>(n_test, status, real, out_plain, out_decay, part);
    XM_LAUNCH_CHECK();
    k_mae_final<<<dim3(1), dim3(64), 0, st>>>(blocks, part, mae);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}
}
