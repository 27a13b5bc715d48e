// stage_e_rows.hip -- the device-resident recommender tail: from the AlterEgo rows stage C leaves in HBM to predictions
// and MAE without a host conversion (reference core/recommenderSim.py -> core/recommenderPrivacy.py ->
// core/recommenderPrediction.py:26-139; DESIGN.md 4 "RecommenderSim").
//
//   k_rec_profiles  : stage-C rows (pass-through segment, then mapped segment, both in user order) -> user-major profiles
//                     in stage-C row order; one row per thread, the destination follows from the two per-user offsets.
//   k_predict_rows  : (predict_rows.h: the pair body, shared with the scoring pass of the top-N recommendation)
//                     item_based_prediction, one WAVE per test pair, lanes = the neighbours of the test item.  Every lane
//                     looks its neighbour up in the test user's profile (the profile streams through the wave 64 rows at
//                     a time, one readlane per row), a prefix scan over the lanes gives the evidence offsets, the
//                     evidence (sim * (rating - neighbour average), |sim|, time) is staged in evidence order -- in LDS
//                     for up to PR_CAP entries, else in an arena slice sized by this count pass (second launch over the
//                     pairs that overflowed) --, the plain sums run left to right over it, the stable time order is a
//                     rank count per entry, the decayed sums run left to right over the sorted copy.  Same operations in
//                     the same order as RecommenderPrediction._predict_pair; there is no limit on the evidence of a pair.
//   k_mae_*         : count of predicted pairs, sum |real - plain|, sum |real - decayed| as double-double sums rounded once.
#include "common.h"
#include "predict_rows.h"      // k_predict_rows: the pair body the top-N scoring shares

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

// rec_model.h: the body of xmap_predict_rows.  The tables are asked for only when there is a pair to predict.
int predict_rows(void *stream, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const RecModel &M, double *out_plain,
                 double *out_decay, int32_t *status, int32_t *h_max_now) {
    XM_ARG(n_test >= 0 && M.n_users >= 0 && M.n_items >= 0 && M.keep >= 1 && M.keep <= 64 && M.n_w >= 1 && M.wtab && M.prof_ptr);
    XM_ARG(n_test == 0 || (test_user && test_item && M.nb_cnt && M.nb_col && M.nb_sim && M.item_avg && out_plain && out_decay && status));
    XM_ARG(M.n_users == 0 || (M.prof_item && M.prof_rating && M.prof_time));
    return predict_rows_run<false>((hipStream_t)stream, n_test, test_user, test_item, M, out_plain, out_decay, status, h_max_now);
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
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    return predict_rows(stream, n_test, test_user, test_item, M, out_plain, out_decay, status, h_max_now);
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
