// stage_c_foldin.hip -- fold-in: AlterEgo profiles of raw profiles that were not rows of the ratings upload (a user who
// arrived after training, a trained user whose profile changed), built with the replacement map a generate pass left resident.
// The model stays frozen: the profiles are a second set of user-major rows for xmap_predict_rows / xmap_topn_rows.
//
// The AlterEgo bodies are stage_c.hip's, reached through xmap_alterego_count / xmap_alterego_fill with an xmap_ratings view of
// the batch.  The fill pass writes pass-through rows at off_t[u] + rank and mapped rows at n_t_total + off_m[u] + rank: with
// n_t_total = 0, off_t[u] = prof_ptr[u] and off_m[u] = prof_ptr[u] + cnt_t[u] that IS the user-major layout xmap_rec_profiles
// makes of the resident rows (a user's pass-through rows, then its mapped rows), so no regrouping pass follows.
//
// New here: the check of the batch (it comes from outside; the resident kernels index flags[item] and map[item] unguarded,
// which is right for resident data only) and the offsets.
#include "common.h"

namespace xmap {

// One pass over ptr[0 .. n_new] and item[0 .. nnz), bounded by the arguments alone.  Position k <= n_new is ptr[k], position
// n_new + 1 + e is item[e].  bad[0] += bad positions, bad[1] = min(bad position).  A batch that passes has 0 = ptr[0] <= ptr[1]
// <= ... <= ptr[n_new] = nnz -- every profile lies inside item[0 .. nnz) -- and every item inside [0, n_items).
__global__ __launch_bounds__(256) void k_foldin_check(long long n_new, long long nnz, const long long *ptr, const int *item,
                                                      int n_items, unsigned long long *bad) {
    const long long total = n_new + 1 + nnz;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += step) {
        bool b;
        if (k <= n_new) {
            const long long p = ptr[k];
            b = k == 0 ? p != 0 : p < ptr[k - 1];
            if (k == n_new) b = b || p != nnz;
        } else {
            const int it = item[k - n_new - 1];
            b = it < 0 || it >= n_items;
        }
        if (b) {                        // (bad input only: no need to spare the atomics)
            atomicAdd(&bad[0], 1ull);
            atomicMin(&bad[1], (unsigned long long)k);
        }
    }
}

// out[u] = a[u] + b[u], u < n: the profile pointers from the scans of the two counts (b64), the offsets of the mapped rows
// from the profile pointers and the pass-through counts (b32)
__global__ __launch_bounds__(256) void k_foldin_offsets(long long n, const long long *a, const long long *b64, const int *b32,
                                                        long long *out) {
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n) out[u] = a[u] + (b64 ? b64[u] : (long long)b32[u]);
}

static xmap_ratings batch_view(int64_t n_new, int64_t nnz, const int64_t *ptr, const int32_t *item, const float *rating,
                               const int64_t *time, int32_t n_items, const uint8_t *flags) {
    xmap_ratings R;
    memset(&R, 0, sizeof(R));
    R.n_users = n_new; R.n_items = n_items; R.nnz = nnz;
    R.user_ptr = ptr; R.user_item = item; R.user_rating = rating; R.user_time = time; R.flags = flags;
    return R;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_foldin_count(void *stream, int64_t n_new, int64_t nnz, const int64_t *ptr, const int32_t *item, int32_t n_items,
                      const uint8_t *flags, const int32_t *map_src2tgt, int32_t *cnt_t, int32_t *cnt_m, int64_t *prof_ptr,
                      int64_t *h_counts) {
    XM_ARG(n_new >= 0 && nnz >= 0 && nnz < 2147483647ll && n_items >= 0);
    XM_ARG(ptr && prof_ptr && h_counts && (nnz == 0 || item) && (n_new == 0 || (cnt_t && cnt_m && flags && map_src2tgt)));
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    // ---- the check: nothing below it runs on a batch that fails, and no output is written
    unsigned long long *bad = nullptr, h_bad[2] = {0, 0};
    XM_HIP(xm_malloc_async((void **)&bad, sizeof(h_bad), st));
    XM_HIP(hipMemsetAsync(bad, 0, sizeof(unsigned long long), st));
    XM_HIP(hipMemsetAsync(bad + 1, 0xff, sizeof(unsigned long long), st));
    const long long total = n_new + 1 + nnz;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    k_foldin_check<<<dim3(blocks), dim3(256), 0, st>>>(n_new, nnz, (const long long *)ptr, item, n_items, bad);
    XM_LAUNCH_CHECK();
    XM_HIP(hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_bad[0]) {
        const long long k = (long long)h_bad[1];
        if (k <= n_new)
            set_error("fold-in batch: %llu bad entries, the first at ptr[%lld] (ptr[0] = 0, non-decreasing, ptr[n_new] = nnz)", h_bad[0], k);
        else
            set_error("fold-in batch: %llu bad entries, the first at item[%lld] (outside [0, %d))", h_bad[0], k - n_new - 1, n_items);
        return XMAP_ERR_ARG;
    }
    // ---- counts (stage_c.hip's bodies over a view of the batch; the count pass reads no rating and no time)
    long long *scan_t = nullptr, *scan_m = nullptr, *n_prof = nullptr;
    XM_HIP(xm_malloc_async((void **)&scan_t, sizeof(long long) * (size_t)(n_new + 1), st));
    XM_HIP(xm_malloc_async((void **)&scan_m, sizeof(long long) * (size_t)(n_new + 1), st));
    XM_HIP(xm_malloc_async((void **)&n_prof, sizeof(long long) * 64, st));
    XM_HIP(hipMemsetAsync(n_prof, 0, sizeof(long long) * 64, st));
    const xmap_ratings R = batch_view(n_new, nnz, ptr, item, nullptr, nullptr, n_items, flags);
    if (n_new > 0) {
        int rc = xmap_alterego_count(st, &R, map_src2tgt, cnt_t, cnt_m, (int64_t *)n_prof);
        if (rc) return rc;
    }
    int rc = xmap_exclusive_scan_i32_to_i64(st, cnt_t, (int64_t *)scan_t, n_new, nullptr);
    if (rc) return rc;
    rc = xmap_exclusive_scan_i32_to_i64(st, cnt_m, (int64_t *)scan_m, n_new, nullptr);
    if (rc) return rc;
    k_foldin_offsets<<<dim3((unsigned)((n_new + 1 + 255) / 256)), dim3(256), 0, st>>>(n_new + 1, scan_t, scan_m, nullptr,
                                                                                       (long long *)prof_ptr);
    XM_LAUNCH_CHECK();
    long long h_t = 0, h_m = 0, h_prof[64];
    XM_HIP(hipMemcpyAsync(&h_t, scan_t + n_new, sizeof(long long), hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(&h_m, scan_m + n_new, sizeof(long long), hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(h_prof, n_prof, sizeof(h_prof), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    h_counts[0] = h_t + h_m; h_counts[1] = h_t; h_counts[2] = 0;
    for (int k = 0; k < 64; k++) h_counts[2] += h_prof[k];
    XM_HIP(xm_free_async(n_prof, st)); XM_HIP(xm_free_async(scan_m, st)); XM_HIP(xm_free_async(scan_t, st));
    XM_HIP(xm_free_async(bad, st));
    return XMAP_OK;
}

int xmap_foldin_fill(void *stream, int64_t n_new, int64_t nnz, const int64_t *ptr, const int32_t *item, const float *rating,
                     const int64_t *time, int32_t n_items, const uint8_t *flags, const int32_t *map_src2tgt,
                     const int32_t *cnt_t, const int64_t *prof_ptr, int32_t *prof_item, double *prof_rating, int64_t *prof_time) {
    XM_ARG(n_new >= 0 && nnz >= 0 && nnz < 2147483647ll && n_items >= 0 && ptr && prof_ptr);
    if (n_new == 0 || nnz == 0) return XMAP_OK;                 // no entry, no row
    XM_ARG(item && rating && time && flags && map_src2tgt && cnt_t && prof_item && prof_rating && prof_time);
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    long long *off_m = nullptr;
    int *row_user = nullptr;            // the fill pass's user column: the profiles do not carry it (rows <= 2 nnz)
    XM_HIP(xm_malloc_async((void **)&off_m, sizeof(long long) * (size_t)n_new, st));
    XM_HIP(xm_malloc_async((void **)&row_user, sizeof(int) * 2 * (size_t)nnz, st));
    k_foldin_offsets<<<dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, st>>>(n_new, (const long long *)prof_ptr, nullptr, cnt_t,
                                                                                   off_m);
    XM_LAUNCH_CHECK();
    const xmap_ratings R = batch_view(n_new, nnz, ptr, item, rating, time, n_items, flags);
    int rc = xmap_alterego_fill(st, &R, map_src2tgt, prof_ptr, (const int64_t *)off_m, 0, row_user, prof_item, prof_rating, prof_time);
    if (rc) return rc;
    XM_HIP(xm_free_async(row_user, st)); XM_HIP(xm_free_async(off_m, st));
    return XMAP_OK;
}
}
