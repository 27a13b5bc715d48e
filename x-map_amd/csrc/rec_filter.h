// rec_filter.h -- the eligibility rules of the filtered top-N and audience calls (xmap_rec_filter; DESIGN.md 4 "Eligibility"):
// what stage_e_topn.hip, stage_e_audience.hip and stage_e_group.hip share.  The candidate passes hold the candidate set of a
// query as an LDS bitmap of a window of the id space (IdBitmap, id_bitmap.h); the rules act on that bitmap, before anything is
// scored:
//   exclusions : the block strides the query's list and clears the ids that fall into the window (their words stay listed as
//                touched, like the words of held items) -- IdBitmap::exclude;
//   allow      : a touched word is ANDed with its word of the mask where it is emitted -- rf_eligible, the ONE statement of
//                "the eligible bits of word w" that the count pass and the fill pass both call: if they ever disagreed the fill
//                pass would write outside buffers of exactly the counted size.  Its one caller is IdBitmap::emit, of which
//                the two passes are two instantiations.
// The floor acts in the selection kernels, beside the status-2 drop.  This file holds rf_eligible and the argument checks.
#ifndef XMAP_REC_FILTER_H
#define XMAP_REC_FILTER_H
#include "common.h"

namespace xmap {

// bw = the candidate bits of word `word` of the id space (bit b = id 32 word + b, all of them < n: a candidate is an id of the
// tables); allow has a word for every id < n, so every touched word has one, and garbage bits at or beyond n meet zeros
template <bool FILT>
__device__ __forceinline__ unsigned int rf_eligible(unsigned int bw, const unsigned int *allow, long long word) {
    if constexpr (FILT) {
        if (allow) bw &= allow[word];
    }
    return bw;
}

// A CSR pointer table ptr[0 .. n]: bad[0] += positions k with ptr[k] < ptr[k - 1] (k = 0: ptr[0] != 0), bad[1] = ptr[n], bad[2] = the
// first such position (the caller sets it to RF_NO_POS).  Bounded by n alone: nothing is read through the table before it has passed.
constexpr unsigned long long RF_NO_POS = ~0ull;
static __global__ __launch_bounds__(256) void k_rf_check(long long n, const long long *ptr, unsigned long long *bad) {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k <= n; k += step) {
        const bool b = k == 0 ? ptr[0] != 0 : ptr[k] < ptr[k - 1];
        if (b) {                                // (bad input only: no need to spare the atomics; a minimum does not depend on their order)
            atomicAdd(&bad[0], 1ull);
            atomicMin(&bad[2], (unsigned long long)k);
        }
        if (k == n) bad[1] = (unsigned long long)ptr[k];
    }
}

// The device check of the pointer table `name` of n lists, for the call `who`: XMAP_ERR_ARG with the count of bad entries and the
// first bad position; *total = ptr[n].  Synchronises.
static int rf_check_ptr(hipStream_t st, int64_t n, const long long *ptr, const char *who, const char *name, long long *total) {
    unsigned long long *bad = nullptr, h_bad[3] = {0, 0, RF_NO_POS};
    XM_HIP(xm_malloc_async((void **)&bad, sizeof(h_bad), st));
    XM_HIP(hipMemcpyAsync(bad, h_bad, sizeof(h_bad), hipMemcpyHostToDevice, st));
    const long long entries = n + 1;
    const unsigned blocks = (unsigned)((entries + 255) / 256 < 1024 ? (entries + 255) / 256 : 1024);
    k_rf_check<<<dim3(blocks), dim3(256), 0, st>>>(n, ptr, bad);
    XM_LAUNCH_CHECK();
    XM_HIP(hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_bad[0]) {
        set_error("%s: %s has %llu bad entries, the first at %s[%llu] (%s[0] = 0, non-decreasing)", who, name, h_bad[0], name, h_bad[2], name);
        return XMAP_ERR_ARG;
    }
    *total = (long long)h_bad[1];
    return XMAP_OK;
}

// The argument checks of a filtered fine-grained call, before any candidate work.  *filt = the candidate pass needs its FILT
// instantiation (a mask or an exclusion list is given); *min_score = the floor (-inf without F).  Synchronises iff ex_ptr is given.
static int rf_prepare(hipStream_t st, int64_t n_query, const xmap_rec_filter *F, bool *filt, double *min_score) {
    *filt = false;
    *min_score = -__builtin_inf();
    if (!F) return XMAP_OK;
    if (F->min_score != F->min_score) {
        set_error("xmap_rec_filter: min_score is NaN");
        return XMAP_ERR_ARG;
    }
    *min_score = F->min_score;
    if (F->ex_ptr && n_query > 0) {
        long long n_ex = 0;
        const int rc = rf_check_ptr(st, n_query, (const long long *)F->ex_ptr, "xmap_rec_filter", "ex_ptr", &n_ex);
        if (rc) return rc;
        if (n_ex > 0 && !F->ex_id) {
            set_error("xmap_rec_filter: ex_ptr lists %lld ids, ex_id is NULL", n_ex);
            return XMAP_ERR_ARG;
        }
    }
    *filt = F->allow != nullptr || (F->ex_ptr != nullptr && n_query > 0);
    return XMAP_OK;
}

}  // namespace xmap
#endif
