// two_pass.h -- the two host idioms of the passes that size their own output (the reverse lists, the holders and the three
// candidate passes of the recommender tail): the launch of a kernel with dynamic LDS, and "count -> exclusive scan -> allocate
// exactly -> fill".
#ifndef XMAP_TWO_PASS_H
#define XMAP_TWO_PASS_H
#include "common.h"

namespace xmap {

// k<<<blocks, threads, lds, st>>>(a...) for a kernel whose dynamic LDS exceeds the default limit
template <class... P, class... A>
static hipError_t launch_dyn_lds(void (*k)(P...), unsigned blocks, int threads, size_t lds, hipStream_t st, A... a) {
    const hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    k<<<dim3(blocks), dim3(threads), lds, st>>>(static_cast<P>(a)...);
    return hipGetLastError();
}

// A pass that runs twice over n rows.  pass(false, cnt, NULL) leaves the entries of every row in cnt[n]; the exclusive scan
// gives (*ptr)[n + 1] and *total (syncs); ready(*total) lets the caller allocate exactly; then, if there is an entry at all,
// pass(true, cnt, *ptr) fills.  pass returns the launch's hipError_t, ready an XMAP_ code.  ATOMIC: the pass counts with
// atomicAdd on cnt and the fill pass takes its positions from the same counters -- cnt is zeroed in front of either pass;
// otherwise the count pass writes every cnt[row] itself.  cnt and *ptr are temporaries of the caller's scope.
template <bool ATOMIC, class Pass, class Ready>
static int count_scan_fill(hipStream_t st, int64_t n, long long **ptr, int64_t *total, Pass pass, Ready ready) {
    const size_t n1 = (size_t)(n ? n : 1);
    int *cnt = nullptr;
    XM_HIP(xm_malloc_async((void **)&cnt, sizeof(int) * n1, st));
    XM_HIP(xm_malloc_async((void **)ptr, sizeof(long long) * (n1 + 1), st));
    if (ATOMIC) XM_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * n1, st));
    XM_HIP(pass(false, cnt, (const long long *)nullptr));
    int rc = xmap_exclusive_scan_i32_to_i64(st, cnt, (int64_t *)*ptr, n, total);
    if (rc) return rc;
    if ((rc = ready(*total))) return rc;
    if (*total > 0) {
        if (ATOMIC) XM_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * n1, st));
        XM_HIP(pass(true, cnt, (const long long *)*ptr));
    }
    return XMAP_OK;
}

}  // namespace xmap
#endif
