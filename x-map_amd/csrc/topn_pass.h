// topn_pass.h -- what the top-N recommendation (stage_e_topn.hip) and the group lists (stage_e_group.hip) share: the geometry of
// the windowed LDS bitmap of the item space, the reverse of the neighbour lists, the block scan of the emit step, and the
// candidate-and-scoring half of a top-N call (the "member pass" of a group call), which stage_e_topn.hip defines.
#ifndef XMAP_TOPN_PASS_H
#define XMAP_TOPN_PASS_H
#include "common.h"

namespace xmap {

constexpr int TN_WINDOW_LOG2 = 19;              // log2 of the items per bitmap pass; stage_e_topn.hip spells TN_WINDOW out and holds it to this
constexpr int TN_WORDS = (1 << TN_WINDOW_LOG2) / 32;    // 64 KB of LDS; two blocks per CU
constexpr int TN_SUMMARY = TN_WORDS / 32;       // second level: bit w of word s = bitmap word 32 s + w was touched
constexpr int TN_THREADS = 256;
constexpr int TN_PER = TN_SUMMARY / TN_THREADS; // summary words a thread emits (consecutive: thread order = item order)
constexpr int TN_MAX_TOP = 64;
constexpr int TN_MAX_BLOCKS = 2048;         // blocks of the candidate pass (grid-stride over the queries: the window is zeroed once per block)
constexpr size_t TN_LDS_BYTES = sizeof(unsigned int) * (TN_WORDS + TN_SUMMARY + TN_THREADS / 64);   // bitmap, summary, scan scratch

template <bool FILL>
__global__ __launch_bounds__(256) void k_tn_rev(int I, int keep, const int *nb_cnt, const int *nb_col, int *rcnt, const long long *rptr,
                                                int *ritem) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = t / keep;
    const int p = (int)(t - i * keep);
    if (i >= I) return;
    int cnt = nb_cnt[i];
    cnt = cnt < keep ? cnt : keep;
    if (p >= cnt) return;
    const int nb = nb_col[(size_t)i * keep + p];
    if (nb < 0 || nb >= I) return;              // ignored, as in the prediction
    const int at = atomicAdd(&rcnt[nb], 1);
    if constexpr (FILL) ritem[rptr[nb] + at] = (int)i;
}

__device__ __forceinline__ int tn_block_scan(int v, int *total, int *smem) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) smem[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < TN_THREADS / 64; k++) {
        const int s = smem[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// The candidate-and-scoring half of a top-N call over n_query query users: reverse neighbour lists -> candidates per query
// through the bitmap (count, scan, fill) -> predict_rows_run<true> over the candidate list.  What it leaves, in the stream's arena
// (valid until the caller's scope ends): per query q the segment [cand_ptr[q], cand_ptr[q + 1]) of (item ascending, each once;
// plain; decayed; status), only pairs with evidence.  n_pairs == 0: the four columns are NULL, cand_ptr is all zeros.
struct TnScored {
    long long *cand_ptr = nullptr;      // [n_query + 1]
    int *cand_item = nullptr;           // [n_pairs]
    double *plain = nullptr, *decay = nullptr;
    int *status = nullptr;
    int64_t n_pairs = 0;
    int32_t max_now = 0;                // the largest `now` met
};
// filt: the FILT instantiation of the candidate kernel with allow / ex_ptr / ex_id (device; each may be NULL); *removed (device,
// may be NULL unless filt) += the candidate pairs the mask or the lists removed.  n_query > 0.  Syncs.
int tn_score_candidates(hipStream_t st, int64_t n_query, const int32_t *query_user, int32_t flags, int64_t n_users, int32_t n_items,
                        int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim, const int64_t *prof_ptr,
                        const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time, const double *item_avg,
                        const double *wtab, int32_t n_w, bool filt, const unsigned int *allow, const long long *ex_ptr, const int *ex_id,
                        unsigned long long *removed, TnScored *out);

}  // namespace xmap
#endif
