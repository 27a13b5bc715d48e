// topn_pass.h -- what the top-N recommendation (stage_e_topn.hip) and the group lists (stage_e_group.hip) share: the geometry of
// their windowed LDS bitmap of the item space (id_bitmap.h holds the bitmap itself), the reverse of the neighbour lists, and the
// candidate-and-scoring half of a top-N call (the "member pass" of a group call), which stage_e_topn.hip defines.
#ifndef XMAP_TOPN_PASS_H
#define XMAP_TOPN_PASS_H
#include "common.h"
#include "id_bitmap.h"
#include "rec_model.h"

namespace xmap {

constexpr int TN_WINDOW_LOG2 = 19;              // log2 of the items per bitmap pass; stage_e_topn.hip spells TN_WINDOW out and holds it to this
constexpr int TN_THREADS = 256;
using TnBitmap = IdBitmap<TN_THREADS, TN_WINDOW_LOG2>;  // 64 KB of LDS, two blocks per CU; a thread emits two summary words
constexpr int TN_MAX_TOP = 64;
constexpr int TN_MAX_BLOCKS = 2048;         // blocks of the candidate pass (grid-stride over the queries: the window is zeroed once per block)

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
int tn_score_candidates(hipStream_t st, int64_t n_query, const int32_t *query_user, int32_t flags, const RecModel &M, bool filt,
                        const unsigned int *allow, const long long *ex_ptr, const int *ex_id, unsigned long long *removed, TnScored *out);

}  // namespace xmap
#endif
