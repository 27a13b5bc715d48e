// au_select.h -- the segmented top-N selection that the audience (stage_e_audience.hip) and the peers (stage_e_peers.hip) share:
// one block per segment, for segments of up to 2^32 - 1 candidates and N up to 1024.  The block keeps the best CAP >= n_top keys
// seen so far sorted in LDS; the segment streams through in tiles, a candidate that beats the current N-th key is staged behind
// them, and when the staging area cannot take another tile the whole array is sorted again by a bitonic network.  A key is
// (score as an ordered integer, position in the segment): keys are distinct, and the sorted prefix is the same whatever order the
// survivors were staged in.  The caller's kernel declares K / P in LDS, calls au_select_segment and writes its own outputs from
// the positions P[0 .. n_top).
#ifndef XMAP_AU_SELECT_H
#define XMAP_AU_SELECT_H
#include "common.h"

namespace xmap {

constexpr int AU_MAX_TOP = 1024;
constexpr int AU_SEL_THREADS = 256;             // threads of a selection block = candidates of a tile
constexpr unsigned long long AU_NO_KEY = ~0ull; // behind every key of a finite score
constexpr unsigned AU_NO_POS = 0xffffffffu;

// a finite score as an integer that ascends where the score DEscends; -0.0 and 0.0 get one key (scores compare as numbers)
__device__ __forceinline__ unsigned long long au_key(double s) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(s + 0.0);        // -0.0 + 0.0 = 0.0
    return (b >> 63) ? b : ~(b | (1ull << 63));         // negative: larger magnitude = later; positive: larger = earlier, before every negative
}

// ascending bitonic sort of (K, P)[0 .. 2 CAP), all threads of the block; keys (K, P) are distinct except among the blanks
template <int CAP>
__device__ __forceinline__ void au_sort(unsigned long long *K, unsigned *P) {
    constexpr int N = 2 * CAP;
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int t = threadIdx.x; t < N / 2; t += AU_SEL_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long ki = K[i], kl = K[l];
                const unsigned pi = P[i], pl = P[l];
                const bool gt = ki > kl || (ki == kl && pi > pl);
                if (gt == ((i & k) == 0)) { K[i] = kl; K[l] = ki; P[i] = pl; P[l] = pi; }
            }
            __syncthreads();
        }
    }
}

// The selection over the segment [a, b) of score / status, by every thread of a block of AU_SEL_THREADS.  K / P [2 CAP] and
// *s_staged are the block's LDS: [0, CAP) the best keys so far, sorted; [CAP, 2 CAP) the staged survivors of the tiles since the
// last sort.  On return P[0 .. n_top) holds the positions (relative to a) of the selected candidates in rank order, AU_NO_POS
// behind them, and every thread may read it.  A candidate with status != 0 is skipped and counted in `dropped` (this thread's
// share); FLOOR: one with score < min_score is skipped and counted in `floored`.
template <int CAP, bool FLOOR>
__device__ __forceinline__ void au_select_segment(long long a, long long b, int n_top, const double *score, const int *status,
                                                  double min_score, unsigned long long *K, unsigned *P, int *s_staged, int &dropped,
                                                  int &floored) {
    static_assert(CAP >= AU_SEL_THREADS && (CAP & (CAP - 1)) == 0, "the staging area takes a tile; bitonic sizes");
    const int tid = threadIdx.x;
    for (int k = tid; k < 2 * CAP; k += AU_SEL_THREADS) { K[k] = AU_NO_KEY; P[k] = AU_NO_POS; }
    if (tid == 0) *s_staged = 0;
    __syncthreads();
    long long p = a;
    while (p < b) {
        const int staged = *s_staged;
        __syncthreads();                        // every thread has read the count before a tile adds to it
        const int tiles = (CAP - staged) / AU_SEL_THREADS;
        if (tiles == 0) {                       // no room for another tile: sort, the best CAP stay, the staging area is blank again
            au_sort<CAP>(K, P);
            for (int k = CAP + tid; k < 2 * CAP; k += AU_SEL_THREADS) { K[k] = AU_NO_KEY; P[k] = AU_NO_POS; }
            if (tid == 0) *s_staged = 0;
            __syncthreads();
            continue;
        }
        // as many tiles as the staging area has room for, against one N-th key
        const unsigned long long wk = K[n_top - 1];
        const unsigned wp = P[n_top - 1];
        for (int t = 0; t < tiles && p < b; t++, p += AU_SEL_THREADS) {
            const long long x = p + tid;
            if (x >= b) continue;
            if (status[x] != 0) { dropped++; continue; }
            const double xs = score[x];
            if constexpr (FLOOR) {
                if (xs < min_score) { floored++; continue; }    // the floor: kept iff score >= min_score
            }
            const unsigned long long xk = au_key(xs);
            const unsigned xp = (unsigned)(x - a);
            if (xk < wk || (xk == wk && xp < wp)) {
                const int at = CAP + atomicAdd(s_staged, 1);
                K[at] = xk; P[at] = xp;
            }
        }
        __syncthreads();
    }
    if (*s_staged > 0) au_sort<CAP>(K, P);
    else __syncthreads();
}

}  // namespace xmap
#endif
