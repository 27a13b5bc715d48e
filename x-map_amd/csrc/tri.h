// tri.h -- stage A, second ("tri") formulation: every unordered item pair is computed ONCE, in the row of its lighter item,
// and mirrored into the CSR afterwards (baseliner_calculate_sim_pipeline, reference utils/assist.py:66-77;
// core/baselinerSim.py:176-216).  sim, mutu and n_ij are symmetric in the reference bit for bit, and both
// directions are emitted by produce_pairwise_items (:182-183), so computing the pair once and writing it twice is the same
// result.
//
// "Weight" of an item = (number of raters, index); the per-user private copy of each profile is sorted heaviest first, so the
// partners a rater contributes to item i are exactly the PREFIX of its sorted profile in front of i: no filtering in the
// inner loop, half the reads, and the heavier an item is the fewer partners its row has (the heaviest rows, which dominate
// the first formulation's cost, become tiny).
//
// One translation unit per concern: tri_layout.hip, tri_pairs.hip, tri_mirror.hip, tri_records.hip; here: what they share.
// Sums are exact (double-double, or plain fp64 in cosine mode for ratings whose sums are exact in any order -- the host's
// predicate, xmap/engine/exactness.py; otherwise cosine runs as XMAP_COSINE_EXACT), so neither the order of raters nor the
// chunking changes a bit of the result.
#pragma once
#include "common.h"
#include "tilesort.h"

namespace xmap {

// LDS table classes of the light rows (plan: plan_item; pair kernels: launch_tri)
constexpr int T_SLOTS = 1024;           // the largest table: bound of a plan's slot target
constexpr int HMAX = 1024;              // |H| <= HMAX: dense LDS table of the heavy kernel
constexpr int SMALL_BOUND = 96;          // rows with at most this many partners use the 128-slot table
constexpr int MID_BOUND = 384;           // ... at most this many: the 512-slot table

constexpr int N_CLASSES = 5;
constexpr int WIDE_MIN = 2048;           // light rows with at least this many raters: 16 waves on one 1024-slot table
// table class (1 = 128 slots, 3 = 256, 2 = 512, 0 = 1024, 4 = 1024 "wide") -> position in the class-major unit list
__host__ __device__ __forceinline__ int class_rank(int cls) {
    return cls == 4 ? 0 : (cls == 0 ? 1 : (cls == 2 ? 2 : (cls == 3 ? 3 : 4)));
}

// RecommenderSim (core/recommenderSim.py:90-133), shared by the LS variant of the pair kernels (tri_pairs.hip) and the item
// fold-in (stage_e_itemfold.hip): the significance weighting of a cosine, and a leave-one-out distance as an integer that
// orders like the number (bit pattern of a non-negative double, NaN above everything: np.max propagates NaN)
__device__ __forceinline__ double weighted(double cs, int n, int cap) {
    const int mn = n < cap ? n : cap;
    return 1.0 * cs * (double)mn / (double)cap;
}
__device__ __forceinline__ unsigned long long ls_key(double d) {
    return (d != d) ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(d);
}

struct RaterRec { int e0; int pos_ge; float rating; int user; };   // 16 B: one rater of an item
// fp64 ratings (the RecommenderSim variant, LS: AlterEgo ratings are np.float64 means, core/generator.py:123-138 ->
// core/recommenderSim.py:64-133): 16-byte profile entries and rater records of their own
struct UbWide { int item_ge; int pad; double rating; };      // 16 B: one entry of a sorted profile, fp64 rating
struct RaterRecWide { int e0; int pos_ge; double rating; };  // 16 B: one rater of an item, fp64 rating (no user: its average is 0)

// The half COO is cut into COO_SHARDS segments with a cursor each (a single cursor word would serialise the ~4e5
// appending waves: one word sustains only ~90 atomics/us); unused entries keep coo_i = -1.
constexpr int COO_SHARDS = 4096;

// ---- defined in tri_mirror.hip, used by the layout as well ----  counts[j] += entries of the half COO whose partner (second index) is j -- the mirrored entries row j will get; self pairs
// (skip_self) have none.  n_ranges ranges of range_cap slots, the first cur[r] of range r valid (cur == NULL: all of them).
// part: range_cap * n_ranges ints of scratch.  Three passes (k_cbs_hist, k_cbs_scatter, k_cb_count), no atomic per entry.
// (The layout counts the raters per item with it: the item column as one range.)
// fills (or NULL): fills of the caller's that are due before the first kernel; they leave in one launch with the bucket counters'
int mirror_counts(hipStream_t st, int n_items, long long range_cap, int n_ranges, const unsigned long long *cur, const int *coo_i,
                  const int *coo_j, bool skip_self, int *part, int *counts, FillList *fills = nullptr);
// tile sort, host side: geometry for K keys and M records (tilesort.h): tile measure 2^ts_log, key weight KW, T = NA * NB tiles
void ts_geometry(int K, long long M, int ch, ts::Geo &G);
// tables of one sort (arena temporaries of the calling entry point) + plan and chunk kernels
// (fills: as for mirror_counts)
int ts_prepare(hipStream_t st, ts::Geo &G, const long long *ptr, FillList *fills = nullptr);

}  // namespace xmap
