/*
 * xmap_hip.h -- C ABI of libxmap_hip.so, the MI355X (gfx950) engine behind X-MAP's hot path.
 *
 * The reference (LPD-EPFL-ML/X-MAP) is pure Python on Spark and has no FFI; the interface this
 * library replaces is the set of L2 "tool" methods that the three pipeline functions of
 * code/xmap/utils/assist.py call.  Each entry point below cites the
 * reference method(s) whose work it performs.  The host-side mirror of the Python API
 * (xmap.utils.assist / xmap.core.*) binds these with ctypes (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer argument is a DEVICE pointer into HBM unless its name starts with h_;
 *     buffers are allocated by the caller (the Python host uses torch tensors as containers);
 *   - `stream` is a hipStream_t passed as void* (0 = default stream);
 *   - items are int32 indices in lexicographic order of the reference's id strings, users are
 *     int32 indices in trainRDD order; string predicates arrive as small per-item arrays
 *     (prefix_cls = class of iid[:2], suffix_cls = class of iid[-2:], contains_mask bit c =
 *     class-c suffix string occurs in iid, flags bit0 = "S:" in iid, bit1 = "T:" in iid);
 *   - return value 0 = ok, negative = error (xmap_last_error() gives the thread-local text);
 *     functions that hand a count back to the host synchronise `stream` before returning.
 */
#ifndef XMAP_HIP_H
#define XMAP_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XMAP_OK 0
#define XMAP_ERR_HIP -1       /* a HIP runtime call or kernel launch failed */
#define XMAP_ERR_ARG -2       /* bad argument */
#define XMAP_ERR_OVERFLOW -3  /* an on-chip accumulator table overflowed; retry with a smaller slot target */
#define XMAP_ERR_CAPACITY -4  /* caller-provided output buffer too small; needed size is reported */

#define XMAP_COSINE 0         /* BaselinerSim.method == "cosine"        (core/baselinerSim.py:213) */
#define XMAP_ADJUST_COSINE 1  /* BaselinerSim.method == "adjust_cosine" (core/baselinerSim.py:215) */
/* "cosine" for ratings whose plain fp64 sums may round (fractional ratings): the pair entry points
 * (xmap_sim2_pairs, xmap_sim2_merge_partials, xmap_sim_count / xmap_sim_fill) sum the dot product as a double-double,
 * like XMAP_ADJUST_COSINE with a zero user average and the plain norms, so the result is the exact sum rounded once
 * whatever the order of the raters.  For ratings where the predicate holds both codes give the same bits. */
#define XMAP_COSINE_EXACT 2

#define XMAP_TOPC 10          /* candidates kept per start item: generator.py:85 keeps 10, :109 keeps 4 */

/* Ratings resident in HBM: CSR by user (trainRDD order, profile order kept) + CSC by item
 * (raters in ascending user index = the order reduceByKey concatenates co-raters in). */
typedef struct xmap_ratings {
    int64_t n_users;
    int32_t n_items;
    int64_t nnz;
    const int64_t *user_ptr;    /* [n_users+1] */
    const int32_t *user_item;   /* [nnz] */
    const float *user_rating;   /* [nnz] */
    const int64_t *user_time;   /* [nnz] unix seconds (stage C only) */
    const int64_t *item_ptr;    /* [n_items+1] */
    const int32_t *item_user;   /* [nnz] */
    const float *item_rating;   /* [nnz] */
    const int32_t *prefix_cls;  /* [n_items] */
    const int32_t *suffix_cls;  /* [n_items] */
    const uint32_t *contains_mask; /* [n_items] */
    const uint8_t *flags;       /* [n_items] */
} xmap_ratings;

const char *xmap_last_error(void);
int xmap_version(void);

/* The library keeps its own temporaries (per thread, device and stream; recycled when a call ends, trimmed to 256 MiB when
 * idle).  xmap_trim hands everything the calling thread's idle arenas still hold back to the driver (synchronises the
 * device).  xmap_debug_arena / xmap_debug_arena_call are test hooks: the arena's live temporaries and reserved bytes, and a
 * call that takes two temporaries and leaves through an error path when fail != 0. */
int xmap_trim(void);
int xmap_debug_arena(void *stream, int64_t *live, int64_t *reserved);
int xmap_debug_arena_call(void *stream, int64_t bytes, int fail);
/* Measurement hook: the library's stable LSD radix sort of n (key, value) pairs by the low `bits` bits of the key, in place, alone
 * -- the yardstick of the calls built around it (item fold-in, peers; profiles/tools/peers_timing.py).  1 <= bits <= 64, n < 2^31. */
int xmap_debug_sort_pairs(void *stream, uint64_t *keys, int32_t *vals, int64_t n, int32_t bits);
/* Test hook, host only (no stream, no device work): the chunk plan of the calls that take max_records (peers, user-kNN top-N, item
 * fold-in, related items, fused lists, shelves).  h_rec [n_query + 1] = the records in front of each query, non-decreasing.  A chunk
 * is a run of consecutive queries with at most max_records records (<= 0: the default 2^22; never more than 2^31 - 2), or one query.
 * cut [n_query + 1] receives the chunk borders cut[0 .. chunks], h_out [3] = {chunks, the most records of a chunk, the most queries
 * of one}.  A query with 2^31 - 1 records or more: XMAP_ERR_CAPACITY, the error names it. */
int xmap_debug_record_chunks(int64_t n_query, const int64_t *h_rec, int64_t max_records, int64_t *cut, int64_t *h_out);

/* exclusive prefix sum of n int64 values; out[n] receives the total; *h_total (may be NULL) too (syncs). */
int xmap_exclusive_scan_i64(void *stream, const int64_t *in, int64_t *out, int64_t n, int64_t *h_total);
int xmap_exclusive_scan_i32_to_i64(void *stream, const int32_t *in, int64_t *out, int64_t n, int64_t *h_total);
/* Two int32 arrays of one length scanned in the same launches: out_a = exclusive scan of in_a (a_plus_b != 0: of in_a + in_b,
 * added up in 64 bits), out_b = exclusive scan of in_b; out_a[n] / out_b[n] the totals, h_totals [2] (host, may be NULL) too
 * (syncs).  The scans take two launches while the array has at most xmap_scan_self_tiles() tiles of 2048 values (every block
 * of the second launch adds up the tile sums in front of it), three beyond that; no block ever waits for another. */
int xmap_exclusive_scan2_i32_to_i64(void *stream, const int32_t *in_a, const int32_t *in_b, int32_t a_plus_b, int64_t *out_a,
                                    int64_t *out_b, int64_t n, int64_t *h_totals);
int xmap_scan_self_tiles(void);

/* ---- stage A: baseliner_calculate_sim_pipeline (utils/assist.py:66-77) ------------------- */

/* CSC (item -> raters) of the ratings from the CSR by user: the device-side counterpart of the flatMap + combineByKey
 * shuffle of get_universal_item_info (core/baselinerSim.py:65-82).  Rater order within an item is unspecified (every
 * consumer sums exactly).  Fills item_ptr / item_user / item_rating, which xmap_ratings then points at. */
int xmap_build_csc(void *stream, int64_t n_users, int32_t n_items, int64_t nnz, const int64_t *user_ptr,
                   const int32_t *user_item, const float *user_rating, int32_t *cnt /*[I] scratch*/,
                   int64_t *item_ptr /*[I+1]*/, int32_t *item_user /*[nnz]*/, float *item_rating /*[nnz]*/);

/* BaselinerSim.get_universal_user_info (core/baselinerSim.py:17-38): avg[u], norm2[u] (fp64). */
int xmap_user_stats(void *stream, const xmap_ratings *R, double *u_avg, double *u_norm2);

/* BaselinerSim.get_universal_item_info (core/baselinerSim.py:40-82): info[i] = (avg, norm2, adjnorm2, n).
 * Also emits the stage-A private copies of the index arrays with bit 31 = (rating >= item avg), which is
 * all retrieve_path_info (core/baselinerSim.py:97-113) needs per co-rating:
 *   ua_item[e] = user_item[e] | ge<<31,  ia_user[p] = item_user[p] | ge<<31.
 * Only the complete-rows formulation (xmap_sim_count / xmap_sim_fill) reads them: pass both NULL to skip them. */
int xmap_item_stats(void *stream, const xmap_ratings *R, const double *u_avg, double *info /*[I][4]*/,
                    double *norms /*[2][I] dense copies of norm2 / adjnorm2, may be NULL*/,
                    int32_t *ua_item /*[nnz] or NULL*/, int32_t *ia_user /*[nnz] or NULL*/,
                    int32_t item_lo, int32_t item_hi /*items [lo, hi): a rank's share when items are sharded (0, n_items: all)*/);

#ifdef XMAP_CROSSCHECK   /* test formulation: exported by libxmap_hip_xcheck.so only (csrc/Makefile), never by the product library */
/* Work decomposition for the pair kernel: unit = (item i, hash partition q of its partner space),
 * Q[i] = ceil(min(W_i, I-1) / slot_target), W_i = sum over raters of (profile length - 1).
 * Writes Q[I], W[I], unit_ptr[I+1] (exclusive scan of Q); *h_n_units, *h_contrib (= sum W_i = P). Syncs. */
int xmap_sim_plan(void *stream, const xmap_ratings *R, int32_t slot_target, int32_t *Q, int64_t *W, int64_t *unit_ptr,
                  int64_t *h_n_units, int64_t *h_contrib);
int xmap_sim_units(void *stream, int32_t n_items, const int32_t *Q, const int64_t *unit_ptr,
                   int32_t *unit_item /*[n_units]*/, int32_t *unit_q /*[n_units]*/);

/* BaselinerSim.calculate_item2item_sim (core/baselinerSim.py:176-216) restricted to the units
 * [unit_lo, unit_hi) (item shards for multi-GPU): produce_pairwise_items + reduceByKey + cosine /
 * adjusted-cosine + significance weighting + mutuality + zero filter.
 * Pass 1 (count): unit_cnt[u] = kept pairs of unit u; h_counters[0] += kept, [1] += evaluated (D),
 *                 [2] = overflow flag.  Pass 2 (fill) writes the kept pairs of unit u at
 *                 unit_off[u] + [0, unit_cnt[u]) as (col, sim fp64, mutu, n_ij).
 * sim, mutu are symmetric bit for bit; frac_mutu = mutu / (n_i + n_j - n_ij) is derived by consumers. */
int xmap_sim_count(void *stream, const xmap_ratings *R, int method, int cap, const double *u_avg,
                   const double *info, const int32_t *ua_item, const int32_t *ia_user, const int32_t *Q,
                   const int32_t *unit_item, const int32_t *unit_q, int64_t unit_lo, int64_t unit_hi,
                   int32_t *unit_cnt /*[n_units]*/, int64_t *d_counters /*[4] device*/, int64_t *h_counters /*[4]*/);
int xmap_sim_fill(void *stream, const xmap_ratings *R, int method, int cap, const double *u_avg,
                  const double *info, const int32_t *ua_item, const int32_t *ia_user, const int32_t *Q,
                  const int32_t *unit_item, const int32_t *unit_q, int64_t unit_lo, int64_t unit_hi,
                  const int64_t *unit_off /*[n_units+1]*/, int32_t *col, double *sim, int32_t *mutu, int32_t *nij);

/* row_ptr[i] = unit_off[unit_ptr[i]], i in [0, I]: CSR row pointers of the kept pairs (units of one
 * item are contiguous, so its partitions concatenate into its row). */
int xmap_sim_row_ptr(void *stream, int32_t n_items, const int64_t *unit_ptr, const int64_t *unit_off /*[n_units+1]*/,
                     int64_t *row_ptr /*[I+1]*/);
#endif /* XMAP_CROSSCHECK */

/* ---- stage A, second formulation (csrc/tri.h; tri_layout.hip, tri_pairs.hip, tri_mirror.hip, tri_records.hip): each unordered pair is computed once, in the row of its lighter
 * item (weight = (rater count, index)), appended to a half COO and mirrored into the CSR.  Same results as
 * xmap_sim_count/fill (sums are exact, hence order-independent); about 40x fewer rater visits on skewed data.
 *   layout : per-user private profile copies sorted heaviest first (ub: item | flag, rating interleaved), one 16-byte
 *            rater record per CSC entry (profile offset, prefix length | flag, rating, user; no atomics, raters stay in
 *            ascending user order), the heavy set H = items with more than CH raters (|H| <= 1024; ctl[0] = CH >=
 *            ch_min, ctl[1] = |H|), pre[v] = #items with fewer than v raters.
 *   plan   : W+[i] = contributions of row i (sum of its raters' prefix lengths); Q[i] hash partitions for light rows,
 *            small[i] = LDS table class of the row (1: 128 slots, 3: 256, 2: 512, 0: 1024, 4: 1024 shared by 16 waves
 *            for light rows with >= 2048 raters), C[i] rater chunks for
 *            rows of H.  The light units are listed class-major (largest tables first): Qcat[rank][i] = Q[i] in the
 *            row's class rank, uq_ptr = exclusive scan over Qcat; h_counts = {light units, heavy units, first unit
 *            of class rank 0..4, light units} (cls_ptr of xmap_sim2_pairs = h_counts + 2).
 *   pairs  : phases = XMAP_PAIRS_* (below): RESET = reset counters/rowcnt, HEAVY = k_pair_heavy (chunk partials of the rows
 *            of H), LIGHT = k_pair_tri
 *            (light units [unit_lo, unit_hi), one launch per table class; 16 / 4 / 2 waves share a 1024 / 1024 / 512-slot table),
 *            HEAVY_MERGE = k_heavy_merge, MIRCOUNT = (last; mircnt == NULL only) the mirrored row counts rowcnt[j]++ from the
 *            COO's partner column, NO_MARKS = with RESET: do not mark the unused COO entries (a caller that reads the COO
 *            through the shard cursors only saves a 4 B x coo_cap fill); with HEAVY | LIGHT | HEAVY_MERGE in one call the
 *            heavy rows (partials, then merge) run on a side stream next to the class launches of the light rows;
 *            kept pairs (i lighter, j heavier) ->
 *            half COO: coo_cap entries cut into 4096 shards with a cursor each (d_shards[0][s]; unused entries keep
 *            coo_i = -1), rowcnt[i]++ / rowcnt[j]++; d_shards[1][s] sums to the unordered pairs evaluated;
 *            d_counters[2] = table overflow, [3] = COO shard overflow.
 *            XMAP_PAIRS_DEAL(m, r) in phases (bits 16-23 / 8-15; m > 1): only the rows of H whose item index % m == r are
 *            computed (item-sharded ranks deal the heavy rows round-robin; partials and merge of a row stay on one rank).
 *   scatter: after an exclusive scan of rowcnt -> row_ptr, both directions of every valid COO entry (n_coo = coo_cap
 *            entries are scanned) into the CSR. */
#define XMAP_PAIRS_HEAVY 1         /* chunk partials of the rows of H */
#define XMAP_PAIRS_LIGHT 2         /* the light rows */
#define XMAP_PAIRS_HEAVY_MERGE 4   /* merge of the chunk partials */
#define XMAP_PAIRS_RESET 8         /* clear the COO cursors, the counters and the row counts first */
#define XMAP_PAIRS_MIRCOUNT 16     /* the round-2 mirrored counts, added to rowcnt (ignored when mircnt is given) */
#define XMAP_PAIRS_RAW 32          /* user-sharded input: unfinished, unfiltered partial sums (see xmap_sim2_pack_partials) */
#define XMAP_PAIRS_SHARD_SUMS 64   /* d_counters[4] / [5] = kept / evaluated unordered pairs */
#define XMAP_PAIRS_NO_MARKS 128    /* with RESET: leave the unused COO entries unmarked */
#define XMAP_PAIRS_DEAL(m, r) ((((m) & 0xff) << 16) | (((r) & 0xff) << 8))
#define XMAP_PAIRS_DEAL_MOD(phases) (((phases) >> 16) & 0xff)
#define XMAP_PAIRS_DEAL_REM(phases) (((phases) >> 8) & 0xff)
int xmap_sim2_layout(void *stream, const xmap_ratings *R, const double *info, int32_t ch_min, int32_t *hist /*[U+2]*/,
                     int64_t *pre /*[U+3]*/, int32_t *ctl /*[4]*/, int32_t *hid /*[I]*/, int32_t *hlist /*[1024]*/,
                     uint64_t *ub_key /*[nnz] scratch*/, void *ub /*[nnz] x 8 B: item|flag, rating*/,
                     void *rc /*[nnz] x 16 B rater records in CSC order*/,
                     uint64_t *Wp /*[I] out: contributions per row (sum of its raters' prefix lengths)*/,
                     int32_t dups /*1: a profile may hold an item more than once (AlterEgo rows)*/, int32_t *h_ctl /*[2]*/);
int xmap_sim2_plan(void *stream, const xmap_ratings *R, int32_t slot_target, const void *rc, const int64_t *pre,
                   const int32_t *hid, const int32_t *ctl, int32_t *Q, int32_t *C, uint8_t *small /*[I]*/,
                   uint64_t *Wp /*[I] as left by xmap_sim2_layout*/, int32_t *Qcat /*[5 I]*/, int64_t *uq_ptr /*[5 I + 1]*/,
                   int64_t *uc_ptr /*[I + 1]*/, int32_t dups, int64_t *h_counts /*[8], host*/);
/* light unit u: uq_item[u] and the 16-byte record uq_q[4 u ..] = (hash partition, first rater, end of raters, partitions of
 * the row): what a pair kernel needs to start, in one round trip */
int xmap_sim2_units(void *stream, int32_t n_items, const int64_t *item_ptr, const int32_t *Qcat, const int64_t *uq_ptr,
                    int32_t *uq_item, int32_t *uq_q /*[4 light units]*/, const int32_t *C, const int64_t *uc_ptr, int32_t *uc_item,
                    int32_t *uc_c);
int xmap_sim2_pairs(void *stream, const xmap_ratings *R, int method, int cap, const double *u_avg, const double *norms,
                    const void *rc, const void *ub, const int32_t *Q,
                    const uint8_t *small, const int32_t *uq_item, const int32_t *uq_q, const int64_t *cls_ptr /*[6], host*/,
                    int64_t unit_lo, int64_t unit_hi, const int32_t *hid,
                    const int32_t *hlist, const int32_t *ctl, const int32_t *C, const int64_t *uc_ptr,
                    const int32_t *uc_item, const int32_t *uc_c, int32_t n_heavy_units, int32_t n_heavy, int phases,
                    double *hp_hi, double *hp_lo, int32_t *hp_cnt, int32_t *hp_mut, int64_t coo_cap, int32_t *coo_i,
                    int32_t *coo_j, double *coo_sim, int32_t *coo_mutu, int32_t *coo_nij,
                    double *coo_ls /*NULL, or the RecommenderSim variant (below)*/, int32_t *rowcnt,
                    int64_t *d_shards /*[2][4096]*/,
                    int64_t *d_counters /*[4]; [6] with phases bit 64: [4] / [5] = kept / evaluated unordered pairs, the sums
                                          of d_shards[0] / [1]*/,
                    int32_t *mircnt /*[I] or NULL.  NULL: rowcnt[i]++ / rowcnt[j]++ as described above.  Else rowcnt counts
                                      the pairs a row computed itself only and mircnt is cleared: the caller gets the mirrored
                                      counts from xmap_sim3_mircount (the pair kernels issue no atomic per kept pair)*/);
int xmap_sim2_scatter(void *stream, int32_t n_items, int64_t n_coo, const int32_t *coo_i, const int32_t *coo_j,
                      const double *coo_sim, const int32_t *coo_mutu, const int32_t *coo_nij, const double *coo_ls /*or NULL*/,
                      const int64_t *row_ptr, int32_t *fill /*[I] scratch*/, const int32_t *hid, const int32_t *hlist,
                      int32_t *col, double *sim, int32_t *mutu, int32_t *nij, double *ls /*or NULL*/);
/* ---- round 3: one transposition per pass -----------------------------------------------------------------------------
 * xmap_sim3_layout replaces xmap_build_csc + xmap_user_stats + xmap_item_stats + xmap_sim2_layout for the "tri" formulation:
 *   k_count3          raters per item in one pass over the CSR (LDS-cached atomics) -> item_ptr (exclusive scan)
 *   k_user_stats      u_avg / u_norm (get_universal_user_info, core/baselinerSim.py:17-38)        [float ratings only]
 *   k_hist .. k_mark_heavy   as xmap_sim2_layout
 *   k_sort_profiles3  profiles sorted heaviest first: ub (8 B per entry; 16 B with rating64) and one sort record per entry
 *                     {item, position, rating, user} (16 B; 24 B with rating64)
 *   tile sort         (csrc/tilesort.h) sort records -> rater records rc in item order (any order inside an item), W+ summed
 *   k_item_stats3 ..  get_universal_item_info (:40-82) from the rater records -> info, norms; items with more than 512
 *                     raters in chunks of 2048 on a wave each, merged in chunk order
 *   flags             `rating >= item average` (retrieve_path_info, :97-113) into the rater records and the profile copy
 * The CSC arrays (R->item_user / item_rating) are neither read nor written; R->item_ptr (= item_ptr) is written.
 * rating64 != NULL: the ratings are fp64 (RecommenderSim over AlterEgo means, core/recommenderSim.py:64-133; R->user_rating is
 * ignored), the user averages are zero by construction (u_avg must be zero-filled, u_norm may be NULL), there is no
 * mutuality, and ub / rc use the 16-byte wide forms xmap_sim2_pairs reads when coo_ls != NULL without XMAP_PAIRS_RAW.
 * phases (XMAP_LAYOUT_*): RECORDS = everything up to the rater records and W+; STATS = item statistics of the items
 * [stats_lo, stats_hi) (and the flags of THEIR rater records); UB_FLAGS = flags of the profile copy, RC_FLAGS = flags of all
 * rater records -- both from the complete info.
 * One GPU: RECORDS | STATS | UB_FLAGS with all items.  Item-sharded ranks: RECORDS | STATS with the rank's share, an all-gather
 * of info / norms (the all-gather of per-item norms), then UB_FLAGS | RC_FLAGS.
 * h_ctl (host, [2], may be NULL) = {CH, |H|}; synchronises if given. */
#define XMAP_LAYOUT_RECORDS 1
#define XMAP_LAYOUT_STATS 2
#define XMAP_LAYOUT_UB_FLAGS 4
#define XMAP_LAYOUT_RC_FLAGS 8
#define XMAP_LAYOUT_ALL 15
int xmap_sim3_layout(void *stream, const xmap_ratings *R, int64_t *item_ptr /*[I+1] = R->item_ptr*/,
                     const double *rating64 /*[nnz] or NULL*/, int32_t ch_min, int32_t phases, int32_t stats_lo, int32_t stats_hi,
                     int32_t *cnt /*[I] scratch*/,
                     double *u_avg /*[U]*/, double *u_norm /*[U] or NULL with rating64*/, int32_t *hist /*[U+2]*/,
                     int64_t *pre /*[U+3]*/, int32_t *ctl /*[4]*/, int32_t *hid /*[I]*/, int32_t *hlist /*[1024]*/,
                     uint64_t *ub_key /*[nnz] scratch*/, void *ub /*[nnz] x 8 B (16 B)*/, void *srec /*[nnz] x 16 B (24 B) scratch*/,
                     void *bufA /*as srec, scratch*/, void *bufB /*as srec, scratch*/, void *rc /*[nnz] x 16 B*/,
                     uint64_t *Wp /*[I]*/, double *info /*[I][4]*/, double *norms /*[2][I]*/, int32_t *h_ctl /*[2], host*/);
/* xmap_sim2_plan + xmap_sim2_units with one synchronisation instead of four: the caller sizes the unit arrays from bounds it
 * knows without asking the device (light units <= contributions / slot_target + n_items with contributions = sum over the
 * users of d (d - 1) / 2; heavy units <= nnz / ch_min + 1024).  h_out [10], host = {light units, heavy units, first unit of
 * table class rank 0..4, light units, CH, |H|} (h_out + 2 is the cls_ptr of xmap_sim2_pairs). */
int xmap_sim3_plan(void *stream, const xmap_ratings *R, int32_t slot_target, const int64_t *pre, const int32_t *hid,
                   const int32_t *ctl, int32_t *Q, int32_t *C, uint8_t *small, uint64_t *Wp, int32_t *Qcat /*[5 I]*/,
                   int64_t *uq_ptr /*[5 I + 1]*/, int64_t *uc_ptr /*[I + 1]*/, int32_t dups, int32_t *uq_item, int32_t *uq_q /*[4 cap_light]*/,
                   int32_t *uc_item, int32_t *uc_c, int64_t cap_light, int64_t cap_heavy, int64_t *h_out /*[10], host*/);
/* The same in two halves, for a caller that has work for the device while the host waits: xmap_sim3_plan_begin queues the plan
 * kernels, the copy of the ten counts into a pinned block (one per thread and device, reused) and an event behind it;
 * xmap_sim3_plan_wait waits for that event only -- not for what was queued on the stream since -- and returns the counts
 * and the checks of xmap_sim3_plan.  One begin, then its wait, per thread and device: a begin whose wait never came is dropped
 * by the next begin (after its copy has landed); a wait without a begin is refused. */
int xmap_sim3_plan_begin(void *stream, const xmap_ratings *R, int32_t slot_target, const int64_t *pre, const int32_t *hid,
                         const int32_t *ctl, int32_t *Q, int32_t *C, uint8_t *small, uint64_t *Wp, int32_t *Qcat /*[5 I]*/,
                         int64_t *uq_ptr /*[5 I + 1]*/, int64_t *uc_ptr /*[I + 1]*/, int32_t dups, int32_t *uq_item, int32_t *uq_q /*[4 cap_light]*/,
                         int32_t *uc_item, int32_t *uc_c, int64_t cap_light, int64_t cap_heavy);
int xmap_sim3_plan_wait(int64_t cap_light, int64_t cap_heavy, int64_t *h_out /*[10], host*/);
/* The read of xmap_sim2_pairs' d_counters [6] (flags, kept / evaluated pairs) the same way: begin after the pair kernels, then
 * whatever does not need the counts (xmap_sim3_mircount), then wait. */
int xmap_sim3_counters_begin(void *stream, const int64_t *d_counters /*[6]*/);
int xmap_sim3_counters_wait(int64_t *h_out /*[6], host*/);
/* mir[j] = entries of a half COO whose second index is j, i.e. the mirrored entries row j gets (skip_self: an entry pairing a
 * row with itself has none).  Three coalesced passes over the partner column (bucket histogram, scatter, LDS windows) instead
 * of the device atomic per kept pair the pair kernels used to issue: those 2.65e7 atomics per pass were what the class
 * launches waited for.  scratch: n_pairs ints.  d_shards as in xmap_sim3_mirror. */
int xmap_sim3_mircount(void *stream, int32_t n_items, int64_t coo_cap, const int32_t *coo_i, const int32_t *coo_j,
                       const int64_t *d_shards /*or NULL*/, int64_t n_pairs, int32_t skip_self, void *scratch, int32_t *mir /*[I] out*/);
/* The mirror of round 3.  own[i] = pairs row i computed (xmap_sim2_pairs' rowcnt), mir[j] = pairs computed in lighter rows
 * (xmap_sim3_mircount).  Row i of the CSR = [own | mirrored]: row_ptr = exclusive scan of own + mir; the own halves are written
 * in runs straight from the COO, the mirrored halves go through the tile sort keyed by the heavier item (positions mptr =
 * exclusive scan of mir).  n_pairs = valid COO entries.  coo_aux / aux (both or neither; RecommenderSim): a sixth column --
 * the pair's local sensitivity -- travels along (32-byte records), and a row may pair with itself: such an entry is an own
 * entry only (xmap_sim2_pairs counted it that way), so the CSR has row_ptr[I] <= 2 n_pairs entries. */
int xmap_sim3_mirror(void *stream, int32_t n_items, int64_t coo_cap, const int32_t *coo_i, const int32_t *coo_j,
                     const double *coo_sim, const int32_t *coo_mutu, const int32_t *coo_nij,
                     const int64_t *d_shards /*[4096] fill of the COO's shards as left by xmap_sim2_pairs (coo_cap / 4096
                                               slots each), or NULL: the COO is one range of n_pairs records*/,
                     int64_t n_pairs, const int32_t *own /*[I]*/, const int32_t *mir /*[I]*/, int32_t *tot /*[I] scratch*/,
                     int64_t *row_ptr /*[I+1] out*/, int64_t *mptr /*[I+1] scratch*/, int32_t *fill /*[I] scratch*/,
                     void *bufA /*[n_pairs] x 24 B (32 B with aux) scratch*/, void *bufB /*as bufA*/, int32_t *col,
                     double *sim, int32_t *mutu, int32_t *nij, const double *coo_aux /*or NULL*/, double *aux /*or NULL*/,
                     int32_t row_lo, int32_t row_hi /*the rows to build: 0, n_items = all.  An item-sharded rank builds its share of
                     the rows from the complete COO: own / mir must be zero outside [row_lo, row_hi), entries of other rows are skipped*/);

/* User-sharded input (BASELINE configs[2]: "reduce-scatter of cross-shard partial similarities"): a rank
 * holds the complete profiles of a share of the USERS.  Per item its share of get_universal_item_info's sums
 * (core/baselinerSim.py:56-82) is xmap_item_partials -> [I][7] = (sum r, sum r^2, sum (r - avg_u)^2, each as an exact (value,
 * error) pair, raters); the shares of all ranks, gathered as [n_parts][I][7], are added up exactly and finished by
 * xmap_item_merge.  xmap_sim2_pairs with XMAP_PAIRS_RAW ("raw": no
 * heavy set, coo_ls != NULL) then emits, for every pair two of the rank's users co-rated, the partial sums of
 * calculate_cosine_sim / calculate_adjusted_cosine_sim (:115-174) and retrieve_path_info (:97-113) unfinished and unfiltered:
 * coo_sim / coo_ls = the dot product as an exact (value, error) pair, coo_nij, coo_mutu.  xmap_sim2_pack_partials turns
 * them into 32-byte records (key = lower index << 32 | higher index, value, error, n_ij | mutu << 32; *h_count of them),
 * xmap_sim2_sort_partials groups them by the rank that owns the lower item (stable radix sort), and -- after the exchange,
 * sorted once more by pair key (stable: the shares of a pair stay in rank order), so that every rank holds ALL records of the
 * pairs it owns -- xmap_sim2_merge_partials adds
 * the shares of a pair up (the dot product exactly), applies cosine, significance weighting and the zero filter
 * (:84-95,:198,:207) with the merged item norms and appends the kept pairs (i < j) to a half COO + row counts, which
 * xmap_sim2_scatter mirrors as usual.  h_counts = {kept, evaluated} unordered pairs. */
/* The exchange of a sharded step's kept pairs before stage B (the reference broadcasts its knn tables, utils/assist.py:88-101):
 * valid entries of a half COO (coo_i >= 0) -> 24-byte records (i | j << 32, sim bits, mutu | n_ij << 32), *h_count of them,
 * in any order; and back into COO columns after the all-gather. */
int xmap_sim2_pack_pairs(void *stream, int64_t n_coo, const int32_t *coo_i, const int32_t *coo_j, const double *coo_sim,
                         const int32_t *coo_mutu, const int32_t *coo_nij, int64_t *rec /*[n_coo][3]*/, int64_t *h_count);
int xmap_sim2_unpack_pairs(void *stream, int64_t n, const int64_t *rec /*[n][3]*/, int32_t *coo_i, int32_t *coo_j, double *coo_sim,
                           int32_t *coo_mutu, int32_t *coo_nij);
int xmap_item_partials(void *stream, const xmap_ratings *R, const double *u_avg, double *partial /*[I][7]*/);
int xmap_item_merge(void *stream, int32_t n_items, int32_t n_parts, const double *parts /*[n_parts][I][7]*/, double *info /*[I][4]*/,
                    double *norms /*[2][I]*/);
int xmap_sim2_pack_partials(void *stream, int64_t n_coo, const int32_t *coo_i, const int32_t *coo_j, const double *coo_hi,
                            const double *coo_lo, const int32_t *coo_mutu, const int32_t *coo_nij, int64_t *rec /*[n_coo][4]*/,
                            int64_t *h_count);
int xmap_sim2_sort_partials(void *stream, int64_t n, const int64_t *rec /*[n][4]*/, int64_t *rec_sorted /*[n][4]*/, int32_t n_items,
                            int32_t n_owners /*> 0: group by the rank owning the lower item (before the exchange); 0: by pair key*/);
int xmap_sim2_merge_partials(void *stream, int method, int cap, int32_t n_items, int64_t n, const int64_t *rec_sorted,
                             const double *norms /*[2][I]*/, int32_t *coo_i, int32_t *coo_j, double *coo_sim, int32_t *coo_mutu,
                             int32_t *coo_nij, int32_t *rowcnt /*[I]*/, int64_t *h_counts /*[2]*/);

/* RecommenderSim.calculate_sim (core/recommenderSim.py:65-133,188-195; both method names take the cosine branch, :190)
 * is the same pair machinery over the AlterEgo rows: call xmap_item_stats with u_avg = 0 (adjnorm is then the exact
 * norm), xmap_sim2_layout with dups = 1 and ch_min > n_users (no heavy set), xmap_sim2_plan with dups = 1, and
 * xmap_sim2_pairs with method XMAP_ADJUST_COSINE (exact double-double sums), u_avg = 0 and coo_ls != NULL: nothing is
 * filtered, an item held twice by a user pairs with itself (one entry, both orders counted), and coo_ls receives the
 * leave-one-out local sensitivity of every pair (second walk over the raters with the final inner product; NaN
 * propagates like np.max).  xmap_sim2_scatter then mirrors (col, sim, n_ij, ls); mutu is unused (0). */

/* ---- stage B: extender_pipeline (utils/assist.py:80-133) ---------------------------------- */

/* Similarity matrix of stage A, CSR by first item (get_item_sim, core/baselinerSim.py:218-233). */
typedef struct xmap_sim {
    int32_t n_items;
    const int64_t *row_ptr; /* [I+1] */
    const int32_t *col;
    const double *sim;
    const int32_t *mutu;
    const int32_t *nij;
    const double *info;     /* [I][4] item info of stage A (n_i is info[i][3]) */
    const double *frac;     /* optional [nnz] frac_mutu per pair; NULL = derive mutu / (n_i + n_j - n_ij) */
} xmap_sim;

/* build_sim_DF + "SELECT DISTINCT id1 ... WHERE label = 1" (core/baselinerSim.py:235-244,
 * utils/assist.py:82-87): bb[i] = 1 iff item i has a kept pair whose 2-char prefixes differ. */
int xmap_bridge_flags(void *stream, const xmap_sim *S, const int32_t *prefix_cls, uint8_t *bb);

/* ExtendSim.find_knn_items (core/extender.py:16-44) + extract_siminfo (utils/assist.py:105-133):
 * per item the two top-k lists by (|sim| desc, col asc): list 0 = BB_BB | NB_BB, list 1 = BB_NB | NB_NN.
 * cls[i] = 0 none, 1 bridge record, 2 non-bridge record. kval = (sim, mutu, frac_mutu) fp64.  Every entry of the rows
 * [row_lo, row_hi) is written (the unused tail of a list with zeros): the tables may come uninitialised. */
int xmap_knn_classify(void *stream, const xmap_sim *S, int top_k, const uint8_t *bb, const int32_t *suffix_cls,
                      const uint32_t *contains_mask, uint8_t *cls, int32_t *kcnt /*[I][2]*/,
                      int32_t *kcol /*[I][2][k]*/, double *kval /*[I][2][k][3]*/,
                      int32_t row_lo, int32_t row_hi /*rows [lo, hi): a rank's share (0, n_items: all)*/);

/* Reverse adjacencies of the knn tables, built deterministically in row order:
 *   mode 0 ATTACH: attach(b) = [x : x non-bridge record, b in NB_BB(x)]   (core/extender.py:48-59,171-173)
 *   mode 1 SRC   : src(t)    = [s : s bridge, "S:" in s, attach(s) != [], t in keys(knn_BB[s])], "T:" in t
 *                               (core/extender.py:61-70,174,176); rflag bit0 = (t,s) also joins TGT (:72-81,175-178)
 *   mode 2 RNN   : rnn(y)    = [x : x non-bridge record, y in NB_NN(x)]    (core/extender.py:142-169 longest_path)
 * count pass: rcnt[I]; fill pass: ridx / rval (sim, mutu, frac) / rflag at rptr[a] + ... */
/* thr[i][l] = {|sim| (double), column (int32), length (int32)} of the LAST entry of list l of item i (16 B each): the
 * membership tests of xmap_reverse_* then cost one gather into a 32 B x n_items table instead of three into the lists. */
int xmap_knn_thresholds(void *stream, int32_t n_items, int top_k, const int32_t *kcnt, const int32_t *kcol, const double *kval,
                        void *thr /*[n_items][2] x 16 B*/);
int xmap_reverse_count(void *stream, const xmap_sim *S, int mode, int top_k, const uint8_t *bb, const uint8_t *cls,
                       const int32_t *kcnt, const int32_t *kcol, const double *kval, const int32_t *suffix_cls,
                       const uint32_t *contains_mask, const uint8_t *flags, const int64_t *attach_ptr,
                       const void *thr /*xmap_knn_thresholds or NULL*/,
                       int32_t *long_rows /*[I+1] scratch or NULL: written here, rows of > 4096 entries get 16 waves*/,
                       uint8_t *eflag /*one byte per entry of the rows [row_lo, row_hi) or NULL: written here (bit 0 = listed,
                       bit 1 = joint); xmap_reverse_fill given the same buffer reads it instead of testing every entry again*/,
                       int32_t *rcnt /*[I]*/, int32_t row_lo, int32_t row_hi /*the rows (= targets of the lists) of this
                       call: the list of a row is built from that row alone, so a rank's share of the rows gives a
                       contiguous share of the lists; [0, I) = all*/);
/* attach (mode 0) and rnn (mode 2) lists counted in ONE pass over the rows -- both ask the same non-bridge neighbours b of an
 * entry, about their two lists: one class gather and one read of the matrix instead of two.  eflag (required) then serves
 * xmap_reverse_fill of mode 0 and of mode 2 (bit 0 / bit 2). */
int xmap_reverse_count_att_rnn(void *stream, const xmap_sim *S, int top_k, const uint8_t *bb, const uint8_t *cls,
                               const int32_t *kcnt, const int32_t *kcol, const double *kval, const int32_t *suffix_cls,
                               const uint32_t *contains_mask, const uint8_t *flags, const void *thr, int32_t *long_rows,
                               uint8_t *eflag, int32_t *rcnt_att /*[I]*/, int32_t *rcnt_rnn /*[I]*/, int32_t row_lo, int32_t row_hi);
int xmap_reverse_fill(void *stream, const xmap_sim *S, int mode, int top_k, const uint8_t *bb, const uint8_t *cls,
                      const int32_t *kcnt, const int32_t *kcol, const double *kval, const int32_t *suffix_cls,
                      const uint32_t *contains_mask, const uint8_t *flags, const int64_t *attach_ptr,
                      const void *thr /*xmap_knn_thresholds or NULL*/,
                      int32_t *long_rows /*as left by xmap_reverse_count, or NULL*/,
                      uint8_t *eflag /*as left by xmap_reverse_count of the same mode and rows, or NULL*/, const int64_t *rptr /*[I+1]*/,
                      int32_t *ridx, double *rval /*[n][3]*/, uint8_t *rflag, int32_t row_lo, int32_t row_hi);

/* The stage-B tables of one pass, as every entry point below that reads them takes them (device pointers).  Members a call
 * does not read may be NULL / 0; each entry point says which it reads.
 *   cls .. flags : the classified top-k lists (xmap_knn_classify) and the item flags of xmap_ratings;
 *   att_* / src_* / rnn_* : the reverse adjacencies (xmap_reverse_*: ptr [I+1], idx, val [n][3]; src_flag bit 0 = joint);
 *   n_nb, nb_id, nb_list : the non-bridge records (xmap_nb_index); midX, dir, dir_ptr: their middle lists (xmap_mid_rows_*);
 *   n_ends, urank, uitem : the end universe (xmap_end_universe), read by xmap_extend_cols only.
 * xmap_path_units: the work units (xmap_path_plan); xmap_path_rows: the accumulator rows; xmap_path_out: the results. */
typedef struct xmap_ext_tables {
    int32_t n_items, top_k;
    const uint8_t *cls; const int32_t *kcnt; const int32_t *kcol; const double *kval; const uint8_t *flags;
    const int64_t *att_ptr; const int32_t *att_idx; const double *att_val;
    const int64_t *src_ptr; const int32_t *src_idx; const double *src_val; const uint8_t *src_flag;
    const int64_t *rnn_ptr; const int32_t *rnn_idx; const double *rnn_val;
    int32_t n_nb; const int32_t *nb_id; const int32_t *nb_list; const void *midX; const void *dir; const int64_t *dir_ptr;
    int32_t n_ends; const int32_t *urank; const int32_t *uitem;
} xmap_ext_tables;
typedef struct xmap_path_units {
    int32_t n_units; const int32_t *unit_start; const int32_t *unit_c; const int32_t *unit_G; const int32_t *unit_row;
    int32_t *unit_nt; int32_t n_heavy; const int32_t *heavy_unit0;
} xmap_path_units;
typedef struct xmap_path_rows { int32_t n_slots; double *acc; int32_t *touched; double *hacc; int32_t *htouched; } xmap_path_rows;
typedef struct xmap_path_out {
    int32_t *n_cand; int32_t *top_end; double *top_val; int64_t xs_cap; int64_t *xs_off; int32_t *xs_end; double *xs_val;
} xmap_path_out;

/* Scheduling weights of the path enumeration: paths[start] = number of paths that start at `start`
 * (exact; tails(s) summed over src(t), heads over NB_BB / rnn).  tmp: 4*n_items int64 of scratch.
 * Reads n_items, top_k, cls, kcnt, kcol, flags, att_ptr, att_idx, src_ptr, src_idx, src_flag, rnn_ptr, rnn_idx (no value
 * column, no middle-list member). */
int xmap_path_weights(void *stream, const xmap_ext_tables *T, int64_t *tmp /*[4][I]*/, int64_t *paths /*[I]*/);

/* ExtendSim.sim_extend + get_final_extension (core/extender.py:46-217), start-sharded and streamed:
 * every path of final_nonjoint_extend / final_joint_extend is enumerated in registers with its
 * s_p, c_p (calculate_path_confidence, :83-89) and accumulated into (sum s_p c_p, sum c_p) per
 * (start, end); xsim = ratio (:198-201).  The sums are kept as double-double (error-free two-sum), so
 * they do not depend on the enumeration order.
 * Reads of T: n_items, top_k, cls .. flags, att_*, src_*, rnn_* (rows are indexed by item: n_ends, urank, uitem and the
 * middle-list members are ignored).
 * Work units U (built by the caller from xmap_path_weights: xmap_path_plan): unit u = (unit_start, chunk unit_c of unit_G).
 *   unit_G == 1, unit_row == -1: one wave owns the start, uses its slot row and finalises it;
 *   unit_G  > 1: the start's (head, t) entries are dealt round-robin to unit_G consecutive units with
 *   dedicated rows unit_row .. unit_row+G-1 of R->hacc / R->htouched; heavy_unit0[h] = first unit of heavy start h
 *   (n_heavy of them); the rows are merged and finalised after the enumeration.
 * For every start that has a unit: O->n_cand[start] = number of distinct ends, O->top_end / O->top_val[start][XMAP_TOPC]
 * = the candidates a Generator reads (stable sort by -|xsim|, generator.py:85,109; ties by ascending end).
 * If O->xs_cap > 0 the full candidate lists are also written: xs_off[start], entries (xs_end, xs_val);
 * needs xs_cap >= total (reported in h_counters[0]; XMAP_ERR_CAPACITY otherwise).  h_counters[1] = paths.
 * scratch R (zero-filled by the caller, left zero): acc[n_slots][I][4], hacc[n_rows][I][4] doubles;
 * touched[n_slots][I], htouched[n_rows][I] int32. */
int xmap_extend_paths(void *stream, const xmap_ext_tables *T, const xmap_path_units *U, const xmap_path_rows *R,
                      const xmap_path_out *O, int64_t *d_counters /*[4] device*/, int64_t *h_counters /*[4]*/);

/* Second formulation of the enumeration ("middle lists"): per non-bridge record x' (nb_list, n_nb of
 * them; nb_id[i] = position of i in nb_list or -1) the middles (t,s,x) of all joint paths through x' are materialised
 * once as 64-byte records grouped per tile (x', x).  A dense n_nb x n_nb table gives the tile sizes (stage_b_xcheck.hip):
 *   xmap_mid_tally : tile_cnt[x'][x] and ng[x'] = number of non-empty tiles of x';
 *   (caller: exclusive scans tile_cnt -> tile_off [n_nb*n_nb+1], ng -> dir_ptr [n_nb+1]; allocates dir, midX)
 *   xmap_mid_place : the tile directory of every x' (24 B per tile: x, 1+|NN(x)|, count, offset) and the records.
 * Both read n_items, top_k, cls .. flags, att_*, src_*; n_nb, nb_list, nb_id; xmap_mid_place also dir_ptr (it writes
 * through its dir / midX arguments: the members of T are const).
 * xmap_extend_paths2 is xmap_extend_paths with the joint paths streamed from these lists, tile-major: the (up to 64)
 * heads of a start are merged by x, a lane keeps its end's double-double sums in registers across all tiles (x', x)
 * of the start's heads, so a start's row is touched once per (start, x) instead of once per path.  Same results
 * (the sums are exact).  Reads what xmap_extend_paths reads + n_nb (> 0), nb_id, nb_list, midX, dir, dir_ptr. */
#ifdef XMAP_CROSSCHECK   /* test formulation: exported by libxmap_hip_xcheck.so only (csrc/Makefile), never by the product library */
int xmap_mid_tally(void *stream, const xmap_ext_tables *T, int32_t *tile_cnt /*[n_nb*n_nb]*/, int32_t *ng /*[n_nb]*/);
int xmap_mid_place(void *stream, const xmap_ext_tables *T, int32_t *tile_cnt, const int64_t *tile_off /*[n_nb*n_nb+1]*/,
                   void *dir /*24 B per tile*/, void *midX /*64 B per record*/);
int xmap_extend_paths2(void *stream, const xmap_ext_tables *T, const xmap_path_units *U, const xmap_path_rows *R,
                       const xmap_path_out *O, const int32_t *ng /*[n_nb] of xmap_mid_tally / xmap_mid_rows_count*/,
                       int64_t *d_counters, int64_t *h_counters);
#endif /* XMAP_CROSSCHECK */
/* Row-wise construction of the same lists (default, any n_nb; mid_rows.hip): one block per x' keeps the tile sizes of its
 * row in LDS -- XMAP_MID_ROWS_SPAN columns at a time; a row with more non-bridge items is built in column ranges, one after
 * the other -- so there is no n_nb x n_nb table and no global atomic:
 *   xmap_mid_rows_count : ng[x'] = non-empty tiles, nrec[x'] = records of x';
 *   (caller: exclusive scans ng -> dir_ptr [n_nb+1], nrec -> rec_ptr [n_nb+1]; allocates dir, midX)
 *   xmap_mid_rows_place : the tile directory (in x order) and the records of every x'.
 * Both read n_items, top_k, cls .. flags, att_*, src_*; n_nb, nb_list, nb_id; xmap_mid_rows_place also dir_ptr (it writes
 * through its dir / midX arguments).
 * Output identical to xmap_mid_tally / xmap_mid_place up to the order of the records inside a tile. */
#define XMAP_MID_ROWS_SPAN 36864   /* columns of a row whose counters fit the LDS of a block (4 B each; 160 KB per CU on gfx950, 7 KB of it the walk's tables) */
int xmap_mid_rows_count(void *stream, const xmap_ext_tables *T, int32_t *ng /*[n_nb]*/, int64_t *nrec /*[n_nb]*/);
int xmap_mid_rows_place(void *stream, const xmap_ext_tables *T, const int64_t *rec_ptr /*[n_nb+1]*/, void *dir /*24 B per tile*/,
                        void *midX /*64 B per record*/);

/* ---- extension, column form (default) ----------------------------------------------------------------------------
 * Same work units and results as xmap_extend_paths2 (units = starts, heavy starts cut into unit_G chunks with dedicated
 * rows), rebuilt around what bounds it: a column (start, x) is ONE set of lanes -- W ends x S record
 * slices, S = 4 / 2 / 1 by the column's width -- and one row update; rows are indexed by the rank of the end among
 * the n_ends items that can end a path at all (xmap_end_universe: urank[item] / uitem[rank]) instead of by item; the
 * ends of a column come from one table of 32-byte records; sums are (value, error) pairs folded at the end.
 * Scratch (zero-filled by the caller once, returned zeroed): acc [n_slots][n_ends][4] doubles, touched
 * [n_slots][n_ends], hacc [rows][n_ends][4], htouched [rows][n_ends].  fast_div: every edge has a positive mutuality
 * and |sim * mutu| within 2^+-400 (what stage A produces), so the division of a path is the bare
 * reciprocal-refinement sequence.  Results as xmap_extend_paths (same exact sums). */
/* fast_div precondition of xmap_extend_cols over a similarity matrix: *h_fast_ok = 1 iff every kept pair has mutu >= 1
 * and sim * mutu is zero or within 2^+-400 (always true for what stage A produces; 0 for a matrix that carries its own
 * frac column, i.e. generic records).  One pass over the pairs; synchronises. */
int xmap_edge_ranges(void *stream, const xmap_sim *S, int32_t *h_fast_ok);
int xmap_end_universe(void *stream, const xmap_ext_tables *T, int32_t *mark /*[I] scratch*/, int64_t *rank /*[I+1] scratch*/,
                      int32_t *urank /*[I]*/, int32_t *uitem /*[I]*/, int64_t *h_n_ends);
int xmap_extend_cols(void *stream, const xmap_ext_tables *T, const xmap_path_units *U, const xmap_path_rows *R,
                      const xmap_path_out *O, int fast_div, int64_t *d_counters /*[8] device*/,
                      int64_t *h_counters /*[8]: candidates, paths, -, -, row updates (read-modify-writes of row entries)*/);
/* Size limits of the extension live in the HOST layer, not here: the Python engine refuses an extension of more than
 * XMAP_MAX_PATHS paths (5e12) before calling xmap_extend_cols and enumerates path by path (xmap_extend_paths) when the middle
 * lists would exceed XMAP_MID_BUDGET_GB (100 GB); xmap_ctx_extend refuses both.  INTEGRATION.md, "Limits a caller can hit".
 * accumulator rows xmap_extend_cols can keep busy: one per wavefront resident on the device (compute units x SIMDs x the
 * kernel's waves per SIMD); what a caller sizes xmap_path_rows.n_slots with (more rows are never touched). */
int xmap_extend_cols_slots(int32_t *h_n_slots);

/* ---- planning steps of stage B (round 1 did these with torch ops on the device) ----------------------------------
 * xmap_nb_index : nb_list = the non-bridge records (cls == 2) in item order, nb_id[item] = position in it or -1.
 * xmap_path_plan: work units of the enumeration from the exact per-start path counts (xmap_path_weights): starts in
 *   [start_lo, start_hi) with more than `chunk` paths (chunk_div > 0: chunk = max(2^22, paths in the range / chunk_div))
 *   are cut into ceil(paths / chunk) chunks with dedicated rows
 *   (chunk doubles until their rows fit max_rows); units heaviest first (own stable radix sort), the chunks of a start
 *   consecutive.  h_out = {units, heavy starts, rows, paths in the range, chunk used}; XMAP_ERR_CAPACITY with the
 *   counts filled in when the unit arrays (cap_units entries each; heavy_unit0: one per heavy start) are too small
 *   (call with cap_units = 0 and NULL arrays to size them).
 * xmap_end_order: reorders the end universe (urank / uitem of xmap_end_universe, in place) so that every end sits
 *   with the first column x whose end list {x} + NN(x) holds it: the ends of a column are then neighbours in a row. */
int xmap_nb_index(void *stream, int32_t n_items, const uint8_t *cls, int32_t *nb_list, int32_t *nb_id, int64_t *h_n_nb);
int xmap_path_plan(void *stream, int32_t n_items, const int64_t *paths, int32_t start_lo, int32_t start_hi, int64_t chunk,
                   int64_t chunk_div, int64_t max_rows, int64_t cap_units, int32_t *unit_start, int32_t *unit_c, int32_t *unit_G,
                   int32_t *unit_row, int32_t *heavy_unit0, int64_t *h_out);
int xmap_end_order(void *stream, int32_t n_items, int top_k, int32_t n_nb, const int32_t *nb_list, const int32_t *kcnt,
                   const int32_t *kcol, int32_t n_ends, int32_t *urank, int32_t *uitem);

/* Candidate arrays from explicit X-Sim lists (an extended_simRDD that did not come from this engine,
 * e.g. a canonically re-fed one): CSR (xs_ptr, xs_end, xs_val) -> n_cand, top_end, top_val as above. */
int xmap_topc_from_lists(void *stream, int32_t n_items, const int64_t *xs_ptr, const int32_t *xs_end,
                         const double *xs_val, int32_t *n_cand, int32_t *top_end, double *top_val);

/* ---- dense item-factor variant (BASELINE.json configs[4]; no counterpart in the reference) --------------------
 * xsim(t, s) = cosine of K-dimensional item factors: a dense (n_t x K) x (K x n_s) contraction on the fp32 matrix
 * cores (v_mfma_f32_32x32x2_f32; the accumulation is the k-ordered fmaf chain, bit for bit) with the per-row top-k
 * by (|sim| desc, source index asc) fused behind it.  normalize: Fn = F / ||F|| (norm in fp64).  top_k <= 64,
 * dim in {64, 128}.  out_idx/out_val: [n_t][top_k], unused entries -1 / 0.  The (row block x source tile) work grid
 * is cut into one equal share per resident workgroup; a row block whose tiles fall into several shares is ranked in
 * pieces that a merge kernel folds.  xmap_dense_layout (host only) returns the pieces per row the scratch
 * part_idx/part_val [n_t][n_pieces][top_k] must hold (1: scratch unused, may be NULL). */
int xmap_dense_normalize(void *stream, int32_t n, int32_t dim, const float *F, float *Fn);
int xmap_dense_layout(int32_t n_t, int32_t n_s, int32_t *n_pieces);
int xmap_dense_topk(void *stream, int32_t n_t, int32_t n_s, int32_t dim, const float *Ft, const float *Fs, int32_t top_k,
                    int32_t n_pieces, int32_t *part_idx, float *part_val, int32_t *out_idx, float *out_val);

/* ---- RecommenderPrivacy.nonprivate_neighbor_selection (core/recommenderPrivacy.py:22-35,141-152)
 * over the RecommenderSim rows (CSR of xmap_sim2_scatter with ls): per item the `keep` (= mapping_range, <= 64)
 * neighbours by (|sim| desc, neighbour index asc) -- the reference's stable sort keeps the arrival order of equal
 * similarities, which Spark does not define.  out_col/out_sim/out_ls: [I][keep], unused entries -1 / 0; out_cnt [I]. */
int xmap_rec_select(void *stream, int32_t n_items, const int64_t *row_ptr, const int32_t *col, const double *sim,
                    const double *ls, int32_t keep, int32_t *out_cnt, int32_t *out_col, double *out_sim, double *out_ls);

/* ---- RecommenderPrediction.item_based_prediction (core/recommenderPrediction.py:26-105): one test pair
 * (user, item) per thread.  test_item = -1: the item has no neighbour list (the reference emits ()), status 1.  Neighbour
 * lists nb_* in the order of the similarity broadcast; the ratings of an item rt_* sorted by user index, stable, so that a
 * user's ratings of an item keep their list order (test_user = -1: a user without ratings); times as numbers whose order
 * and ties are those of the reference's time objects.  wtab[d] = exp(-alpha d) for d = 0 .. n_w - 1, made by the host with
 * the reference's np.exp.  out_plain / out_decay: bound_rating(prediction without / with temporal decay) (:17-23, :86-97);
 * status 2: more than 64 evidence entries (or more ranks than wtab holds) -- the caller decides that pair on the host.
 * The reference tests `uid in rater_id` (substring); the host maps that to user indices (equality when all ids have one
 * length). */
int xmap_predict(void *stream, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const int64_t *nb_ptr,
                 const int32_t *nb_item, const double *nb_sim, const int64_t *rt_ptr, const int32_t *rt_user, const double *rt_rating,
                 const double *rt_time, const double *item_avg, const double *wtab, int32_t n_w, double *out_plain,
                 double *out_decay, int32_t *status);

/* ---- the device-resident recommender tail (csrc/stage_e_rows.hip): AlterEgo rows -> profiles -> prediction -> MAE, no host
 * conversion in between.
 * xmap_rec_profiles: the rows of xmap_alterego_fill (pass-through segment [0, n_target_rows), then the mapped segment, each in
 *   user order; off_t / off_m [U+1] = the exclusive scans of xmap_alterego_count's counts that the fill pass took) -> user-major
 *   profiles prof_ptr [U+1], prof_item / prof_rating / prof_time [n_rows]: a user's rows contiguous, in stage-C row order
 *   (its pass-through rows, then its mapped rows).  Item indices are unchanged (the engine's index space), so the profiles
 *   are the CSR that xmap_sim3_layout takes with rating64 = prof_rating (RecommenderSim).
 * xmap_predict_rows: RecommenderPrediction.item_based_prediction (core/recommenderPrediction.py:26-105), one wave per test
 *   pair.  Neighbour lists in the layout xmap_rec_select writes: nb_cnt [I] (<= 0: the item has no list, status 1),
 *   nb_col / nb_sim [I][keep], keep <= 64; evidence = for each neighbour in list order the rows of the test user's profile
 *   that hold it, in profile order (user test = equality of indices; test_user outside [0, n_users): a user without rows);
 *   item_avg [I]; wtab[d] = exp(-alpha d), d = 0 .. n_w - 1, made by the caller.  Sums left to right in fp64, decayed sums in
 *   stable time order, equal times share a rank, now = ranks + 1, bound_rating -- the Python statement bit for bit.  No limit
 *   on the evidence of a pair (more than 128 entries: a second launch stages them in a temporary sized by the first).
 *   status: 0 predicted, 1 no neighbour list, 2 the Python statement raises here (zero weight sum, non-finite value) or
 *   now > n_w.  *h_max_now (may be NULL) = the largest `now` met: a table of that many entries serves every pair.  Syncs.
 * xmap_mae: calculate_mae (:107-139) over the pairs with status 0: mae[0] = their count, mae[1] = sum |real - plain|,
 *   mae[2] = sum |real - decayed| (device, 3 doubles); exact double-double sums rounded once, independent of the order. */
int xmap_rec_profiles(void *stream, int64_t n_users, int64_t n_rows, int64_t n_target_rows, const int64_t *off_t, const int64_t *off_m,
                      const int32_t *user, const int32_t *item, const double *rating, const int64_t *time, int64_t *prof_ptr,
                      int32_t *prof_item, double *prof_rating, int64_t *prof_time);
int xmap_predict_rows(void *stream, int64_t n_test, const int32_t *test_user, const int32_t *test_item, int64_t n_users,
                      int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim,
                      const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time,
                      const double *item_avg, const double *wtab, int32_t n_w, double *out_plain, double *out_decay,
                      int32_t *status, int32_t *h_max_now);
int xmap_mae(void *stream, int64_t n_test, const int32_t *status, const double *real, const double *out_plain, const double *out_decay,
             double *mae /*[3], device*/);

/* ---- top-N recommendation (csrc/stage_e_topn.hip): per query user the n_top best items among those the user's own rows give
 * evidence for, ranked by the UNROUNDED prediction.  Same arrays as xmap_predict_rows (neighbour lists nb_cnt [I], nb_col /
 * nb_sim [I][keep], keep <= 64; profiles; item_avg [I]; wtab[d] = exp(-alpha d), d = 0 .. n_w - 1).
 *   candidates of user u: the items i with nb_cnt[i] > 0 of whose first min(nb_cnt[i], keep) neighbours u's profile holds at
 *     least one (an entry outside [0, I) is ignored), and -- without XMAP_TOPN_KEEP_HELD -- that u does not hold itself.  An
 *     item without evidence is never a candidate (its prediction is the item average, the same for every user).
 *   scores: `plain` and `decayed`, the two values xmap_predict_rows holds before bound_rating -- the same kernel body, so the
 *     same operations in the same order (evidence in list order, within a neighbour in profile order, sums left to right in
 *     fp64, decayed sums in stable time order, equal times share a rank, now = ranks + 1); no limit on the evidence.  A
 *     candidate xmap_predict_rows would give status 2 (zero weight sum, non-finite value, now > n_w) is dropped and counted.
 *   ranking: by rank_by (0 plain, 1 decayed) descending, item index ascending on equal scores (scores compare as numbers).
 *   outputs per query q (device): out_cnt[q] = min(n_top, candidates kept); out_item [q][n_top] (-1 behind the count),
 *     out_plain / out_decay [q][n_top] (0.0 behind the count).  1 <= n_top <= 64.  A query user outside [0, n_users) or without
 *     rows gets count 0; query users may repeat, in any order.  The result is a pure function of the inputs.
 *   h_stats (host, [4] or NULL): candidates scored, candidates dropped, the largest `now` met (beyond n_w: call again with a
 *     table of that length, as with xmap_predict_rows), the largest candidate count of one query.
 * Passes: reverse neighbour lists (count, scan, fill) -> candidates per query through an LDS bitmap of the item space (count,
 * scan, fill: buffers of exactly the counted size) -> scores -> segmented selection.  Temporaries from the stream's arena.  Syncs. */
#define XMAP_TOPN_KEEP_HELD 1
int xmap_topn_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                   int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                   const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                   const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w,
                   int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay,
                   int64_t *h_stats /* host, [4] or NULL: candidates scored, candidates dropped (status 2),
                                       largest `now`, largest candidate count of one query */);

/* ---- diversified top-N (csrc/stage_e_diverse.hip; DESIGN.md 4 "Diversified lists"): a greedy maximal-marginal-relevance
 * re-ranking of a top-M pool into a top-N list by item similarity, and the intra-list similarity (ILS) of every returned list.
 * xmap_div_index: the diversity index of a RecommenderSim CSR (row_ptr [I+1], col / sim [nnz], as xmap_ctx_rec_sim and
 *   Engine.rec_sim leave it; any order inside a row): dv_col [nnz] = every row's columns ascending, dv_abs [nnz] = fabs(sim)
 *   beside them; row_ptr is shared.  A pure function of the CSR as a set of entries per row.  A row holds a column at most once:
 *   the repeated (row, column) entries are counted into *h_dups (host, may be NULL) and, if there are any, the call returns
 *   XMAP_ERR_ARG (as for a column outside [0, I)).  nnz < 2^31.  Temporaries (24 B per entry) from the stream's arena.  Syncs.
 * xmap_diversify_rows: per query q the pool in_cnt[q], in_item / in_plain / in_decay [q][n_pool] as xmap_topn_rows writes it with
 *   n_top = n_pool (pool position = rank; entries behind the count are ignored), 1 <= n_top <= n_pool <= 64, weight finite and
 *   >= 0 (else XMAP_ERR_ARG before any device work):
 *     n = min(in_cnt, n_top); live = positions 0 .. in_cnt-1; pen[j] = sum[j] = 0.0; pairsum = 0.0
 *     for r = 0 .. n-1:
 *       obj[j] = score[j] - weight * pen[j]      (score by rank_by; one fp64 multiply, one fp64 subtract)
 *       j* = the live position with the largest obj (as numbers), the smallest position on equal obj
 *       out_item / out_plain / out_decay [q][r] = the pool's at j*, out_pos[q][r] = j*, out_pen[q][r] = pen[j*]
 *       pairsum += sum[j*]; j* leaves live
 *       if r + 1 < n and 0 <= in_item[j*] < n_items: for every live c whose item is a column of row in_item[j*], with v = dv_abs
 *         there: pen[c] = v if v > pen[c] (a NaN never raises a penalty); sum[c] += v
 *     out_cnt[q] = n; out_ils[q] = pairsum / (n (n - 1) / 2), 0.0 for n < 2
 *   Behind the count: item -1, position -1, 0.0.  Sums in fp64 in pick order.  weight = 0 returns the pool's prefix bit for bit,
 *   with its ILS.  The similarities are finite (an infinite one makes obj a NaN at weight 0: no order is promised then).  Outputs
 *   may not alias inputs.  h_stats (host, [2] or NULL): queries whose list differs from the pool's prefix, sum of out_cnt; the
 *   call syncs only when it is given.  One wave per query; a pure function of the inputs. */
int xmap_div_index(void *stream, int32_t n_items, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const double *sim,
                   int32_t *dv_col, double *dv_abs, int64_t *h_dups /* host, may be NULL */);
int xmap_diversify_rows(void *stream, int64_t n_query, int32_t n_pool, const int32_t *in_cnt, const int32_t *in_item,
                        const double *in_plain, const double *in_decay, int32_t rank_by, double weight, int32_t n_top,
                        int32_t n_items, const int64_t *row_ptr, const int32_t *dv_col, const double *dv_abs,
                        int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos,
                        double *out_pen, double *out_ils,
                        int64_t *h_stats /* host [2] or NULL: queries whose list differs from the pool prefix, sum of out_cnt */);

/* ---- audience of an item (csrc/stage_e_audience.hip): per query item the n_top best USERS among those whose own rows give
 * evidence for it, ranked by the UNROUNDED prediction -- xmap_topn_rows seen from the item.  Same arrays as xmap_topn_rows, in its
 * order; query_item replaces query_user and out_user replaces out_item.
 *   candidates of item i: the users u whose profile holds at least one of the first min(nb_cnt[i], keep) neighbours of i (an
 *     entry outside [0, I) is ignored) and -- without XMAP_AUDIENCE_KEEP_HOLDERS -- who do not hold i itself.  (u, i) is a
 *     candidate pair here iff i is a candidate of u in xmap_topn_rows (KEEP_HOLDERS <-> KEEP_HELD).  Within a query the
 *     candidates are scored in ascending user index, each once (also a user who holds a neighbour twice, or two neighbours).
 *   scores: `plain` and `decayed` of the pair (u, i), the values xmap_predict_rows holds before bound_rating -- the same kernel
 *     body over the candidate list, so the same bits as xmap_topn_rows gives the pair.  A candidate xmap_predict_rows would give
 *     status 2 (zero weight sum, non-finite value, now > n_w) is dropped and counted.
 *   ranking: by rank_by (0 plain, 1 decayed) descending, user index ascending on equal scores (scores compare as numbers:
 *     -0.0 == 0.0).
 *   outputs per query q (device): out_cnt[q] = min(n_top, candidates kept); out_user [q][n_top] (-1 behind the count),
 *     out_plain / out_decay [q][n_top] (0.0 behind the count).  1 <= n_top <= 1024; keep <= 64; n_users < 2^31.  A query item
 *     outside [0, n_items) or with nb_cnt <= 0 gets count 0; query items may repeat, in any order.  The result is a pure function
 *     of the inputs: it depends neither on the grid nor on the order of any atomic.
 *   h_stats (host, [4] or NULL): candidates scored, candidates dropped, the largest `now` met (beyond n_w: call again with a
 *     table of that length, as with xmap_predict_rows), the largest candidate count of one query.
 * Passes: holders = the profiles by item (count, scan, fill: 8 B per profile row, built inside every call) -> candidates per
 * query through an LDS bitmap of the user space, window by window (count, scan, fill: buffers of exactly the counted size) ->
 * scores -> segmented selection, one block per query.  Temporaries from the stream's arena.  Syncs. */
#define XMAP_AUDIENCE_KEEP_HOLDERS 1
int xmap_audience_rows(void *stream, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags,
                       int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                       const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                       const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w,
                       int32_t *out_cnt, int32_t *out_user, double *out_plain, double *out_decay,
                       int64_t *h_stats /* host, [4] or NULL: candidates scored, candidates dropped (status 2),
                                           largest `now`, largest candidate count of one query */);

/* ---- explanation of a recommendation (csrc/stage_e_explain.hip): WHY the score of a (user, item) pair is what it is -- the
 * strongest evidence entries of the score, and for each of those AlterEgo rows the raw ratings stage C made it from.
 * xmap_explain_rows: n_pairs pairs (typically the lists of xmap_topn_rows) against the arrays of xmap_predict_rows, in its
 *   order.  The pair body is the prediction's own (csrc/predict_rows.h, one more compile-time mode), so the evidence list of a
 *   pair -- for l in range(min(nb_cnt[i], keep)), nb = nb_col[i][l] (outside [0, n_items): skipped), for p in
 *   range(prof_ptr[u], prof_ptr[u + 1]) with prof_item[p] == nb: entry q with slot l, row p, e0 = s (prof_rating[p] -
 *   item_avg[nb]), e1 = |s|, time prof_time[p]; n entries --, p1, d1, now, the time ranks, the decay weight wt_q =
 *   wtab[now - rank_q] and the status are exactly what xmap_predict_rows computes.
 *   share of entry q: rank_by 0: e0[q] / p1; rank_by 1: (e0[q] * wt_q) / d1 -- the product rounded first (the same product the
 *   decayed sum adds), then one division.  The shares are what an entry adds to score - item_avg[i]; their rounded sum is NOT
 *   required to reproduce that difference bit for bit (the score divides the sum once, the shares divide every term).
 *   ranking: |share| descending, compared as numbers; ties to the smaller evidence index q (list order, then profile order: the
 *   index before the time sort, also for rank_by 1).  The first min(n_ev, n) entries are reported, 1 <= n_ev <= 16.
 *   outputs per pair t (device): ex_status[t] = the status xmap_predict_rows gives the pair with the same table (0 predicted, 1
 *   no neighbour list, 2 the Python statement raises or now > n_w); ex_total[t] = n (0 when the status is not 0; status 0 with
 *   n = 0 is legal: the score is item_avg[i]); ex_cnt[t] = min(n_ev, n); ex_score[t] = the unrounded score of rank_by (0.0 when
 *   the status is not 0); ex_row [t][n_ev] = absolute index into the profile arrays (-1 behind the count); ex_slot [t][n_ev] =
 *   the list position l (-1 behind the count); ex_share [t][n_ev] (0.0 behind the count).  *h_max_now as xmap_predict_rows.
 *   No limit on n (more than 128 entries: the second launch, as the prediction).  A pure function of the inputs.  Syncs.
 * xmap_explain_sources: the provenance of the reported rows through stage C (k_alterego_grp), which writes a user's profile as
 *   its cnt_t[u] pass-through rows (the raw entries with flags[item] & 2, in raw order), then one row per distinct
 *   map_src2tgt[item] >= 0 in first-seen order carrying the fp64 mean of the group's ratings.  For row p of user u, k = p -
 *   prof_ptr[u]: k < cnt_t[u]: the source is the k-th raw entry of u with flags[item] & 2, src_total = 1; otherwise the sources
 *   are all raw entries e of u with map_src2tgt[raw_item[e]] == prof_item[p], in raw order, src_total their number (the row's
 *   rating is the left-to-right fp64 mean of their fp32 ratings).  Pass cnt_t [n_users] OR off_t [n_users + 1] (its exclusive
 *   scan, as xmap_alterego_fill takes it): exactly one of the two, the other NULL.  raw_ptr [n_users + 1] / raw_item: the raw
 *   profiles the rows were made from (the upload's CSR; a fold-in batch's CSR with its cnt_t).
 *   outputs per (pair, entry): src_total [t][n_ev] (0 behind ex_cnt[t]; -1 for an ex_row outside [prof_ptr[u], prof_ptr[u + 1])
 *   or a pair_user outside [0, n_users): nothing is indexed), src_pos [t][n_ev][n_src] = absolute positions of the first
 *   min(n_src, src_total) sources in the raw arrays (-1 behind that), 1 <= n_src <= 8.  A raw item outside [0, n_items) matches
 *   nothing.  One wave per (pair, entry), no atomics.  Does not sync. */
int xmap_explain_rows(void *stream, int64_t n_pairs, const int32_t *pair_user, const int32_t *pair_item, int32_t rank_by,
                      int32_t n_ev, int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                      const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                      const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w, int32_t *ex_status,
                      int32_t *ex_total, int32_t *ex_cnt, double *ex_score, int64_t *ex_row, int32_t *ex_slot, double *ex_share,
                      int32_t *h_max_now);
int xmap_explain_sources(void *stream, int64_t n_pairs, const int32_t *pair_user, int32_t n_ev, const int32_t *ex_cnt,
                         const int64_t *ex_row, int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                         const int32_t *cnt_t /*[n_users] or NULL*/, const int64_t *off_t /*[n_users + 1] or NULL: exactly one of the two*/,
                         const int64_t *raw_ptr, const int32_t *raw_item, const uint8_t *flags, const int32_t *map_src2tgt,
                         int32_t n_src, int32_t *src_total, int64_t *src_pos);

/* ---- hold-out evaluation of the top-N lists (csrc/stage_e_eval.hip): what xmap_mae is to xmap_predict_rows.  The lists stay
 * where xmap_topn_rows wrote them; the held-out (user, item, rating) pairs are the ones xmap_ctx_predict takes.
 * xmap_eval_users: held-out pairs -> the users worth ranking for.  A pair is IGNORED if user is outside [0, U), item outside
 *   [0, I) or the rating is NaN; otherwise RELEVANT iff rating >= rel_min (rel_min NaN: XMAP_ERR_ARG).  n_rel[u] = relevant
 *   pairs of u (occurrences: the caller passes every (user, item) once, as baselinerSplit does; a repeated relevant pair counts
 *   as often as it occurs here and once as a hit).  eval_user[0 .. n_eval) = the users with n_rel > 0, ascending.
 *   h_counts = {n_eval, relevant pairs, ignored pairs, pairs below rel_min}.  Syncs.
 * xmap_topn_eval: lists as xmap_topn_rows wrote them (out_cnt [Q], out_item [Q][n_top], 1 <= n_top <= 64) for DISTINCT
 *   in-range query users (a repeated user: XMAP_ERR_ARG, found on the device) + the same pairs -> per query the hit mask
 *   (bit r = out_item[q][r] is a relevant held-out item of query_user[q], r < out_cnt[q]), per query and cutoff the five
 *   metrics, and the aggregates.  h_cut: 1 <= n_cut <= 8 cutoffs, strictly ascending, 1 <= c <= n_top.
 *   dtab[r], r < n_top: the rank discount, made by the caller (1 / log2(r + 2)), like wtab.
 *   Per evaluated query -- L the list, R the relevant set, n = n_rel[user], c the cutoff -- every operation fp64 IEEE, the
 *   divisions correctly rounded, sums left to right in ascending rank:
 *       h = 0; dcg = ap = rr = 0.0
 *       for r in range(min(c, len(L))):
 *           if L[r] in R:
 *               h += 1; dcg = dcg + dtab[r]; ap = ap + h / (r + 1)
 *               if rr == 0.0: rr = 1.0 / (r + 1)
 *       idcg = 0.0
 *       for r in range(min(c, n)): idcg = idcg + dtab[r]
 *       precision, recall, ndcg, ap, rr = h / c, h / n, dcg / idcg, ap / min(c, n), rr
 *   q_metric [Q][n_cut][5] = (precision, recall, ndcg, ap, rr); may be NULL.
 *   A query whose user is out of range or has n_rel == 0 is not evaluated: mask 0, metrics 0.0, not counted.
 *   agg [n_cut][8] (device) = {evaluated queries, queries with a hit within c, hits within c, sum precision, sum recall,
 *   sum ndcg, sum ap, sum rr}: the first three exact integers, the sums exact double-double sums rounded once (as xmap_mae),
 *   so independent of grid and order.  cover [n_cut] (device) = distinct items in the first min(c, out_cnt[q]) positions
 *   over ALL queries.  Temporaries from the stream's arena.  Syncs. */
int xmap_eval_users(void *stream, int64_t n_test, const int32_t *test_user, const int32_t *test_item,
                    const double *test_rating, double rel_min, int64_t n_users, int32_t n_items,
                    int32_t *n_rel /*[U]*/, int32_t *eval_user /*[U]*/, int64_t *h_counts /*[4]*/);
int xmap_topn_eval(void *stream, int64_t n_test, const int32_t *test_user, const int32_t *test_item,
                   const double *test_rating, double rel_min, int64_t n_users, int32_t n_items, const int32_t *n_rel,
                   int64_t n_query, const int32_t *query_user, int32_t n_top, const int32_t *out_cnt,
                   const int32_t *out_item, int32_t n_cut, const int32_t *h_cut, const double *dtab,
                   uint64_t *q_mask /*[Q]*/, double *q_metric /*[Q][n_cut][5] or NULL*/, double *agg, int64_t *cover);

/* ---- stage C: generator_pipeline (utils/assist.py:136-150) ---------------------------------- */

/* Generator.cross_private_mapping / cross_nonprivate_mapping (core/generator.py:27-111) + map_to_dict
 * (utils/assist.py:210-215).  private: choice = candidate 0 (arg-max |xsim|).  non-private: choice =
 * top4[picks[start]], picks drawn on the host with np.random.randint in ascending start order.
 * n_top[start] = min(private ? 10 : 4, n_cand); map_src2tgt[choice] = largest start choosing it, else -1. */
int xmap_select_map(void *stream, int32_t n_items, int private_flag, const int32_t *n_cand, const int32_t *top_end,
                    const int32_t *picks /* may be NULL */, int32_t *n_top, int32_t *choice, int32_t *map_src2tgt);

/* Generator.build_alterEgo (core/generator.py:113-157).  count pass: cnt_t[u] pass-through rows
 * ("T:" in iid), cnt_m[u] AlterEgo rows (distinct mapped targets, first-seen order).  fill pass writes
 * rows [off_t[u]..) and [n_t_total + off_m[u]..): (user, item, rating = mean fp32, time of first row). */
int xmap_alterego_count(void *stream, const xmap_ratings *R, const int32_t *map_src2tgt, int32_t *cnt_t, int32_t *cnt_m,
                        int64_t *d_profiles /* [64] device, zeroed by the caller: the users with at least one output row are
                                               added to these 64 counters (their sum is the number of profiles); or NULL */);
int xmap_alterego_fill(void *stream, const xmap_ratings *R, const int32_t *map_src2tgt, const int64_t *off_t,
                       const int64_t *off_m, int64_t n_t_total, int32_t *out_user, int32_t *out_item,
                       double *out_rating, int64_t *out_time);
/* The count pass reads n_users, user_ptr, user_item and flags of R; the fill pass user_rating and user_time as well. */

/* ---- fold-in (csrc/stage_c_foldin.hip): AlterEgo profiles of raw profiles that were NOT rows of the ratings upload -- a user
 * who arrived after training, a trained user whose profile changed -- with the replacement map of a finished generate pass.
 * The model stays frozen (the standard item-based fold-in): the profiles enter neither RecommenderSim nor the neighbour lists
 * nor the item averages; they are a second set of user-major profiles for xmap_predict_rows / xmap_topn_rows (n_users = n_new).
 * The batch: n_new profiles as a CSR, ptr [n_new + 1], item / rating / time [nnz], items in the index space of flags and
 * map_src2tgt ([n_items]), source and target items mixed, repeats allowed.  The AlterEgo profile of one raw profile is what
 * xmap_alterego_fill + xmap_rec_profiles give a row of the upload (the same device code): its pass-through rows first (flag
 * bit 1, "T:" in iid) in profile order, then one row per distinct map_src2tgt[item] >= 0 in first-seen order (rating = the
 * fp64 mean of the group's fp32 ratings, time = that of the group's first entry); an entry that is neither gives no row, one
 * that is both gives two.  rows <= 2 nnz.
 * xmap_foldin_count: FIRST checks the batch on the device, reading ptr[0 .. n_new] and item[0 .. nnz) only: ptr[0] == 0, ptr
 *   non-decreasing, ptr[n_new] == nnz, 0 <= item < n_items.  A batch that fails: XMAP_ERR_ARG, xmap_last_error() names the first
 *   bad position, no output is written and nothing has indexed flags or map_src2tgt.  Otherwise cnt_t / cnt_m [n_new] = the
 *   pass-through / mapped rows per profile, prof_ptr [n_new + 1] = the exclusive scan of their sums, h_counts (host) = {rows,
 *   pass-through rows, profiles with at least one row}.  Syncs.
 * xmap_foldin_fill: the rows, into buffers of exactly h_counts[0] entries (not read when that is 0), with the arrays
 *   xmap_foldin_count accepted and its cnt_t and prof_ptr.  Does not sync.
 * n_new == 0 is valid for both (nnz must then be 0).  nnz < 2^31 - 1.  Temporaries from the stream's arena. */
int xmap_foldin_count(void *stream, int64_t n_new, int64_t nnz, const int64_t *ptr, const int32_t *item, int32_t n_items,
                      const uint8_t *flags, const int32_t *map_src2tgt, int32_t *cnt_t /*[n_new]*/, int32_t *cnt_m /*[n_new]*/,
                      int64_t *prof_ptr /*[n_new+1]*/, int64_t *h_counts /* host [3]: rows, pass-through rows, profiles with a row */);
int xmap_foldin_fill(void *stream, int64_t n_new, int64_t nnz, const int64_t *ptr, const int32_t *item, const float *rating,
                     const int64_t *time, int32_t n_items, const uint8_t *flags, const int32_t *map_src2tgt,
                     const int32_t *cnt_t, const int64_t *prof_ptr, int32_t *prof_item, double *prof_rating, int64_t *prof_time);

/* ---- item fold-in (csrc/stage_e_itemfold.hip): one row of RecommenderSim for an ITEM that was not in the ratings upload -- a book
 * that enters the catalogue -- against the resident user-major profiles, with the frozen norms.  The mirror of the user fold-in:
 * the model stays frozen, no resident list or average changes, a batch rating is never evidence.
 * Resident data, read only: prof_ptr [U + 1], prof_item / prof_rating [rows] as xmap_rec_profiles or xmap_union_fill leave them
 * (items inside [0, n_items)); item_norm [I] = the norms RecommenderSim used; cap = its num_atleast.
 * The batch: n_new items as a CSR of raters, ptr [n_new + 1], user [nnz] (indices of resident users), rating [nnz] (fp64); a user
 * may appear more than once under an item, an item may have no entries; there are no times.
 * Records: entries in batch order, within an entry the rater's profile rows in profile order; (entry, row) is one record (q, j =
 * prof_item, r0 = batch rating, r1 = prof_rating).  All sums double-double (dd_add), hi is the value used:
 *   per item q: new_avg = hi(sum r0) / entries, new_norm = nx = sqrt(hi(sum r0 r0)) over its entries (0.0 without entries)
 *   per (q, j) with a record, records in that order: n = their number, inner = hi(sum fl(r0 r1)), ny = item_norm[j], np = nx ny,
 *     sim = weighted(np != 0 ? 1.0 inner / np : 0.0, n, cap) with weighted(x, n, cap) = 1.0 x min(n, cap) / cap (NaN != 0 divides);
 *     ls = the maximum over the records of |weighted(m != 0 ? rest / m : 0.0, n - 1, cap) - sim| for rest = inner - r0 r1 and
 *     m = sqrt((nx nx - r0 r0)(ny ny)), then m = sqrt((nx nx)(ny ny - r1 r1)); NaN ranks above everything -- the operations of
 *     RecommenderSim's resident rows (xmap_sim2_pairs, LS variant), so a copy of a resident item gets that item's row (j != i)
 *   row q of the output: one entry (col = j, sim, ls, nij = n) per such j, in no particular order.  A pure function of the inputs.
 * xmap_itemfold_count: FIRST checks the batch on the device, reading ptr and user only: ptr[0] == 0, ptr non-decreasing,
 *   ptr[n_new] == nnz, 0 <= user < n_users.  A batch that fails: XMAP_ERR_ARG, xmap_last_error() names the first bad position, no
 *   output is written and nothing has been indexed by an unchecked value.  Otherwise cnt [n_new] = entries per row, row_ptr
 *   [n_new + 1] = their exclusive scan, h_counts (host) = {pairs, records, items with a pair}.  Syncs.
 * xmap_itemfold_fill: the rows, into buffers of exactly h_counts[0] entries, with the arrays xmap_itemfold_count accepted and its
 *   row_ptr; new_avg / new_norm [n_new].  Syncs.
 * Both work in chunks of consecutive batch items whose records number at most max_records (0: the library's default, 2^22; a
 * single item above the bound is a chunk of its own; a chunk's records stay below 2^31: XMAP_ERR_CAPACITY for a larger single
 * item): expand -> stable radix sort by (item, partner) -> run heads -> one lane per run.  No lock, no floating-point atomic,
 * every output position from counts and scans; the result does not depend on max_records.  n_new == 0 is valid.  nnz < 2^31 - 1.
 * Temporaries from the stream's arena.
 * The neighbour list of q: xmap_rec_select over these rows with n_items = n_new.  The EXTENDED tables of I' = I + n_new items --
 * rows [0, I) the resident nb_cnt / nb_col / nb_sim and item_avg, row I + q the list and new_avg of q; list entries are resident
 * indices < I -- serve xmap_predict_rows, xmap_topn_rows and xmap_explain_rows as they are, with the unchanged profiles.
 * xmap_itemfold_audience_rows: xmap_audience_rows over the extended tables (n_items = n_resident + n_new; the arguments of
 *   xmap_audience_rows position for position, then three more): the holders of item n_resident + q are its raters new_user[new_ptr[q]
 *   .. new_ptr[q + 1]) (device) -- without XMAP_AUDIENCE_KEEP_HOLDERS they are no candidates, with it they are. */
int xmap_itemfold_count(void *stream, int64_t n_new, int64_t nnz, const int64_t *ptr, const int32_t *user, int64_t n_users,
                        int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                        int64_t max_records /* 0: the library's default */, int32_t *cnt /*[n_new]*/, int64_t *row_ptr /*[n_new+1]*/,
                        int64_t *h_counts /* host [3]: pairs, records, items with a pair */);
int xmap_itemfold_fill(void *stream, int64_t n_new, int64_t nnz, const int64_t *ptr, const int32_t *user, const double *rating,
                       int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                       const double *item_norm, int32_t cap, int64_t max_records, const int64_t *row_ptr, int32_t *col, double *sim,
                       double *ls, int32_t *nij, double *new_avg /*[n_new]*/, double *new_norm /*[n_new]*/);
int xmap_itemfold_audience_rows(void *stream, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags,
                                int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                                const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                                const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w,
                                int32_t *out_cnt, int32_t *out_user, double *out_plain, double *out_decay,
                                int64_t *h_stats /* host, [4] or NULL, as xmap_audience_rows */,
                                int32_t n_resident, const int64_t *new_ptr /*[n_new+1]*/, const int32_t *new_user);

/* ---- eligibility rules for xmap_topn_rows and xmap_audience_rows (csrc/rec_filter.h; DESIGN.md 4 "Eligibility"): which ids a
 * call may return at all.  The rules act inside the candidate pass, BEFORE scoring -- no ineligible pair is scored -- so the n_top
 * best ELIGIBLE candidates are selected, which no filter over a returned list can do.  n = n_items (top-N) or n_users (audience). */
typedef struct {
    const uint32_t *allow;  /* bit (id & 31) of word (id >> 5) set: id is eligible.  (n + 31) / 32 words, n = n_items (top-N)
                               or n_users (audience).  Bits at or beyond n may hold anything.  NULL: every id is eligible. */
    const int64_t *ex_ptr;  /* [n_query + 1], ex_ptr[0] = 0, non-decreasing.  NULL: no exclusions. */
    const int32_t *ex_id;   /* ids never returned for query q: ex_id[ex_ptr[q] .. ex_ptr[q + 1]).  Any order, repeats allowed,
                               an id outside [0, n) is ignored.  Per QUERY, not per user: a repeated query may carry another list. */
    double min_score;       /* a scored candidate is kept iff its rank_by score >= min_score (as numbers).  -INFINITY: no floor.
                               NaN: XMAP_ERR_ARG. */
} xmap_rec_filter;
/* The fine-grained calls take DEVICE pointers in the struct (itself in host memory), the coarse calls host pointers.  F == NULL
 * means {NULL, NULL, NULL, -INFINITY}, and with such a filter the calls return, bit for bit, what the unfiltered calls return.
 * Order of the rules: (1) the candidates as in the unfiltered call; (2) without the KEEP_* flag the held items / the holders
 * leave; (3) the ids of the query's exclusion list leave; (4) what remains is intersected with allow; (5) scores; (6) the
 * status-2 candidates are dropped and counted; (7) the candidates below the floor are dropped and counted; (8) selection --
 * ranking, ties and padding exactly as in the unfiltered calls.
 * h_stats (host, [6] or NULL): [0..3] as in the unfiltered calls, taken over the ELIGIBLE candidates; [4] = candidates with status
 * 0 whose rank_by score is below min_score; [5] = candidate pairs removed by the mask or the exclusion lists = the [0] of the
 * unfiltered call minus this call's [0] (a held item that is also excluded does not count, a repeated exclusion counts once).
 * The scoring pass, shared with the unfiltered calls and xmap_predict_rows, starts one wave per pair; it is launched in ranges of
 * 15 * 2^22 (6.3e7) pairs, so the pair count of a call (h_stats[0]) is bounded by the memory per pair only (28 B of temporaries per candidate
 * pair, 16 B per pair in xmap_predict_rows), not by the 2^32 threads of a grid.
 * ex_ptr is checked on the device before any candidate work (ex_ptr[0] == 0, non-decreasing; ids listed while ex_id == NULL):
 * XMAP_ERR_ARG, nothing is read through a table that fails.
 * xmap_topn_rows_filtered: the arguments of xmap_topn_rows up to out_decay, then F and h_stats [6].
 * xmap_audience_rows_filtered: the arguments of xmap_itemfold_audience_rows up to out_decay, then n_resident, new_ptr, new_user
 *   (new_ptr == NULL: resident items only, n_resident is ignored), then F and h_stats [6]: one entry for both audience calls. */
int xmap_topn_rows_filtered(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                            int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                            const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                            const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w,
                            int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay,
                            const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [6] or NULL */);
int xmap_audience_rows_filtered(void *stream, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by, int32_t flags,
                                int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                                const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                                const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w,
                                int32_t *out_cnt, int32_t *out_user, double *out_plain, double *out_decay,
                                int32_t n_resident, const int64_t *new_ptr /*[n_new+1] or NULL*/, const int32_t *new_user,
                                const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [6] or NULL */);

/* ---- group lists (csrc/stage_e_group.hip; DESIGN.md 4 "Group lists"): ONE top-N list for several users -- a household, a party
 * of four, a shared account -- by aggregating the members' UNROUNDED predictions.  Combining per-member lists of xmap_topn_rows on
 * the host cannot do this: the cut is inside the kernel (an item that is tenth for every member is first for the group and in
 * nobody's list), and a member without evidence for an item still predicts it -- the item average -- which no list carries.
 * Inputs: the arrays of xmap_topn_rows (profiles, nb_cnt / nb_col / nb_sim [I][keep], item_avg, wtab / n_w), and
 *   groups as a CSR: grp_ptr [G + 1] (grp_ptr[0] = 0, non-decreasing), grp_user [grp_ptr[G]]; how = XMAP_GROUP_MEAN (average),
 *   XMAP_GROUP_MIN (least misery) or XMAP_GROUP_MAX (most pleasure); veto; flags (XMAP_TOPN_KEEP_HELD only); F or NULL.
 * Members: group g has the members u_0 .. u_{m-1} in list order, 0 <= m <= XMAP_GROUP_MAX_MEMBERS.  A repeated member counts as
 *   often as it is listed (a weight).  A member outside [0, n_users) or without rows is still a member: it holds nothing and has
 *   no evidence for anything, as in xmap_predict_rows.
 * Candidates of g: (1) the items i that are a candidate of at least one member in the sense of xmap_topn_rows with KEEP_HELD
 *   (nb_cnt[i] > 0 and the member's profile holds one of the first min(nb_cnt[i], keep) neighbours; an entry outside [0, I) is
 *   ignored); (2) without XMAP_TOPN_KEEP_HELD every item that ANY member holds leaves; (3) the ids of the group's exclusion list
 *   leave (F->ex_ptr is indexed by group); (4) the rest is intersected with F->allow.  In ascending item index, each once.
 * Member scores: s_j = the unrounded `plain` (and, separately, `decayed`) of the pair (u_j, i), exactly as xmap_topn_rows gives
 *   it; if u_j has no evidence for i, s_j = item_avg[i], the same bits (the prediction's own answer for such a pair).  A
 *   candidate is dropped and counted in stats[1] if some member's pair has status 2 (zero weight sum, non-finite value, now > n_w)
 *   or some member lacks evidence while item_avg[i] is not finite.  stats[2] = the largest `now` met; beyond n_w: call again with
 *   a table of that length, as with xmap_topn_rows.
 * Aggregate, for plain and for decayed by the same rule: MEAN = (((s_0 + s_1) + ...) + s_{m-1}) / (double)m -- fp64 sums left to
 *   right starting from s_0 (not from 0.0 + s_0), one division; MIN / MAX: compared as numbers, on equal values the earliest member
 *   in list order supplies the bits.
 * Veto ("average without misery"): a candidate leaves and is counted in stats[6] if some member's rank_by score is < veto, as
 *   numbers, under every `how`.  veto = -INFINITY: no veto.  NaN: XMAP_ERR_ARG.
 * Floor: F->min_score acts on the AGGREGATE rank_by score; counted in stats[4].  Order of the drops: status 2, veto, floor.
 * Ranking: by the aggregate rank_by score descending, item index ascending on equal scores (scores compare as numbers).
 * Outputs (device): out_cnt [G]; out_item / out_plain / out_decay [G][n_top] with -1 / 0.0 / 0.0 behind the count, exactly as
 *   xmap_topn_rows writes them -- so xmap_diversify_rows takes them as a pool unchanged; out_low [G][n_top] = the position j in the
 *   group's list of the member with the smallest rank_by score for that item, the smallest such j on ties, -1 behind the count
 *   ("who likes this least").  1 <= n_top <= 64.  A group with m = 0 gets count 0.  A pure function of the inputs: it depends on
 *   neither the grid nor the order of the atomics.
 * h_stats (host, [8] or NULL): [0] member pairs scored (pairs with evidence only), [1] group candidates dropped for status 2,
 *   [2] largest `now`, [3] largest candidate count of one group, [4] group candidates below the floor, [5] group candidates
 *   removed by the exclusion lists (a bit still set after step 2; a repeated exclusion counts once; an item F->allow leaves out
 *   is never marked, so it is not counted here), [6] group candidates vetoed, [7] group candidates after steps 1-4, summed over
 *   the groups.  [0] and [2] are taken over the pairs the member pass scores: per listing of a member, the items its rows give
 *   evidence for that F->allow admits and -- without XMAP_TOPN_KEEP_HELD -- that the member does not hold itself.
 * A group of one member under any `how`, veto = -INFINITY, returns the list of xmap_topn_rows_filtered for that user bit for bit,
 *   out_low = 0, stats[0..4] equal.
 * Passes: grp_ptr is checked on the device before any other work (XMAP_ERR_ARG with a message; nothing is read through a table
 *   that fails, the outputs are untouched) -> member pass: the candidate-and-scoring half of xmap_topn_rows over the flattened
 *   member list, under F->allow and the call's flags (an item a member holds leaves the group without KEEP_HELD whoever has
 *   evidence for it, so that member's pair is never needed): per member a segment of (item ascending, plain, decayed, status),
 *   pairs with evidence only -- a pair without evidence predicts item_avg and costs no wave.  A masked item is never scored; an
 *   excluded one may be (the exclusion lists belong to groups, and are short) -> the groups' candidates through the LDS bitmap
 *   (count, scan, fill) -> aggregate and select, one wave per group, a member's score found by bisection in its segment.
 *   Temporaries from the stream's arena; every offset is int64.  Syncs. */
#define XMAP_GROUP_MEAN 0
#define XMAP_GROUP_MIN 1
#define XMAP_GROUP_MAX 2
#define XMAP_GROUP_MAX_MEMBERS 64
int xmap_group_topn_rows(void *stream, int64_t n_groups, const int64_t *grp_ptr, const int32_t *grp_user, int32_t n_top, int32_t rank_by,
                         int32_t flags, int32_t how, double veto,
                         int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col,
                         const double *nb_sim, const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating,
                         const int64_t *prof_time, const double *item_avg, const double *wtab, int32_t n_w,
                         int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_low,
                         const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [8] or NULL */);

/* ---- peers (csrc/stage_e_peers.hip; DESIGN.md 4 "Peers"): "who is this user like?" -- for every query user the n_top resident
 * users with the most similar profiles, by the significance-weighted cosine of RecommenderSim taken between USERS.  All
 * arithmetic is fp64, one rounded operation per step, no fused multiply-add.
 * A profile row p is VALID iff 0 <= prof_item[p] < n_items; invalid rows are ignored everywhere.  x of a row = prof_rating[p] -
 *   centre[prof_item[p]]; centre == NULL: the rating itself.  HOLDER ORDER of item n: the valid resident rows that hold n by
 *   ascending row index (user ascending, then profile order); a user who holds an item twice appears twice.
 * Records of query q with query user a: for each valid row p of a in profile order, for each holder row h of its item in holder
 *   order, the record (v = user of h, t = x of p times x of h).  A user holding an item twice on either side multiplies out.
 * Candidates of q: the users v with at least one record; n = the records of v; dot = the high word of the double-double sum of
 *   t in record order; norm2 of a user = the same form of the user with itself (p over its valid rows, r over its valid rows with
 *   the same item, both in profile order), nrm = sqrt of it (a negative or NaN argument: NaN); the query's nrm by the same code
 *   over the query CSR.  np = nrm of a * nrm of v; cs = np != 0 ? dot / np : 0.0; sim = 1.0 * cs * min(n, cap) / cap.
 * Rules, in this order: (1) the candidates; (2) with XMAP_PEERS_SAME (the query CSR is the resident CSR) v == query_user[q]
 *   leaves unless XMAP_PEERS_KEEP_SELF; (3) the ids of the query's exclusion list leave; (4) the rest is intersected with
 *   F->allow -- the mask and the ids are USERS, one exclusion list per query, and the mask acts in the expansion: no record of an
 *   ineligible user is written; (5) n < min_common: dropped, counted; (6) sim; non-finite: dropped, counted; (7) sim < F->min_score:
 *   dropped, counted; (8) selection by sim descending as numbers, user index ascending on equal sim.  F == NULL: no rules.
 * Outputs (device): out_cnt [n_query]; out_user / out_sim / out_common [n_query][n_top] with -1 / 0.0 / 0 behind the count;
 *   out_common = n of the entry.  1 <= n_top <= 1024, cap >= 1 (cap = 1 returns cs), min_common >= 1, n_users < 2^31.  A query
 *   user outside the query CSR or without valid rows gets count 0; queries may repeat.  A pure function of the inputs: it depends
 *   on neither the grid, nor the order of any atomic, nor max_records.
 * h_stats (host, [6] or NULL): [0] candidates after rules 2-4, [1] dropped by min_common, [2] dropped as non-finite, [3] dropped
 *   below the floor, [4] the largest candidate count (after rules 2-4) of one query, [5] records expanded.
 * xmap_peer_index: hd_ptr [n_items + 1], hd_user / hd_x [n_rows] (n_rows = prof_ptr[n_users] < 2^31; the entries behind
 *   hd_ptr[n_items] are not part of the index), nrm [n_users]; *h_rows = rows indexed = hd_ptr[n_items].  The transposition is a
 *   stable sort of the row indices by item.  Temporaries: 24 B per profile row.  Syncs.
 * xmap_peer_rows: the queries index the CSR q_ptr / q_item / q_rating of n_q_users users (the resident profiles, or a fold-in
 *   batch); centre must be the one the index was built with.  The queries are cut into chunks of consecutive queries whose records
 *   number at most max_records (0: the library's default, 2^22); a single query above that is a chunk of its own and its records
 *   must stay below 2^31 (XMAP_ERR_CAPACITY).  Per chunk: record counts per query row -> scan -> expansion (one thread per record)
 *   -> stable radix sort on (q - q0) << user_bits | v -> run heads -> scan -> one lane per run -> segmented selection.
 *   Temporaries from the stream's arena: 64 B per record of the largest chunk (48 B per record + 16 B per run, sized for as many runs as records).  n_top, cap, min_common, flags and
 *   a NaN floor are checked on the host before any device work, the pointers too; ex_ptr and the row count of the queries on the
 *   device, before an output is written.  max_records above 2^31 - 2 counts as 2^31 - 2.  Syncs.
 * xmap_peer_centre: centre[i] = the average of hd_x over the holders of item i (0.0 without holders) of an index built with
 *   centre == NULL -- the double-double sum (exact to 2^-104) rounded once, divided by the entries, as RecommenderSim takes its item averages
 *   (xmap_ctx_rec_download's item_avg) -- so a caller centres without a RecommenderSim pass: index without centre, this call,
 *   index with it.  hd_x may be NULL iff no row is indexed.  One wave per item.  Does not sync.
 * Launches: every kernel that takes one wave or one block per user, query, query row or item is launched in ranges below 2^32
 *   threads, so the sizes are bounded as stated -- n_users < 2^31, profile rows < 2^31, n_query <= 2^28, query rows of
 *   one call < 2^31, records of one query < 2^31 - 1 -- and by memory, not by a grid. */
#define XMAP_PEERS_SAME 1
#define XMAP_PEERS_KEEP_SELF 2
#define XMAP_PEERS_CENTRED 4    /* xmap_ctx_peers only: centre by the context's item averages */
int xmap_peer_index(void *stream, int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                    const double *prof_rating, const double *centre /*[I] or NULL*/, int64_t *hd_ptr /*[I+1]*/, int32_t *hd_user,
                    double *hd_x /*[n_rows]*/, double *nrm /*[n_users]*/, int64_t *h_rows /*host, may be NULL*/);
int xmap_peer_centre(void *stream, int32_t n_items, const int64_t *hd_ptr, const double *hd_x, double *centre /*[I]*/);
int xmap_peer_rows(void *stream, int64_t n_query, const int32_t *query_user, int64_t n_q_users, const int64_t *q_ptr,
                   const int32_t *q_item, const double *q_rating, int32_t flags, int32_t n_top, int32_t cap, int32_t min_common,
                   int64_t n_users, int32_t n_items, const double *centre, const int64_t *hd_ptr, const int32_t *hd_user,
                   const double *hd_x, const double *nrm, int64_t max_records /*0: library default*/, int32_t *out_cnt,
                   int32_t *out_user, double *out_sim, int32_t *out_common,
                   const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [6] or NULL */);
/* xmap_peer_rows_ls: xmap_peer_rows plus the LOCAL SENSITIVITY of every returned entry -- the second half of the reference's
 * ((id1, id2), [sim, LS]) record of a user method (cosine_user), by which the private perturbation scales its noise.  out_cnt /
 * out_user / out_sim / out_common and h_stats are the bytes xmap_peer_rows writes for the same inputs; rules, chunking, masks,
 * exclusions, floor, fold-in queries and flags are unchanged.  For a returned entry (q, v) with its n records in record order,
 * record t made of a_t = the x of the query's row and b_t = the x of the holder's row, inner = the entry's dot, nx = the query's
 * nrm, ny = nrm[v]; per record, one rounded fp64 operation per step, no fused multiply-add:
 *   rest = inner - a_t * b_t;  m1 = sqrt((nx * nx - a_t * a_t) * (ny * ny));  m2 = sqrt((nx * nx) * (ny * ny - b_t * b_t));
 *   d1 = |w(m1 != 0 ? 1.0 * rest / m1 : 0.0) - sim|, d2 likewise with m2, w(c) = 1.0 * c * min(n - 1, cap) / cap
 * out_ls [n_query][n_top] = the largest d over the records, a NaN above everything (a maximum of bit patterns: no order of
 * evaluation enters); 0.0 behind the count.  An entry of one record has ls = |sim|.  It depends on neither the grid, nor the
 * chunking, nor max_records.  The expansion writes the two factors instead of their product and the reduce multiplies them (the
 * same bits); the sensitivity is taken for the returned entries only, one wave per entry, which finds its run by bisection.
 * Temporaries: 80 B per record of the largest chunk instead of 64 B (the second factor, and the dot of every run).  The host
 * checks of xmap_peer_rows; out_ls == NULL is XMAP_ERR_ARG before any device work.  Syncs. */
int xmap_peer_rows_ls(void *stream, int64_t n_query, const int32_t *query_user, int64_t n_q_users, const int64_t *q_ptr,
                      const int32_t *q_item, const double *q_rating, int32_t flags, int32_t n_top, int32_t cap, int32_t min_common,
                      int64_t n_users, int32_t n_items, const double *centre, const int64_t *hd_ptr, const int32_t *hd_user,
                      const double *hd_x, const double *nrm, int64_t max_records /*0: library default*/, int32_t *out_cnt,
                      int32_t *out_user, double *out_sim, int32_t *out_common, double *out_ls /*[n_query][n_top], 0.0 behind the count*/,
                      const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [6] or NULL */);

/* ---- user-kNN (csrc/stage_e_uknn.hip; DESIGN.md 4 "User-kNN"): "people like you rated this highly" -- predictions and top-N
 * lists from the peer lists of xmap_peer_rows.  The reference's user_based_prediction restated.  All arithmetic is fp64, one
 * rounded operation per step, no fused multiply-add.
 * A profile row p is VALID iff 0 <= prof_item[p] < n_items; invalid rows are ignored everywhere.
 * Lists: n_query lists in the layout xmap_peer_rows writes -- nb_cnt [n_query] (<= 0: the query has no list), nb_user / nb_sim
 *   [n_query][n_nb], 1 <= n_nb <= 1024; the list of q is its first min(nb_cnt[q], n_nb) entries (v_j, s_j), j in list order.  An
 *   entry whose v_j is outside [0, n_users) is a neighbour without rows.  query_avg [n_query] = the mean of the QUERY user, given
 *   beside the lists so that a folded-in query (not a resident user) works; user_avg [n_users] = the resident means (read with
 *   XMAP_UKNN_OWN_MEAN only, may be NULL without it).
 * Evidence of (q, i): for each neighbour j in list order, each row p of v_j's profile with prof_item[p] == i in profile order
 *   is the entry (s_j, d), d = prof_rating[p] - query_avg[q]; with XMAP_UKNN_OWN_MEAN d = prof_rating[p] - user_avg[v_j]
 *   (Resnick's formula; flags 0 is the reference's, which subtracts the QUERY's mean).  A neighbour that holds i twice gives two
 *   entries; there is no cap.  num = the sum of fl(s_j * d), den = the sum of |s_j|, both from 0.0 left to right in entry order.
 *   score = query_avg[q] + num / den; without evidence score = query_avg[q].  No temporal decay.
 * xmap_uknn_means: user_avg[u] = the mean over the valid rows of user u: the double-double sum (exact to 2^-104) rounded once,
 *   divided by the count, as RecommenderSim takes its item averages and xmap_peer_centre its centre (lane l of 64 sums the rows
 *   l, l + 64, .. of the profile, the fixed butterfly of dd_reduce folds the lanes); user_cnt[u] = the valid rows.  A user
 *   without valid rows gets 0.0 and 0.  One wave per user, launched in ranges below 2^32 threads.  n_users < 2^31.  Does not sync.
 * xmap_uknn_predict_rows: one wave per test pair t = (test_q[t], test_item[t]); test_q indexes the lists.  status[t]: 3 = test_q
 *   outside [0, n_query) or test_item outside [0, n_items); else 1 = nb_cnt[q] <= 0 (the reference skips the user's pairs, and
 *   calculate_mae does not count them); else 2 = the Python statement raises here (evidence with den == 0.0, or a score that is
 *   not finite); else 0 = predicted, with or without evidence.  out_score[t] = the score, out_bound[t] = bound_rating of it
 *   (round half up, clamp to [0, 5]), both 0.0 unless status is 0; out_n[t] = the evidence entries (0 for status 1 and 3).
 *   The sums do not depend on the grid.  The MAE of the call is xmap_mae(status, real, out_bound, out_bound).  Launched in ranges
 *   below 2^32 threads; no temporaries.  Does not sync.
 * xmap_uknn_topn_rows: per query q the n_top (1..1024) items its neighbours hold, ranked by the unrounded score.  Records of q:
 *   for each neighbour j in list order, each valid row of v_j in profile order, the record (item, s_j, d).  Rules, in this
 *   order: (1) the candidates are the items with at least one record; (2) the items query_user[q] holds in the query CSR q_ptr /
 *   q_item of n_q_users users (any row with that item; a query user outside the CSR holds nothing) leave unless
 *   XMAP_UKNN_KEEP_HELD; (3) the ids of the query's exclusion list leave, and the rest is intersected with F->allow -- the mask
 *   and the ids are ITEMS, one exclusion list per query, and the mask acts in the expansion: no record of an ineligible item is
 *   written; (4) support = the records of the item; support < min_support (>= 1): dropped, counted; (5) the score as above over
 *   the item's records in record order; not finite (den == 0.0 among them): dropped, counted; (6) score < F->min_score: dropped,
 *   counted; (7) selection by score descending as numbers, item index ascending on equal scores.  F == NULL: no rules.
 *   Outputs (device): out_cnt [n_query]; out_item / out_score / out_support [n_query][n_top] with -1 / 0.0 / 0 behind the count.
 *   Queries may repeat.  A pure function of the inputs: it depends on neither the grid, nor the order of any atomic, nor
 *   max_records.  h_stats (host, [6] or NULL): [0] candidates after rules 2-3, [1] dropped by min_support, [2] dropped as
 *   non-finite, [3] dropped below the floor, [4] the largest candidate count (after rules 2-3) of one query, [5] records expanded.
 *   The queries are cut into chunks of consecutive queries whose records number at most max_records (0: the library's default,
 *   2^22); a single query above that is a chunk of its own and its records must stay below 2^31 (XMAP_ERR_CAPACITY).  Per chunk:
 *   record counts per (query, list position) -> scan -> expansion (one wave per position compacts its rows) -> stable radix sort
 *   on (q - q0) << item_bits | item -> run heads -> scan -> one lane per run -> segmented selection.  Temporaries from the
 *   stream's arena: 72 B per record of the largest chunk (56 B per record + 16 B per run, sized for as many runs as records) and
 *   12 B per (query, list position); n_query * n_nb < 2^31, n_query <= 2^28.  n_top, n_nb, min_support, flags, a NaN floor and
 *   the pointers are checked on the host before any device work; ex_ptr and the record counts on the device, before an output is
 *   written.  max_records above 2^31 - 2 counts as 2^31 - 2.  Syncs. */
#define XMAP_UKNN_OWN_MEAN 1
#define XMAP_UKNN_KEEP_HELD 2   /* xmap_uknn_topn_rows / xmap_ctx_uknn_recommend only */
int xmap_uknn_means(void *stream, int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                    const double *prof_rating, double *user_avg /*[U]*/, int32_t *user_cnt /*[U]*/);
int xmap_uknn_predict_rows(void *stream, int64_t n_test, const int32_t *test_q, const int32_t *test_item, int64_t n_query,
                           const double *query_avg, int32_t n_nb, const int32_t *nb_cnt, const int32_t *nb_user, const double *nb_sim,
                           int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                           const double *prof_rating, const double *user_avg /*[U] or NULL*/, int32_t flags, double *out_score,
                           double *out_bound, int32_t *out_n, int32_t *status);
int xmap_uknn_topn_rows(void *stream, int64_t n_query, const int32_t *query_user, int64_t n_q_users, const int64_t *q_ptr,
                        const int32_t *q_item, const double *query_avg, int32_t n_nb, const int32_t *nb_cnt, const int32_t *nb_user,
                        const double *nb_sim, int64_t n_users, int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item,
                        const double *prof_rating, const double *user_avg /*[U] or NULL*/, int32_t flags, int32_t n_top,
                        int32_t min_support, int64_t max_records /*0: library default*/, int32_t *out_cnt, int32_t *out_item,
                        double *out_score, int32_t *out_support,
                        const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [6] or NULL */);

/* ---- related items (csrc/stage_e_related.hip; DESIGN.md 4 "Related items"): "what goes with these items" -- the n_top items most
 * related to a SET of items (a cart, an anonymous session, "more like this"), read off the rows of the RecommenderSim CSR.  No
 * user and no rating takes part.  Merging per-member neighbour lists on the host cannot do this: the cut is per member (an item
 * that is eleventh for every member and first for the basket is in nobody's list).  All arithmetic is fp64, one rounded operation
 * per step, no fused multiply-add.
 * The matrix: the RecommenderSim CSR as xmap_sim2_scatter leaves it (row_ptr [n_items + 1], col / sim): rows in storage order,
 *   not sorted; a row may hold a column twice and may hold its own index; resident, trusted, read only; a row holds fewer than
 *   2^31 - 1 entries.  An entry whose column is outside [0, n_items) is ignored.
 * The baskets: a CSR of n_query baskets, b_ptr [n_query + 1] (b_ptr[0] = 0, non-decreasing), b_item [b_ptr[n_query]], b_weight
 *   beside it or NULL.  A member outside [0, n_items) is a member without a row; a repeated member counts once per occurrence;
 *   an empty basket is valid.
 * Records of query q: for each basket position p in order whose member b is valid, each entry e of row b in storage order, the
 *   record (item = col[e], v = fl(b_weight[p] * sim[e])); b_weight == NULL: v = sim[e], nothing is multiplied.
 * Rules, in this order: (1) the candidates are the items with at least one record; (2) the basket's own valid members leave
 *   unless XMAP_RELATED_KEEP_MEMBERS; (3) the ids of the query's exclusion list leave, and the rest is intersected with F->allow
 *   -- the mask and the ids are ITEMS, one exclusion list per query, and both act in the expansion: no record of an ineligible
 *   item is written; (4) support = the records of the item; support < min_support (>= 1): dropped, counted; (5) the score over
 *   the item's records in record order -- XMAP_RELATED_SUM: from 0.0 left to right; XMAP_RELATED_MEAN: that sum / (double)support;
 *   XMAP_RELATED_MAX: the largest v as numbers, the first occurrence's bits among equals, NaN if any v is NaN; (6) a score that
 *   is not finite: dropped, counted; (7) score < F->min_score: dropped, counted; (8) selection by score descending as numbers,
 *   item index ascending on equal scores.  F == NULL: no rules.
 * Outputs (device): out_cnt [n_query]; out_item / out_score / out_support [n_query][n_top] with -1 / 0.0 / 0 behind the count;
 *   1 <= n_top <= 1024.  Queries may repeat.  A pure function of the inputs: it depends on neither the grid, nor the order of
 *   any atomic, nor max_records.  h_stats (host, [6] or NULL): [0] candidates after rules 2-3, [1] dropped by min_support, [2]
 *   dropped as non-finite, [3] dropped below the floor, [4] the largest candidate count (after rules 2-3) of one query, [5]
 *   records expanded (the records of the items rule 3 lets through, members' included; the markers below are not counted).
 * The queries are cut into chunks of consecutive queries whose records number at most max_records (0: the library's default,
 *   2^22); a single query above that is a chunk of its own and its records must stay below 2^31 (XMAP_ERR_CAPACITY).  Per chunk:
 *   record counts per basket position -> scan -> expansion (one wave per position compacts the member's row under the mask and
 *   the exclusion list) -> stable radix sort on (q - q0) << item_bits | item -> run heads -> scan -> one lane per run ->
 *   segmented selection.  Rule 2 takes no second walk: every valid position also emits one MARKER record for its own item, which
 *   sorts into that item's run and makes the run no candidate; markers count towards a chunk's size only.  Temporaries from the
 *   stream's arena: 64 B per record of the largest chunk (48 B per record + 16 B per run, sized for as many runs as records),
 *   12 B per basket position and 8 B per query; n_query <= 2^28.  n_top, how, flags, min_support, a NaN floor and the pointers
 *   are checked on the host before any device work; b_ptr, ex_ptr (the error names the first bad position) and the record
 *   counts on the device, before anything is indexed through the tables or an output is written.  max_records above 2^31 - 2
 *   counts as 2^31 - 2.  The exclusion list of a query is walked whole for every row entry of its members, in the count pass
 *   and in the expansion (row length * list length steps per basket position): meant for short lists.  Syncs. */
#define XMAP_RELATED_SUM 0
#define XMAP_RELATED_MEAN 1
#define XMAP_RELATED_MAX 2
#define XMAP_RELATED_KEEP_MEMBERS 1
int xmap_related_rows(void *stream, int64_t n_query, const int64_t *b_ptr /*[n_query+1]*/, const int32_t *b_item,
                      const double *b_weight /* or NULL: every weight 1.0, and no multiplication is performed */,
                      int32_t n_items, const int64_t *row_ptr /*[I+1]*/, const int32_t *col, const double *sim,
                      int32_t how, int32_t flags, int32_t n_top, int32_t min_support, int64_t max_records /*0: library default*/,
                      int32_t *out_cnt, int32_t *out_item, double *out_score, int32_t *out_support,
                      const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [6] or NULL */);

/* ---- fused lists (csrc/stage_e_fuse.hip; DESIGN.md 4 "Fused lists"): several lists of the same queries -- item-kNN, user-kNN,
 * related items, one list per source domain -- become one list per query, by rank (reciprocal rank fusion) or by score (weighted
 * sum, weighted mean).  All arithmetic is fp64, one rounded operation per step, no fused multiply-add; the divisions are IEEE.
 * The lists: n_lists (1 .. XMAP_FUSE_MAX_LISTS) of xmap_fuse_list, a host array with device pointers inside: cnt [n_query], item
 *   [n_query][width], score beside it (may be NULL with XMAP_FUSE_RRF), width in 1 .. 1024 (the row stride), weight finite, any
 *   sign.  Row q of every list belongs to the same query.  The ids are just ids in [0, n_ids): items for top-N lists, users for
 *   audiences or peers.  Lists may alias each other; outputs may not alias inputs.
 * Records of query q: for l = 0 .. n_lists - 1, for r = 0 .. m - 1 with m = min(max(cnt_l[q], 0), width_l): if id = item_l[q][r]
 *   lies in [0, n_ids), the record (id, l, r).  An id a list holds twice gives two records.
 * Term of a record: XMAP_FUSE_RRF: t = w_l / (rrf_c + (double)(r + 1)); XMAP_FUSE_SUM and XMAP_FUSE_MEAN: t = fl(w_l * score_l[q][r]).
 * Score of an id, over its records in record order (l ascending, then r ascending): num from 0.0 left to right over t, den from
 *   0.0 left to right over w_l, mask |= 1 << l.  RRF and SUM give num, MEAN gives num / den.
 * Rules, in this order: (1) the candidates are the ids with a record; (2) popcount(mask) < min_lists (1 .. n_lists): dropped,
 *   counted; (3) a score that is not finite (an inf or NaN input score, den == 0.0): dropped, counted; (4) selection by score
 *   descending as numbers (-0.0 equals 0.0), id ascending on equal scores.
 * Outputs (device): out_cnt [n_query]; out_id / out_score / out_lists [n_query][n_top] hold the id, the score's own bits and the
 *   mask, with -1 / 0.0 / 0 behind the count; 1 <= n_top <= 1024.  h_stats (host, [5] or NULL): [0] candidates, [1] dropped by
 *   min_lists, [2] dropped as non-finite, [3] the largest candidate count of one query, [4] records.  A pure function of the
 *   inputs: it depends on neither the grid, nor the chunking, nor which of the two routes below ran.
 * Two routes, chosen from W = the sum of the widths alone:
 *   W <= XMAP_FUSE_BLOCK_RECORDS: one workgroup per query, launched in ranges below 2^32 threads, keeps the query's records in
 *     LDS from the first load to the selected list: keys id << 14 | l << 10 | r (distinct, so the bitonic network sorts them
 *     stably), run heads by comparing neighbours, the head lane walks its run, a second network on (score key, position).  The
 *     networks span the power of two at or above the entries the query offers (at least 128), whatever the widths.  No global
 *     temporaries, no host decision between load and store.
 *   otherwise: record counts per (query, list) -> scan -> chunks of consecutive queries of at most max_records records (0: the
 *     library's default, 2^22; a single query above that is a chunk of its own) -> expansion in (l, r) order -> stable radix sort
 *     on (q - q0) << id_bits | id -> run heads -> scan -> one lane per run -> segmented selection.  Temporaries from the stream's
 *     arena: 56 B per record of the largest chunk, 12 B per (query, list) and 8 B per query.
 * n_lists, every width, weight and pointer, how, rrf_c (finite, >= 0), min_lists, n_top, n_ids, max_records and n_query (<= 2^28)
 *   are checked on the host before any device work, each check naming its argument: on XMAP_ERR_ARG nothing is written.  Syncs. */
#define XMAP_FUSE_RRF 0
#define XMAP_FUSE_SUM 1
#define XMAP_FUSE_MEAN 2
#define XMAP_FUSE_MAX_LISTS 16
#define XMAP_FUSE_BLOCK_RECORDS 2048
typedef struct {
    const int32_t *cnt;       /* [n_query] */
    const int32_t *item;      /* [n_query][width] */
    const double *score;      /* [n_query][width]; may be NULL with XMAP_FUSE_RRF */
    int32_t width;            /* 1 .. 1024: the row stride */
    double weight;            /* finite, any sign */
} xmap_fuse_list;
int xmap_fuse_rows(void *stream, int64_t n_query, int32_t n_lists, const xmap_fuse_list *lists /* host array, device pointers inside */,
                   int32_t n_ids, int32_t how, double rrf_c, int32_t min_lists, int32_t n_top, int64_t max_records /*0: library default*/,
                   int32_t *out_cnt, int32_t *out_id, double *out_score, int32_t *out_lists, int64_t *h_stats /* host, [5] or NULL */);

/* ---- shelves (csrc/stage_e_shelf.hip; DESIGN.md 4 "Shelves"): a page of shelves -- a top-N per LABEL of the items ("Top picks in
 * Cookery") and the best shelves of this user -- in one call.  No returned list can be cut into shelves: the cut of every other call
 * is inside the kernel, a user's fifth-best cookery book may be candidate number 300.
 * Labels: a CSR over the item space, lab_ptr int64 [n_items + 1], lab_id int32 [lab_ptr[n_items]], ids in [0, n_labels), 1 <=
 *   n_labels <= XMAP_SHELF_MAX_LABELS.  Checked on the device before any other work: lab_ptr[0] == 0; lab_ptr non-decreasing; every
 *   id in range; the labels of ONE item strictly ascending (so a label stands once per item).  A table that fails: XMAP_ERR_ARG, the
 *   message names the rule and the first offending index, nothing is read through the table, the outputs keep every byte.  An item
 *   with no label is on no shelf.  lab_allow: a bitmap over the LABELS in the bit order of xmap_rec_filter.allow ((n_labels + 31) /
 *   32 words; NULL: every label): which labels may form a shelf ("genre" labels may, "format" labels of the same table may not).
 * Candidates and scores: for query q the kept candidates C_q are exactly steps (1)-(7) of xmap_topn_rows_filtered (candidates, held
 *   items unless XMAP_TOPN_KEEP_HELD, the query's exclusion list, F->allow, scoring, status-2 drops, the floor on the rank_by score);
 *   the scores are the same bits.
 * A shelf (q, l), l an allowed label: the members of C_q whose item carries l, ranked by the rank_by score descending as numbers
 *   (-0.0 equals 0.0), item index ascending on equal scores.  size = the members, cnt = min(size, n_top), the content = the first cnt
 *   entries.  A shelf with size < min_fill (min_fill >= 1) is not formed; it is counted.
 * The shelf's score and the order of the shelves, by shelf_by:
 *   XMAP_SHELF_BY_BEST  : the rank_by score of entry 0, its bits; score descending as numbers, label ascending on equal scores
 *   XMAP_SHELF_BY_MEAN  : (((s_0 + s_1) + ...) + s_{cnt-1}) / (double)cnt over the RETURNED entries in rank order, fp64, starting
 *                         from s_0, one division, no fused multiply-add; order as BEST
 *   XMAP_SHELF_BY_LABEL : the score of BEST; label ascending (a page with a fixed layout)
 *   The first n_shelf shelves in that order are returned.
 * Limits: 1 <= n_shelf <= 64, 1 <= n_top <= 64, rank_by 0 or 1, flags: XMAP_TOPN_KEEP_HELD only.  The status-0 scores are finite
 *   (the scoring pass guarantees it; for xmap_shelf_segments a precondition: no order is promised for a NaN).
 * Outputs (device): out_nshelf [Q]; out_label [Q][n_shelf] (-1 behind the count); out_sscore [Q][n_shelf] (0.0 behind); out_size
 *   [Q][n_shelf]: the WHOLE shelf's size, the "see all 212" number (0 behind); out_cnt [Q][n_shelf] (0 behind); out_item / out_plain
 *   / out_decay [Q][n_shelf][n_top]: -1 / 0.0 / 0.0 behind a shelf's count and for the shelves behind out_nshelf.  The slice [q][s]
 *   has the layout of a row of xmap_topn_rows: out_cnt, out_item, out_plain, out_decay viewed as [Q * n_shelf] and [Q * n_shelf]
 *   [n_top] are a pool for xmap_diversify_rows and a list for xmap_fuse_rows, unchanged.
 * A query user outside the users, or one without rows, has 0 shelves.  Queries may repeat.  The result is a pure function of the
 *   inputs: it depends on no grid, no atomic order and no chunking (no floating-point atomic, no lock).
 * xmap_shelf_segments: the back half on its own, over scored segments in the layout the candidate-and-scoring half of a top-N
 *   call leaves: cand_ptr [Q + 1] (checked on the device like the other pointer tables), and per candidate cand_item (ascending
 *   within a segment, each once; an item outside [0, n_items) carries no label), plain, decay, status.  A candidate is kept iff
 *   status == 0 and its rank_by score is >= min_score (-INFINITY: no floor; NaN: XMAP_ERR_ARG).  For callers with other scored
 *   segments (user-kNN candidates, say).  h_stats (host, [4] or NULL) = [6..9] below.
 * xmap_shelf_rows: the arguments of xmap_topn_rows_filtered up to n_w, then the labels, n_shelf, shelf_by, min_fill, max_records,
 *   the outputs, F and h_stats (host, [10] or NULL): [0..5] as xmap_topn_rows_filtered; [6] (candidate, allowed label) records; [7]
 *   shelves with size >= 1; [8] of those, the shelves below min_fill; [9] the largest number of formed shelves of one query.
 * max_records: the records sorted at a time, in chunks of consecutive queries (a single query above it is a chunk of its own); 0:
 *   the library's default 2^22; the result does not depend on it.  Temporaries: 12 B per candidate, 48 B per record of a chunk, 8
 *   + 4 n_shelf B per query -- never records x n_top: the chosen shelves are selected twice instead. */
#define XMAP_SHELF_BY_BEST 0
#define XMAP_SHELF_BY_MEAN 1
#define XMAP_SHELF_BY_LABEL 2
#define XMAP_SHELF_MAX_LABELS 16777216
int xmap_shelf_segments(void *stream, int64_t n_query, const int64_t *cand_ptr /*[n_query+1]*/, const int32_t *cand_item,
                        const double *plain, const double *decay, const int32_t *status, double min_score, int32_t n_items,
                        int32_t n_labels, const int64_t *lab_ptr /*[n_items+1]*/, const int32_t *lab_id,
                        const uint32_t *lab_allow /* or NULL */, int32_t n_shelf, int32_t n_top, int32_t rank_by, int32_t shelf_by,
                        int32_t min_fill, int64_t max_records /*0: library default*/, int32_t *out_nshelf, int32_t *out_label,
                        double *out_sscore, int32_t *out_size, int32_t *out_cnt, int32_t *out_item, double *out_plain,
                        double *out_decay, int64_t *h_stats /* host, [4] or NULL */);
int xmap_shelf_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                    int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim,
                    const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time,
                    const double *item_avg, const double *wtab, int32_t n_w, int32_t n_labels, const int64_t *lab_ptr /*[n_items+1]*/,
                    const int32_t *lab_id, const uint32_t *lab_allow /* or NULL */, int32_t n_shelf, int32_t shelf_by,
                    int32_t min_fill, int64_t max_records /*0: library default*/, int32_t *out_nshelf, int32_t *out_label,
                    double *out_sscore, int32_t *out_size, int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay,
                    const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [10] or NULL */);

/* ---- label quotas and calibrated lists (csrc/stage_e_quota.hip; DESIGN.md 4 "Quotas and calibrated lists"): ONE list with a
 * guaranteed mix of labels -- "at most two cookery books in my top ten" (caps), "a 70 % crime / 30 % history reader gets a 70 / 30
 * list" (seat shares).  No returned list can be re-cut on the host: the cut of every other call is inside the kernel, the third
 * admissible cookery book of a crime reader may be candidate number 300.
 * Labels: the table of the shelves (lab_ptr, lab_id, n_labels), checked on the device by the same rules with the same messages; a
 *   table that fails: XMAP_ERR_ARG, the outputs keep every byte.  GOVERNED labels: those lab_allow admits (a bitmap over the labels
 *   in the bit order of xmap_rec_filter.allow; NULL: every label).  An ungoverned label is invisible to everything below.
 * Pool of query q: the positions j = 0 .. m - 1 in the caller's order, m = clamp(in_cnt[q], 0, n_pool); position is rank, nothing is
 *   sorted again.  L(j) = the governed labels of in_item[q][j]; an item outside [0, n_items) carries none; the same item at two
 *   positions counts as two independent positions.
 * Limits: 1 <= n_top <= n_pool <= XMAP_QUOTA_MAX_POOL; rank_by 0 or 1; 1 <= n_labels <= XMAP_SHELF_MAX_LABELS; n_pool * (the longest
 *   label row of the WHOLE table, one integer max-reduction beside the table check) <= XMAP_QUOTA_MAX_RECORDS, else XMAP_ERR_ARG
 *   naming n_pool, the longest label row and the limit -- a property of the table, not of a query: no call fails for some queries.
 * mode XMAP_QUOTA_CAP: cap(l) = lab_cap[l] (device int32 [n_labels]; a negative entry: XMAP_ERR_ARG naming the first such label,
 *   checked on the device before any other work; 0 bars the label; INT32_MAX is no cap), or the scalar cap >= 1 where lab_cap is NULL.
 *     taken[*] = 0; r = 0
 *     for j = 0 .. m-1 while r < n_top:
 *         if every l in L(j) has taken[l] < cap(l):  out[r] = position j; taken[l] += 1 for every l in L(j); r += 1
 *         else: refused += 1
 *     out_cnt = r
 *   A position without governed labels is always accepted; a position refused because label A is full consumes nothing of its label B.
 * mode XMAP_QUOTA_SHARE: calibrated by Sainte-Lague seats.  Weights w[l], uint32 < 2^31 (a precondition): lab_weight (device
 *   [n_labels], one editorial mix for all queries), or, where it is NULL, the query user's own history: w[l] = the rows of the
 *   user's profile (prof_ptr / prof_item; nothing else of the profile is read) whose item carries governed label l -- a row held
 *   twice counts twice, an item outside the table nothing, a query user outside [0, n_users) or without rows has all-zero weights.
 *     s[*] = 0; left = {0 .. m-1}; n = min(m, n_top)
 *     for r = 0 .. n-1:
 *         E = { governed l : w[l] > 0 and some j in left has l in L(j) }
 *         if E is empty:  j* = min(left); claim = -1                         (off-profile fill, in pool order)
 *         else:  l* = the l of E with the largest w[l] / (2 s[l] + 1), compared exactly: a beats b iff w[a] * (2 s[b] + 1) > w[b] *
 *                (2 s[a] + 1) in 64-bit unsigned products; on equality the smaller label id wins
 *                j* = the smallest j in left with l* in L(j); claim = l*
 *         out[r] = position j*; out_label[r] = claim; left -= {j*}; s[l] += 1 for every l in L(j*)
 *     out_cnt = n
 *   No floating point takes part in either mode; the returned scores are the pool's own bits.
 * Outputs (device, the top-N layout: xmap_diversify_rows up to its 64, xmap_topn_fill_rows and xmap_fuse_rows take them unchanged):
 *   out_cnt [Q]; out_item / out_plain / out_decay [Q][n_top] (-1 / 0.0 / 0.0 behind the count); out_pos [Q][n_top]: the pool position
 *   of each entry (-1 behind); out_label [Q][n_top]: SHARE: the claiming label, -1 for a fill; CAP: the smallest governed label the
 *   item carries, -1 for none; -1 behind the count.
 *   h_stats (host, [4] or NULL; xmap_quota_pool synchronises only when it is given): [0] queries whose list is not the pool's
 *   first min(m, n_top) positions; [1] the sum of out_cnt; [2] CAP: positions refused, SHARE: slots filled with E empty; [3] CAP:
 *   queries with out_cnt < n_top and in_cnt >= n_pool -- the pool cut the list short, the caller should widen it; SHARE: 0.
 * The result is a pure function of the inputs: no grid, no atomic order, no chunking (integer LDS atomics; no floating-point atomic,
 *   no lock).  One workgroup per query; the labels of a pool live in LDS (hence XMAP_QUOTA_MAX_RECORDS).
 * xmap_quota_pool: the back half over any pool in the top-N layout (item-based, user-kNN, group, related lists).  rank_by is kept
 *   for symmetry (checked 0 / 1).  query_user / n_users / prof_ptr / prof_item: read in SHARE mode without lab_weight only.
 * xmap_quota_rows: the whole call.  The arguments of xmap_topn_rows_filtered up to n_w (its n_top is this call's n_top), then
 *   n_pool, the mode arguments, the labels, the outputs, F, h_stats.  The candidates are scored exactly by steps (1)-(7) of
 *   xmap_topn_rows_filtered (the same score bits); the kept candidates of a query are ranked into a pool of n_pool by the rank_by score
 *   descending as numbers (-0.0 equals 0.0), item ascending on equal scores -- for n_pool <= 64 by definition what
 *   xmap_topn_rows_filtered returns with n_top = n_pool -- selected straight into LDS, never written to memory; the back half runs
 *   over it (out_pos: the rank in that pool).  The history of SHARE mode: the profiles of the call.  h_stats (host, [10] or NULL):
 *   [0..5] as xmap_topn_rows_filtered, [6..9] the four above ([9]: the pool was full). */
#define XMAP_QUOTA_CAP 0
#define XMAP_QUOTA_SHARE 1
#define XMAP_QUOTA_MAX_POOL 1024
#define XMAP_QUOTA_MAX_RECORDS 8192
int xmap_quota_pool(void *stream, int64_t n_query, int32_t n_pool, const int32_t *in_cnt, const int32_t *in_item,
                    const double *in_plain, const double *in_decay, int32_t rank_by, int32_t mode, int32_t cap,
                    const int32_t *lab_cap /* device [n_labels], or NULL */, const uint32_t *lab_weight /* device [n_labels], or NULL */,
                    const int32_t *query_user /* SHARE without lab_weight; else may be NULL */, int64_t n_users,
                    const int64_t *prof_ptr, const int32_t *prof_item, int32_t n_items, int32_t n_labels,
                    const int64_t *lab_ptr /*[n_items+1]*/, const int32_t *lab_id, const uint32_t *lab_allow /* or NULL */,
                    int32_t n_top, int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos,
                    int32_t *out_label, int64_t *h_stats /* host, [4] or NULL */);
int xmap_quota_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                    int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim,
                    const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time,
                    const double *item_avg, const double *wtab, int32_t n_w, int32_t n_pool, int32_t mode, int32_t cap,
                    const int32_t *lab_cap /* or NULL */, const uint32_t *lab_weight /* or NULL */, int32_t n_labels,
                    const int64_t *lab_ptr /*[n_items+1]*/, const int32_t *lab_id, const uint32_t *lab_allow /* or NULL */,
                    int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_pos, int32_t *out_label,
                    const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [10] or NULL */);

/* ---- allotment: top-N for many queries under item capacities (csrc/stage_e_allot.hip; DESIGN.md 4 "Allotment"): 500 coupons per
 * title, 40 seats per event, 3 slots per newsletter -- "item i goes to at most cap(i) recipients, recipient q gets at most n_top
 * items".  A constraint ACROSS queries, which no per-query call can honour: recipient-proposing deferred acceptance (Gale-Shapley,
 * many-to-many) over pools that are already on the device.
 * Inputs: Q pools in the top-N layout: in_cnt [Q], in_item / in_plain / in_decay [Q][n_pool]; rank_by 0 (plain) or 1 (decayed).
 * Limits: 1 <= n_top <= n_pool <= XMAP_ALLOT_MAX_POOL and Q * n_pool < 2^31, else XMAP_ERR_ARG naming the argument, checked on the
 *   host before any device work: the outputs keep every byte.
 * Capacities: cap(i) = item_cap[i] (device int32 [n_items]), or the scalar cap >= 1 where item_cap is NULL.  A negative entry:
 *   XMAP_ERR_ARG naming the first such item, found on the device before any other work, the outputs untouched.  0 bars the item;
 *   INT32_MAX is no cap.
 * Definitions: m(q) = clamp(in_cnt[q], 0, n_pool).  Position (q, j) is VOID if j >= m(q), the item is outside [0, n_items), or its
 *   capacity is 0.  The same item at two positions of one pool is two independent positions, as in xmap_quota_pool (the scorers
 *   never produce that).  Query users may repeat: a query is a recipient.
 * Offer order: k(q, j) = (au_key(score), q, j), ascending lexicographically = better first; au_key (csrc/au_select.h) over the bits
 *   of score + 0.0: b = those bits as uint64; au_key = b if its top bit is set, else ~(b | 2^63).  Defined for every bit pattern;
 *   -0.0 equals 0.0; a larger score is better; ties go to the smaller query index, then the smaller position.
 * Outcome: R is the SMALLEST set of refused positions such that the three statements hold together:
 *     the proposals P(q) of each query are its first n_top positions that are neither void nor in R;
 *     the offers of each item i are all proposals holding i;
 *     every offer of i that is not among its cap(i) best by k is in R.
 *   Equivalently: iterate "propose, refuse the excess, add to R" from R = {} until nothing is added; positions never leave R.  Every
 *   query holds its best positions that no item refused, every item the cap best offers it was made: the recipient-optimal stable
 *   assignment.  R is the least fixed point of a monotone operator, so every schedule of rounds reaches it: the outcome is a pure
 *   function of the inputs.  No floating-point arithmetic takes part after au_key; the returned scores are the pool's own bits.
 * Outputs (device, the top-N layout: xmap_topn_fill_rows, xmap_fuse_rows and xmap_quota_pool take them unchanged, xmap_diversify_rows
 *   up to its 64): out_cnt[q] = |P(q)|; out_item / out_plain / out_decay / out_pos [Q][n_top] hold P(q) in ascending position (out_pos:
 *   the pool position), -1 / 0.0 / 0.0 / -1 behind the count.  item_taken (device int32 [n_items], or NULL): the offers each item
 *   holds.  A caller serving users in batches passes cap - taken to the next batch; BATCHING CHANGES THE OUTCOME: the batches are
 *   not one market (an early batch keeps seats that better offers of a later batch would have won).
 *   h_stats (host [6], or NULL; the call synchronises anyway, it reads a counter per round): [0] queries whose list is not the pool's
 *   first min(m, n_top) positions; [1] the sum of out_cnt; [2] |R|; [3] void positions below m(q); [4] rounds run, the last empty one
 *   included (a property of the schedule, not of the result); [5] queries with out_cnt < n_top and in_cnt >= n_pool (the pool cut
 *   the list short: widen it).
 * Temporaries (the stream's arena): 28 bytes per pool position, 4 per 32 positions of bitmap; every round sorts Q * n_top records of
 *   12 bytes over all queries at once (an item's run crosses any chunking by queries).
 * xmap_allot_pool: the back half over any pool (item-based, user-kNN up to 1 024 wide, group, related, fused lists).
 * xmap_allot_rows: the arguments of xmap_topn_rows_filtered up to n_w -- its n_top is this call's n_pool, hence n_pool <= 64 here --
 *   then n_top, cap, item_cap, the outputs, F, h_stats (host [12], or NULL): [0..5] the filtered call's, [6..11] the six above.  The
 *   pool is by definition what xmap_topn_rows_filtered returns, so the eligibility rules act before the pool is cut. */
#define XMAP_ALLOT_MAX_POOL 1024
int xmap_allot_pool(void *stream, int64_t n_query, int32_t n_pool, const int32_t *in_cnt, const int32_t *in_item,
                    const double *in_plain, const double *in_decay, int32_t rank_by, int32_t n_items, int32_t cap,
                    const int32_t *item_cap /* device [n_items], or NULL */, int32_t n_top, int32_t *out_cnt, int32_t *out_item,
                    double *out_plain, double *out_decay, int32_t *out_pos, int32_t *item_taken /* device [n_items], or NULL */,
                    int64_t *h_stats /* host, [6] or NULL */);
int xmap_allot_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t rank_by, int32_t flags,
                    int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim,
                    const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time,
                    const double *item_avg, const double *wtab, int32_t n_w, int32_t n_top, int32_t cap,
                    const int32_t *item_cap /* device [n_items], or NULL */, int32_t *out_cnt, int32_t *out_item, double *out_plain,
                    double *out_decay, int32_t *out_pos, int32_t *item_taken /* device [n_items], or NULL */,
                    const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [12] or NULL */);

/* ---- popularity fill (csrc/stage_e_fill.hip; DESIGN.md 4 "Popularity fill"): a ranking of the items by popularity, and the
 * completion of short top-N lists with its head.  Every other list of the tail is cut from candidates with evidence; these two
 * calls answer when there is none (a user without rows, a one-rating fold-in, a 1 % mask, the anonymous visitor).
 * xmap_pop_index: the ranking over an index xmap_peer_index built with centre == NULL (hd_x = raw ratings).  Per item i:
 *   n_i = hd_ptr[i + 1] - hd_ptr[i] (a user holding an item twice counts twice, as in the peers); S_i = the double-double sum of
 *   hd_x over the item's holders rounded once (what xmap_peer_centre divides); T = hd_ptr[n_items]; G = the double-double sum of
 *   all indexed hd_x rounded once, taken over the per-item (hi, lo) partials in a fixed shape (one block: thread t of 1024 adds the
 *   items t, t + 1024, ..., then a fixed tree), so its bits depend on no grid; mu = T > 0 ? G / T : 0.0.  Scores, fp64, one rounded
 *   operation per step, no fused multiply-add: XMAP_POP_COUNT: (double)n_i; XMAP_POP_MEAN: (S_i + damping * mu) / ((double)n_i +
 *   damping).  Item i is ranked iff n_i >= min_count and its score is finite; the others are counted into h_counts[1] (below
 *   min_count) and h_counts[2] (non-finite; a non-finite G makes every MEAN score non-finite).  Order: score descending as numbers
 *   (-0.0 equals 0.0), item index ascending on equal scores.  pop_item / pop_score [0 .. ranked) hold the ranking (the score's own
 *   bits), -1 / 0.0 behind it; pop_pos[i] = i's position or -1; h_counts[0] = ranked.  A pure function of the index.  damping
 *   (finite, >= 0), min_count (>= 1) and how are checked before any device work.  One stable radix sort of n_items 64-bit keys
 *   and one pass over the indexed rows; temporaries (48 B per item) from the stream's arena.  Syncs.
 * xmap_topn_fill_rows: completes, in place, lists in the layout xmap_topn_rows, xmap_topn_rows_filtered, xmap_diversify_rows and
 *   xmap_group_topn_rows write (cnt [Q], item / plain / decay [Q][n_top], 1 <= n_top <= 64; cnt outside [0, n_top] counts as the
 *   nearer bound).  The profiles are the CSR the queries index (the resident profiles or a fold-in batch; prof_item only).
 *   n_pop_items = the size of the ranked id space (pop_pos has that many entries); ids in [n_pop_items, n_items) -- the batch items
 *   of an item fold-in -- have no position and are never filled.  Per query q, u = query_user[q], c = cnt[q], L = item[q][0 .. c):
 *     for r in 0 .. n_ranked - 1 while c < n_top:  i = pop_item[r]
 *       skip if i in L (or appended by this loop); skip if not (flags & XMAP_TOPN_KEEP_HELD) and u in [0, n_users) and a row of u
 *       holds i; skip if F and i in ex_id[ex_ptr[q] .. ex_ptr[q + 1]) (ids outside [0, n_items) ignored, repeats allowed); skip if
 *       F and F->allow and bit i of allow is clear;
 *       item[q][c] = i; plain[q][c] = decay[q][c] = item_avg[i]; out_src[q][c] = 1; c += 1
 *     cnt[q] = c; out_src[q][t] = 0 for t < the count on entry, -1 behind the final count.
 *   item_avg[i] is what the model predicts for a pair without evidence.  A list that is full on entry keeps every byte.
 *   F->min_score is a floor on PREDICTIONS: it does not apply to a fill (a NaN floor is still XMAP_ERR_ARG).  The fill knows the
 *   lists, not the scores: an item the scoring pass dropped (status 2, or below the floor) may return as a fill.  A user outside
 *   [0, n_users) holds nothing: such a query is the anonymous visitor, whose list is the eligible head of the ranking.  Queries may
 *   repeat, each with its own exclusion list.  ex_ptr is checked on the device before any output is written, as in the filtered
 *   calls: XMAP_ERR_ARG, the outputs untouched.  A pure function of the inputs.  h_stats (host, [4] or NULL): queries short on
 *   entry, of those filled to n_top, fill entries written, queries still short.
 *   One wave per query walks the ranking XMAP_FILL_WINDOW positions at a time: every skip id is looked up once per window in
 *   pop_pos and marked in an LDS bitmap of the window; a query re-walks only when its skip ids cover a whole window of the head
 *   (at most ceil((need + skip ids) / XMAP_FILL_WINDOW) windows).  With F->allow the ranking is compacted once per call to its
 *   allowed positions (16 B per ranked item + 4 B per item of temporaries), so a sparse mask costs one pass over the items.  Syncs. */
#define XMAP_POP_COUNT 0
#define XMAP_POP_MEAN 1
#define XMAP_FILL_WINDOW 4096
int xmap_pop_index(void *stream, int32_t n_items, const int64_t *hd_ptr /*[I+1]*/, const double *hd_x, int32_t how, double damping,
                   int32_t min_count, int32_t *pop_item /*[I]*/, double *pop_score /*[I]*/, int32_t *pop_pos /*[I]*/,
                   int64_t *h_counts /* host, [3] or NULL: ranked, below min_count, non-finite score */);
int xmap_topn_fill_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t flags, int64_t n_users,
                        int32_t n_items, const int64_t *prof_ptr, const int32_t *prof_item, const double *item_avg, int32_t n_ranked,
                        const int32_t *pop_item, const int32_t *pop_pos, int32_t n_pop_items, int32_t *cnt, int32_t *item,
                        double *plain, double *decay /* in place, [Q] / [Q][n_top] */, int32_t *out_src /*[Q][n_top]*/,
                        const xmap_rec_filter *F /* device pointers inside, or NULL */, int64_t *h_stats /* host, [4] or NULL */);

/* ---- union of AlterEgo rows (csrc/stage_c_union.hip): the rows of D independent two-domain problems -> ONE set of user-major
 * profiles, the reference's alterEgo_profile1.union(alterEgo_profile2) [.distinct()] (code/multidomain_demo.py:128), in the
 * layout xmap_rec_profiles writes -- xmap_sim3_layout (RecommenderSim), xmap_rec_select, xmap_predict_rows, xmap_topn_rows,
 * xmap_topn_eval and xmap_mae take it as they take one domain's profiles.
 * A part = one domain's stage-C output as xmap_alterego_fill leaves it (rows [0, n_target_rows) pass-through, then the mapped
 * rows, both in user order; off_t / off_m [n_users + 1] the exclusive scans the fill pass took; `time` may point at any int64
 * column of n_rows entries to carry instead, e.g. ranks that compare across the parts; `user` is not read) + two maps:
 * user_map [n_users] -> union user, injective within the part; item_map [n_items] -> union item, or -1: rows of that item are
 * dropped.  `parts` is a HOST array of 1 <= n_parts <= 16 descriptors holding device pointers.  n_rows < 2^31 - 1 in all.
 * The rows of union user g, in this order: parts in the order given; within a part the rows of the local user u with
 * user_map[u] = g, its pass-through rows first, then its mapped rows, each in stage-C order (what xmap_rec_profiles gives).
 * flags = XMAP_UNION_DISTINCT: a row is removed if an earlier kept row of the same union user has the same union item, the same
 * time and a rating equal as a number (-0.0 == 0.0; the first occurrence stays, bits included; ratings are finite) --
 * LocalRDD.distinct() over (uid, iid, rating, time) in first-occurrence order.  flags = 0: nothing is removed (plain union).
 * xmap_union_count: FIRST checks every part on the device -- user_map within [0, n_users) and injective, item_map within
 *   [-1, n_items), off_t / off_m starting at 0, non-decreasing and ending at n_target_rows / n_rows - n_target_rows, row items
 *   within [0, the part's n_items) -- and returns XMAP_ERR_ARG (xmap_last_error() names the first bad position) with no output
 *   written and nothing indexed by an unchecked value.  Otherwise prof_ptr [n_users + 1] and h_counts (host) = {rows out, rows
 *   removed as duplicates, rows dropped by item_map == -1, union users with a row}.  Syncs.
 * xmap_union_fill: the rows, into buffers of n_out = h_counts[0] entries (not read when that is 0), with the parts
 *   xmap_union_count accepted and its prof_ptr.  Does not sync.
 * The result is a pure function of the inputs: positions come from counts and scans.  Users of up to 32 rows take a 32-lane
 * group each, up to 2048 rows a block with an LDS hash set, beyond that a block with a hash set in global memory.
 * Temporaries from the stream's arena. */
#define XMAP_UNION_DISTINCT 1
typedef struct xmap_union_part {
    int64_t n_users;            /* users of the part's index space (rows of off_t / off_m, entries of user_map) */
    int32_t n_items;            /* items of the part's index space (entries of item_map) */
    int64_t n_rows, n_target_rows;
    const int32_t *user;        /* [n_rows] not read */
    const int32_t *item;        /* [n_rows] */
    const double *rating;       /* [n_rows] */
    const int64_t *time;        /* [n_rows] */
    const int64_t *off_t;       /* [n_users + 1] */
    const int64_t *off_m;       /* [n_users + 1] */
    const int32_t *user_map;    /* [n_users] */
    const int32_t *item_map;    /* [n_items] */
} xmap_union_part;
int xmap_union_count(void *stream, int32_t n_parts, const xmap_union_part *parts /* host */, int64_t n_users, int32_t n_items,
                     int32_t flags, int64_t *prof_ptr /*[n_users+1]*/,
                     int64_t *h_counts /* host [4]: rows, duplicates removed, rows dropped, users with a row */);
int xmap_union_fill(void *stream, int32_t n_parts, const xmap_union_part *parts /* host */, int64_t n_users, int32_t n_items,
                    int32_t flags, const int64_t *prof_ptr, int64_t n_out, int32_t *prof_item, double *prof_rating,
                    int64_t *prof_time);

/* ==== coarse, handle-based entry points =============================================================
 * What a host in any language binds to replace the three pipelines: plain host buffers in, plain host buffers out,
 * sizes reported by the stage call; the library owns every device buffer, prefix sum, overflow retry and work-unit
 * plan (csrc/api.hip).  All ids are int32 indices into the caller's lexicographically sorted id tables; the four
 * per-item predicate arrays are the string tests of the reference evaluated once per item (xmap/engine/ids.py):
 * prefix_cls (iid[:2] class, baselinerSim.py:191), suffix_cls (iid[-2:] class), contains_mask (bit c: the suffix of
 * class c occurs in the id, extender.py:29-35), flags (bit 0 "S:" in iid, bit 1 "T:" in iid).
 *   xmap_ctx_upload_ratings : trainRDD in index space, CSR by user in trainRDD / profile order      (assist.py:66).  The input
 *                             is checked on the host first (xmap_check_ratings, no repeats allowed): XMAP_ERR_ARG naming the first
 *                             offending position, nothing dropped, allocated or launched -- the context stays as it was, the
 *                             previous upload and its results included.  NaN and +-inf ratings pass
 *   xmap_check_ratings      : that check on its own (host code, O(nnz), one int64 stamp per item; no device, no context):
 *                             user_ptr[0] == 0; user_ptr non-decreasing (a decrease is a negative profile length in every kernel
 *                             of stage A); user_ptr[n_users] < 2^31 - 1; 0 <= item < n_items; no item twice in one profile unless
 *                             allow_repeats (a trainRDD holds one rating per (user, item): remove_invalid; stage A sizes its tables
 *                             for that -- only RecommenderSim's AlterEgo profiles may repeat an item); suffix_cls in [0, 32) (a
 *                             shift count of stage B); prefix_cls >= 0.  prefix_cls / suffix_cls may be NULL (not checked)
 *   xmap_ctx_item_sim       : baseliner_calculate_sim_pipeline (assist.py:66-77) -> n_kept directed pairs kept
 *   xmap_ctx_sim_download   : CSR by first item (row_ptr [I+1], col/sim/mutu/n_ij [n_kept]; rows not sorted), item info
 *                             [I][4], user averages [U]; any pointer may be NULL
 *   xmap_ctx_extend         : extender_pipeline (assist.py:80-102), lazy: per start item the number of candidates and
 *                             the XMAP_TOPC best by (|xsim| desc, end asc); n_out = sum of the candidate counts
 *   xmap_ctx_ext_lists      : the (start, [(end, xsim)*]) lists themselves (xs_off [I], xs_end/xs_val [n_out]): the
 *                             enumeration runs once more into buffers of exactly n_out entries
 *   xmap_ctx_candidates     : n_top[start] = min(candidates, 4): what cross_nonprivate_mapping draws from
 *                             (generator.py:109-110); the caller draws picks[start] in [0, n_top - 1) itself
 *   xmap_ctx_generate       : generator_pipeline (assist.py:136-150): private: arg-max |xsim|; else picks [I];
 *                             choice [I] (or NULL) receives the chosen source item per start (-1: none)
 *   xmap_ctx_gen_download   : AlterEgo rows (user, item, rating fp64, time), pass-through target rows first
 * The recommender tail over those rows, all on the device (call order: generate -> rec_sim -> rec_select or
 * rec_set_neighbors -> predict | recommend | evaluate_topn; any of item_sim / extend / generate / upload drops the tail):
 *   xmap_ctx_rec_sim        : recommender_calculate_sim_pipeline (assist.py:153-177): user-major profiles of the AlterEgo
 *                             rows, then RecommenderSim (cosine branch, cap) -> n_pairs directed pairs, a self pair once
 *   xmap_ctx_rec_profiles_download : the profiles (prof_ptr [U+1], item / rating / time [n_rows]); any pointer may be NULL
 *   xmap_ctx_rec_download   : CSR by first item (row_ptr [I+1]; col / sim / ls / n_ij [n_pairs]; rows not sorted), per-item
 *                             average of the AlterEgo ratings and norm [I]; any pointer may be NULL
 *   xmap_ctx_rec_select     : nonprivate_neighbor_selection (recommenderPrivacy.py:22-35), keep <= 64
 *   xmap_ctx_rec_set_neighbors : neighbour lists made by the host instead (the private selection, perturbed similarities):
 *                             cnt [I], col / sim [I][keep]
 *   xmap_ctx_rec_neighbors_download : cnt [I], col / sim / ls [I][keep] (ls = 0 for host-made lists); NULL = skip
 *   xmap_ctx_predict        : recommender_prediction_pipeline (assist.py:195-207): n_test pairs (user, item); wtab = the
 *                             caller's exp(-alpha d), d = 0 .. n_w - 1; out_plain / out_decay / status [n_test] as
 *                             xmap_predict_rows; test_rating may be NULL, else mae [3] (may be NULL) = {predicted pairs,
 *                             sum |real - plain|, sum |real - decayed|}; *max_now (may be NULL) = table length that serves
 *                             every pair (status 2 pairs of a shorter table: call again with a longer one)
 *   xmap_ctx_recommend      : top-N recommendation (xmap_topn_rows over the resident profiles, lists and averages): host
 *                             arrays in and out; n_query user indices, 1 <= n_top <= 64, rank_by 0 plain / 1 decayed, flags
 *                             0 or XMAP_TOPN_KEEP_HELD; out_cnt [n_query], out_item / out_plain / out_decay [n_query][n_top];
 *                             stats [4] (may be NULL) as h_stats; stats[2] > n_w: call again with a table of that length.
 *                             Needs the same stages as xmap_ctx_predict and is dropped by the same calls
 *   xmap_ctx_evaluate_topn  : hold-out evaluation of the top-N lists (xmap_eval_users -> xmap_topn_rows over eval_user with the
 *                             resident profiles, lists and averages -> xmap_topn_eval): host arrays in and out; the n_test
 *                             pairs (user, item, rating) of xmap_ctx_predict, every (user, item) once; rel_min, n_cut cutoffs
 *                             `cut` and the discounts dtab [n_top] as xmap_topn_eval takes them; n_top, rank_by, flags, wtab,
 *                             n_w as xmap_ctx_recommend.  agg [n_cut][8], cover [n_cut]; user_nrel [U] and user_mask [U] (0
 *                             for a user not evaluated) may be NULL; stats [8] (may be NULL) = the four h_counts of
 *                             xmap_eval_users, then the four h_stats of xmap_topn_rows; stats[6] > n_w: call again with a
 *                             table of that length.  n_test == 0 or no evaluated user: zeroed outputs.  Needs the same
 *                             stages as xmap_ctx_recommend and is dropped by the same calls
 * Fold-in, for profiles that were not rows of the upload (call order: generate -> foldin; rec_sim -> rec_select or
 * rec_set_neighbors before foldin_predict / foldin_recommend, on either side of foldin).  The batch hangs on the replacement
 * map: upload, item_sim, extend and generate drop it; rec_sim, rec_select and rec_set_neighbors leave it.  No fold-in call
 * changes what a resident call returns.
 *   xmap_ctx_foldin         : n_new raw profiles (ptr [n_new + 1], item / rating / time [ptr[n_new]], item indices of the upload)
 *                             -> their AlterEgo profiles (xmap_foldin_count / xmap_foldin_fill with the resident map and flags),
 *                             kept on the device; the batch replaces the previous one.  The input is checked on the host first
 *                             (ptr[0] == 0, ptr non-decreasing, 0 <= item < n_items): XMAP_ERR_ARG naming the position, no device
 *                             work started.  A failed call leaves the context as it was, the previous batch included.  counts
 *                             [3] (may be NULL) = {rows, pass-through rows, profiles with a row}.  n_new == 0 is valid
 *   xmap_ctx_foldin_download : the batch's profiles (prof_ptr [n_new + 1], item / rating / time [rows]); any pointer may be NULL
 *   xmap_ctx_foldin_recommend : xmap_ctx_recommend over the batch: query_user = indices into the batch
 *   xmap_ctx_foldin_predict : xmap_ctx_predict over the batch: test_user = indices into the batch
 *                             (both: an index outside [0, n_new) behaves like a user without rows; they need a batch and the
 *                             neighbour lists)
 * Multi-domain: the union of the AlterEgo rows of n_parts contexts (one two-domain problem each, after xmap_ctx_generate).
 *   xmap_ctx_union          : dst becomes a TAIL-ONLY context over the union (xmap_union_count / xmap_union_fill): n_users union
 *                             users, n_items union items, the profiles of the union in place of stage-C rows.  src [n_parts]
 *                             (1 .. 16): contexts with generated rows on dst's device, read only and unchanged; user_map[d]
 *                             [users of src[d]] / item_map[d] [items of src[d]] (host arrays) as xmap_union_part takes them --
 *                             checked on the device, XMAP_ERR_ARG leaves dst as it was; times are the contexts' own int64 times;
 *                             flags 0 or XMAP_UNION_DISTINCT; counts [4] (may be NULL) as h_counts.  dst holds copies and no
 *                             pointer into a source: destroying a source afterwards is legal.  On dst xmap_ctx_rec_sim,
 *                             _rec_profiles_download, _rec_download, _rec_select, _rec_set_neighbors, _rec_neighbors_download,
 *                             _predict, _recommend and _evaluate_topn work as on a two-domain context; the stage entries,
 *                             xmap_ctx_gen_download and the fold-in entries return XMAP_ERR_ARG.  A later xmap_ctx_union into
 *                             dst or xmap_ctx_upload_ratings drops the union and its tail.  dst may not be one of src
 * Explanations (needs the same stages as xmap_ctx_predict and is dropped by the same calls):
 *   xmap_ctx_explain        : xmap_explain_rows over the resident profiles, lists and averages, and with n_src > 0
 *                             xmap_explain_sources over the upload's own CSR: host arrays in and out.  n_pairs pairs (user,
 *                             item), rank_by 0 / 1, 1 <= n_ev <= 16, 0 <= n_src <= 8, wtab / n_w / *max_now as xmap_ctx_predict;
 *                             ex_status / ex_total / ex_cnt / ex_score [n_pairs], ex_row / ex_slot / ex_share [n_pairs][n_ev];
 *                             ex_row indexes the profiles of xmap_ctx_rec_profiles_download.  n_src > 0: src_total
 *                             [n_pairs][n_ev], src_pos [n_pairs][n_ev][n_src] = positions in the item / rating / time arrays of
 *                             the UPLOAD, which the host holds: it can print "this item, because of these ratings of yours"
 *                             without downloading anything else; n_src == 0: both may be NULL and are not written.  On a union
 *                             context n_src == 0 works (evidence only) and n_src > 0 is XMAP_ERR_ARG: a union has one map and one
 *                             raw profile per part.  n_pairs == 0 is valid.  Argument errors start no device work
 *   xmap_ctx_foldin_explain : the same over the fold-in batch: pair_user = indices into the batch, ex_row indexes the profiles of
 *                             xmap_ctx_foldin_download, src_pos the batch's own item / rating / time arrays (xmap_ctx_foldin
 *                             keeps the batch's raw ptr / item and its pass-through counts on the device, swapped in on success)
 * Audience of an item (needs the same stages as xmap_ctx_recommend and is dropped by the same calls; works on a union context):
 *   xmap_ctx_audience       : xmap_audience_rows over the resident profiles, lists and averages: host arrays in and out;
 *                             n_query item indices, 1 <= n_top <= 1024, rank_by 0 plain / 1 decayed, flags 0 or
 *                             XMAP_AUDIENCE_KEEP_HOLDERS; out_cnt [n_query], out_user / out_plain / out_decay [n_query][n_top];
 *                             stats [4] (may be NULL) as h_stats; stats[2] > n_w: call again with a table of that length.
 *                             Argument errors start no device work and leave the outputs untouched
 *   xmap_ctx_foldin_audience : the same over the fold-in batch: out_user = indices into the batch ("which of the users who
 *                             arrived today"); needs a batch and the neighbour lists, as xmap_ctx_foldin_recommend
 * Item fold-in, for items that were not in the upload (call order: rec_sim -> rec_select or rec_set_neighbors -> item_foldin; it
 * reads only the tail, so it works on a union context).  The batch hangs on the tail and its lists: everything that drops the
 * tail drops it, and so do rec_sim, rec_select and rec_set_neighbors.  No item fold-in call changes what a resident call returns.
 *   xmap_ctx_item_foldin    : n_new items as a CSR of raters (ptr [n_new + 1], user / rating [ptr[n_new]], indices of resident
 *                             users) -> their RecommenderSim rows (xmap_itemfold_count / xmap_itemfold_fill with the resident
 *                             profiles, norms and the cap of xmap_ctx_rec_sim), their lists (xmap_rec_select with the context's
 *                             keep) and the extended tables of I + n_new items, kept on the device; the batch replaces the
 *                             previous one.  The input is checked on the host first (ptr[0] == 0, ptr non-decreasing, 0 <= user <
 *                             n_users): XMAP_ERR_ARG naming the position, no device work started.  A failed call leaves the
 *                             context as it was, the previous batch included.  counts [3] (may be NULL) = {pairs, records, items
 *                             with a pair}.  n_new == 0 is valid
 *   xmap_ctx_item_foldin_download : the batch's rows (row_ptr [n_new + 1], col / sim / ls / nij [pairs], rows not sorted), avg /
 *                             norm [n_new] and lists (nb_cnt [n_new], nb_col / nb_sim / nb_ls [n_new][keep]); any pointer may be NULL
 *   xmap_ctx_item_foldin_audience : xmap_ctx_audience for the batch's items: query_item = indices into the batch; their raters
 *                             are their holders (XMAP_AUDIENCE_KEEP_HOLDERS keeps them)
 *   xmap_ctx_item_foldin_predict : xmap_ctx_predict for pairs (resident user, batch item): test_item = indices into the batch
 *                             (both: an index outside [0, n_new) behaves like an item without a list)
 *   xmap_ctx_item_foldin_recommend : xmap_ctx_recommend over all I + n_new items: a batch item q is returned as I + q.  Limit:
 *                             top-N does not leave a batch item out of its own raters' lists -- the frozen profiles do not hold it
 * Eligibility (xmap_rec_filter above, HOST pointers inside; F == NULL: no rule): one entry per direction serves all three sources
 *   xmap_ctx_recommend_filtered : source XMAP_SRC_RESIDENT = xmap_ctx_recommend (also on a union context), XMAP_SRC_FOLDIN =
 *                             xmap_ctx_foldin_recommend, XMAP_SRC_ITEM_FOLDIN = xmap_ctx_item_foldin_recommend -- each with the
 *                             preconditions and the index spaces of that call; the mask and the exclusion ids are ITEMS (n = I, or
 *                             I + n_new for source 2)
 *   xmap_ctx_audience_filtered : likewise xmap_ctx_audience / xmap_ctx_foldin_audience / xmap_ctx_item_foldin_audience; the mask
 *                             and the exclusion ids are USERS (the batch's users for source 1)
 *                             stats [6] (may be NULL) as h_stats of the fine-grained calls.  The host checks min_score (NaN), ex_ptr
 *                             (ex_ptr[0] == 0, non-decreasing), ex_id (NULL while ids are listed) and source before any device
 *                             work: XMAP_ERR_ARG, the outputs untouched, the context as it was
 *   xmap_ctx_recommend_group : group lists (xmap_group_topn_rows) over the same three sources; stats [8] as its h_stats
 * Errors: negative return code, text in xmap_last_error(). */
typedef struct xmap_ctx xmap_ctx;

/* ---- native feeder (csrc/feeder.hip; host code, no GPU): raw lines `uid iid rating unix_ts` (reference README.md:41-42) ->
 * id tables + CSR + predicate arrays, with the reference's clean stage in between (core/baselinerClean.py:40-101: fields =
 * re.split(r"\s+"), local-time year in [year_from, year_to], item id = field + label, the latest rating of an item wins in
 * place, users with fewer than min_ratings ratings dropped; users in first-seen order, items in lexicographic id order).
 *   xmap_feed_text   : one domain's text                       xmap_feed_merge : source + target feed of one problem
 *   xmap_feed_texts  : the domains of one problem in one call (= the merge of their feeds, without building them)
 *   xmap_feed_sizes  : {users, items, ratings, bytes of the user ids, bytes of the item ids, lines read, lines in the period}
 *   xmap_feed_arrays : copies into caller buffers (any but user_ptr may be NULL); when = the timestamps as doubles
 *   xmap_feed_ids    : the id strings back to back + offsets [n + 1] (which = 0 users, 1 items; bytes may be NULL); which | 2:
 *                      a newline behind every id (bytes + n in all; offsets may then be NULL)
 *   xmap_ctx_upload_feed : the coarse ABI's upload straight from a feed (xmap_ctx_upload_ratings on its arrays); a rating
 *                      float32 does not hold exactly (NaN aside) -> XMAP_ERR_ARG naming uid, iid and value, context unchanged
 *   xmap_feed_format : test / bench utility, the inverse for one domain (items [item_lo, item_hi) of a CSR -> text) */
typedef struct xmap_feed xmap_feed;
int xmap_feed_text(const char *text, int64_t len, int32_t year_from, int32_t year_to, const char *label, int32_t min_ratings,
                   xmap_feed **out);
int xmap_feed_texts(int32_t n_parts, const char *const *texts, const int64_t *lens, const char *const *labels, int32_t year_from,
                    int32_t year_to, int32_t min_ratings, xmap_feed **out);
int xmap_feed_merge(const xmap_feed *a, const xmap_feed *b, xmap_feed **out);
int xmap_feed_sizes(const xmap_feed *f, int64_t *sizes /*[7]*/);
int xmap_feed_arrays(const xmap_feed *f, int64_t *user_ptr, int32_t *item, double *rating, double *when, int32_t *prefix_cls,
                     int32_t *suffix_cls, uint32_t *contains_mask, uint8_t *flags);
int xmap_feed_ids(const xmap_feed *f, int32_t which, char *bytes, int64_t *offsets);
void xmap_feed_free(xmap_feed *f);
int xmap_ctx_upload_feed(xmap_ctx *ctx, const xmap_feed *f);
int xmap_feed_format(int64_t n_users, const int64_t *user_ptr, const int32_t *item, const float *rating, const int64_t *when,
                     const char *uid_fmt, const char *iid_fmt, const int64_t *item_number, int32_t item_lo, int32_t item_hi,
                     char *out, int64_t cap, int64_t *written);

int xmap_ctx_create(int device, xmap_ctx **out);
void xmap_ctx_destroy(xmap_ctx *ctx);
int xmap_check_ratings(int64_t n_users, int32_t n_items, const int64_t *user_ptr, const int32_t *item, const int32_t *prefix_cls,
                       const int32_t *suffix_cls, int32_t allow_repeats);
int xmap_ctx_upload_ratings(xmap_ctx *ctx, int64_t n_users, int32_t n_items, const int64_t *user_ptr, const int32_t *item,
                            const float *rating, const int64_t *time, const int32_t *prefix_cls, const int32_t *suffix_cls,
                            const uint32_t *contains_mask, const uint8_t *flags);
int xmap_ctx_item_sim(xmap_ctx *ctx, int method, int cap, int64_t *n_kept, int64_t *n_evaluated);
int xmap_ctx_sim_download(xmap_ctx *ctx, int64_t *row_ptr, int32_t *col, double *sim, int32_t *mutu, int32_t *nij, double *info,
                          double *user_avg);
int xmap_ctx_extend(xmap_ctx *ctx, int top_k, int64_t *n_out, int64_t *n_paths);
int xmap_ctx_ext_download(xmap_ctx *ctx, int32_t *n_cand, int32_t *top_end, double *top_val);
int xmap_ctx_ext_lists(xmap_ctx *ctx, int64_t *xs_off, int32_t *xs_end, double *xs_val);
int xmap_ctx_candidates(xmap_ctx *ctx, int32_t *n_top);
int xmap_ctx_generate(xmap_ctx *ctx, int private_flag, const int32_t *picks, int32_t *choice, int64_t *n_rows,
                      int64_t *n_target_rows);
int xmap_ctx_gen_download(xmap_ctx *ctx, int32_t *user, int32_t *item, double *rating, int64_t *time);
int xmap_ctx_rec_sim(xmap_ctx *ctx, int cap, int64_t *n_pairs);
int xmap_ctx_rec_profiles_download(xmap_ctx *ctx, int64_t *prof_ptr, int32_t *prof_item, double *prof_rating, int64_t *prof_time);
int xmap_ctx_rec_download(xmap_ctx *ctx, int64_t *row_ptr, int32_t *col, double *sim, double *ls, int32_t *nij, double *item_avg,
                          double *item_norm);
int xmap_ctx_rec_select(xmap_ctx *ctx, int keep);
int xmap_ctx_rec_set_neighbors(xmap_ctx *ctx, int keep, const int32_t *cnt, const int32_t *col, const double *sim);
int xmap_ctx_rec_neighbors_download(xmap_ctx *ctx, int32_t *cnt, int32_t *col, double *sim, double *ls);
int xmap_ctx_predict(xmap_ctx *ctx, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const double *test_rating,
                     const double *wtab, int32_t n_w, double *out_plain, double *out_decay, int32_t *status, double *mae,
                     int32_t *max_now);
int xmap_ctx_recommend(xmap_ctx *ctx, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by,
                       int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_item,
                       double *out_plain, double *out_decay, int64_t *stats /* [4] or NULL */);
int xmap_ctx_evaluate_topn(xmap_ctx *ctx, int64_t n_test, const int32_t *test_user, const int32_t *test_item,
                           const double *test_rating, double rel_min, int32_t n_top, int32_t rank_by, int32_t flags,
                           const double *wtab, int32_t n_w, int32_t n_cut, const int32_t *cut, const double *dtab,
                           double *agg /*[n_cut][8]*/, int64_t *cover /*[n_cut]*/,
                           int32_t *user_nrel /*[U] or NULL*/, uint64_t *user_mask /*[U] or NULL: 0 for a user not evaluated*/,
                           int64_t *stats /*[8] or NULL*/);
int xmap_ctx_foldin(xmap_ctx *ctx, int64_t n_new, const int64_t *ptr, const int32_t *item, const float *rating,
                    const int64_t *time, int64_t *counts /*[3] or NULL*/);
int xmap_ctx_foldin_download(xmap_ctx *ctx, int64_t *prof_ptr, int32_t *prof_item, double *prof_rating, int64_t *prof_time);
int xmap_ctx_foldin_recommend(xmap_ctx *ctx, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by,
                              int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_item,
                              double *out_plain, double *out_decay, int64_t *stats /* [4] or NULL */);
int xmap_ctx_foldin_predict(xmap_ctx *ctx, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const double *test_rating,
                            const double *wtab, int32_t n_w, double *out_plain, double *out_decay, int32_t *status, double *mae,
                            int32_t *max_now);
int xmap_ctx_audience(xmap_ctx *ctx, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by,
                      int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user,
                      double *out_plain, double *out_decay, int64_t *stats /* [4] or NULL */);
int xmap_ctx_foldin_audience(xmap_ctx *ctx, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by,
                             int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user,
                             double *out_plain, double *out_decay, int64_t *stats /* [4] or NULL */);
int xmap_ctx_item_foldin(xmap_ctx *ctx, int64_t n_new, const int64_t *ptr, const int32_t *user, const double *rating,
                         int64_t *counts /*[3] or NULL*/);
int xmap_ctx_item_foldin_download(xmap_ctx *ctx, int64_t *row_ptr, int32_t *col, double *sim, double *ls, int32_t *nij, double *avg,
                                  double *norm, int32_t *nb_cnt, int32_t *nb_col, double *nb_sim, double *nb_ls);
int xmap_ctx_item_foldin_audience(xmap_ctx *ctx, int64_t n_query, const int32_t *query_item, int32_t n_top, int32_t rank_by,
                                  int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user,
                                  double *out_plain, double *out_decay, int64_t *stats /* [4] or NULL */);
int xmap_ctx_item_foldin_predict(xmap_ctx *ctx, int64_t n_test, const int32_t *test_user, const int32_t *test_item, const double *test_rating,
                                 const double *wtab, int32_t n_w, double *out_plain, double *out_decay, int32_t *status, double *mae,
                                 int32_t *max_now);
int xmap_ctx_item_foldin_recommend(xmap_ctx *ctx, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by,
                                   int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_item,
                                   double *out_plain, double *out_decay, int64_t *stats /* [4] or NULL */);
#define XMAP_SRC_RESIDENT 0
#define XMAP_SRC_FOLDIN 1
#define XMAP_SRC_ITEM_FOLDIN 2
int xmap_ctx_recommend_filtered(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top,
                                int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_item,
                                double *out_plain, double *out_decay, const xmap_rec_filter *F /* host pointers inside, or NULL */,
                                int64_t *stats /* [6] or NULL */);
int xmap_ctx_audience_filtered(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_item, int32_t n_top,
                               int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t *out_cnt, int32_t *out_user,
                               double *out_plain, double *out_decay, const xmap_rec_filter *F /* host pointers inside, or NULL */,
                               int64_t *stats /* [6] or NULL */);
/* Diversified top-N: xmap_ctx_recommend_filtered with n_top = n_pool into device temporaries, then xmap_diversify_rows over the
 * context's diversity index of the resident RecommenderSim -- so the rules of F act before the pool is cut, and the floor before
 * the re-ranking.  Sources: XMAP_SRC_RESIDENT (also on a union context) and XMAP_SRC_FOLDIN; XMAP_SRC_ITEM_FOLDIN is XMAP_ERR_ARG
 * (the rows of batch items are not part of the index).  weight finite and >= 0, 1 <= n_top <= n_pool <= 64 and the source are
 * checked on the host before any device work: on XMAP_ERR_ARG the outputs are untouched and the context is as it was.  The index
 * is built on first use, dropped with the RecommenderSim result (any earlier stage run again) and kept by
 * xmap_ctx_rec_set_neighbors / xmap_ctx_rec_select: it belongs to the matrix, not to the lists.  Host outputs: out_cnt [n_query],
 * out_item / out_plain / out_decay / out_pen [n_query][n_top], out_ils [n_query]. */
int xmap_ctx_recommend_diverse(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_pool,
                               int32_t n_top, int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, double weight,
                               const xmap_rec_filter *F /* host pointers inside, or NULL */, int32_t *out_cnt, int32_t *out_item,
                               double *out_plain, double *out_decay, double *out_pen, double *out_ils,
                               int64_t *stats /* [8] or NULL: the six of xmap_ctx_recommend_filtered, then the two of
                                                 xmap_diversify_rows */);
/* Group lists: xmap_group_topn_rows over the resident tables, host arrays in and out.  Sources as xmap_ctx_recommend_filtered; with
 * XMAP_SRC_FOLDIN the members index the fold-in batch (a party of guests nobody trained on), with XMAP_SRC_ITEM_FOLDIN a batch
 * item q is returned as I + q.  The mask and the exclusion ids are ITEMS; F->ex_ptr has one list per GROUP.  how, veto (NaN),
 * n_top, rank_by, flags, grp_ptr (grp_ptr[0] == 0, non-decreasing, sizes <= XMAP_GROUP_MAX_MEMBERS), the filter and the source
 * are checked on the host before any device work: on XMAP_ERR_ARG the outputs are untouched and the context is as it was.  Host
 * outputs: out_cnt [n_groups], out_item / out_plain / out_decay / out_low [n_groups][n_top]. */
int xmap_ctx_recommend_group(xmap_ctx *ctx, int32_t source, int64_t n_groups, const int64_t *grp_ptr, const int32_t *grp_user,
                             int32_t n_top, int32_t rank_by, int32_t flags, int32_t how, double veto, const double *wtab, int32_t n_w,
                             int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay, int32_t *out_low,
                             const xmap_rec_filter *F /* host pointers inside, or NULL */, int64_t *stats /* [8] or NULL */);
/* Peers: xmap_peer_rows over the context's profiles, host arrays in and out.  XMAP_SRC_RESIDENT: the queries are resident users
 * and the library sets XMAP_PEERS_SAME (also on a union context); XMAP_SRC_FOLDIN: the queries index the fold-in batch, the
 * candidates are the resident users, no self rule; XMAP_SRC_ITEM_FOLDIN is XMAP_ERR_ARG.  flags: XMAP_PEERS_KEEP_SELF,
 * XMAP_PEERS_CENTRED (centre by the context's item averages).  Needs the result of xmap_ctx_rec_sim: have_rec, the profiles and the averages.
 * The index is cached in the context per centring: built on first use, dropped by whatever drops the profiles or the averages.
 * The mask and the exclusion ids are USERS.  n_top, cap, min_common, flags, the source and the filter are checked on the host
 * before any device work: on XMAP_ERR_ARG the outputs keep every byte.  Host outputs: out_cnt [n_query], out_user / out_sim /
 * out_common [n_query][n_top]. */
int xmap_ctx_peers(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t flags, int32_t cap,
                   int32_t min_common, int32_t *out_cnt, int32_t *out_user, double *out_sim, int32_t *out_common,
                   const xmap_rec_filter *F /* host pointers inside, or NULL */, int64_t *stats /* [6] or NULL */);
/* xmap_ctx_peers plus the local sensitivity of every returned entry (xmap_peer_rows_ls): the same sources, flags, index cache
 * and host checks -- on XMAP_ERR_ARG (out_ls == NULL included) the outputs keep every byte.  Host out_ls [n_query][n_top]. */
int xmap_ctx_peers_ls(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t flags,
                      int32_t cap, int32_t min_common, int32_t *out_cnt, int32_t *out_user, double *out_sim, int32_t *out_common,
                      double *out_ls, const xmap_rec_filter *F /* host pointers inside, or NULL */, int64_t *stats /* [6] or NULL */);
/* User-kNN: the peers of the users in question by xmap_peer_rows exactly as xmap_ctx_peers runs it (source, n_nb as its n_top,
 * peer_flags = XMAP_PEERS_KEEP_SELF | XMAP_PEERS_CENTRED, cap, min_common; no rules on the peers), the means by xmap_uknn_means
 * (the resident users'; with XMAP_SRC_FOLDIN the queries' own means over the batch's profiles), then xmap_uknn_predict_rows /
 * xmap_uknn_topn_rows over the resident profiles.  Host arrays in and out.  XMAP_SRC_ITEM_FOLDIN is XMAP_ERR_ARG.  Needs what
 * xmap_ctx_peers needs.  n_nb, n_top, min_support, cap, min_common, both flag words, the source and the filter are checked on the
 * host before the context is read or any device work is done: on XMAP_ERR_ARG the outputs keep every byte.
 * xmap_ctx_uknn_predict: test_user indexes the resident users or the batch; the distinct users of the pairs are the queries.
 *   flags: XMAP_UKNN_OWN_MEAN.  Host outputs out_score / out_bound / out_n / status [n_test] as xmap_uknn_predict_rows writes
 *   them (status 3 cannot occur for a user: a user outside the source has no list, status 1).  mae ([2] or NULL; needs
 *   test_rating) = {pairs with status 0, sum |test_rating - out_bound| over them} by xmap_mae.
 * xmap_ctx_uknn_recommend: query_user indexes the resident users or the batch; the held items are the query's own rows there.
 *   flags: XMAP_UKNN_OWN_MEAN | XMAP_UKNN_KEEP_HELD.  The mask and the exclusion ids of F are ITEMS.  Host outputs: out_cnt
 *   [n_query], out_item / out_score / out_support [n_query][n_top]; stats as the h_stats of xmap_uknn_topn_rows. */
int xmap_ctx_uknn_predict(xmap_ctx *ctx, int32_t source, int64_t n_test, const int32_t *test_user, const int32_t *test_item,
                          const double *test_rating /* or NULL */, int32_t n_nb, int32_t peer_flags, int32_t cap, int32_t min_common,
                          int32_t flags, double *out_score, double *out_bound, int32_t *out_n, int32_t *status,
                          double *mae /* [2] or NULL */);
int xmap_ctx_uknn_recommend(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_nb,
                            int32_t peer_flags, int32_t cap, int32_t min_common, int32_t flags, int32_t n_top, int32_t min_support,
                            int32_t *out_cnt, int32_t *out_item, double *out_score, int32_t *out_support,
                            const xmap_rec_filter *F /* host pointers inside, or NULL */, int64_t *stats /* [6] or NULL */);
/* Related items for a basket: xmap_related_rows over the context's RecommenderSim CSR.  Host arrays in (b_ptr / b_item / b_weight,
 * F with host pointers), host arrays out, as xmap_related_rows defines them; stats as its h_stats.  Needs the result of
 * xmap_ctx_rec_sim only (have_rec) -- no neighbour lists -- so it works right after xmap_ctx_rec_sim and on a union context, and
 * goes with whatever drops the RecommenderSim rows.  n_top, how, flags, min_support, max_records, the pointers, b_ptr and the
 * filter are checked on the host before the context is read or any device work is done: on XMAP_ERR_ARG the outputs keep every
 * byte. */
int xmap_ctx_related(xmap_ctx *ctx, int64_t n_query, const int64_t *b_ptr /*[n_query+1]*/, const int32_t *b_item,
                     const double *b_weight /* or NULL */, int32_t how, int32_t flags, int32_t n_top, int32_t min_support,
                     int64_t max_records /*0: library default*/, int32_t *out_cnt, int32_t *out_item, double *out_score,
                     int32_t *out_support, const xmap_rec_filter *F /* host pointers inside, or NULL */, int64_t *stats /* [6] or NULL */);
/* Popularity fill: the ranking (xmap_pop_index) over the context's peer index of the raw ratings, built on first use and kept
 * beside it with the (how, damping, min_count) it was built for: rebuilt when those differ, dropped with the tail.  One ranking
 * per context.
 *   xmap_ctx_popular        : the head of the ranking: out_item / out_score [n_max] (host; -1 / 0.0 behind the ranking's end).  ALL
 *                             n_max entries of both are written, also where n_max exceeds the number of items: the caller's
 *                             buffers hold n_max entries, not min(n_max, n_items).  *n_ranked = the whole ranking's length.  Needs the resident profiles (have_rec), also on a union context.
 *   xmap_ctx_recommend_filled : xmap_ctx_recommend_filtered into device temporaries, then xmap_topn_fill_rows; out_src [n_query][n_top]
 *                             as it writes it.  Sources as the filtered call: XMAP_SRC_FOLDIN: held is the batch's rows, popularity
 *                             is the resident users'; XMAP_SRC_ITEM_FOLDIN: the batch items are never filled.  stats [10]: the six of
 *                             xmap_ctx_recommend_filtered, then the four of xmap_topn_fill_rows.
 * n_top, rank_by, how, damping, min_count, source, flags, a NaN floor and n_max are checked on the host before the context is
 * read, each check naming its argument: on XMAP_ERR_ARG the outputs keep every byte. */
int xmap_ctx_popular(xmap_ctx *ctx, int32_t how, double damping, int32_t min_count, int64_t n_max, int32_t *out_item,
                     double *out_score /* host [n_max] */, int64_t *n_ranked /* host, the whole ranking's length */);
int xmap_ctx_recommend_filled(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top,
                              int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t how, double damping,
                              int32_t min_count, int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay,
                              int32_t *out_src, const xmap_rec_filter *F /* host pointers inside, or NULL */,
                              int64_t *stats /* [10] or NULL */);
/* Fused lists: xmap_fuse_rows with host arrays in and out.
 *   xmap_ctx_fuse : lists holds HOST pointers (cnt [n_query], item / score [n_query][width]); they are uploaded, fused with the
 *                   library's default max_records, and out_cnt [n_query], out_id / out_score / out_lists [n_query][n_top] and
 *                   stats ([5] or NULL, the h_stats of xmap_fuse_rows) come back.  The context is used for its device and stream
 *                   only: no stage needs to have run.  The host checks of xmap_fuse_rows are made before the context is read: a
 *                   NULL context with good arguments fails on the context check alone.
 *   xmap_ctx_recommend_hybrid : the item-based and the user-based lists of the same query users, fused.  List 0 is what
 *                   xmap_ctx_recommend_filtered returns with n_top = n_pool_items (1 .. 64): the score of rank_by (0 plain, 1
 *                   decayed), with wtab / n_w and topn_flags.  List 1 is what xmap_ctx_uknn_recommend returns with n_top =
 *                   n_pool_users (1 .. 1024), given n_nb, peer_flags, cap, min_common, uknn_flags and min_support.  The one F
 *                   acts on both halves (the mask and the exclusion ids are ITEMS).  Both lists stay in device temporaries and
 *                   are fused with w_items, w_users, how, rrf_c, min_lists (1 .. 2) over n_ids = the context's items.  Sources:
 *                   XMAP_SRC_RESIDENT (also on a union context) and XMAP_SRC_FOLDIN; XMAP_SRC_ITEM_FOLDIN is XMAP_ERR_ARG, as in
 *                   the user-kNN calls.  Needs what both calls need.  stats ([17] or NULL): the six of
 *                   xmap_ctx_recommend_filtered, the six of xmap_ctx_uknn_recommend, the five of xmap_fuse_rows.  Defined as
 *                   equal, byte for byte, to calling the three public coarse calls one after the other.
 * Every argument is checked on the host before the context is read, each check naming its argument: on XMAP_ERR_ARG the outputs
 * keep every byte. */
int xmap_ctx_fuse(xmap_ctx *ctx, int64_t n_query, int32_t n_lists, const xmap_fuse_list *lists /* host pointers inside */,
                  int32_t n_ids, int32_t how, double rrf_c, int32_t min_lists, int32_t n_top, int32_t *out_cnt, int32_t *out_id,
                  double *out_score, int32_t *out_lists, int64_t *stats /* [5] or NULL */);
int xmap_ctx_recommend_hybrid(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_top,
                              int32_t n_pool_items, int32_t rank_by, int32_t topn_flags, const double *wtab, int32_t n_w,
                              int32_t n_pool_users, int32_t n_nb, int32_t peer_flags, int32_t cap, int32_t min_common,
                              int32_t uknn_flags, int32_t min_support, double w_items, double w_users, int32_t how, double rrf_c,
                              int32_t min_lists, const xmap_rec_filter *F /* host pointers inside, or NULL */, int32_t *out_cnt,
                              int32_t *out_item, double *out_score, int32_t *out_lists, int64_t *stats /* [17] or NULL */);
/* Shelves: xmap_shelf_rows over the resident tables, host arrays in and out.
 *   xmap_ctx_set_labels : the label table of the context's item space (host arrays: lab_ptr [n_items + 1], lab_id), checked as
 *                   xmap_shelf_rows checks it and kept on the device beside the tail.  A second call replaces the table (a table
 *                   that fails leaves the earlier one in place); n_labels == 0 drops it (lab_ptr / lab_id are not read).  The labels
 *                   survive a retraining of the tail (xmap_ctx_rec_sim, xmap_ctx_rec_select); they go with the item space (an
 *                   upload, a union) and with the context.  Needs the item space (have_gen; also on a union context).
 *   xmap_ctx_recommend_shelves : sources as xmap_ctx_recommend_filtered (XMAP_SRC_RESIDENT also on a union context; XMAP_SRC_FOLDIN;
 *                   XMAP_SRC_ITEM_FOLDIN: the batch items carry no label, lab_ptr is extended by its last value).  lab_allow: host
 *                   words over the labels, or NULL.  The outputs are those of xmap_shelf_rows in host memory; max_records is the
 *                   library's default.  Without labels set: XMAP_ERR_ARG, the message says so.
 * Every argument is checked on the host before the context is read, each check naming its argument: on XMAP_ERR_ARG the outputs
 * keep every byte. */
int xmap_ctx_set_labels(xmap_ctx *ctx, int32_t n_labels, const int64_t *lab_ptr /*[n_items+1]*/, const int32_t *lab_id);
int xmap_ctx_recommend_shelves(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_shelf, int32_t n_top,
                               int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t shelf_by, int32_t min_fill,
                               const uint32_t *lab_allow /* host words, or NULL */, int32_t *out_nshelf, int32_t *out_label,
                               double *out_sscore, int32_t *out_size, int32_t *out_cnt, int32_t *out_item, double *out_plain,
                               double *out_decay, const xmap_rec_filter *F /* host pointers inside, or NULL */,
                               int64_t *stats /* [10] or NULL */);
/* Quotas and calibrated lists: xmap_quota_rows over the resident tables and the labels of xmap_ctx_set_labels, host arrays in and
 * out.  Sources as xmap_ctx_recommend_shelves (XMAP_SRC_FOLDIN: the history of SHARE mode is the fold-in batch's profiles;
 * XMAP_SRC_ITEM_FOLDIN: the batch items carry no label).  lab_cap / lab_weight: host arrays [n_labels of the context], or NULL;
 * lab_allow: host words over the labels, or NULL.  The outputs are those of xmap_quota_rows in host memory.  Without labels set:
 * XMAP_ERR_ARG, the message says so.  Every scalar argument is checked on the host before the context is read, each check naming
 * its argument (n_query >= 0, n_pool, n_top, rank_by, flags, mode, cap >= 1 where lab_cap is NULL in CAP mode, source, a NaN floor
 * in F): on XMAP_ERR_ARG the outputs keep every byte. */
int xmap_ctx_recommend_quota(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t n_top,
                             int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t mode, int32_t cap,
                             const int32_t *lab_cap /* host, or NULL */, const uint32_t *lab_weight /* host, or NULL */,
                             const uint32_t *lab_allow /* host words, or NULL */, int32_t *out_cnt, int32_t *out_item,
                             double *out_plain, double *out_decay, int32_t *out_pos, int32_t *out_label,
                             const xmap_rec_filter *F /* host pointers inside, or NULL */, int64_t *stats /* [10] or NULL */);
/* Allotment: xmap_allot_rows over the three sources (as xmap_ctx_recommend_quota), host arrays in and out.  item_cap: host int32
 * [n_cap], or NULL (then the scalar cap >= 1); n_cap must equal the item count of the source's tables (the resident items, plus the
 * batch items for XMAP_SRC_ITEM_FOLDIN), which the context check holds it to.  item_taken: host int32 [n_cap items of the source], or
 * NULL.  The outputs are those of xmap_allot_rows in host memory; stats [12].  Every argument that can be is checked on the host
 * before the context is read, each check naming its argument (n_query, n_pool 1 .. 64, n_top, rank_by, flags, cap, a negative
 * item_cap entry, source, a NaN floor in F): on XMAP_ERR_ARG the outputs keep every byte. */
int xmap_ctx_recommend_allot(xmap_ctx *ctx, int32_t source, int64_t n_query, const int32_t *query_user, int32_t n_pool, int32_t n_top,
                             int32_t rank_by, int32_t flags, const double *wtab, int32_t n_w, int32_t cap,
                             const int32_t *item_cap /* host [n_cap], or NULL */, int32_t n_cap, int32_t *out_cnt, int32_t *out_item,
                             double *out_plain, double *out_decay, int32_t *out_pos, int32_t *item_taken /* host, or NULL */,
                             const xmap_rec_filter *F /* host pointers inside, or NULL */, int64_t *stats /* [12] or NULL */);
int xmap_ctx_union(xmap_ctx *dst, int n_parts, xmap_ctx *const *src, const int32_t *const *user_map, const int32_t *const *item_map,
                   int64_t n_users, int32_t n_items, int flags, int64_t *counts /*[4] or NULL*/);
int xmap_ctx_explain(xmap_ctx *ctx, int64_t n_pairs, const int32_t *pair_user, const int32_t *pair_item, int32_t rank_by,
                     int32_t n_ev, int32_t n_src, const double *wtab, int32_t n_w, int32_t *ex_status, int32_t *ex_total,
                     int32_t *ex_cnt, double *ex_score, int64_t *ex_row, int32_t *ex_slot, double *ex_share,
                     int32_t *src_total /*[n_pairs][n_ev]; NULL with n_src == 0*/,
                     int64_t *src_pos /*[n_pairs][n_ev][n_src]; NULL with n_src == 0*/, int32_t *max_now /*or NULL*/);
int xmap_ctx_foldin_explain(xmap_ctx *ctx, int64_t n_pairs, const int32_t *pair_user, const int32_t *pair_item, int32_t rank_by,
                            int32_t n_ev, int32_t n_src, const double *wtab, int32_t n_w, int32_t *ex_status, int32_t *ex_total,
                            int32_t *ex_cnt, double *ex_score, int64_t *ex_row, int32_t *ex_slot, double *ex_share,
                            int32_t *src_total, int64_t *src_pos, int32_t *max_now);

#ifdef __cplusplus
}
#endif
#endif
