// stage_e_shelf.hip -- shelves on the device (DESIGN.md 4 "Shelves"): a page is not one ranking but a top-N per LABEL of the items
// ("Top picks in Cookery"), and the page shows the best shelves of this user.  Items carry labels as a CSR over the item space
// (lab_ptr, lab_id; the labels of one item strictly ascending); per query the kept candidates are those of xmap_topn_rows_filtered
// -- tn_score_candidates (topn_pass.h) is the front half, unchanged -- and the back half here works on its scored segments:
//   k_rf_check    : (rec_filter.h) cand_ptr / lab_ptr: [0] == 0, non-decreasing, the first bad position
//   k_sh_check    : lab_id: every id in [0, n_labels), strictly ascending inside an item; the first bad index of either rule.
//                   Nothing is read through a table before it passed
//   k_sh_count    : one lane per candidate: records = the allowed labels of a kept candidate (sh_records: the ONE statement of
//                   "the records of candidate p" that the count and the expansion both call) -> scan
//   k_sh_expand   : per chunk of consecutive queries: key = (q - q0) << label_bits | label, value = the candidate's position in its
//                   segment; the records of a query come in candidate order = ascending item
//   pr_run_tables : (sorted_runs.h, as are the chunk plan pr_plan_chunks and the walk pr_each_chunk) the stable sort -- a run
//                   (q, label) = a shelf, its records in ascending item --, the runs, per query of the chunk its first run
//   k_sh_runs     : one wave per run: the shelf's score.  The run streams 64 records at a time through the register insertion of
//                   k_tn_select (sh_select: lane j holds the j-th best); BEST and LABEL keep one entry (the arg-max), MEAN n_top,
//                   then sums them in rank order in every lane alike
//   k_sh_pick     : one wave per query: the n_shelf best formed runs by (score, label) -- by label alone under LABEL -- with the
//                   same insertion; writes the per-shelf outputs and the chosen run of every slot
//   k_sh_fill     : one wave per chosen (q, s): the selection again, n_top wide, straight into the outputs.  The chosen runs are
//                   selected twice; no temporary of runs x n_top exists.
//   k_sh_blank    : counts and padding
// Temporaries: 12 B per candidate, 48 B per record of the largest chunk, 8 + 4 n_shelf B per query.  No floating-point atomic, no
// lock, every offset int64: the bytes depend on no grid, no atomic order and no chunking.
#include <vector>

#include "common.h"
#include "predict_rows.h"
#include "rec_filter.h"
#include "sorted_runs.h"
#include "topn_pass.h"

namespace xmap {

// A record takes 48 B of temporaries: the default chunk (PR_MAX_RECORDS) 201 MB.
constexpr int SH_MAX = 64;                              // n_top and n_shelf: one lane per entry
constexpr unsigned SH_MAX_BLOCKS = 1u << 16;            // blocks of a grid-stride launch (4 waves each)
static_assert(SH_MAX == TN_MAX_TOP && SH_MAX == WAVE, "a shelf has the layout of a row of xmap_topn_rows; lane j holds entry j");

// lab_id over the items [0, I): bad[0] = the first index with an id outside [0, n_labels), bad[1] = the first index whose id is
// not above the id in front of it inside one item (RF_NO_POS: none).  lab_ptr has passed k_rf_check.
__global__ __launch_bounds__(256) void k_sh_check(int I, int n_labels, const long long *lab_ptr, const int *lab_id, unsigned long long *bad) {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < I; i += step) {
        const long long a = lab_ptr[i], b = lab_ptr[i + 1];
        for (long long k = a; k < b; k++) {
            const int l = lab_id[k];
            if (l < 0 || l >= n_labels) atomicMin(&bad[0], (unsigned long long)k);      // (a minimum does not depend on the order)
            if (k > a && l <= lab_id[k - 1]) atomicMin(&bad[1], (unsigned long long)k);
        }
    }
}

// The ONE statement of "candidate p is kept, and these are its records": status 0, the rank_by score not below the floor (as
// k_tn_select tests it), an item of the label table, one record per allowed label in ascending label.  Returns the count.
template <class Emit>
__device__ __forceinline__ int sh_records(long long p, const int *cand_item, const double *plain, const double *decay, const int *status,
                                          int rank_by, double min_score, int I, const long long *lab_ptr, const int *lab_id,
                                          const unsigned int *lab_allow, int &dropped, int &floored, Emit emit) {
    dropped = floored = 0;
    if (status[p] != 0) { dropped = 1; return 0; }
    const double xs = rank_by ? decay[p] : plain[p];
    if (xs < min_score) { floored = 1; return 0; }
    const int it = cand_item[p];
    if (it < 0 || it >= I) return 0;
    int c = 0;
    const long long b = lab_ptr[it + 1];
    for (long long k = lab_ptr[it]; k < b; k++) {
        const int l = lab_id[k];
        if (lab_allow && !bit_allowed(lab_allow, l)) continue;
        emit(c, l);
        c++;
    }
    return c;
}

// cnt[p] = records of candidate p; st4: [0] += candidates with status != 0, [2] += kept-status candidates below the floor
__global__ __launch_bounds__(256) void k_sh_count(long long base, long long n, const int *cand_item, const double *plain, const double *decay,
                                                  const int *status, int rank_by, double min_score, int I, const long long *lab_ptr,
                                                  const int *lab_id, const unsigned int *lab_allow, int *cnt, unsigned long long *st4) {
    const long long p = base + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = p < n;
    int d = 0, f = 0;
    if (in) cnt[p] = sh_records(p, cand_item, plain, decay, status, rank_by, min_score, I, lab_ptr, lab_id, lab_allow, d, f, [](int, int) {});
    const int nd = __popcll(__ballot(d != 0)), nf = __popcll(__ballot(f != 0));
    if (lane_id() == 0) {
        if (nd) atomicAdd(&st4[0], (unsigned long long)nd);
        if (nf) atomicAdd(&st4[2], (unsigned long long)nf);
    }
}

// qrec[q] = records in front of query q = rec_off[cand_ptr[q]], q <= n_query; st4[1] = the largest segment
__global__ __launch_bounds__(256) void k_sh_qrec(long long n_query, const long long *cand_ptr, const long long *rec_off, long long *qrec,
                                                 unsigned long long *st4) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > n_query) return;
    qrec[q] = rec_off[cand_ptr[q]];
    if (q < n_query) atomicMax(&st4[1], (unsigned long long)(cand_ptr[q + 1] - cand_ptr[q]));
}

// one lane per candidate p of the chunk [c0 + base .. c1): its records at rec_off[p] - rec0
__global__ __launch_bounds__(256) void k_sh_expand(long long p0, long long p1, long long rec0, long long q0, long long n_query,
                                                   const long long *cand_ptr, const int *cand_item, const double *plain, const double *decay,
                                                   const int *status, int rank_by, double min_score, int I, const long long *lab_ptr,
                                                   const int *lab_id, const unsigned int *lab_allow, const long long *rec_off,
                                                   int label_bits, unsigned long long *keys, int *vals) {
    const long long p = p0 + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= p1) return;
    const long long o = rec_off[p] - rec0, end = rec_off[p + 1] - rec0;
    if (o == end) return;                       // no record
    const long long q = pr_last_le(cand_ptr, 0, n_query, p);       // the last q with cand_ptr[q] <= p: empty segments are passed over
    const unsigned long long qk = (unsigned long long)(q - q0) << label_bits;
    const int at = (int)(p - cand_ptr[q]);
    int d, f;
    sh_records(p, cand_item, plain, decay, status, rank_by, min_score, I, lab_ptr, lab_id, lab_allow, d, f, [&](int c, int l) {
        if (o + c < end) {                      // (the count pass saw the same table)
            keys[o + c] = qk | (unsigned long long)(unsigned)l;
            vals[o + c] = at;
        }
    });
}

// The register insertion of k_tn_select over the records [s, e) of a sorted chunk (candidate = base + vals[t], ascending item
// inside a run): on return lane j < have holds the j-th best by (rank_by score descending as numbers, item ascending), have <=
// n_sel.  Every lane of the wave calls it with the same arguments.
__device__ __forceinline__ void sh_select(long long s, long long e, const int *vals, long long base, const int *cand_item, const double *plain,
                                          const double *decay, int rank_by, int n_sel, double &ks, double &kp, double &kd, int &ki,
                                          int &have) {
    const int lane = lane_id();
    ks = kp = kd = 0.0;
    ki = -1;
    have = 0;
    for (long long t = s; t < e; t += WAVE) {
        const bool in = t + lane < e;
        const long long p = in ? base + vals[t + lane] : 0;
        const int xi = in ? cand_item[p] : 0;
        const double xp = in ? plain[p] : 0.0, xd = in ? decay[p] : 0.0;
        const double xs = rank_by ? xd : xp;
        const double ws = rld(ks, n_sel - 1);
        const int wi = rl32(ki, n_sel - 1);
        unsigned long long m = __ballot(in && (have < n_sel || xs > ws || (xs == ws && xi < wi)));
        while (m) {
            const int j = __ffsll((long long)m) - 1;
            m &= m - 1;
            const double es = rld(xs, j), ep = rld(xp, j), ed = rld(xd, j);
            const int ei = rl32(xi, j);
            const int pos = __popcll(__ballot(lane < have && (ks > es || (ks == es && ki < ei))));
            if (pos >= n_sel) continue;
            const double us = __shfl_up(ks, 1, 64), up = __shfl_up(kp, 1, 64), ud = __shfl_up(kd, 1, 64);
            const int ui = __shfl_up(ki, 1, 64);
            if (lane > pos) { ks = us; kp = up; kd = ud; ki = ui; }
            else if (lane == pos) { ks = es; kp = ep; kd = ed; ki = ei; }
            have = have < n_sel ? have + 1 : n_sel;
        }
    }
}

// one wave per run r of the chunk: r_score[r].  st4: [1] += runs, [2] += runs below min_fill
__global__ __launch_bounds__(256) void k_sh_runs(long long n, long long q0, const unsigned long long *keys, const int *vals,
                                                 const long long *run_idx, const int *run_start, int label_bits, const long long *cand_ptr,
                                                 const int *cand_item, const double *plain, const double *decay, int rank_by, int n_top,
                                                 int shelf_by, int min_fill, double *r_score, unsigned long long *st4) {
    const long long n_runs = run_idx[n];
    const long long step = (long long)gridDim.x * (blockDim.x / WAVE);
    int small = 0;
    for (long long r = (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6); r < n_runs; r += step) {      // (wave-uniform)
        const long long s = run_start[r], e = run_start[r + 1];
        const long long base = cand_ptr[q0 + (long long)(keys[s] >> label_bits)];
        double ks, kp, kd;
        int ki, have;
        sh_select(s, e, vals, base, cand_item, plain, decay, rank_by, shelf_by == XMAP_SHELF_BY_MEAN ? n_top : 1, ks, kp, kd, ki, have);
        double score = rld(ks, 0);              // the bits of entry 0
        if (shelf_by == XMAP_SHELF_BY_MEAN) {   // (((s_0 + s_1) + ...) + s_{cnt-1}) / cnt, in every lane alike
            for (int j = 1; j < have; j++) score += rld(ks, j);
            score = score / (double)have;
        }
        if (lane_id() == 0) r_score[r] = score;
        small += e - s < min_fill ? 1 : 0;
    }
    if (lane_id() == 0 && small) atomicAdd(&st4[2], (unsigned long long)small);
    if (blockIdx.x == 0 && threadIdx.x == 0 && n_runs) atomicAdd(&st4[1], (unsigned long long)n_runs);
}

// one wave per query x of the chunk: the n_shelf best formed runs of [first[x], first[x + 1]) (ascending label); lane j holds the
// j-th best shelf.  sel_run[x][s] = the chosen run (-1 behind the count).  st4[3] = the most formed shelves of one query
__global__ __launch_bounds__(256) void k_sh_pick(long long nq, long long q0, int n_shelf, int n_top, int shelf_by, int min_fill,
                                                 const long long *first, const unsigned long long *keys, const int *run_start,
                                                 int label_bits, const double *r_score, int *sel_run, int *out_nshelf, int *out_label,
                                                 double *out_sscore, int *out_size, int *out_cnt, unsigned long long *st4) {
    const int lane = lane_id();
    const long long step = (long long)gridDim.x * (blockDim.x / WAVE);
    const unsigned long long lmask = (1ull << label_bits) - 1ull;
    for (long long x = (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6); x < nq; x += step) {
        const long long a = first[x], b = first[x + 1];
        double kc = 0.0, ksc = 0.0;             // the score the order compares (0.0 under LABEL), the shelf's score
        int kl = -1, kr = -1, kz = 0, have = 0, formed = 0;
        for (long long r = a; r < b; r += WAVE) {
            const bool in = r + lane < b;
            const int rs = in ? run_start[r + lane] : 0, re = in ? run_start[r + lane + 1] : 0;
            const bool ok = in && re - rs >= min_fill;
            formed += __popcll(__ballot(ok));
            const int xl = ok ? (int)(keys[rs] & lmask) : 0, xr = (int)(r + lane), xz = re - rs;
            const double xsc = ok ? r_score[r + lane] : 0.0;
            const double xc = shelf_by == XMAP_SHELF_BY_LABEL ? 0.0 : xsc;
            const double wc = rld(kc, n_shelf - 1);
            const int wl = rl32(kl, n_shelf - 1);
            unsigned long long m = __ballot(ok && (have < n_shelf || xc > wc || (xc == wc && xl < wl)));
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                const double ec = rld(xc, j), esc = rld(xsc, j);
                const int el = rl32(xl, j), er = rl32(xr, j), ez = rl32(xz, j);
                const int pos = __popcll(__ballot(lane < have && (kc > ec || (kc == ec && kl < el))));
                if (pos >= n_shelf) continue;
                const double uc = __shfl_up(kc, 1, 64), usc = __shfl_up(ksc, 1, 64);
                const int ul = __shfl_up(kl, 1, 64), ur = __shfl_up(kr, 1, 64), uz = __shfl_up(kz, 1, 64);
                if (lane > pos) { kc = uc; ksc = usc; kl = ul; kr = ur; kz = uz; }
                else if (lane == pos) { kc = ec; ksc = esc; kl = el; kr = er; kz = ez; }
                have = have < n_shelf ? have + 1 : n_shelf;
            }
        }
        if (lane < n_shelf) {
            const size_t o = (size_t)(q0 + x) * n_shelf + lane;
            const bool v = lane < have;
            out_label[o] = v ? kl : -1;
            out_sscore[o] = v ? ksc : 0.0;
            out_size[o] = v ? kz : 0;
            out_cnt[o] = v ? (kz < n_top ? kz : n_top) : 0;
            sel_run[(size_t)x * n_shelf + lane] = v ? kr : -1;
        }
        if (lane == 0) {
            out_nshelf[q0 + x] = have;
            if (formed) atomicMax(&st4[3], (unsigned long long)formed);
        }
    }
}

// one wave per slot (x, s) of the chunk: the content of the chosen run, in the layout of a row of xmap_topn_rows
__global__ __launch_bounds__(256) void k_sh_fill(long long n_slots, long long q0, int n_shelf, int n_top, int rank_by, const int *sel_run,
                                                 const int *vals, const int *run_start, const long long *cand_ptr, const int *cand_item,
                                                 const double *plain, const double *decay, int *out_item, double *out_plain,
                                                 double *out_decay) {
    const int lane = lane_id();
    const long long step = (long long)gridDim.x * (blockDim.x / WAVE);
    for (long long t = (long long)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6); t < n_slots; t += step) {
        const int r = sel_run[t];
        if (r < 0) continue;                    // (wave-uniform; the blank slice stands)
        const long long x = t / n_shelf;
        double ks, kp, kd;
        int ki, have;
        sh_select(run_start[r], run_start[r + 1], vals, cand_ptr[q0 + x], cand_item, plain, decay, rank_by, n_top, ks, kp, kd, ki, have);
        if (lane < n_top) {
            const size_t o = ((size_t)q0 * n_shelf + (size_t)t) * n_top + lane;
            const bool v = lane < have;
            out_item[o] = v ? ki : -1;
            out_plain[o] = v ? kp : 0.0;
            out_decay[o] = v ? kd : 0.0;
        }
    }
}

// the outputs of a page without a shelf: the counts and the padding
__global__ __launch_bounds__(256) void k_sh_blank(long long n_query, int n_shelf, int n_top, int *out_nshelf, int *out_label,
                                                  double *out_sscore, int *out_size, int *out_cnt, int *out_item, double *out_plain,
                                                  double *out_decay) {
    const long long n_sh = n_query * n_shelf, total = n_sh * n_top, step = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += step) {
        if (k < n_query) out_nshelf[k] = 0;
        if (k < n_sh) { out_label[k] = -1; out_sscore[k] = 0.0; out_size[k] = 0; out_cnt[k] = 0; }
        out_item[k] = -1; out_plain[k] = 0.0; out_decay[k] = 0.0;
    }
}

static unsigned sh_wave_blocks(long long waves) {
    const long long b = (waves + 3) / 4;
    return (unsigned)(b < 1 ? 1 : b < (long long)SH_MAX_BLOCKS ? b : (long long)SH_MAX_BLOCKS);
}

// rec_model.h: the host checks of the shelf calls, each naming its argument; nothing is written
int shelf_check_args(const char *who, int64_t n_query, int32_t n_shelf, int32_t n_top, int32_t rank_by, int32_t flags, int32_t shelf_by,
                     int32_t min_fill, int32_t n_labels, int64_t max_records) {
#define SH_BAD(cond, ...) do { if (cond) { set_error(__VA_ARGS__); return XMAP_ERR_ARG; } } while (0)
    SH_BAD(n_query < 0 || n_query > (1ll << 28), "%s: n_query = %lld, not in 0 .. 2^28", who, (long long)n_query);
    SH_BAD(n_shelf < 1 || n_shelf > SH_MAX, "%s: n_shelf = %d, not in 1 .. 64", who, n_shelf);
    SH_BAD(n_top < 1 || n_top > SH_MAX, "%s: n_top = %d, not in 1 .. 64", who, n_top);
    SH_BAD(rank_by != 0 && rank_by != 1, "%s: rank_by = %d, not 0 or 1", who, rank_by);
    SH_BAD((flags & ~XMAP_TOPN_KEEP_HELD) != 0, "%s: flags = %d, only XMAP_TOPN_KEEP_HELD is known", who, flags);
    SH_BAD(shelf_by != XMAP_SHELF_BY_BEST && shelf_by != XMAP_SHELF_BY_MEAN && shelf_by != XMAP_SHELF_BY_LABEL,
           "%s: shelf_by = %d, not XMAP_SHELF_BY_BEST, _MEAN or _LABEL", who, shelf_by);
    SH_BAD(min_fill < 1, "%s: min_fill = %d, not >= 1", who, min_fill);
    SH_BAD(n_labels < 1 || n_labels > XMAP_SHELF_MAX_LABELS, "%s: n_labels = %d, not in 1 .. 2^24", who, n_labels);
    SH_BAD(max_records < 0, "%s: max_records = %lld, not >= 0", who, (long long)max_records);
#undef SH_BAD
    return XMAP_OK;
}

// rec_model.h: the device check of a label table over n_items items; *n_lab = lab_ptr[n_items].  Synchronises.
int shelf_check_labels(hipStream_t st, const char *who, int32_t n_items, int32_t n_labels, const int64_t *lab_ptr, const int32_t *lab_id,
                       int64_t *n_lab) {
    XM_SCOPE(st);
    if (!lab_ptr) { set_error("%s: lab_ptr is NULL", who); return XMAP_ERR_ARG; }
    long long total = 0;
    int rc = rf_check_ptr(st, n_items, (const long long *)lab_ptr, who, "lab_ptr", &total);
    if (rc) return rc;
    *n_lab = total;
    if (total == 0) return XMAP_OK;
    if (!lab_id) { set_error("%s: lab_ptr lists %lld labels, lab_id is NULL", who, total); return XMAP_ERR_ARG; }
    unsigned long long *bad = nullptr, h_bad[2] = {RF_NO_POS, RF_NO_POS};
    XM_HIP(xm_malloc_async((void **)&bad, sizeof(h_bad), st));
    XM_HIP(hipMemcpyAsync(bad, h_bad, sizeof(h_bad), hipMemcpyHostToDevice, st));
    const unsigned blocks = blocks_for(n_items, 256) < 4096u ? blocks_for(n_items, 256) : 4096u;
    k_sh_check<<<dim3(blocks), dim3(256), 0, st>>>(n_items, n_labels, (const long long *)lab_ptr, lab_id, bad);
    XM_LAUNCH_CHECK();
    XM_HIP(hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_bad[0] != RF_NO_POS) {
        set_error("%s: lab_id out of range: the first at lab_id[%llu] (every id in [0, n_labels = %d))", who, h_bad[0], n_labels);
        return XMAP_ERR_ARG;
    }
    if (h_bad[1] != RF_NO_POS) {
        set_error("%s: lab_id not strictly ascending inside an item: the first at lab_id[%llu]", who, h_bad[1]);
        return XMAP_ERR_ARG;
    }
    return XMAP_OK;
}

// The back half over scored segments whose tables have passed their checks.  h8 (host): [0] candidates with status != 0, [1] the
// largest segment, [2] candidates below the floor, [3] unused, [4..7] = records, shelves, shelves below min_fill, the most formed
// shelves of one query.  Synchronises.
static int shelf_back(hipStream_t st, int64_t n_query, const long long *cand_ptr, const int *cand_item, const double *plain,
                      const double *decay, const int *status, long long n_cand, double min_score, int I, const ShelfLabels &L,
                      int n_shelf, int n_top, int rank_by, int shelf_by, int min_fill, int64_t max_records, const ShelfOut &O,
                      unsigned long long h8[8]) {
    for (int k = 0; k < 8; k++) h8[k] = 0;
    const long long *lab_ptr = (const long long *)L.lab_ptr;
    const unsigned int *lab_allow = (const unsigned int *)L.lab_allow;
    const size_t nq1 = (size_t)n_query + 1;
    const auto blank = [&]() {
        const unsigned bb = blocks_for((long long)n_query * n_shelf * n_top, 256);
        k_sh_blank<<<dim3(bb < PR_BLANK_BLOCKS ? bb : PR_BLANK_BLOCKS), dim3(256), 0, st>>>(n_query, n_shelf, n_top, O.nshelf, O.label, O.sscore,
                                                                                            O.size, O.cnt, O.item, O.plain, O.decay);
    };
    if (n_cand == 0) {
        blank();
        XM_LAUNCH_CHECK();
        XM_HIP(hipStreamSynchronize(st));
        return XMAP_OK;
    }
    // ---- records per candidate (the outputs are first written once the record counts have passed)
    int *rcnt = nullptr;
    long long *rec_off = nullptr, *qrec = nullptr;
    unsigned long long *st4 = nullptr;          // [0..3] the candidate counters, [4..7] the shelf counters
    XM_HIP(xm_malloc_async((void **)&rcnt, sizeof(int) * (size_t)n_cand, st));
    XM_HIP(xm_malloc_async((void **)&rec_off, sizeof(long long) * ((size_t)n_cand + 1), st));
    XM_HIP(xm_malloc_async((void **)&qrec, sizeof(long long) * nq1, st));
    XM_HIP(xm_malloc_async((void **)&st4, sizeof(unsigned long long) * 8, st));
    XM_HIP(hipMemsetAsync(st4, 0, sizeof(unsigned long long) * 8, st));
    int rc = for_pair_ranges(n_cand, 256, [&](long long base, long long end, dim3 grid) {
        k_sh_count<<<grid, dim3(256), 0, st>>>(base, end, cand_item, plain, decay, status, rank_by, min_score, I, lab_ptr, L.lab_id, lab_allow,
                                               rcnt, st4);
    });
    if (rc) return rc;
    if ((rc = xmap_exclusive_scan_i32_to_i64(st, rcnt, (int64_t *)rec_off, n_cand, nullptr))) return rc;
    k_sh_qrec<<<dim3(blocks_for(n_query + 1, 256)), dim3(256), 0, st>>>(n_query, cand_ptr, rec_off, qrec, st4);
    XM_LAUNCH_CHECK();
    RecordChunks C;
    C.rec.resize(nq1);
    std::vector<long long> h_cptr(nq1);
    XM_HIP(hipMemcpyAsync(C.rec.data(), qrec, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(h_cptr.data(), cand_ptr, sizeof(long long) * nq1, hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    // ---- the chunks; the shelves' own condition on the query that opens a chunk: its candidates too number fewer than 2^31
    if ((rc = pr_plan_chunks("shelves", n_query, max_records, PR_MAX_RECORDS, &C))) return rc;
    for (size_t k = 0; k + 1 < C.cut.size(); k++) {
        const long long q0 = C.cut[k];
        if (h_cptr[q0 + 1] - h_cptr[q0] >= 2147483647ll) {
            set_error("shelves: query %lld has %lld candidates, a chunk holds fewer than 2^31", q0, h_cptr[q0 + 1] - h_cptr[q0]);
            return XMAP_ERR_CAPACITY;
        }
    }
    blank();
    XM_LAUNCH_CHECK();
    if (C.n_max > 0) {
        const int label_bits = bits_for(L.n_labels);
        RunTables T;
        int *sel_run = nullptr;
        double *r_score = nullptr;
        if ((rc = pr_alloc_runs(st, C.n_max, C.nq_max, label_bits, true, &T))) return rc;
        XM_HIP(xm_malloc_async((void **)&r_score, sizeof(double) * (size_t)C.n_max, st));
        XM_HIP(xm_malloc_async((void **)&sel_run, sizeof(int) * (size_t)C.nq_max * n_shelf, st));
        rc = pr_each_chunk(C, [&](long long q0, long long q1, long long n) {
            const long long nq = q1 - q0, c0 = h_cptr[q0];
            int rc = for_pair_ranges(h_cptr[q1] - c0, 256, [&](long long base, long long end, dim3 grid) {  // candidates [base, end) of the chunk
                k_sh_expand<<<grid, dim3(256), 0, st>>>(c0 + base, c0 + end, C.rec[q0], q0, n_query, cand_ptr, cand_item, plain, decay, status,
                                                        rank_by, min_score, I, lab_ptr, L.lab_id, lab_allow, rec_off, label_bits, T.keys, T.vals);
            });
            if (rc || (rc = pr_run_tables(st, T, n, nq, label_bits))) return rc;
            k_sh_runs<<<dim3(sh_wave_blocks(n)), dim3(256), 0, st>>>(n, q0, T.keys, T.vals, T.run_idx, T.run_start, label_bits, cand_ptr, cand_item,
                                                                     plain, decay, rank_by, n_top, shelf_by, min_fill, r_score, st4 + 4);
            XM_LAUNCH_CHECK();
            k_sh_pick<<<dim3(sh_wave_blocks(nq)), dim3(256), 0, st>>>(nq, q0, n_shelf, n_top, shelf_by, min_fill, T.first, T.keys, T.run_start,
                                                                      label_bits, r_score, sel_run, O.nshelf, O.label, O.sscore, O.size, O.cnt,
                                                                      st4 + 4);
            XM_LAUNCH_CHECK();
            k_sh_fill<<<dim3(sh_wave_blocks(nq * n_shelf)), dim3(256), 0, st>>>(nq * n_shelf, q0, n_shelf, n_top, rank_by, sel_run, T.vals,
                                                                                T.run_start, cand_ptr, cand_item, plain, decay, O.item, O.plain,
                                                                                O.decay);
            XM_LAUNCH_CHECK();
            return XMAP_OK;
        });
        if (rc) return rc;
    }
    XM_HIP(hipMemcpyAsync(h8, st4, sizeof(unsigned long long) * 8, hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    h8[4] = (unsigned long long)C.rec[n_query];
    return XMAP_OK;
}

static int shelf_check_out(const char *who, int64_t n_query, const ShelfOut &O) {
    if (n_query > 0 && !(O.nshelf && O.label && O.sscore && O.size && O.cnt && O.item && O.plain && O.decay)) {
        set_error("%s: an output is NULL", who);
        return XMAP_ERR_ARG;
    }
    return XMAP_OK;
}

// rec_model.h: xmap_shelf_rows
int shelf_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags, const RecModel &M,
               const ShelfLabels &L, int32_t n_shelf, int32_t shelf_by, int32_t min_fill, int64_t max_records, const ShelfOut &O,
               const xmap_rec_filter *F, int64_t *h_stats) {
    const char *who = "xmap_shelf_rows";
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    int rc = shelf_check_args(who, n_query, n_shelf, n_top, rank_by, flags, shelf_by, min_fill, L.n_labels, max_records);
    if (rc) return rc;
    if ((rc = rec_model_check(M))) return rc;
    XM_ARG(n_query == 0 || query_user);
    if ((rc = shelf_check_out(who, n_query, O))) return rc;
    bool filt = false;
    double min_score = 0.0;
    if ((rc = rf_prepare(st, n_query, F, &filt, &min_score))) return rc;
    if (n_query == 0) {
        if (h_stats) for (int k = 0; k < 10; k++) h_stats[k] = 0;
        return XMAP_OK;
    }
    int64_t n_lab = 0;
    if ((rc = shelf_check_labels(st, who, M.n_items, L.n_labels, L.lab_ptr, L.lab_id, &n_lab))) return rc;
    if (h_stats) for (int k = 0; k < 10; k++) h_stats[k] = 0;
    unsigned long long *removed = nullptr;
    XM_HIP(xm_malloc_async((void **)&removed, sizeof(unsigned long long), st));
    XM_HIP(hipMemsetAsync(removed, 0, sizeof(unsigned long long), st));
    TnScored S;
    rc = tn_score_candidates(st, n_query, query_user, flags, M, filt, filt ? (const unsigned int *)F->allow : nullptr,
                             filt ? (const long long *)F->ex_ptr : nullptr, filt ? F->ex_id : nullptr, removed, &S);
    if (rc) return rc;
    unsigned long long h8[8], h_removed = 0;
    rc = shelf_back(st, n_query, S.cand_ptr, S.cand_item, S.plain, S.decay, S.status, S.n_pairs, min_score, M.n_items, L, n_shelf, n_top, rank_by,
                    shelf_by, min_fill, max_records, O, h8);
    if (rc) return rc;
    XM_HIP(hipMemcpyAsync(&h_removed, removed, sizeof(h_removed), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (h_stats) {
        h_stats[0] = S.n_pairs; h_stats[1] = (int64_t)h8[0]; h_stats[2] = S.max_now; h_stats[3] = (int64_t)h8[1];
        h_stats[4] = (int64_t)h8[2]; h_stats[5] = (int64_t)h_removed;
        for (int k = 0; k < 4; k++) h_stats[6 + k] = (int64_t)h8[4 + k];
    }
    return XMAP_OK;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_shelf_segments(void *stream, int64_t n_query, const int64_t *cand_ptr, const int32_t *cand_item, const double *plain,
                        const double *decay, const int32_t *status, double min_score, int32_t n_items, int32_t n_labels,
                        const int64_t *lab_ptr, const int32_t *lab_id, const uint32_t *lab_allow, int32_t n_shelf, int32_t n_top,
                        int32_t rank_by, int32_t shelf_by, int32_t min_fill, int64_t max_records, int32_t *out_nshelf, int32_t *out_label,
                        double *out_sscore, int32_t *out_size, int32_t *out_cnt, int32_t *out_item, double *out_plain, double *out_decay,
                        int64_t *h_stats) {
    const char *who = "xmap_shelf_segments";
    hipStream_t st = (hipStream_t)stream;
    XM_SCOPE(st);
    const ShelfLabels L{n_labels, lab_ptr, lab_id, lab_allow};
    const ShelfOut O{out_nshelf, out_label, out_sscore, out_size, out_cnt, out_item, out_plain, out_decay};
    // the host checks: before any device work
    int rc = shelf_check_args(who, n_query, n_shelf, n_top, rank_by, 0, shelf_by, min_fill, n_labels, max_records);
    if (rc) return rc;
    if (min_score != min_score) { set_error("%s: min_score is NaN", who); return XMAP_ERR_ARG; }
    if (n_items < 0) { set_error("%s: n_items = %d, not >= 0", who, n_items); return XMAP_ERR_ARG; }
    if (n_query > 0 && !cand_ptr) { set_error("%s: cand_ptr is NULL", who); return XMAP_ERR_ARG; }
    if ((rc = shelf_check_out(who, n_query, O))) return rc;
    if (n_query == 0) {
        if (h_stats) for (int k = 0; k < 4; k++) h_stats[k] = 0;
        return XMAP_OK;
    }
    // ---- the pointer tables and the labels on the device: nothing is indexed through one that fails, no output is written
    long long n_cand = 0;
    if ((rc = rf_check_ptr(st, n_query, (const long long *)cand_ptr, who, "cand_ptr", &n_cand))) return rc;
    if (n_cand > 0 && !(cand_item && plain && decay && status)) {
        set_error("%s: cand_ptr lists %lld candidates, a candidate column is NULL", who, n_cand);
        return XMAP_ERR_ARG;
    }
    int64_t n_lab = 0;
    if ((rc = shelf_check_labels(st, who, n_items, n_labels, lab_ptr, lab_id, &n_lab))) return rc;
    unsigned long long h8[8];
    rc = shelf_back(st, n_query, (const long long *)cand_ptr, cand_item, plain, decay, status, n_cand, min_score, n_items, L, n_shelf, n_top,
                    rank_by, shelf_by, min_fill, max_records, O, h8);
    if (rc) return rc;
    if (h_stats) for (int k = 0; k < 4; k++) h_stats[k] = (int64_t)h8[4 + k];
    return XMAP_OK;
}

int xmap_shelf_rows(void *stream, int64_t n_query, const int32_t *query_user, int32_t n_top, int32_t rank_by, int32_t flags,
                    int64_t n_users, int32_t n_items, int32_t keep, const int32_t *nb_cnt, const int32_t *nb_col, const double *nb_sim,
                    const int64_t *prof_ptr, const int32_t *prof_item, const double *prof_rating, const int64_t *prof_time,
                    const double *item_avg, const double *wtab, int32_t n_w, int32_t n_labels, const int64_t *lab_ptr,
                    const int32_t *lab_id, const uint32_t *lab_allow, int32_t n_shelf, int32_t shelf_by, int32_t min_fill,
                    int64_t max_records, int32_t *out_nshelf, int32_t *out_label, double *out_sscore, int32_t *out_size, int32_t *out_cnt,
                    int32_t *out_item, double *out_plain, double *out_decay, const xmap_rec_filter *F, int64_t *h_stats) {
    const RecModel M{n_users, n_items, keep, nb_cnt, nb_col, nb_sim, prof_ptr, prof_item, prof_rating, prof_time, item_avg, wtab, n_w};
    return shelf_rows(stream, n_query, query_user, n_top, rank_by, flags, M, ShelfLabels{n_labels, lab_ptr, lab_id, lab_allow}, n_shelf,
                      shelf_by, min_fill, max_records,
                      ShelfOut{out_nshelf, out_label, out_sscore, out_size, out_cnt, out_item, out_plain, out_decay}, F, h_stats);
}
}
