// reverse.hip -- stage B: the reverse adjacencies of the knn tables (attach / src / rnn; core/extender.py:48-81,142-178),
// built in row order with an O(1) membership test against the k-th entry of the neighbour's list.  The count pass (attach +
// rnn together) leaves a byte per entry, the fill passes read it (bound by the CU's gather rate).
//
// Kernels:
//   k_reverse<FILL>      : rows up to rev_long entries, one wave per row
//   k_rev_long_rows      : lists the longer rows
//   k_reverse_long<FILL> : the long rows, 16 waves per row
// Entry points: xmap_reverse_count, xmap_reverse_count_att_rnn, xmap_reverse_fill (all through reverse_common).
#include "paths.h"
#include <stdlib.h>

namespace xmap {

struct RevArgs {
    int I, k, mode;
    int row_lo, row_hi;          // the rows (= targets of the reverse lists) of this call: a rank's share, or [0, I)
    const KnnThr *thr;
    const int *long_rows;        // [0] = count, then the rows with more than rev_long entries (or NULL)
    uint8_t *eflag;              // per entry of the rows [row_lo, row_hi) (index p - row_ptr[row_lo]), or NULL: the count pass leaves
                                 // bit 0 = "b lists a", bit 1 = joint here and the fill pass reads it instead of testing again
    int rev_long;
    const long long *row_ptr;
    const int *col;
    const double *sim;
    const int *mutu;
    const int *nij;
    const double *info;
    const double *frac;
    const uint8_t *bb;
    const uint8_t *cls;
    const int *kcnt;
    const int *kcol;
    const double *kval;
    const int *suffix_cls;
    const uint32_t *contains_mask;
    const uint8_t *flags;
    const long long *attach_ptr;
    int *rcnt;
    int *rcnt2;                  // mode 3 (attach and rnn lists counted in ONE pass over the rows): the rnn counts
    const long long *rptr;
    int *ridx;
    double *rval;
    uint8_t *rflag;
};

// membership of item a in list l of neighbour b, given |sim(a,b)| (bit-symmetric by construction):
// a is in the list iff it passes the list's class predicate and sorts at or before the list's
// last entry in the order (|sim| desc, col asc) -- or the list is not full.
__device__ __forceinline__ bool in_list(const RevArgs &A, int b, int l, int a, double abs_sim) {
    KnnThr th;
    th.cnt = 0; th.col = 0; th.la = 0.0;
    if (A.thr) th = A.thr[(size_t)b * 2 + l];        // one 16-byte gather instead of count, last value, last column
    int c = A.thr ? th.cnt : A.kcnt[(size_t)b * 2 + l];
    if (c == 0) return false;
    bool pred;
    if (A.cls[b] == 1) {
        bool has = (A.contains_mask[a] >> A.suffix_cls[b]) & 1u;
        pred = (l == 0) ? !has : has;
    } else {
        pred = (l == 0) ? (A.bb[a] != 0) : true;
    }
    if (!pred) return false;
    if (c < A.k) return true;
    if (A.thr) return (abs_sim > th.la) || (abs_sim == th.la && a <= th.col);
    size_t o = ((size_t)b * 2 + l) * A.k + (c - 1);
    double la = fabs(A.kval[o * 3]);
    return (abs_sim > la) || (abs_sim == la && a <= A.kcol[o]);
}

// one entry p of row a: does b = col[p] list a?  (mode 0 attach, 1 src, 2 rnn; fl: the (t,s) is joint)
__device__ __forceinline__ bool rev_entry(const RevArgs &A, int a, long long p, long long hi, int &b, double &sv, uint8_t &fl) {
    bool ok = false;
    b = 0; sv = 0.0; fl = 0;
    if (p < hi) {
        b = A.col[p];
        sv = A.sim[p];
        double ab = fabs(sv);
        int cb = A.cls[b];     // (a 1-byte gather from a 400 KB table; the 16-byte threshold record only for the entries that pass it --
                               //  packing the class into that record made EVERY entry gather it: 6.7 -> 8.3 ms, round 4)
        if (A.mode == 0) {           // attach(a): x = b non-bridge record with a in NB_BB(x)
            ok = (cb == 2) && in_list(A, b, 0, a, ab);
        } else if (A.mode == 1) {    // src(t = a): s = b
            // (the three per-item tests packed into one byte table, one gather instead of up to three: 5.2 ms either way, round 4)
            ok = (cb == 1) && (A.flags[b] & 1) && (A.attach_ptr[b + 1] > A.attach_ptr[b]) &&
                 (in_list(A, b, 0, a, ab) || in_list(A, b, 1, a, ab));
            if (ok) {
                bool joint = (A.cls[a] == 1) && (A.attach_ptr[a + 1] > A.attach_ptr[a]) &&
                             (in_list(A, a, 0, b, ab) || in_list(A, a, 1, b, ab));
                fl = joint ? 1 : 0;
            }
        } else if (A.mode == 3) {    // attach and rnn together (count pass only): ok = attach, fl bit 1 = rnn (eflag bit 2)
            if (cb == 2) { ok = in_list(A, b, 0, a, ab); if (in_list(A, b, 1, a, ab)) fl = 2; }
        } else {                     // rnn(y = a): x = b non-bridge record with a in NB_NN(x)
            ok = (cb == 2) && in_list(A, b, 1, a, ab);
        }
    }
    return ok;
}
__device__ __forceinline__ void rev_write(const RevArgs &A, int a, long long p, long long o, int b, double sv, uint8_t fl) {
    double mu = (double)A.mutu[p];
    A.ridx[o] = b;
    A.rval[o * 3] = sv;
    A.rval[o * 3 + 1] = mu;
    A.rval[o * 3 + 2] = A.frac ? A.frac[p] : 1.0 * mu / (A.info[(size_t)a * 4 + 3] + A.info[(size_t)b * 4 + 3] - (double)A.nij[p]);
    if (A.rflag) A.rflag[o] = fl;
}

// The test of one entry, once: the count pass evaluates it (a 1-byte class gather per entry, a 16-byte threshold gather for
// those that pass: the passes run at the CU's rate of random gathers, not at the matrix's bandwidth) and, given A.eflag, leaves
// the outcome as a byte per entry; the fill pass then streams the bytes and touches only the entries it writes.
template <bool FILL>
__device__ __forceinline__ bool rev_test(const RevArgs &A, int a, long long p, long long hi, long long p0, int &b, double &sv,
                                         uint8_t &fl) {
    if (!A.eflag) return rev_entry(A, a, p, hi, b, sv, fl);
    if (!FILL) {
        const bool ok = rev_entry(A, a, p, hi, b, sv, fl);
        // (bit 0 = attach / src, bit 1 = joint (src), bit 2 = rnn: a fused count serves the fill passes of both of its lists)
        if (p < hi) A.eflag[p - p0] = (uint8_t)((ok ? (A.mode == 2 ? 4 : 1) : 0) | (fl << 1));
        return ok;
    }
    b = 0; sv = 0.0; fl = 0;
    bool ok = false;
    if (p < hi) {
        const uint8_t e = A.eflag[p - p0];
        ok = (e & (A.mode == 2 ? 4 : 1)) != 0;
        fl = (uint8_t)((e >> 1) & 1);
        if (ok) { b = A.col[p]; sv = A.sim[p]; }
    }
    return ok;
}

// Rows up to REV_LONG entries: one wave per row.  The rows of the popular items have 10^5 entries and more; walked by
// one wave each they were the whole duration of the pass (5 ms per pass for 0.2 ms of streaming): those rows are listed
// (k_rev_long_rows) and walked by blocks of 16 waves, 1024 entries per step, in the same (row) order.
constexpr int REV_LONG = 4096;      // default of RevArgs::rev_long (XMAP_REV_LONG overrides it: tests walk every row both ways)
constexpr int REV_WAVES = 16;
template <bool FILL>
__global__ __launch_bounds__(256) void k_reverse(RevArgs A) {
    int a = A.row_lo + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= A.row_hi) return;
    int lane = lane_id();
    long long lo = A.row_ptr[a], hi = A.row_ptr[a + 1];
    if (A.long_rows && hi - lo > A.rev_long) return;
    bool row_ok = true;
    if (A.mode == 1) row_ok = (A.flags[a] & 2) != 0;  // "T:" in t
    long long out = FILL ? A.rptr[a] : 0;
    int total = 0, total2 = 0;
    const long long p0 = A.eflag ? A.row_ptr[A.row_lo] : 0;
    if (row_ok)
        for (long long base = lo; base < hi; base += 64) {
            long long p = base + lane;
            int b; double sv; uint8_t fl;
            const bool ok = rev_test<FILL>(A, a, p, hi, p0, b, sv, fl);
            unsigned long long m = __ballot(ok);
            if (FILL && ok) rev_write(A, a, p, out + __popcll(m & lanemask_lt()), b, sv, fl);
            int c = __popcll(m);
            out += c;
            total += c;
            if (!FILL && A.mode == 3) total2 += __popcll(__ballot((fl & 2) != 0));
        }
    if (!FILL && lane == 0) { A.rcnt[a] = total; if (A.mode == 3) A.rcnt2[a] = total2; }
}

__global__ __launch_bounds__(256) void k_rev_long_rows(int row_lo, int row_hi, const long long *row_ptr, int rev_long,
                                                       int *long_rows /*[0] = count*/) {
    const int a = row_lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (a < row_hi && row_ptr[a + 1] - row_ptr[a] > rev_long) long_rows[1 + atomicAdd(&long_rows[0], 1)] = a;
}

template <bool FILL>
__global__ __launch_bounds__(64 * REV_WAVES) void k_reverse_long(RevArgs A) {
    __shared__ int s_cnt[REV_WAVES];
    __shared__ int s_tot2;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int n_long = A.long_rows[0];
    const long long p0 = A.eflag ? A.row_ptr[A.row_lo] : 0;
    for (int r = blockIdx.x; r < n_long; r += gridDim.x) {
        const int a = A.long_rows[1 + r];
        const long long lo = A.row_ptr[a], hi = A.row_ptr[a + 1];
        const bool row_ok = (A.mode != 1) || ((A.flags[a] & 2) != 0);
        long long out = FILL ? A.rptr[a] : 0;
        int total = 0, total2 = 0;
        if (!FILL && A.mode == 3) { if (threadIdx.x == 0) s_tot2 = 0; __syncthreads(); }
        if (row_ok)
            for (long long base = lo; base < hi; base += 64 * REV_WAVES) {
                const long long p = base + threadIdx.x;
                int b; double sv; uint8_t fl;
                const bool ok = rev_test<FILL>(A, a, p, hi, p0, b, sv, fl);
                const unsigned long long m = __ballot(ok);
                if (!FILL && A.mode == 3) total2 += __popcll(__ballot((fl & 2) != 0));      // (this wave's rnn entries)
                if (lane == 0) s_cnt[w] = __popcll(m);
                __syncthreads();
                int before = 0, all = 0;
                for (int o = 0; o < REV_WAVES; o++) { const int c = s_cnt[o]; if (o < w) before += c; all += c; }
                if (FILL && ok) rev_write(A, a, p, out + before + __popcll(m & lanemask_lt()), b, sv, fl);
                out += all;
                total += all;
                __syncthreads();
            }
        if (!FILL && A.mode == 3) {
            if (lane == 0) atomicAdd(&s_tot2, total2);
            __syncthreads();
            if (threadIdx.x == 0) A.rcnt2[a] = s_tot2;
            __syncthreads();
        }
        if (!FILL && threadIdx.x == 0) A.rcnt[a] = total;
    }
}

}  // namespace xmap

using namespace xmap;

extern "C" {

static int reverse_common(void *stream, bool fill, const xmap_sim *S, int mode, int top_k, const uint8_t *bb,
                          const uint8_t *cls, const int32_t *kcnt, const int32_t *kcol, const double *kval,
                          const int32_t *suffix_cls, const uint32_t *contains_mask, const uint8_t *flags,
                          const int64_t *attach_ptr, const void *thr, int32_t *long_rows, uint8_t *eflag, int32_t *rcnt,
                          const int64_t *rptr, int32_t *ridx, double *rval, uint8_t *rflag, int32_t row_lo, int32_t row_hi,
                          int32_t *rcnt2 = nullptr) {
    XM_ARG(S && bb && cls && kcnt && kcol && kval && suffix_cls && contains_mask && flags);
    XM_ARG((mode >= 0 && mode <= 2) || (mode == 3 && !fill && rcnt2 && eflag));
    XM_ARG(mode != 1 || attach_ptr);
    XM_ARG(row_lo >= 0 && row_lo <= row_hi && row_hi <= S->n_items);
    if (row_hi == row_lo) return XMAP_OK;
    RevArgs A;
    A.I = S->n_items; A.k = top_k; A.mode = mode; A.thr = (const KnnThr *)thr; A.long_rows = long_rows; A.eflag = eflag;
    A.row_lo = row_lo; A.row_hi = row_hi;
    const char *rl = getenv("XMAP_REV_LONG");
    A.rev_long = (rl && atoi(rl) > 0) ? atoi(rl) : REV_LONG;
    A.row_ptr = (const long long *)S->row_ptr; A.col = S->col; A.sim = S->sim; A.mutu = S->mutu; A.nij = S->nij;
    A.info = S->info; A.frac = S->frac; A.bb = bb; A.cls = cls; A.kcnt = kcnt; A.kcol = kcol; A.kval = kval;
    A.suffix_cls = suffix_cls; A.contains_mask = contains_mask; A.flags = flags;
    A.attach_ptr = (const long long *)attach_ptr;
    A.rcnt2 = rcnt2;
    A.rcnt = rcnt; A.rptr = (const long long *)rptr; A.ridx = ridx; A.rval = rval; A.rflag = rflag;
    const int n_rows = row_hi - row_lo;
    dim3 grid((unsigned)((n_rows + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;

    if (long_rows && !fill) {     // the count pass lists the long rows, the fill pass that follows reuses the list
        XM_HIP(hipMemsetAsync(long_rows, 0, sizeof(int32_t), st));
        k_rev_long_rows<<<dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st>>>(row_lo, row_hi, (const long long *)S->row_ptr,
                                                                                  A.rev_long, long_rows);
        XM_LAUNCH_CHECK();
    }
    if (fill) k_reverse<true><<<grid, block, 0, st>>>(A);
    else k_reverse<false><<<grid, block, 0, st>>>(A);
    XM_LAUNCH_CHECK();
    if (long_rows) {
        if (fill) k_reverse_long<true><<<dim3(512), dim3(64 * REV_WAVES), 0, st>>>(A);
        else k_reverse_long<false><<<dim3(512), dim3(64 * REV_WAVES), 0, st>>>(A);
        XM_LAUNCH_CHECK();
    }
    return XMAP_OK;
}

int xmap_reverse_count(void *stream, const xmap_sim *S, int mode, int top_k, const uint8_t *bb, const uint8_t *cls,
                       const int32_t *kcnt, const int32_t *kcol, const double *kval, const int32_t *suffix_cls,
                       const uint32_t *contains_mask, const uint8_t *flags, const int64_t *attach_ptr, const void *thr,
                       int32_t *long_rows, uint8_t *eflag, int32_t *rcnt, int32_t row_lo, int32_t row_hi) {
    XM_ARG(rcnt);
    return reverse_common(stream, false, S, mode, top_k, bb, cls, kcnt, kcol, kval, suffix_cls, contains_mask, flags,
                          attach_ptr, thr, long_rows, eflag, rcnt, nullptr, nullptr, nullptr, nullptr, row_lo, row_hi);
}

int xmap_reverse_count_att_rnn(void *stream, const xmap_sim *S, int top_k, const uint8_t *bb, const uint8_t *cls,
                               const int32_t *kcnt, const int32_t *kcol, const double *kval, const int32_t *suffix_cls,
                               const uint32_t *contains_mask, const uint8_t *flags, const void *thr, int32_t *long_rows,
                               uint8_t *eflag, int32_t *rcnt_att, int32_t *rcnt_rnn, int32_t row_lo, int32_t row_hi) {
    XM_ARG(rcnt_att && rcnt_rnn && eflag);
    return reverse_common(stream, false, S, 3, top_k, bb, cls, kcnt, kcol, kval, suffix_cls, contains_mask, flags, nullptr, thr,
                          long_rows, eflag, rcnt_att, nullptr, nullptr, nullptr, nullptr, row_lo, row_hi, rcnt_rnn);
}

int xmap_reverse_fill(void *stream, const xmap_sim *S, int mode, int top_k, const uint8_t *bb, const uint8_t *cls,
                      const int32_t *kcnt, const int32_t *kcol, const double *kval, const int32_t *suffix_cls,
                      const uint32_t *contains_mask, const uint8_t *flags, const int64_t *attach_ptr, const void *thr,
                      int32_t *long_rows, uint8_t *eflag, const int64_t *rptr, int32_t *ridx, double *rval, uint8_t *rflag,
                      int32_t row_lo, int32_t row_hi) {
    XM_ARG(rptr && ridx && rval);
    return reverse_common(stream, true, S, mode, top_k, bb, cls, kcnt, kcol, kval, suffix_cls, contains_mask, flags,
                          attach_ptr, thr, long_rows, eflag, nullptr, rptr, ridx, rval, rflag, row_lo, row_hi);
}

}
