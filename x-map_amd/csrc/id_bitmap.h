// id_bitmap.h -- the windowed LDS bitmap of an id space that the three candidate passes share: k_tn_candidates
// (stage_e_topn.hip), k_au_candidates (stage_e_audience.hip) and k_gr_candidates (stage_e_group.hip).  A block holds the
// candidate set of one query as a bitmap of WINDOW consecutive ids, walks the id space window by window, and lets the set
// leave in ascending id.  A second level -- one bit per bitmap word that was touched -- is all the emit step scans, and it
// zeroes exactly the words it visits: the window is cleared once per block, never per query.
//
// A kernel keeps what is its own: the query loop, the mark loop, the un-mark of what the query holds, and the writer.  Per window:
//     mark(id - lo) ...; __syncthreads();  unmark(id - lo) ...; __syncthreads();  exclude<...>(...);  total += emit<...>(...);
// The eligibility rules (rec_filter.h) act here: exclude() clears the query's exclusion ids, and emit() -- the ONLY reader of
// the summary -- takes every touched word through rf_eligible in the count instantiation and in the fill instantiation alike,
// so the two cannot disagree about what a buffer of exactly the counted size has to hold.
#ifndef XMAP_ID_BITMAP_H
#define XMAP_ID_BITMAP_H
#include "common.h"
#include "rec_filter.h"

namespace xmap {

// exclusive scan of v over the THREADS threads of the block, *total = the block's sum; smem: THREADS / 64 ints
template <int THREADS>
__device__ __forceinline__ int block_scan(int v, int *total, int *smem) {
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
    for (int k = 0; k < THREADS / 64; k++) {
        const int s = smem[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

template <int THREADS, int WINDOW_LOG2>
struct IdBitmap {
    static constexpr int WINDOW = 1 << WINDOW_LOG2;     // ids per pass
    static constexpr int WORDS = WINDOW / 32;
    static constexpr int SUMMARY = WORDS / 32;          // second level: bit w of word s = bitmap word 32 s + w was touched
    static constexpr int PER = SUMMARY / THREADS;       // summary words a thread emits (consecutive: thread order = id order)
    static constexpr size_t LDS_BYTES = sizeof(unsigned int) * (WORDS + SUMMARY + THREADS / 64);    // bitmap, summary, scan scratch
    static_assert(PER >= 1 && PER * THREADS == SUMMARY, "every thread emits the same number of summary words");

    unsigned int *bits, *summ;          // [WORDS], [SUMMARY]: all zero between two queries
    int *scan;                          // [THREADS / 64]
    unsigned int gone = 0;              // count pass: candidates of this thread's ids and words that the rules removed

    // over the block's dynamic LDS (LDS_BYTES of it); clears the window, once per block
    __device__ __forceinline__ explicit IdBitmap(unsigned int *lds) : bits(lds), summ(lds + WORDS), scan((int *)(lds + WORDS + SUMMARY)) {
        for (int k = threadIdx.x; k < WORDS + SUMMARY; k += THREADS) lds[k] = 0u;
        __syncthreads();
    }

    // x = id - first id of the window; ids of another window are passed over
    __device__ __forceinline__ void mark(long long x) {
        if (x < 0 || x >= WINDOW) return;
        const int w = (int)(x >> 5);
        const unsigned int old = atomicOr(&bits[w], 1u << (x & 31));
        if (old == 0u) atomicOr(&summ[w >> 5], 1u << (w & 31));
    }
    // (the word stays listed as touched)
    __device__ __forceinline__ void unmark(long long x) {
        if (x >= 0 && x < WINDOW) atomicAnd(&bits[x >> 5], ~(1u << (x & 31)));
    }

    // The exclusion list of query q (ex_ptr may be NULL: no lists) over an id space of n ids, behind the un-mark: the block strides
    // the list and clears the ids of the window [lo, lo + WINDOW).  COUNT: a bit that was still set is a candidate removed, once.
    template <bool COUNT>
    __device__ __forceinline__ void exclude(const long long *ex_ptr, const int *ex_id, long long q, long long n, long long lo) {
        if (!ex_ptr) return;
        const long long e1 = ex_ptr[q + 1];
        for (long long e = ex_ptr[q] + threadIdx.x; e < e1; e += THREADS) {
            const long long id = ex_id[e], x = id - lo;
            if (id < 0 || id >= n || x < 0 || x >= WINDOW) continue;
            const unsigned int bit = 1u << (x & 31);
            const unsigned int old = atomicAnd(&bits[x >> 5], ~bit);
            if constexpr (COUNT) gone += (old & bit) ? 1u : 0u;
        }
        __syncthreads();
    }

    // The window leaves in ascending id: count per thread, scan over the block, write; the visited words are zeroed on the way.
    // Returns the eligible ids of the window.  FILL: write(out + rank in the window, id) for each of them; the count
    // instantiation writes nothing.  FILT: a touched word meets its word of the mask `allow` (rf_eligible; FILT = false reads
    // no mask).  COUNT_MASKED: the count instantiation adds what the mask removed to `gone`.
    template <bool FILL, bool FILT, bool COUNT_MASKED, class Write>
    __device__ __forceinline__ int emit(long long lo, const unsigned int *allow, long long out, Write write) {
        const int tid = threadIdx.x;
        int c = 0;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            unsigned int sw = summ[tid * PER + k];
            while (sw) {
                const int w = (tid * PER + k) * 32 + __ffs(sw) - 1;
                sw &= sw - 1;
                const unsigned int raw = bits[w], bw = rf_eligible<FILT>(raw, allow, (lo >> 5) + w);
                c += __popc(bw);
                if constexpr (COUNT_MASKED && !FILL) gone += __popc(raw) - __popc(bw);
            }
        }
        int tot;
        [[maybe_unused]] long long o = out + block_scan<THREADS>(c, &tot, scan);
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int s = tid * PER + k;
            unsigned int sw = summ[s];
            if (sw == 0u) continue;
            summ[s] = 0u;
            while (sw) {
                const int w = s * 32 + __ffs(sw) - 1;
                sw &= sw - 1;
                [[maybe_unused]] unsigned int bw = bits[w];
                bits[w] = 0u;
                if constexpr (FILL) {
                    bw = rf_eligible<FILT>(bw, allow, (lo >> 5) + w);
                    while (bw) {
                        const int bit = __ffs(bw) - 1;
                        bw &= bw - 1;
                        write(o++, lo + (long long)w * 32 + bit);
                    }
                }
            }
        }
        __syncthreads();
        return tot;
    }

    // the count pass, at the end of the block: *removed += what the rules removed from this thread's ids and words
    __device__ __forceinline__ void add_gone(unsigned long long *removed) const {
        if (gone) atomicAdd(removed, (unsigned long long)gone);
    }
};

}  // namespace xmap
#endif
