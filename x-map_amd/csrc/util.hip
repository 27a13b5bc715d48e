// util.hip -- error plumbing and the prefix sums every count->fill pair needs.
#include <stdarg.h>
#include <stdlib.h>
#include <vector>

#include "common.h"

namespace xmap {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- temporaries of the library ----------------------------------------------------------------------------------------
// Scratch that lives for one entry-point call (scan tile sums, sort histograms, planning arrays, the column end table).
// Round 1 took it from the stream-ordered allocator (hipMallocAsync / hipFreeAsync).  Under the ROCm 7.2 runtime of this
// image that gave wrong results from the second pass of a process on (a block handed out again while kernels of the
// same stream still read it; not with the 7.0 runtime PyTorch bundles -- INTEGRATION.md, "HIP runtime versions"), so
// the library keeps its own arenas instead: one per (thread, device, stream), bump allocation inside a call, everything
// recycled when the last temporary of the call is released.  Reuse is ordered by the stream itself: a later call on the
// same stream runs after the kernels of the earlier one.
namespace {
struct Chunk { char *base; size_t size, used; };
struct Arena { int dev; hipStream_t st; std::vector<Chunk> chunks; size_t live; };
thread_local std::vector<Arena> g_arenas;
// What an idle arena may keep: chunks beyond this are handed back to the driver when the arena resets (high-water
// temporaries -- the 24 B/record buffers of the partial-record sort, the column end table -- would otherwise stay pinned
// outside the caller's allocator for the life of the process).
constexpr size_t ARENA_KEEP = (size_t)256 << 20;
Arena *arena_find(int dev, hipStream_t st) {
    for (Arena &a : g_arenas) if (a.dev == dev && a.st == st) return &a;
    return nullptr;
}
Arena *arena_of(hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    if (Arena *a = arena_find(dev, st)) return a;
    g_arenas.push_back(Arena{dev, st, {}, 0});
    return &g_arenas.back();
}
// all temporaries released: recycle the chunks; beyond ARENA_KEEP they go back to the driver (after the stream has
// drained: a kernel of this call may still be reading them)
void arena_reset(Arena *a) {
    size_t total = 0;
    for (Chunk &c : a->chunks) { c.used = 0; total += c.size; }
    if (total <= ARENA_KEEP) return;
    if (hipStreamSynchronize(a->st) != hipSuccess) return;
    // keep the smallest chunks up to the cap, free the rest (largest first)
    std::vector<Chunk> keep;
    size_t kept = 0;
    std::vector<Chunk> all = a->chunks;
    for (size_t i = 0; i < all.size(); i++)
        for (size_t j = i + 1; j < all.size(); j++)
            if (all[j].size < all[i].size) { Chunk t = all[i]; all[i] = all[j]; all[j] = t; }
    for (Chunk &c : all) {
        if (kept + c.size <= ARENA_KEEP) { keep.push_back(c); kept += c.size; }
        else (void)hipFree(c.base);
    }
    a->chunks.swap(keep);
}
}  // namespace

XmScope::XmScope(hipStream_t s) : dev(0), st(s), live0(0), ok(false) {
    if (hipGetDevice(&dev) != hipSuccess) return;
    ok = true;
    if (Arena *a = arena_find(dev, st)) live0 = a->live;
}
XmScope::~XmScope() {
    if (!ok) return;
    Arena *a = arena_find(dev, st);       // (looked up again: a nested call on another stream may have grown the vector)
    if (!a || a->live <= live0) return;
    a->live = live0;                      // a path that returned between a malloc and its free
    if (a->live == 0) arena_reset(a);
}

hipError_t xm_malloc_async(void **p, size_t bytes, hipStream_t st) {
    Arena *a = arena_of(st);
    if (!a) return hipErrorInvalidDevice;
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    for (Chunk &c : a->chunks)
        if (c.size - c.used >= bytes) { *p = c.base + c.used; c.used += bytes; a->live++; return hipSuccess; }
    Chunk c;
    c.size = bytes > ((size_t)32 << 20) ? bytes : ((size_t)32 << 20);
    c.used = bytes;
    hipError_t e = hipMalloc((void **)&c.base, c.size);
    if (e != hipSuccess) return e;
    a->chunks.push_back(c);
    *p = c.base;
    a->live++;
    return hipSuccess;
}
hipError_t xm_free_async(void *p, hipStream_t st) {
    (void)p;
    Arena *a = arena_of(st);
    if (!a || a->live == 0) return hipErrorInvalidValue;
    if (--a->live == 0) arena_reset(a);
    return hipSuccess;
}

// ---- read-backs that do not drain the stream ----
// A host decision in the middle of a pass (the plan's counts, the pair kernels' counters) is copied into a pinned block and
// followed by an event; the caller queues whatever does not depend on the decision behind the copy and waits for the event
// only then, so that the device has work while the host reads, allocates and launches.  One block and one event per slot,
// created once per thread and device and never destroyed (as the side streams of the pair kernels).
HostWait *host_wait() {
    static thread_local HostWait *cur[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { set_error("hipGetDevice failed"); return nullptr; }
    if (cur[dev]) return cur[dev];
    HostWait *p = new HostWait();
    p->dev = dev;
    bool ok = hipHostMalloc((void **)&p->h, sizeof(int64_t) * HW_SLOTS * HW_WORDS, hipHostMallocDefault) == hipSuccess;
    for (int s = 0; s < HW_SLOTS && ok; s++) {
        ok = hipEventCreateWithFlags(&p->ev[s], hipEventDisableTiming) == hipSuccess;
        p->pending[s] = false;
    }
    if (!ok) { set_error("could not create the pinned read-back block"); delete p; return nullptr; }
    cur[dev] = p;
    return p;
}
int host_wait_post(hipStream_t st, int slot, const void *d_src, int words) {
    XM_ARG(slot >= 0 && slot < HW_SLOTS && words >= 0 && words <= HW_WORDS);
    HostWait *w = host_wait();
    if (!w) return XMAP_ERR_HIP;
    if (w->pending[slot]) {         // a read-back nobody took (its caller left through an error): let its copy land, then drop it
        XM_HIP(hipEventSynchronize(w->ev[slot]));
        w->pending[slot] = false;
    }
    int64_t *h = w->h + (size_t)slot * HW_WORDS;
    for (int x = 0; x < HW_WORDS; x++) h[x] = 0;
    if (words) XM_HIP(hipMemcpyAsync(h, d_src, sizeof(int64_t) * (size_t)words, hipMemcpyDeviceToHost, st));
    XM_HIP(hipEventRecord(w->ev[slot], st));
    w->pending[slot] = true;
    return XMAP_OK;
}
int host_wait_take(int slot, const int64_t **h) {
    XM_ARG(slot >= 0 && slot < HW_SLOTS && h);
    HostWait *w = host_wait();
    if (!w) return XMAP_ERR_HIP;
    if (!w->pending[slot]) {
        set_error("read-back slot %d waited for without a post", slot);
        return XMAP_ERR_ARG;
    }
    w->pending[slot] = false;
    XM_HIP(hipEventSynchronize(w->ev[slot]));
    *h = w->h + (size_t)slot * HW_WORDS;
    return XMAP_OK;
}

// ---- the small fills of one phase in one launch: range y of the list is blockIdx.y ----
__global__ __launch_bounds__(256) void k_fill_multi(FillList F) {
    const int y = blockIdx.y;
    unsigned *p = (unsigned *)F.p[y];
    const unsigned long long n = F.words[y];
    const unsigned v = F.val[y];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) p[i] = v;
}
int fill_multi(hipStream_t st, const FillList &F) {
    XM_ARG(F.n >= 0 && F.n <= FillList::MAX);
    unsigned long long most = 0;
    for (int y = 0; y < F.n; y++) most = F.words[y] > most ? F.words[y] : most;
    if (F.n == 0 || most == 0) return XMAP_OK;
    unsigned long long bx = (most + 1023) / 1024;         // four words per thread, at most 2048 blocks per range
    if (bx > 2048) bx = 2048;
    k_fill_multi<<<dim3((unsigned)bx, (unsigned)F.n), dim3(256), 0, st>>>(F);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

// ---- exclusive scan: tile sums, then tile scans.  Up to SCAN2_MAX_TILES tiles every block of the second pass adds up the
// tile sums in front of it itself (two launches; no block waits for another: the first launch has ended); beyond that a
// one-block scan of the tile sums runs in between (three launches).  grid.y = 2 scans two arrays of one length in the
// same launches; `plus`: the first array is scanned as in0 + in1 (row totals of the mirror: own + mirrored). ----
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;
constexpr int SCAN2_MAX_TILES = 2048;

__device__ __forceinline__ long long block_exclusive_scan(long long v, long long *total, long long *smem) {
    // inclusive scan inside the wave, then across the 4 waves
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) smem[w] = inc;
    __syncthreads();
    long long base = 0, tot = 0;
    for (int k = 0; k < SCAN_THREADS / 64; k++) {
        long long s = smem[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

template <typename TIn>
struct ScanIn {
    const TIn *in0, *in1;
    int plus;
    __device__ __forceinline__ long long load(int y, long long i) const {
        if (y) return (long long)in1[i];
        long long v = (long long)in0[i];
        if (plus) v += (long long)in1[i];
        return v;
    }
};

template <typename TIn>
__global__ __launch_bounds__(SCAN_THREADS) void k_tile_sums(ScanIn<TIn> S, long long n, long long n_tiles, long long *tile_sum) {
    __shared__ long long smem[4];
    const int y = blockIdx.y;
    long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    long long s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++)
        if (base + k < n) s += S.load(y, base + k);
    long long tot;
    block_exclusive_scan(s, &tot, smem);
    if (threadIdx.x == 0) tile_sum[(long long)y * n_tiles + blockIdx.x] = tot;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_tile_sums(long long *tile_sum, long long n_tiles, long long *grand0, long long *grand1) {
    __shared__ long long smem[4];
    tile_sum += (long long)blockIdx.y * n_tiles;
    long long carry = 0;
    for (long long b = 0; b < n_tiles; b += SCAN_THREADS) {
        long long i = b + threadIdx.x;
        long long v = i < n_tiles ? tile_sum[i] : 0;
        long long tot;
        long long ex = block_exclusive_scan(v, &tot, smem);
        if (i < n_tiles) tile_sum[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *(blockIdx.y ? grand1 : grand0) = carry;
}

// SELF: tile_sum holds the tiles' sums and the block adds up those in front of its own (the last block leaves the grand total
// in out[n]); else tile_sum holds their exclusive scan already
template <typename TIn, bool SELF>
__global__ __launch_bounds__(SCAN_THREADS) void k_tile_scan(ScanIn<TIn> S, long long n, long long n_tiles, const long long *tile_sum,
                                                            long long *out0, long long *out1) {
    __shared__ long long smem[4];
    const int y = blockIdx.y;
    tile_sum += (long long)y * n_tiles;
    long long *out = y ? out1 : out0;
    long long off;
    if (SELF) {
        long long part = 0;
        for (long long t = threadIdx.x; t < (long long)blockIdx.x; t += SCAN_THREADS) part += tile_sum[t];
        block_exclusive_scan(part, &off, smem);
    } else {
        off = tile_sum[blockIdx.x];
    }
    long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    long long v[SCAN_ITEMS];
    long long s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        v[k] = (base + k < n) ? S.load(y, base + k) : 0;
        s += v[k];
    }
    long long tot;
    long long ex = block_exclusive_scan(s, &tot, smem) + off;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        if (base + k < n) out[base + k] = ex;
        ex += v[k];
    }
    if (SELF && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = off + tot;
}

// n_arrays = 1: in0 -> out0; 2: (plus ? in0 + in1 : in0) -> out0 and in1 -> out1.  h_total [n_arrays] (host, or NULL)
template <typename TIn>
static int exclusive_scan(hipStream_t st, int n_arrays, const TIn *in0, const TIn *in1, int plus, int64_t *out0, int64_t *out1, int64_t n,
                          int64_t *h_total) {
    XM_ARG(n >= 0 && (n_arrays == 1 || n_arrays == 2));
    XM_SCOPE(st);
    // out[n] doubles as the grand total; tile sums live in a small temporary
    const int64_t n_tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    XM_ARG(n_tiles < 0x7fffffffLL);
    const ScanIn<TIn> S{in0, in1, plus};
    if (n_tiles == 0) {
        XM_HIP(hipMemsetAsync(out0 + n, 0, sizeof(int64_t), st));
        if (n_arrays == 2) XM_HIP(hipMemsetAsync(out1 + n, 0, sizeof(int64_t), st));
    } else {
        long long *tile = nullptr;
        XM_HIP(xm_malloc_async((void **)&tile, sizeof(long long) * (size_t)n_tiles * (size_t)n_arrays, st));
        const dim3 grid((unsigned)n_tiles, (unsigned)n_arrays);
        k_tile_sums<TIn><<<grid, dim3(SCAN_THREADS), 0, st>>>(S, n, n_tiles, tile);
        XM_LAUNCH_CHECK();
        if (n_tiles <= SCAN2_MAX_TILES) {
            k_tile_scan<TIn, true><<<grid, dim3(SCAN_THREADS), 0, st>>>(S, n, n_tiles, tile, (long long *)out0, (long long *)out1);
            XM_LAUNCH_CHECK();
        } else {
            k_scan_tile_sums<<<dim3(1, (unsigned)n_arrays), dim3(SCAN_THREADS), 0, st>>>(tile, n_tiles, (long long *)(out0 + n),
                                                                                          (long long *)(out1 ? out1 + n : nullptr));
            XM_LAUNCH_CHECK();
            k_tile_scan<TIn, false><<<grid, dim3(SCAN_THREADS), 0, st>>>(S, n, n_tiles, tile, (long long *)out0, (long long *)out1);
            XM_LAUNCH_CHECK();
        }
        XM_HIP(xm_free_async(tile, st));
    }
    if (h_total) {
        XM_HIP(hipMemcpyAsync(h_total, out0 + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (n_arrays == 2) XM_HIP(hipMemcpyAsync(h_total + 1, out1 + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
    }
    return XMAP_OK;
}
}  // namespace xmap

extern "C" {
const char *xmap_last_error(void) { return xmap::g_err; }
int xmap_version(void) { return 125; }

/* The library's temporaries: give every idle arena's memory of the calling thread back to the driver (arenas with live
 * temporaries are left alone).  Synchronises the device. */
int xmap_trim(void) {
    XM_HIP(hipDeviceSynchronize());
    int dev = 0;
    XM_HIP(hipGetDevice(&dev));
    for (xmap::Arena &a : xmap::g_arenas) {
        if (a.dev != dev || a.live != 0) continue;
        for (xmap::Chunk &c : a.chunks) (void)hipFree(c.base);
        a.chunks.clear();
    }
    return XMAP_OK;
}

/* test hooks: state of the calling thread's arena of `stream` (live temporaries, bytes reserved), and a call that takes two
 * temporaries and then leaves through an error path (fail != 0) the way an entry point would */
int xmap_debug_arena(void *stream, int64_t *live, int64_t *reserved) {
    XM_ARG(live && reserved);
    int dev = 0;
    XM_HIP(hipGetDevice(&dev));
    *live = 0; *reserved = 0;
    if (xmap::Arena *a = xmap::arena_find(dev, (hipStream_t)stream)) {
        *live = (int64_t)a->live;
        for (xmap::Chunk &c : a->chunks) *reserved += (int64_t)c.size;
    }
    return XMAP_OK;
}
int xmap_debug_arena_call(void *stream, int64_t bytes, int fail) {
    using namespace xmap;
    XM_SCOPE(stream);
    hipStream_t st = (hipStream_t)stream;
    void *a = nullptr, *b = nullptr;
    XM_HIP(xm_malloc_async(&a, (size_t)bytes, st));
    XM_HIP(xm_malloc_async(&b, 1024, st));
    XM_ARG(!fail);                      // the early return under test
    XM_HIP(xm_free_async(b, st));
    XM_HIP(xm_free_async(a, st));
    return XMAP_OK;
}

int xmap_exclusive_scan_i64(void *stream, const int64_t *in, int64_t *out, int64_t n, int64_t *h_total) {
    XM_ARG(out && (in || n == 0));
    return xmap::exclusive_scan<long long>((hipStream_t)stream, 1, (const long long *)in, nullptr, 0, out, nullptr, n, h_total);
}
int xmap_exclusive_scan_i32_to_i64(void *stream, const int32_t *in, int64_t *out, int64_t n, int64_t *h_total) {
    XM_ARG(out && (in || n == 0));
    return xmap::exclusive_scan<int>((hipStream_t)stream, 1, in, nullptr, 0, out, nullptr, n, h_total);
}
int xmap_exclusive_scan2_i32_to_i64(void *stream, const int32_t *in_a, const int32_t *in_b, int32_t a_plus_b, int64_t *out_a,
                                    int64_t *out_b, int64_t n, int64_t *h_totals) {
    XM_ARG(out_a && out_b && ((in_a && in_b) || n == 0));
    return xmap::exclusive_scan<int>((hipStream_t)stream, 2, in_a, in_b, a_plus_b ? 1 : 0, out_a, out_b, n, h_totals);
}
int xmap_scan_self_tiles(void) { return xmap::SCAN2_MAX_TILES; }
}
