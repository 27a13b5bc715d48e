// mid_rows.hip -- stage B: the middle lists of the joint paths (MidArgs / MidX / MidDir and what they hold: paths.h), built
// row-wise: per non-bridge x' the (t, s, x) records of its joint paths, grouped by column x (tile directory + 64-byte
// records); one block per x', tile counters in LDS, flat walk.
//
// Kernels:
//   k_joint_list                    : the joint (t, s) of every source list, compacted
//   k_att_columns                   : the column of every attach entry
//   k_joint_records, k_row_records  : the exact record count of a row before it is built (rows wider than the LDS span)
//   k_mid_rows<PHASE, ONE_RANGE>    : PHASE 0 counts a row's records and tiles, PHASE 1 writes its directory and records
// Entry points: xmap_mid_rows_count, xmap_mid_rows_place (mid_rows_run: mid_joints, mid_rows_lds, the launch).
#include "paths.h"
#include <stdlib.h>

namespace xmap {

// Row-wise construction of the middle lists (default): ONE block per x', the tile sizes of its row in LDS (the row of
// the dense table without the table).  PHASE 0 counts the row's records and non-empty tiles; PHASE 1 repeats the tally,
// turns it into offsets (block scan), writes the row's tile directory in x order and places the records with LDS cursors.
// No global atomics (the table form spends 1.6e8 of them per pass, twice, on a 3 GB table) and no n_nb^2 memory.
// The LDS holds the counters of `span` columns (<= XMAP_MID_ROWS_SPAN): a row with more non-bridge items than that is
// built in column ranges [x0, x0 + span), one after the other -- every range walks the row's (t, s, x) again and keeps the
// x of its range, the directory and the records of the ranges follow each other (x order is kept).  Rounds 1-2 fell back
// to the dense n_nb x n_nb table beyond 40 000 non-bridge items (120 GB at 1e5) and the coarse ABI refused.

// joint (t, s) of every source list, compacted in list order: joff[jptr[t] .. jptr[t+1]) = the offsets inside src(t) of the
// entries with the joint flag (2.3 % of them at BASELINE configs[1]: the walk of k_mid_rows reads these instead of scanning the
// lists of a row's neighbours once per row).  joff == NULL: the counts (jcnt) only.
__global__ __launch_bounds__(256) void k_joint_list(int I, const long long *src_ptr, const uint8_t *src_flag, int *jcnt,
                                                    const long long *jptr, int *joff) {
    // a wave takes 64 items: their ranges one per lane (most items have no source list), then the non-empty lists one by one
    const int t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (t0 >= I) return;
    const int lane = lane_id();
    const int tl = t0 + lane;
    long long s0l = 0, s1l = 0, outl = 0;
    if (tl < I) { s0l = src_ptr[tl]; s1l = src_ptr[tl + 1]; if (joff) outl = jptr[tl]; }
    int totl = 0;
    unsigned long long todo = __ballot(s1l > s0l);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const long long s0 = rl64(s0l, l), s1 = rl64(s1l, l);
        long long out = rl64(outl, l);
        int total = 0;
        for (long long base = s0; base < s1; base += 64) {
            const long long p = base + lane;
            const bool ok = p < s1 && (src_flag[p] & 1);
            const unsigned long long m = __ballot(ok);
            if (joff && ok) joff[out + __popcll(m & lanemask_lt())] = (int)(p - s0);
            out += __popcll(m);
            total += __popcll(m);
        }
        if (lane == l) totl = total;
    }
    if (!joff && tl < I) jcnt[tl] = totl;
}

// the column (index among the non-bridge items) of every attach entry: nb_id[att_idx[ap]] gathered ONCE per call -- the walks of
// k_mid_rows read it 1.6e8 times per walk, and a gather of 64 random lines costs the CU ~320 cycles per instruction
// (profiles/ta_rate.hip): 1.3 ms per walk, three walks per call
__global__ __launch_bounds__(256) void k_att_columns(long long bound, int I, const long long *att_ptr, const int *att_idx, const int *nb_id,
                                                     int *axid) {
    const long long ap = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ap < bound && ap < att_ptr[I]) axid[ap] = nb_id[att_idx[ap]];
}

// records behind every t: sum of the attach-list lengths over its joint (t, s) -- and per row x' over its neighbours t: the
// exact record count of a row BEFORE it is built (rows wider than the LDS span keep their records' columns in a scratch list)
__global__ __launch_bounds__(256) void k_joint_records(int I, const long long *jptr, const int *joff, const long long *src_ptr,
                                                       const int *src_idx, const long long *att_ptr, long long *jrec) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= I) return;
    const int lane = lane_id();
    const long long j0 = jptr[t], j1 = jptr[t + 1], s0 = src_ptr[t];
    long long sum = 0;
    for (long long j = j0 + lane; j < j1; j += 64) {
        const int sx = src_idx[s0 + joff[j]];
        sum += att_ptr[sx + 1] - att_ptr[sx];
    }
    sum = wave_sum_ll(sum);
    if (lane == 0) jrec[t] = sum;
}
__global__ __launch_bounds__(256) void k_row_records(int n_nb, int k, const int *nb_list, const int *kcnt, const int *kcol,
                                                     const uint8_t *flags, const long long *jrec, long long *rowrec) {
    const int xpid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (xpid >= n_nb) return;
    const int lane = lane_id();
    const int xp = nb_list[xpid];
    const int nq = kcnt[(size_t)xp * 2];
    long long sum = 0;
    for (int q = lane; q < nq; q += 64) {
        const int t = kcol[((size_t)xp * 2) * k + q];
        if (flags[t] & 2) sum += jrec[t];
    }
    sum = wave_sum_ll(sum);
    if (lane == 0) rowrec[xpid] = sum;
}

constexpr int MIDROW_WAVES = 16;
template <int PHASE, bool ONE_RANGE>
__global__ __launch_bounds__(64 * MIDROW_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_mid_rows(MidArgs A, int span, int *ng, long long *nrec, const long long *dir_ptr,
                                                                const long long *rec_ptr, MidDir *dir) {
    extern __shared__ int bins[];                      // [span]
    __shared__ unsigned long long s_wave[MIDROW_WAVES];
    const int xpid = blockIdx.x;
    const int xp = A.nb_list[xpid];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int n_nb = A.n_nb;
    const int nq = A.kcnt[(size_t)xp * 2];
    // The walk, round 4.  A row of configs[1] has 10 000 records on average (median 12, p90 33 000, maximum 93 000:
    // profiles/r04m_mid_walk.txt) behind <= 50 neighbours t and their joint (t, s), and ONE block builds it: what the block
    // takes is the chain of dependent memory trips of its slowest wave.  The first form ran the neighbours as a serial loop
    // (three trips per t), scanned their source lists for the joint flag (2.3 % of the entries have it) and gave a wave one
    // joint per step: ~300 trips per wave and walk in the big rows.  Now:
    //  * the joint entries of every source list are compacted once per call (k_joint_list: jptr / joff), and the row's
    //    neighbours are loaded one per LANE into a block-shared table with the prefix sums of their joint counts: the row's
    //    joints are ONE flat list, taken 64 at a time by every wave alike (three trips: offset -> s -> attach range);
    //  * the records of a chunk of 64 joints are a flat list too (scan of the attach-list lengths over the lanes; a record's
    //    joint by a six-step search over the starts in LDS), dealt to the waves in rounds of 64 and walked MID_UNROLL rounds
    //    at a time, so that the two trips of a round (attach entry -> its column) overlap with those of its neighbours.
    // ~100 trips per wave and walk in the biggest row, and every lane of every round but a chunk's last is busy.
    constexpr int MID_UNROLL = PHASE == 0 ? 4 : 2;      // (the placement keeps a record's values live: two rounds fit 64 VGPRs)
    __shared__ long long q_s0[64], q_jlo[64];
    __shared__ double q_v2[64], q_m2[64], q_f2[64];
    __shared__ int q_joff[65];
    __shared__ int s_off[MIDROW_WAVES][64];          // (what else a record needs of its joint comes from the joint's LANE by
    volatile int *w_off = s_off[w];                  //  ds_bpermute: with 64.5 KB of counters at configs[1], two blocks per CU need the rest small)
    auto walk = [&](int x0, int x1, auto &&body) {
        long long cbase = 0;                            // records of the chunks in front: a record's index in the row's walk order
        for (int qb = 0; qb < nq; qb += 64) {
            __syncthreads();                            // (nobody reads the previous table any more)
            if (w == 0) {
                const int ql = qb + lane;
                long long s0 = 0, jlo = 0;
                int jn = 0;
                double v2 = 0.0, m2 = 0.0, f2 = 0.0;
                if (ql < nq) {
                    const size_t o = ((size_t)xp * 2) * A.k + ql;
                    const int t = A.kcol[o];
                    if (A.flags[t] & 2) {
                        s0 = A.src_ptr[t]; jlo = A.jptr[t]; jn = (int)(A.jptr[t + 1] - jlo);
                        v2 = A.kval[o * 3]; m2 = A.kval[o * 3 + 1]; f2 = A.kval[o * 3 + 2];          // edge (x', t)
                    }
                }
                int incl = jn;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
                q_s0[lane] = s0; q_jlo[lane] = jlo; q_v2[lane] = v2; q_m2[lane] = m2; q_f2[lane] = f2;
                q_joff[lane] = incl - jn;               // joints of the neighbours in front (a neighbour without joints: its successor's)
                if (lane == 63) q_joff[64] = incl;
            }
            __syncthreads();
            const int J = q_joff[64];
            for (int g0 = 0; g0 < J; g0 += 64) {        // 64 joints of the row; every wave takes every chunk, the ROUNDS are dealt
                const int g = g0 + lane;
                int q = 0;                              // the last neighbour whose joints start at or before g
#pragma unroll
                for (int st = 32; st >= 1; st >>= 1) if (q_joff[q + st] <= g) q += st;
                int jo = 0, len = 0;
                long long a0 = 0;
                if (g < J) {
                    jo = A.joff[q_jlo[q] + (g - q_joff[q])];
                    const int s = A.src_idx[q_s0[q] + jo];
                    a0 = A.att_ptr[s];
                    len = (int)(A.att_ptr[s + 1] - a0);
                }
                int incl = len;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
                const int T = rl32(incl, 63);
                if (T == 0) continue;
                const long long cb = cbase;
                cbase += T;
                __builtin_amdgcn_wave_barrier();
                w_off[lane] = incl - len;                // first record of the lane's joint (lanes without records: their successor's)
                __builtin_amdgcn_wave_barrier();
                const int a0_lo = (int)(a0 & 0xffffffffll), a0_hi = (int)(a0 >> 32);
                for (int r0 = 64 * w; r0 < T; r0 += 64 * MIDROW_WAVES * MID_UNROLL) {
                    int jj[MID_UNROLL], xi[MID_UNROLL], rr[MID_UNROLL];
                    long long ap[MID_UNROLL];
#pragma unroll
                    for (int u = 0; u < MID_UNROLL; u++) {
                        const int r = r0 + u * 64 * MIDROW_WAVES + lane;
                        rr[u] = r;
                        int j = 0;                       // the last lane whose joint starts at or before record r
#pragma unroll
                        for (int st = 32; st >= 1; st >>= 1) if (w_off[j + st] <= r) j += st;
                        jj[u] = r < T ? j : -1;
                        const long long ja0 = ((long long)__shfl(a0_hi, j, 64) << 32) | (unsigned int)__shfl(a0_lo, j, 64);
                        ap[u] = r < T ? ja0 + (r - w_off[j]) : 0;
                    }
#pragma unroll
                    for (int u = 0; u < MID_UNROLL; u++) xi[u] = jj[u] >= 0 ? A.axid[ap[u]] : -1;
#pragma unroll
                    for (int u = 0; u < MID_UNROLL; u++) {
                        const int jl = jj[u] >= 0 ? jj[u] : 0;
                        const int qq = __shfl(q, jl, 64), jjo = __shfl(jo, jl, 64);      // (all lanes take part in the exchange)
                        // (every lane calls: the placement moves its records between the lanes of a quad)
                        body(jj[u] >= 0 && (ONE_RANGE || (xi[u] >= x0 && xi[u] < x1)), xi[u], q_v2[qq], q_m2[qq], q_f2[qq], q_s0[qq] + jjo, ap[u], cb + rr[u]);
                    }
                }
            }
        }
    };
    unsigned long long done = 0;                        // (non-empty tiles << 40 | records) of the ranges before this one
    const long long rbase = PHASE ? rec_ptr[xpid] : 0, dbase = PHASE ? dir_ptr[xpid] : 0;
    // A row wider than the LDS span is built range by range, and every range needs the tally of ITS columns.  The first form
    // walked the row again for every tally (27 walks per row at the S1 shape: nine ranges, count + tally + placement); now ONE
    // walk leaves the column of every record in a scratch list (the walk order is deterministic and the rows' record counts
    // are known beforehand: k_joint_records / k_row_records), and the ranges' tallies stream it.
    int *stash = nullptr;
    long long n_stash = 0;
    if (!ONE_RANGE) {
        stash = A.xl + A.xoff[xpid];
        n_stash = A.xoff[xpid + 1] - A.xoff[xpid];
        walk(0, n_nb, [&](bool valid, int xid, double, double, double, long long, long long, long long ridx) { if (valid && ridx < n_stash) stash[ridx] = xid; });
        __syncthreads();
    }
    for (int x0 = 0; x0 < n_nb; x0 += ONE_RANGE ? n_nb : span) {
        const int x1 = (ONE_RANGE || (x0 + span) >= n_nb) ? n_nb : (x0 + span), nx = x1 - x0;
        if (!ONE_RANGE) __syncthreads();                // (the previous range's placement is over)
        for (int i = threadIdx.x; i < nx; i += 64 * MIDROW_WAVES) bins[i] = 0;
        __syncthreads();
        if (!ONE_RANGE) {
            for (long long i = threadIdx.x; i < n_stash; i += 64 * MIDROW_WAVES) {
                const int xid = stash[i];
                if (xid >= x0 && xid < x1) atomicAdd(&bins[xid - x0], 1);
            }
        } else
        walk(x0, x1, [&](bool valid, int xid, double, double, double, long long, long long, long long) { if (valid) atomicAdd(&bins[xid - x0], 1); });
        __syncthreads();
        // per thread a run of consecutive bins: (non-empty tiles << 40 | records), block-wide exclusive scan
        const int per = (nx + 64 * MIDROW_WAVES - 1) / (64 * MIDROW_WAVES);
        const int b0 = threadIdx.x * per, b1 = (b0 + per) < nx ? (b0 + per) : nx;
        unsigned long long mine = 0;
        for (int i = b0; i < b1; i++) { const int c = bins[i]; mine += (unsigned long long)c + (c ? (1ull << 40) : 0ull); }
        unsigned long long incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned long long t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
        if (lane == 63) s_wave[w] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (int o = 0; o < MIDROW_WAVES; o++) { const unsigned long long v = s_wave[o]; if (o < w) before += v; total += v; }
        if (PHASE == 1) {
            const unsigned long long ex = done + before + incl - mine;
            int rank = (int)(ex >> 40);
            long long off = (long long)(ex & ((1ull << 40) - 1));
            for (int i = b0; i < b1; i++) {
                const int c = bins[i];
                bins[i] = (int)off;                         // placement cursor of the tile (records of a row fit 31 bits)
                if (c) {
                    MidDir d;
                    d.x = A.nb_list[x0 + i]; d.ne = 1 + A.kcnt[(size_t)d.x * 2 + 1]; d.cnt = c; d.pad = x0 + i; d.off = rbase + off;
                    dir[dbase + rank] = d;
                    rank++;
                    off += c;
                }
            }
            __syncthreads();
            walk(x0, x1, [&](bool valid, int xid, double v2, double m2, double f2, long long p, long long ap, long long) {
                long long pos = 0;
                MidX r;
                r.sm2 = 0.0; r.sm3 = 0.0; r.sm4 = 0.0; r.f2 = 0.0; r.f3 = 0.0; r.f4 = 0.0; r.mu = 0.0; r.xid = 0; r.pad = 0;
                if (valid) {
                    pos = rbase + atomicAdd(&bins[xid - x0], 1);
                    const double v3 = A.src_val[p * 3], m3 = A.src_val[p * 3 + 1], f3 = A.src_val[p * 3 + 2];      // edge (t, s)
                    const double v4 = A.att_val[ap * 3], m4 = A.att_val[ap * 3 + 1], f4 = A.att_val[ap * 3 + 2];  // edge (s, x)
                    r.sm2 = v2 * m2; r.sm3 = v3 * m3; r.sm4 = v4 * m4; r.f2 = f2; r.f3 = f3; r.f4 = f4;
                    r.mu = (m2 + m3) + m4; r.xid = xid; r.pad = 0;
                }
                // The four records of a QUAD of lanes leave as four store instructions of 16 lines each instead of four of 64
                // (the CU's memory path charges a store by the lines it touches, profiles/ta_rate.hip): the 4 x 4 pieces of 16 bytes
                // are transposed inside the quad (two DPP butterfly steps), lane q then holds piece q of each of the quad's records
                uint4 P[4];
                {
                    const long long b0 = __double_as_longlong(r.sm2), b1 = __double_as_longlong(r.sm3), b2 = __double_as_longlong(r.sm4);
                    const long long b3 = __double_as_longlong(r.f2), b4 = __double_as_longlong(r.f3), b5 = __double_as_longlong(r.f4);
                    const long long b6 = __double_as_longlong(r.mu);
                    P[0] = make_uint4((unsigned)b0, (unsigned)(b0 >> 32), (unsigned)b1, (unsigned)(b1 >> 32));
                    P[1] = make_uint4((unsigned)b2, (unsigned)(b2 >> 32), (unsigned)b3, (unsigned)(b3 >> 32));
                    P[2] = make_uint4((unsigned)b4, (unsigned)(b4 >> 32), (unsigned)b5, (unsigned)(b5 >> 32));
                    P[3] = make_uint4((unsigned)b6, (unsigned)(b6 >> 32), (unsigned)r.xid, (unsigned)r.pad);
                }
                const int ql = lane & 3;
                const bool odd = (ql & 1) != 0, high = (ql & 2) != 0;
#define XM_SWAP4(CTRL, V) make_uint4((unsigned)__builtin_amdgcn_update_dpp(0, (int)(V).x, CTRL, 0xf, 0xf, true), \
                                     (unsigned)__builtin_amdgcn_update_dpp(0, (int)(V).y, CTRL, 0xf, 0xf, true), \
                                     (unsigned)__builtin_amdgcn_update_dpp(0, (int)(V).z, CTRL, 0xf, 0xf, true), \
                                     (unsigned)__builtin_amdgcn_update_dpp(0, (int)(V).w, CTRL, 0xf, 0xf, true))
#pragma unroll
                for (int m = 0; m < 2; m++) {       // lane ^ 1: the off-diagonal pieces of every 2 x 2 block
                    const uint4 send = odd ? P[2 * m] : P[2 * m + 1];
                    const uint4 recv = XM_SWAP4(0xB1, send);
                    if (odd) P[2 * m] = recv; else P[2 * m + 1] = recv;
                }
#pragma unroll
                for (int c = 0; c < 2; c++) {       // lane ^ 2: the off-diagonal 2 x 2 blocks
                    const uint4 send = high ? P[c] : P[2 + c];
                    const uint4 recv = XM_SWAP4(0x4E, send);
                    if (high) P[c] = recv; else P[2 + c] = recv;
                }
#undef XM_SWAP4
                uint4 *out16 = reinterpret_cast<uint4 *>(A.midX);
#define XM_QSTORE(J) { const long long pj = __double_as_longlong(quad_bcast<J>(__longlong_as_double(pos)));                       \
                       const int vj = __builtin_amdgcn_update_dpp(0, valid ? 1 : 0, (J) | ((J) << 2) | ((J) << 4) | ((J) << 6), 0xf, 0xf, true); \
                       if (vj) out16[pj * 4 + ql] = P[J]; }
                XM_QSTORE(0) XM_QSTORE(1) XM_QSTORE(2) XM_QSTORE(3)
#undef XM_QSTORE
            });
        }
        done += total;
    }
    if (PHASE == 0 && threadIdx.x == 0) { ng[xpid] = (int)(done >> 40); nrec[xpid] = (long long)(done & ((1ull << 40) - 1)); }
}

}  // namespace xmap

using namespace xmap;

// row-wise construction (k_mid_rows); the tile counters of a column range of the row live in LDS
static_assert((size_t)XMAP_MID_ROWS_SPAN * 4 + (size_t)MIDROW_WAVES * 64 * 4 + 3072 + 256 <= 160 * 1024,
              "k_mid_rows: tile counters + the neighbour table + the waves' walk state must fit the LDS of a gfx950 CU");
// the compacted joint lists of one call (temporaries of the caller's scope)
static int mid_joints(hipStream_t st, MidArgs &A, bool ranges) {
    int *jcnt = nullptr, *joff = nullptr;
    long long *jptr = nullptr;
    const int I = A.I;
    XM_HIP(xm_malloc_async((void **)&jcnt, sizeof(int) * (size_t)(I > 0 ? I : 1), st));
    XM_HIP(xm_malloc_async((void **)&jptr, sizeof(long long) * (size_t)(I + 1), st));
    int64_t nj = 0;
    if (I > 0) {
        k_joint_list<<<dim3((unsigned)((I + 255) / 256)), dim3(256), 0, st>>>(I, A.src_ptr, A.src_flag, jcnt, nullptr, nullptr);
        XM_LAUNCH_CHECK();
    }
    int rc = xmap_exclusive_scan_i32_to_i64(st, jcnt, (int64_t *)jptr, I, &nj);      // (one synchronisation: the size of joff)
    if (rc) return rc;
    XM_HIP(xm_malloc_async((void **)&joff, sizeof(int) * (size_t)(nj > 0 ? nj : 1), st));
    if (I > 0) {
        k_joint_list<<<dim3((unsigned)((I + 255) / 256)), dim3(256), 0, st>>>(I, A.src_ptr, A.src_flag, nullptr, jptr, joff);
        XM_LAUNCH_CHECK();
    }
    A.jptr = jptr; A.joff = joff;
    {   // (attach lists belong to the non-bridge items' first lists: at most k entries each)
        const long long bound = (long long)A.n_nb * A.k;
        int *axid = nullptr;
        XM_HIP(xm_malloc_async((void **)&axid, sizeof(int) * (size_t)(bound > 0 ? bound : 1), st));
        if (bound > 0) {
            k_att_columns<<<dim3((unsigned)((bound + 255) / 256)), dim3(256), 0, st>>>(bound, I, A.att_ptr, A.att_idx, A.nb_id, axid);
            XM_LAUNCH_CHECK();
        }
        A.axid = axid;
    }
    if (ranges && A.n_nb > 0) {      // rows wider than the LDS span: where the columns of a row's records are kept between its ranges
        long long *jrec = nullptr, *rowrec = nullptr, *xoff = nullptr;
        int *xl = nullptr;
        XM_HIP(xm_malloc_async((void **)&jrec, sizeof(long long) * (size_t)(I > 0 ? I : 1), st));
        XM_HIP(xm_malloc_async((void **)&rowrec, sizeof(long long) * (size_t)A.n_nb, st));
        XM_HIP(xm_malloc_async((void **)&xoff, sizeof(long long) * ((size_t)A.n_nb + 1), st));
        k_joint_records<<<dim3((unsigned)((I + 3) / 4)), dim3(256), 0, st>>>(I, jptr, joff, A.src_ptr, A.src_idx, A.att_ptr, jrec);
        XM_LAUNCH_CHECK();
        k_row_records<<<dim3((unsigned)((A.n_nb + 3) / 4)), dim3(256), 0, st>>>(A.n_nb, A.k, A.nb_list, A.kcnt, A.kcol, A.flags, jrec, rowrec);
        XM_LAUNCH_CHECK();
        int64_t total = 0;
        rc = xmap_exclusive_scan_i64(st, (const int64_t *)rowrec, (int64_t *)xoff, A.n_nb, &total);
        if (rc) return rc;
        XM_HIP(xm_malloc_async((void **)&xl, sizeof(int) * (size_t)(total > 0 ? total : 1), st));
        A.xoff = xoff; A.xl = xl;
    }
    return XMAP_OK;
}
static int mid_rows_lds(int32_t n_nb, size_t *bytes, int *span) {
    int cap = XMAP_MID_ROWS_SPAN;
    if (const char *e = getenv("XMAP_MID_ROWS_SPAN")) {      // tests: several column ranges on small inputs
        const int v = atoi(e);
        if (v >= 1 && v < cap) cap = v;
    }
    *span = n_nb < cap ? n_nb : cap;
    *bytes = sizeof(int32_t) * (size_t)(*span > 0 ? *span : 1);
    return XMAP_OK;
}


// both passes: the joint lists of the call, then one block per x'
template <int PHASE>
static int mid_rows_run(void *stream, const xmap_ext_tables *T, MidX *midX, int32_t *ng, int64_t *nrec, const int64_t *rec_ptr,
                        MidDir *dir) {
    size_t lds;
    int span;
    int rc = mid_rows_lds(T->n_nb, &lds, &span);
    if (rc) return rc;
    MidArgs A = mid_args(T);
    A.midX = midX;
    XM_ARG(T->src_flag);
    XM_SCOPE(stream);
    rc = mid_joints((hipStream_t)stream, A, span < T->n_nb);
    if (rc) return rc;
    const dim3 grid((unsigned)T->n_nb), block(64 * MIDROW_WAVES);
    if (span >= T->n_nb) {
        XM_HIP(hipFuncSetAttribute((const void *)k_mid_rows<PHASE, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_mid_rows<PHASE, true><<<grid, block, lds, (hipStream_t)stream>>>(A, span, ng, (long long *)nrec, (const long long *)T->dir_ptr,
                                                                           (const long long *)rec_ptr, dir);
    } else {
        XM_HIP(hipFuncSetAttribute((const void *)k_mid_rows<PHASE, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        k_mid_rows<PHASE, false><<<grid, block, lds, (hipStream_t)stream>>>(A, span, ng, (long long *)nrec, (const long long *)T->dir_ptr,
                                                                            (const long long *)rec_ptr, dir);
    }
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

extern "C" {

int xmap_mid_rows_count(void *stream, const xmap_ext_tables *T, int32_t *ng /*[n_nb]*/, int64_t *nrec /*[n_nb]*/) {
    XM_ARG(T);
    XM_ARG(T->cls && T->kcnt && T->kcol && T->kval && T->flags && T->att_ptr && T->src_ptr && T->nb_list && T->nb_id && ng && nrec);
    if (T->n_nb == 0) return XMAP_OK;
    return mid_rows_run<0>(stream, T, nullptr, ng, nrec, nullptr, nullptr);
}

int xmap_mid_rows_place(void *stream, const xmap_ext_tables *T, const int64_t *rec_ptr /*[n_nb+1]*/, void *dir, void *midX) {
    XM_ARG(T);
    XM_ARG(T->cls && T->kcnt && T->kcol && T->kval && T->flags && T->att_ptr && T->src_ptr && T->nb_list && T->nb_id);
    XM_ARG(T->dir_ptr && rec_ptr && dir && midX);
    if (T->n_nb == 0) return XMAP_OK;
    return mid_rows_run<1>(stream, T, (MidX *)midX, nullptr, nullptr, rec_ptr, (MidDir *)dir);
}

}
