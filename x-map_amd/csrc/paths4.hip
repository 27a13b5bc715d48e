// paths4.hip -- the path enumeration of stage B (default; DESIGN.md section "Stage B"):
//   k_edge_ranges              : may the bare division sequence be used (xmap_edge_ranges)
//   k_mark_ends, k_end_ranks   : the items that can end a path and their ranks (xmap_end_universe)
//   k_col_home, k_col_ends     : the home column of every end; the ends of every column as 32-byte records
//   k_paths4 (heads_Q), finalize_*
//                              : start-major, heads merged by column, one row update per column, rows indexed by end rank,
//                                exact (value, error) sums, fused top-10                          (random HBM row updates)
//   k_merge_groups, k_merge    : the partial rows of the heavy starts added up and finalised
#include "paths.h"

namespace xmap {

// ---- helpers of k_paths4 -------------------------------------------------------------------------------------
// a / b rounded to nearest for b > 0 and operands far from the ends of the exponent range: v_rcp_f64 + two Newton steps
// + one correction of the quotient, i.e. the sequence the compiler emits for `/` without v_div_scale / v_div_fmas'
// rescaling / v_div_fixup (which only act on operands near the ends of the range, zero, inf or nan)
__device__ __forceinline__ double div_mid(double a, double b) {
    double y = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    const double q = a * y;
    const double r = __builtin_fma(-b, q, a);
    return __builtin_fma(r, y, q);
}

// two-sum, rounding errors collected in lo (not renormalised: hi + lo is the sum to ~2^-104 like dd_add's pair)
__device__ __forceinline__ void acc2(double &hi, double &lo, double x) {
    const double s = hi + x;
    const double bb = s - hi;
    lo += (hi - (s - bb)) + (x - bb);
    hi = s;
}

// exchange inside a group of four adjacent lanes (DPP quad_perm: no LDS traffic)
template <int CTRL>
__device__ __forceinline__ double quad_swap(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}


// =============================================================================================
// k_paths4 (default).  What the ablations of k_paths2 / k_paths3 at BASELINE configs[1] say (profiles/README.md, round 2):
// a column (start, x) costs a fixed price -- merge step, end list, row update, bookkeeping -- that outweighs its
// arithmetic (10 records x 22 ends on average), and the row updates are random 32-byte read-modify-writes.  Hence:
//   * ONE row update per column: the lanes of a step are  W ends x S record slices  with S = 4 / 2 / 1 for a column of
//     <= 16 / <= 32 / more ends, so every column is a single set of lanes whatever its width; the S slices of an end
//     are adjacent lanes and are added up by one or two DPP exchanges;
//   * rows are indexed by the rank of the end among the U items that can end a path at all (xmap_end_universe; ranks
//     in column order, so that the ends of a column are neighbours in the row): 2.7x shorter rows, 5x less scratch;
//   * the ends of a column come from one table of 32-byte records (k_col_ends: rank and last edge), not from three
//     dependent gathers; the row entries are requested before the records are reduced;
//   * prepared records of all participating heads are staged in LDS (128 per round) in sets of 64, one record per lane
//     whichever head it belongs to: the records of all the heads of a column are ONE round trip (a trip per head had been
//     2.5 dependent trips per column), requested together with the end records; the row entries are requested next, before
//     the records are prepared.  Loads are unconditional (clamped indices) and consumed at unconditional places -- see the
//     comment in heads_Q; division and sums as in k_paths3.
// Round 4: heads_Q reads both tables of a column as 16-byte pieces, one per lane, where rounds 2-3 read whole records per
// lane (profiles/r04d_paths_pieces.txt: -2.7 %).  A software-pipelined form of the column loop, which overlapped the
// memory trips of consecutive columns, hid them and was not faster: 539-544 ms at four waves per SIMD against 526 ms for
// heads_Q at five (profiles/r04b_paths_pipelined.txt): a column costs work, not latency.
constexpr int Q_CAP = 64;                  // prepared records per round (the head records take the LDS of the other 64)
struct QLds {
    // (three arrays, not one record of four words per quad as the quad leaves them: that layout -- one 512-byte store, b64 +
    //  b128 reads at a 32-byte stride in the record loop -- measured 515 ms against 475, profiles/r04h_paths_columns.txt)
    double bsm[Q_CAP + 1], bc[Q_CAP + 1], bmu[Q_CAP + 1];      // (entry Q_CAP: the neutral record (0, 0, 1) of heads_Q's record loop)
    double hd[3][64];                      // first edge of every head of the batch: [0] sim * mutu, [1] frac, [2] mutu
    uint4 ep[128];                         // the chunk's end records as loaded: 16-byte pieces, two per end (the table's own layout)
};

struct QAcc {
    double *acc; int *touched;             // the unit's row [U][4] and touched list [U]
    const int *urank;
    int nt;
    unsigned long long paths;
    unsigned long long updates;            // read-modify-writes of row entries (the kernel's bound: DESIGN.md 4)
    __device__ __forceinline__ void add(bool active, int end, Carry p) {
        bool first = false;
        int u = 0;
        if (active) {
            u = urank[end];
            const double sp = (p.mu != 0.0) ? 1.0 * p.sm / p.mu : 0.0;   // calculate_path_confidence (extender.py:83-89)
            double *a = acc + (size_t)u * 4;
            double s_hi = a[0], s_lo = a[1], c_hi = a[2], c_lo = a[3];
            first = (c_hi == 0.0);
            acc2(s_hi, s_lo, sp * p.c);
            acc2(c_hi, c_lo, p.c);
            a[0] = s_hi; a[1] = s_lo; a[2] = c_hi; a[3] = c_lo;
        }
        const unsigned long long m = __ballot(first);
        if (first) touched[nt + __popcll(m & lanemask_lt())] = u;
        nt += __popcll(m);
        const int na = __popcll(__ballot(active));
        paths += na;
        updates += na;
    }
};

// An all-zero row entry: where the lanes of HOME ends read their "old" value from.  The home column of an end is the lowest
// column that lists it (ColEnd::u bit 30, k_col_home); columns are visited in ascending order and a unit visits its columns
// before anything else touches its row, so in the first head batch an end's entry is still zero when its home column
// comes by -- the update of a home end needs no load from the row: its lanes read this one cached line instead (the add
// of zero is exact, `first` comes out true by itself), and what the memory system sees is a store.
__device__ double g_zero_entry[4] = {0.0, 0.0, 0.0, 0.0};
constexpr int END_HOME = 1 << 30;

template <bool FASTDIV>
__device__ __forceinline__ void heads_Q(const Path2Args &B, QAcc &W, int start, long long h0, long long nH, int self, int xlo, int xhi,
                                        bool fresh) {
    __shared__ QLds stageq[4];          // one per wave of the block; DS operations of a wave execute in order
    const PathArgs &A = B.P;
    QLds &L = stageq[threadIdx.x >> 6];
    const int lane = lane_id();
    const int k = A.k;
    const int INF = 0x7fffffff;
    // this lane's head
    const long long h = h0 + lane;
    const bool hv = h < nH;
    double sm1 = 0.0, mu1 = 0.0, f1 = 1.0;      // (the neutral first edge: the start itself as head)
    long long dpos = 0, dend = 0;
    if (hv) {
        int xp = start;
        if (h >= self) {
            const long long rp = A.rnn_ptr[start] + (h - self);
            xp = A.rnn_idx[rp];
            const double sv = A.rnn_val[rp * 3], mu = A.rnn_val[rp * 3 + 1];
            sm1 = sv * mu; mu1 = mu; f1 = A.rnn_val[rp * 3 + 2];
        }
        const int xpid = B.nb_id[xp];
        dpos = B.dir_ptr[xpid];
        dend = B.dir_ptr[xpid + 1];
        if (xlo > 0) {   // lower bound of xlo in this head's directory (sorted by x)
            long long lo = dpos, hi = dend;
            while (lo < hi) {
                long long mid = (lo + hi) >> 1;
                if (B.dir[mid].x < xlo) lo = mid + 1; else hi = mid;
            }
            dpos = lo;
        }
    }
    MidDir cur;
    cur.x = INF; cur.ne = 0; cur.cnt = 0; cur.pad = 0; cur.off = 0;
    if (hv && dpos < dend) { cur = B.dir[dpos]; if (cur.x >= xhi) cur.x = INF; }
    const int nloc = (nH - h0) < 64 ? (int)(nH - h0) : 64;      // heads of this batch (lanes 0 .. nloc-1)
    if (lane == 0) { L.bsm[Q_CAP] = 0.0; L.bc[Q_CAP] = 0.0; L.bmu[Q_CAP] = 1.0; }       // the neutral record of the record loop
    // Merged records as 16-byte PIECES (record r = the four lanes 4r .. 4r+3 = {sm2, sm3}, {sm4, f2}, {f3, f4}, {mu, -}): one
    // load instruction per group of 16 records instead of four over the same lines; the first edge of a record's head comes
    // from a 24-byte LDS record per head (one ds_read_b64 per lane: lane 0 of a quad needs sim * mutu, lane 2 frac, lane 3 mutu)
    L.hd[0][lane] = sm1; L.hd[1][lane] = f1; L.hd[2][lane] = mu1;
    const uint4 *recp = reinterpret_cast<const uint4 *>(B.midX);
    const int pq = lane & 3, prec = lane >> 2;
    const int pfield = pq == 0 ? 0 : (pq == 2 ? 1 : 2);
    for (;;) {
        // smallest column among the heads: xor butterfly inside each half of the wave (ds_swizzle: no address registers),
        // then the two halves
        int xmin = cur.x;
#define XM_DPP_MIN(CTRL) { const int o = __builtin_amdgcn_update_dpp(INF, xmin, CTRL, 0xf, 0xf, false); xmin = o < xmin ? o : xmin; }
#define XM_SWZ_MIN(PAT) { const int o = __builtin_amdgcn_ds_swizzle(xmin, PAT); xmin = o < xmin ? o : xmin; }
        if (nloc <= 16) {      // the common batch of a few heads: DPP inside the first row of lanes, no LDS round trips
            XM_DPP_MIN(0xB1) XM_DPP_MIN(0x4E)                               // quad_perm [1,0,3,2], [2,3,0,1]
            if (nloc > 4) { XM_DPP_MIN(0x141) XM_DPP_MIN(0x140) }           // row_half_mirror, row_mirror
            xmin = rl32(xmin, 0);
        } else {
            XM_SWZ_MIN(0x041F) XM_SWZ_MIN(0x081F) XM_SWZ_MIN(0x101F) XM_SWZ_MIN(0x201F) XM_SWZ_MIN(0x401F)
            const int x0 = rl32(xmin, 0), x1 = rl32(xmin, 32);
            xmin = x0 < x1 ? x0 : x1;
        }
#undef XM_SWZ_MIN
#undef XM_DPP_MIN
        if (xmin == INF) break;
        const bool mine = cur.x == xmin;
        const unsigned long long part = __ballot(mine);
        const int first_l = __ffsll((long long)part) - 1;
        const int ne = rl32(cur.ne, first_l);
        const ColEnd *ce = B.cend + (size_t)rl32(cur.pad, first_l) * (k + 1);
        for (int b = 0; b < ne; b += 64) {
            const int nact = (ne - b) < 64 ? (ne - b) : 64;
            const int sh = nact <= 16 ? 2 : (nact <= 32 ? 1 : 0);     // log2 of the record slices per end
            const int ns = 1 << sh;
            const int q = lane >> sh, slice = lane & (ns - 1);
            // Memory round trips of a column: {end records, first set of merged records} together, then the row entries
            // (under the preparation and reduction of the records).  Every load is unconditional (clamped index) and is
            // consumed at one unconditional place: a load whose use sits behind a branch stays "pending" on the other
            // path, and the compiler then waits for ALL outstanding loads at the next join, which serialises the trips.
            // the end records as 16-byte PIECES, one per lane (two per end): ONE load instruction for up to 32 ends where the
            // whole-record form needs two over the same lines; the pieces go to LDS as they come and are read back per (end, slice)
            const int np = 2 * nact;
            const uint4 *cep = reinterpret_cast<const uint4 *>(ce) + 2 * b;
            const uint4 e0 = cep[lane < np ? lane : np - 1];
            unsigned long long pm = part;
            int pos = 0;                      // records of the current head already staged
            int set_n, my_h;
            long long my_rec;
            // a group = up to 16 records, four lanes each, of whichever participating heads they fall to
            auto assign = [&]() {
                set_n = 0; my_h = 0;
                my_rec = rl64(cur.off, __ffsll((long long)pm) - 1) * 4;     // lanes beyond the group: any piece
                for (;;) {
                    pm = ((unsigned long long)(unsigned)uniform((int)(pm >> 32)) << 32) | (unsigned)uniform((int)pm);
                    pos = uniform(pos); set_n = uniform(set_n);
                    if (pm == 0 || set_n >= 16) break;
                    const int l = __ffsll((long long)pm) - 1;
                    const int cnt = rl32(cur.cnt, l);
                    const long long off = rl64(cur.off, l);
                    int n = cnt - pos;
                    if (n > 16 - set_n) n = 16 - set_n;
                    if (lane >= 4 * set_n && lane < 4 * (set_n + n)) { my_rec = (off + pos) * 4 + (lane - 4 * set_n); my_h = l; }
                    set_n += n; pos += n;
                    if (pos == cnt) { pm &= pm - 1; pos = 0; }
                }
            };
            // prepared form of a group's records, computed inside the quad (same operations in the same order)
            auto prepare = [&](const uint4 &v, int fill) {
                const double H = L.hd[pfield][my_h];
                const double X = __longlong_as_double(((long long)v.y << 32) | v.x), Y = __longlong_as_double(((long long)v.w << 32) | v.z);
                const double X1 = quad_bcast<1>(X), Y1 = quad_bcast<1>(Y);      // sm4, f2 of the record
                const double v_sm = ((H + X) + Y) + X1;                           // lane 0: ((sm1 + sm2) + sm3) + sm4
                const double v_c = ((H * Y1) * X) * Y;                            // lane 2: ((f1 * f2) * f3) * f4
                const double v_mu = X + H;                                        // lane 3: mu + mu1
                const double val = pq == 0 ? v_sm : (pq == 2 ? v_c : v_mu);
                if (pq != 1 && prec < set_n) { if (pq == 0) L.bsm[fill + prec] = val; else if (pq == 2) L.bc[fill + prec] = val; else L.bmu[fill + prec] = val; }
            };
            assign();
            uint4 m0 = recp[my_rec];
            if (nact > 32) L.ep[64 + lane] = cep[64 + lane < np ? 64 + lane : np - 1];
            L.ep[lane] = e0;
            asm volatile("" ::: "memory");
            const bool ok = q < nact;
            const uint4 ea = L.ep[2 * (ok ? q : 0)], eb = L.ep[2 * (ok ? q : 0) + 1];
            const double sm5 = __longlong_as_double(((long long)ea.y << 32) | ea.x), mu5 = __longlong_as_double(((long long)ea.w << 32) | ea.z);
            const double f5 = __longlong_as_double(((long long)eb.y << 32) | eb.x);
            const int eur = (int)eb.z;
            const int eu = eur & (END_HOME - 1);
            const bool fl_ = ok && slice == 0;
            double *a = W.acc + (size_t)(ok ? eu : 0) * 4;
            const double *la = (ok && fresh && (eur & END_HOME)) ? g_zero_entry : a;
            for (;;) {
                // one round = up to Q_CAP prepared records (a column with more, < 1 % of them, updates its row once per round)
                double h0_ = 0.0, l0_ = 0.0, h1_ = 0.0, l1_ = 0.0;
                h0_ = la[0]; l0_ = la[1]; h1_ = la[2]; l1_ = la[3];     // requested before the records are prepared and reduced
                la = a;                                                 // (a second round of the same column finds the first one's sums)
                int fill = 0;
                {   // up to four groups requested together (one trip for up to 64 records), then prepared
                    const int h0g = my_h, g0 = uniform(set_n);
                    uint4 m1 = m0, m2 = m0, m3 = m0;
                    int h1g = 0, h2g = 0, h3g = 0, g1 = 0, g2 = 0, g3 = 0;
                    if (pm) { assign(); m1 = recp[my_rec]; h1g = my_h; g1 = uniform(set_n); }
                    if (pm) { assign(); m2 = recp[my_rec]; h2g = my_h; g2 = uniform(set_n); }
                    if (pm) { assign(); m3 = recp[my_rec]; h3g = my_h; g3 = uniform(set_n); }
                    my_h = h0g; set_n = g0; prepare(m0, fill); fill += g0;
                    if (g1) { my_h = h1g; set_n = g1; prepare(m1, fill); fill += g1; }
                    if (g2) { my_h = h2g; set_n = g2; prepare(m2, fill); fill += g2; }
                    if (g3) { my_h = h3g; set_n = g3; prepare(m3, fill); fill += g3; }
                    fill = uniform(fill);
                }
                asm volatile("" ::: "memory");
                double a_sh = 0.0, a_sl = 0.0, a_ch = 0.0, a_cl = 0.0;
                const int steps = (fill + ns - 1) >> sh;
                // The record loop without a branch and two records per iteration (round 4).  A lane whose slice has no
                // record in a step takes the NEUTRAL record (0, 0, 1): its path weight c = 0 * f is zero, so both sums get
                // + 0 -- exact, no effect -- and the compare / mask / skip-branch instructions of a step are gone; lanes beyond
                // the column's ends compute on the last end's record (never stored).  Two records per iteration: no
                // loop-carried register copies, one LDS round trip for both.
                auto step = [&](double rsm, double rc, double rmu) {
                    const double sm = rsm + sm5;
                    const double c = rc * f5;
                    const double mu = rmu + mu5;
                    double sp;
                    if (FASTDIV) sp = div_mid(sm, mu);
                    else sp = (mu != 0.0) ? 1.0 * sm / mu : 0.0;          // calculate_path_confidence (extender.py:83-89)
                    acc2(a_sh, a_sl, sp * c);
                    acc2(a_ch, a_cl, c);
                };
                int it = 0;
                for (; it + 1 < steps; it += 2) {
                    const int ra = (it << sh) + slice, rb = ra + ns;      // ra < fill in every step but a round's last
                    const int rbc = rb < fill ? rb : Q_CAP;
                    const double s0 = L.bsm[ra], c0 = L.bc[ra], u0 = L.bmu[ra];
                    const double s1 = L.bsm[rbc], c1 = L.bc[rbc], u1 = L.bmu[rbc];
                    asm volatile("" :: "v"(s0), "v"(c0), "v"(u0), "v"(s1), "v"(c1), "v"(u1));      // (both records: one LDS round trip)
                    step(s0, c0, u0);
                    step(s1, c1, u1);
                }
                if (it < steps) {
                    const int ra = (it << sh) + slice;
                    const int rc_ = ra < fill ? ra : Q_CAP;
                    step(L.bsm[rc_], L.bc[rc_], L.bmu[rc_]);
                }
                // the slices of an end sit in adjacent lanes
                if (sh >= 1) {
                    const double o_sh = quad_swap<0xB1>(a_sh), o_sl = quad_swap<0xB1>(a_sl);      // lane ^ 1
                    const double o_ch = quad_swap<0xB1>(a_ch), o_cl = quad_swap<0xB1>(a_cl);
                    acc2(a_sh, a_sl, o_sh); a_sl += o_sl;
                    acc2(a_ch, a_cl, o_ch); a_cl += o_cl;
                }
                if (sh == 2) {
                    const double o_sh = quad_swap<0x4E>(a_sh), o_sl = quad_swap<0x4E>(a_sl);      // lane ^ 2
                    const double o_ch = quad_swap<0x4E>(a_ch), o_cl = quad_swap<0x4E>(a_cl);
                    acc2(a_sh, a_sl, o_sh); a_sl += o_sl;
                    acc2(a_ch, a_cl, o_ch); a_cl += o_cl;
                }
                asm volatile("" :: "v"(h0_), "v"(l0_), "v"(h1_), "v"(l1_) : "memory");
                bool first = false;
                // The entry's two 16-byte halves leave from the end's first TWO slice lanes in ONE store instruction (round 4; before,
                // both left from the first lane): the CU's memory path charges an instruction by the lines it touches
                // (profiles/ta_rate.hip), and the two stores of the one-lane form touch the same ~15 lines twice: 490-492 -> 478-481 ms.
                // (The two LOADS split the same way: no change -- the second load of the one-lane form hits L1.  The finalisation
                //  with an entry per lane pair: +4 ms -- half as many line requests, but the division twice per entry.)
                if (fl_) {
                    first = (h1_ == 0.0);
                    acc2(h0_, l0_, a_sh); l0_ += a_sl;
                    acc2(h1_, l1_, a_ch); l1_ += a_cl;
                }
                if (sh >= 1) {
                    const double p_h = quad_swap<0xB1>(h1_), p_l = quad_swap<0xB1>(l1_);      // (slice 1 <- slice 0)
                    double *dst = a + (slice == 0 ? 0 : 2);
                    const double v0 = slice == 0 ? h0_ : p_h, v1 = slice == 0 ? l0_ : p_l;
                    if (ok && slice <= 1) { dst[0] = v0; dst[1] = v1; }
                } else if (fl_) {
                    a[0] = h0_; a[1] = l0_; a[2] = h1_; a[3] = l1_;
                }
                const unsigned long long fm = __ballot(first);
                if (first) W.touched[W.nt + __popcll(fm & lanemask_lt())] = eu;
                W.nt += __popcll(fm);
                W.paths += (unsigned long long)fill * (unsigned long long)nact;
                W.updates += (unsigned long long)nact;
                if (!pm) break;
                assign();
                m0 = recp[my_rec];
            }
        }
        if (mine) {    // advance the heads that took part
            dpos++;
            cur.x = INF;
            if (dpos < dend) { cur = B.dir[dpos]; if (cur.x >= xhi) cur.x = INF; }
        }
    }
}


// Waves per SIMD of k_paths4 (96 VGPRs); xmap_extend_cols_slots sizes one accumulator row per resident wave by it
constexpr int P_WAVES = 5;
template <bool FASTDIV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(P_WAVES, P_WAVES))) void k_paths4(Path2Args B) {
    __shared__ FinBuf fin[4];
    const PathArgs &A = B.P;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= A.n_slots) return;
    const int lane = lane_id();
    QAcc W;
    W.paths = 0; W.updates = 0; W.urank = A.urank;
    unsigned long long cand_total = 0;
    for (;;) {
        int u_ = 0;
        if (lane == 0) u_ = (int)atomicAdd(&A.counters[2], 1ull);
        const int unit = uniform(u_);
        if (unit >= A.n_units) break;  // every wave reaches this exit: the cursor only grows
        const int start = uniform(A.unit_start[unit]);
        const int c = uniform(A.unit_c[unit]);
        const int G = uniform(A.unit_G[unit]);
        const int row = uniform(A.unit_row[unit]);
        if (row < 0) {
            W.acc = A.acc + (size_t)slot * (size_t)A.row_stride * 4;
            W.touched = A.touched + (size_t)slot * A.U;
        } else {
            W.acc = A.hacc + (size_t)row * A.U * 4;
            W.touched = A.htouched + (size_t)row * A.U;
        }
        W.nt = 0;
        // work entries of a start, numbered: role T; per head its (t,s) part; per (64-head batch, column range) the tiles.
        // The tiles are walked FIRST (the numbering is what deals the entries to the G units of a heavy start, not the
        // order): while the first head batch runs nothing else has touched the unit's row, which is what lets the home
        // ends of a column be stored without a load (heads_Q); sums are exact, so the order does not show in the result.
        const bool role_t = (A.flags[start] & 2) != 0;
        const long long r0 = uniform((int)A.rnn_ptr[start]), r1 = uniform((int)A.rnn_ptr[start + 1]);
        const int self = (A.cls[start] == 2) ? 1 : 0;   // head 0 = the start itself (target_path, extender.py:160-163)
        const long long nH = self + (r1 - r0);          // heads >= self: start in NN(x') (longest_path, :164-167)
        const long long nbatch = (nH + 63) / 64;
        const int RX = (nbatch > 0) ? (int)((G + nbatch - 1) / nbatch) : 1;   // column ranges: nbatch * RX >= G entries
        const int n_nb = B.n_nb;
        long long ent = (role_t ? 1 : 0) + nH;
        for (long long bt = 0; bt < nbatch; bt++)
            for (int rx = 0; rx < RX; rx++) {
                if (G == 1 || ent % G == c) {
                    const int xlo = (rx == 0) ? 0 : B.nb_list[(long long)rx * n_nb / RX];
                    const int xhi = (rx == RX - 1) ? 0x7fffffff : B.nb_list[(long long)(rx + 1) * n_nb / RX];
                    heads_Q<FASTDIV>(B, W, start, bt * 64, nH, self, xlo, xhi, bt == 0);
                }
                ent++;
            }
        ent = 0;
        if (role_t) {   // role T: non-joint paths from t = start (final_nonjoint_extend, extender.py:124-140,:180)
            if (G == 1 || ent % G == c) {
                Carry none; none.sm = 0; none.mu = 0; none.c = 0;
                through_t(A, W, start, false, none);
            }
            ent++;
        }
        for (long long h = 0; h < nH; h++) {
            if (G == 1 || ent % G == c) {
                const bool has_e1 = h >= self;
                const int xp = has_e1 ? A.rnn_idx[r0 + h - self] : start;
                Carry e1; e1.sm = 0; e1.mu = 0; e1.c = 1.0;
                if (has_e1) e1 = first_edge(A.rnn_val[(r0 + h - self) * 3], A.rnn_val[(r0 + h - self) * 3 + 1],
                                            A.rnn_val[(r0 + h - self) * 3 + 2]);
                head_S(A, W, xp, has_e1, e1);
            }
            ent++;
        }
        if (row < 0) cand_total += finalize_start(A, fin[threadIdx.x >> 6], W.acc, W.touched, W.nt, start);
        else if (lane == 0) A.unit_nt[unit] = W.nt;
    }
    if (lane == 0) {
        atomicAdd(&A.counters[0], cand_total);
        atomicAdd(&A.counters[1], W.paths);
        atomicAdd(&A.counters[4], W.updates);
    }
}

// precondition of the bare division sequence (div_mid): every kept pair has a mutuality >= 1 (an int32 count, so at most
// 2^31 - 1) and a product sim * mutu that is zero (either sign) or strictly inside (2^-400, 2^400); NaN and inf fail both
// tests -- then a path's mutuality sum is never zero and no operand is near the ends of the exponent range.  What stage A
// produces always qualifies; records fed by a caller are checked (every kept pair here; the listed pairs alone by the NumPy
// twin in Engine.ext_tables_from_knn).  tests/test_gpu_fed_sim.py pins the answer at the bounds and compares the two
// divisions bit for bit over the admitted range.
__global__ __launch_bounds__(256) void k_edge_ranges(long long n, const double *sim, const int *mutu, int *bad) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const double m = (double)mutu[p], sm = fabs(sim[p] * m);
    const bool ok = (m >= 1.0) && (sm == 0.0 || (sm > 0x1p-400 && sm < 0x1p400));      // mutu is an int32 count: >= 1 is "positive"
    if (!ok) atomicOr(bad, 1);
}

// the ends of every column x (non-bridge record): x itself, then NN(x) in list order, as 32-byte records
// home column of every end = the lowest column x whose end list {x} + NN(x) holds it (home[] preset to INT_MAX)
__global__ __launch_bounds__(256) void k_col_home(int n_nb, int k, const int *nb_list, const int *kcnt, const int *kcol, int *home) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_nb * (k + 1)) return;
    const int xid = (int)(t / (k + 1)), idx = (int)(t % (k + 1));
    const int x = nb_list[xid];
    int e = -1;
    if (idx == 0) e = x;
    else if (idx - 1 < kcnt[(size_t)x * 2 + 1]) e = kcol[((size_t)x * 2 + 1) * k + (idx - 1)];
    if (e >= 0) atomicMin(&home[e], x);
}

__global__ __launch_bounds__(256) void k_col_ends(int n_nb, int k, const int *nb_list, const int *kcnt, const int *kcol, const double *kval,
                                                  const int *urank, const int *home, ColEnd *cend) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_nb * (k + 1)) return;
    const int xid = (int)(t / (k + 1)), idx = (int)(t % (k + 1));
    const int x = nb_list[xid];
    ColEnd e;
    e.sm = 0.0; e.mu = 0.0; e.f = 1.0; e.u = -1; e.pad = 0;
    int item = -1;
    if (idx == 0) item = x;
    else if (idx - 1 < kcnt[(size_t)x * 2 + 1]) {
        const size_t o = ((size_t)x * 2 + 1) * k + (idx - 1);
        const double v = kval[o * 3], m = kval[o * 3 + 1];
        e.sm = v * m; e.mu = m; e.f = kval[o * 3 + 2];
        item = kcol[o];
    }
    if (item >= 0) e.u = urank[item] | (home[item] == x ? END_HOME : 0);      // (the ends of a column are distinct items)
    cend[t] = e;
}

// items that can end a path: the s of every src record, the x of every attach record, x and NN(x) of every non-bridge record
__global__ __launch_bounds__(256) void k_mark_ends(int I, int k, const uint8_t *cls, const int *kcnt, const int *kcol, long long n_src,
                                                   const int *src_idx, long long n_att, const int *att_idx, int *mark) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_src) mark[src_idx[t]] = 1;
    if (t < n_att) mark[att_idx[t]] = 1;
    if (t < (long long)I * k) {
        const int x = (int)(t / k), q = (int)(t % k);
        if (cls[x] == 2) {
            if (q == 0) mark[x] = 1;
            if (q < kcnt[(size_t)x * 2 + 1]) mark[kcol[((size_t)x * 2 + 1) * k + q]] = 1;
        }
    }
}
__global__ __launch_bounds__(256) void k_end_ranks(int I, const int *mark, const long long *rank64, int *urank, int *uitem) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I) return;
    const int r = (int)rank64[i];
    urank[i] = mark[i] ? r : -1;
    if (mark[i]) uitem[r] = i;
}

// heavy starts: add the G partial rows into the first one (double-double merge), then finalise.  One block of
// MERGE_WAVES waves per job: the touched entries of a partial row are distinct, so the waves take 64 of them at a
// time side by side (a single wave per start had left a chain of G - 1 serial merges: 68 ms at BASELINE configs[1]);
// the finalisation pass is shared the same way, every wave keeping the best of its share, wave 0 the best of those.
// Two levels for the starts with more than MERGE_GROUP rows (the heaviest has 133): level 1 folds every group of
// MERGE_GROUP consecutive rows into the group's first row (one block per group), level 2 the group heads into row 0.
constexpr int MERGE_WAVES = 16;
constexpr int MERGE_GROUP = 12;

// rows of one start: add row (acc_s, touched_s[0..nt_s)) into (acc_d, touched_d, *s_nt); all waves of the block
// (four sets of 64 entries per wave and step with all their loads in flight -- 120 VGPRs, one block per CU -- made the two
//  kernels slower: 5.35 + 6.07 ms against 4.23 + 5.45, round 4)
// An entry per lane PAIR (round 4): the even lane adds the (value, error) pair of the sums, the odd lane that of the weights --
// the two halves are independent, and every load / store instruction touches each line once: k_merge_groups 4.07 -> 3.55 ms,
// k_merge 5.62 -> 5.03 ms against an entry per lane (rocprof)
__device__ __forceinline__ void merge_row(double *acc_d, int *touched_d, int *s_nt, double *acc_s, const int *touched_s, int nt_s) {
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int half = (lane & 1) * 2;
    for (int b0 = 32 * w; b0 < nt_s; b0 += 32 * MERGE_WAVES) {
        const int b = b0 + (lane >> 1);
        bool first = false;
        int e = 0;
        if (b < nt_s) {
            e = touched_s[b];
            double *s = acc_s + (size_t)e * 4 + half, *d = acc_d + (size_t)e * 4 + half;
            double hi = d[0], lo = d[1];
            first = half == 2 && hi == 0.0;
            dd_add(hi, lo, s[0]); dd_add(hi, lo, s[1]);
            d[0] = hi; d[1] = lo;
            s[0] = 0.0; s[1] = 0.0;
        }
        const unsigned long long m = __ballot(first);
        int base = 0;
        if (lane == 0 && m) base = atomicAdd(s_nt, __popcll(m));
        base = rl32(base, 0);
        if (first) touched_d[base + __popcll(m & lanemask_lt())] = e;
    }
    __syncthreads();      // the destination row and its touched list are complete before the next row (entries repeat)
}

__global__ __launch_bounds__(64 * MERGE_WAVES) void k_merge_groups(PathArgs A, int n_heavy, const int *heavy_unit0) {
    __shared__ int s_nt;
    const int h = blockIdx.x;
    if (h >= n_heavy) return;
    const int u0 = heavy_unit0[h];
    const int G = A.unit_G[u0], r0 = A.unit_row[u0];
    if (G <= MERGE_GROUP) return;
    for (int g = blockIdx.y; g * MERGE_GROUP < G; g += gridDim.y) {
        const int b = g * MERGE_GROUP;
        const int e = (b + MERGE_GROUP) < G ? (b + MERGE_GROUP) : G;
        if (threadIdx.x == 0) s_nt = A.unit_nt[u0 + b];
        __syncthreads();
        for (int c = b + 1; c < e; c++)
            merge_row(A.hacc + (size_t)(r0 + b) * A.U * 4, A.htouched + (size_t)(r0 + b) * A.U, &s_nt,
                      A.hacc + (size_t)(r0 + c) * A.U * 4, A.htouched + (size_t)(r0 + c) * A.U, A.unit_nt[u0 + c]);
        if (threadIdx.x == 0) A.unit_nt[u0 + b] = s_nt;
        __syncthreads();
    }
}

__global__ __launch_bounds__(64 * MERGE_WAVES) void k_merge(PathArgs A, int n_heavy, const int *heavy_unit0) {
    __shared__ FinBuf fin[MERGE_WAVES];
    __shared__ int s_nt, s_ns[MERGE_WAVES], s_full;
    __shared__ unsigned long long s_off;
    const int h = blockIdx.x;
    if (h >= n_heavy) return;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const int u0 = heavy_unit0[h];
    const int start = A.unit_start[u0], G = A.unit_G[u0], r0 = A.unit_row[u0];
    double *acc0 = A.hacc + (size_t)r0 * A.U * 4;
    int *touched0 = A.htouched + (size_t)r0 * A.U;
    if (threadIdx.x == 0) s_nt = A.unit_nt[u0];
    __syncthreads();
    const int stride = G > MERGE_GROUP ? MERGE_GROUP : 1;     // group heads (k_merge_groups ran) or all rows
    for (int c = stride; c < G; c += stride)
        merge_row(acc0, touched0, &s_nt, A.hacc + (size_t)(r0 + c) * A.U * 4, A.htouched + (size_t)(r0 + c) * A.U,
                  A.unit_nt[u0 + c]);
    const int nt = s_nt;
    if (w == 0) {
        if (lane == 0) A.n_cand[start] = nt;
        unsigned long long off;
        const bool full = fin_list_offset(A, nt, start, off);
        if (lane == 0) { s_off = off; s_full = full ? 1 : 0; }
    }
    __syncthreads();
    const int ns = finalize_slice(A, fin[w], acc0, touched0, nt, s_off, s_full != 0, w, MERGE_WAVES);
    if (lane == 0) s_ns[w] = ns;
    __syncthreads();
    if (w == 0) {       // the best of the waves' best
        volatile double *bv = fin[0].v;
        volatile int *be = fin[0].e;
        int nbuf = 0;
        for (int o = 0; o < MERGE_WAVES; o++) {
            const int n = s_ns[o];
            int te = 0;
            double tv = 0.0;
            if (lane < n) { te = ((volatile int *)fin[o].oe)[lane]; tv = ((volatile double *)fin[o].ov)[lane]; }
            if (lane < n) { be[nbuf + lane] = te; bv[nbuf + lane] = tv; }
            nbuf += n;
        }
        fin_cut(fin[0], nbuf, A.top_end + (size_t)start * XMAP_TOPC, A.top_val + (size_t)start * XMAP_TOPC);
        if (lane == 0) atomicAdd(&A.counters[0], (unsigned long long)nt);
    }
}

// the partial rows of the heavy starts: groups of MERGE_GROUP rows first, then the group heads, then finalised
int merge_heavy(hipStream_t st, const PathArgs &A, int n_heavy, const int *heavy_unit0) {
    k_merge_groups<<<dim3((unsigned)n_heavy, 16), dim3(64 * MERGE_WAVES), 0, st>>>(A, n_heavy, heavy_unit0);
    XM_LAUNCH_CHECK();
    k_merge<<<dim3((unsigned)n_heavy), dim3(64 * MERGE_WAVES), 0, st>>>(A, n_heavy, heavy_unit0);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

}  // namespace xmap

using namespace xmap;

extern "C" {

int xmap_edge_ranges(void *stream, const xmap_sim *S, int32_t *h_fast_ok) {
    XM_SCOPE(stream);
    XM_ARG(S && h_fast_ok);
    *h_fast_ok = 1;
    if (S->n_items == 0) return XMAP_OK;
    hipStream_t st = (hipStream_t)stream;
    long long n = 0;
    XM_HIP(hipMemcpyAsync(&n, S->row_ptr + S->n_items, sizeof(long long), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    if (n == 0) return XMAP_OK;
    if (S->frac) { *h_fast_ok = 0; return XMAP_OK; }      // caller-supplied fractions: generic records, take the checked division
    int *bad = nullptr;
    XM_HIP(xm_malloc_async((void **)&bad, sizeof(int), st));
    XM_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
    k_edge_ranges<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(n, S->sim, S->mutu, bad);
    XM_LAUNCH_CHECK();
    int h = 0;
    XM_HIP(hipMemcpyAsync(&h, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    XM_HIP(hipStreamSynchronize(st));
    XM_HIP(xm_free_async(bad, st));
    *h_fast_ok = h ? 0 : 1;
    return XMAP_OK;
}

int xmap_end_universe(void *stream, const xmap_ext_tables *T, int32_t *mark /*[I] scratch*/, int64_t *rank /*[I+1] scratch*/,
                      int32_t *urank /*[I]*/, int32_t *uitem /*[I]*/, int64_t *h_n_ends) {
    XM_ARG(T && mark && rank && urank && uitem && h_n_ends);
    const int I = T->n_items, k = T->top_k;
    *h_n_ends = 0;
    if (I == 0) return XMAP_OK;
    hipStream_t st = (hipStream_t)stream;
    long long h_n[2];
    XM_HIP(hipMemcpyAsync(&h_n[0], T->src_ptr + I, sizeof(long long), hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemcpyAsync(&h_n[1], T->att_ptr + I, sizeof(long long), hipMemcpyDeviceToHost, st));
    XM_HIP(hipMemsetAsync(mark, 0, sizeof(int32_t) * (size_t)I, st));
    XM_HIP(hipStreamSynchronize(st));
    long long n = (long long)I * k;
    if (h_n[0] > n) n = h_n[0];
    if (h_n[1] > n) n = h_n[1];
    k_mark_ends<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(I, k, T->cls, T->kcnt, T->kcol, h_n[0], T->src_idx, h_n[1],
                                                                          T->att_idx, mark);
    XM_LAUNCH_CHECK();
    int rc = xmap_exclusive_scan_i32_to_i64(stream, mark, rank, I, h_n_ends);
    if (rc) return rc;
    k_end_ranks<<<dim3((unsigned)((I + 255) / 256)), dim3(256), 0, st>>>(I, mark, (const long long *)rank, urank, uitem);
    XM_LAUNCH_CHECK();
    return XMAP_OK;
}

int xmap_extend_cols_slots(int32_t *h_n_slots) {
    XM_ARG(h_n_slots);
    int dev = 0;
    hipDeviceProp_t prop;
    XM_HIP(hipGetDevice(&dev));
    XM_HIP(hipGetDeviceProperties(&prop, dev));
    *h_n_slots = prop.multiProcessorCount * 4 * P_WAVES;
    return XMAP_OK;
}

int xmap_extend_cols(void *stream, const xmap_ext_tables *T, const xmap_path_units *Un, const xmap_path_rows *R,
                      const xmap_path_out *O, int fast_div, int64_t *d_counters, int64_t *h_counters) {
    XM_SCOPE(stream);
    XM_ARG(T && Un && R && O && d_counters);
    XM_ARG(T->cls && T->kcnt && T->kcol && T->kval && T->flags && T->att_ptr && T->src_ptr && T->rnn_ptr);
    XM_ARG(T->n_ends >= 0 && (T->n_items == 0 || (T->urank && T->uitem)));
    XM_ARG(R->n_slots > 0 && R->acc && R->touched && O->n_cand && O->top_end && O->top_val);
    XM_ARG(Un->n_units >= 0 && Un->n_heavy >= 0);
    XM_ARG(Un->n_units == 0 || (Un->unit_start && Un->unit_c && Un->unit_G && Un->unit_row && Un->unit_nt));
    XM_ARG(Un->n_units == 0 || T->n_nb == 0 || (T->nb_id && T->nb_list && T->midX && T->dir && T->dir_ptr));
    XM_ARG(Un->n_heavy == 0 || (Un->heavy_unit0 && R->hacc && R->htouched));
    XM_ARG(O->xs_cap == 0 || (O->xs_off && O->xs_end && O->xs_val));
    hipStream_t st = (hipStream_t)stream;
    XM_HIP(hipMemsetAsync(d_counters, 0, 8 * sizeof(int64_t), st));
    if (Un->n_units > 0) {
        Path2Args B;
        memset(&B, 0, sizeof(B));
        PathArgs &A = B.P;
        A = path_args(T, Un, R, O, d_counters);
        A.U = T->n_ends; A.urank = T->urank; A.uitem = T->uitem; A.row_stride = T->n_ends;      // rows indexed by end rank
        B.nb_id = T->nb_id; B.nb_list = T->nb_list; B.n_nb = T->n_nb; B.midX = (const MidX *)T->midX; B.dir = (const MidDir *)T->dir;
        B.dir_ptr = (const long long *)T->dir_ptr; B.ng = nullptr;
        ColEnd *cend = nullptr;
        int *home = nullptr;
        if (T->n_nb > 0) {
            const long long n = (long long)T->n_nb * (T->top_k + 1);
            XM_HIP(xm_malloc_async((void **)&cend, sizeof(ColEnd) * (size_t)n, st));
            XM_HIP(xm_malloc_async((void **)&home, sizeof(int) * (size_t)T->n_items, st));
            XM_HIP(hipMemsetAsync(home, 0x7f, sizeof(int) * (size_t)T->n_items, st));
            const dim3 cgrid((unsigned)((n + 255) / 256));
            k_col_home<<<cgrid, dim3(256), 0, st>>>(T->n_nb, T->top_k, T->nb_list, T->kcnt, T->kcol, home);
            XM_LAUNCH_CHECK();
            k_col_ends<<<cgrid, dim3(256), 0, st>>>(T->n_nb, T->top_k, T->nb_list, T->kcnt, T->kcol, T->kval, T->urank, home, cend);
            XM_LAUNCH_CHECK();
            XM_HIP(xm_free_async(home, st));
        }
        B.cend = cend;
        const dim3 grid((unsigned)((A.n_slots + 3) / 4)), block(256);
        if (fast_div) k_paths4<true><<<grid, block, 0, st>>>(B);
        else k_paths4<false><<<grid, block, 0, st>>>(B);
        XM_LAUNCH_CHECK();
        if (cend) XM_HIP(xm_free_async(cend, st));
        if (Un->n_heavy > 0) {
            const int rc = merge_heavy(st, A, Un->n_heavy, Un->heavy_unit0);
            if (rc) return rc;
        }
    }
    if (h_counters) {
        XM_HIP(hipMemcpyAsync(h_counters, d_counters, 8 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        XM_HIP(hipStreamSynchronize(st));
        if (O->xs_cap > 0 && h_counters[0] > O->xs_cap) {
            set_error("candidate buffer too small: need %lld entries, have %lld", (long long)h_counters[0], (long long)O->xs_cap);
            return XMAP_ERR_CAPACITY;
        }
    }
    return XMAP_OK;
}
}
