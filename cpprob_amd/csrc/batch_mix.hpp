// Gaussian-mixture vector emissions of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables: state s of problem b emits a vector
// y in R^D, 1 <= D <= kMixMaxDim, with the density sum over c < M of w[b][s][c] prod_d N(y_d; mean[b][s][c][d], sigma[b][s][c][d]),
// 1 <= M <= kMixMaxComp components (cpprob_hip_batch_begin_problems_mix, _retable_mix*, _mix_stats*, _mstep_mix_device).  As for every
// family, only what WRITES rows and tables, and the statistic the M-step needs, is stated here:
//   table_exp       exp(x) for x in [-1000, 0], table_log's sibling: uncontracted IEEE operations and no library call, so that the host
//                   begin's rows have the device's bits.  t = x kMixInvLn2 - 0.5, n = (int)t (towards zero: the integer nearest x / ln 2);
//                   r = (x - n kLn2Hi) - n kLn2Lo, the first product exact (kLn2Hi has 21 trailing zero bits, |n| < 2^11), |r| < 0.35;
//                   p = the Horner form of r^13 / 13! + ... + r^2 / 2! + r over the doubles of 1 / i!, one product and one sum a term,
//                   then 1.0 + p; n is added to the exponent bits.  Where the exponent field would be < 1 (a subnormal result, x below
//                   about -708.4) the result is exactly 0.0; table_exp(0.0) is exactly 1.0.  At most 1 ulp from numpy.exp over the domain
//                   (profiles/r43_notes.md: measured on the CPU)
//   weights         per state tot = ((0.0 + w_0) + w_1) + ... over c < M; lw[s][c] = table_log(w_c / tot) for w_c > 0, -inf for w_c == 0
//   log_norm        ln[s][c] = diag_log_norm over scale_log_norm(sigma[s][c][d]): the diagonal family's operations
//   rows            lc_c = lw[s][c] + diag_entry(y, D, mean[s][c], sigma[s][c], ., ln[s][c]); m = lc_0, then m = lc_c where lc_c > m,
//                   ascending; e_c = table_exp(fmax(lc_c - m, -1000.0)), and 0.0 without a call for lc_c = -inf;
//                   S = ((0.0 + e_0) + e_1) + ...; ll[s] = m + table_log(S); -inf where m = -inf (so where any |y_d| is infinite), and
//                   for s >= k.  At M = 1: lw = 0, e = 1, table_log(1) = 0, and the row is diag_entry's value
//   check           retable_check's two bits on the transition rows, kRetableBadMean and kRetableBadScale as in diag_check, and
//                   kRetableBadMixWeight (128): a weight not finite or < 0, a state whose tot is not > 0 and finite, or a positive
//                   w_c / tot that is not a normal number.  A problem with a bit set keeps rows, words and tables
//   record          kMixStats (2200) doubles a problem: the 88 of batch_smooth_stats_kernel with coordinate 0 as the observe, then a
//                   block of 33 for every (s, c) at 88 + 33 (8 s + c): occ_c, sy[d] at 1 + d, syy[d] at 17 + d.  With r = e_c / S formed
//                   again from the tables in force and v = dmul_rn(g_t[s], r), a step adds v, dmul_rn(v, y_d) and
//                   dmul_rn(v, dmul_rn(y_d, y_d)), from 0.0 in the walk's order t = T-1 .. 0.  A step with an infinite coordinate adds
//                   nothing; a state whose row is -inf has v = 0.0.  Slots outside (k, M, D) are 0.0
//   M-step          mix_mstep: the transition row as retable_mstep forms it; occ = ((0.0 + occ_0) + occ_1) + ...; for a state with
//                   occ > 0: w'_c = occ_c / occ; a component with occ_c > 0 takes mean' = sy / occ_c and
//                   sigma' = scale_sigma(occ_c, syy, mean', floor); one with occ_c == 0 keeps mean and sigma, and w'_c = 0.0.  A state
//                   without mass keeps everything
// Every function of this file runs with fp contract off and forms its products through dmul_rn.  tests/mix_ref.py restates all of it.
//
// batch_retable_mix_kernel: the re-table grid (blockIdx.x the problem, blockIdx.y strides over tiles of kRetableRows steps).  The row work
// is M times the diagonal family's, so a row takes a whole wavefront: lane (s, c) = lane >> 3, lane & 7 is one component, and a
// wavefront writes the eight rows 8 w .. 8 w + 7 of a tile in turn.  Prologue: thread tid checks the (s, c, d) slots tid + 256 q, q < 4
// (d the fast index: the loads of a component are consecutive), takes their scale_log_norms and keeps them in registers; the first
// wavefront's lane (s, c) checks its weight, forms tot by __shfl inside its 8-lane group and lw.  __syncthreads_or joins one status bit
// at a time; a problem with a bit set leaves after the joins, before any barrier only some threads would reach.  Means, sigmas and the
// coordinates' logarithms are staged TRANSPOSED, slot (s, c, d) at 64 d + 8 s + c: the 64 lanes of a row read 512 consecutive bytes a
// coordinate.  The observes of a tile go coalesced through an LDS tile of row stride kMixTileStride = 17 doubles, as in the diagonal
// kernel; all lanes of a row read one address.  The eight lc_c of a state are gathered by __shfl inside the 8-lane group, ascending, so
// m, and after one table_exp a lane the ascending sum S, stand alike on the group's lanes with no LDS round trip; lanes (s, 0) store the
// row, 64 consecutive bytes.  Workgroup y = 0 alone stores the status, the 64 threshold words and the tables in force: lw [B][64], ln
// [B][64], means and sigmas [B][64][16] (read back from LDS, so the stores are consecutive); slots outside the table 0.0.  Every trip
// count is the workgroup's.  No atomics; no result depends on gridDim.y.
// E-step: batch_full_walk_kernel (csrc/batch_full.hpp) as it is -- the serial chain, the 88 doubles and every step's marginals
// g[steps][8] -- then batch_mix_moments_kernel, which has no chain.  A workgroup a problem (past kSymbolGridMax workgroups the problems
// are strided); the tables in force are staged once a problem, slot (s, c, d) at 128 c + 8 d + s, so the eight states of a row read 64
// consecutive bytes.  Tiles of 32 steps from the top of the sequence down, the rows of a tile descending: the walk's order.  Phase A:
// thread (row, s) = tid >> 3, tid & 7 runs mix_join on its state's components, forms v_c = dmul_rn(g, e_c / S) and writes it to
// v[row][c][s] (16 KB).  Phase B: thread tid owns the accumulators a = tid + 256 q, q < 9, slot 88 + a of the record; neighbouring
// threads read neighbouring coordinates of the Y tile and mostly one v.  Column 16 of the Y tile holds 1.0, so occ_c's addition is
// dmul_rn(v, 1.0) = v and the inner loop has one form.  The accumulators are private over all of T: no reduction, no atomics, two
// barriers a tile with a workgroup-uniform trip count.
// batch_mstep_mix_kernel: one thread a (problem, state, component); the thread with c = 0 also writes the transition row.
// Resources (gfx950, tools/kernel_resources.py; profiles/r43_notes.md): batch_retable_mix_kernel 53 VGPRs, 30720 B LDS, scratch 0;
// batch_mix_moments_kernel 132 VGPRs, 38272 B LDS, scratch 0; batch_mstep_mix_kernel 30 VGPRs, no LDS, scratch 0.
#pragma once
#include "batch_full.hpp"

namespace cph {

constexpr int kMixMaxDim = 16;                                  // D at most
constexpr int kMixMaxComp = 8;                                  // M at most: a state's components are an 8-lane group
constexpr int kMixComps = 8 * kMixMaxComp;                      // (s, c) slots of a problem: a wavefront
constexpr int kMixSlots = kMixComps * kMixMaxDim;               // (s, c, d) slots of a problem's means, and of its sigmas
constexpr int kMixBlock = 1 + 2 * kMixMaxDim;                   // 33 doubles a component of the record: occ_c, sy[16], syy[16]
constexpr int kMixStats = kSuffStats + kMixComps * kMixBlock;   // 2200 doubles a problem
constexpr int kMixAccs = (kMixComps * kMixBlock + kThreads - 1) / kThreads;     // 9 accumulators a thread of the moments kernel
constexpr int kMixTileStride = kMixMaxDim + 1;                  // doubles between two rows of the observes' LDS tile: odd
constexpr int kMixChecks = kMixSlots / kThreads;                // 4 slots a thread of the re-table's check
constexpr int kRetableBadMixWeight = 128;                       // (the bits 1 .. 64 are taken)
constexpr double kMixExpFloor = -1000.0;
constexpr double kMixInvLn2 = 0x1.71547652b82fep+0;
static_assert(kMixStats == 2200 && kMixAccs == 9 && kMixChecks == 4 && kRetableRows == 32, "the record's layout and the tile");

// exp(x), x in [-1000, 0]
__host__ __device__ inline double table_exp(double x)
{
#pragma clang fp contract(off)
    double t = dmul_rn(x, kMixInvLn2);
    t = t - 0.5;
    const int n = (int)t;
    const double nd = (double)n;
    double r = x - dmul_rn(nd, kLn2Hi);
    r = r - dmul_rn(nd, kLn2Lo);
    double p = 0x1.6124613a86d09p-33;                                 // 1 / 13!
    p = dmul_rn(p, r); p = p + 0x1.1eed8eff8d898p-29;               // 1 / 12!
    p = dmul_rn(p, r); p = p + 0x1.ae64567f544e4p-26;               // 1 / 11!
    p = dmul_rn(p, r); p = p + 0x1.27e4fb7789f5cp-22;               // 1 / 10!
    p = dmul_rn(p, r); p = p + 0x1.71de3a556c734p-19;               // 1 / 9!
    p = dmul_rn(p, r); p = p + 0x1.a01a01a01a01ap-16;               // 1 / 8!
    p = dmul_rn(p, r); p = p + 0x1.a01a01a01a01ap-13;               // 1 / 7!
    p = dmul_rn(p, r); p = p + 0x1.6c16c16c16c17p-10;               // 1 / 6!
    p = dmul_rn(p, r); p = p + 0x1.1111111111111p-7;                // 1 / 5!
    p = dmul_rn(p, r); p = p + 0x1.5555555555555p-5;                // 1 / 4!
    p = dmul_rn(p, r); p = p + 0x1.5555555555555p-3;                // 1 / 3!
    p = dmul_rn(p, r); p = p + 0.5;
    p = dmul_rn(p, r); p = p + 1.0;
    p = dmul_rn(p, r);
    p = 1.0 + p;
    uint64_t u;
    __builtin_memcpy(&u, &p, sizeof u);
    const int e = (int)((u >> 52) & 0x7ffu) + n;
    if (e < 1) return 0.0;
    u = (u & 0x000fffffffffffffull) | ((uint64_t)e << 52);
    __builtin_memcpy(&p, &u, sizeof p);
    return p;
}

// a weight's share of its state's total that the route does not take (a weight of zero is taken: its share is not formed)
__host__ __device__ inline bool mix_share_bad(double w, double tot)
{
#pragma clang fp contract(off)
    return w > 0.0 && !(w / tot >= kScaleMinNormal);
}

// lw of a weight w >= 0 of a state with total tot
__host__ __device__ inline double mix_log_weight(double w, double tot)
{
#pragma clang fp contract(off)
    return w > 0.0 ? table_log(w / tot) : -INFINITY;
}

// e_c of a component from its lc and the state's m
__host__ __device__ inline double mix_exp(double lc, double m)
{
#pragma clang fp contract(off)
    return lc == -INFINITY ? 0.0 : table_exp(fmax(lc - m, kMixExpFloor));
}

// a state's row entry from its components' lc (c < M is read): e (0.0 for c >= M) and S as stated.  Fully unrolled under the uniform M,
// so that lc and e stay in registers on the device
__host__ __device__ inline double mix_join(const double (&lc)[kMixMaxComp], int M, double (&e)[kMixMaxComp], double& S)
{
#pragma clang fp contract(off)
    double m = lc[0];
#pragma unroll
    for (int c = 1; c < kMixMaxComp; ++c) if (c < M && lc[c] > m) m = lc[c];
    double tot = 0.0;
#pragma unroll
    for (int c = 0; c < kMixMaxComp; ++c) {
        e[c] = 0.0;
        if (c < M) {
            if (m != -INFINITY) e[c] = mix_exp(lc[c], m);
            tot = tot + e[c];
        }
    }
    S = tot;
    if (m == -INFINITY) return -INFINITY;
    return m + table_log(tot);
}

// a state's components' lc: y the step's D coordinates; mean and sigma the state's slot (c = 0, d = 0), cs doubles between two
// components and ds between two coordinates; lw and ln the state's entries of component 0, ws doubles between two components
__host__ __device__ inline void mix_components(const double* y, int D, int M, const double* mean, const double* sigma, int cs, int ds, const double* lw, const double* ln,
                                               int ws, double (&lc)[kMixMaxComp])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < kMixMaxComp; ++c) lc[c] = c < M ? lw[c * ws] + diag_entry(y, D, mean + c * cs, sigma + c * cs, ds, ln[c * ws]) : -INFINITY;
}

// the bits of one problem's mixture table (weights [k][M], means and sigmas [k][M][D], trans [k][k]), serially: the host's validation
// and the kernel's parallel check form these bits
inline int mix_check(const double* weights, const double* means, const double* sigmas, const double* trans, int k, int M, int D)
{
#pragma clang fp contract(off)
    int bits = 0;
    for (int s = 0; s < k; ++s) {
        double tot = 0.0;
        for (int j = 0; j < k; ++j) {
            const double w = trans[s * k + j];
            if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
            tot += w;
        }
        if (!(tot > 0.0)) bits |= kRetableNoMass;
        double wt = 0.0;
        for (int c = 0; c < M; ++c) {
            const double w = weights[s * M + c];
            if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadMixWeight;
            wt = wt + w;
        }
        if (!(wt > 0.0) || !(wt < INFINITY)) bits |= kRetableBadMixWeight;
        for (int c = 0; c < M; ++c) {
            if (mix_share_bad(weights[s * M + c], wt)) bits |= kRetableBadMixWeight;
            for (int d = 0; d < D; ++d) {
                if (!(fabs(means[(s * M + c) * D + d]) < INFINITY)) bits |= kRetableBadMean;
                if (scale_bad(sigmas[(s * M + c) * D + d])) bits |= kRetableBadScale;
            }
        }
    }
    return bits;
}

// entry (s, c) of one problem's mixture M-step: rec its record [kMixStats]; weights [k][M], means and sigmas [k][M][D] and trans [k][k]
// updated in place; c = 0 also forms the state's transition row
__host__ __device__ inline void mix_mstep(const double* rec, int k, int M, int D, int s, int c, double* weights, double* means, double* sigmas, double* trans, double floor)
{
#pragma clang fp contract(off)
    if (c == 0) {
        double row = 0.0;
        for (int j = 0; j < k; ++j) row = row + rec[8 * s + j];
        if (row > 0.0) for (int j = 0; j < k; ++j) trans[s * k + j] = rec[8 * s + j] / row;
    }
    const double* blocks = rec + kSuffStats + kMixBlock * kMixMaxComp * s;
    double occ = 0.0;
    for (int j = 0; j < M; ++j) occ = occ + blocks[kMixBlock * j];
    if (!(occ > 0.0)) return;
    const double* blk = blocks + kMixBlock * c;
    const double oc = blk[0];
    if (oc > 0.0) {
        weights[s * M + c] = oc / occ;
        for (int d = 0; d < D; ++d) {
            const double m = blk[1 + d] / oc;
            means[(s * M + c) * D + d] = m;
            sigmas[(s * M + c) * D + d] = scale_sigma(oc, blk[1 + kMixMaxDim + d], m, floor);
        }
    } else weights[s * M + c] = 0.0;
}

struct BatchRetableMixArgs {
    const BatchProblem* prob;                  // [B]: T_b
    const int64_t* first;                      // [B]: problem b's first step in obs (the lengths before it; D doubles a step)
    const double* weights;                     // [B][k][M]
    const double* means;                       // [B][k][M][D]
    const double* sigmas;                      // [B][k][M][D]
    const double* trans;                       // [B][k][k]
    const double* obs;                         // the observes, packed problem after problem, step after step, D doubles a step
    double* tab;                               // [B][T_max][kBatchTab]
    uint64_t* thr;                             // [B][64]
    int32_t* status;                           // [B]: 0, or the bits of mix_check
    double* lw_out;                            // [B][64]: the log-weights in force, (s, c) at 8 s + c (slots outside the table 0.0)
    double* ln_out;                            // [B][64]: the components' log_norms in force
    double* mean_out;                          // [B][64][16]: the means in force
    double* sigma_out;                         // [B][64][16]: the sigmas in force
    int T_max, k, M, D;
};

__global__ __launch_bounds__(kThreads) void batch_retable_mix_kernel(BatchRetableMixArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_trans[64];                              // the problem's transition rows, [k][k]
    __shared__ double s_mean[kMixSlots], s_sigma[kMixSlots];    // transposed: slot (s, c, d) at 64 d + 8 s + c
    __shared__ double s_lnd[kMixSlots];                         // scale_log_norm of every sigma, transposed alike
    __shared__ double s_lw[kMixComps], s_ln[kMixComps];         // (s, c) at 8 s + c
    __shared__ double s_y[kRetableRows * kMixTileStride];       // a tile's observes: row r, coordinate d at 17 r + d
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, k = a.k, M = a.M, D = a.D;
    const int lane = tid & 63, wave = tid >> 6, s = lane >> 3, c = lane & 7;
    const bool comp = s < k && c < M;                           // the lane's component lies in the table
    int bits = 0;
    // the thread's slots: slot e = tid + 256 q is (sc, d) = (e >> 4, e & 15)
    double m0[kMixChecks], g0[kMixChecks];
#pragma unroll
    for (int q = 0; q < kMixChecks; ++q) {
        const int e = tid + kThreads * q, sc = e >> 4, d = e & 15;
        const bool in = (sc >> 3) < k && (sc & 7) < M && d < D;
        const int64_t at = (((int64_t)b * k + (sc >> 3)) * M + (sc & 7)) * D + d;
        m0[q] = in ? a.means[at] : 0.0;
        g0[q] = in ? a.sigmas[at] : 0.0;
        if (in && !(fabs(m0[q]) < INFINITY)) bits |= kRetableBadMean;
        if (in && scale_bad(g0[q])) bits |= kRetableBadScale;
    }
    if (tid < k * k) {
        const double w = a.trans[(int64_t)b * k * k + tid];
        s_trans[tid] = w;
        if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
    }
    double w0 = 0.0, wt = 0.0;
    if (wave == 0) {                                            // (wavefront-uniform: every lane of the first wavefront runs every shuffle)
        w0 = comp ? a.weights[((int64_t)b * k + s) * M + c] : 0.0;
        if (!(w0 >= 0.0) || !(fabs(w0) < INFINITY)) bits |= kRetableBadMixWeight;
        for (int j = 0; j < M; ++j) wt = wt + __shfl(w0, j, kMixMaxComp);
        if (s < k && (!(wt > 0.0) || !(wt < INFINITY))) bits |= kRetableBadMixWeight;
        if (comp && mix_share_bad(w0, wt)) bits |= kRetableBadMixWeight;
    }
    __syncthreads();
    if (tid < k) {
        double tot = 0.0;
        for (int j = 0; j < k; ++j) tot += s_trans[tid * k + j];
        if (!(tot > 0.0)) bits |= kRetableNoMass;
    }
    // (__syncthreads_or joins a predicate, not a word: one call a bit; uniform from here on)
    bits = (__syncthreads_or(bits & kRetableBadWeight) ? kRetableBadWeight : 0) | (__syncthreads_or(bits & kRetableNoMass) ? kRetableNoMass : 0) |
           (__syncthreads_or(bits & kRetableBadMean) ? kRetableBadMean : 0) | (__syncthreads_or(bits & kRetableBadScale) ? kRetableBadScale : 0) |
           (__syncthreads_or(bits & kRetableBadMixWeight) ? kRetableBadMixWeight : 0);
    if (blockIdx.y == 0 && tid == 0) a.status[b] = bits;
    if (bits) return;
#pragma unroll
    for (int q = 0; q < kMixChecks; ++q) {
        const int e = tid + kThreads * q, sc = e >> 4, d = e & 15;
        const bool in = (sc >> 3) < k && (sc & 7) < M && d < D;
        s_mean[64 * d + sc] = m0[q];
        s_sigma[64 * d + sc] = g0[q];
        s_lnd[64 * d + sc] = in ? scale_log_norm(g0[q]) : 0.0;
    }
    if (wave == 0) s_lw[lane] = comp ? mix_log_weight(w0, wt) : 0.0;
    __syncthreads();
    if (wave == 0) s_ln[lane] = comp ? diag_log_norm(s_lnd + lane, D, kMixComps) : 0.0;
    __syncthreads();
    if (blockIdx.y == 0) {
        for (int e = tid; e < kMixSlots; e += kThreads) {
            a.mean_out[(int64_t)b * kMixSlots + e] = s_mean[64 * (e & 15) + (e >> 4)];
            a.sigma_out[(int64_t)b * kMixSlots + e] = s_sigma[64 * (e & 15) + (e >> 4)];
        }
        if (tid < kMixComps) {
            a.lw_out[(int64_t)b * kMixComps + tid] = s_lw[tid];
            a.ln_out[(int64_t)b * kMixComps + tid] = s_ln[tid];
            a.thr[(int64_t)b * 64 + tid] = retable_threshold(s_trans, k, tid >> 3, tid & 7);
        }
    }
    const int64_t T = a.prob[b].T, stride = (int64_t)gridDim.y * kRetableRows;
    const double* y = a.obs + a.first[b] * D;
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    const double lw = s_lw[lane], ln = s_ln[lane];
    // (t0, T and stride are the workgroup's: every thread takes every trip and reaches both barriers)
    for (int64_t t0 = (int64_t)blockIdx.y * kRetableRows; t0 < T; t0 += stride) {
        const int n_rows = (int)(T - t0 < kRetableRows ? T - t0 : kRetableRows), n = n_rows * D;
        const double* src = y + t0 * D;
        for (int e = tid; e < n; e += kThreads) s_y[(e / D) * kMixTileStride + e % D] = src[e];
        __syncthreads();
        // (the wavefront's rows 8 wave .. 8 wave + 7: r and n_rows are the wavefront's, so every lane runs every shuffle)
        for (int r = 8 * wave; r < 8 * wave + 8 && r < n_rows; ++r) {
            const double lc = comp ? lw + diag_entry(s_y + r * kMixTileStride, D, s_mean + lane, s_sigma + lane, kMixComps, ln) : -INFINITY;
            double m = __shfl(lc, 0, kMixMaxComp);
            for (int j = 1; j < M; ++j) {
                const double o = __shfl(lc, j, kMixMaxComp);
                if (o > m) m = o;
            }
            const double e = m != -INFINITY && c < M ? mix_exp(lc, m) : 0.0;
            double S = 0.0;
            for (int j = 0; j < M; ++j) S = S + __shfl(e, j, kMixMaxComp);
            if (c == 0) rows[(t0 + r) * kBatchTab + s] = s < k && m != -INFINITY ? m + table_log(S) : -INFINITY;
        }
        __syncthreads();                                        // (the next trip's load overwrites the tile)
    }
}

struct BatchMixMomentsArgs {
    const BatchSmoothProblem* desc;            // [B]: T and trows (first step: the lengths before it)
    const double* obs;                         // the observes packed problem after problem, D doubles a step
    const double* g;                           // [steps][8]: the walk's marginals, row trows + t
    const double* lw;                          // [B][64], and below: the tables in force, as batch_retable_mix_kernel leaves them
    const double* ln;                          // [B][64]
    const double* mean;                        // [B][64][16]
    const double* sigma;                       // [B][64][16]
    double* stats;                             // [B][kMixStats]: the slots 88 .. are written
    int B, k, M, D;
};

__global__ __launch_bounds__(kThreads) void batch_mix_moments_kernel(BatchMixMomentsArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_mean[kMixSlots], s_sigma[kMixSlots];    // slot (s, c, d) at 128 c + 8 d + s
    __shared__ double s_lw[kMixComps], s_ln[kMixComps];         // (s, c) at 8 c + s
    __shared__ double s_v[kRetableRows * kMixComps];            // a tile's v: row r, (s, c) at 64 r + 8 c + s
    __shared__ double s_y[kRetableRows * kMixTileStride];       // a tile's observes: row r, coordinate d at 17 r + d; column 16 is 1.0
    __shared__ int s_ok[kRetableRows];                          // the row has no infinite coordinate
    const int tid = (int)threadIdx.x, k = a.k, M = a.M, D = a.D, s = tid & 7, row = tid >> 3;
    // the thread's accumulators: slot 88 + a of the record, a = tid + 256 q; where it reads v and the Y tile, whether y is squared
    int vat[kMixAccs], yat[kMixAccs];
    bool sq[kMixAccs], live[kMixAccs], slot[kMixAccs];
#pragma unroll
    for (int q = 0; q < kMixAccs; ++q) {
        const int acc = tid + kThreads * q, sc = acc / kMixBlock, item = acc - sc * kMixBlock;
        const int d = item == 0 ? 0 : (item - 1) & 15;
        slot[q] = acc < kMixComps * kMixBlock;
        live[q] = slot[q] && (sc >> 3) < k && (sc & 7) < M && d < D;
        sq[q] = item > kMixMaxDim;
        vat[q] = live[q] ? 8 * (sc & 7) + (sc >> 3) : 0;
        yat[q] = !live[q] ? 0 : item == 0 ? kMixMaxDim : d;
    }
    if (tid < kRetableRows) s_y[tid * kMixTileStride + kMixMaxDim] = 1.0;
    for (int b = (int)blockIdx.x; b < a.B; b += (int)gridDim.x) {   // (the workgroup's: every thread reaches every barrier)
        const BatchSmoothProblem d = a.desc[b];
        const int T = d.T;
        const double* y = a.obs + d.trows * D;
        const double* g = a.g + d.trows * 8;
        __syncthreads();                                        // (the problem before this one has read its tables)
        for (int e = tid; e < kMixSlots; e += kThreads) {
            const int sc = e >> 4, at = 128 * (sc & 7) + 8 * (e & 15) + (sc >> 3);
            s_mean[at] = a.mean[(int64_t)b * kMixSlots + e];
            s_sigma[at] = a.sigma[(int64_t)b * kMixSlots + e];
        }
        if (tid < kMixComps) {
            s_lw[8 * (tid & 7) + (tid >> 3)] = a.lw[(int64_t)b * kMixComps + tid];
            s_ln[8 * (tid & 7) + (tid >> 3)] = a.ln[(int64_t)b * kMixComps + tid];
        }
        double acc[kMixAccs];
#pragma unroll
        for (int q = 0; q < kMixAccs; ++q) acc[q] = 0.0;
        for (int t0 = ((T - 1) / kRetableRows) * kRetableRows; T > 0 && t0 >= 0; t0 -= kRetableRows) {
            const int n_rows = T - t0 < kRetableRows ? T - t0 : kRetableRows, n = n_rows * D;
            const double* src = y + (int64_t)t0 * D;
            for (int e = tid; e < n; e += kThreads) s_y[(e / D) * kMixTileStride + e % D] = src[e];
            __syncthreads();                                    // (the tile, and on the first trip the tables)
            // phase A: thread (row, s)
            if (row < n_rows) {
                const double* yr = s_y + row * kMixTileStride;
                double v[kMixMaxComp];
#pragma unroll
                for (int c = 0; c < kMixMaxComp; ++c) v[c] = 0.0;
                if (s < k) {
                    double lc[kMixMaxComp], e[kMixMaxComp], S;
                    mix_components(yr, D, M, s_mean + s, s_sigma + s, 128, 8, s_lw + s, s_ln + s, 8, lc);
                    const double ll = mix_join(lc, M, e, S);
                    const double gt = g[(int64_t)(t0 + row) * 8 + s];
                    if (ll != -INFINITY) {
#pragma unroll
                        for (int c = 0; c < kMixMaxComp; ++c) if (c < M) v[c] = dmul_rn(gt, e[c] / S);
                    }
                }
#pragma unroll
                for (int c = 0; c < kMixMaxComp; ++c) s_v[kMixComps * row + 8 * c + s] = v[c];
                if (s == 0) {
                    bool fin = true;
                    for (int dd = 0; dd < D; ++dd) if (fabs(yr[dd]) == INFINITY) fin = false;
                    s_ok[row] = fin ? 1 : 0;
                }
            }
            __syncthreads();
            // phase B: thread tid's accumulators over the tile's rows, descending
            for (int r = n_rows - 1; r >= 0; --r) {
                if (!s_ok[r]) continue;                         // (the workgroup's)
#pragma unroll
                for (int q = 0; q < kMixAccs; ++q)
                    if (live[q]) {
                        const double u = s_y[r * kMixTileStride + yat[q]];
                        const double f = sq[q] ? dmul_rn(u, u) : u;
                        acc[q] = acc[q] + dmul_rn(s_v[kMixComps * r + vat[q]], f);
                    }
            }
            __syncthreads();                                    // (the next tile's load overwrites the tile and v)
        }
        double* out = a.stats + (int64_t)b * kMixStats + kSuffStats;
#pragma unroll
        for (int q = 0; q < kMixAccs; ++q) if (slot[q]) out[tid + kThreads * q] = live[q] ? acc[q] : 0.0;
    }
}

struct BatchMstepMixArgs {
    const double* stats;                       // [B][kMixStats]
    double* weights;                           // [B][k][M]
    double* means;                             // [B][k][M][D]
    double* sigmas;                            // [B][k][M][D]
    double* trans;                             // [B][k][k]
    double floor;
    int64_t B;
    int k, M, D;
};

// one thread a (problem, state s < k, component c < M)
__global__ __launch_bounds__(kThreads) void batch_mstep_mix_kernel(BatchMstepMixArgs a)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x, km = (int64_t)a.k * a.M;
    if (i >= a.B * km) return;
    const int64_t b = i / km;
    const int sc = (int)(i % km);
    mix_mstep(a.stats + b * kMixStats, a.k, a.M, a.D, sc / a.M, sc % a.M, a.weights + b * km, a.means + b * km * a.D, a.sigmas + b * km * a.D, a.trans + b * a.k * a.k, a.floor);
}

}  // namespace cph
