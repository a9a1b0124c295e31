// Full-covariance Gaussian vector emissions of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables: state s of problem b emits a
// vector y in R^D, 1 <= D <= kFullMaxDim, y ~ N(mean[b][s], cov[b][s]); cov is [D][D] and only its lower triangle (i >= j) is read
// (cpprob_hip_batch_begin_problems_full, _retable_full*, _full_stats*, _mstep_full_device).  As for every family, only what WRITES rows
// and tables, and the statistic the M-step needs, is stated here:
//   factor          full_factor, Cholesky column by column: for j = 0..D-1 and i = j..D-1, a = cov[i][j], then for p = 0..j-1 ascending
//                   a = a - dmul_rn(L[i][p], L[j][p]); i == j: L[j][j] = sqrt(a); i > j: L[i][j] = a / L[j][j], a real division.  It
//                   fails where an entry read is not finite or a pivot has !(a > 0) or scale_bad(sqrt(a)): kRetableBadCov.  L is
//                   packed, entry (i, j) at i (i + 1) / 2 + j, kFullTri = 136 doubles a state
//   log_norm        diag_log_norm on the pivots: ((0.0 + scale_log_norm(L[0][0])) + scale_log_norm(L[1][1])) + ...
//   rows            full_entry, forward substitution: z_i = ((y_i - mean_i) - sum over p < i of dmul_rn(L[i][p], z_p)) / L[i][i], the
//                   subtractions ascending over p; q = ((0.0 + z_0 z_0) + z_1 z_1) + ...; ll[s] = (q + log_norm[s]) (-0.5); -inf where
//                   any |y_d| is infinite, and for s >= k.  With a diagonal cov = sigma^2 every product is a zero and every pivot is
//                   sigma again: the rows and log_norms are diag_entry's bits, and at D = 1 scale_entry's
//   check           retable_check's two bits on the transition rows, kRetableBadMean for a mean that is not finite, kRetableBadCov
//   record          kFullStats (1304) doubles a problem: the 88 of batch_smooth_stats_kernel with coordinate 0 as the observe, then
//                   sy[s][d] = sum over t of g_t[s] y_t[d] at 88 + 16 s + d and syy[s][i][j] = sum over t of g_t[s] (y_t[i] y_t[j]),
//                   j <= i, at 216 + 136 s + i (i + 1) / 2 + j, each one addition a step from 0.0 in the walk's order t = T-1 .. 0,
//                   every product one dmul_rn; slots with s >= k or i >= D are 0.0
//   M-step          full_mstep: the transition row as retable_mstep forms it; for a state with occ > 0: mean' = sy / occ,
//                   c[i][j] = syy[i][j] / occ - dmul_rn(mean'_i, mean'_j), a diagonal entry c >= floor floor ? c : floor floor (a NaN
//                   takes the floor too); the candidate goes through full_factor, and where it does not factor the state keeps mean
//                   and covariance as a state without mass does; else the mean and both triangles of cov are written.  So a re-table
//                   never refuses an M-step's output
// Every function of this file runs with fp contract off.  tests/full_ref.py restates all of it.
//
// batch_retable_full_kernel: the re-table grid (blockIdx.x the problem, blockIdx.y strides over tiles of kRetableRows steps, eight lanes
// a row, lane s the state).  Prologue: thread (s, i), s = tid >> 4 and i = tid & 15, owns row i of state s's factor in sixteen registers
// (128 threads work, two wavefronts).  The columns go in sequence and the pivot row's entries are taken by __shfl inside the 16-lane
// group, not from LDS: the exchange stays inside a wavefront, so the sixteen columns need no workgroup barrier (an LDS row would need one
// a column, 16 barriers of 256 threads for the work of 128), and the loops are fully unrolled so that the row never leaves registers.
// Every thread of the two wavefronts runs every shuffle (rows and columns outside (k, D) work on zeros and flag nothing).  The
// operations of an entry are full_factor's, in its order: the same bits.  __syncthreads_or joins one status bit at a time; a problem
// with a bit set keeps rows, words and tables and leaves after the joins, before any barrier only some threads would reach.  L is staged
// TRANSPOSED in LDS, entry (s, idx) at 8 idx + s (8704 B), the means alike at 8 d + s: the eight lanes of a row read 64 consecutive
// bytes an index.  The observes of a tile, kRetableRows x D doubles contiguous in global memory, are loaded coalesced into an LDS tile of
// row stride kFullTileStride = 17 doubles (odd: the rows of a wavefront fall on different banks); each thread runs full_entry with z[16]
// in registers.  Workgroup y = 0 alone stores the status, the 64 threshold words and the tables in force: means [B][8][16], packed L
// [B][8][136] (read back from LDS, so the stores are consecutive), log_norms [B][8]; slots outside the table 0.0.  No atomics; no
// result depends on gridDim.y.
// batch_full_walk_kernel: batch_diag_stats_kernel's walk without sy and syy -- one wavefront a problem, kWaves problems a workgroup, at
// most kSymbolGridMax workgroups, the rest strided.  It writes the 88 doubles and, every step, the lanes (0, s) store g_t[s] into the
// workspace g[steps][8], one 64-byte store a step, off the serial chain.  No LDS, no barrier, no atomics.
// batch_full_moments_kernel: no serial chain.  A workgroup a problem (past kSymbolGridMax workgroups the problems are strided).  The
// problem's 1216 accumulators are 152 items a state (16 singles, 136 pairs) x 8 states; thread tid owns the accumulators a = tid + 256 q,
// q < 5, item = a >> 3, s = a & 7: eight neighbouring lanes share an item -- one address of the Y tile -- and read one state each of the
// g row, 64 consecutive bytes.  Tiles of 32 steps are taken from the top of the sequence downwards and the rows inside a tile descending,
// the walk's order; the Y tile (stride 17) and the g tile [32][8] are loaded coalesced into LDS.  A thread forms dmul_rn(y_i, y_j) (a
// pair) or y_d (a single) once a step and adds dmul_rn(g, .) to its register.  The accumulators are private over all of T: no
// reduction, no atomics, one barrier pair a tile with a workgroup-uniform trip count.  Slots outside (k, D) store 0.0.
// The f64 matrix instruction would fit Y^T diag(g) Y, but the order of the sums inside it is not one full_ref.py can state (an
// assumption about the instruction, not a measurement): vector code with the stated order.
// batch_mstep_full_kernel: one thread a (problem, state) running full_mstep, serial 16 x 16 work.  The candidate and its factor take 136
// doubles a thread: they stand in LDS, entry idx of thread l at kFullMstepThreads idx + l (32 threads a workgroup, 34816 B), so a
// runtime index is an address and nothing spills.
// Resources (gfx950, tools/kernel_resources.py; profiles/r42_notes.md): batch_retable_full_kernel 73 VGPRs, 15936 B LDS, scratch 0;
// batch_full_walk_kernel 106 VGPRs, no LDS, scratch 0; batch_full_moments_kernel 60 VGPRs, 6400 B LDS, scratch 0;
// batch_mstep_full_kernel 58 VGPRs, 34816 B LDS, scratch 0.
#pragma once
#include "batch_diag.hpp"

namespace cph {

constexpr int kFullMaxDim = 16;                                 // D at most: a row of the factor in sixteen registers
constexpr int kFullTri = kFullMaxDim * (kFullMaxDim + 1) / 2;   // 136: the packed lower triangle of a state
constexpr int kFullMeanSlots = 8 * kFullMaxDim;                 // (s, d) slots of a problem's means
constexpr int kFullTriSlots = 8 * kFullTri;                     // (s, idx) slots of a problem's factors
constexpr int kFullItems = kFullMaxDim + kFullTri;              // 152 accumulators a state: 16 singles, 136 pairs
constexpr int kFullStats = kSuffStats + 8 * kFullItems;         // 1304 doubles a problem
constexpr int kFullSyy = kSuffStats + kFullMeanSlots;           // 216: the first syy
constexpr int kFullTileStride = kFullMaxDim + 1;                // doubles between two rows of the observes' LDS tile: odd
constexpr int kFullAccs = (8 * kFullItems + kThreads - 1) / kThreads;   // 5 accumulators a thread of the moments kernel
constexpr int kFullMstepThreads = 32;                           // (problem, state) pairs a workgroup of the M-step
constexpr int kRetableBadCov = 64;                              // a covariance that does not factor (the bits 1 .. 32 are taken)
static_assert(kFullStats == 1304 && kFullSyy == 216 && kFullAccs == 5, "the record's layout");
static_assert(2 * kFullMeanSlots == kThreads, "a thread of the first two wavefronts owns a row of a state's factor");

__host__ __device__ inline int full_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// The factor of the packed lower triangle c (entry idx at c[idx * cs]) into L (entry idx at L[idx * ls]); L may be c itself.  false:
// it does not factor, and L holds nothing to read.
__host__ __device__ inline bool full_factor(const double* c, int cs, int D, double* L, int ls)
{
#pragma clang fp contract(off)
    for (int j = 0; j < D; ++j)
        for (int i = j; i < D; ++i) {
            double a = c[full_tri(i, j) * cs];
            if (!(fabs(a) < INFINITY)) return false;
            for (int p = 0; p < j; ++p) a = a - dmul_rn(L[full_tri(i, p) * ls], L[full_tri(j, p) * ls]);
            if (i == j) {
                if (!(a > 0.0)) return false;
                const double r = sqrt(a);
                if (scale_bad(r)) return false;
                L[full_tri(j, j) * ls] = r;
            } else L[full_tri(i, j) * ls] = a / L[full_tri(j, j) * ls];
        }
    return true;
}

// the state's log_norm from its packed factor
__host__ __device__ inline double full_log_norm(const double* L, int ls, int D)
{
#pragma clang fp contract(off)
    double tot = 0.0;
    for (int d = 0; d < D; ++d) tot = tot + scale_log_norm(L[full_tri(d, d) * ls]);
    return tot;
}

// log N(y; mean[s], L L^T) up to log_norm: y the step's D coordinates; mean the state's coordinate 0, ms doubles between two
// coordinates; L the state's packed entry 0, ls doubles between two entries (8 in the kernel's transposed staging, 1 in a packed array).
// Fully unrolled under the uniform D, so that z stays in registers on the device.
__host__ __device__ inline double full_entry(const double* y, int D, const double* mean, int ms, const double* L, int ls, double log_norm)
{
#pragma clang fp contract(off)
    double z[kFullMaxDim];
    bool inf = false;
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < kFullMaxDim; ++i) {
        z[i] = 0.0;
        if (i < D) {
            const double yi = y[i];
            if (fabs(yi) == INFINITY) inf = true;
            double a = yi - mean[i * ms];
#pragma unroll
            for (int p = 0; p < i; ++p) a = a - dmul_rn(L[(i * (i + 1) / 2 + p) * ls], z[p]);
            a = a / L[(i * (i + 1) / 2 + i) * ls];
            z[i] = a;
            q = q + dmul_rn(a, a);
        }
    }
    if (inf) return -INFINITY;
    q += log_norm;
    q *= -0.5;
    return q;
}

// the bits of one problem's full table (means [k][D], covs [k][D][D], trans [k][k]), serially: the host's validation
inline int full_check(const double* means, const double* covs, const double* trans, int k, int D)
{
#pragma clang fp contract(off)
    int bits = 0;
    double c[kFullTri];
    for (int s = 0; s < k; ++s) {
        double tot = 0.0;
        for (int j = 0; j < k; ++j) {
            const double w = trans[s * k + j];
            if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
            tot += w;
        }
        if (!(tot > 0.0)) bits |= kRetableNoMass;
        for (int d = 0; d < D; ++d) if (!(fabs(means[s * D + d]) < INFINITY)) bits |= kRetableBadMean;
        for (int i = 0; i < D; ++i) for (int j = 0; j <= i; ++j) c[full_tri(i, j)] = covs[((size_t)s * D + i) * D + j];
        if (!full_factor(c, 1, D, c, 1)) bits |= kRetableBadCov;
    }
    return bits;
}

// entry (i, j), j <= i, of the state's candidate covariance from its record: sy [16], syy packed [136]
__host__ __device__ inline double full_candidate(const double* sy, const double* syy, double occ, int i, int j, double ff)
{
#pragma clang fp contract(off)
    const double mi = sy[i] / occ, mj = sy[j] / occ;
    double c = syy[full_tri(i, j)] / occ;
    c = c - dmul_rn(mi, mj);
    if (i == j) c = c >= ff ? c : ff;
    return c;
}

// state s of one problem's full M-step: rec its record [kFullStats]; means [k][D], covs [k][D][D] and trans [k][k] updated in place;
// work: kFullTri doubles of the caller's, entry idx at work[idx * ws]
__host__ __device__ inline void full_mstep(const double* rec, int k, int D, int s, double* means, double* covs, double* trans, double floor, double* work, int ws)
{
#pragma clang fp contract(off)
    double row = 0.0;
    for (int j = 0; j < k; ++j) row = row + rec[8 * s + j];
    if (row > 0.0) for (int j = 0; j < k; ++j) trans[s * k + j] = rec[8 * s + j] / row;
    const double occ = rec[64 + s];
    if (!(occ > 0.0)) return;
    const double* sy = rec + kSuffStats + kFullMaxDim * s;
    const double* syy = rec + kFullSyy + kFullTri * s;
    const double ff = floor * floor;
    for (int i = 0; i < D; ++i) for (int j = 0; j <= i; ++j) work[full_tri(i, j) * ws] = full_candidate(sy, syy, occ, i, j, ff);
    if (!full_factor(work, ws, D, work, ws)) return;             // (the state keeps its mean and covariance)
    // (the factor stands where the candidate stood: its entries are formed again, the same operations)
    for (int i = 0; i < D; ++i) {
        means[s * D + i] = sy[i] / occ;
        for (int j = 0; j <= i; ++j) {
            const double c = full_candidate(sy, syy, occ, i, j, ff);
            covs[((size_t)s * D + i) * D + j] = c;
            covs[((size_t)s * D + j) * D + i] = c;
        }
    }
}

struct BatchRetableFullArgs {
    const BatchProblem* prob;                  // [B]: T_b
    const int64_t* first;                      // [B]: problem b's first step in obs (the lengths before it; D doubles a step)
    const double* means;                       // [B][k][D]
    const double* covs;                        // [B][k][D][D], the lower triangle read
    const double* trans;                       // [B][k][k]
    const double* obs;                         // the observes, packed problem after problem, step after step, D doubles a step
    double* tab;                               // [B][T_max][kBatchTab]
    uint64_t* thr;                             // [B][64]
    int32_t* status;                           // [B]: 0, or the bits of full_check
    double* mean_out;                          // [B][8][16]: the means in force (slots outside the table 0.0)
    double* L_out;                             // [B][8][136]: the packed factors in force (slots outside the table 0.0)
    double* log_norm_out;                      // [B][8]: the states' log_norms (states >= k 0.0)
    int T_max, k, D;
};

__global__ __launch_bounds__(kThreads) void batch_retable_full_kernel(BatchRetableFullArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_trans[64];                              // the problem's transition rows, [k][k]
    __shared__ double s_L[kFullTriSlots];                       // transposed: entry (s, idx) at 8 idx + s
    __shared__ double s_mean[kFullMeanSlots], s_ln[kFullMeanSlots];     // transposed: entry (s, d) at 8 d + s
    __shared__ double s_log_norm[8];
    __shared__ double s_y[kRetableRows * kFullTileStride];      // a tile's observes: row r, coordinate d at 17 r + d
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, k = a.k, D = a.D;
    const int s0 = (tid >> 4) & 7, i0 = tid & 15;
    const bool owner = tid < kFullMeanSlots, in = owner && s0 < k && i0 < D;
    int bits = 0;
    if (tid < k * k) {
        const double w = a.trans[(int64_t)b * k * k + tid];
        s_trans[tid] = w;
        if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
    }
    double Lrow[kFullMaxDim], m0 = 0.0, piv = 0.0;
#pragma unroll
    for (int j = 0; j < kFullMaxDim; ++j) Lrow[j] = 0.0;
    if (owner) {                                                // (wavefront-uniform: the first two wavefronts, every lane of them)
        m0 = in ? a.means[((int64_t)b * k + s0) * D + i0] : 0.0;
        if (in && !(fabs(m0) < INFINITY)) bits |= kRetableBadMean;
        const double* cov = a.covs + (((int64_t)b * k + (in ? s0 : 0)) * D + (in ? i0 : 0)) * D;   // (row i0 of state s0; in bounds for every lane)
#pragma unroll
        for (int j = 0; j < kFullMaxDim; ++j)
            if (j < D) {                                        // (uniform)
                const bool mine = in && i0 >= j;
                double av = mine ? cov[j] : 0.0;
                if (mine && !(fabs(av) < INFINITY)) bits |= kRetableBadCov;
#pragma unroll
                for (int p = 0; p < j; ++p) av = av - dmul_rn(Lrow[p], __shfl(Lrow[p], j, kFullMaxDim));
                if (i0 == j) {
                    const double r = sqrt(av);
                    if (in && (!(av > 0.0) || scale_bad(r))) bits |= kRetableBadCov;
                    Lrow[j] = r;
                    piv = r;
                }
                const double d = __shfl(Lrow[j], j, kFullMaxDim);
                if (i0 > j) Lrow[j] = mine ? av / d : 0.0;
            }
    }
    __syncthreads();
    if (tid < k) {
        double tot = 0.0;
        for (int j = 0; j < k; ++j) tot += s_trans[tid * k + j];
        if (!(tot > 0.0)) bits |= kRetableNoMass;
    }
    // (__syncthreads_or joins a predicate, not a word: one call a bit; uniform from here on)
    bits = (__syncthreads_or(bits & kRetableBadWeight) ? kRetableBadWeight : 0) | (__syncthreads_or(bits & kRetableNoMass) ? kRetableNoMass : 0) |
           (__syncthreads_or(bits & kRetableBadMean) ? kRetableBadMean : 0) | (__syncthreads_or(bits & kRetableBadCov) ? kRetableBadCov : 0);
    if (blockIdx.y == 0 && tid == 0) a.status[b] = bits;
    if (bits) return;
    if (owner) {
        s_mean[8 * i0 + s0] = m0;
        s_ln[8 * i0 + s0] = in ? scale_log_norm(piv) : 0.0;
#pragma unroll
        for (int j = 0; j < kFullMaxDim; ++j)
            if (j <= i0) s_L[8 * (i0 * (i0 + 1) / 2 + j) + s0] = in && j < D ? Lrow[j] : 0.0;
    }
    __syncthreads();
    if (tid < 8) s_log_norm[tid] = tid < k ? diag_log_norm(s_ln + tid, D, 8) : 0.0;
    __syncthreads();
    if (blockIdx.y == 0) {
        if (owner) a.mean_out[(int64_t)b * kFullMeanSlots + tid] = m0;
        for (int e = tid; e < kFullTriSlots; e += kThreads) a.L_out[(int64_t)b * kFullTriSlots + e] = s_L[8 * (e % kFullTri) + e / kFullTri];
        if (tid < 8) a.log_norm_out[(int64_t)b * 8 + tid] = s_log_norm[tid];
        if (tid < 64) a.thr[(int64_t)b * 64 + tid] = retable_threshold(s_trans, k, tid >> 3, tid & 7);
    }
    const int s = tid & 7, r = tid >> 3;
    const int64_t T = a.prob[b].T, stride = (int64_t)gridDim.y * kRetableRows;
    const double* y = a.obs + a.first[b] * D;
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    const double log_norm = s_log_norm[s];
    // (t0, T and stride are the workgroup's: every thread takes every trip and reaches both barriers)
    for (int64_t t0 = (int64_t)blockIdx.y * kRetableRows; t0 < T; t0 += stride) {
        const int n_rows = (int)(T - t0 < kRetableRows ? T - t0 : kRetableRows), n = n_rows * D;
        const double* src = y + t0 * D;
        for (int e = tid; e < n; e += kThreads) s_y[(e / D) * kFullTileStride + e % D] = src[e];
        __syncthreads();
        if (r < n_rows) rows[(t0 + r) * kBatchTab + s] = s < k ? full_entry(s_y + r * kFullTileStride, D, s_mean + s, 8, s_L + s, 8, log_norm) : -INFINITY;
        __syncthreads();                                        // (the next trip's load overwrites the tile)
    }
}

struct BatchFullStatsArgs {
    const BatchSmoothProblem* desc;            // [B]: T, rows (first row in the m table) and trows (first step: the lengths before it)
    const double* mass;                        // the m table the counting pass left
    const uint64_t* thr;                       // as BatchSmoothArgs::thr
    const double* obs;                         // the observes packed problem after problem, D doubles a step
    double* g;                                 // [steps][8]: the walk's marginals, row trows + t (the walk writes, the moments read)
    double* stats;                             // [B][stats_stride]: kFullStats of a full batch (the walk serves csrc/batch_mix.hpp's record too)
    int B, k, D, thr_stride, stats_stride;
};

__global__ __launch_bounds__(kThreads) void batch_full_walk_kernel(BatchFullStatsArgs a)
{
#pragma clang fp contract(off)
    const int lane = lane_id(), sp = lane >> 3, s = lane & 7;
    const int D = a.D;
    for (int b = suff_uniform((int)blockIdx.x * kWaves + wave_id()); b < a.B; b += (int)gridDim.x * kWaves) {   // (wavefront-uniform)
        const BatchSmoothProblem d = a.desc[b];
        double* out = a.stats + (int64_t)b * a.stats_stride;
        const int T = d.T;
        double xi = 0.0, occ = 0.0, occ_y = 0.0, occ_yy = 0.0;
        if (T > 0) {
            const double* mass = a.mass + d.rows * 8;
            const double* y = a.obs + d.trows * D;
            double* gw = a.g + d.trows * 8;
            const double p = smooth_trans_mass(a.thr + (int64_t)b * a.thr_stride, a.k, s, sp);
            double g = smooth_marginal_start(mass + (int64_t)(T - 1) * 8, s);
            double yt = y[(int64_t)(T - 1) * D];
            if (sp == 0) gw[(int64_t)(T - 1) * 8 + s] = g;
            occ = occ + g;
            occ_y = occ_y + dmul_rn(g, yt);
            occ_yy = occ_yy + dmul_rn(g, dmul_rn(yt, yt));
            // the row and the observe of the step to come (T = 1: row 0 once more, never used)
            int tn = T - 2 > 0 ? T - 2 : 0;
            double m[8];
            double mt = smooth_load_row(mass + (int64_t)tn * 8, s, m);
            yt = y[(int64_t)tn * D];
            for (int t = T - 2; t >= 0; --t) {
                double mc[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) mc[j] = m[j];
                const double mtc = mt, yc = yt;
                tn = t > 0 ? t - 1 : 0;                             // (step 0 loads its own row again: in bounds, never used)
                mt = smooth_load_row(mass + (int64_t)tn * 8, s, m);
                yt = y[(int64_t)tn * D];
                const double term = smooth_marginal_term(mtc, mc, p, g, sp);
                xi = xi + term;
                g = smooth_marginal_sum(term, s);
                if (sp == 0) gw[(int64_t)t * 8 + s] = g;
                occ = occ + g;
                occ_y = occ_y + dmul_rn(g, yc);
                occ_yy = occ_yy + dmul_rn(g, dmul_rn(yc, yc));
            }
        }
        out[8 * s + sp] = xi;
        if (sp == 0) { out[64 + s] = occ; out[72 + s] = occ_y; out[80 + s] = occ_yy; }
    }
}

__global__ __launch_bounds__(kThreads) void batch_full_moments_kernel(BatchFullStatsArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_y[kRetableRows * kFullTileStride];      // a tile's observes: row r, coordinate d at 17 r + d
    __shared__ double s_g[kRetableRows * 8];                    // a tile's marginals
    const int tid = (int)threadIdx.x, k = a.k, D = a.D, s = tid & 7;
    // the thread's accumulators: where the item reads the Y tile, whether it is a pair, whether it lies in (k, D), where it is stored
    int yi[kFullAccs], yj[kFullAccs], at[kFullAccs];
    bool pair[kFullAccs], live[kFullAccs];
#pragma unroll
    for (int q = 0; q < kFullAccs; ++q) {
        const int item = (tid + kThreads * q) >> 3;
        int i = item, j = item;
        pair[q] = item >= kFullMaxDim;
        if (pair[q]) {
            const int idx = item - kFullMaxDim;
            i = 0;
            while ((i + 1) * (i + 2) / 2 <= idx) ++i;
            j = idx - i * (i + 1) / 2;
        }
        const bool slot = item < kFullItems;
        live[q] = slot && s < k && i < D;
        yi[q] = live[q] ? i : 0; yj[q] = live[q] ? j : 0;
        at[q] = !slot ? -1 : pair[q] ? kFullSyy + kFullTri * s + (item - kFullMaxDim) : kSuffStats + kFullMaxDim * s + item;
    }
    for (int b = (int)blockIdx.x; b < a.B; b += (int)gridDim.x) {   // (the workgroup's: every thread reaches every barrier)
        const BatchSmoothProblem d = a.desc[b];
        const int T = d.T;
        const double* y = a.obs + d.trows * D;
        const double* g = a.g + d.trows * 8;
        double acc[kFullAccs];
#pragma unroll
        for (int q = 0; q < kFullAccs; ++q) acc[q] = 0.0;
        for (int t0 = ((T - 1) / kRetableRows) * kRetableRows; T > 0 && t0 >= 0; t0 -= kRetableRows) {
            const int n_rows = T - t0 < kRetableRows ? T - t0 : kRetableRows, n = n_rows * D;
            const double* src = y + (int64_t)t0 * D;
            for (int e = tid; e < n; e += kThreads) s_y[(e / D) * kFullTileStride + e % D] = src[e];
            if (tid < n_rows * 8) s_g[tid] = g[(int64_t)t0 * 8 + tid];
            __syncthreads();
            for (int r = n_rows - 1; r >= 0; --r) {
                const double gt = s_g[8 * r + s];
#pragma unroll
                for (int q = 0; q < kFullAccs; ++q)
                    if (live[q]) {
                        const double u = s_y[r * kFullTileStride + yi[q]], w = s_y[r * kFullTileStride + yj[q]];
                        const double v = pair[q] ? dmul_rn(u, w) : u;
                        acc[q] = acc[q] + dmul_rn(gt, v);
                    }
            }
            __syncthreads();                                    // (the next tile's load overwrites both)
        }
        double* out = a.stats + (int64_t)b * kFullStats;
#pragma unroll
        for (int q = 0; q < kFullAccs; ++q) if (at[q] >= 0) out[at[q]] = live[q] ? acc[q] : 0.0;
    }
}

struct BatchMstepFullArgs {
    const double* stats;                       // [B][kFullStats]
    double* means;                             // [B][k][D]
    double* covs;                              // [B][k][D][D]
    double* trans;                             // [B][k][k]
    double floor;
    int64_t B;
    int k, D;
};

// one thread a (problem, state s < k)
__global__ __launch_bounds__(kFullMstepThreads) void batch_mstep_full_kernel(BatchMstepFullArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_work[kFullTri * kFullMstepThreads];    // entry idx of thread l at 32 idx + l
    const int64_t i = (int64_t)blockIdx.x * kFullMstepThreads + (int64_t)threadIdx.x;
    if (i >= a.B * a.k) return;
    const int64_t b = i / a.k, kd = (int64_t)a.k * a.D;
    full_mstep(a.stats + b * kFullStats, a.k, a.D, (int)(i % a.k), a.means + b * kd, a.covs + b * kd * a.D, a.trans + b * a.k * a.k, a.floor,
               s_work + threadIdx.x, kFullMstepThreads);
}

}  // namespace cph
