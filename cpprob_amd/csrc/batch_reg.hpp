// Switching-regression emissions of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables: state s of problem b emits the scalar
// y_t ~ N(sum over i of coef[b][s][i] x_t[i], sigma[b][s]) on 1 <= P <= kRegMaxCov covariates known at the step
// (cpprob_hip_batch_begin_problems_reg, _retable_reg*, _reg_stats*, _mstep_reg_device).  A step's observe is the 1 + P doubles
// z_t = (y_t, x_t[0], .., x_t[P-1]): the response first, so that coordinate 0 is the observe of the 88-double record as for every
// family.  An intercept is a covariate column of ones; none is added here.  The autoregressive HMM is the case x_t = (1, y_{t-1}, ..).
// As for every family, only what WRITES rows and tables, and what solves the M-step, is stated here:
//   rows            reg_entry: pred = 0.0, then ascending over i pred = pred + dmul_rn(coef[s][i], x[i]); the entry is
//                   scale_entry(y, pred, sigma[s], log_norm[s]), log_norm = scale_log_norm(sigma); -inf where y or any covariate is
//                   infinite, and for s >= k
//   check           retable_check's two bits on the transition rows, kRetableBadMean for a coefficient that is not finite,
//                   kRetableBadScale for a sigma scale_bad refuses
//   record          the full family's kFullStats (1304) doubles at D = 1 + P, as batch_full_walk_kernel and batch_full_moments_kernel
//                   leave them: with syy the packed triangle of sum over t of g_t[s] z_t z_t^T, c0 = syy[s][0][0],
//                   b_i = syy[s][1+i][0], A_ij = syy[s][1+i][1+j], j <= i
//   M-step          reg_mstep: the transition row as retable_mstep forms it.  For a state with occ > 0 the normal equations
//                   A beta = b go through the square-root-free factorisation A = L D L^T, L unit lower, column by column: for
//                   j = 0..P-1 and i = j..P-1, a = A_ij, then for p = 0..j-1 ascending a = a - dmul_rn(W[i][p], L[j][p]); i == j:
//                   d_j = a; i > j: W[i][j] = a and L[i][j] = a / d_j, a real division (W = L D, so every term is ONE product).
//                   Forward solve: u_i = b_i, then for p = 0..i-1 ascending u_i = u_i - dmul_rn(L[i][p], u_p).  w_i = u_i / d_i.
//                   Back solve, by columns from the last: beta = w, then for p = P-1 down to 1 and every i < p
//                   beta_i = beta_i - dmul_rn(L[p][i], beta_p): the subtractions of an entry DESCEND over p.  Then v = c0 / occ and
//                   ascending over i v = v - dmul_rn(beta_i, b_i / occ); sigma' = sqrt(v) where v >= floor floor, else floor (a NaN
//                   takes the floor too); log_norm' = scale_log_norm(sigma').  The state keeps coefficients and sigma, as a state
//                   without mass does, where occ, c0, a b_i or an A_ij is not finite, a pivot has !(d > 0) or is not finite, or a
//                   solved coefficient is not finite: a re-table never refuses an M-step's coefficients
// At P = 1 with the covariate identically 1.0 the record's A_00, b_0 and c0 are occ's, occ_y's and occ_yy's bits, the pivot is occ,
// beta = occ_y / occ and v = occ_yy / occ - beta beta: rows, log_norms, threshold words and M-step are the scaled family's bit for bit.
// A duplicated covariate column gives L[1][0] = 1.0 and a second pivot of exactly 0.0: the state is kept.
// Every function of this file runs with fp contract off.  tests/reg_ref.py restates all of it.
//
// batch_retable_reg_kernel: the re-table grid (blockIdx.x the problem, blockIdx.y strides over tiles of kRetableRows steps, eight lanes
// a row, lane s the state).  Thread (s, i), s = tid >> 4 and i = tid & 15 (the first two wavefronts), checks coefficient (s, i) and
// stages it TRANSPOSED in LDS, entry (s, i) at 8 i + s: the eight lanes of a row read 64 consecutive bytes an index; thread s < 8 checks
// one sigma and takes its one logarithm.  __syncthreads_or joins one status bit at a time; a problem with a bit set keeps rows, words
// and tables and leaves after the joins.  A tile's kRetableRows x (1 + P) observes, contiguous in global memory, are loaded coalesced
// into an LDS tile of row stride kFullTileStride = 17 doubles; each thread runs reg_entry, unrolled under the uniform P.  Workgroup
// y = 0 alone stores the status, the 64 threshold words and the tables in force: coef [B][8][16], sigma [B][8], log_norm [B][8], slots
// outside the table 0.0.  No atomics; no result depends on gridDim.y.
// batch_mstep_reg_kernel: a state is a 16-lane group, lane i holds row i of A, of W and of L and b_i in registers; 128 threads serve a
// problem, a 256-thread workgroup two problems, at most kRegMstepGridMax workgroups, the rest strided.  The pivot, the pivot row's
// L[j][p], the solved u_p and beta_p and the column entries L[p][i] of the back solve travel by __shfl inside the group; every lane of
// a wavefront runs every shuffle (rows outside (k, P) work on zeros and store nothing), the loops are fully unrolled, there is no LDS
// and no barrier.  What a state must agree on -- a non-finite entry or coefficient of any lane -- is one __ballot, read by group.  The
// operations of an entry are reg_mstep's, in its order: the same bits.
// The E-step is batch_full_walk_kernel and batch_full_moments_kernel as they are, at D = 1 + P.
// Resources (gfx950, tools/kernel_resources.py; profiles/r44_notes.md): batch_retable_reg_kernel 30 VGPRs, 6272 B LDS, scratch 0;
// batch_mstep_reg_kernel 161 VGPRs, no LDS, scratch 0, nothing spilled.
#pragma once
#include "batch_full.hpp"

namespace cph {

constexpr int kRegMaxCov = kFullMaxDim - 1;                     // P at most: 1 + P coordinates fit the full family's tile and record
constexpr int kRegCoefSlots = 8 * kFullMaxDim;                  // (s, i) slots of a problem's coefficients, [8][16]
constexpr int kRegMstepGridMax = 2048;                          // workgroups of the M-step at most: two problems each, the rest strided
static_assert(kRegCoefSlots == kThreads / 2, "a thread of the first two wavefronts owns a coefficient; half a workgroup a problem's M-step");

// log N(y; coef . x, sigma) up to log_norm: z the step's 1 + P doubles (y, x); coef the state's coefficient 0, cs doubles between two
// coefficients (8 in the kernel's transposed staging, 1 in a packed array).  Fully unrolled under the uniform P.
__host__ __device__ inline double reg_entry(const double* z, int P, const double* coef, int cs, double sigma, double log_norm)
{
#pragma clang fp contract(off)
    double pred = 0.0;
    bool inf = false;
#pragma unroll
    for (int i = 0; i < kRegMaxCov; ++i)
        if (i < P) {
            const double x = z[1 + i];
            if (fabs(x) == INFINITY) inf = true;
            pred = pred + dmul_rn(coef[i * cs], x);
        }
    if (inf) return -INFINITY;
    return scale_entry(z[0], pred, sigma, log_norm);
}

// the bits of one problem's regression table (coef [k][P], sigmas [k], trans [k][k]), serially: the host's validation
__host__ __device__ inline int reg_check(const double* coef, const double* sigmas, const double* trans, int k, int P)
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
        for (int i = 0; i < P; ++i) if (!(fabs(coef[s * P + i]) < INFINITY)) bits |= kRetableBadMean;
        if (scale_bad(sigmas[s])) bits |= kRetableBadScale;
    }
    return bits;
}

// state s of one problem's regression M-step: rec its record [kFullStats]; coef [k][P], sigmas [k], log_norms [k] (may be null) and
// trans [k][k] updated in place.  Serial: the statement the device's 16-lane form is held to.
__host__ __device__ inline void reg_mstep(const double* rec, int k, int P, int s, double* coef, double* sigmas, double* log_norms, double* trans, double floor)
{
#pragma clang fp contract(off)
    double row = 0.0;
    for (int j = 0; j < k; ++j) row = row + rec[8 * s + j];
    if (row > 0.0) for (int j = 0; j < k; ++j) trans[s * k + j] = rec[8 * s + j] / row;
    const double occ = rec[64 + s];
    if (!(occ > 0.0) || !(occ < INFINITY)) return;
    const double* syy = rec + kFullSyy + kFullTri * s;
    const double c0 = syy[0];
    if (!(fabs(c0) < INFINITY)) return;
    double W[kFullTri], L[kFullTri], d[kRegMaxCov], beta[kRegMaxCov];
    for (int j = 0; j < P; ++j)
        for (int i = j; i < P; ++i) {
            double a = syy[full_tri(1 + i, 1 + j)];
            if (!(fabs(a) < INFINITY)) return;
            for (int p = 0; p < j; ++p) a = a - dmul_rn(W[full_tri(i, p)], L[full_tri(j, p)]);
            if (i == j) {
                if (!(a > 0.0) || !(a < INFINITY)) return;      // (the state keeps its coefficients and sigma)
                d[j] = a;
            } else { W[full_tri(i, j)] = a; L[full_tri(i, j)] = a / d[j]; }
        }
    for (int i = 0; i < P; ++i) {
        double u = syy[full_tri(1 + i, 0)];
        if (!(fabs(u) < INFINITY)) return;
        for (int p = 0; p < i; ++p) u = u - dmul_rn(L[full_tri(i, p)], beta[p]);
        beta[i] = u;                                            // (u_i: divided once every u stands)
    }
    for (int i = 0; i < P; ++i) beta[i] = beta[i] / d[i];
    for (int p = P - 1; p >= 1; --p)
        for (int i = 0; i < p; ++i) beta[i] = beta[i] - dmul_rn(L[full_tri(p, i)], beta[p]);
    for (int i = 0; i < P; ++i) if (!(fabs(beta[i]) < INFINITY)) return;
    double v = c0 / occ;
    for (int i = 0; i < P; ++i) v = v - dmul_rn(beta[i], syy[full_tri(1 + i, 0)] / occ);
    const double ff = floor * floor;
    const double sg = v >= ff ? sqrt(v) : floor;
    for (int i = 0; i < P; ++i) coef[s * P + i] = beta[i];
    sigmas[s] = sg;
    if (log_norms) log_norms[s] = scale_bad(sg) ? NAN : scale_log_norm(sg);          // (a scale the check refuses has no logarithm here)
}

struct BatchRetableRegArgs {
    const BatchProblem* prob;                  // [B]: T_b
    const int64_t* first;                      // [B]: problem b's first step in obs (the lengths before it; 1 + P doubles a step)
    const double* coef;                        // [B][k][P]
    const double* sigmas;                      // [B][k]
    const double* trans;                       // [B][k][k]
    const double* obs;                         // the observes, packed problem after problem, step after step, (y, x[0..P)) a step
    double* tab;                               // [B][T_max][kBatchTab]
    uint64_t* thr;                             // [B][64]
    int32_t* status;                           // [B]: 0, or the bits of reg_check
    double* coef_out;                          // [B][8][16]: the coefficients in force (slots outside the table 0.0)
    double* sigma_out;                         // [B][8]: the sigmas in force (states >= k 0.0)
    double* log_norm_out;                      // [B][8]: their log_norms (states >= k 0.0)
    int T_max, k, P;
};

__global__ __launch_bounds__(kThreads) void batch_retable_reg_kernel(BatchRetableRegArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_trans[64];                              // the problem's transition rows, [k][k]
    __shared__ double s_coef[kRegCoefSlots];                    // transposed: entry (s, i) at 8 i + s
    __shared__ double s_sigma[8], s_log_norm[8];
    __shared__ double s_z[kRetableRows * kFullTileStride];      // a tile's observes: row r, coordinate d at 17 r + d
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, k = a.k, P = a.P, D = 1 + a.P;
    const int s0 = (tid >> 4) & 7, i0 = tid & 15;
    const bool owner = tid < kRegCoefSlots, in = owner && s0 < k && i0 < P;
    int bits = 0;
    if (tid < k * k) {
        const double w = a.trans[(int64_t)b * k * k + tid];
        s_trans[tid] = w;
        if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
    }
    const double c = in ? a.coef[((int64_t)b * k + s0) * P + i0] : 0.0;
    if (in && !(fabs(c) < INFINITY)) bits |= kRetableBadMean;
    const double sg = tid < k ? a.sigmas[(int64_t)b * k + tid] : 1.0;
    if (tid < k && scale_bad(sg)) bits |= kRetableBadScale;
    __syncthreads();
    if (tid < k) {
        double tot = 0.0;
        for (int j = 0; j < k; ++j) tot += s_trans[tid * k + j];
        if (!(tot > 0.0)) bits |= kRetableNoMass;
    }
    // (__syncthreads_or joins a predicate, not a word: one call a bit; uniform from here on)
    bits = (__syncthreads_or(bits & kRetableBadWeight) ? kRetableBadWeight : 0) | (__syncthreads_or(bits & kRetableNoMass) ? kRetableNoMass : 0) |
           (__syncthreads_or(bits & kRetableBadMean) ? kRetableBadMean : 0) | (__syncthreads_or(bits & kRetableBadScale) ? kRetableBadScale : 0);
    if (blockIdx.y == 0 && tid == 0) a.status[b] = bits;
    if (bits) return;
    if (owner) s_coef[8 * i0 + s0] = c;
    if (tid < 8) { s_sigma[tid] = tid < k ? sg : 0.0; s_log_norm[tid] = tid < k ? scale_log_norm(sg) : 0.0; }
    __syncthreads();
    if (blockIdx.y == 0) {
        if (owner) a.coef_out[(int64_t)b * kRegCoefSlots + tid] = c;        // (tid = 16 s + i)
        if (tid < 8) { a.sigma_out[(int64_t)b * 8 + tid] = s_sigma[tid]; a.log_norm_out[(int64_t)b * 8 + tid] = s_log_norm[tid]; }
        if (tid < 64) a.thr[(int64_t)b * 64 + tid] = retable_threshold(s_trans, k, tid >> 3, tid & 7);
    }
    const int s = tid & 7, r = tid >> 3;
    const int64_t T = a.prob[b].T, stride = (int64_t)gridDim.y * kRetableRows;
    const double* z = a.obs + a.first[b] * D;
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    const double sigma = s_sigma[s], log_norm = s_log_norm[s];
    // (t0, T and stride are the workgroup's: every thread takes every trip and reaches both barriers)
    for (int64_t t0 = (int64_t)blockIdx.y * kRetableRows; t0 < T; t0 += stride) {
        const int n_rows = (int)(T - t0 < kRetableRows ? T - t0 : kRetableRows), n = n_rows * D;
        const double* src = z + t0 * D;
        for (int e = tid; e < n; e += kThreads) s_z[(e / D) * kFullTileStride + e % D] = src[e];
        __syncthreads();
        if (r < n_rows) rows[(t0 + r) * kBatchTab + s] = s < k ? reg_entry(s_z + r * kFullTileStride, P, s_coef + s, 8, sigma, log_norm) : -INFINITY;
        __syncthreads();                                        // (the next trip's load overwrites the tile)
    }
}

struct BatchMstepRegArgs {
    const double* stats;                       // [B][kFullStats]
    double* coef;                              // [B][k][P]
    double* sigmas;                            // [B][k]
    double* log_norms;                         // [B][k], or null
    double* trans;                             // [B][k][k]
    double floor;
    int64_t B;
    int k, P;
};

// a 16-lane group a (problem, state), lane i row i of the state's system; half a workgroup a problem
__global__ __launch_bounds__(kThreads) void batch_mstep_reg_kernel(BatchMstepRegArgs a)
{
#pragma clang fp contract(off)
    const int tid = (int)threadIdx.x, k = a.k, P = a.P;
    const int half = tid >> 7, s0 = (tid >> 4) & 7, i0 = tid & 15;
    const bool state = s0 < k, live = state && i0 < P;
    const double ff = a.floor * a.floor;
    for (int64_t b = (int64_t)blockIdx.x * 2 + half; b < a.B; b += (int64_t)gridDim.x * 2) {       // (wavefront-uniform)
        const double* rec = a.stats + b * kFullStats;
        if (state) {
            double row = 0.0;
            for (int j = 0; j < k; ++j) row = row + rec[8 * s0 + j];
            if (row > 0.0 && i0 < k) a.trans[(b * k + s0) * k + i0] = rec[8 * s0 + i0] / row;
        }
        const double occ = state ? rec[64 + s0] : 0.0;
        const double* syy = rec + kFullSyy + kFullTri * (state ? s0 : 0);
        const double c0 = state ? syy[0] : 0.0, bi = live ? syy[full_tri(1 + i0, 0)] : 0.0;
        bool bad = !(fabs(c0) < INFINITY) || !(fabs(bi) < INFINITY);      // this lane's: an entry or a coefficient that is not finite
        bool keep = !(occ > 0.0) || !(occ < INFINITY);                   // the group's: every lane of a state holds the same
        double W[kRegMaxCov], L[kRegMaxCov], dj = 1.0;
#pragma unroll
        for (int j = 0; j < kRegMaxCov; ++j) { W[j] = 0.0; L[j] = 0.0; }
#pragma unroll
        for (int j = 0; j < kRegMaxCov; ++j)
            if (j < P) {                                        // (uniform)
                const bool mine = live && i0 >= j;
                double av = mine ? syy[full_tri(1 + i0, 1 + j)] : 0.0;
                if (!(fabs(av) < INFINITY)) bad = true;
#pragma unroll
                for (int p = 0; p < j; ++p) av = av - dmul_rn(W[p], __shfl(L[p], j, kFullMaxDim));
                const double d = __shfl(av, j, kFullMaxDim);    // the pivot, lane j's
                if (!(d > 0.0) || !(d < INFINITY)) keep = true;
                if (i0 == j) dj = d;
                if (i0 > j) { W[j] = mine ? av : 0.0; L[j] = mine ? av / d : 0.0; }
            }
        double u = bi;
#pragma unroll
        for (int p = 0; p < kRegMaxCov - 1; ++p)
            if (p + 1 < P) {
                const double up = __shfl(u, p, kFullMaxDim);
                if (i0 > p) u = u - dmul_rn(L[p], up);
            }
        double beta = live ? u / dj : 0.0;
#pragma unroll
        for (int p = kRegMaxCov - 1; p >= 1; --p)
            if (p < P) {
                const double bp = __shfl(beta, p, kFullMaxDim);
#pragma unroll
                for (int i = 0; i < p; ++i) {
                    const double l = __shfl(L[i], p, kFullMaxDim);      // L[p][i], lane p's
                    if (i0 == i) beta = beta - dmul_rn(l, bp);
                }
            }
        if (!(fabs(beta) < INFINITY)) bad = true;
        if (((__ballot(bad) >> (lane_id() & 48)) & 0xffffull) != 0) keep = true;
        const double term = live ? dmul_rn(beta, bi / occ) : 0.0;
        double v = c0 / occ;
#pragma unroll
        for (int i = 0; i < kRegMaxCov; ++i)
            if (i < P) v = v - __shfl(term, i, kFullMaxDim);
        if (state && !keep) {
            if (i0 < P) a.coef[(b * k + s0) * P + i0] = beta;
            if (i0 == 0) {
                const double sg = v >= ff ? sqrt(v) : a.floor;
                a.sigmas[b * k + s0] = sg;
                if (a.log_norms) a.log_norms[b * k + s0] = scale_bad(sg) ? NAN : scale_log_norm(sg);
            }
        }
    }
}

}  // namespace cph
