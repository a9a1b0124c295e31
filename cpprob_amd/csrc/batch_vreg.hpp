// Markov-switching vector regressions (MS-VAR) of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables: state s of problem b emits
// the vector y_t in R^Q, y_t ~ N(B_s x_t, Sigma_s), on P covariates x_t known at the step, 1 <= Q, 1 <= P, Q + P <= kFullMaxDim (so
// Q P <= 64) (cpprob_hip_batch_begin_problems_vreg, _retable_vreg*, _vreg_stats*, _mstep_vreg_device).  The tables are coef [k][Q][P],
// cov [k][Q][Q] (only the lower triangle is read) and trans [k][k].  A step's observe is the Q + P doubles z_t = (y_t, x_t): the
// responses first.  An intercept is a covariate column of ones; none is added here.  Hamilton's Markov-switching VAR is the case
// x_t = (1, y_{t-1}, .., y_{t-p}).  As for every family, only what WRITES rows and tables, and what solves the M-step, is stated here:
//   rows            vreg_entry: pred_q = 0.0, then ascending over i pred_q = pred_q + dmul_rn(coef[s][q][i], x_i); the entry is
//                   full_entry(y, Q, pred, 1, L_s, ls, log_norm_s), the full family's forward substitution with the prediction where
//                   the mean stood; L_s = full_factor(cov[s]) at dimension Q and log_norm_s = full_log_norm; -inf where any |y_q| or
//                   |x_i| is infinite, and for s >= k
//   check           vreg_check: retable_check's two bits on the transition rows, kRetableBadMean for a coefficient that is not finite,
//                   kRetableBadCov for a covariance full_factor refuses.  No new status bit
//   record          the full family's kFullStats (1304) doubles at D = Q + P, as batch_full_walk_kernel and batch_full_moments_kernel
//                   leave them: with syy the packed triangle of sum over t of g_t[s] z_t z_t^T, A_ij = syy[Q+i][Q+j], j <= i,
//                   b_{q,i} = syy[Q+i][q] and C_qr = syy[q][r], r <= q
//   M-step          vreg_mstep: the transition row as retable_mstep forms it.  For a state with occ > 0, A = L D L^T exactly as
//                   reg_mstep factors it (W = L D kept, L[i][j] = a / d_j a real division).  For every q the forward solve, the
//                   division by the pivots and the back solve by columns from the last run on b_{q,.}: reg_mstep's operations in its
//                   order (the back solve's subtractions of an entry DESCEND over p); the L entries used do not depend on q.  The
//                   candidate covariance: for r <= q, c_qr = C_qr / occ, then ascending over i
//                   c_qr = c_qr - dmul_rn(beta_{q,i}, b_{r,i} / occ); a diagonal entry c >= floor floor ? c : floor floor (a NaN takes
//                   the floor too); the candidate goes through full_factor.  The state keeps coefficients and covariance, as a state
//                   without mass does, where occ is not > 0 or not finite, an entry read is not finite, a pivot of A has !(d > 0) or
//                   is infinite, a solved coefficient is not finite, or the candidate does not factor.  Otherwise coef and both
//                   triangles of cov are written: a re-table never refuses an M-step's output
// Anchors (tests/test_batch_vreg_host.py and tests/test_gpu_batch_vreg.py rest on them):
//   Q = 1           rows, log_norm, threshold words and coefficients are the regression family's bits (csrc/batch_reg.hpp) with
//                   cov = sigma sigma, for sigmas with sqrt(fl(sigma sigma)) == sigma; the fitted cov is the regression's v where
//                   v >= floor floor
//   P = 1, x = 1.0  pred = coef, A_00 is occ's bits and the pivot is occ, beta_q = sy_q / occ, and
//                   c_qr = syy_qr / occ - dmul_rn(mean_q, mean_r): the full family's rows, M-step and candidate, bit for bit
// Every function of this file runs with fp contract off.  tests/vreg_ref.py restates all of it.
//
// batch_retable_vreg_kernel: the re-table grid (blockIdx.x the problem, blockIdx.y strides over tiles of kRetableRows steps, eight lanes
// a row, lane s the state).  Prologue: thread (s, i), s = tid >> 4 and i = tid & 15 (the first two wavefronts), holds row i of state s's
// Q x Q covariance in registers and factors it column by column, the pivot row travelling by __shfl inside the 16-lane group: the form
// of batch_retable_full_kernel's prologue, no workgroup barrier a column.  Every thread checks the two coefficient slots tid and
// tid + 256 of the problem's [8][64] and stages them TRANSPOSED in LDS, entry (s, q, i) at 8 (q P + i) + s (4096 B): the eight lanes of
// a row read 64 consecutive bytes an index.  L is staged transposed at 8 idx + s; the observes go through the stride-17 tile.  A row
// thread runs vreg_entry: the covariates and its Q predictions in registers, then the forward substitution on them, both loops
// unrolled under the uniform (Q, P) so that nothing is indexed at run time.  __syncthreads_or joins one status bit at a time; a problem
// with a bit set keeps rows, words and tables and leaves after the joins.  Workgroup y = 0 alone stores the status, the 64 threshold
// words and the tables in force: coef [B][8][64] with (q, i) at q P + i, packed L [B][8][136], log_norm [B][8]; slots outside the table
// 0.0.  No atomics; no result depends on gridDim.y.
// batch_mstep_vreg_kernel: a 16-lane group a (problem, state), 128 threads a problem, a 256-thread workgroup two problems, at most
// kRegMstepGridMax workgroups, the rest strided by PAIRS of problems so that the trip count is the workgroup's (the kernel has two
// barriers a trip; an odd batch's last half-workgroup works on zeros and stores nothing).  Lane i holds row i of A, of W and of L and
// its entries b_{q,i} of all Q right-hand sides in registers.  The factorisation's shuffles are batch_mstep_reg_kernel's.  In the forward
// solve a lane's own L[i][p] meets the Q shuffled u_{q,p}; in the back solve the column entry L[p][i] is fetched ONCE by its shuffles
// and applied to all Q right-hand sides: 105 + 14 Q shuffles where Q calls of the old kernel would take 119 Q.  Lane i leaves
// beta_{q,i} and b_{q,i} / occ in a per-state LDS slab (2 x 64 doubles a state, 16 KiB a workgroup); after a barrier lane q forms row q
// of the candidate from the slab, ascending over i -- the serial statement's bits --, and the rows are factored by the re-table's
// shuffle Cholesky at dimension Q, whose broadcast pivot tells every lane of a failure (scale_bad(sqrt(a)) holds for every a with
// !(a > 0), and a candidate entry that is not finite reaches a pivot as NaN or -inf: full_factor's refusals).  One __ballot a group
// carries "something was not finite".  The loops are fully unrolled under the uniform (Q, P); rows outside work on zeros.
// The E-step is batch_full_walk_kernel and batch_full_moments_kernel as they are, at D = Q + P.
// Resources (gfx950, tools/kernel_resources.py; profiles/r45_notes.md): batch_retable_vreg_kernel 101 VGPRs, 19008 B LDS, scratch 0;
// batch_mstep_vreg_kernel 228 VGPRs, 16384 B LDS, scratch 0, nothing spilled.
#pragma once
#include "batch_reg.hpp"

namespace cph {

constexpr int kVregMaxResp = kFullMaxDim - 1;                   // Q at most (P = 1); P at most is kRegMaxCov (Q = 1)
constexpr int kVregCoefs = 64;                                  // Q P at most under Q + P <= 16: (q, i) slots of a state, (q, i) at q P + i
constexpr int kVregCoefSlots = 8 * kVregCoefs;                  // (s, q, i) slots of a problem's coefficients, [8][64]
static_assert(kVregCoefSlots == 2 * kThreads, "a thread of the re-table owns two coefficient slots");
static_assert((kFullMaxDim / 2) * (kFullMaxDim / 2) == kVregCoefs, "Q P is largest at Q = P = 8");

// log N(y; B x, L L^T) up to log_norm: z the step's Q + P doubles (y, x); coef the state's coefficient (0, 0), cs doubles between two
// coefficients and L the state's packed entry 0, ls doubles between two entries (8 in the kernel's transposed staging, 1 in a packed
// array).  Fully unrolled under the uniform (Q, P): x and pred stay in registers on the device.
__host__ __device__ inline double vreg_entry(const double* z, int Q, int P, const double* coef, int cs, const double* L, int ls, double log_norm)
{
#pragma clang fp contract(off)
    double x[kRegMaxCov], pred[kFullMaxDim];
    bool inf = false;
#pragma unroll
    for (int i = 0; i < kRegMaxCov; ++i) {
        x[i] = 0.0;
        if (i < P) {
            x[i] = z[Q + i];
            if (fabs(x[i]) == INFINITY) inf = true;
        }
    }
    pred[kVregMaxResp] = 0.0;
#pragma unroll
    for (int q = 0; q < kVregMaxResp; ++q) {
        double a = 0.0;
        if (q < Q) {
#pragma unroll
            for (int i = 0; i < kRegMaxCov; ++i)
                if (i < P) a = a + dmul_rn(coef[(q * P + i) * cs], x[i]);
        }
        pred[q] = a;
    }
    if (inf) return -INFINITY;
    return full_entry(z, Q, pred, 1, L, ls, log_norm);
}

// the bits of one problem's table (coef [k][Q][P], covs [k][Q][Q], trans [k][k]), serially: the host's validation
inline int vreg_check(const double* coef, const double* covs, const double* trans, int k, int Q, int P)
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
        for (int e = 0; e < Q * P; ++e) if (!(fabs(coef[s * Q * P + e]) < INFINITY)) bits |= kRetableBadMean;
        for (int i = 0; i < Q; ++i) for (int j = 0; j <= i; ++j) c[full_tri(i, j)] = covs[((size_t)s * Q + i) * Q + j];
        if (!full_factor(c, 1, Q, c, 1)) bits |= kRetableBadCov;
    }
    return bits;
}

// state s of one problem's M-step: rec its record [kFullStats]; coef [k][Q][P], covs [k][Q][Q] and trans [k][k] updated in place.
// Serial: the statement the device's 16-lane form is held to.
inline void vreg_mstep(const double* rec, int k, int Q, int P, int s, double* coef, double* covs, double* trans, double floor)
{
#pragma clang fp contract(off)
    double row = 0.0;
    for (int j = 0; j < k; ++j) row = row + rec[8 * s + j];
    if (row > 0.0) for (int j = 0; j < k; ++j) trans[s * k + j] = rec[8 * s + j] / row;
    const double occ = rec[64 + s];
    if (!(occ > 0.0) || !(occ < INFINITY)) return;
    const double* syy = rec + kFullSyy + kFullTri * s;
    for (int i = 0; i < Q + P; ++i) for (int j = 0; j <= i; ++j) if (!(fabs(syy[full_tri(i, j)]) < INFINITY)) return;
    double W[kFullTri], L[kFullTri], d[kRegMaxCov], beta[kVregCoefs], cand[kFullTri];
    for (int j = 0; j < P; ++j)
        for (int i = j; i < P; ++i) {
            double a = syy[full_tri(Q + i, Q + j)];
            for (int p = 0; p < j; ++p) a = a - dmul_rn(W[full_tri(i, p)], L[full_tri(j, p)]);
            if (i == j) {
                if (!(a > 0.0) || !(a < INFINITY)) return;      // (the state keeps its coefficients and covariance)
                d[j] = a;
            } else { W[full_tri(i, j)] = a; L[full_tri(i, j)] = a / d[j]; }
        }
    for (int q = 0; q < Q; ++q) {
        double* bq = beta + q * P;
        for (int i = 0; i < P; ++i) {
            double u = syy[full_tri(Q + i, q)];
            for (int p = 0; p < i; ++p) u = u - dmul_rn(L[full_tri(i, p)], bq[p]);
            bq[i] = u;
        }
        for (int i = 0; i < P; ++i) bq[i] = bq[i] / d[i];
        for (int p = P - 1; p >= 1; --p)
            for (int i = 0; i < p; ++i) bq[i] = bq[i] - dmul_rn(L[full_tri(p, i)], bq[p]);
        for (int i = 0; i < P; ++i) if (!(fabs(bq[i]) < INFINITY)) return;
    }
    const double ff = floor * floor;
    for (int q = 0; q < Q; ++q)
        for (int r = 0; r <= q; ++r) {
            double c = syy[full_tri(q, r)] / occ;
            for (int i = 0; i < P; ++i) c = c - dmul_rn(beta[q * P + i], syy[full_tri(Q + i, r)] / occ);
            if (q == r) c = c >= ff ? c : ff;
            cand[full_tri(q, r)] = c;
        }
    if (!full_factor(cand, 1, Q, W, 1)) return;                 // (W is free: the factor is not kept)
    for (int e = 0; e < Q * P; ++e) coef[s * Q * P + e] = beta[e];
    for (int q = 0; q < Q; ++q)
        for (int r = 0; r <= q; ++r) {
            covs[((size_t)s * Q + q) * Q + r] = cand[full_tri(q, r)];
            covs[((size_t)s * Q + r) * Q + q] = cand[full_tri(q, r)];
        }
}

struct BatchRetableVregArgs {
    const BatchProblem* prob;                  // [B]: T_b
    const int64_t* first;                      // [B]: problem b's first step in obs (the lengths before it; Q + P doubles a step)
    const double* coef;                        // [B][k][Q][P]
    const double* covs;                        // [B][k][Q][Q], the lower triangle read
    const double* trans;                       // [B][k][k]
    const double* obs;                         // the observes, packed problem after problem, step after step, (y[0..Q), x[0..P)) a step
    double* tab;                               // [B][T_max][kBatchTab]
    uint64_t* thr;                             // [B][64]
    int32_t* status;                           // [B]: 0, or the bits of vreg_check
    double* coef_out;                          // [B][8][64]: the coefficients in force, (q, i) at q P + i (slots outside the table 0.0)
    double* L_out;                             // [B][8][136]: the packed factors in force (slots outside the table 0.0)
    double* log_norm_out;                      // [B][8]: the states' log_norms (states >= k 0.0)
    int T_max, k, Q, P;
};

__global__ __launch_bounds__(kThreads) void batch_retable_vreg_kernel(BatchRetableVregArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_trans[64];                              // the problem's transition rows, [k][k]
    __shared__ double s_L[kFullTriSlots];                       // transposed: entry (s, idx) at 8 idx + s
    __shared__ double s_coef[kVregCoefSlots];                   // transposed: entry (s, q, i) at 8 (q P + i) + s
    __shared__ double s_ln[kFullMeanSlots];                     // transposed: the pivots' logarithms, entry (s, d) at 8 d + s
    __shared__ double s_log_norm[8];
    __shared__ double s_z[kRetableRows * kFullTileStride];      // a tile's observes: row r, coordinate d at 17 r + d
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, k = a.k, Q = a.Q, P = a.P, D = a.Q + a.P, QP = a.Q * a.P;
    const int s0 = (tid >> 4) & 7, i0 = tid & 15;
    const bool owner = tid < kFullMeanSlots, in = owner && s0 < k && i0 < Q;
    int bits = 0;
    if (tid < k * k) {
        const double w = a.trans[(int64_t)b * k * k + tid];
        s_trans[tid] = w;
        if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
    }
    // the coefficient slots tid and tid + 256 of [8][64]: states tid >> 6 and 4 + (tid >> 6), entry tid & 63
    const int cs0 = tid >> 6, ce = tid & (kVregCoefs - 1);
    const bool cin0 = cs0 < k && ce < QP, cin1 = cs0 + 4 < k && ce < QP;
    const double c0 = cin0 ? a.coef[((int64_t)b * k + cs0) * QP + ce] : 0.0, c1 = cin1 ? a.coef[((int64_t)b * k + cs0 + 4) * QP + ce] : 0.0;
    if (!(fabs(c0) < INFINITY) || !(fabs(c1) < INFINITY)) bits |= kRetableBadMean;
    double Lrow[kFullMaxDim], piv = 0.0;                        // (column 15 stays 0.0: Q <= 15)
#pragma unroll
    for (int j = 0; j < kFullMaxDim; ++j) Lrow[j] = 0.0;
    if (owner) {                                                // (wavefront-uniform: the first two wavefronts, every lane of them)
        const double* cov = a.covs + (((int64_t)b * k + (in ? s0 : 0)) * Q + (in ? i0 : 0)) * Q;   // (row i0 of state s0; in bounds for every lane)
#pragma unroll
        for (int j = 0; j < kVregMaxResp; ++j)
            if (j < Q) {                                        // (uniform)
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
    s_coef[8 * ce + cs0] = c0;
    s_coef[8 * ce + cs0 + 4] = c1;
    if (owner) {
        s_ln[8 * i0 + s0] = in ? scale_log_norm(piv) : 0.0;
#pragma unroll
        for (int j = 0; j < kFullMaxDim; ++j)
            if (j <= i0) s_L[8 * (i0 * (i0 + 1) / 2 + j) + s0] = in && j < Q ? Lrow[j] : 0.0;
    }
    __syncthreads();
    if (tid < 8) s_log_norm[tid] = tid < k ? diag_log_norm(s_ln + tid, Q, 8) : 0.0;
    __syncthreads();
    if (blockIdx.y == 0) {
        a.coef_out[(int64_t)b * kVregCoefSlots + tid] = c0;     // (slot tid = 64 s + (q P + i))
        a.coef_out[(int64_t)b * kVregCoefSlots + kThreads + tid] = c1;
        for (int e = tid; e < kFullTriSlots; e += kThreads) a.L_out[(int64_t)b * kFullTriSlots + e] = s_L[8 * (e % kFullTri) + e / kFullTri];
        if (tid < 8) a.log_norm_out[(int64_t)b * 8 + tid] = s_log_norm[tid];
        if (tid < 64) a.thr[(int64_t)b * 64 + tid] = retable_threshold(s_trans, k, tid >> 3, tid & 7);
    }
    const int s = tid & 7, r = tid >> 3;
    const int64_t T = a.prob[b].T, stride = (int64_t)gridDim.y * kRetableRows;
    const double* z = a.obs + a.first[b] * D;
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    const double log_norm = s_log_norm[s];
    // (t0, T and stride are the workgroup's: every thread takes every trip and reaches both barriers)
    for (int64_t t0 = (int64_t)blockIdx.y * kRetableRows; t0 < T; t0 += stride) {
        const int n_rows = (int)(T - t0 < kRetableRows ? T - t0 : kRetableRows), n = n_rows * D;
        const double* src = z + t0 * D;
        for (int e = tid; e < n; e += kThreads) s_z[(e / D) * kFullTileStride + e % D] = src[e];
        __syncthreads();
        if (r < n_rows) rows[(t0 + r) * kBatchTab + s] = s < k ? vreg_entry(s_z + r * kFullTileStride, Q, P, s_coef + s, 8, s_L + s, 8, log_norm) : -INFINITY;
        __syncthreads();                                        // (the next trip's load overwrites the tile)
    }
}

struct BatchMstepVregArgs {
    const double* stats;                       // [B][kFullStats]
    double* coef;                              // [B][k][Q][P]
    double* covs;                              // [B][k][Q][Q]
    double* trans;                             // [B][k][k]
    double floor;
    int64_t B;
    int k, Q, P;
};

// a 16-lane group a (problem, state), lane i row i of the state's system and, after the solves, row i of its candidate covariance
__global__ __launch_bounds__(kThreads) void batch_mstep_vreg_kernel(BatchMstepVregArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_beta[2 * kVregCoefSlots];               // a slab a group: beta_{q,i} at q P + i
    __shared__ double s_bocc[2 * kVregCoefSlots];               // ... and b_{q,i} / occ
    const int tid = (int)threadIdx.x, k = a.k, Q = a.Q, P = a.P, QP = a.Q * a.P;
    const int half = tid >> 7, s0 = (tid >> 4) & 7, i0 = tid & 15;
    double* sb = s_beta + kVregCoefs * (tid >> 4);
    double* so = s_bocc + kVregCoefs * (tid >> 4);
    const double ff = a.floor * a.floor;
    for (int64_t pb = (int64_t)blockIdx.x; pb * 2 < a.B; pb += (int64_t)gridDim.x) {       // (the workgroup's: every thread reaches both barriers)
        const int64_t b = pb * 2 + half;
        const bool state = s0 < k && b < a.B, live = state && i0 < P, liveq = state && i0 < Q;
        const double* rec = a.stats + (state ? b : 0) * kFullStats;
        if (state) {
            double row = 0.0;
            for (int j = 0; j < k; ++j) row = row + rec[8 * s0 + j];
            if (row > 0.0 && i0 < k) a.trans[(b * k + s0) * k + i0] = rec[8 * s0 + i0] / row;
        }
        const double occ = state ? rec[64 + s0] : 0.0;
        const double* syy = rec + kFullSyy + kFullTri * (state ? s0 : 0);
        bool bad = false;                                                // this lane's: an entry or a coefficient that is not finite
        bool keep = !(occ > 0.0) || !(occ < INFINITY);                   // the group's: every lane of a state holds the same
        // lane i's b_{q,i} (then u, then beta) of every right-hand side, and row i of C (then of the candidate)
        double u[kVregMaxResp], c[kVregMaxResp];
#pragma unroll
        for (int q = 0; q < kVregMaxResp; ++q) {
            u[q] = live && q < Q ? syy[full_tri(Q + i0, q)] : 0.0;
            c[q] = liveq && q <= i0 ? syy[full_tri(i0, q)] : 0.0;
            if (!(fabs(u[q]) < INFINITY) || !(fabs(c[q]) < INFINITY)) bad = true;
            if (live && q < Q) so[q * P + i0] = u[q] / occ;
        }
        double W[kRegMaxCov], L[kRegMaxCov], dj = 1.0;
#pragma unroll
        for (int j = 0; j < kRegMaxCov; ++j) { W[j] = 0.0; L[j] = 0.0; }
#pragma unroll
        for (int j = 0; j < kRegMaxCov; ++j)
            if (j < P) {                                        // (uniform)
                const bool mine = live && i0 >= j;
                double av = mine ? syy[full_tri(Q + i0, Q + j)] : 0.0;
                if (!(fabs(av) < INFINITY)) bad = true;
#pragma unroll
                for (int p = 0; p < j; ++p) av = av - dmul_rn(W[p], __shfl(L[p], j, kFullMaxDim));
                const double d = __shfl(av, j, kFullMaxDim);    // the pivot, lane j's
                if (!(d > 0.0) || !(d < INFINITY)) keep = true;
                if (i0 == j) dj = d;
                if (i0 > j) { W[j] = mine ? av : 0.0; L[j] = mine ? av / d : 0.0; }
            }
        // forward: the lane's own L[i][p] on the Q shuffled u_{q,p}
#pragma unroll
        for (int p = 0; p < kRegMaxCov - 1; ++p)
            if (p + 1 < P) {
#pragma unroll
                for (int q = 0; q < kVregMaxResp; ++q)
                    if (q < Q) {
                        const double up = __shfl(u[q], p, kFullMaxDim);
                        if (i0 > p) u[q] = u[q] - dmul_rn(L[p], up);
                    }
            }
#pragma unroll
        for (int q = 0; q < kVregMaxResp; ++q) u[q] = live && q < Q ? u[q] / dj : 0.0;
        // back, by columns from the last: L[p][i], lane p's, fetched once for all Q right-hand sides
#pragma unroll
        for (int p = kRegMaxCov - 1; p >= 1; --p)
            if (p < P) {
                double lp = 0.0;
#pragma unroll
                for (int i = 0; i < p; ++i) {
                    const double l = __shfl(L[i], p, kFullMaxDim);
                    if (i0 == i) lp = l;
                }
#pragma unroll
                for (int q = 0; q < kVregMaxResp; ++q)
                    if (q < Q) {
                        const double bp = __shfl(u[q], p, kFullMaxDim);
                        if (i0 < p) u[q] = u[q] - dmul_rn(lp, bp);
                    }
            }
#pragma unroll
        for (int q = 0; q < kVregMaxResp; ++q) {
            if (!(fabs(u[q]) < INFINITY)) bad = true;
            if (live && q < Q) sb[q * P + i0] = u[q];
        }
        if (((__ballot(bad) >> (lane_id() & 48)) & 0xffffull) != 0) keep = true;
        __syncthreads();
        // row i0 of the candidate from the slab, ascending over i (lanes outside Q read slab row 0 and keep zeros)
        const int qa = liveq ? i0 * P : 0;
#pragma unroll
        for (int r = 0; r < kVregMaxResp; ++r)
            if (r < Q) {                                        // (uniform)
                double v = c[r] / occ;
                for (int i = 0; i < P; ++i) v = v - dmul_rn(sb[qa + i], so[r * P + i]);
                if (i0 == r) v = v >= ff ? v : ff;
                c[r] = liveq && r <= i0 ? v : 0.0;
            }
        // the re-table's shuffle Cholesky at dimension Q on the rows c; the broadcast pivot is every lane's
        double F[kVregMaxResp];
#pragma unroll
        for (int j = 0; j < kVregMaxResp; ++j) F[j] = 0.0;
#pragma unroll
        for (int j = 0; j < kVregMaxResp; ++j)
            if (j < Q) {                                        // (uniform)
                const bool mine = liveq && i0 >= j;
                double av = mine ? c[j] : 0.0;
#pragma unroll
                for (int p = 0; p < j; ++p) av = av - dmul_rn(F[p], __shfl(F[p], j, kFullMaxDim));
                if (i0 == j) F[j] = sqrt(av);
                const double d = __shfl(F[j], j, kFullMaxDim);
                if (scale_bad(d)) keep = true;
                if (i0 > j) F[j] = mine ? av / d : 0.0;
            }
        if (state && !keep) {
            const int64_t at = b * k + s0;
#pragma unroll
            for (int q = 0; q < kVregMaxResp; ++q) {
                if (q < Q && i0 < P) a.coef[at * QP + q * P + i0] = u[q];
                if (i0 < Q && q <= i0) { a.covs[(at * Q + i0) * Q + q] = c[q]; a.covs[(at * Q + q) * Q + i0] = c[q]; }
            }
        }
        __syncthreads();                                        // (the next trip's solves overwrite the slab)
    }
}

}  // namespace cph
