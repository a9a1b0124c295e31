// Diagonal-Gaussian vector emissions of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables: state s of problem b emits a vector
// y in R^D, 1 <= D <= kDiagMaxDim, with independent coordinates y_d ~ N(mean[b][s][d], sigma[b][s][d])
// (cpprob_hip_batch_begin_problems_diag, _retable_diag*, _diag_stats*, _mstep_diag_device).  The step kernel and every pass behind it read
// the emission through the rows tab[t][8] alone, so only what WRITES rows and tables, and the statistic the M-step needs, is stated here:
//   log_norm        log_norm[s] = ((0.0 + scale_log_norm(sigma[s][0])) + scale_log_norm(sigma[s][1])) + ..., ascending over d
//   rows            diag_entry: r_d = (y_d - mean[s][d]) / sigma[s][d], a real division as in scale_entry; q = ((0.0 + r_0 r_0) + r_1 r_1)
//                   + ..., ascending over d; ll[s] = (q + log_norm[s]) (-0.5); -inf where any |y_d| is infinite, and for s >= k.  At D = 1
//                   these are scale_entry's bits
//   check           retable_check's two bits on the transition rows, kRetableBadMean for a mean that is not finite, kRetableBadScale for a
//                   sigma with scale_bad(sigma).  Nothing is normalised
//   record          kSymbolStats (600) doubles a problem: the 88 of batch_smooth_stats_kernel with coordinate 0 as the observe, then
//                   sy[s][d] = sum over t of g_t[s] y_t[d] at 88 + 64 s + d and syy[s][d] = sum over t of g_t[s] (y_t[d] y_t[d]) at
//                   88 + 64 s + 32 + d, each one addition a step from 0.0 in the walk's order t = T-1 .. 0, every product one dmul_rn;
//                   slots with d >= D or s >= k are 0.0.  At D = 1 sy and syy are occ_y and occ_yy
//   M-step          the transition row as retable_mstep forms it; for a state with occ > 0 and every d < D: mean' = sy / occ,
//                   sigma' = scale_sigma(occ, syy, mean', floor); a state without mass keeps its tables.  At D = 1: scale_mstep's bits
// Every function of this file runs with fp contract off.  tests/diag_ref.py restates all of it.
//
// batch_retable_diag_kernel: the re-table grid (blockIdx.x the problem, blockIdx.y strides over tiles of kRetableRows steps, eight lanes
// a row, lane s the state, a wavefront stores 512 consecutive bytes).  Thread i takes slot i of the 256 (s = i >> 5, d = i & 31: the
// loads of a state are consecutive, and so are the stores of the tables in force), tests its own mean and sigma, takes its one
// scale_log_norm and stages all three TRANSPOSED, (s, d) at 8 d + s, so the eight lanes of a row read 64 consecutive bytes of LDS for
// each d.  Eight threads add the logarithms ascending over d after a barrier.  __syncthreads_or joins one status bit at a time; a
// problem with a bit set keeps rows, words and tables and leaves after the joins, before any barrier only some threads would reach.
// The observes of a tile, kRetableRows x D doubles contiguous in global memory, are loaded coalesced by all 256 threads into an LDS
// tile whose row stride, kDiagTileStride = 33 doubles, puts the eight rows of a wavefront on eight different bank pairs (a stride of
// 32 would put them on one); the lanes of a row read the same address.  A workgroup that walks a second tile reuses the buffer: a
// barrier stands between the last read of a tile and the next tile's load.  The trip count is the workgroup's alone (T_b, blockIdx.y,
// gridDim.y), so every thread reaches every barrier.  Workgroup y = 0 alone stores the status word, the 64 threshold words and the
// means, sigmas and log_norms in force ([B][8][32], [B][8][32], [B][8]; slots outside the table 0.0).  No atomics; no result depends on
// gridDim.y.
// batch_diag_stats_kernel: batch_symbol_stats_kernel's walk, statement for statement -- one wavefront a problem, kWaves problems a
// workgroup, at most kSymbolGridMax workgroups and the remaining problems strided -- with lane (d', s) keeping sy[s][8 i + d'] and
// syy[s][8 i + d'], i = 0..3, in eight registers in place of cnt.  The lane's at most four coordinates of y_t are loaded with the
// prefetch of the next row, off the serial chain: the eight lanes (d', .) read one address, a wavefront 256 consecutive bytes; the
// number of live i is wavefront-uniform, (D + 7) / 8, and a coordinate >= D is never loaded.  g_t[s] stands alike on the lanes (., s)
// after smooth_marginal_sum, so lane (0, s)'s sy[0] repeats occ_y's additions.  No LDS, no barrier, no atomics.
// batch_mstep_diag_kernel: one thread a (problem, state s < k, coordinate d < D); the thread with d = 0 also writes the transition row.
#pragma once
#include "batch_categorical.hpp"

namespace cph {

constexpr int kDiagMaxDim = 32;                     // D at most: a lane's four accumulators of eight coordinates, twice
constexpr int kDiagSlots = 8 * kDiagMaxDim;         // (s, d) slots of a problem's means, and of its sigmas
constexpr int kDiagTileStride = kDiagMaxDim + 1;    // doubles between two rows of the observes' LDS tile: odd, so 8 rows take 8 bank pairs
static_assert(kSymbolStats == kSuffStats + 2 * kDiagSlots, "sy and syy fill the 512 doubles behind the 88");
static_assert(kDiagSlots == kThreads, "a thread of the re-table stages one slot of the means and the sigmas");

// log N(y; mean[s], diag sigma[s]^2) up to log_norm: y the step's D coordinates; mean and sigma the state's entries of coordinate 0,
// stride the doubles between two coordinates of a state (8 in the kernel's transposed staging, 1 in a [s][32] array)
__host__ __device__ inline double diag_entry(const double* y, int D, const double* mean, const double* sigma, int stride, double log_norm)
{
#pragma clang fp contract(off)
    bool inf = false;
    double q = 0.0;
    for (int d = 0; d < D; ++d) {
        const double yd = y[d];
        if (fabs(yd) == INFINITY) inf = true;
        double r = (yd - mean[d * stride]) / sigma[d * stride];
        r *= r;
        q = q + r;
    }
    if (inf) return -INFINITY;
    q += log_norm;
    q *= -0.5;
    return q;
}

// the sum of the coordinates' log_norms, ascending from 0.0: ln the state's logarithm of coordinate 0, stride as in diag_entry
__host__ __device__ inline double diag_log_norm(const double* ln, int D, int stride)
{
#pragma clang fp contract(off)
    double tot = 0.0;
    for (int d = 0; d < D; ++d) tot = tot + ln[d * stride];
    return tot;
}

// the bits of one problem's diagonal table (means [k][D], sigmas [k][D], trans [k][k]), serially: the host's validation and the kernel's
// parallel check form these bits
__host__ __device__ inline int diag_check(const double* means, const double* sigmas, const double* trans, int k, int D)
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
        for (int d = 0; d < D; ++d) {
            if (!(fabs(means[s * D + d]) < INFINITY)) bits |= kRetableBadMean;
            if (scale_bad(sigmas[s * D + d])) bits |= kRetableBadScale;
        }
    }
    return bits;
}

// entry (s, d) of one problem's diagonal M-step: rec its record [kSymbolStats]; means and sigmas [k][D] and trans [k][k] updated in
// place; d = 0 also forms the state's transition row
__host__ __device__ inline void diag_mstep(const double* rec, int k, int D, int s, int d, double* means, double* sigmas, double* trans, double floor)
{
#pragma clang fp contract(off)
    if (d == 0) {
        double row = 0.0;
        for (int j = 0; j < k; ++j) row = row + rec[8 * s + j];
        if (row > 0.0) for (int j = 0; j < k; ++j) trans[s * k + j] = rec[8 * s + j] / row;
    }
    const double occ = rec[64 + s];
    if (occ > 0.0) {
        const double* sy = rec + kSuffStats + 2 * kDiagMaxDim * s;
        const double m = sy[d] / occ;
        means[s * D + d] = m;
        sigmas[s * D + d] = scale_sigma(occ, sy[kDiagMaxDim + d], m, floor);
    }
}

struct BatchRetableDiagArgs {
    const BatchProblem* prob;                  // [B]: T_b
    const int64_t* first;                      // [B]: problem b's first step in obs (the lengths before it; D doubles a step)
    const double* means;                       // [B][k][D]
    const double* sigmas;                      // [B][k][D]
    const double* trans;                       // [B][k][k]
    const double* obs;                         // the observes, packed problem after problem, step after step, D doubles a step
    double* tab;                               // [B][T_max][kBatchTab]
    uint64_t* thr;                             // [B][64]
    int32_t* status;                           // [B]: 0, or the bits of diag_check
    double* mean_out;                          // [B][8][32]: the means in force (slots outside the table 0.0)
    double* sigma_out;                         // [B][8][32]: the sigmas in force (slots outside the table 0.0)
    double* log_norm_out;                      // [B][8]: the states' log_norms (states >= k 0.0)
    int T_max, k, D;
};

__global__ __launch_bounds__(kThreads) void batch_retable_diag_kernel(BatchRetableDiagArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_trans[64];                              // the problem's transition rows, [k][k]
    __shared__ double s_mean[kDiagSlots], s_sigma[kDiagSlots];  // transposed: entry (s, d) at 8 d + s
    __shared__ double s_ln[kDiagSlots];                         // scale_log_norm of every sigma, transposed alike
    __shared__ double s_log_norm[8];                            // the states' sums of them
    __shared__ double s_y[kRetableRows * kDiagTileStride];      // a tile's observes: row r, coordinate d at 33 r + d
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, k = a.k, D = a.D;
    // the thread's slot
    const int s0 = tid >> 5, d0 = tid & 31;
    const bool in = s0 < k && d0 < D;
    const int64_t at = ((int64_t)b * k + s0) * D + d0;
    const double m0 = in ? a.means[at] : 0.0, g0 = in ? a.sigmas[at] : 0.0;
    int bits = 0;
    if (in && !(fabs(m0) < INFINITY)) bits |= kRetableBadMean;
    if (in && scale_bad(g0)) bits |= kRetableBadScale;
    if (tid < k * k) {
        const double w = a.trans[(int64_t)b * k * k + tid];
        s_trans[tid] = w;
        if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
    }
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
    s_mean[8 * d0 + s0] = m0;
    s_sigma[8 * d0 + s0] = g0;
    s_ln[8 * d0 + s0] = in ? scale_log_norm(g0) : 0.0;
    __syncthreads();
    if (tid < 8) s_log_norm[tid] = tid < k ? diag_log_norm(s_ln + tid, D, 8) : 0.0;
    __syncthreads();
    if (blockIdx.y == 0) {
        a.mean_out[(int64_t)b * kDiagSlots + tid] = m0;
        a.sigma_out[(int64_t)b * kDiagSlots + tid] = g0;
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
        for (int e = tid; e < n; e += kThreads) s_y[(e / D) * kDiagTileStride + e % D] = src[e];
        __syncthreads();
        if (r < n_rows) rows[(t0 + r) * kBatchTab + s] = s < k ? diag_entry(s_y + r * kDiagTileStride, D, s_mean + s, s_sigma + s, 8, log_norm) : -INFINITY;
        __syncthreads();                                        // (the next trip's load overwrites the tile)
    }
}

struct BatchDiagStatsArgs {
    const BatchSmoothProblem* desc;            // [B]: T, rows (first row in the m table) and trows (first step: the lengths before it)
    const double* mass;                        // the m table the counting pass left
    const uint64_t* thr;                       // as BatchSmoothArgs::thr
    const double* obs;                         // the observes packed problem after problem, D doubles a step
    double* stats;                             // [B][kSymbolStats]
    int B, k, D, thr_stride;
};

// the lane's coordinates 8 i + dp of the step at y, i < live; a coordinate >= D is not loaded and reads as 0.0
__device__ __forceinline__ void diag_load(double (&v)[4], const double* y, int dp, int D, int live)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (i < live && 8 * i + dp < D) ? y[8 * i + dp] : 0.0;
}

// step t's additions: g y and g (y y) of the lane's live coordinates
__device__ __forceinline__ void diag_add(double (&sy)[4], double (&syy)[4], const double (&v)[4], double g, int live)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < live) {                                         // (wavefront-uniform)
            sy[i] = sy[i] + dmul_rn(g, v[i]);
            syy[i] = syy[i] + dmul_rn(g, dmul_rn(v[i], v[i]));
        }
}

__global__ __launch_bounds__(kThreads) void batch_diag_stats_kernel(BatchDiagStatsArgs a)
{
#pragma clang fp contract(off)
    const int lane = lane_id(), sp = lane >> 3, s = lane & 7;
    const int D = a.D, live = suff_uniform((D + 7) >> 3);
    for (int b = suff_uniform((int)blockIdx.x * kWaves + wave_id()); b < a.B; b += (int)gridDim.x * kWaves) {   // (wavefront-uniform)
        const BatchSmoothProblem d = a.desc[b];
        double* out = a.stats + (int64_t)b * kSymbolStats;
        const int T = d.T;
        double xi = 0.0, occ = 0.0, occ_y = 0.0, occ_yy = 0.0;
        double sy[4], syy[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { sy[i] = 0.0; syy[i] = 0.0; }
        if (T > 0) {
            const double* mass = a.mass + d.rows * 8;
            const double* y = a.obs + d.trows * D;
            const double p = smooth_trans_mass(a.thr + (int64_t)b * a.thr_stride, a.k, s, sp);
            double g = smooth_marginal_start(mass + (int64_t)(T - 1) * 8, s);
            double yt = y[(int64_t)(T - 1) * D];
            double v[4];
            diag_load(v, y + (int64_t)(T - 1) * D, sp, D, live);
            occ = occ + g;
            occ_y = occ_y + dmul_rn(g, yt);
            occ_yy = occ_yy + dmul_rn(g, dmul_rn(yt, yt));
            diag_add(sy, syy, v, g, live);
            // the row and the observes of the step to come (T = 1: row 0 once more, never used)
            int tn = T - 2 > 0 ? T - 2 : 0;
            double m[8];
            double mt = smooth_load_row(mass + (int64_t)tn * 8, s, m);
            yt = y[(int64_t)tn * D];
            diag_load(v, y + (int64_t)tn * D, sp, D, live);
            for (int t = T - 2; t >= 0; --t) {
                double mc[8], vc[4];
#pragma unroll
                for (int j = 0; j < 8; ++j) mc[j] = m[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) vc[i] = v[i];
                const double mtc = mt, yc = yt;
                tn = t > 0 ? t - 1 : 0;                             // (step 0 loads its own row again: in bounds, never used)
                mt = smooth_load_row(mass + (int64_t)tn * 8, s, m);
                yt = y[(int64_t)tn * D];
                diag_load(v, y + (int64_t)tn * D, sp, D, live);
                const double term = smooth_marginal_term(mtc, mc, p, g, sp);
                xi = xi + term;
                g = smooth_marginal_sum(term, s);
                occ = occ + g;
                occ_y = occ_y + dmul_rn(g, yc);
                occ_yy = occ_yy + dmul_rn(g, dmul_rn(yc, yc));
                diag_add(sy, syy, vc, g, live);
            }
        }
        out[8 * s + sp] = xi;
        if (sp == 0) { out[64 + s] = occ; out[72 + s] = occ_y; out[80 + s] = occ_yy; }
        // lane (d', s) holds sy[s][8 i + d'] and syy[s][8 i + d']; states >= k and coordinates >= D are zero
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = s < a.k && 8 * i + sp < D;
            out[kSuffStats + 2 * kDiagMaxDim * s + 8 * i + sp] = in ? sy[i] : 0.0;
            out[kSuffStats + 2 * kDiagMaxDim * s + kDiagMaxDim + 8 * i + sp] = in ? syy[i] : 0.0;
        }
    }
}

struct BatchMstepDiagArgs {
    const double* stats;                       // [B][kSymbolStats]
    double* means;                             // [B][k][D]
    double* sigmas;                            // [B][k][D]
    double* trans;                             // [B][k][k]
    double floor;
    int64_t B;
    int k, D;
};

// one thread a (problem, state s < k, coordinate d < D)
__global__ __launch_bounds__(kThreads) void batch_mstep_diag_kernel(BatchMstepDiagArgs a)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x, kd = (int64_t)a.k * a.D;
    if (i >= a.B * kd) return;
    const int64_t b = i / kd;
    const int sd = (int)(i % kd);
    diag_mstep(a.stats + b * kSymbolStats, a.k, a.D, sd / a.D, sd % a.D, a.means + b * kd, a.sigmas + b * kd, a.trans + b * a.k * a.k, a.floor);
}

}  // namespace cph
