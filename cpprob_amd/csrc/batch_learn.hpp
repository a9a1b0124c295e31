// Online EM of an online CPPROB_HIP_MODEL_HMM_TABLE batch (cpprob_hip_batch_learn_begin, _learn_begin_scaled, _advance_learn): the tables
// of a stream that are not known in advance, learned on the device while its observes arrive -- the stochastic-approximation form of
// Cappe 2011, Alg. 1.  A learning advance enqueues three steps: the rows kernel, the run (batch_launch, as it is), the learn kernel.
// Each of the two is one body, batch_learn_rows_body<kScaled> and batch_learn_body<kScaled>, under two kernels: batch_learn_rows_kernel
// and batch_learn_kernel for a batch of unit scales, batch_learn_rows_scaled_kernel and batch_learn_scaled_kernel for a batch with
// per-state emission scales (csrc/batch_scale.hpp).  What the scales add stands under `if constexpr (kScaled)`: the unit kernels load
// no scale and read neither `fit` nor `floor`.
//
// Rows.  Row t of problem b, t in [L_b, L_b + dT_b):  tab[(b T_max + t) 8 + s] = retable_entry(y_t, mean_b[s], log_norm) for s < k,
// -inf beyond, from the device-resident means in force (log_norm from the host, csrc/batch_retable.hpp); kScaled: scale_entry on the
// device-resident mean, sigma and log_norm of the state (the [B][8] arrays of the context's own; it takes no logarithm).  blockIdx.x
// the problem, blockIdx.y strides over tiles of kRetableRows new steps; eight lanes a row, lane s the entry s: a wavefront stores 512
// consecutive bytes.  Rows a problem has taken before, rows past its new length and everything else in the workspace are not touched.
//
// Learn.  One wavefront a problem, kWaves problems a workgroup, the lane layout of batch_online_stats_kernel: lane (s', c) = 8 s' + c
// keeps the columns j = 8 i + c, i = 0..10, of row s' of a tau of the learner's own in registers.
//   (a) the discounted step t in [done_b, L_b) with observe y, g = gamma[t], om = 1.0 - g:
//         t = 0:  tau'[s'][.] = 0.0
//         t >= 1: w[s'][s] = online_weight;  tau'[s'][j] = sum over s = 0..k-1 ascending, from 0.0, of dmul_rn(w[s'][s], v),
//                 v = dmul_rn(om, tau[s][j]), and v + g where j == 8 s + s'
//         then    tau'[s'][64 + s'] += g,  tau'[s'][72 + s'] += dmul_rn(g, y),  tau'[s'][80 + s'] += dmul_rn(g, dmul_rn(y, y));
//                 rows s' >= k stay 0.0
//       p of online_weight is read from the threshold words before (c) writes them: the words the advance's steps were drawn with.
//   (b) the record at the new length, batch_online_stats_kernel's read-out, stored in stats[b][88]; a problem of length 0: 88 zeros.
//   (c) where done_b < L_b and L_b >= t_min: the M-step on the record, in registers -- lane (s, j) forms retable_mstep's row total of
//       state s with eight shuffles and its entry trans'[s][j], lane (., c) the mean of state c --, retable_check's predicates on the
//       new table (a row's bits on its lanes, gathered with shuffles), and
//         no bit set:  the table is stored over the old one, word 8 s + j of the problem's 64 threshold words is rewritten by
//                      retable_threshold on the new row s, status[b] = 0
//         a bit set:   nothing but status[b] = the bits is stored: the old table and the old words stay in force
//       A problem (c) does not visit keeps its table, its words and its status word.
//       kScaled: lane (., c) also holds state c's sigma and log_norm and -- where the learner fits the scales (fit != 0) and the state
//       has mass -- forms scale_sigma on occ, occ_yy and the new mean, and scale_log_norm of it where scale_bad does not refuse it.
//       The check is retable_check's predicates and bit 8 for a refused sigma (scale_check).  No bit set: the sigmas and the log_norms
//       are stored with the table; a bit set: they stay with it.  fit == 0 (a plain cpprob_hip_batch_learn_begin on a scaled batch):
//       sigmas and log_norms are read, checked and never written.
// With gamma[t] = 1 / (t + 1) the record is the running mean of batch_online_stats' sums.  Nothing is contracted, no LDS, no barrier, no
// atomics, no result that depends on the grid.  tests/learn_ref.py and tests/scale_ref.py restate it; tests/host_kernels/
// batch_learn_main.cpp and batch_learn_scaled_main.cpp run this text on the host; tests/test_gpu_batch_learn_scaled.py holds the
// resident scaled stream against a host-stepped one.
#pragma once
#include "batch_onlinestats.hpp"
#include "batch_scale.hpp"

namespace cph {

struct BatchLearnRowsArgs {
    const BatchProblem* prob;                  // [B]: T_b, the new length
    const int32_t* first;                      // [B]: the length before the advance; < 0: the problem is idle
    const int64_t* ofirst;                     // [B]: problem b's first new observe in obs
    const double* means;                       // [B][k], the device-resident tables
    const double* obs;                         // the new observes, packed problem after problem
    double* tab;                               // [B][T_max][kBatchTab]
    double log_norm;                           // log(2 pi 1 1), from the host
    int T_max, k;
};

struct BatchLearnRowsScaledArgs {             // (BatchLearnRowsArgs with the resident scales in the host's log_norm's place)
    const BatchProblem* prob;
    const int32_t* first;
    const int64_t* ofirst;
    const double* means;
    const double* sigmas;                      // [B][8]
    const double* log_norms;                   // [B][8]
    const double* obs;
    double* tab;
    int T_max, k;
};

// Args: BatchLearnRowsArgs, or kScaled: BatchLearnRowsScaledArgs
template <bool kScaled, class Args>
__device__ __forceinline__ void batch_learn_rows_body(Args a)
{
#pragma clang fp contract(off)
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, s = tid & 7;
    const int64_t L0 = a.first[b], L = a.prob[b].T;
    if (L0 < 0 || L0 >= L) return;                              // (workgroup-uniform)
    const double mean = s < a.k ? a.means[(int64_t)b * a.k + s] : 0.0;
    double sigma = 1.0, log_norm;
    if constexpr (kScaled) { sigma = s < a.k ? a.sigmas[(int64_t)b * 8 + s] : 1.0; log_norm = s < a.k ? a.log_norms[(int64_t)b * 8 + s] : 0.0; }
    else log_norm = a.log_norm;
    const double* y = a.obs + a.ofirst[b] - L0;                 // (indexed by the absolute step: y[t], t in [L0, L))
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    const int64_t stride = (int64_t)gridDim.y * kRetableRows;
    for (int64_t t = L0 + (int64_t)blockIdx.y * kRetableRows + (tid >> 3); t < L; t += stride)
        rows[t * kBatchTab + s] = s < a.k ? (kScaled ? scale_entry(y[t], mean, sigma, log_norm) : retable_entry(y[t], mean, log_norm)) : -INFINITY;
}

__global__ __launch_bounds__(kThreads) void batch_learn_rows_kernel(BatchLearnRowsArgs a)
{
#pragma clang fp contract(off)
    batch_learn_rows_body<false>(a);
}

__global__ __launch_bounds__(kThreads) void batch_learn_rows_scaled_kernel(BatchLearnRowsScaledArgs a)
{
#pragma clang fp contract(off)
    batch_learn_rows_body<true>(a);
}

struct BatchLearnArgs {
    const BatchSmoothProblem* desc;            // [B]: T (the length reached), rows (first row in the m table), trows (first new observe), lo (done)
    const double* mass;                        // the m table: rows [0, T) of every problem are valid
    uint64_t* thr;                             // [B][64]: read for p, rewritten under (c)
    const double* obs;                         // the observes of the steps [done_b, T_b), packed problem after problem
    const double* gamma;                       // the step sizes, indexed by the absolute step
    double* tau;                               // [B][8][88], the learner's own; a problem with done = 0 is never read
    double* stats;                             // [B][kOnlineStats]
    double* means;                             // [B][k]
    double* trans;                             // [B][k][k]
    int32_t* status;                           // [B]
    int B, k, t_min;
};

// retable_check's predicates on row s of a table (row: its k weights, mean: its mean)
__device__ __forceinline__ int learn_row_bits(const double (&row)[8], double mean, int k)
{
#pragma clang fp contract(off)
    int bits = 0;
    double tot = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < k) {
            const double w = row[j];
            if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
            tot += w;
        }
    }
    if (!(tot > 0.0)) bits |= kRetableNoMass;
    if (!(fabs(mean) < INFINITY)) bits |= kRetableBadMean;
    return bits;
}

struct BatchLearnScaledArgs {
    BatchLearnArgs base;                       // batch_learn_kernel's arguments
    double* sigmas;                            // [B][8]
    double* log_norms;                         // [B][8]
    double floor;                              // the scales' floor (fit != 0)
    int fit;                                   // the learner fits the scales
};

// Args: BatchLearnArgs, or kScaled: BatchLearnScaledArgs
template <bool kScaled, class Args>
__device__ __forceinline__ void batch_learn_body(Args sa)
{
#pragma clang fp contract(off)
    BatchLearnArgs a;
    if constexpr (kScaled) a = sa.base; else a = sa;
    const int lane = lane_id(), sp = lane >> 3, c = lane & 7;
    const bool live = sp < a.k, diag = live && c == sp;
    for (int b = online_uniform((int)blockIdx.x * kWaves + wave_id()); b < a.B; b += (int)gridDim.x * kWaves) {   // (wavefront-uniform)
        const BatchSmoothProblem d = a.desc[b];
        double* out = a.stats + (int64_t)b * kOnlineStats;
        const int T = d.T;
        if (T <= 0) {                                           // nothing reached yet
#pragma unroll
            for (int i = 0; i < kOnlineCols; ++i) if (sp == 0) out[8 * i + c] = 0.0;
            continue;
        }
        const double* mass = a.mass + d.rows * 8;
        const double* y = a.obs + d.trows;
        double* tp = a.tau + (int64_t)b * kOnlineTau + sp * kOnlineStats + c;
        uint64_t* thr = a.thr + (int64_t)b * 64;
        const int done = d.lo < T ? d.lo : T;
        double tau[kOnlineCols];
#pragma unroll
        for (int i = 0; i < kOnlineCols; ++i) tau[i] = done > 0 ? tp[8 * i] : 0.0;
        if (done < T) {
            const double p = smooth_trans_mass(thr, a.k, c, sp);            // (the words the new steps were drawn with)
            double m[8];
            double mt = smooth_load_row(mass + (int64_t)(done > 0 ? done - 1 : 0) * 8, c, m);
            double yt = y[0], gt = a.gamma[done];
            for (int t = done; t < T; ++t) {
                double mc[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) mc[j] = m[j];
                const double mtc = mt, yc = yt, g = gt, om = 1.0 - g;
                mt = smooth_load_row(mass + (int64_t)t * 8, c, m);          // (row t serves step t + 1; t < T: reached, the last one never used)
                const int tn = t + 1 < T ? t + 1 : t;
                yt = y[tn - done]; gt = a.gamma[tn];
                double acc[kOnlineCols];
#pragma unroll
                for (int i = 0; i < kOnlineCols; ++i) acc[i] = 0.0;
                if (t > 0) {
                    const double w_own = online_weight(mtc, mc, p, sp);
                    double w[8];
#pragma unroll
                    for (int s = 0; s < 8; ++s) w[s] = __shfl(w_own, sp * 8 + s);
#pragma unroll
                    for (int s = 0; s < 8; ++s) {
                        if (s < a.k) {                                      // (uniform)
#pragma unroll
                            for (int i = 0; i < kOnlineCols; ++i) {
                                double v = dmul_rn(om, __shfl(tau[i], s * 8 + c));
                                if (i == s) v = diag ? v + g : v;           // j == 8 s + s': the transition s -> s'
                                acc[i] = acc[i] + dmul_rn(w[s], v);
                            }
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < kOnlineCols; ++i) tau[i] = live ? acc[i] : 0.0;
                if (diag) { tau[8] = tau[8] + g; tau[9] = tau[9] + dmul_rn(g, yc); tau[10] = tau[10] + dmul_rn(g, dmul_rn(yc, yc)); }
            }
#pragma unroll
            for (int i = 0; i < kOnlineCols; ++i) tp[8 * i] = tau[i];
        }
        // (b) the record: every lane (., c) ends with rec[8 i + c] in o[i]
        const double gm = smooth_marginal_start(mass + (int64_t)(T - 1) * 8, sp);
        double o[kOnlineCols];
#pragma unroll
        for (int i = 0; i < kOnlineCols; ++i) {
            const double term = dmul_rn(gm, tau[i]);
            double r = 0.0;
#pragma unroll
            for (int s = 0; s < 8; ++s) if (s < a.k) r = r + __shfl(term, s * 8 + c);
            o[i] = r;
            if (sp == 0) out[8 * i + c] = r;
        }
        if (done >= T || T < a.t_min) continue;                 // (uniform)
        // (c) the M-step: lane (s, j) holds xi[s][j] = rec[8 s + j] and forms trans'[s][j]; lane (., c) forms the mean of state c and,
        // kScaled, holds its sigma and its log_norm
        const bool entry = live && c < a.k;
        double* trans = a.trans + (int64_t)b * a.k * a.k;
        double* means = a.means + (int64_t)b * a.k;
        double *sigmas = nullptr, *log_norms = nullptr;
        if constexpr (kScaled) { sigmas = sa.sigmas + (int64_t)b * 8; log_norms = sa.log_norms + (int64_t)b * 8; }
        double xi = 0.0;
#pragma unroll
        for (int i = 0; i < 8; ++i) xi = i == sp ? o[i] : xi;
        double rsum = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const double x = __shfl(xi, sp * 8 + j); if (j < a.k) rsum = rsum + x; }
        double tr = entry ? trans[sp * a.k + c] : 0.0;
        if (rsum > 0.0) tr = entry ? xi / rsum : 0.0;
        double mean = c < a.k ? means[c] : 0.0;
        if (o[8] > 0.0) mean = c < a.k ? o[9] / o[8] : 0.0;
        double sigma = 1.0, log_norm = 0.0;
        int bad_scale = 0;
        if constexpr (kScaled) {
            sigma = c < a.k ? sigmas[c] : 1.0; log_norm = c < a.k ? log_norms[c] : 0.0;
            const bool fitted = sa.fit != 0 && c < a.k && o[8] > 0.0;
            if (fitted) sigma = scale_sigma(o[8], o[10], mean, sa.floor);
            bad_scale = c < a.k && scale_bad(sigma) ? kRetableBadScale : 0;
            if (fitted && !bad_scale) log_norm = scale_log_norm(sigma);
        }
        // the new row s' on each of its lanes, its bits, every row's bits
        double row[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) row[j] = __shfl(tr, sp * 8 + j);
        const double mean_row = __shfl(mean, sp);               // (the mean of state s': lane (0, s') holds it)
        int bad_row = 0;
        if constexpr (kScaled) bad_row = __shfl(bad_scale, sp);  // (every lane takes part: the shuffle stands outside `live`)
        const int mine = live ? learn_row_bits(row, mean_row, a.k) | bad_row : 0;
        int bits = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) bits |= __shfl(mine, s * 8);
        if (lane == 0) a.status[b] = bits;
        if (bits) continue;                                     // (uniform: the old table, scales and words stay)
        if (entry) trans[sp * a.k + c] = tr;
        if (sp == 0 && c < a.k) means[c] = mean;
        if constexpr (kScaled) if (sa.fit != 0 && sp == 0 && c < a.k) { sigmas[c] = sigma; log_norms[c] = log_norm; }
        thr[lane] = live ? retable_threshold(row, a.k, 0, c) : ~0ull;      // (the row alone is row 0 of retable_threshold's table)
    }
}

__global__ __launch_bounds__(kThreads) void batch_learn_kernel(BatchLearnArgs a)
{
#pragma clang fp contract(off)
    batch_learn_body<false>(a);
}

__global__ __launch_bounds__(kThreads) void batch_learn_scaled_kernel(BatchLearnScaledArgs sa)
{
#pragma clang fp contract(off)
    batch_learn_body<true>(sa);
}

}  // namespace cph
