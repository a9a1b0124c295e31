// Online EM of an online CPPROB_HIP_MODEL_HMM_TABLE batch with per-state emission scales (cpprob_hip_batch_learn_begin_scaled, and
// cpprob_hip_batch_learn_begin on a scaled batch): the siblings of csrc/batch_learn.hpp's two kernels, which are not touched.
//
// Rows.  batch_learn_rows_scaled_kernel: batch_learn_rows_kernel's grid and lanes; the entry is scale_entry on the device-resident mean,
// sigma and log_norm of the state (the [B][8] arrays of the context's own).  It takes no logarithm.
//
// Learn.  batch_learn_scaled_kernel: batch_learn_kernel's steps, statement for statement, with changes in (c) alone:
//   (a) the discounted tau step and (b) the record: unchanged
//   (c) lane (s, j) forms trans'[s][j] as before; lane (., c) holds state c's mean, sigma and log_norm and forms the new mean and --
//       where the learner fits the scales (fit != 0) and the state has mass -- scale_sigma on occ, occ_yy and the new mean, and
//       scale_log_norm of it where scale_bad does not refuse it.  The check is retable_check's predicates and bit 8 for a refused
//       sigma (scale_check).  No bit set: the table, the sigmas, the log_norms and the threshold words are stored, status[b] = 0;
//       a bit set: nothing but status[b] = the bits.  fit == 0 (a plain cpprob_hip_batch_learn_begin on a scaled batch): sigmas and
//       log_norms are read, checked and never written.
// One wavefront a problem, no LDS, no barrier, no atomics, no result that depends on the grid; nothing is contracted.
// tests/test_gpu_batch_learn_scaled.py holds the resident stream against a host-stepped one on tests/learn_ref.py and tests/scale_ref.py.
#pragma once
#include "batch_learn.hpp"
#include "batch_scale.hpp"

namespace cph {

struct BatchLearnRowsScaledArgs {
    const BatchProblem* prob;                  // [B]: T_b, the new length
    const int32_t* first;                      // [B]: the length before the advance; < 0: the problem is idle
    const int64_t* ofirst;                     // [B]: problem b's first new observe in obs
    const double* means;                       // [B][k], the device-resident tables
    const double* sigmas;                      // [B][8]
    const double* log_norms;                   // [B][8]
    const double* obs;                         // the new observes, packed problem after problem
    double* tab;                               // [B][T_max][kBatchTab]
    int T_max, k;
};

__global__ __launch_bounds__(kThreads) void batch_learn_rows_scaled_kernel(BatchLearnRowsScaledArgs a)
{
#pragma clang fp contract(off)
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, s = tid & 7;
    const int64_t L0 = a.first[b], L = a.prob[b].T;
    if (L0 < 0 || L0 >= L) return;                              // (workgroup-uniform)
    const double mean = s < a.k ? a.means[(int64_t)b * a.k + s] : 0.0;
    const double sigma = s < a.k ? a.sigmas[(int64_t)b * 8 + s] : 1.0, log_norm = s < a.k ? a.log_norms[(int64_t)b * 8 + s] : 0.0;
    const double* y = a.obs + a.ofirst[b] - L0;                 // (indexed by the absolute step: y[t], t in [L0, L))
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    const int64_t stride = (int64_t)gridDim.y * kRetableRows;
    for (int64_t t = L0 + (int64_t)blockIdx.y * kRetableRows + (tid >> 3); t < L; t += stride)
        rows[t * kBatchTab + s] = s < a.k ? scale_entry(y[t], mean, sigma, log_norm) : -INFINITY;
}

struct BatchLearnScaledArgs {
    BatchLearnArgs base;                       // batch_learn_kernel's arguments
    double* sigmas;                            // [B][8]
    double* log_norms;                         // [B][8]
    double floor;                              // the scales' floor (fit != 0)
    int fit;                                   // the learner fits the scales
};

__global__ __launch_bounds__(kThreads) void batch_learn_scaled_kernel(BatchLearnScaledArgs sa)
{
#pragma clang fp contract(off)
    const BatchLearnArgs& a = sa.base;
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
        // (c) the scaled M-step: lane (s, j) forms trans'[s][j]; lane (., c) the mean, the sigma and the log_norm of state c
        const bool entry = live && c < a.k;
        double* trans = a.trans + (int64_t)b * a.k * a.k;
        double* means = a.means + (int64_t)b * a.k;
        double* sigmas = sa.sigmas + (int64_t)b * 8;
        double* log_norms = sa.log_norms + (int64_t)b * 8;
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
        double sigma = c < a.k ? sigmas[c] : 1.0, log_norm = c < a.k ? log_norms[c] : 0.0;
        const bool fitted = sa.fit != 0 && c < a.k && o[8] > 0.0;
        if (fitted) sigma = scale_sigma(o[8], o[10], mean, sa.floor);
        const int bad_scale = c < a.k && scale_bad(sigma) ? kRetableBadScale : 0;
        if (fitted && !bad_scale) log_norm = scale_log_norm(sigma);
        // the new row s' on each of its lanes, its bits, every row's bits
        double row[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) row[j] = __shfl(tr, sp * 8 + j);
        const double mean_row = __shfl(mean, sp);               // (the mean of state s': lane (0, s') holds it)
        const int bad_row = __shfl(bad_scale, sp);
        const int mine = live ? learn_row_bits(row, mean_row, a.k) | bad_row : 0;
        int bits = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) bits |= __shfl(mine, s * 8);
        if (lane == 0) a.status[b] = bits;
        if (bits) continue;                                     // (uniform: the old table, scales and words stay)
        if (entry) trans[sp * a.k + c] = tr;
        if (sp == 0 && c < a.k) means[c] = mean;
        if (sa.fit != 0 && sp == 0 && c < a.k) { sigmas[c] = sigma; log_norms[c] = log_norm; }
        thr[lane] = live ? retable_threshold(row, a.k, 0, c) : ~0ull;      // (the row alone is row 0 of retable_threshold's table)
    }
}

}  // namespace cph
