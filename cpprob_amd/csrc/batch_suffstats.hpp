// Expected sufficient statistics of a batch (cpprob_hip_batch_smooth_stats, _smooth_stats_device): the E-step of an EM fit of the
// problems' HMM tables, from the backward smoother's own walk (csrc/batch_smooth.hpp).  The term lane (s', s) forms at step t is the
// two-slice posterior P(x_t = s, x_{t+1} = s' | y); the marginals sum it over s' and drop it, this pass also sums it over t.
//
// Per problem (T its length, m_t its masses, y_t its observes), walking t = T-1 .. 0 as smooth_marginals does -- the same start, the
// same pair smooth_marginal_term / smooth_marginal_sum, so every g_t is the marginals' bits:
//   xi[s][s'] = sum over t = T-2 .. 0 of term_t(s', s)           (terms with g_{t+1}[s'] = 0 are 0)
//   occ[s]    = sum over t = T-1 .. 0 of g_t[s]
//   occ_y[s]  = sum over t of g_t[s] * y_t,  occ_yy[s] = sum over t of g_t[s] * (y_t * y_t)
// Every accumulator starts at 0.0 and takes one addition a step, in walk order; every product is one rounded multiplication, nothing
// is contracted.  The record of a problem: 88 doubles, xi at 8 s + s', then occ[8], occ_y[8], occ_yy[8]; states >= k are zero, a
// problem of length 0 is all zero, T = 1 has xi = 0.  tests/suffstats_ref.py restates it.
//
// One wavefront a problem, kWaves problems a workgroup (and the problems gridDim.x * kWaves apart): lane (s', s) = 8 s' + s keeps its
// xi accumulator in a register for the whole walk -- the 64 lanes are the 64 entries -- and the lanes (0, s) keep occ, occ_y, occ_yy.
// No LDS, no barrier, no atomics, no result that depends on the grid.  The walk is a serial chain (a row, 17 shuffles and a division
// a step), so the row and the observe of step t - 1 are loaded before step t's arithmetic and waited for after it; the problem index
// is made wavefront-uniform for the compiler: the descriptor is a scalar load, the row's eight masses and y_t loads of one address.
#pragma once
#include "batch_smooth.hpp"

namespace cph {

constexpr int kSuffStats = 88;                      // doubles a problem: xi[8][8], occ[8], occ_y[8], occ_yy[8]

struct BatchSmoothStatsArgs {
    const BatchSmoothProblem* desc;            // [B]: T, rows (first row in the m table) and trows (first observe: the lengths before it)
    const double* mass;                        // the m table the counting pass left
    const uint64_t* thr;                       // as BatchSmoothArgs::thr
    const double* obs;                         // the observes packed problem after problem by the lengths reached; nullptr: occ_y, occ_yy stay 0
    double* stats;                             // [B][kSuffStats]
    int B, k, thr_stride;
};

// v, which every lane of the wavefront holds alike, as a value the compiler knows to be uniform
__device__ __forceinline__ int suff_uniform(int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

__global__ __launch_bounds__(kThreads) void batch_smooth_stats_kernel(BatchSmoothStatsArgs a)
{
#pragma clang fp contract(off)
    const int lane = lane_id(), sp = lane >> 3, s = lane & 7;
    for (int b = suff_uniform((int)blockIdx.x * kWaves + wave_id()); b < a.B; b += (int)gridDim.x * kWaves) {   // (wavefront-uniform)
        const BatchSmoothProblem d = a.desc[b];
        double* out = a.stats + (int64_t)b * kSuffStats;
        const int T = d.T;
        double xi = 0.0, occ = 0.0, occ_y = 0.0, occ_yy = 0.0;
        if (T > 0) {
            const double* mass = a.mass + d.rows * 8;
            const double* y = a.obs ? a.obs + d.trows : nullptr;
            const double p = smooth_trans_mass(a.thr + (int64_t)b * a.thr_stride, a.k, s, sp);
            double g = smooth_marginal_start(mass + (int64_t)(T - 1) * 8, s);
            double yt = y ? y[T - 1] : 0.0;
            occ = occ + g;
            occ_y = occ_y + dmul_rn(g, yt);
            occ_yy = occ_yy + dmul_rn(g, dmul_rn(yt, yt));
            // the row and the observe of the step to come (T = 1: row 0 once more, never used)
            int tn = T - 2 > 0 ? T - 2 : 0;
            double m[8];
            double mt = smooth_load_row(mass + (int64_t)tn * 8, s, m);
            yt = y ? y[tn] : 0.0;
            for (int t = T - 2; t >= 0; --t) {
                double mc[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) mc[j] = m[j];
                const double mtc = mt, yc = yt;
                tn = t > 0 ? t - 1 : 0;                             // (step 0 loads its own row again: in bounds, never used)
                mt = smooth_load_row(mass + (int64_t)tn * 8, s, m);
                yt = y ? y[tn] : 0.0;
                const double term = smooth_marginal_term(mtc, mc, p, g, sp);
                xi = xi + term;
                g = smooth_marginal_sum(term, s);
                occ = occ + g;
                occ_y = occ_y + dmul_rn(g, yc);
                occ_yy = occ_yy + dmul_rn(g, dmul_rn(yc, yc));
            }
        }
        out[8 * s + sp] = xi;
        if (sp == 0) { out[64 + s] = occ; out[72 + s] = occ_y; out[80 + s] = occ_yy; }
    }
}

}  // namespace cph
