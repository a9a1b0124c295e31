// Running sufficient statistics of an online batch, forward-only (cpprob_hip_batch_online_stats, _online_stats_device): the 88 numbers
// of cpprob_hip_batch_smooth_stats (csrc/batch_suffstats.hpp) at the length a stream has reached, for the cost of its new steps.  The
// backward walk sums the two-slice posteriors over all L rows of the m table on every call; the forward-only smoothing of additive
// functionals (Cappe 2011; Del Moral, Doucet & Singh 2010) keeps, for every current state s',
//   tau_t[s'][.] = E[statistics of steps 0..t | x_t = s', y_0..y_t]
// and pushes it one step with the backward kernel the smoother already forms from row t - 1 of the m table.  In exact arithmetic the
// read-out below IS the backward walk's record (tests/test_onlinestats_ref_host.py, in Fractions); in doubles the two differ by rounding.
//
// The statement, per problem (k its states, m_t its rows of the m table with states >= k zero, p[s][s'] = smooth_trans_mass, y_t its
// observes -- 0.0 where none are passed; column j of a row of tau as the record's: 8 s + s'' for xi[s][s''], 64 + s occ, 72 + s occ_y,
// 80 + s occ_yy).  tau[8][88] lives on the device for the life of the online batch, `done` (host state) counts the steps consumed.
//   step t = done with observe y:
//     t = 0:  tau'[s'][.] = 0.0
//     t >= 1, m = m_{t-1}:  a[s'][s] = dmul_rn(m[s], p[s][s']);  D[s'] = sum of a[s'][s], s = 0..7 in that order from 0.0;  Dm the same sum
//             of m[s];  w[s'][s] = D[s'] == 0.0 ? m[s] / Dm : a[s'][s] / D[s']   (smooth_marginal_term's numerator, denominator and
//             defensive rule, before its multiplication by g)
//             tau'[s'][j] = sum over s = 0..k-1 ascending, from 0.0, of dmul_rn(w[s'][s], v),  v = tau[s][j] + 1.0 where j == 8 s + s'
//             (the transition s -> s' this step takes), else tau[s][j]
//     then    tau'[s'][64 + s'] += 1.0,  tau'[s'][72 + s'] += y,  tau'[s'][80 + s'] += dmul_rn(y, y);  rows s' >= k stay 0.0
//   read-out at length L (tau unchanged):  L = 0: 88 zeros;  else g[s'] = smooth_marginal_start(m_{L-1}, s') and
//             out[j] = sum over s' = 0..k-1 ascending, from 0.0, of dmul_rn(g[s'], tau[s'][j])
// Nothing is contracted.  tests/onlinestats_ref.py restates it.
//
// One wavefront a problem, kWaves problems a workgroup (and the problems gridDim.x * kWaves apart), as batch_smooth_stats_kernel.  Lane
// (s', c) = 8 s' + c keeps the eleven columns j = 8 i + c, i = 0..10, of row s' of tau in registers for the whole walk; it forms
// w[s'][c] as the smoother's lane (s', s = c) does (eight shuffles for D, one division), gathers its row's eight weights and, for every
// source state s < k, row s of tau from the lanes (s, c) with wavefront shuffles.  No LDS, no barrier, no atomics, no result that depends
// on the grid.  The walk over steps [done, L) is a serial chain: the row and the observe of step t + 1 are loaded before step t's
// arithmetic.  A problem with no new steps loads tau and does the read-out only; tau is stored back only where a step was taken.
#pragma once
#include "batch_smooth.hpp"

namespace cph {

constexpr int kOnlineStats = 88;                    // doubles a record: xi[8][8], occ[8], occ_y[8], occ_yy[8]
constexpr int kOnlineCols = kOnlineStats / 8;       // columns of tau a lane keeps
constexpr int kOnlineTau = 8 * kOnlineStats;        // doubles of tau a problem: [8][88]

struct BatchOnlineStatsArgs {
    const BatchSmoothProblem* desc;            // [B]: T (the length reached), rows (first row in the m table), trows (first new observe), lo (done)
    const double* mass;                        // the m table: rows [0, T) of every problem are valid
    const uint64_t* thr;                       // as BatchSmoothArgs::thr
    const double* obs;                         // the observes of the steps [done_b, T_b), packed problem after problem; nullptr: every y is 0.0
    double* tau;                               // [B][8][88]; a problem with done = 0 is never read
    double* stats;                             // [B][kOnlineStats]
    int B, k, thr_stride;
};

// v, which every lane of the wavefront holds alike, as a value the compiler knows to be uniform
__device__ __forceinline__ int online_uniform(int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

// w[s'][c] on lane (s', c): mt = m[c], the step's masses m = m_{t-1}[0..8) and p = double(P[c][s']).
__device__ __forceinline__ double online_weight(double mt, const double (&m)[8], double p, int sp)
{
#pragma clang fp contract(off)
    const double av = dmul_rn(mt, p);
    double D = 0.0, Dm = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { D = D + __shfl(av, sp * 8 + j); Dm = Dm + m[j]; }
    const bool none = D == 0.0;                                 // (the defensive rule: the row falls back to the filtering masses)
    return (none ? mt : av) / (none ? Dm : D);
}

__global__ __launch_bounds__(kThreads) void batch_online_stats_kernel(BatchOnlineStatsArgs a)
{
#pragma clang fp contract(off)
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
        const double* y = a.obs ? a.obs + d.trows : nullptr;
        double* tp = a.tau + (int64_t)b * kOnlineTau + sp * kOnlineStats + c;
        const int done = d.lo < T ? d.lo : T;
        double tau[kOnlineCols];
#pragma unroll
        for (int i = 0; i < kOnlineCols; ++i) tau[i] = done > 0 ? tp[8 * i] : 0.0;
        if (done < T) {
            const double p = smooth_trans_mass(a.thr + (int64_t)b * a.thr_stride, a.k, c, sp);
            // the row and the observe of the first step walked (step 0 has no row: row 0, never used)
            double m[8];
            double mt = smooth_load_row(mass + (int64_t)(done > 0 ? done - 1 : 0) * 8, c, m);
            double yt = y ? y[0] : 0.0;
            for (int t = done; t < T; ++t) {
                double mc[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) mc[j] = m[j];
                const double mtc = mt, yc = yt;
                mt = smooth_load_row(mass + (int64_t)t * 8, c, m);          // (row t serves step t + 1; t < T: reached, the last one never used)
                yt = y ? y[(t + 1 < T ? t + 1 : t) - done] : 0.0;
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
                                double v = __shfl(tau[i], s * 8 + c);
                                if (i == s) v = diag ? v + 1.0 : v;         // j == 8 s + s': the transition s -> s'
                                acc[i] = acc[i] + dmul_rn(w[s], v);
                            }
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < kOnlineCols; ++i) tau[i] = live ? acc[i] : 0.0;
                if (diag) { tau[8] = tau[8] + 1.0; tau[9] = tau[9] + yc; tau[10] = tau[10] + dmul_rn(yc, yc); }
            }
#pragma unroll
            for (int i = 0; i < kOnlineCols; ++i) tp[8 * i] = tau[i];
        }
        const double g = smooth_marginal_start(mass + (int64_t)(T - 1) * 8, sp);
#pragma unroll
        for (int i = 0; i < kOnlineCols; ++i) {
            const double term = dmul_rn(g, tau[i]);
            double o = 0.0;
#pragma unroll
            for (int s = 0; s < 8; ++s) if (s < a.k) o = o + __shfl(term, s * 8 + c);
            if (sp == 0) out[8 * i + c] = o;
        }
    }
}

}  // namespace cph
