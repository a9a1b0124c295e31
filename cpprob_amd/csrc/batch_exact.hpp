// Exact filter runs of a batch (cpprob_hip_batch_run_exact): the forward recursion of a CPPROB_HIP_MODEL_HMM_TABLE problem over all of
// its k <= 8 states, with no particles.  Like a conditional run (cpprob_hip_batch_run_conditional) it is another forward pass that leaves the backward
// smoother's m table (csrc/batch_smooth.hpp) and nothing else, so whatever serves a filtering batch that keeps its masses serves this
// one unchanged: with it the smoother's statistics are Baum-Welch's, the backward simulation is exact forward filtering / backward
// sampling, the decode is Viterbi over all states and the predictive rows are the exact prequential likelihood.  It costs T k^2 a
// problem whatever n is, takes no seeds, and reads the emission through the rows of `tab` alone: unit, scaled and Poisson batches alike.
//
// The statement, per problem (T its length, k its states, ll_t[0..8) its row of tab, P[s][s'] = smooth_trans_mass of its threshold words,
// the integers the device draws from; tests/exact_ref.py restates it in Python, bit for bit; DESIGN.md section 5 states it once more):
//   t = 0    u_0[s] = 1.0 for s < k, else 0.0: the uniform initial state the runs draw
//   t >= 1   u_t[s'] = sum over s = 0..7 ascending, from 0.0, of dmul_rn(m_{t-1}[s], P[s][s']): the smoother's own D_{t-1}[s'] (states
//            >= k add 0.0)
//   M_t      = max{ll_t[s] : s < k, u_t[s] > 0}
//   q_t[s]   = fix_weight(ll_t[s], M_t) for s < k, else 0: the engine's 32-bit weight
//   w_t[s]   = dmul_rn(u_t[s], double(q_t[s]));  W_t and U_t the sums of w_t[s] and of u_t[s] over s = 0..7 ascending, from 0.0
//   m_t[s]   = rint(dmul_rn(w_t[s] / W_t, 2^44)): an integer <= 2^44, exact as a double; 0.0 for s >= k
//   log_z    = log_z + ((M_t + (table_log(W_t) - table_log(U_t))) - kExactLn2x32), from 0.0: the step's exact predictive likelihood
//              sum_s (u_t[s] / U_t) exp(ll_t[s]), the 2^32 of the weights taken off
// Nothing is contracted (fp contract off in every function of this file; products through dmul_rn).
// Scale: the readers document entries below 2^45 and sum a row as uint64_t (smooth_marginal_start, the conditional run); the forecast,
// the decode and the trajectory statistics read a row through those or through its signs alone.  A row here sums to 2^44 within 4
// units, so 2^44 keeps every reader's bound and none needs less.
// Dead steps: a step with M_t = -inf (every reachable state has a -inf row: an observe outside the emission family's domain) is dead.
// From the first dead step on log_z = -inf and this and every later row are zeros; dead[b] is that step, -1 where there is none.
// table_log's arguments: the state that attains M_t has u > 0 and the weight 2^32 - 1, so W_t >= 1 and U_t >= 1, both below 2^112.
// Horizon: fix_weight gives a state more than about 22 nats below M_t the weight 0, as it does in the particle runs; with the 2^-32
// grid of P and the 2^-44 grid of m these are the run's three quantisations, and it is exact in the sense the device's transition law is.
//
// batch_exact_kernel: one wavefront a problem, kWaves problems a workgroup, the problems gridDim.x * kWaves apart
// (batch_online_stats_kernel's layout): no result depends on the grid.  Lane (s', s) = 8 s' + s keeps P[s][s'] and m_{t-1}[s] in
// registers for the whole walk.  A step: one product a lane; eight shuffles gather the lane's row in order into u[s']; eight more
// gather the u, which with the row's eight ll (wavefront-uniform loads) give M, U and, after ONE fix_weight a lane (its state s'), W;
// a division, a rint; one shuffle puts m[s] back on lane (s', s); lanes (0, s) store the row, 64 consecutive bytes.  The walk over t is
// one serial chain, so row t + 1 of tab is loaded before step t's arithmetic; the two logarithms of a step hang off the chain, not in it.
// (Taking step t + 1's weights off the chain by a reachable-state bitmask is not done: a state's mass can round to 0 on the 2^-44 grid,
// so the reachable set is a function of the values, not of P's zero pattern alone.)  A dead step leaves the walk by a wavefront-uniform
// branch that shuffles nothing.  No LDS, no barrier, no atomics; rows t >= T_b and everything else in the workspace are not touched.
//
// batch_exact_advance_kernel (cpprob_hip_batch_advance_exact): the same statement for the steps t in [first[b], T_b) of every problem of
// an online batch, in the same layout; the step (exact_step) and the walk (exact_walk) are one text under both kernels.  first[b] < 0
// or >= T_b: the problem is idle, nothing of it is read or written.  first[b] == 0 starts as above.  first[b] > 0 resumes: m_{t-1} is
// row first[b] - 1 of the m table -- integers <= 2^44, exact as doubles, so the lanes (s', s) hold the bits the one-shot walk holds --
// and log_z and dead are the problem's entries of the evidence buffers, which are the carry.  The resumed walk is therefore the
// one-shot walk of the length reached, bit for bit.  A problem already dead stores zeros in its new rows; its log_z = -inf and its
// dead stay.  Rows t < first[b] and t >= T_b and everything else in the workspace are not touched.
#pragma once
#include "batch_scale.hpp"
#include "batch_smooth.hpp"

namespace cph {

constexpr double kExactScale = 0x1p44;              // a row of the m table sums to this (within 4 units)
constexpr double kExactLn2x32 = 0x1.62e42fefa39efp+4;   // 32 ln 2, the double of ln 2 times 32 (exact)
constexpr int kExactGridMax = 2048;                 // workgroups at most: kWaves times it problems in flight, the rest strided

struct BatchExactArgs {
    const double* tab;                         // [B][T_max][kBatchTab]: ll_t[0..8) of row b T_max + t
    const uint64_t* thr;                       // problem b's 64 threshold words at thr + b * thr_stride, the layout of ModelParams::hk_thr
    const BatchProblem* prob;                  // [B], described batch; nullptr: uniform
    double* mass;                              // [B][T_max][8]: row (b, t) at (b T_max + t) * 8
    double* log_z;                             // [B]
    int32_t* dead;                             // [B]
    int B, T_max;                              // T_max: uniform: every problem's T
    int k, thr_stride;                         // thr_stride: 0 (one shared table) or 64 (a table a problem)
};

// v, which every lane of the wavefront holds alike, as a value the compiler knows to be uniform (the problem's loads become scalar)
__device__ __forceinline__ int exact_uniform(int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

// Row `row` = ll_t[0..8) of tab as a step takes it: the eight in ll, the entry of the lane's state s' returned.
__device__ __forceinline__ double exact_load_row(const double* row, int sp, double (&ll)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) ll[j] = row[j];
    return row[sp];
}

// One step t of the statement on the lanes (s', s): lc the step's row, lc_sp its entry of state s', ms = m_{t-1}[s] on entry and
// m_t[s] on return, row = row t of the m table (the lanes (0, s) store it).  false: the step is dead, and nothing has been stored.
__device__ __forceinline__ bool exact_step(int t, int k, int sp, int s, double p, const double (&lc)[8], double lc_sp, double& ms, double& log_z, double* row)
{
#pragma clang fp contract(off)
    // u[s'] on the lanes (s', .)
    const double av = dmul_rn(ms, p);
    double u = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) u = u + __shfl(av, sp * 8 + j);
    if (t == 0) u = sp < k ? 1.0 : 0.0;
    // M and U from the eight u, alike in every lane
    double M = -INFINITY, U = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double uj = __shfl(u, 8 * j);
        if (j < k && uj > 0.0) M = fmax(M, lc[j]);
        U = U + uj;
    }
    if (M == -INFINITY) return false;                       // (wavefront-uniform)
    const uint32_t q = sp < k ? fix_weight(lc_sp, M) : 0u;
    const double w = dmul_rn(u, (double)q);
    double W = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) W = W + __shfl(w, 8 * j);
    const double mn = rint(dmul_rn(w / W, kExactScale));    // m_t[s'] on the lanes (s', .)
    ms = __shfl(mn, 8 * s);
    if (sp == 0) row[s] = ms;
    const double dl = table_log(W) - table_log(U);
    log_z = log_z + ((M + dl) - kExactLn2x32);
    return true;
}

// The steps [t0, T) of one problem from its carry (ms = m_{t0-1}[s], log_z; the problem is not dead), the rows read from tab.
__device__ __forceinline__ void exact_walk(const double* tab, double* mass, int t0, int T, int k, int sp, int s, double p, double ms, double& log_z, int& dead)
{
#pragma clang fp contract(off)
    double ll[8];
    double ll_sp = t0 < T ? exact_load_row(tab + (int64_t)t0 * kBatchTab, sp, ll) : 0.0;
    for (int t = t0; t < T; ++t) {
        double lc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) lc[j] = ll[j];
        const double lc_sp = ll_sp;
        ll_sp = exact_load_row(tab + (int64_t)(t + 1 < T ? t + 1 : t) * kBatchTab, sp, ll);   // (the last step loads its own row again: in bounds, never used)
        if (!exact_step(t, k, sp, s, p, lc, lc_sp, ms, log_z, mass + (int64_t)t * 8)) {       // a dead step: zeros from here on
            dead = t;
            log_z = -INFINITY;
            for (int tt = t; tt < T; ++tt) if (sp == 0) mass[(int64_t)tt * 8 + s] = 0.0;
            break;
        }
    }
}

__global__ __launch_bounds__(kThreads) void batch_exact_kernel(BatchExactArgs a)
{
#pragma clang fp contract(off)
    const int lane = lane_id(), sp = lane >> 3, s = lane & 7;
    for (int b = exact_uniform((int)blockIdx.x * kWaves + wave_id()); b < a.B; b += (int)gridDim.x * kWaves) {   // (wavefront-uniform)
        const int T = a.prob ? (int)a.prob[b].T : a.T_max;
        const double p = smooth_trans_mass(a.thr + (int64_t)b * a.thr_stride, a.k, s, sp);
        double log_z = 0.0;
        int dead = -1;
        exact_walk(a.tab + (int64_t)b * a.T_max * kBatchTab, a.mass + (int64_t)b * a.T_max * 8, 0, T, a.k, sp, s, p, 0.0, log_z, dead);
        if (lane == 0) { a.log_z[b] = log_z; a.dead[b] = dead; }
    }
}

// The resumed walk of an online batch (cpprob_hip_batch_advance_exact): batch_exact_kernel's arguments and the advance's first steps.
struct BatchExactAdvanceArgs {
    BatchExactArgs run;                        // prob: the lengths reached (never nullptr); log_z, dead: the carry, read and rewritten
    const int32_t* first;                      // [B]: the length before the advance; < 0 or >= T_b: the problem is idle
};

// Problem b's carry at step t0 > 0: m_{t0-1}[s] from the m table onto the lanes (s', s), log_z and dead from the evidence buffers.
__device__ __forceinline__ double exact_resume(const double* mass, const double* lz, const int32_t* dd, int b, int t0, int s, double& log_z, int& dead)
{
    log_z = lz[b];
    dead = exact_uniform(dd[b]);
    return mass[(int64_t)(t0 - 1) * 8 + s];
}

__global__ __launch_bounds__(kThreads) void batch_exact_advance_kernel(BatchExactAdvanceArgs aa)
{
#pragma clang fp contract(off)
    const BatchExactArgs& a = aa.run;
    const int lane = lane_id(), sp = lane >> 3, s = lane & 7;
    for (int b = exact_uniform((int)blockIdx.x * kWaves + wave_id()); b < a.B; b += (int)gridDim.x * kWaves) {   // (wavefront-uniform)
        const int T = (int)a.prob[b].T, t0 = exact_uniform(aa.first[b]);
        if (t0 < 0 || t0 >= T) continue;                        // idle: nothing of it is read or written
        double* mass = a.mass + (int64_t)b * a.T_max * 8;
        double log_z = 0.0, ms = 0.0;
        int dead = -1;
        if (t0 > 0) ms = exact_resume(mass, a.log_z, a.dead, b, t0, s, log_z, dead);
        if (dead >= 0) {                                        // dead before this advance: zeros, the carry stays
            for (int tt = t0; tt < T; ++tt) if (sp == 0) mass[(int64_t)tt * 8 + s] = 0.0;
            continue;
        }
        const double p = smooth_trans_mass(a.thr + (int64_t)b * a.thr_stride, a.k, s, sp);
        exact_walk(a.tab + (int64_t)b * a.T_max * kBatchTab, mass, t0, T, a.k, sp, s, p, ms, log_z, dead);
        if (lane == 0) { a.log_z[b] = log_z; a.dead[b] = dead; }
    }
}

}  // namespace cph
