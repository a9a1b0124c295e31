// The learning advance of an exact stream in one launch (cpprob_hip_batch_advance_learn_exact*): what a learning advance enqueues as
// three kernels -- the rows kernel (csrc/batch_learn.hpp), the run, the learn kernel -- done by the problem's own wavefront, one after
// the other.  All three share one layout: one wavefront a problem, kWaves problems a workgroup, the problems gridDim.x * kWaves apart,
// 8 x 8 lanes; at one observe a stream the launches are the cost, not the arithmetic.  batch_exact_learn_kernel serves a batch of unit
// scales, batch_exact_learn_scaled_kernel a batch with per-state emission scales: one body, exact_learn_body<kScaled>.
//
// For problem b, the steps t in [first[b], T_b) (first[b] < 0 or >= T_b: phases (i) and (ii) read and write nothing of it):
//   (i)   Rows.  Lane (., c) forms entry c of row t exactly as batch_learn_rows_body forms it -- retable_entry(y_t, mean_b[c], log_norm),
//         kScaled: scale_entry on the resident mean, sigma and log_norm of state c; -inf for c >= k -- from the tables in force.  Eight
//         shuffles hand the entries to every lane (the step wants the row uniform), a ninth the entry of the lane's state s'; the lanes
//         (0, c) store the row, because cpprob_hip_batch_predictive, the decode and cpprob_hip_batch_copy_step_tables read tab.  Row
//         t + 1's entries are formed before step t's arithmetic: they hang off the walk's chain.
//   (ii)  Walk.  exact_step of csrc/batch_exact.hpp on those rows, from the carry batch_exact_advance_kernel resumes from (row
//         first[b] - 1 of the m table, the evidence buffers); the m rows, log_z and dead are stored as that kernel stores them.  A dead
//         problem stores zeros in its m rows and goes on writing its rows of tab.
//   (iii) Learn.  batch_learn_body of csrc/batch_learn.hpp: (i) and (ii) are the `before` it runs ahead of the statement, so the push,
//         the record, the M-step, the checks, the table and the threshold words are that text, in its arithmetic and its order.
// The transition masses p of (ii) and of (iii) are read from the threshold words before (iii)(c) rewrites them: (ii) ends before
// (iii) begins, and (iii) reads p at its start, as the learn kernel does.  The means (and sigmas, log_norms) of (i) are those in force
// before (iii)(c) for the same reason.
//
// The hand-over from (ii) to (iii).  (iii) reads rows of the m table that other lanes of the same wavefront stored in (ii) (the lanes
// (0, s) store a row, every lane loads all of it).  The rows go through memory, with a workgroup-scope fence, __threadfence_block(),
// between the phases; registers would have to hold dT rows, and dT is not bounded.  The fence is enough on gfx950: the lanes of a
// wavefront are in one workgroup, so a workgroup-scope release/acquire pair orders the stores before the loads; a workgroup runs on
// one compute unit and its vector loads and stores go through that unit's one vector L1 in issue order, so the fence costs a wait for
// the outstanding stores (s_waitcnt vmcnt(0)) and no cache write-back or invalidate.  It also keeps the compiler from moving a load of
// (iii) above a store of (ii).  The loads must be vector loads: the scalar cache is not coherent with vector stores.  They are, since
// the compiler selects scalar loads only for memory that no store of the kernel may alias, and the m table is stored through `mass`
// in this kernel (the arguments carry no __restrict__).  The rows of tab do not need the fence: (ii) takes them from registers.
// No LDS, no barrier, no atomics, nothing contracted, no result that depends on the grid.
#pragma once
#include "batch_exact.hpp"
#include "batch_learn.hpp"

namespace cph {

struct BatchExactLearnArgs {                   // (what the fused advance needs beside the learn kernel's arguments)
    const int32_t* first;                      // [B]: the length before the advance; < 0 or >= T_b: the problem is idle
    double* tab;                               // [B][T_max][kBatchTab]
    double* mass;                              // [B][T_max][8], the m table of the workspace: the learner's `mass` is the same memory
    double* log_z;                             // [B], the carry
    int32_t* dead;                             // [B], the carry
    double log_norm;                           // log(2 pi 1 1), from the host (unit scales)
    int T_max;
};

// Phases (i) and (ii) for problem b.  la: the learner's arguments (desc: T_b and the problem's first new observe; thr, obs, means, k);
// sigmas, log_norms: kScaled: the resident scales [B][8], else not read.
template <bool kScaled>
__device__ __forceinline__ void exact_learn_walk(const BatchLearnArgs& la, const BatchExactLearnArgs& x, const double* sigmas, const double* log_norms, int b)
{
#pragma clang fp contract(off)
    const int lane = lane_id(), sp = lane >> 3, s = lane & 7, k = la.k;
    const int T = la.desc[b].T, t0 = exact_uniform(x.first[b]);
    if (t0 < 0 || t0 >= T) return;                              // idle (wavefront-uniform)
    const double mean = s < k ? la.means[(int64_t)b * k + s] : 0.0;
    double sigma = 1.0, log_norm = x.log_norm;
    if constexpr (kScaled) { sigma = s < k ? sigmas[(int64_t)b * 8 + s] : 1.0; log_norm = s < k ? log_norms[(int64_t)b * 8 + s] : 0.0; }
    const double* y = la.obs + la.desc[b].trows - t0;           // (indexed by the absolute step: y[t], t in [t0, T))
    double* tab = x.tab + (int64_t)b * x.T_max * kBatchTab;
    double* mass = x.mass + (int64_t)b * x.T_max * 8;
    auto entry = [&](int t) { return s < k ? (kScaled ? scale_entry(y[t], mean, sigma, log_norm) : retable_entry(y[t], mean, log_norm)) : -INFINITY; };
    double log_z = 0.0, ms = 0.0;
    int dead = -1;
    if (t0 > 0) ms = exact_resume(mass, x.log_z, x.dead, b, t0, s, log_z, dead);
    const bool was_dead = dead >= 0;
    const double p = smooth_trans_mass(la.thr + (int64_t)b * 64, k, s, sp);
    double e = entry(t0);
    for (int t = t0; t < T; ++t) {
        const double ec = e;
        e = entry(t + 1 < T ? t + 1 : t);                       // (the last step forms its own row again: in bounds, never used)
        if (sp == 0) tab[(int64_t)t * kBatchTab + s] = ec;
        double lc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) lc[j] = __shfl(ec, j);
        const double lc_sp = __shfl(ec, sp);
        if (dead < 0 && !exact_step(t, k, sp, s, p, lc, lc_sp, ms, log_z, mass + (int64_t)t * 8)) { dead = t; log_z = -INFINITY; }
        if (dead >= 0 && sp == 0) mass[(int64_t)t * 8 + s] = 0.0;      // (wavefront-uniform: zeros from the dead step on)
    }
    if (lane == 0 && !was_dead) { x.log_z[b] = log_z; x.dead[b] = dead; }
    __threadfence_block();                                      // (iii) loads the m rows other lanes of this wavefront stored
}

// Args: BatchLearnArgs, or kScaled: BatchLearnScaledArgs
template <bool kScaled, class Args>
__device__ __forceinline__ void exact_learn_body(Args sa, BatchExactLearnArgs x)
{
#pragma clang fp contract(off)
    BatchLearnArgs la;
    const double *sigmas = nullptr, *log_norms = nullptr;
    if constexpr (kScaled) { la = sa.base; sigmas = sa.sigmas; log_norms = sa.log_norms; } else la = sa;
    batch_learn_body<kScaled>(sa, [&](int b) { exact_learn_walk<kScaled>(la, x, sigmas, log_norms, b); });
}

__global__ __launch_bounds__(kThreads) void batch_exact_learn_kernel(BatchLearnArgs a, BatchExactLearnArgs x)
{
#pragma clang fp contract(off)
    exact_learn_body<false>(a, x);
}

__global__ __launch_bounds__(kThreads) void batch_exact_learn_scaled_kernel(BatchLearnScaledArgs sa, BatchExactLearnArgs x)
{
#pragma clang fp contract(off)
    exact_learn_body<true>(sa, x);
}

}  // namespace cph
