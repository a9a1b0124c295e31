// Trajectory sufficient statistics of a batch (cpprob_hip_batch_traj_stats, _traj_stats_device): the complete-data statistics of every
// backward-simulated trajectory, counted while the trajectory is drawn.  Trajectory j of problem b under draw_index IS column j of
// cpprob_hip_batch_smooth's trajectories for that draw_index -- batch_smooth_kernel's start rule, its smooth_pick, its Philox block
// draw_block(seed_b, j >> 1, 2^41 + (draw_index << 24) + t) and word pair j & 1 -- and does not depend on n_traj; it is never stored.
//
// Per trajectory x_0 .. x_{T-1} (T the length reached, y_t the observes), walking t = T-1 .. 0:
//   xi[s][s'] = #{t < T-1 : x_t = s, x_{t+1} = s'}       occ[s] = #{t : x_t = s}
//   occ_y[x_t] = occ_y[x_t] + y_t                        occ_yy[x_t] = occ_yy[x_t] + dmul_rn(y_t, y_t)
// Every accumulator starts at 0.0 and takes one IEEE addition a step it is visited, in walk order; nothing is contracted.  The counts
// are integers (below 2^24) written as doubles.  The record is batch_smooth_stats_kernel's: 88 doubles, xi at 8 s + s', then occ[8],
// occ_y[8], occ_yy[8]; states >= k are zero, a problem of length 0 is all zero, T = 1 has xi = 0.  Output [B][n_traj][88].
// tests/trajstats_ref.py restates it.
//
// blockIdx.x the problem, blockIdx.y a tile of kTrajStatsTile = kThreads trajectories, a lane a trajectory.  P is staged in LDS and,
// where 64 T bytes fit the launch's dynamic LDS, the m table, as batch_smooth_kernel stages them; the row and the observe of step
// t - 1 are loaded before step t's arithmetic (they do not depend on the state).  The lane keeps K * K 32-bit transition counters and
// 2 K doubles in registers and updates them with a statically unrolled compare-and-add: no register array is indexed by the state, so
// nothing goes to scratch memory.  occ is the row sums of xi plus the last state.  One barrier (after the staging), no atomics, no
// result that depends on the grid; a lane past n_traj walks along and stores nothing.
#pragma once
#include "batch_smooth.hpp"

namespace cph {

constexpr int kTrajStats = 88;                      // doubles a trajectory: xi[8][8], occ[8], occ_y[8], occ_yy[8] (kSuffStats' layout)
constexpr int kTrajStatsTile = kThreads;            // trajectories a workgroup

struct BatchTrajStatsArgs {
    const BatchSmoothProblem* desc;            // [B]: T, rows (first row in the m table) and trows (first observe: the lengths before it)
    const double* mass;                        // the m table the counting pass left
    const uint64_t* thr;                       // as BatchSmoothArgs::thr
    const uint64_t* seeds;                     // [B]
    const double* obs;                         // the observes packed problem after problem by the lengths reached; nullptr: occ_y, occ_yy stay 0
    double* stats;                             // [B][n_traj][kTrajStats]
    uint64_t draw_base;                        // kBackwardDrawBase + (draw_index << 24)
    int k, thr_stride, n_traj, lds_bytes;
};

// K: the states walked a step (3: CPPROB_HIP_MODEL_HMM3; 8: CPPROB_HIP_MODEL_HMM_TABLE, states >= k carry no mass)
template <int K>
__global__ __launch_bounds__(kThreads) void batch_traj_stats_kernel(BatchTrajStatsArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double s_tmass[];   // [T][8] where it fits
    __shared__ double s_pt[64];                                         // s_pt[8 s' + s] = double(P[s][s'])
    const int b = (int)blockIdx.x, tid = threadIdx.x;
    const BatchSmoothProblem d = a.desc[b];                     // workgroup-uniform
    const int j = (int)blockIdx.y * kTrajStatsTile + tid;       // (gridDim.y tiles cover n_traj: a lane past it is in the last tile)
    double* out = a.stats + ((int64_t)b * a.n_traj + j) * kTrajStats;
    const int T = d.T;
    if (T <= 0) {                                               // nothing reached yet: the zero record
        if (j < a.n_traj) for (int i = 0; i < kTrajStats; ++i) out[i] = 0.0;
        return;
    }
    const double* mass = a.mass + d.rows * 8;
    if (tid < 64) s_pt[tid] = smooth_trans_mass(a.thr + (int64_t)b * a.thr_stride, a.k, tid & 7, tid >> 3);
    const bool staged = (int64_t)T * 64 <= (int64_t)a.lds_bytes;
    if (staged) for (int i = tid; i < T * 8; i += kThreads) s_tmass[i] = mass[i];
    __syncthreads();
    const double* y = a.obs ? a.obs + d.trows : nullptr;
    const uint64_t seed = a.seeds[b];
    uint32_t cnt[K * K];                                        // cnt[K s + s']
    double sy[K], syy[K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) cnt[i] = 0u;
#pragma unroll
    for (int s = 0; s < K; ++s) { sy[s] = 0.0; syy[s] = 0.0; }
    double m[K];
    if (staged) {
#pragma unroll
        for (int s = 0; s < K; ++s) m[s] = s_tmass[(T - 1) * 8 + s];
    } else {
#pragma unroll
        for (int s = 0; s < K; ++s) m[s] = mass[(int64_t)(T - 1) * 8 + s];
    }
    double yt = y ? y[T - 1] : 0.0;
    int x = 0, x_last = 0;
    for (int t = T - 1; t >= 0; --t) {
        double mc[K];
#pragma unroll
        for (int s = 0; s < K; ++s) mc[s] = m[s];
        const double yc = yt;
        const int tn = t > 0 ? t - 1 : 0;                       // (step 0 loads its own row again: in bounds, never used)
        if (staged) {
#pragma unroll
            for (int s = 0; s < K; ++s) m[s] = s_tmass[tn * 8 + s];
        } else {
#pragma unroll
            for (int s = 0; s < K; ++s) m[s] = mass[(int64_t)tn * 8 + s];
        }
        yt = y ? y[tn] : 0.0;
        const u32x4 r = draw_block(seed, (uint64_t)(j >> 1), a.draw_base + (uint64_t)t);
        const double u = (j & 1) ? u01_53(r.z, r.w) : u01_53(r.x, r.y);
        double w[K];
        double D = 0.0;
#pragma unroll
        for (int s = 0; s < K; ++s) { w[s] = t == T - 1 ? mc[s] : dmul_rn(mc[s], s_pt[x * 8 + s]); D = D + w[s]; }
        if (D == 0.0) {
#pragma unroll
            for (int s = 0; s < K; ++s) w[s] = mc[s];
        }
        const int xn = x;                                       // x_{t+1}
        x = smooth_pick<K>(w, u);
        const int pair = t == T - 1 ? -1 : x * K + xn;          // (the last step opens no transition)
        x_last = t == T - 1 ? x : x_last;
#pragma unroll
        for (int i = 0; i < K * K; ++i) cnt[i] += pair == i ? 1u : 0u;
        const double yy = dmul_rn(yc, yc);
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const double ny = sy[s] + yc, nyy = syy[s] + yy;
            sy[s] = x == s ? ny : sy[s];
            syy[s] = x == s ? nyy : syy[s];
        }
    }
    if (j >= a.n_traj) return;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        uint32_t row = 0u;
#pragma unroll
        for (int sn = 0; sn < 8; ++sn) {
            const uint32_t c = s < K && sn < K ? cnt[(s < K ? s : 0) * K + (sn < K ? sn : 0)] : 0u;
            row += c;
            out[8 * s + sn] = (double)c;
        }
        out[64 + s] = (double)(row + (x_last == s ? 1u : 0u));
        out[72 + s] = s < K ? sy[s < K ? s : 0] : 0.0;
        out[80 + s] = s < K ? syy[s < K ? s : 0] : 0.0;
    }
}

}  // namespace cph
