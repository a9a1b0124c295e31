// Forecasts of a batch (cpprob_hip_batch_forecast, _forecast_device, cpprob_hip_batch_predictive, _predictive_device): what lies ahead
// of the last observe, from the backward smoother's m table (csrc/batch_smooth.hpp) and the transition law the device itself draws
// from -- the 32-bit threshold words, whose integer differences P[s][s'] smooth_trans_mass returns.
//
// The arithmetic, per problem (L = the length reached, k its states, m_t[0..8) its rows of the m table, c[s][.] its threshold words;
// DESIGN.md section 5 states it once more):
//   P[s][s']      = c[s][s'] - c[s][s'-1] (smooth_trans_mass);  p[s][s'] = double(P[s][s']) * 2^-32, exact: a scaling by a power of two
//   push(f)[s']   = sum over s = 0..k-1, in that order, of dmul_rn(f[s], p[s][s']); the sum starts from 0.0 and leaves out the terms
//                   with f[s] == 0
//   marginals       f_0 = smooth_marginal_start(m_{L-1}), the smoother's own last row from the same device function;
//                   f_h = push(f_{h-1}), h = 1 .. H; the output rows are h = 1 .. H; a problem of length 0 gets zero rows
//   predictive rows r_0[s] = 1.0 / double(k) for s < k (the uniform initial state: no row of the table is read);
//                   r_t = push(smooth_marginal_start(m_{t-1})) for 1 <= t <= L.  r_L is f_1 bit for bit (the same function walks
//                   both); r_t reads row t - 1 alone: final when first available, the same however an online batch was cut
//   futures         trajectory j.  Row 0, the present state, is drawn from m_{L-1} by the backward simulation's start rule: running
//                   sums in the order s = 0..k-1, target = u * c_{k-1}, the first s with c_s > target, else the last s with positive
//                   weight; u = the 53-bit uniform of word pair j & 1 of Philox block draw_block(seed_b, j >> 1,
//                   2^42 + (draw_index << 24) + 0).  Row h >= 1: w = 32-bit word 2 (j & 1) of block draw_block(seed_b, j >> 1,
//                   2^42 + (draw_index << 24) + h), x_h = #{i < k-1 : w >= c[x_{h-1}][i]} -- the statement of ModelHmmK::apply4, so
//                   the simulated law is exactly P.  A problem of length 0 owns rows of zeros.
// No product is contracted into a neighbouring sum (fp contract off in every function of this file; products through dmul_rn): the
// rows are a pure function of integers and IEEE operations, and tests/forecast_ref.py restates them bit for bit.
//
// batch_forecast_kernel: blockIdx.x the problem; row blockIdx.y = 0 its H marginal rows on ONE wavefront (lane (s', s) = 8 s' + s
// holds p[s][s']; the ordered sums gather their terms with wavefront shuffles, as smooth_marginals does); rows blockIdx.y >= 1 are
// tiles of kTile trajectories: the problem's threshold words staged in static LDS, a lane owning trajectories tid, tid + 256, ... of
// its tile and walking h upwards, one Philox block a step and pair of trajectories, consecutive lanes writing consecutive bytes of
// output row h.  No dynamic LDS, no atomics, no barrier after the staging.  batch_predictive_kernel: work items (problem, step) on a
// two-dimensional grid, a wavefront an item, the items gridDim.y * kWaves apart where a problem owes more rows than the grid holds
// (batch_smooth_lag_kernel's striding).  The items are independent: no barrier, no atomics, no result that depends on the grid.
#pragma once
#include "batch_smooth.hpp"

namespace cph {

constexpr int kForecastMaxH = 1 << 24;              // horizon < this: h sits below draw_index << 24 in the draw ordinal
// Ordinals in [2^42, 2^43) are the forecast's own: the particles' statements use the step index, the resampling draws 2^40 plus up
// to 2^39 (kResampleDrawBase), the backward smoother [2^41, 2^42) (kBackwardDrawBase).
constexpr uint64_t kForecastDrawBase = 1ull << 42;
constexpr int kPredictiveGridMax = 4096;            // gridDim.y of batch_predictive_kernel at most: kWaves times it items a problem and trip

struct BatchForecastArgs {
    const BatchSmoothProblem* desc;            // [B]: T, rows (first row in the m table) and mfrom (the first predictive row wanted)
    const double* mass;                        // the m table
    const uint64_t* thr;                       // as BatchSmoothArgs::thr
    const uint64_t* seeds;                     // [B]
    double* marg;                              // [B][rows][spp], zeroed by the caller; nullptr: not wanted
    int8_t* traj;                              // [B][H + 1][n_traj]; nullptr: not wanted
    uint64_t draw_base;                        // kForecastDrawBase + (draw_index << 24)
    int k, spp, thr_stride, n_traj;
    int H, rows;                               // the horizon; rows a problem in marg (H: the forecast, n_rows: the predictive rows)
};

// p[s][s'] of the threshold rows `thr`: the integer mass scaled by 2^-32 (exact); 0 outside the k x k table
__device__ __forceinline__ double forecast_trans_prob(const uint64_t* thr, int k, int s, int sn)
{
#pragma clang fp contract(off)
    return dmul_rn(smooth_trans_mass(thr, k, s, sn), 0x1p-32);
}

// One step on one wavefront, lane (s', s) = 8 s' + s: f holds f[s] (the same in the eight lanes (., s)), p = p[s][s']; returns
// push(f)[s], the same in the eight lanes (., s).  The term of lane (s', s) is f[s] p[s][s']; the lanes (s, 0..7) hold the terms of
// push(f)[s] in the order of the sum.
__device__ __forceinline__ double forecast_push(double f, double p, int s)
{
#pragma clang fp contract(off)
    const double term = f != 0.0 ? dmul_rn(f, p) : 0.0;          // (a term left out and a zero added are the same sum)
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = acc + __shfl(term, s * 8 + j);
    return acc;
}

// Predictive rows: blockIdx.x the problem; item blockIdx.y * kWaves + wavefront (and the items gridDim.y * kWaves apart) is step
// t = mfrom + item <= T, output row `item`.
__global__ __launch_bounds__(kThreads) void batch_predictive_kernel(BatchForecastArgs a)
{
#pragma clang fp contract(off)
    const int b = (int)blockIdx.x, lane = lane_id(), sp = lane >> 3, s = lane & 7;
    const BatchSmoothProblem d = a.desc[b];                     // workgroup-uniform
    const int items = d.mfrom > d.T ? 0 : d.T + 1 - d.mfrom;
    const double* mass = a.mass + d.rows * 8;
    const double p = forecast_trans_prob(a.thr + (int64_t)b * a.thr_stride, a.k, s, sp);
    double* out = a.marg + (int64_t)b * a.rows * a.spp;
    const bool put = sp == 0 && s < a.spp;
    for (int item = (int)blockIdx.y * kWaves + wave_id(); item < items; item += (int)gridDim.y * kWaves) {   // (wavefront-uniform)
        const int t = d.mfrom + item;
        double r;
        if (t == 0) r = s < a.k ? 1.0 / (double)a.k : 0.0;
        else r = forecast_push(smooth_marginal_start(mass + (int64_t)(t - 1) * 8, s), p, s);
        if (put) out[(int64_t)item * a.spp + s] = r;
    }
}

// K: the states walked at row 0 (3: CPPROB_HIP_MODEL_HMM3; 8: CPPROB_HIP_MODEL_HMM_TABLE, states >= k carry no mass)
template <int K>
__global__ __launch_bounds__(kThreads) void batch_forecast_kernel(BatchForecastArgs a)
{
#pragma clang fp contract(off)
    __shared__ uint64_t s_thr[64];                              // the problem's threshold rows [k][8]
    const int b = (int)blockIdx.x, tid = threadIdx.x;
    const BatchSmoothProblem d = a.desc[b];                     // workgroup-uniform
    const uint64_t* thr = a.thr + (int64_t)b * a.thr_stride;
    if (blockIdx.y == 0) {
        if (!a.marg || d.T <= 0 || tid >= kWave) return;        // (a problem of length 0: its rows stay zero)
        const int lane = lane_id(), sp = lane >> 3, s = lane & 7;
        const double p = forecast_trans_prob(thr, a.k, s, sp);
        double* out = a.marg + (int64_t)b * a.rows * a.spp;
        double f = smooth_marginal_start(a.mass + (d.rows + (int64_t)(d.T - 1)) * 8, s);
        for (int h = 1; h <= a.H; ++h) {
            f = forecast_push(f, p, s);
            if (sp == 0 && s < a.spp) out[(int64_t)(h - 1) * a.spp + s] = f;
        }
        return;
    }
    const int i0 = ((int)blockIdx.y - 1) * kTile;
    if (!a.traj || i0 >= a.n_traj) return;                      // a tile past the trajectories asked for
    int8_t* out = a.traj + (int64_t)b * (a.H + 1) * a.n_traj;
    if (d.T <= 0) {                                             // nothing reached yet: rows of zeros
        for (int h = 0; h <= a.H; ++h) {
#pragma unroll
            for (int q = 0; q < kPPT; ++q) {
                const int j = i0 + q * kThreads + tid;
                if (j < a.n_traj) out[(int64_t)h * a.n_traj + j] = 0;
            }
        }
        return;
    }
    if (tid < 8 * a.k) s_thr[tid] = thr[tid];
    __syncthreads();
    const uint64_t seed = a.seeds[b];
    const double* row = a.mass + (d.rows + (int64_t)(d.T - 1)) * 8;
    double m[K];
#pragma unroll
    for (int s = 0; s < K; ++s) m[s] = row[s];
    int x[kPPT];
#pragma unroll
    for (int q = 0; q < kPPT; ++q) {                            // row 0: the present state
        const int j = i0 + q * kThreads + tid;                  // (a lane past n_traj walks along and stores nothing)
        const u32x4 r = draw_block(seed, (uint64_t)(j >> 1), a.draw_base);
        const double u = (j & 1) ? u01_53(r.z, r.w) : u01_53(r.x, r.y);
        x[q] = smooth_pick<K>(m, u);
        if (j < a.n_traj) out[j] = (int8_t)x[q];
    }
    for (int h = 1; h <= a.H; ++h) {
        int8_t* orow = out + (int64_t)h * a.n_traj;
#pragma unroll
        for (int q = 0; q < kPPT; ++q) {
            const int j = i0 + q * kThreads + tid;
            const u32x4 r = draw_block(seed, (uint64_t)(j >> 1), a.draw_base + (uint64_t)h);
            const uint64_t w = (j & 1) ? r.z : r.x;
            const uint64_t* c = s_thr + 8 * x[q];
            int v = 0;
#pragma unroll
            for (int i = 0; i < K - 1; ++i) v += i < a.k - 1 && w >= c[i] ? 1 : 0;
            x[q] = v;
            if (j < a.n_traj) orow[j] = (int8_t)v;
        }
    }
}

}  // namespace cph
