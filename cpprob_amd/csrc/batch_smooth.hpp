// Backward smoothing of a batch: forward filtering / backward smoothing and backward simulation over the store batch_smc_kernel left
// (cpprob_hip_batch_smooth, _smooth_device).  The lineage read-outs (batch_smc_kernel's own, batch_paths_kernel) rest the early steps on
// the few ancestors the final particles still share; here every generation's whole filtering approximation takes part.  The states are
// discrete (k <= 8) and, with resampling after every step, a particle's weight depends on its state alone, so generation t IS k numbers.
//
// The arithmetic, per problem (T = its current length, n its particles, k its states; DESIGN.md section 5 states it once more):
//   P[s][s']   = c[s][s'] - c[s][s'-1], c the problem's transition thresholds ceil(2^32 cumulative probability), c[s][-1] = 0 and
//                c[s][k-1] = 2^32: the law the forward draw realises on 32-bit words, as integers
//   m_t[s]     = cnt_t[s] * fix_weight(ll_t[s], M_t), cnt_t[s] = #{i : values[t][i] = s}, M_t = max{ll_t[s] : cnt_t[s] > 0}: an integer
//                below 2^45, exact as a double
//   a_t[s'][s] = double(m_t[s]) * double(P[s][s']) (one rounded product), D_t[s'] = sum over s = 0..k-1 in that order; a row whose D is 0
//                takes double(m_t[s]) instead (unreachable from a store a run wrote)
//   marginals    g_{T-1}[s] = double(m_{T-1}[s]) / double(sum_s m_{T-1}[s]);  g_t[s] = sum over s' = 0..k-1 of (a_t[s'][s] / D_t[s']) * g_{t+1}[s'],
//                terms with g_{t+1}[s'] = 0 left out
//   trajectory j for t = T-1 .. 0: w[s] = double(m_{T-1}[s]) at t = T-1, else row x_{t+1} of a_t (or its fallback); c_s the running sums in
//                the order s = 0..k-1; target = u * c_{k-1}; x_t = the first s with c_s > target, else the last s with w[s] > 0;
//                u = the 53-bit uniform of word pair j & 1 of Philox block draw_block(seed_b, j >> 1, 2^41 + (draw_index << 24) + t)
// No product is contracted into a neighbouring sum (fp contract off in every function of this file; products through dmul_rn): the
// trajectories are a pure function of integers and IEEE operations, and tests/backward_ref.py restates them bit for bit.
//
// Two launches.  batch_smooth_count_kernel: work items (problem, step) on a two-dimensional grid, a workgroup a step at a time --
// n state bytes, packed per-state wavefront sums (batch_smc_kernel's count phase), one workgroup reduction, 64 bytes out: m_t[0..8)
// into a table of the context's own (it is no part of the batch workspace).  batch_smooth_kernel: blockIdx.x the problem; row
// blockIdx.y = 0 is its marginals, O(T k^2), on ONE wavefront (lane (s', s) holds a_t[s'][s]; the ordered sums gather their terms with
// wavefront shuffles); rows blockIdx.y >= 1 are tiles of kTile trajectories.  A tile stages the problem's k x k masses P and, where
// 64 T bytes fit the launch's dynamic LDS, its m table; longer problems read m from global memory (L2-resident: every tile of the
// problem reads the same rows).  A lane owns trajectories tid, tid + 256, ... of its tile -- kPPT independent chains -- and walks t
// backwards: k products, k sums and one Philox block a step and trajectory; consecutive lanes write consecutive bytes of output row t.
//
// Fixed-lag smoothing (cpprob_hip_batch_smooth_lag, _smooth_lag_device) works on the same table.  G_t is the recursion above started
// from the filtering masses of the end step e(t) = min(t + lag, T - 1) instead of T - 1: final once lag more steps have run, and a
// function of rows t .. e(t) alone.  The counting pass takes a range of rows a problem ([cfrom, cto): an online batch's table is
// addressed by capacity, rows never move, and the host counts the rows that arrived since its last call); batch_smooth_lag_kernel's
// work items are (problem, end step), a wavefront each: the item of end e < T - 1 walks lag steps and writes G_{e - lag}, the item of
// end T - 1 writes every requested t >= T - 1 - lag in one walk.  Both it and smooth_marginals take their steps through
// smooth_marginal_start / smooth_marginal_term / smooth_marginal_sum, so the rows whose end is T - 1 are the full smoother's bits.  The trajectories stop at
// a lower step `lo` (the window's first step; 0 for the full call), stage rows lo .. T - 1 only, and keep the absolute step in the draw
// ordinal: a window row is the full call's row.
#pragma once
#include "batch_smc.hpp"

namespace cph {

constexpr int kBackwardMaxT = 1 << 24;              // steps a problem may have: t sits below draw_index << 24 in the draw ordinal
constexpr int kBackwardMaxTraj = 1 << 20;           // trajectories a problem in one call
constexpr int kBackwardMaxDraws = 1 << 16;          // draw_index < this: the ordinals stay inside [2^41, 2^42)
constexpr uint64_t kBackwardDrawBase = 1ull << 41;  // clear of the particles' statement ordinals and of the resampling draws at 2^40 + ...
constexpr int kBackwardLdsMax = 32768;              // bytes of m table a tile stages: T <= 512
constexpr int kSmoothCountGroups = 8192;            // workgroups the counting pass aims at: gridDim.y = min(rows owed, max(8, ceil(this / B)))
constexpr int kSmoothLagGridMax = 4096;             // gridDim.y of batch_smooth_lag_kernel at most: kWaves times it items a problem and trip

// Problem b as the passes need it: its length, particles, first entry in the store, its first row in the m table (the rows of the
// problems before it, or their capacities: an online batch), its first row of trajectory output (n_traj times that is its first
// entry), the rows [cfrom, cto) the counting pass owes, the step the trajectories stop at and the first step whose fixed-lag marginal
// is wanted (output row 0).
struct BatchSmoothProblem { int32_t T, n; int64_t store, rows, trows; int32_t cfrom, cto, lo, mfrom; };
static_assert(sizeof(BatchSmoothProblem) == 48, "one problem's smoothing descriptor");

struct BatchSmoothArgs {
    const BatchSmoothProblem* desc;            // [B]
    const int8_t* values;                      // the batch's particle store
    const double* tab;                         // [B][T_max][kBatchTab]
    const uint64_t* thr;                       // problem b's 64 threshold words at thr + b * thr_stride, the layout of ModelParams::hk_thr
    const uint64_t* seeds;                     // [B]
    double* mass;                              // [sum of T_b][8]: m_t[0..8) of row desc[b].rows + t
    double* marg;                              // [B][marg_rows][spp], zeroed by the caller; nullptr: not wanted
    int8_t* traj;                              // packed: problem b's [T_b - lo_b][n_traj] from n_traj * desc[b].trows on; nullptr: not wanted
    uint64_t draw_base;                        // kBackwardDrawBase + (draw_index << 24)
    int T_max, k, spp, thr_stride, n_traj, lds_bytes;
    int marg_rows, lag;                        // rows a problem in marg (T_max: the full call); batch_smooth_lag_kernel's lag
};

__global__ __launch_bounds__(kThreads) void batch_smooth_count_kernel(BatchSmoothArgs a)
{
    __shared__ uint64_t s_cnt[2][kWaves][2];                    // per-wavefront packed state counts (16 bits a state), by round parity
    const int b = (int)blockIdx.x, tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    const BatchSmoothProblem d = a.desc[b];                     // workgroup-uniform
    const int8_t* vals = a.values + d.store;
    int round = 0;
    for (int t = d.cfrom + (int)blockIdx.y; t < d.cto; t += (int)gridDim.y, ++round) {   // (an empty range: the workgroup returns at once)
        const int8_t* row = vals + (int64_t)t * d.n;
        uint64_t cA = 0, cB = 0;
        for (int i = tid; i < d.n; i += kThreads) {             // (byte loads: a row starts where the rows before it end)
            const int s = row[i] & 7;
            cA += s < 4 ? 1ull << (16 * s) : 0ull;
            cB += s >= 4 ? 1ull << (16 * (s - 4)) : 0ull;
        }
        cA = wave_sum_u64(cA);
        cB = wave_sum_u64(cB);
        if (lane == 0) { s_cnt[round & 1][wv][0] = cA; s_cnt[round & 1][wv][1] = cB; }
        __syncthreads();                                        // (one barrier a round: round + 2 writes this parity again, past round + 1's barrier)
        if (tid < 8) {
            uint64_t tA = 0, tB = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) { tA += s_cnt[round & 1][w][0]; tB += s_cnt[round & 1][w][1]; }
            const double* ll = a.tab + ((int64_t)b * a.T_max + t) * kBatchTab;
            double M = -INFINITY;
            uint32_t mine = 0;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const uint32_t c = (uint32_t)((s < 4 ? tA : tB) >> (16 * (s & 3))) & 0xffffu;
                if (s < a.k && c) M = fmax(M, ll[s]);
                mine = s == tid ? c : mine;
            }
            const uint32_t q = tid < a.k ? fix_weight(ll[tid], M) : 0u;
            a.mass[(d.rows + t) * 8 + tid] = u64_to_double((uint64_t)mine * q);
        }
    }
}

// P[s][s'] of the threshold rows `thr` ([k][8], entries 0..k-2 of a row), as a double; 0 outside the k x k table
__device__ __forceinline__ double smooth_trans_mass(const uint64_t* thr, int k, int s, int sn)
{
    if (s >= k || sn >= k) return 0.0;
    const uint64_t hi = sn == k - 1 ? 1ull << 32 : thr[s * 8 + sn];
    const uint64_t lo = sn == 0 ? 0ull : thr[s * 8 + sn - 1];
    return u64_to_double(hi - lo);
}

// The recursion's start on one wavefront, lane (s', s) = 8 s' + s: g_e[s] of the filtering masses m_fin of the end step, the same in
// the eight lanes (., s).
__device__ __forceinline__ double smooth_marginal_start(const double* m_fin, int s)
{
#pragma clang fp contract(off)
    uint64_t tot = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) tot += (uint64_t)m_fin[j];
    return m_fin[s] / u64_to_double(tot);
}

// One step of it in two parts, the one statement of the step: the full-length marginals, the fixed-lag kernel and the sufficient
// statistics (csrc/batch_suffstats.hpp) all walk through here.  The term of lane (s', s): (a_t[s'][s] / D_t[s']) g_{t+1}[s'], the
// two-slice posterior P(x_t = s, x_{t+1} = s' | y), from g_{t+1} (in g), mt = m_t[s], the step's masses m = m_t[0..8) (their ordered
// sum serves the defensive rule) and p = double(P[s][s']).
__device__ __forceinline__ double smooth_marginal_term(double mt, const double (&m)[8], double p, double g, int sp)
{
#pragma clang fp contract(off)
    const double av = dmul_rn(mt, p);
    double D = 0.0, Dm = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { D = D + __shfl(av, sp * 8 + j); Dm = Dm + m[j]; }
    const bool none = D == 0.0;                                 // (the defensive rule: the row falls back to the filtering masses)
    const double num = none ? mt : av, den = none ? Dm : D;
    const double g_sp = __shfl(g, sp);                          // lane (0, s') holds g_{t+1}[s']
    return g_sp != 0.0 ? dmul_rn(num / den, g_sp) : 0.0;        // (a term left out and a zero added are the same sum)
}

// g_t[s]: the terms of the lanes (., s) summed in the order s' = 0..7, the same in the eight lanes (., s).
__device__ __forceinline__ double smooth_marginal_sum(double term, int s)
{
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = acc + __shfl(term, j * 8 + s);
    return acc;
}

// Row `row` = m_t[0..8) of the m table as the pair takes it: the lane's own mass returned, the eight in m.
__device__ __forceinline__ double smooth_load_row(const double* row, int s, double (&m)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = row[j];
    return row[s];
}

// The marginals of one problem on one wavefront.
__device__ __forceinline__ void smooth_marginals(const BatchSmoothArgs& a, int b, int T, const double* mass, const uint64_t* thr)
{
#pragma clang fp contract(off)
    const int lane = lane_id(), sp = lane >> 3, s = lane & 7;
    const double p = smooth_trans_mass(thr, a.k, s, sp);
    double* out = a.marg + (int64_t)b * a.marg_rows * a.spp;
    double g = smooth_marginal_start(mass + (int64_t)(T - 1) * 8, s);
    if (sp == 0 && s < a.spp) out[(int64_t)(T - 1) * a.spp + s] = g;
    for (int t = T - 2; t >= 0; --t) {
        double m[8];
        const double mt = smooth_load_row(mass + (int64_t)t * 8, s, m);
        g = smooth_marginal_sum(smooth_marginal_term(mt, m, p, g, sp), s);
        if (sp == 0 && s < a.spp) out[(int64_t)t * a.spp + s] = g;
    }
}

// Fixed-lag marginals: blockIdx.x the problem; item blockIdx.y * kWaves + wavefront (and the items gridDim.y * kWaves apart) has the
// end step T - 1 - item.  Output row t - mfrom.  The items are independent: no barrier, no atomics, no result that depends on the grid.
__global__ __launch_bounds__(kThreads) void batch_smooth_lag_kernel(BatchSmoothArgs a)
{
#pragma clang fp contract(off)
    const int b = (int)blockIdx.x, lane = lane_id(), sp = lane >> 3, s = lane & 7;
    const BatchSmoothProblem d = a.desc[b];                     // workgroup-uniform
    // the ends that own a row: T - 1 (every t >= T - 1 - lag asked for) and mfrom + lag .. T - 2 (t = end - lag)
    const int items = d.mfrom >= d.T ? 0 : (d.T - d.mfrom - a.lag > 1 ? d.T - d.mfrom - a.lag : 1);
    const double* mass = a.mass + d.rows * 8;
    const double p = smooth_trans_mass(a.thr + (int64_t)b * a.thr_stride, a.k, s, sp);
    double* out = a.marg + ((int64_t)b * a.marg_rows - d.mfrom) * a.spp;
    const bool put = sp == 0 && s < a.spp;
    for (int item = (int)blockIdx.y * kWaves + wave_id(); item < items; item += (int)gridDim.y * kWaves) {   // (wavefront-uniform)
        const int e = d.T - 1 - item;
        const int first = e - a.lag > d.mfrom ? e - a.lag : d.mfrom;   // the step the walk ends at
        double g = smooth_marginal_start(mass + (int64_t)e * 8, s);
        if (put && (item == 0 || e == first)) out[(int64_t)e * a.spp + s] = g;
        for (int t = e - 1; t >= first; --t) {
            double m[8];
            const double mt = smooth_load_row(mass + (int64_t)t * 8, s, m);
            g = smooth_marginal_sum(smooth_marginal_term(mt, m, p, g, sp), s);
            if (put && (item == 0 || t == first)) out[(int64_t)t * a.spp + s] = g;
        }
    }
}

// One backward draw: the first s whose running sum exceeds u times the total, else the last s with mass.
template <int K>
__device__ __forceinline__ int smooth_pick(const double (&w)[K], double u)
{
#pragma clang fp contract(off)
    double c[K];
    double run = 0.0;
#pragma unroll
    for (int s = 0; s < K; ++s) { run = run + w[s]; c[s] = run; }
    const double target = dmul_rn(u, run);
    int x = -1, last = 0;
#pragma unroll
    for (int s = K - 1; s >= 0; --s) x = c[s] > target ? s : x;
#pragma unroll
    for (int s = 0; s < K; ++s) last = w[s] > 0.0 ? s : last;
    return x < 0 ? last : x;
}

// K: the states walked a step (3: CPPROB_HIP_MODEL_HMM3; 8: CPPROB_HIP_MODEL_HMM_TABLE, states >= k carry no mass)
template <int K>
__global__ __launch_bounds__(kThreads) void batch_smooth_kernel(BatchSmoothArgs a)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double s_mass[];    // [T - lo][8] where it fits
    __shared__ double s_pt[64];                                         // s_pt[8 s' + s] = double(P[s][s'])
    const int b = (int)blockIdx.x, tid = threadIdx.x;
    const BatchSmoothProblem d = a.desc[b];                     // workgroup-uniform
    if (d.T <= 0) return;                                       // nothing reached yet
    const double* mass = a.mass + d.rows * 8;
    const uint64_t* thr = a.thr + (int64_t)b * a.thr_stride;
    if (blockIdx.y == 0) {
        if (a.marg && tid < kWave) smooth_marginals(a, b, d.T, mass, thr);
        return;
    }
    const int i0 = ((int)blockIdx.y - 1) * kTile;
    if (!a.traj || i0 >= a.n_traj) return;                      // a tile past the trajectories asked for
    if (tid < 64) s_pt[tid] = smooth_trans_mass(thr, a.k, tid & 7, tid >> 3);
    const int lo = d.lo;                                        // the first step walked: output row 0
    const bool staged = (int64_t)(d.T - lo) * 64 <= (int64_t)a.lds_bytes;
    if (staged) for (int i = tid; i < (d.T - lo) * 8; i += kThreads) s_mass[i] = mass[(int64_t)lo * 8 + i];
    __syncthreads();
    const uint64_t seed = a.seeds[b];
    int8_t* out = a.traj + d.trows * a.n_traj;
    int x[kPPT];
    lane_fill(x, 0);
    for (int t = d.T - 1; t >= lo; --t) {
        double m[K];
        if (staged) {
#pragma unroll
            for (int s = 0; s < K; ++s) m[s] = s_mass[(t - lo) * 8 + s];
        } else {
#pragma unroll
            for (int s = 0; s < K; ++s) m[s] = mass[(int64_t)t * 8 + s];
        }
        int8_t* orow = out + (int64_t)(t - lo) * a.n_traj;
#pragma unroll
        for (int q = 0; q < kPPT; ++q) {
            const int j = i0 + q * kThreads + tid;              // (a lane past n_traj walks along and stores nothing)
            const u32x4 r = draw_block(seed, (uint64_t)(j >> 1), a.draw_base + (uint64_t)t);
            const double u = (j & 1) ? u01_53(r.z, r.w) : u01_53(r.x, r.y);
            double w[K];
            double D = 0.0;
#pragma unroll
            for (int s = 0; s < K; ++s) { w[s] = t == d.T - 1 ? m[s] : dmul_rn(m[s], s_pt[x[q] * 8 + s]); D = D + w[s]; }
            if (D == 0.0) {
#pragma unroll
                for (int s = 0; s < K; ++s) w[s] = m[s];
            }
            x[q] = smooth_pick<K>(w, u);
            if (j < a.n_traj) orow[j] = (int8_t)x[q];
        }
    }
}

}  // namespace cph
