// Conditional SMC runs of a batch (cpprob_hip_batch_run_conditional, _run_conditional_device): the forward pass of particle Gibbs with
// backward sampling.  Every problem runs a particle filter in which one particle, slot 0, is pinned to a reference path r_0 .. r_{T-1}
// the caller hands in (the trajectory the previous sweep's backward simulation left), and the run leaves the backward smoother's
// m table (csrc/batch_smooth.hpp) and nothing else: whatever serves a filtering batch that keeps its masses serves this one.  With
// the retained particle the sweep "conditional run, then one backward-simulated trajectory" leaves the smoothing law invariant at
// every n >= 1 (Whiteley 2010; Lindsten & Schon 2013), where the unconditional run's sweep does so only as n grows.
//
// The resampling is multinomial, the form whose invariance is proven; on discrete states it needs no comb, no ancestor array and no
// particle store: a particle's ancestor matters through the ancestor's STATE alone, and the states of generation t - 1 are the k
// integer masses of row t - 1.  The statement, per problem (T its length, n its particles, k its states, c[s][.] its threshold words;
// tests/csmc_ref.py restates it in Python integers, bit for bit; DESIGN.md section 5 states it once more):
//   slot 0          x_t^0 = r_t & 7, a value >= k taken as k - 1; its Philox words are not used
//   slot i >= 1     w = word i & 3 of draw_block(seed, i >> 2, t): the forward run's own statement and counters (ModelHmmK::draw4)
//     t = 0         x = smallint_from_word(w, 0, k - 1)
//     t >= 1        m[s] the integer masses of row t - 1, C_s their inclusive sums in the order s = 0..k-1 (64-bit), S = C_{k-1};
//                   W = (hi << 32) | lo, lo and hi words 2 (i & 1) and 2 (i & 1) + 1 of draw_block(seed, i >> 1, 2^43 + t);
//                   V = umul64hi(W, S); the ancestor's state a = #{s < k-1 : V >= C_s}; x = #{j < k-1 : w >= c[a][j]}
//   row t           batch_mass_row(cnt_t, ll_t, k, .) of csrc/batch_smc.hpp on the counts of the n slots, slot 0 among them
// Integers only: no floating-point operation other than batch_mass's takes part, so there is nothing to contract.
//
// One workgroup a problem, taken in order[] (the longest first) as batch_smc_kernel takes them; lane-owned runs of 4 particles in
// passes of 1024 -- one Philox block per 4 particles for the words, one per 2 for the ancestors.  The per-state counts are packed 16
// bits a state: a wave_sum_u64 a half, then one LDS word per wavefront, double-buffered by step parity, which makes ONE barrier a
// step; the staged thresholds are first read at step 1, behind step 0's barrier.  Every thread derives cnt, the row and C_s from the
// wavefronts' totals; eight lanes of wavefront 1 write the row.  No atomics, no dynamic LDS; rows t >= T_b are not touched.
#pragma once
#include "batch_smc.hpp"

namespace cph {

// Ordinals in [2^43, 2^43 + 2^24) are the conditional run's own ancestor draws: the particles' statements use the step index, the
// resampling draws 2^40 plus up to 2^39 (kResampleDrawBase), the backward smoother [2^41, 2^42) (kBackwardDrawBase), the forecast
// [2^42, 2^43) (kForecastDrawBase).
constexpr uint64_t kConditionalDrawBase = 1ull << 43;

struct BatchCsmcArgs {
    const double* tab;                         // [B][T_max][kBatchTab]: ll_t[0..8) of row b T_max + t
    const uint64_t* seeds;                     // [B]
    const uint64_t* thr;                       // problem b's 64 threshold words at thr + b * thr_stride, the layout of ModelParams::hk_thr
    const BatchProblem* prob;                  // [B], described batch; nullptr: uniform
    const int32_t* order;                      // [B], described batch: workgroup i runs problem order[i]
    const int8_t* ref;                         // the reference paths, packed as cpprob_hip_batch_smooth_layout(T, B, 1) packs trajectories
    const int64_t* first;                      // [B], described batch: problem b's first entry in ref; nullptr: b * T_max
    double* mass;                              // [B][T_max][8]: row (b, t) at (b T_max + t) * 8
    int T_max, n;                              // uniform: every problem's T and n
    int k, thr_stride;                         // thr_stride: 0 (one shared table) or 64 (a table a problem)
};

__global__ __launch_bounds__(kThreads) void batch_csmc_kernel(BatchCsmcArgs a)
{
    __shared__ uint64_t s_cnt[2][kWaves][2];                    // per-wavefront packed state counts (16 bits a state), by step parity
    __shared__ uint64_t s_thr[64];                              // the problem's threshold rows [k][8]
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    // the problem this workgroup runs and its shape (workgroup-uniform)
    const int b = a.order ? (int)a.order[blockIdx.x] : (int)blockIdx.x;
    const int n = a.prob ? (int)a.prob[b].n : a.n;
    const int T = a.prob ? (int)a.prob[b].T : a.T_max;
    const int k = a.k;
    const int passes = (n + kTile - 1) / kTile;
    const uint64_t seed = a.seeds[b];
    const double* tab = a.tab + (int64_t)b * a.T_max * kBatchTab;
    const int8_t* ref = a.ref + (a.first ? a.first[b] : (int64_t)b * a.T_max);
    double* mass = a.mass + (int64_t)b * a.T_max * 8;
    if (tid < 64) s_thr[tid] = a.thr[(int64_t)b * a.thr_stride + tid];    // (read from step 1 on: step 0's barrier stands in between)
    uint64_t C[8] = {0, 0, 0, 0, 0, 0, 0, 0};                   // the inclusive sums of the previous row's masses
    for (int t = 0; t < T; ++t) {
        const int r = (int)ref[t] & 7;
        const int x_ref = r < k ? r : k - 1;
        const uint64_t S = C[7];
        uint64_t cA = 0, cB = 0;
        for (int p = 0; p < passes; ++p) {
            const int i0 = p * kTile + tid * kPPT;
            if (i0 >= n) continue;
            uint32_t w[kPPT];
            draw_words4(seed, (uint64_t)i0, (uint64_t)t, w);
            uint64_t V[kPPT] = {0, 0, 0, 0};
            if (t > 0) {
                const u32x4 g0 = draw_block(seed, (uint64_t)(i0 >> 1), kConditionalDrawBase + (uint64_t)t);
                const u32x4 g1 = draw_block(seed, (uint64_t)(i0 >> 1) + 1, kConditionalDrawBase + (uint64_t)t);
                V[0] = __umul64hi(((uint64_t)g0.y << 32) | g0.x, S); V[1] = __umul64hi(((uint64_t)g0.w << 32) | g0.z, S);
                V[2] = __umul64hi(((uint64_t)g1.y << 32) | g1.x, S); V[3] = __umul64hi(((uint64_t)g1.w << 32) | g1.z, S);
            }
#pragma unroll
            for (int q = 0; q < kPPT; ++q) {
                const int i = i0 + q;
                if (i >= n) continue;
                int x;
                if (t == 0) x = (int)smallint_from_word(w[q], 0, (uint64_t)k - 1);
                else {
                    int anc = 0;
#pragma unroll
                    for (int s = 0; s < 7; ++s) anc += s < k - 1 && V[q] >= C[s] ? 1 : 0;
                    const uint64_t* c = s_thr + 8 * anc;
                    x = 0;
#pragma unroll
                    for (int j = 0; j < 7; ++j) x += j < k - 1 && (uint64_t)w[q] >= c[j] ? 1 : 0;
                }
                x = i == 0 ? x_ref : x;                         // the retained particle
                cA += x < 4 ? 1ull << (16 * x) : 0ull;
                cB += x >= 4 ? 1ull << (16 * (x - 4)) : 0ull;
            }
        }
        cA = wave_sum_u64(cA);
        cB = wave_sum_u64(cB);
        if (lane == 0) { s_cnt[t & 1][wv][0] = cA; s_cnt[t & 1][wv][1] = cB; }
        __syncthreads();                                        // (one barrier a step: step t + 2 writes this parity again, past step t + 1's barrier)
        uint64_t tA = 0, tB = 0;
#pragma unroll
        for (int wf = 0; wf < kWaves; ++wf) { tA += s_cnt[t & 1][wf][0]; tB += s_cnt[t & 1][wf][1]; }
        uint32_t cnt[8];
#pragma unroll
        for (int s = 0; s < 4; ++s) { cnt[s] = (uint32_t)(tA >> (16 * s)) & 0xffffu; cnt[s + 4] = (uint32_t)(tB >> (16 * s)) & 0xffffu; }
        const double* ll = tab + (int64_t)t * kBatchTab;
        double m[8];
        batch_mass_row(cnt, ll, k, m);
        uint64_t run = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) { run += (uint64_t)m[s]; C[s] = run; }          // (integers below 2^45: the conversion is exact)
        if (tid >= kWave && tid < kWave + 8) {
            double mine = 0.0;
#pragma unroll
            for (int s = 0; s < 8; ++s) mine = tid - kWave == s ? m[s] : mine;
            mass[(int64_t)t * 8 + (tid - kWave)] = mine;
        }
    }
}

}  // namespace cph
