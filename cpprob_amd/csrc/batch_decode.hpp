// Decoding a batch (cpprob_hip_batch_decode, _decode_device, cpprob_hip_batch_decode_lag, _decode_lag_device): the single most probable
// state path of every problem given its observes, by dynamic programming over the states the particles occupy (the particle form of the
// MAP sequence estimate: Godsill, Doucet & West 2001).  It reads what the batch already holds -- the backward smoother's m table
// (csrc/batch_smooth.hpp; m_t[s] > 0 is the support), the per-step log-likelihood rows of `tab` and the 32-bit threshold words, whose
// integer differences P[s][s'] smooth_trans_mass returns -- and touches no particle.
//
// The arithmetic, per problem (L = the length reached, k its states, m_t[0..8) its rows of the m table, ll_t[s] entry s < k of its
// per-step table row; DESIGN.md section 5 states it once more):
//   lp[s][s']  = log(double(P[s][s']) * 2^-32), -inf where P = 0;  lp0 = log(1.0 / double(k)).  Both computed ON THE HOST with std::log
//                (decode_log_table below) and handed to the kernels as doubles: the device evaluates no logarithm
//   support      S_t = { s < k : m_t[s] > 0 }
//   v_0[s]     = lp0 + ll_0[s] for s in S_0, else -inf;  bp_0[.] = 0
//   t >= 1, each s' < k: best = -inf, arg = 0; for s = 0 .. k-1 in that order c = v_{t-1}[s] + lp[s][s'] (one addition), taken if
//                c > best (strict: ties go to the lowest s, an all -inf column keeps arg = 0);  bp_t[s'] = arg;
//                v_t[s'] = best + ll_t[s'] (one addition) for s' in S_t, else -inf
//   end_t      = the first s of the same strict scan over v_t[0..k)
//   step word    w_t = sum over s' < 8 of bp_t[s'] << (3 s') | end_t << 24: one uint32 a step, states >= k zero; all a traceback reads
//   full decode  x_{L-1} = end_{L-1};  x_{t-1} = (w_t >> 3 x_t) & 7;  score = v_{L-1}[end_{L-1}], the log joint density of path and
//                observes under the realised law
//   fixed lag    e(t) = min(t + lag, L - 1);  X_t = the state at t of the traceback started at end_{e(t)}: final once lag more observes
//                have arrived, a function of words t+1 .. e(t) alone; the rows with e(t) = L - 1 are the full decode's
// On a store a run wrote every column of a supported state has a finite candidate (each particle's ancestor had positive mass and its
// transition was realised), so the -inf rules are defensive, as the smoother's D = 0 rule is.  Only additions and comparisons of
// doubles occur (fp contract off in every function of this file): the words are a pure function of the inputs' bits, and
// tests/decode_ref.py restates them bit for bit.
//
// Two launches, not one: the words are written by one lane and read by every lane of the traceback, and stream order makes the writes
// visible without fences.  batch_decode_forward_kernel: one wavefront a problem, kWaves problems a workgroup (and the problems
// gridDim.x * kWaves apart: batch_smooth_stats_kernel's grid).  Lane (s', s) = 8 s' + s holds lp[s][s']; the ordered strict-max scan
// gathers its eight candidates with wavefront shuffles, as smooth_marginal_sum gathers its terms.  It walks the steps [lo, L) from the
// saved v row of the problem (8 doubles; lo = 0 reads none), writes one word a step, the new v row and the score.  The walk is a
// dependent chain over t, so the ll and m entries of step t + 1 are loaded before step t's arithmetic.
// batch_decode_trace_kernel: blockIdx.x the problem.  Row blockIdx.y = 0 is the item of end L - 1 on ONE wavefront: it stores every
// requested t >= L - 1 - lag (the full decode: every t), staging the words 64 at a time (one coalesced load) and stepping through them
// with shuffles, not one dependent global load a step; consecutive steps go to consecutive bytes.  Rows blockIdx.y >= 1 hold the
// items of the ends e < L - 1, one LANE an item, the items (gridDim.y - 1) * kThreads apart (batch_smooth_lag_kernel's striding): a
// lane walks lag words and stores X_{e - lag}.  The items are independent: no barrier, no atomics, no LDS, no result that depends on
// the grid.
#pragma once
#include "batch_smooth.hpp"

namespace cph {

constexpr int kDecodeTraceGridMax = 4096;           // gridDim.y - 1 of batch_decode_trace_kernel at most: kThreads times it items a problem and trip

struct BatchDecodeArgs {
    const BatchSmoothProblem* desc;            // [B]: T, rows (first row in the m table AND first word), lo (the first step the forward
                                               // pass walks), trows (first entry of the packed path), mfrom (the first fixed-lag row wanted)
    const double* mass;                        // the m table
    const double* tab;                         // [B][T_max][kBatchTab]
    const double* lp;                          // problem b's log masses at lp + b * lp_stride, lp[s][s'] at 8 s + s'
    double lp0;                                // log(1.0 / double(k))
    double* v;                                 // [B][8]: v_{L-1} of the steps walked so far
    uint32_t* words;                           // the step words, addressed as the m table's rows
    double* score;                             // [B], zeroed by the caller; nullptr: not wanted
    int8_t* path;                              // full: packed by the lengths reached; fixed lag: [B][n_rows], filled with -1 by the caller
    int B, T_max, k, lp_stride;
    int full, lag, n_rows;                     // full != 0: the whole path; else the fixed-lag rows
};

// lp[s][s'] (at 8 s + s') and lp0 of the threshold rows `thr` ([k][8], entries 0..k-2 of a row: smooth_trans_mass's statement).  Host
// code: the one place a logarithm is taken.
inline void decode_log_table(const uint64_t* thr, int k, double* lp, double* lp0)
{
    for (int s = 0; s < 8; ++s) {
        for (int sn = 0; sn < 8; ++sn) {
            uint64_t P = 0;
            if (s < k && sn < k) {
                const uint64_t hi = sn == k - 1 ? 1ull << 32 : thr[s * 8 + sn];
                const uint64_t lo = sn == 0 ? 0ull : thr[s * 8 + sn - 1];
                P = hi - lo;
            }
            lp[s * 8 + sn] = P ? std::log((double)P * 0x1p-32) : -INFINITY;
        }
    }
    *lp0 = std::log(1.0 / (double)k);
}

// v, which every lane of the wavefront holds alike, as a value the compiler knows to be uniform (the descriptor becomes a scalar load)
__device__ __forceinline__ int decode_uniform(int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

// The first s of the strict scan over v[0..8), lane (s', .) holding v[s']: the same in every lane; its value in `top`.
__device__ __forceinline__ int decode_end(double vm, double& top)
{
#pragma clang fp contract(off)
    double best = -INFINITY;
    int end = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double vj = __shfl(vm, 8 * j);
        if (vj > best) { best = vj; end = j; }
    }
    top = best;
    return end;
}

__global__ __launch_bounds__(kThreads) void batch_decode_forward_kernel(BatchDecodeArgs a)
{
#pragma clang fp contract(off)
    const int lane = lane_id(), sp = lane >> 3, s = lane & 7;
    for (int b = decode_uniform((int)blockIdx.x * kWaves + wave_id()); b < a.B; b += (int)gridDim.x * kWaves) {   // (wavefront-uniform)
        const BatchSmoothProblem d = a.desc[b];
        const int L = d.T;
        if (L <= 0) continue;                                   // nothing reached yet: its score stays 0
        const double* mass = a.mass + d.rows * 8;
        const double* tab = a.tab + (int64_t)b * a.T_max * kBatchTab;
        uint32_t* words = a.words + d.rows;
        double* vrow = a.v + (int64_t)b * 8;
        const double lp = a.lp[(int64_t)b * a.lp_stride + 8 * s + sp];
        double vs = d.lo > 0 ? vrow[s] : -INFINITY;             // v_{t-1}[s]
        double vm = d.lo > 0 ? vrow[sp] : -INFINITY;            // v_{t-1}[s'] (no step to walk: the row as it was saved)
        // the entries of the step to come (nothing to walk: row L - 1 once more, never used)
        int tn = d.lo < L ? d.lo : L - 1;
        double ll = tab[(int64_t)tn * kBatchTab + sp], m = mass[(int64_t)tn * 8 + sp];
        for (int t = d.lo; t < L; ++t) {
            const double llc = ll, mc = m;
            tn = t + 1 < L ? t + 1 : t;                         // (the last step loads its own row again: in bounds, never used)
            ll = tab[(int64_t)tn * kBatchTab + sp];
            m = mass[(int64_t)tn * 8 + sp];
            const double c = vs + lp;
            double best = -INFINITY;
            int arg = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {                       // (lp is -inf for the states >= k: they are never taken)
                const double cj = __shfl(c, sp * 8 + j);
                if (cj > best) { best = cj; arg = j; }
            }
            if (t == 0) { best = a.lp0; arg = 0; }
            vm = sp < a.k && mc > 0.0 ? best + llc : -INFINITY; // (the defensive rule: a state off the support carries no path)
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) w |= (uint32_t)__shfl(arg, 8 * j) << (3 * j);
            double top;
            const int end = decode_end(vm, top);
            vs = __shfl(vm, 8 * s);
            if (lane == 0) words[t] = w | (uint32_t)end << 24;
        }
        double top;
        (void)decode_end(vm, top);
        if (s == 0) vrow[sp] = vm;
        if (lane == 0 && a.score) a.score[b] = top;
    }
}

__global__ __launch_bounds__(kThreads) void batch_decode_trace_kernel(BatchDecodeArgs a)
{
    const int b = (int)blockIdx.x, tid = threadIdx.x, lane = lane_id();
    const BatchSmoothProblem d = a.desc[b];                     // workgroup-uniform
    const int L = d.T, from = a.full ? 0 : d.mfrom;
    if (from >= L) return;                                      // nothing reached yet, or no row asked for
    const uint32_t* words = a.words + d.rows;
    int8_t* out = a.full ? a.path + d.trows : a.path + ((int64_t)b * a.n_rows - from);   // out[t]
    const int lag = a.full || a.lag > L ? L : a.lag;
    if (blockIdx.y == 0) {
        if (tid >= kWave) return;
        const int first = L - 1 - lag > from ? L - 1 - lag : from;   // the step the walk ends at
        int x = 0;
        for (int hi = L - 1; hi >= first; hi -= kWave) {        // lane i of a chunk has step hi - i
            const int t = hi - lane;
            const uint32_t w = t >= first ? words[t] : 0u;
            if (hi == L - 1) x = (int)(__shfl(w, 0) >> 24);
            int mine = 0;
#pragma unroll 8
            for (int i = 0; i < kWave; ++i) {                   // (eight steps' words in flight, not all 64: they would not fit the scalar registers)
                const uint32_t wi = __shfl(w, i);
                mine = lane == i ? x : mine;
                x = (int)(wi >> (3 * x)) & 7;
            }
            if (t >= first) out[t] = (int8_t)mine;
        }
        return;
    }
    const int items = L - 1 - from - lag;                       // the ends from + lag .. L - 2
    for (int item = ((int)blockIdx.y - 1) * kThreads + tid; item < items; item += ((int)gridDim.y - 1) * kThreads) {
        const int e = L - 2 - item;
        int x = (int)(words[e] >> 24);
        for (int t = e; t > e - lag; --t) x = (int)(words[t] >> (3 * x)) & 7;
        out[e - lag] = (int8_t)x;
    }
}

}  // namespace cph
