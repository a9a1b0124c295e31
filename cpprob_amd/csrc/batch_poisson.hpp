// Poisson emissions of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables: state s of problem b emits Poisson(rate[b][s]) in place
// of N(mean[s], sigma[s]) (cpprob_hip_batch_begin_problems_poisson, _retable_poisson*, _mstep_poisson_device).  The rates live where the
// means live ([B][k]).  The step kernel and every pass behind it read the emission through the rows tab[t][8] alone, and a record's
// occ_y / occ is the M-step of a rate as it is of a mean, so only what WRITES rows and tables is stated here, next to its Gaussian
// siblings of csrc/batch_retable.hpp and csrc/batch_scale.hpp:
//   log-factorials  poisson_log_fact_table: lf[0] = lf[1] = 0.0, lf[i] = lf[i - 1] + table_log((double)i) up to kPoissonMaxCount,
//                   ascending.  The host fills the table once a context and uploads it (32 KB); the device only looks it up -- no loop
//                   over y and no library lgamma runs in a kernel
//   count           poisson_count(y): the integer 0 .. kPoissonMaxCount that y is, or -1 (NaN, infinities, negatives, non-integers,
//                   counts above the cap)
//   rows            poisson_entry: y log_rate, minus rate, minus lf[y] -- a product and two subtractions, none contracted; -inf for a y
//                   that is no count (the row an infinite observe has under the Gaussian routes), on host and device alike
//   check           retable_check's two bits on the transition rows and bit 16 (kRetableBadRate): a rate not > 0, not finite or not a
//                   normal number (the argument table_log takes).  Bit 4 (a bad mean) is not used
//   M-step          retable_mstep for the transition row and the rate (occ_y / occ), then for a state with occ > 0: rate' = the rate where
//                   it is >= floor, else floor (a NaN too), log_rate' = table_log(rate'), NaN for a rate' the check refuses; a state
//                   without mass keeps rate and logarithm
// Every function of this file runs with fp contract off.  tests/poisson_ref.py restates all of it; tests/host_kernels/batch_poisson_main.cpp
// runs the kernels' text on the host.
//
// batch_retable_poisson_kernel: batch_retable_scaled_kernel's grid and lanes (blockIdx.x the problem, blockIdx.y strides over tiles of
// kRetableRows steps, eight lanes a row, a wavefront stores 512 consecutive bytes).  Every workgroup stages 8 rates and 64 weights in LDS
// (one barrier) and checks them; lane s takes the one logarithm of its state.  Workgroup y = 0 alone stores the status word, the 64
// threshold words and the problem's rates and log-rates in force ([B][8] arrays of the context's own).  A problem with a bit set keeps
// rows, words, rates and log-rates.  No atomics; no result depends on gridDim.y.  64 bytes written and 8 read a step, and lf[c] a gather
// from a table that stays in cache: the launch is bound by HBM.
// batch_mstep_poisson_kernel: one thread a (problem, state), batch_mstep_kernel's layout with the log-rates out where asked for.
#pragma once
#include "batch_scale.hpp"

namespace cph {

constexpr int kRetableBadRate = 16;
constexpr int kPoissonMaxCount = 4095;              // the largest count a row is written for; the log-factorials hold kPoissonMaxCount + 1 doubles

// lf[c] = log(c!), c = 0 .. kPoissonMaxCount
__host__ __device__ inline void poisson_log_fact_table(double* lf)
{
#pragma clang fp contract(off)
    lf[0] = 0.0;
    lf[1] = 0.0;
    for (int i = 2; i <= kPoissonMaxCount; ++i) lf[i] = lf[i - 1] + table_log((double)i);
}

// the count y is, or -1
__host__ __device__ inline int poisson_count(double y)
{
#pragma clang fp contract(off)
    if (!(y >= 0.0) || !(y <= (double)kPoissonMaxCount)) return -1;
    const int c = (int)y;
    return (double)c == y ? c : -1;
}

// log Poisson(y; rate), log_rate = table_log(rate), lf the log-factorials
__host__ __device__ inline double poisson_entry(double y, double rate, double log_rate, const double* lf)
{
#pragma clang fp contract(off)
    const int c = poisson_count(y);
    if (c < 0) return -INFINITY;
    double r = y * log_rate;
    r = r - rate;
    r = r - lf[c];
    return r;
}

// a rate the Poisson route does not take
__host__ __device__ inline bool poisson_bad(double rate)
{
#pragma clang fp contract(off)
    return !(rate > 0.0) || !(rate < INFINITY) || !(rate >= kScaleMinNormal);
}

// the bits of one problem's Poisson table (rates [k], trans [k][k])
__host__ __device__ inline int poisson_check(const double* rates, const double* trans, int k)
{
#pragma clang fp contract(off)
    int bits = retable_check(rates, trans, k) & (kRetableBadWeight | kRetableNoMass);
    for (int s = 0; s < k; ++s) if (poisson_bad(rates[s])) bits |= kRetableBadRate;
    return bits;
}

// state s of one problem's Poisson M-step: rec its record [88]; rates, log_rates [k] and trans [k][k] updated in place (log_rates may
// be null)
__host__ __device__ inline void poisson_mstep(const double* rec, int k, int s, double* rates, double* log_rates, double* trans, double floor)
{
#pragma clang fp contract(off)
    retable_mstep(rec, k, s, rates, trans);
    const double occ = rec[64 + s];
    if (occ > 0.0) {
        const double r = rates[s] >= floor ? rates[s] : floor;
        rates[s] = r;
        if (log_rates) log_rates[s] = poisson_bad(r) ? NAN : table_log(r);      // (a rate the check refuses has no logarithm here)
    }
}

struct BatchRetablePoissonArgs {
    const BatchProblem* prob;                  // [B]: T_b
    const int64_t* first;                      // [B]: problem b's first observe in obs
    const double* rates;                       // [B][k]
    const double* trans;                       // [B][k][k]
    const double* obs;                         // the observes, packed problem after problem
    const double* lfact;                       // [kPoissonMaxCount + 1]: poisson_log_fact_table's
    double* tab;                               // [B][T_max][kBatchTab]
    uint64_t* thr;                             // [B][64]
    int32_t* status;                           // [B]: 0, or the bits of poisson_check
    double* rate_out;                          // [B][8]: the rates in force (states >= k: not touched)
    double* log_rate_out;                      // [B][8]: their logarithms
    int T_max, k;
};

__global__ __launch_bounds__(kThreads) void batch_retable_poisson_kernel(BatchRetablePoissonArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_pois[8 + 64];                           // the problem's rates, then its transition rows
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, k = a.k;
    if (tid < k) s_pois[tid] = a.rates[(int64_t)b * k + tid];
    else if (tid >= 8 && tid < 8 + k * k) s_pois[tid] = a.trans[(int64_t)b * k * k + (tid - 8)];
    __syncthreads();
    const int bits = poisson_check(s_pois, s_pois + 8, k);      // (uniform)
    if (blockIdx.y == 0 && tid == 0) a.status[b] = bits;
    if (bits) return;
    if (blockIdx.y == 0 && tid < 64) a.thr[(int64_t)b * 64 + tid] = retable_threshold(s_pois + 8, k, tid >> 3, tid & 7);
    const int s = tid & 7;
    const double rate = s < k ? s_pois[s] : 1.0;
    const double log_rate = table_log(rate);
    if (blockIdx.y == 0 && tid < k) { a.rate_out[(int64_t)b * 8 + tid] = rate; a.log_rate_out[(int64_t)b * 8 + tid] = log_rate; }
    const int64_t T = a.prob[b].T, stride = (int64_t)gridDim.y * kRetableRows;
    const double* y = a.obs + a.first[b];
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    for (int64_t t = (int64_t)blockIdx.y * kRetableRows + (tid >> 3); t < T; t += stride)
        rows[t * kBatchTab + s] = s < k ? poisson_entry(y[t], rate, log_rate, a.lfact) : -INFINITY;
}

struct BatchMstepPoissonArgs {
    const double* stats;                       // [B][kRetableStats]
    double* rates;                             // [B][k]
    double* trans;                             // [B][k][k]
    double* log_rates;                         // [B][k], or null
    double floor;
    int64_t B;
    int k;
};

// one thread a (problem, state s < k)
__global__ __launch_bounds__(kThreads) void batch_mstep_poisson_kernel(BatchMstepPoissonArgs a)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
    if (i >= a.B * a.k) return;
    const int64_t b = i / a.k;
    poisson_mstep(a.stats + b * kRetableStats, a.k, (int)(i % a.k), a.rates + b * a.k, a.log_rates ? a.log_rates + b * a.k : nullptr,
                  a.trans + b * a.k * a.k, a.floor);
}

}  // namespace cph
