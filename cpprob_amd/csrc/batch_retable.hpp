// New tables for a begun CPPROB_HIP_MODEL_HMM_TABLE batch, where it stands (cpprob_hip_batch_retable, _retable_device), and the M-step of
// particle EM on the device (cpprob_hip_batch_mstep_device).  Between two sweeps of a fitting loop only the tables change -- 72 doubles a
// problem --; the observes, lengths, particle counts, dispatch order, descriptors and workspace stay.  What a begin derives from a table
// is restated here so that the device writes it, stream-ordered, with the bits the host's begin writes:
//   rows        tab[(b T_max + t) 8 + s] = log N(y_t; mean[s], 1) for s < k, -inf beyond: normal_logpdf's statements with its logarithm
//               passed in (log_norm = log(2 pi 1 1), evaluated once on the host with normal_logpdf's own expression) -- a subtraction, a
//               division by 1.0, a product, a sum and a product by -0.5, none contracted; the device takes no logarithm
//   thresholds  hmmk_thresholds: row s < k, tot = the row's weights added from 0.0 in the order j = 0..k-1, acc the same running sum;
//               word 8 s + j = (uint64_t)ceil((acc / tot) * 4294967296.0) for j < k - 1, every other of the 64 words ~0
//   check       batch_check_tables' predicates: bit 1 a weight not finite or not >= 0, bit 2 a row whose total is not > 0, bit 4 a mean
//               not finite; a problem with a bit set is left as it was (rows and thresholds) and its bits are stored in status[b]
//   M-step      cpprob_amd.em.m_step / hmm_table_fit on a record of cpprob_hip_batch_smooth_stats: row = ((0.0 + xi[s][0]) + xi[s][1]) +
//               ...; row > 0: trans[s][j] = xi[s][j] / row; occ[s] > 0: means[s] = occ_y[s] / occ[s]; no mass: the value stays
// Every function of this file runs with fp contract off.  retable_entry restates normal_logpdf_hoisted (include/cpprob/detail/dist.hpp)
// statement for statement instead of calling it: the pragma is lexical, and that function's own statements carry the translation unit's
// contraction on the device (r * r + log_norm as one fused operation, which the host's begin does not form).
// tests/host_kernels/batch_retable_main.cpp holds the two against each other on the host; tests/retable_ref.py restates all of it.
//
// batch_retable_kernel: blockIdx.x the problem, blockIdx.y strides over tiles of kRetableRows steps.  Eight lanes a row, lane s the
// entry s: a wavefront stores 512 consecutive bytes, the eight lanes of a row read the same y_t.  Every workgroup stages the problem's
// table in LDS (72 doubles, one barrier) and checks it -- uniform work of k^2 values --, workgroup y = 0 alone stores the status word and
// the 64 threshold words.  gridDim.y is retable_grid_y's and no result depends on it.  Rows t >= T_b and everything else in the
// workspace are not touched.  No atomics.  64 bytes written and 8 read a step: the launch is bound by HBM.
#pragma once
#include "batch_smc.hpp"

namespace cph {

constexpr int kRetableRows = kThreads / 8;          // rows a workgroup writes a trip
constexpr int kRetableGridMax = 64;                 // gridDim.y at most: a longer problem's workgroups stride
constexpr int kRetableGroups = 4096;                // workgroups a launch aims at: a batch of many problems takes fewer of them a problem, so
                                                    // that a workgroup's staging and check are shared by several trips
constexpr int kRetableBadWeight = 1, kRetableNoMass = 2, kRetableBadMean = 4;
constexpr int kRetableStats = 88;                   // doubles a record of cpprob_hip_batch_smooth_stats: xi[8][8], occ[8], occ_y[8], occ_yy[8]

struct BatchRetableArgs {
    const BatchProblem* prob;                  // [B]: T_b
    const int64_t* first;                      // [B]: problem b's first observe in obs (the sum of the lengths before it)
    const double* means;                       // [B][k]
    const double* trans;                       // [B][k][k]
    const double* obs;                         // the observes, packed problem after problem
    double* tab;                               // [B][T_max][kBatchTab]
    uint64_t* thr;                             // [B][64]
    int32_t* status;                           // [B]: 0, or the bits of retable_check
    double log_norm;                           // log(2 pi 1 1), from the host
    int T_max, k;
};

// gridDim.y of the launch over B problems of at most T_max steps: the trips of the longest problem, capped by kRetableGridMax and by
// kRetableGroups / B
__host__ __device__ inline unsigned retable_grid_y(int64_t T_max, int64_t B)
{
    const int64_t trips = (T_max + kRetableRows - 1) / kRetableRows, share = kRetableGroups / (B < 1 ? 1 : B);
    const int64_t cap = share < 1 ? 1 : (share > kRetableGridMax ? kRetableGridMax : share);
    return (unsigned)(trips < 1 ? 1 : (trips > cap ? cap : trips));
}

// log N(y; mean, 1): normal_logpdf(y, mean, 1.0) with log_norm in place of its logarithm
__host__ __device__ inline double retable_entry(double y, double mean, double log_norm)
{
#pragma clang fp contract(off)
    if (fabs(y) == INFINITY) return -INFINITY;
    double r = (y - mean) / 1.0;
    r *= r;
    r += log_norm;
    r *= -0.5;
    return r;
}

// word 8 s + j of the table's thresholds (trans [k][k])
__host__ __device__ inline uint64_t retable_threshold(const double* trans, int k, int s, int j)
{
#pragma clang fp contract(off)
    if (s >= k || j + 1 >= k) return ~0ull;
    double tot = 0.0, acc = 0.0;
    for (int i = 0; i < k; ++i) tot += trans[s * k + i];
    for (int i = 0; i <= j; ++i) acc += trans[s * k + i];
    return (uint64_t)ceil((acc / tot) * 4294967296.0);
}

__host__ __device__ inline void retable_thresholds(const double* trans, int k, uint64_t* thr /* [64] */)
{
#pragma clang fp contract(off)
    for (int w = 0; w < 64; ++w) thr[w] = retable_threshold(trans, k, w >> 3, w & 7);
}

// the bits of one problem's table (means [k], trans [k][k]); 0: the table is one a begin takes
__host__ __device__ inline int retable_check(const double* means, const double* trans, int k)
{
#pragma clang fp contract(off)
    int bits = 0;
    for (int s = 0; s < k; ++s) {
        double tot = 0.0;
        for (int j = 0; j < k; ++j) {
            const double w = trans[s * k + j];
            if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
            tot += w;
        }
        if (!(tot > 0.0)) bits |= kRetableNoMass;
        if (!(fabs(means[s]) < INFINITY)) bits |= kRetableBadMean;
    }
    return bits;
}

// state s of one problem's M-step: rec its record [88], means [k] and trans [k][k] updated in place
__host__ __device__ inline void retable_mstep(const double* rec, int k, int s, double* means, double* trans)
{
#pragma clang fp contract(off)
    double row = 0.0;
    for (int j = 0; j < k; ++j) row = row + rec[8 * s + j];
    if (row > 0.0) for (int j = 0; j < k; ++j) trans[s * k + j] = rec[8 * s + j] / row;
    const double occ = rec[64 + s];
    if (occ > 0.0) means[s] = rec[72 + s] / occ;
}

__global__ __launch_bounds__(kThreads) void batch_retable_kernel(BatchRetableArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_tab[8 + 64];                            // the problem's means, then its transition rows
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, k = a.k;
    if (tid < k) s_tab[tid] = a.means[(int64_t)b * k + tid];
    else if (tid >= 8 && tid < 8 + k * k) s_tab[tid] = a.trans[(int64_t)b * k * k + (tid - 8)];
    __syncthreads();
    const int bits = retable_check(s_tab, s_tab + 8, k);        // (uniform)
    if (blockIdx.y == 0 && tid == 0) a.status[b] = bits;
    if (bits) return;
    if (blockIdx.y == 0 && tid < 64) a.thr[(int64_t)b * 64 + tid] = retable_threshold(s_tab + 8, k, tid >> 3, tid & 7);
    const int s = tid & 7;
    const int64_t T = a.prob[b].T, stride = (int64_t)gridDim.y * kRetableRows;
    const double mean = s < k ? s_tab[s] : 0.0;
    const double* y = a.obs + a.first[b];
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    for (int64_t t = (int64_t)blockIdx.y * kRetableRows + (tid >> 3); t < T; t += stride)
        rows[t * kBatchTab + s] = s < k ? retable_entry(y[t], mean, a.log_norm) : -INFINITY;
}

struct BatchMstepArgs {
    const double* stats;                       // [B][kRetableStats]
    double* means;                             // [B][k]
    double* trans;                             // [B][k][k]
    int64_t B;
    int k;
};

// one thread a (problem, state s < k)
__global__ __launch_bounds__(kThreads) void batch_mstep_kernel(BatchMstepArgs a)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
    if (i >= a.B * a.k) return;
    const int64_t b = i / a.k;
    retable_mstep(a.stats + b * kRetableStats, a.k, (int)(i % a.k), a.means + b * a.k, a.trans + b * a.k * a.k);
}

}  // namespace cph
