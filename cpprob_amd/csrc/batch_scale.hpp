// Per-state emission scales of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables: the emission of state s is N(mean[s], sigma[s])
// in place of N(mean[s], 1) (cpprob_hip_batch_begin_problems_scaled, _retable_scaled*, _mstep_scaled_device).  The step kernel and every
// pass behind it read the emission through the rows tab[t][8] alone, so only what WRITES rows and tables is restated here, next to its
// unit-scale sibling of csrc/batch_retable.hpp:
//   table_log   log(x) for a normal positive finite x, in uncontracted IEEE operations and without a library call, so that host and
//               device run the same operations and a row the host's begin writes has the bits of the row the device writes: exponent e
//               and mantissa m in [1, 2) by bit operations; m >= kLogSqrt2: m = m * 0.5, e = e + 1, so m lies in [sqrt(1/2), sqrt(2));
//               f = (m - 1) / (m + 1), s = f f; p = the Horner form of c[11] s^10 + ... + c[2] s + c[1] over c[i] = the double of
//               1 / (2 i + 1); r = (f + f) (1.0 + s p); the result is e kLn2Hi + (e kLn2Lo + r).  Twelve terms of the odd series (the
//               1.0 and c[1] .. c[11]); kLn2Hi has 21 trailing zero bits, so e kLn2Hi is exact.  table_log(2 pi) has the bits of the
//               host library's log(2 pi): with every sigma 1.0 the scaled route writes the unit route's rows.
//   log_norm    scale_log_norm(sigma) = table_log(((2 pi) sigma) sigma), normal_logpdf's order of multiplication
//   rows        scale_entry: normal_logpdf_hoisted's statements with a real division -- (y - mean) / sigma, squared, plus log_norm,
//               times -0.5; -inf for an infinite y
//   check       retable_check's three bits and bit 8 (kRetableBadScale): a sigma not finite, not > 0, or with a 2 pi sigma^2 that is not
//               a normal finite number (the argument table_log takes)
//   M-step      retable_mstep for the transition row and the mean, then for a state with occ > 0: v = occ_yy / occ - mean' mean' (a
//               division, a product, a subtraction; mean' the new mean), sigma' = sqrt(v) where v >= floor floor, else floor (a NaN v
//               too), log_norm' = scale_log_norm(sigma'); a state without mass keeps mean, sigma and log_norm.  sqrt is the correctly
//               rounded IEEE square root on the host and, under the compiler's defaults, on gfx950 (tests/test_gpu_batch_scale.py holds
//               the device's against numpy's).
// Every function of this file runs with fp contract off.  tests/scale_ref.py restates all of it; tests/host_kernels/batch_scale_main.cpp
// runs the kernels' text on the host.
//
// batch_retable_scaled_kernel: batch_retable_kernel's grid and lanes (blockIdx.x the problem, blockIdx.y strides over tiles of
// kRetableRows steps, eight lanes a row, a wavefront stores 512 consecutive bytes).  Every workgroup stages 8 means, 8 sigmas and 64
// weights in LDS (one barrier) and checks them; lane s takes the one logarithm of its state.  Workgroup y = 0 alone stores the status
// word, the 64 threshold words and the problem's sigmas and log_norms ([B][8] arrays of the context's own).  A problem with a bit set
// keeps rows, words, sigmas and log_norms.  No atomics; no result depends on gridDim.y.
// batch_mstep_scaled_kernel: one thread a (problem, state), batch_mstep_kernel's layout with the sigmas (and, where asked for, the
// log_norms) in and out.
#pragma once
#include "batch_retable.hpp"

namespace cph {

constexpr int kRetableBadScale = 8;
constexpr double kScaleTwoPi = 2 * 3.14159265358979323846;          // (2 * kPi of cpprob/detail/dist.hpp: a doubling, exact)
constexpr double kLogSqrt2 = 0x1.6a09e667f3bcdp+0;
constexpr double kLn2Hi = 0x1.62e42feep-1, kLn2Lo = 0x1.a39ef35793c76p-33;
constexpr double kScaleMinNormal = 0x1p-1022;

// log(x), x normal, positive and finite
__host__ __device__ inline double table_log(double x)
{
#pragma clang fp contract(off)
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    int e = (int)((u >> 52) & 0x7ffu) - 1023;
    u = (u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    __builtin_memcpy(&m, &u, sizeof m);
    if (m >= kLogSqrt2) { m = m * 0.5; e = e + 1; }
    const double f = (m - 1.0) / (m + 1.0);
    const double s = f * f;
    double p = 0x1.642c8590b2164p-5;                                 // 1 / 23
    p = p * s; p = p + 0x1.8618618618618p-5;                        // 1 / 21
    p = p * s; p = p + 0x1.af286bca1af28p-5;                        // 1 / 19
    p = p * s; p = p + 0x1.e1e1e1e1e1e1ep-5;                        // 1 / 17
    p = p * s; p = p + 0x1.1111111111111p-4;                        // 1 / 15
    p = p * s; p = p + 0x1.3b13b13b13b14p-4;                        // 1 / 13
    p = p * s; p = p + 0x1.745d1745d1746p-4;                        // 1 / 11
    p = p * s; p = p + 0x1.c71c71c71c71cp-4;                        // 1 / 9
    p = p * s; p = p + 0x1.2492492492492p-3;                        // 1 / 7
    p = p * s; p = p + 0x1.999999999999ap-3;                        // 1 / 5
    p = p * s; p = p + 0x1.5555555555555p-2;                        // 1 / 3
    double q = s * p;
    q = 1.0 + q;
    const double r = (f + f) * q;
    const double ed = (double)e;
    double lo = ed * kLn2Lo;
    lo = lo + r;
    const double hi = ed * kLn2Hi;
    return hi + lo;
}

// 2 pi sigma^2 in normal_logpdf's order of multiplication
__host__ __device__ inline double scale_norm_arg(double sigma)
{
#pragma clang fp contract(off)
    double a = kScaleTwoPi * sigma;
    a = a * sigma;
    return a;
}

// a sigma the scaled route does not take
__host__ __device__ inline bool scale_bad(double sigma)
{
#pragma clang fp contract(off)
    const double a = scale_norm_arg(sigma);
    return !(sigma > 0.0) || !(sigma < INFINITY) || !(a >= kScaleMinNormal) || !(a < INFINITY);
}

__host__ __device__ inline double scale_log_norm(double sigma)
{
#pragma clang fp contract(off)
    return table_log(scale_norm_arg(sigma));
}

// log N(y; mean, sigma): normal_logpdf_hoisted's statements
__host__ __device__ inline double scale_entry(double y, double mean, double sigma, double log_norm)
{
#pragma clang fp contract(off)
    if (fabs(y) == INFINITY) return -INFINITY;
    double r = (y - mean) / sigma;
    r *= r;
    r += log_norm;
    r *= -0.5;
    return r;
}

// the bits of one problem's scaled table (means [k], sigmas [k], trans [k][k])
__host__ __device__ inline int scale_check(const double* means, const double* sigmas, const double* trans, int k)
{
#pragma clang fp contract(off)
    int bits = retable_check(means, trans, k);
    for (int s = 0; s < k; ++s) if (scale_bad(sigmas[s])) bits |= kRetableBadScale;
    return bits;
}

// the scale of a state with mass occ > 0 from its record and its new mean
__host__ __device__ inline double scale_sigma(double occ, double occ_yy, double mean, double floor)
{
#pragma clang fp contract(off)
    double v = occ_yy / occ;
    const double mm = mean * mean;
    v = v - mm;
    const double ff = floor * floor;
    return v >= ff ? sqrt(v) : floor;
}

// state s of one problem's scaled M-step: rec its record [88]; means, sigmas, log_norms [k] and trans [k][k] updated in place
// (log_norms may be null)
__host__ __device__ inline void scale_mstep(const double* rec, int k, int s, double* means, double* sigmas, double* log_norms, double* trans, double floor)
{
#pragma clang fp contract(off)
    retable_mstep(rec, k, s, means, trans);
    const double occ = rec[64 + s];
    if (occ > 0.0) {
        const double sg = scale_sigma(occ, rec[80 + s], means[s], floor);
        sigmas[s] = sg;
        if (log_norms) log_norms[s] = scale_bad(sg) ? NAN : scale_log_norm(sg);      // (a scale the check refuses has no logarithm here)
    }
}

struct BatchRetableScaledArgs {
    const BatchProblem* prob;                  // [B]: T_b
    const int64_t* first;                      // [B]: problem b's first observe in obs
    const double* means;                       // [B][k]
    const double* sigmas;                      // [B][k]
    const double* trans;                       // [B][k][k]
    const double* obs;                         // the observes, packed problem after problem
    double* tab;                               // [B][T_max][kBatchTab]
    uint64_t* thr;                             // [B][64]
    int32_t* status;                           // [B]: 0, or the bits of scale_check
    double* sigma_out;                         // [B][8]: the sigmas in force (states >= k: not touched)
    double* log_norm_out;                      // [B][8]: their log_norms
    int T_max, k;
};

__global__ __launch_bounds__(kThreads) void batch_retable_scaled_kernel(BatchRetableScaledArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_scaled[8 + 8 + 64];                     // the problem's means, its sigmas, then its transition rows
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, k = a.k;
    if (tid < k) s_scaled[tid] = a.means[(int64_t)b * k + tid];
    else if (tid >= 8 && tid < 8 + k) s_scaled[tid] = a.sigmas[(int64_t)b * k + (tid - 8)];
    else if (tid >= 16 && tid < 16 + k * k) s_scaled[tid] = a.trans[(int64_t)b * k * k + (tid - 16)];
    __syncthreads();
    const int bits = scale_check(s_scaled, s_scaled + 8, s_scaled + 16, k);      // (uniform)
    if (blockIdx.y == 0 && tid == 0) a.status[b] = bits;
    if (bits) return;
    if (blockIdx.y == 0 && tid < 64) a.thr[(int64_t)b * 64 + tid] = retable_threshold(s_scaled + 16, k, tid >> 3, tid & 7);
    const int s = tid & 7;
    const double mean = s < k ? s_scaled[s] : 0.0, sigma = s < k ? s_scaled[8 + s] : 1.0;
    const double log_norm = scale_log_norm(sigma);
    if (blockIdx.y == 0 && tid < k) { a.sigma_out[(int64_t)b * 8 + tid] = sigma; a.log_norm_out[(int64_t)b * 8 + tid] = log_norm; }
    const int64_t T = a.prob[b].T, stride = (int64_t)gridDim.y * kRetableRows;
    const double* y = a.obs + a.first[b];
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    for (int64_t t = (int64_t)blockIdx.y * kRetableRows + (tid >> 3); t < T; t += stride)
        rows[t * kBatchTab + s] = s < k ? scale_entry(y[t], mean, sigma, log_norm) : -INFINITY;
}

struct BatchMstepScaledArgs {
    const double* stats;                       // [B][kRetableStats]
    double* means;                             // [B][k]
    double* trans;                             // [B][k][k]
    double* sigmas;                            // [B][k]
    double* log_norms;                         // [B][k], or null
    double floor;
    int64_t B;
    int k;
};

// one thread a (problem, state s < k)
__global__ __launch_bounds__(kThreads) void batch_mstep_scaled_kernel(BatchMstepScaledArgs a)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
    if (i >= a.B * a.k) return;
    const int64_t b = i / a.k;
    scale_mstep(a.stats + b * kRetableStats, a.k, (int)(i % a.k), a.means + b * a.k, a.sigmas + b * a.k, a.log_norms ? a.log_norms + b * a.k : nullptr,
                a.trans + b * a.k * a.k, a.floor);
}

}  // namespace cph
