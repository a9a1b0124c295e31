// The conjugate draw of a Gibbs sweep over the tables of a CPPROB_HIP_MODEL_HMM_TABLE batch (cpprob_hip_batch_draw_tables_device): given
// a trajectory's record a problem (csrc/batch_trajstats.hpp; pooled over a tie by csrc/batch_pool.hpp), the next table is drawn on the
// device -- every transition row from its Dirichlet posterior, every mean from its normal posterior and, for a batch with emission scales
// (csrc/batch_scale.hpp), every variance from its inverse-gamma posterior -- so that a sampler's sweep (run, statistics, draw, re-table)
// is enqueued without the host looking at anything.  cpprob_amd.gibbs.sample_tables states the same posteriors on numpy's generator; this
// is another generator and therefore another chain.
//
// The variates need log, sqrt and divide only: table_log (csrc/batch_scale.hpp) and the correctly rounded IEEE division and square root,
// none contracted, so host, device and the plain-Python restatement tests/gibbs_ref.py give the same bits.
//   words    Philox blocks draw_block(seed_b, v, kTableDrawBase + (sweep << 24) + i): v the variate's slot in the problem -- transition
//            entry (s, j) 8 s + j, the mean of state c 64 + c, its variance 72 + c --, attempt a of a variate takes i = 2 a for its
//            normal pair and i = 2 a + 1 for its uniform.  A variate is a pure function of (seed, slot, sweep, attempt): nothing depends
//            on lanes or grid.  sweep < 2^16, a < 64.
//   normal   gibbs_normal_attempt, Marsaglia's polar method on one block (x, y, z, w):  v1 = 2 u01_53(x, y) - 1, v2 = 2 u01_53(z, w) - 1,
//            s = v1 v1 + v2 v2;  refused where s >= 1 or s == 0;  z = v1 sqrt((-2 table_log(s)) / s).  The pair's second variate is
//            dropped.  (v1 and v2 are multiples of 2^-52: an s that is not 0 is a normal number.)
//   gamma    gibbs_gamma_attempt, Marsaglia & Tsang 2000 for a shape >= 1 without the squeeze step:  d = shape - 1.0 / 3.0,
//            c = 1 / sqrt(9 d);  an attempt takes z, then v = 1 + c z, v3 = (v v) v, then u = u01_53 of its uniform block's (x, y), and
//            accepts d v3 iff  table_log(u) < (((0.5 z) z + d) - d v3) + d table_log(v3).  Refused: a refused z, v <= 0, u == 0,
//            v3 < kScaleMinNormal (outside table_log's domain).
//   loops    gibbs_normal and gibbs_gamma try attempts 0 .. max_attempts - 1 (max_attempts <= kGibbsMaxAttempts = 64) and take the first
//            that is not refused; a variate that exhausts them is 0.0 and raises kGibbsNoDraw.  No loop is unbounded.  (A polar attempt
//            is refused with probability 1 - pi / 4; a whole gamma attempt at shape 1 with about 0.25.)
//   table    G[s][j] ~ Gamma(alpha + xi[s][j]), total = ((0.0 + G[s][0]) + G[s][1]) + ..., trans'[s][j] = G[s][j] / total;
//            t2 = tau0 tau0;  unit: prec = 1 / t2 + occ, mean' = (mu0 / t2 + occ_y) / prec + z / sqrt(prec);
//            scaled: var = sigma sigma, prec = 1 / t2 + occ / var, mean' = (mu0 / t2 + occ_y / var) / prec + z / sqrt(prec), then
//            g ~ Gamma(a0 + occ / 2), rate = b0 + ((occ_yy - (2 mean') occ_y) + (mean' mean') occ) / 2, sigma' = sqrt(rate / g).
//   check    a variate without a draw: status = kGibbsNoDraw and nothing else is looked at.  Otherwise retable_check's predicates on the
//            new table (learn_row_bits) and, scaled, bit 8 for a sigma' scale_bad refuses.  status 0: means, rows (and sigmas) are
//            stored over the caller's arrays; any bit: status alone is stored and the problem keeps its table for the sweep.
// Every function of this file runs with fp contract off.
//
// batch_draw_tables_kernel, batch_draw_tables_scaled_kernel: one body, batch_draw_tables_body<kScaled>.  One wavefront a problem, kWaves
// problems a workgroup, the lane layout of batch_learn_kernel: lane (s, j) = 8 s + j draws G[s][j], lane (c, c) also the mean of state
// c and, kScaled, its variance -- up to three variates, one after the other.  The rejection loops diverge inside the wavefront; every
// shuffle (the row totals, the rows and bits for the check) and the ballot of kGibbsNoDraw stand outside them.  No LDS, no barrier, no
// atomics.  The kernels write no rows, no threshold words and no log_norm: cpprob_hip_batch_retable_device does, from these tables.
#pragma once
#include "batch_learn.hpp"

namespace cph {

// Ordinals in [2^44, 2^44 + 2^40) are the table draws' own: the particles' statements use the step index, the resampling draws 2^40
// plus up to 2^39 (kResampleDrawBase), the backward smoother [2^41, 2^42) (kBackwardDrawBase), the forecast [2^42, 2^43)
// (kForecastDrawBase), the conditional run's ancestor draws [2^43, 2^43 + 2^24).
constexpr uint64_t kTableDrawBase = 1ull << 44;
constexpr int kGibbsNoDraw = 32;                    // a status bit beside retable_check's: a variate exhausted its attempts
constexpr int kGibbsMaxAttempts = 64;
constexpr uint64_t kGibbsMaxSweep = 1ull << 16;
constexpr int kGibbsMeanSlot = 64, kGibbsVarSlot = 72;

struct GibbsPrior { double alpha, mu0, tau0, a0, b0; };        // (cpprob_hip_gibbs_prior's fields)

// u01_53's statement where the host runs it too
__host__ __device__ inline double gibbs_u01(uint32_t lo, uint32_t hi)
{
#pragma clang fp contract(off)
    return (double)((uint64_t)lo | ((uint64_t)(hi >> 11) << 32)) * kTwoPowM53;
}

// one polar attempt on a block's four words; false: refused
__host__ __device__ inline bool gibbs_normal_attempt(uint32_t x, uint32_t y, uint32_t z, uint32_t w, double& out)
{
#pragma clang fp contract(off)
    double v1 = 2.0 * gibbs_u01(x, y);
    v1 = v1 - 1.0;
    double v2 = 2.0 * gibbs_u01(z, w);
    v2 = v2 - 1.0;
    double s = v1 * v1;
    const double t = v2 * v2;
    s = s + t;
    if (s >= 1.0 || s == 0.0) return false;
    double q = -2.0 * table_log(s);
    q = q / s;
    out = v1 * sqrt(q);
    return true;
}

// d and c of a shape >= 1
__host__ __device__ inline void gibbs_gamma_setup(double shape, double& d, double& c)
{
#pragma clang fp contract(off)
    d = shape - 1.0 / 3.0;
    c = 9.0 * d;
    c = sqrt(c);
    c = 1.0 / c;
}

// one Marsaglia-Tsang attempt on an accepted normal z and a uniform u; false: refused
__host__ __device__ inline bool gibbs_gamma_attempt(double d, double c, double z, double u, double& out)
{
#pragma clang fp contract(off)
    double v = c * z;
    v = 1.0 + v;
    if (!(v > 0.0)) return false;
    double v3 = v * v;
    v3 = v3 * v;
    if (u == 0.0 || v3 < kScaleMinNormal) return false;
    double r = 0.5 * z;
    r = r * z;
    r = r + d;
    const double dv = d * v3;
    r = r - dv;
    const double dl = d * table_log(v3);
    r = r + dl;
    if (!(table_log(u) < r)) return false;
    out = d * v3;
    return true;
}

// the standard normal of slot `slot`; base = kTableDrawBase + (sweep << 24).  drawn = false and 0.0 where every attempt is refused
__device__ __forceinline__ double gibbs_normal(uint64_t seed, uint64_t slot, uint64_t base, int max_attempts, bool& drawn)
{
#pragma clang fp contract(off)
    double z = 0.0;
    drawn = false;
    for (int a = 0; a < max_attempts && !drawn; ++a) {
        const u32x4 r = draw_block(seed, slot, base + 2 * (uint64_t)a);
        drawn = gibbs_normal_attempt(r.x, r.y, r.z, r.w, z);
    }
    return drawn ? z : 0.0;
}

// Gamma(shape, 1), shape >= 1, of slot `slot`
__device__ __forceinline__ double gibbs_gamma(double shape, uint64_t seed, uint64_t slot, uint64_t base, int max_attempts, bool& drawn)
{
#pragma clang fp contract(off)
    double d, c, g = 0.0;
    gibbs_gamma_setup(shape, d, c);
    drawn = false;
    for (int a = 0; a < max_attempts && !drawn; ++a) {
        const u32x4 r = draw_block(seed, slot, base + 2 * (uint64_t)a);
        double z;
        if (!gibbs_normal_attempt(r.x, r.y, r.z, r.w, z)) continue;
        const u32x4 ru = draw_block(seed, slot, base + 2 * (uint64_t)a + 1);
        drawn = gibbs_gamma_attempt(d, c, z, gibbs_u01(ru.x, ru.y), g);
    }
    return drawn ? g : 0.0;
}

// the mean of a state from its record and a standard normal z; scaled: var = the square of the sigma in force
__host__ __device__ inline double gibbs_mean(double occ, double occ_y, double var, bool scaled, double mu0, double tau0, double z)
{
#pragma clang fp contract(off)
    const double t2 = tau0 * tau0;
    double prec = scaled ? occ / var : occ;
    prec = 1.0 / t2 + prec;
    double m = scaled ? occ_y / var : occ_y;
    m = mu0 / t2 + m;
    m = m / prec;
    return m + z / sqrt(prec);
}

// the inverse-gamma posterior's rate of a state at the mean just drawn
__host__ __device__ inline double gibbs_rate(double occ, double occ_y, double occ_yy, double mean, double b0)
{
#pragma clang fp contract(off)
    double r = 2.0 * mean;
    r = r * occ_y;
    r = occ_yy - r;
    double q = mean * mean;
    q = q * occ;
    r = r + q;
    r = r / 2.0;
    return b0 + r;
}

struct BatchDrawTablesArgs {
    const double* stats;                       // [B][kRetableStats]: a trajectory's record a problem (a tie's members: the pooled one)
    const uint64_t* seeds;                     // [B]
    double* means;                             // [B][k]
    double* trans;                             // [B][k][k]
    double* sigmas;                            // [B][k]; the unit kernel does not read the field
    int32_t* status;                           // [B], or null
    GibbsPrior prior;
    uint64_t draw_base;                        // kTableDrawBase + (sweep << 24)
    int B, k, max_attempts;
};

template <bool kScaled>
__device__ __forceinline__ void batch_draw_tables_body(const BatchDrawTablesArgs& a)
{
#pragma clang fp contract(off)
    const int lane = lane_id(), sp = lane >> 3, c = lane & 7;
    const bool live = sp < a.k, entry = live && c < a.k, diag = live && c == sp;
    for (int b = online_uniform((int)blockIdx.x * kWaves + wave_id()); b < a.B; b += (int)gridDim.x * kWaves) {   // (wavefront-uniform)
        const double* rec = a.stats + (int64_t)b * kRetableStats;
        const uint64_t seed = a.seeds[b];
        double* trans = a.trans + (int64_t)b * a.k * a.k;
        double* means = a.means + (int64_t)b * a.k;
        bool missing = false;
        // lane (s, j): G[s][j]
        double G = 0.0;
        if (entry) {
            bool drawn;
            G = gibbs_gamma(a.prior.alpha + rec[lane], seed, (uint64_t)lane, a.draw_base, a.max_attempts, drawn);
            missing = !drawn;
        }
        // lane (c, c): the mean of state c and, kScaled, its sigma
        double mean = 0.0, sigma = 1.0;
        int bad_scale = 0;
        if (diag) {
            const double occ = rec[64 + c], occ_y = rec[72 + c];
            bool drawn;
            const double z = gibbs_normal(seed, (uint64_t)(kGibbsMeanSlot + c), a.draw_base, a.max_attempts, drawn);
            missing = missing || !drawn;
            double var = 1.0;
            if constexpr (kScaled) { const double sg = a.sigmas[(int64_t)b * a.k + c]; var = sg * sg; }
            mean = gibbs_mean(occ, occ_y, var, kScaled, a.prior.mu0, a.prior.tau0, z);
            if constexpr (kScaled) {
                const double g = gibbs_gamma(a.prior.a0 + occ / 2.0, seed, (uint64_t)(kGibbsVarSlot + c), a.draw_base, a.max_attempts, drawn);
                missing = missing || !drawn;
                sigma = sqrt(gibbs_rate(occ, occ_y, rec[80 + c], mean, a.prior.b0) / g);
                bad_scale = scale_bad(sigma) ? kRetableBadScale : 0;
            }
        }
        // (the wavefront is whole again) the row totals, the new rows on each of their lanes, their bits
        const bool no_draw = __ballot(missing) != 0;
        double total = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const double x = __shfl(G, sp * 8 + j); if (j < a.k) total = total + x; }
        const double tr = entry ? G / total : 0.0;
        double row[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) row[j] = __shfl(tr, sp * 8 + j);
        const double mean_row = __shfl(mean, sp * 9);           // (the mean of state s': lane (s', s') holds it)
        int bad_row = 0;
        if constexpr (kScaled) bad_row = __shfl(bad_scale, sp * 9);
        const int mine = live ? learn_row_bits(row, mean_row, a.k) | bad_row : 0;
        int bits = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) bits |= __shfl(mine, s * 8);
        if (no_draw) bits = kGibbsNoDraw;
        if (a.status && lane == 0) a.status[b] = bits;
        if (bits) continue;                                     // (uniform: the problem keeps its table)
        if (entry) trans[sp * a.k + c] = tr;
        if (diag) means[c] = mean;
        if constexpr (kScaled) if (diag) a.sigmas[(int64_t)b * a.k + c] = sigma;
    }
}

__global__ __launch_bounds__(kThreads) void batch_draw_tables_kernel(BatchDrawTablesArgs a)
{
#pragma clang fp contract(off)
    batch_draw_tables_body<false>(a);
}

__global__ __launch_bounds__(kThreads) void batch_draw_tables_scaled_kernel(BatchDrawTablesArgs a)
{
#pragma clang fp contract(off)
    batch_draw_tables_body<true>(a);
}

}  // namespace cph
