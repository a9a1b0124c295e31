// Categorical emissions of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables: state s of problem b emits symbol v of an alphabet
// of V <= kCategoricalMaxSymbols symbols with probability E[b][s][v] (cpprob_hip_batch_begin_problems_categorical, _retable_categorical*,
// _symbol_stats*, _mstep_categorical_device).  The step kernel and every pass behind it read the emission through the rows tab[t][8]
// alone, so only what WRITES rows and tables, and the one statistic the 88-double record cannot give, is stated here:
//   symbol          categorical_symbol(y, V): the integer 0 .. V-1 that y is, or -1 (NaN, infinities, negatives, non-integers, y >= V)
//   rows            categorical_entry: logE[s][c] for the symbol c that y is, logE[s][v] = table_log(E[s][v]); -inf for a y that is no
//                   symbol (the row an infinite observe has under the Gaussian routes) and for s >= k, on host and device alike
//   check           retable_check's two bits on the transition rows and bit 32 (kRetableBadProb): an E[s][v], s < k, v < V, not > 0,
//                   not finite or not a normal number (the argument table_log takes).  The rows of E are used AS GIVEN: nothing here
//                   normalises them, and a row that does not sum to 1 is the caller's model
//   symbol counts   cnt[s][v] = sum over the steps t with symbol(y_t) = v of g_t[s], g_t the smoother's marginal: beside the 88 doubles
//                   of batch_smooth_stats_kernel, whose bits the record's first 88 are (occ_y and occ_yy with the symbol values as the
//                   observes).  No sum over y recovers cnt from occ, occ_y, occ_yy, so the walk keeps it
//   M-step          the transition row as retable_mstep forms it; tot = ((0.0 + cnt[s][0]) + cnt[s][1]) + ... + cnt[s][V-1]; tot > 0:
//                   E'[s][v] = cnt[s][v] / tot where that is >= floor, else floor (a NaN too); a state without mass keeps its row.  A
//                   fitted row may therefore sum to as much as 1 + 64 floor: it is NOT renormalised (the choice rate_floor makes)
// Every function of this file runs with fp contract off and forms its products through dmul_rn.  tests/categorical_ref.py restates all
// of it.
//
// batch_retable_categorical_kernel: batch_retable_poisson_kernel's grid and lanes (blockIdx.x the problem, blockIdx.y strides over tiles
// of kRetableRows steps, eight lanes a row, a wavefront stores 512 consecutive bytes).  A workgroup stages the problem's transition
// weights and its emission matrix: thread i takes the slots i and i + 256 of the 512 (slot = 64 s + v), tests them, takes their two
// logarithms and stores them TRANSPOSED, logE[v][8], so the eight lanes of a row read 64 consecutive bytes of LDS ([s][64] would put
// them 512 bytes apart, all on one bank).  Slots with s >= k or v >= V hold -inf.  The check is parallel: a thread tests its own two
// entries, threads < k^2 a weight, threads < k a row's total, and __syncthreads_or joins each bit.  Workgroup y = 0 alone stores the
// status word, the 64 threshold words and E and logE in force ([B][8][64], slots outside the table 0.0 and -inf).  A problem with a bit
// set keeps rows, words and tables.  No atomics; no result depends on gridDim.y.
// batch_symbol_stats_kernel: batch_smooth_stats_kernel's walk, statement for statement -- one wavefront a problem, kWaves problems a
// workgroup, lane (s', s), the same smooth_marginal_start / _term / _sum, the same prefetch -- and on top of it lane (v', s) keeps
// cnt[s][8 i + v'], i = 0..7, in eight registers.  c_t is wavefront-uniform (one load of one address and one conversion, taken with
// the prefetch, off the serial chain); after g_t[s] stands alike on the lanes (., s), the lanes with v' == (c_t & 7) add it to the
// accumulator c_t >> 3, chosen by an unrolled select.  No LDS, no barrier, no atomics; the grid is capped at kSymbolGridMax workgroups
// (the problems gridDim.x * kWaves apart) and no result depends on it.  The walk keeps its sibling's T == 0 branch (an all-zero record),
// and the enqueue its sibling's memset for a batch without steps, but no caller reaches either today: only a described begin makes a
// categorical batch, it refuses a problem of length 0, and there is no online categorical begin.  Neither is covered by a test.
// batch_mstep_categorical_kernel: one thread a (problem, state s < k).
#pragma once
#include "batch_poisson.hpp"
#include "batch_suffstats.hpp"

namespace cph {

constexpr int kRetableBadProb = 32;
constexpr int kCategoricalMaxSymbols = 64;          // V at most: a lane group's eight accumulators of eight symbols
constexpr int kCategoricalSlots = 8 * kCategoricalMaxSymbols;
constexpr int kSymbolStats = kSuffStats + kCategoricalSlots;   // doubles a problem: the 88 of kSuffStats, then cnt[s][v] at 88 + 64 s + v
constexpr int kSymbolGridMax = 2048;                // workgroups at most: kWaves times it problems in flight, the rest strided

// the symbol y is, or -1
__host__ __device__ inline int categorical_symbol(double y, int V)
{
#pragma clang fp contract(off)
    if (!(y >= 0.0) || !(y < (double)V)) return -1;
    const int c = (int)y;
    return (double)c == y ? c : -1;
}

// log E[s][symbol(y)]: col = the state's logarithm of symbol 0, stride = the doubles between two symbols of a state (8 in the kernel's
// transposed staging, 1 in a [s][64] array)
__host__ __device__ inline double categorical_entry(double y, int V, const double* col, int stride)
{
#pragma clang fp contract(off)
    const int c = categorical_symbol(y, V);
    return c < 0 ? -INFINITY : col[c * stride];
}

// a probability the categorical route does not take
__host__ __device__ inline bool categorical_bad(double p)
{
#pragma clang fp contract(off)
    return !(p > 0.0) || !(p < INFINITY) || !(p >= kScaleMinNormal);
}

// the bits of one problem's categorical table (E [k][V], trans [k][k]), serially: the host's validation and the kernel's parallel check
// form these bits
__host__ __device__ inline int categorical_check(const double* E, const double* trans, int k, int V)
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
        for (int v = 0; v < V; ++v) if (categorical_bad(E[s * V + v])) bits |= kRetableBadProb;
    }
    return bits;
}

// state s of one problem's categorical M-step: rec its record [kSymbolStats]; E [k][V] and trans [k][k] updated in place
__host__ __device__ inline void categorical_mstep(const double* rec, int k, int V, int s, double* E, double* trans, double floor)
{
#pragma clang fp contract(off)
    double row = 0.0;
    for (int j = 0; j < k; ++j) row = row + rec[8 * s + j];
    if (row > 0.0) for (int j = 0; j < k; ++j) trans[s * k + j] = rec[8 * s + j] / row;
    const double* cnt = rec + kSuffStats + kCategoricalMaxSymbols * s;
    double tot = 0.0;
    for (int v = 0; v < V; ++v) tot = tot + cnt[v];
    if (tot > 0.0)
        for (int v = 0; v < V; ++v) {
            const double p = cnt[v] / tot;
            E[s * V + v] = p >= floor ? p : floor;
        }
}

struct BatchRetableCategoricalArgs {
    const BatchProblem* prob;                  // [B]: T_b
    const int64_t* first;                      // [B]: problem b's first observe in obs
    const double* emission;                    // [B][k][V]
    const double* trans;                       // [B][k][k]
    const double* obs;                         // the observes, packed problem after problem
    double* tab;                               // [B][T_max][kBatchTab]
    uint64_t* thr;                             // [B][64]
    int32_t* status;                           // [B]: 0, or the bits of categorical_check
    double* e_out;                             // [B][8][64]: the matrix in force (slots outside the table 0.0)
    double* log_e_out;                         // [B][8][64]: its logarithms (slots outside the table -inf)
    int T_max, k, V;
};

static_assert(kCategoricalSlots == 2 * kThreads, "a thread of the re-table stages two slots of the emission matrix");

__global__ __launch_bounds__(kThreads) void batch_retable_categorical_kernel(BatchRetableCategoricalArgs a)
{
#pragma clang fp contract(off)
    __shared__ double s_trans[64];                              // the problem's transition rows, [k][k]
    __shared__ double s_log[kCategoricalSlots];                 // logE transposed: entry (s, v) at 8 v + s
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, k = a.k, V = a.V;
    // the thread's two slots: (s0, v) and (s0 + 4, v)
    const int s0 = tid >> 6, s1 = s0 + 4, v = tid & 63;
    const bool in0 = s0 < k && v < V, in1 = s1 < k && v < V;
    const double* E = a.emission + (int64_t)b * k * V;
    const double e0 = in0 ? E[s0 * V + v] : 0.0, e1 = in1 ? E[s1 * V + v] : 0.0;
    int bits = 0;
    if ((in0 && categorical_bad(e0)) || (in1 && categorical_bad(e1))) bits |= kRetableBadProb;
    if (tid < k * k) {
        const double w = a.trans[(int64_t)b * k * k + tid];
        s_trans[tid] = w;
        if (!(w >= 0.0) || !(fabs(w) < INFINITY)) bits |= kRetableBadWeight;
    }
    __syncthreads();
    if (tid < k) {
        double tot = 0.0;
        for (int j = 0; j < k; ++j) tot += s_trans[tid * k + j];
        if (!(tot > 0.0)) bits |= kRetableNoMass;
    }
    // (__syncthreads_or joins a predicate, not a word: one call a bit; uniform from here on)
    bits = (__syncthreads_or(bits & kRetableBadWeight) ? kRetableBadWeight : 0) | (__syncthreads_or(bits & kRetableNoMass) ? kRetableNoMass : 0) |
           (__syncthreads_or(bits & kRetableBadProb) ? kRetableBadProb : 0);
    if (blockIdx.y == 0 && tid == 0) a.status[b] = bits;
    if (bits) return;
    const double l0 = in0 ? table_log(e0) : -INFINITY, l1 = in1 ? table_log(e1) : -INFINITY;
    s_log[8 * v + s0] = l0;
    s_log[8 * v + s1] = l1;
    if (blockIdx.y == 0) {
        const int64_t at = (int64_t)b * kCategoricalSlots;
        a.e_out[at + tid] = e0; a.e_out[at + kThreads + tid] = e1;
        a.log_e_out[at + tid] = l0; a.log_e_out[at + kThreads + tid] = l1;
        if (tid < 64) a.thr[(int64_t)b * 64 + tid] = retable_threshold(s_trans, k, tid >> 3, tid & 7);
    }
    __syncthreads();
    const int s = tid & 7;
    const int64_t T = a.prob[b].T, stride = (int64_t)gridDim.y * kRetableRows;
    const double* y = a.obs + a.first[b];
    double* rows = a.tab + (int64_t)b * a.T_max * kBatchTab;
    for (int64_t t = (int64_t)blockIdx.y * kRetableRows + (tid >> 3); t < T; t += stride)
        rows[t * kBatchTab + s] = categorical_entry(y[t], V, s_log + s, 8);     // (s >= k: the slot holds -inf)
}

struct BatchSymbolStatsArgs {
    const BatchSmoothProblem* desc;            // [B]: T, rows (first row in the m table) and trows (first observe: the lengths before it)
    const double* mass;                        // the m table the counting pass left
    const uint64_t* thr;                       // as BatchSmoothArgs::thr
    const double* obs;                         // the observes (symbols held in doubles) packed problem after problem
    double* stats;                             // [B][kSymbolStats]
    int B, k, V, thr_stride;
};

// step t's addition: the lanes (v', s) with v' == (c & 7) add g to the accumulator c >> 3; c < 0 adds to no bin
__device__ __forceinline__ void symbol_count(double (&cnt)[8], int c, int vp, double g)
{
#pragma clang fp contract(off)
    const bool mine = c >= 0 && vp == (c & 7);
    const int hi = c >> 3;
#pragma unroll
    for (int i = 0; i < 8; ++i) cnt[i] = (mine && hi == i) ? cnt[i] + g : cnt[i];
}

__global__ __launch_bounds__(kThreads) void batch_symbol_stats_kernel(BatchSymbolStatsArgs a)
{
#pragma clang fp contract(off)
    const int lane = lane_id(), sp = lane >> 3, s = lane & 7;
    for (int b = suff_uniform((int)blockIdx.x * kWaves + wave_id()); b < a.B; b += (int)gridDim.x * kWaves) {   // (wavefront-uniform)
        const BatchSmoothProblem d = a.desc[b];
        double* out = a.stats + (int64_t)b * kSymbolStats;
        const int T = d.T;
        double xi = 0.0, occ = 0.0, occ_y = 0.0, occ_yy = 0.0;
        double cnt[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) cnt[i] = 0.0;
        if (T > 0) {
            const double* mass = a.mass + d.rows * 8;
            const double* y = a.obs + d.trows;
            const double p = smooth_trans_mass(a.thr + (int64_t)b * a.thr_stride, a.k, s, sp);
            double g = smooth_marginal_start(mass + (int64_t)(T - 1) * 8, s);
            double yt = y[T - 1];
            int ct = suff_uniform(categorical_symbol(yt, a.V));
            occ = occ + g;
            occ_y = occ_y + dmul_rn(g, yt);
            occ_yy = occ_yy + dmul_rn(g, dmul_rn(yt, yt));
            symbol_count(cnt, ct, sp, g);
            // the row, the observe and the symbol of the step to come (T = 1: row 0 once more, never used)
            int tn = T - 2 > 0 ? T - 2 : 0;
            double m[8];
            double mt = smooth_load_row(mass + (int64_t)tn * 8, s, m);
            yt = y[tn];
            ct = suff_uniform(categorical_symbol(yt, a.V));
            for (int t = T - 2; t >= 0; --t) {
                double mc[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) mc[j] = m[j];
                const double mtc = mt, yc = yt;
                const int cc = ct;
                tn = t > 0 ? t - 1 : 0;                             // (step 0 loads its own row again: in bounds, never used)
                mt = smooth_load_row(mass + (int64_t)tn * 8, s, m);
                yt = y[tn];
                ct = suff_uniform(categorical_symbol(yt, a.V));
                const double term = smooth_marginal_term(mtc, mc, p, g, sp);
                xi = xi + term;
                g = smooth_marginal_sum(term, s);
                occ = occ + g;
                occ_y = occ_y + dmul_rn(g, yc);
                occ_yy = occ_yy + dmul_rn(g, dmul_rn(yc, yc));
                symbol_count(cnt, cc, sp, g);
            }
        }
        out[8 * s + sp] = xi;
        if (sp == 0) { out[64 + s] = occ; out[72 + s] = occ_y; out[80 + s] = occ_yy; }
        // lane (v', s) holds cnt[s][8 i + v']; states >= k are zero
#pragma unroll
        for (int i = 0; i < 8; ++i) out[kSuffStats + kCategoricalMaxSymbols * s + 8 * i + sp] = s < a.k ? cnt[i] : 0.0;
    }
}

struct BatchMstepCategoricalArgs {
    const double* stats;                       // [B][kSymbolStats]
    double* emission;                          // [B][k][V]
    double* trans;                             // [B][k][k]
    double floor;
    int64_t B;
    int k, V;
};

// one thread a (problem, state s < k)
__global__ __launch_bounds__(kThreads) void batch_mstep_categorical_kernel(BatchMstepCategoricalArgs a)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + (int64_t)threadIdx.x;
    if (i >= a.B * a.k) return;
    const int64_t b = i / a.k;
    categorical_mstep(a.stats + b * kSymbolStats, a.k, a.V, (int)(i % a.k), a.emission + b * a.k * a.V, a.trans + b * a.k * a.k, a.floor);
}

}  // namespace cph
