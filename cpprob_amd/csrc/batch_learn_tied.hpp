// Tied online EM (cpprob_hip_batch_learn_tie): the streams of a group (cpprob_hip_batch_tie) learn ONE table on the device while their
// observes arrive.  A tied learning advance enqueues, behind the rows kernel and the run, three launches:
//   learn   batch_learn_kernel / batch_learn_scaled_kernel (csrc/batch_learn.hpp) with t_min = INT32_MAX: its steps (a) and (b) -- every
//           problem's discounted push and its record --, never its step (c);
//   pool    batch_pool_stats_kernel (csrc/batch_pool.hpp), compact, R = 1: pooled[g][e] = ((0.0 + rec[b_0][e]) + rec[b_1][e]) + ... over
//           the group's members in ascending problem order.  Every stream's record is a convex running average, so the streams of a
//           group weigh equally whatever their lengths (a member of length 0 contributes 88 zeros); weighting by length is not built;
//   tied    the kernels of this file: the group's M-step on pooled[g], its check, and the broadcast of the new table.
//
// One wavefront a group, kWaves groups a workgroup, the grid ceil(G / kWaves): no striding, no result that depends on the grid.  The
// member list is read through `members` and `first` of the tie, as csrc/batch_pool.hpp reads it.  Group g FIRES in this advance iff
//   some member received observes in it (desc[b].lo < desc[b].T), and
//   the group has seen at least t_min observes in all (the members' desc[b].T, summed in 64 bits, >= t_min);
// lane l looks at the members first[g] + l, + 64, ..., and two wavefront sums decide.  A group that does not fire keeps its tables, its
// words and its status words untouched.
// A firing group runs step (c) of batch_learn_body in its register-and-shuffle form -- lane (s, j) = 8 s + j holds xi[s][j] =
// pooled[g][8 s + j] and forms retable_mstep's row total with eight shuffles and its entry trans'[s][j]; lane (., c) holds state c's
// mean and, kScaled, its sigma and log_norm (scale_sigma, scale_bad, scale_log_norm) -- starting from the table of the group's FIRST
// member (the members of a group hold equal tables: cpprob_hip_batch_learn_tie checks it and nothing else writes them), then
// retable_check's predicates on the new table and bit 8 for a refused sigma:
//   no bit set:  member by member, the k^2 weights (lanes 0 .. k^2 - 1: the entries are moved there by one shuffle, so a member's
//                table is stored by consecutive lanes), the k means (lanes 0 .. k - 1), kScaled and fit != 0: the sigmas and log_norms,
//                the 64 threshold words (lane l word l, retable_threshold on the new row) and status = 0 (lane 0);
//   a bit set:   nothing but the bits, in every member's status word.
// fit == 0 on a scaled batch: sigmas and log_norms are read, checked and never written.
// The first member's table is read by lanes other than those that store it; the shuffles between the loads and the stores need every
// lane's loaded value, so no store of the wavefront leaves before its last load has returned, and no other wavefront touches the group.
// Nothing is contracted, no LDS, no barrier, no atomics; the only logarithm is table_log's, through scale_log_norm.
// tests/learn_tied_ref.py restates it; tests/host_kernels/batch_learn_tied_main.cpp runs this text on the host.
#pragma once
#include "batch_learn.hpp"
#include "batch_pool.hpp"

namespace cph {

struct BatchLearnTiedArgs {
    const int32_t* members;                    // [B]: the problems sorted by (group, problem)
    const int32_t* first;                      // [G + 1]: group g's members are members[first[g] .. first[g + 1])
    const BatchSmoothProblem* desc;            // [B]: the learn launch's descriptors -- T (the length reached), lo (the length before)
    const double* pooled;                      // [G][kPoolStats]
    uint64_t* thr;                             // [B][64]
    double* means;                             // [B][k]
    double* trans;                             // [B][k][k]
    int32_t* status;                           // [B]
    int64_t t_min;
    int G, k;
};

struct BatchLearnTiedScaledArgs {
    BatchLearnTiedArgs base;                   // batch_learn_tied_kernel's arguments
    double* sigmas;                            // [B][8]
    double* log_norms;                         // [B][8]
    double floor;                              // the scales' floor (fit != 0)
    int fit;                                   // the learner fits the scales
};

// Args: BatchLearnTiedArgs, or kScaled: BatchLearnTiedScaledArgs
template <bool kScaled, class Args>
__device__ __forceinline__ void batch_learn_tied_body(Args sa)
{
#pragma clang fp contract(off)
    BatchLearnTiedArgs a;
    if constexpr (kScaled) a = sa.base; else a = sa;
    const int lane = lane_id(), sp = lane >> 3, c = lane & 7, k = a.k;
    const bool live = sp < k;
    const int g = pool_uniform((int)blockIdx.x) * kWaves + pool_uniform(wave_id());          // (wavefront-uniform)
    if (g >= a.G) return;
    const int lo = a.first[g], hi = a.first[g + 1];                                         // (a group has a member: lo < hi)
    // the firing rule
    uint64_t fed = 0, seen = 0;
    for (int i = lo + lane; i < hi; i += kWave) {
        const BatchSmoothProblem d = a.desc[a.members[i]];
        if (d.lo < d.T) fed += 1;
        if (d.T > 0) seen += (uint64_t)d.T;
    }
    fed = wave_sum_u64(fed);
    seen = wave_sum_u64(seen);
    if (fed == 0 || (int64_t)seen < a.t_min) return;                                        // (uniform)
    // the M-step: every lane (., c) holds pooled[g][8 i + c] in o[i]; the table is the first member's
    const int b0 = a.members[lo];
    const double* rec = a.pooled + (int64_t)g * kPoolStats;
    double o[kOnlineCols];
#pragma unroll
    for (int i = 0; i < kOnlineCols; ++i) o[i] = rec[8 * i + c];
    const bool entry = live && c < k;
    double xi = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) xi = i == sp ? o[i] : xi;
    double rsum = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const double x = __shfl(xi, sp * 8 + j); if (j < k) rsum = rsum + x; }
    double tr = entry ? a.trans[(int64_t)b0 * k * k + sp * k + c] : 0.0;
    if (rsum > 0.0) tr = entry ? xi / rsum : 0.0;
    double mean = c < k ? a.means[(int64_t)b0 * k + c] : 0.0;
    if (o[8] > 0.0) mean = c < k ? o[9] / o[8] : 0.0;
    double sigma = 1.0, log_norm = 0.0;
    int bad_scale = 0;
    if constexpr (kScaled) {
        sigma = c < k ? sa.sigmas[(int64_t)b0 * 8 + c] : 1.0; log_norm = c < k ? sa.log_norms[(int64_t)b0 * 8 + c] : 0.0;
        const bool fitted = sa.fit != 0 && c < k && o[8] > 0.0;
        if (fitted) sigma = scale_sigma(o[8], o[10], mean, sa.floor);
        bad_scale = c < k && scale_bad(sigma) ? kRetableBadScale : 0;
        if (fitted && !bad_scale) log_norm = scale_log_norm(sigma);
    }
    // the new row s' on each of its lanes, its bits, every row's bits
    double row[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) row[j] = __shfl(tr, sp * 8 + j);
    const double mean_row = __shfl(mean, sp);                   // (the mean of state s': lane (0, s') holds it)
    int bad_row = 0;
    if constexpr (kScaled) bad_row = __shfl(bad_scale, sp);      // (every lane takes part: the shuffle stands outside `live`)
    const int mine = live ? learn_row_bits(row, mean_row, k) | bad_row : 0;
    int bits = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) bits |= __shfl(mine, s * 8);
    if (bits) {                                                 // (uniform: the old tables, scales and words stay with every member)
        for (int i = lo + lane; i < hi; i += kWave) a.status[a.members[i]] = bits;
        return;
    }
    // the broadcast: lane l < k^2 takes entry l of the table [k][k], so that a member's stores stand on consecutive lanes
    const int kk = k * k;
    const double packed = __shfl(tr, lane < kk ? (lane / k) * 8 + lane % k : lane);
    const uint64_t word = live ? retable_threshold(row, k, 0, c) : ~0ull;          // (the row alone is row 0 of retable_threshold's table)
    for (int i = lo; i < hi; ++i) {
        const int b = a.members[i];                             // (uniform)
        if (lane < kk) a.trans[(int64_t)b * kk + lane] = packed;
        if (lane < k) a.means[(int64_t)b * k + lane] = mean;
        if constexpr (kScaled) if (sa.fit != 0 && lane < k) { sa.sigmas[(int64_t)b * 8 + lane] = sigma; sa.log_norms[(int64_t)b * 8 + lane] = log_norm; }
        a.thr[(int64_t)b * 64 + lane] = word;
        if (lane == 0) a.status[b] = 0;
    }
}

__global__ __launch_bounds__(kThreads) void batch_learn_tied_kernel(BatchLearnTiedArgs a)
{
#pragma clang fp contract(off)
    batch_learn_tied_body<false>(a);
}

__global__ __launch_bounds__(kThreads) void batch_learn_tied_scaled_kernel(BatchLearnTiedScaledArgs sa)
{
#pragma clang fp contract(off)
    batch_learn_tied_body<true>(sa);
}

}  // namespace cph
