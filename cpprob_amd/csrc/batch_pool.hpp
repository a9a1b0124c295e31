// Pooled sufficient statistics of a tied batch (cpprob_hip_batch_pool_stats, _pool_stats_device): the problems of a begun batch that share
// one table (cpprob_hip_batch_tie: a partition of the problems into groups) have their records summed, so that the unchanged M-step fits
// one table a group.  The record is additive over sequences: xi, occ, occ_y and occ_yy of a collection are the sums of its sequences'.
//
// Records [B][R][88] (R = 1: cpprob_hip_batch_smooth_stats, _online_stats; R = n_traj: _traj_stats).  For a group g with the members
// b_0 < b_1 < ..., every r < R and every entry e < 88:
//   pooled[g][r][e] = (((0.0 + rec[b_0][r][e]) + rec[b_1][r][e]) + ...)
// one addition a member, in ascending problem order, from 0.0, nothing contracted; all 88 entries whatever the batch's k.  Compact:
// out [G][R][88]; broadcast: out [B][R][88], every member of g receives pooled[g] -- out may then be the records themselves.
// cpprob_amd.em.pool_stats states it in numpy, tests/pool_ref.py in plain Python.
//
// One wavefront a (group, r) pair, kWaves pairs a workgroup, the grid ceil(G R / kWaves): no striding, no result that depends on the
// grid.  Lane e keeps entry e in a register, the lanes below 24 also entry 64 + e (the others read their own entry e once more and drop
// it: no lane reads what another writes); a record is 704 consecutive bytes.  The pair is made wavefront-uniform for the compiler, so
// the member list is read through scalar loads.  The additions are a serial chain the loads do not depend on: the records of kPoolAhead
// members are in flight while the chain consumes them in order, the member indices of the block behind those are loaded a block earlier
// still, and every load is unconditional (past the group's end: its last member once more, never added) so that the waits count.  In
// broadcast mode a lane stores only after it has read its entries of every member, which is what makes the in-place form safe; pairs
// touch disjoint records.  No LDS, no barrier, no atomics.
#pragma once
#include "batch_smc.hpp"

namespace cph {

constexpr int kPoolStats = 88;                      // doubles a record: xi[8][8], occ[8], occ_y[8], occ_yy[8]
constexpr int kPoolAhead = 6;                       // members whose records are in flight ahead of the chain of additions

struct BatchPoolArgs {
    const int32_t* members;                    // [B]: the problems sorted by (group, problem)
    const int32_t* first;                      // [G + 1]: group g's members are members[first[g] .. first[g + 1])
    const double* rec;                         // [B][R][kPoolStats]
    double* out;                               // compact [G][R][kPoolStats]; broadcast [B][R][kPoolStats] (may be rec)
    int64_t pairs;                             // G R
    int R, broadcast;
};

// v, which every lane of the wavefront holds alike, as a value the compiler knows to be uniform
__device__ __forceinline__ int pool_uniform(int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

__global__ __launch_bounds__(kThreads) void batch_pool_stats_kernel(BatchPoolArgs a)
{
#pragma clang fp contract(off)
    const int lane = lane_id();
    const int64_t pair = (int64_t)pool_uniform((int)blockIdx.x) * kWaves + pool_uniform(wave_id());      // (wavefront-uniform)
    if (pair >= a.pairs) return;
    const int g = (int)(pair / a.R), r = (int)(pair % a.R);
    const int lo = a.first[g], hi = a.first[g + 1], last = hi - 1;              // (a group has a member: lo <= last)
    const int e1 = lane < 24 ? 64 + lane : lane;
    const int64_t at = (int64_t)r * kPoolStats;
    const int64_t stride = (int64_t)a.R * kPoolStats;
    // the records of the first kPoolAhead members and the indices of the kPoolAhead behind them
    double v0[kPoolAhead], v1[kPoolAhead];
    int nxt[kPoolAhead];
#pragma unroll
    for (int j = 0; j < kPoolAhead; ++j) {
        const int i = lo + j < last ? lo + j : last;
        const double* p = a.rec + (int64_t)a.members[i] * stride + at;
        v0[j] = p[lane];
        v1[j] = p[e1];
    }
#pragma unroll
    for (int j = 0; j < kPoolAhead; ++j) {
        const int i = lo + kPoolAhead + j < last ? lo + kPoolAhead + j : last;
        nxt[j] = a.members[i];
    }
    double s0 = 0.0, s1 = 0.0;
    for (int base = lo; base < hi; base += kPoolAhead) {
#pragma unroll
        for (int j = 0; j < kPoolAhead; ++j) {
            const double c0 = v0[j], c1 = v1[j];
            const double* p = a.rec + (int64_t)nxt[j] * stride + at;
            v0[j] = p[lane];
            v1[j] = p[e1];
            const int i = base + 2 * kPoolAhead + j < last ? base + 2 * kPoolAhead + j : last;
            nxt[j] = a.members[i];
            const bool member = base + j < hi;                                  // (uniform)
            s0 = member ? s0 + c0 : s0;
            s1 = member ? s1 + c1 : s1;
        }
    }
    if (!a.broadcast) {
        double* q = a.out + pair * kPoolStats;
        q[lane] = s0;
        if (lane < 24) q[64 + lane] = s1;
        return;
    }
    for (int i = lo; i < hi; ++i) {
        double* q = a.out + (int64_t)a.members[i] * stride + at;
        q[lane] = s0;
        if (lane < 24) q[64 + lane] = s1;
    }
}

}  // namespace cph
