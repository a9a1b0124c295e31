// Posterior traces of a batch: the surviving lineages of EVERY problem of the batch last run, resolved in ONE launch
// (cpprob_hip_batch_paths, _paths_device).  It reads what batch_smc_kernel left -- the problems' rows of values / anc and the
// per-step tables -- and writes nothing of it, so it serves uniform, described and online batches alike and leaves that kernel alone.
//
// Per final particle i < m_b of problem b (T_b = its current length, rows n_b apart from store_b on, as batch_smc_kernel addresses them):
//   p = i;  for t = T_b - 1 .. 0:  out[first_b + t m_b + i] = values[store_b + t n_b + p];  if t > 0: p = anc[store_b + t n_b + p]
//   logw[wfirst_b + i] = tab[(b T_max + T_b - 1) kBatchTab + values[store_b + (T_b - 1) n_b + i]]
// (anc row t holds generation t's ancestors in generation t - 1: the walk of batch_smc_kernel's own read-out, without its sums).
// m_b = n_b, or min(n_b, max_particles): the device form of Options::dump_max_particles.  The output is packed problem after problem
// (cpprob_hip_batch_paths_layout); a problem of length 0 -- an online batch's -- owns nothing.
//
// Work items are (problem, tile of kTile final particles): blockIdx.x the problem, blockIdx.y the tile, so a few 8192-particle
// problems still spread over eight workgroups each.  A workgroup's scalars come from its problem's descriptor (one scalar load);
// tiles past m_b return at once.  A lane owns particles tid, tid + 256, ... of its tile -- kPPT independent chains of dependent
// gathers -- so consecutive lanes write consecutive bytes of every output row.  The rows gathered from are at most 8 KiB (values)
// and 32 KiB (anc): they stay in L2 between the lanes that hit them.  Byte stores: row t of a problem starts at first_b + t m_b,
// which is 4-byte aligned only by accident.
#pragma once
#include "batch_smc.hpp"

namespace cph {

// Problem b as the walk needs it: the host writes these from the lengths it holds (an online batch's change with every advance).
struct BatchPathsProblem { int32_t T, n, m, pad_; int64_t store, first, wfirst; };
static_assert(sizeof(BatchPathsProblem) == 40, "one problem's paths descriptor");

struct BatchPathsArgs {
    const BatchPathsProblem* desc;             // [B]
    const int8_t* values; const int32_t* anc;  // the batch's particle store
    const double* tab;                         // [B][T_max][kBatchTab]
    int8_t* paths;                             // packed: problem b's [T_b][m_b] from desc[b].first on
    double* logw;                              // packed: problem b's [m_b] from desc[b].wfirst on; nullptr: not wanted
    int T_max;
};

__global__ __launch_bounds__(kThreads) void batch_paths_kernel(BatchPathsArgs a)
{
    const int b = (int)blockIdx.x, tid = threadIdx.x;
    const BatchPathsProblem d = a.desc[b];                      // workgroup-uniform
    const int i0 = (int)blockIdx.y * kTile;
    if (d.T <= 0 || i0 >= d.m) return;                          // nothing reached yet, or a tile past this problem's particles
    const int8_t* vals = a.values + d.store;
    const int32_t* anc = a.anc + d.store;
    int8_t* out = a.paths + d.first;
    // A lane past m_b walks particle 0 and stores nothing: with every load unconditional the kPPT chains' gathers of a step are in
    // flight together (guarded by `i < m`, each chain waited for its own loads before the next one issued).
    int p[kPPT];
    bool live[kPPT];
#pragma unroll
    for (int k = 0; k < kPPT; ++k) { const int i = i0 + k * kThreads + tid; live[k] = i < d.m; p[k] = live[k] ? i : 0; }
    if (a.logw) {
        const double* row = a.tab + ((int64_t)b * a.T_max + (d.T - 1)) * kBatchTab;
        const int8_t* fin = vals + (int64_t)(d.T - 1) * d.n;
        double w[kPPT];
#pragma unroll
        for (int k = 0; k < kPPT; ++k) w[k] = row[fin[p[k]] & (kBatchTab - 1)];
#pragma unroll
        for (int k = 0; k < kPPT; ++k) if (live[k]) a.logw[d.wfirst + p[k]] = w[k];
    }
    for (int t = d.T - 1; t >= 0; --t) {
        const int8_t* vrow = vals + (int64_t)t * d.n;
        const int32_t* arow = anc + (int64_t)t * d.n;
        int8_t* orow = out + (int64_t)t * d.m + i0 + tid;
        int8_t v[kPPT];
        int32_t q[kPPT];
#pragma unroll
        for (int k = 0; k < kPPT; ++k) { v[k] = vrow[p[k]]; q[k] = arow[p[k]]; }      // (row 0 of anc exists: read, then unused)
#pragma unroll
        for (int k = 0; k < kPPT; ++k) {
            if (live[k]) orow[k * kThreads] = v[k];
            // (an ancestor is an index into the problem's own row: the clamp keeps a damaged store from sending the walk elsewhere)
            p[k] = (int)min((uint32_t)q[k], (uint32_t)(d.n - 1));
        }
    }
}

}  // namespace cph
