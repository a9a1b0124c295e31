// Batched SMC: B independent every-step SMC problems of the table-weight HMMs in ONE launch, one workgroup per problem.
//
// Each problem is what a one-context run begun with its own seed (particle_offset 0, run_index 0) computes: same Philox counters
// (particle ids 0..n-1), same arithmetic -- the prefix-count form of step_counts.hpp for CPPROB_HIP_MODEL_HMM3, the fixed-point form
// of step_fixed.hpp for CPPROB_HIP_MODEL_HMM_TABLE -- so its ancestors are the oracle's and its statistics the single path's.  The
// difference is where the population lives: n <= kBatchMaxN particles fit one workgroup's LDS, so a generation's totals are one
// workgroup reduction, the comb is one workgroup scan, and no hierarchy, atomic or second launch sits between two steps.
//
// A step, workgroup-wide, with barriers between the phases:
//   draw      particle i (lane-owned runs of 4, passes of 1024) takes its ancestor's state from LDS, draws its new state (Model::draw4 /
//             apply4: ids 0..n-1) and leaves it in the other LDS state buffer (keep_history: also in the problem's rows in HBM)
//   count     the per-state counts of the generation: one packed 64-bit wavefront sum per 4 states, one LDS word per wavefront
//   books     every thread derives the generation's totals from the counts; thread 0 keeps the books with the single path's own
//             functions (counts_step_bookkeep / counts_final_bookkeep; fixed_decide / fixed_bookkeep).  HMM_TABLE: the reference is the
//             step's bound B_t, or the exact maximum when that sits more than kFixGapLimit nats below it -- the repair the single path
//             does with extra launches (settle_fixed) is this branch, counted in n_requantised
//   comb      the inclusive prefix (packed state counts, or 64-bit masses of the fixed-point weights) by a wavefront scan a pass; lane
//             k's first output G_k (TableCdf::first / FixedCdf::first) marks a slot; a prefix maximum over the slots leaves every
//             output's ancestor in LDS, where the next step's draw reads it
// After the last step the read-out runs in the same workgroup: the lineage walk over the problem's rows (keep_history = 1; integer
// sums per predict hit, trace_stat's evaluation for HMM3) or nothing (filtering: the books wrote every row).  Workgroups never wait
// on each other.  LDS: 4 bytes of ancestor + 2 bytes of state per particle (48 KiB at n = 8192), so the limit is an LDS limit.
//
// Two kinds of batch run through it; they differ only in where a workgroup's scalars come from (BatchArgs).  Uniform
// (cpprob_hip_batch_begin): workgroup i runs problem i, every problem has T_max steps and n particles, the thresholds are one table and
// the particle store is [B][T_max][n].  Described (cpprob_hip_batch_begin_problems): workgroup i runs problem order[i] (the longest
// chains first) with the T, n and packed store offset of its BatchProblem and, for HMM_TABLE, its own thresholds.  Either way problem b
// owns rows b T_max + t of the small per-step regions (tab, stats, ess, resampled), of which a described problem writes its first T_b.
// The launch's dynamic LDS is batch_lds_bytes of the batch's largest n; each workgroup carves it by its own npad.
//
// A third kind is advanced in pieces (cpprob_hip_batch_begin_online / _advance): a launch runs steps [first[b], prob[b].T) of problem
// b, and what it leaves equals a one-shot run of prob[b].T steps bit for bit.  In the shorter run generation first - 1 was final (no
// resampling, the final books); now it is an ordinary one.  So a resumed workgroup enters the step loop one generation early, at
// t = first - 1, with the draw replaced by a reload of that generation's states (row first - 1 of its values, or its carry region in
// a filtering batch) and the books' running values (log_z, n_resampled, fix_gap, first_bad, n_requantised) put back to what they were
// before that generation's final books (BatchSnap, written where every piece ends).  Count, books, comb and prefix maximum of the
// reloaded generation are then the loop's own, in the resampling form, with the junction's own Philox draw.  A piece without steps
// (first = T) re-keeps the final books, to the same values, on its way to the read-out; without a read-out to do (first = -1: the
// host knows the problem's statistics are those of its length) it returns at once.
#pragma once
#include "step_counts.hpp"
#include "step_fixed.hpp"

namespace cph {

constexpr int kBatchMaxN = 8192;              // particles per problem (the 16-bit packed state counts would reach 65535)
constexpr int kBatchTab = 8;                  // doubles per (problem, step) in the table: HMM3 {ll_0..2, e_0..2, max ll, 0}, HMM_TABLE ll_0..7
constexpr int kBatchCtrlBytes = 256;          // one problem's StepCtrl, padded
static_assert(sizeof(StepCtrl) <= kBatchCtrlBytes, "a problem's control block");

__host__ __device__ inline int64_t batch_lds_bytes(int64_t n) { const int64_t np = (n + kTile - 1) / kTile * kTile; return np * 6; }

// A described problem: its length, its particle count and the first of its T * n entries in the packed values / anc.
struct BatchProblem { int32_t T, n; int64_t store; };
static_assert(sizeof(BatchProblem) == 16, "one problem's descriptor");

// What generation T - 1's final books overwrite, as it stood before them: where the next piece resumes.
struct BatchSnap { double log_z, fix_gap; int32_t n_resampled, first_bad, n_requant, pad_; };
static_assert(sizeof(BatchSnap) == 32, "one problem's snapshot");

struct BatchArgs {
    ModelParams mp;                            // HMM3: hmm_thr; HMM_TABLE: hk (the thresholds are `thr`: mp.hk_thr is not read)
    const double* tab;                         // [B][T_max][kBatchTab]
    const uint64_t* seeds;                     // [B]
    const uint64_t* thr;                       // HMM_TABLE: problem b's 64 words at thr + b * thr_stride, the layout of ModelParams::hk_thr
    const BatchProblem* prob;                  // [B], described batch; nullptr: uniform
    const int32_t* order;                      // [B], described batch: workgroup i runs problem order[i]
    int8_t* values; int32_t* anc;              // keep_history: [B][T_max][n] (uniform) or packed by prob[b].store; else nullptr
    char* ctrl;                                // [B] control blocks of kBatchCtrlBytes
    double* stats; double* ess; int32_t* resampled;   // [B][T_max][spp], [B][T_max], [B][T_max]
    int32_t* n_requant;                        // [B]
    int T_max, n;                              // T_max: rows a problem holds in the small regions; uniform: every problem's T = T_max and n
    int thr_stride;                            // words: 0 (one shared table) or 64 (a table a problem)
    int spp;
    double ess_frac;
    // a batch advanced in pieces (the RESUME kernels; the others read none of these)
    const int32_t* first;                      // [B]: problem b's first step of this launch (its length before it); -1: nothing to do for it
    BatchSnap* snap;                           // [B]
    uint8_t* carry;                            // filtering: problem b's final generation, n bytes at carry + prob[b].store
    int skip_readout;                          // keep_history: 1 leaves the lineage walk to a later piece
    // a filtering batch that keeps the backward smoother's m table (CPPROB_HIP_BATCH_KEEP_MASSES: the MASS kernels; the others do not read it)
    double* mass;                              // [B][T_max][8]: row (b, t) at (b T_max + t) * 8, as tab; nullptr: not kept
};

// The m table of the backward smoother (csrc/batch_smooth.hpp), formed where a generation's counts stand: entry s of the row of a
// generation with per-state counts cnt and log-weights ll[0..k), m[s] = cnt[s] * fix_weight(ll[s], M), M the largest ll over the
// states with cnt > 0 -- the exact maximum, not the step's reference (the bound B_t unless the generation was requantised: q[s] of
// the step is another number whenever the bound-setting state is unoccupied).  batch_smooth_count_kernel's statement on the counts
// it re-derives from the store; the two agree bit for bit.  (cnt is indexed by constants only: it lives in registers.)
__host__ __device__ inline double batch_mass(const uint32_t (&cnt)[8], const double* ll, int k, int s)
{
    double M = -INFINITY;
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < k && cnt[j]) M = fmax(M, ll[j]);
        mine = j == s ? cnt[j] : mine;
    }
    return s < k ? u64_to_double((uint64_t)mine * fix_weight(ll[s], M)) : 0.0;
}
// ... and the whole row m[0..8), states >= k zero
__host__ __device__ inline void batch_mass_row(const uint32_t (&cnt)[8], const double* ll, int k, double* out)
{
    for (int s = 0; s < 8; ++s) out[s] = batch_mass(cnt, ll, k, s);
}

__device__ __forceinline__ uint32_t batch_sel8(const uint32_t (&q)[8], int s)
{
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) r = s == j ? q[j] : r;
    return r;
}

// RESUME: the kernel of a batch advanced in pieces.  (A template parameter, not a run-time switch on a.first: with the switch the two
// <HMM3, KEEP> kernels of the one-shot batches reserved a 68-byte private segment -- profiles/r12_notes.md, "Kernel resources".)
// MASS: the kernel of a filtering batch that keeps the m table (KEEP = false only).  (A template parameter too: as a run-time switch
// on a.mass the eight filtering kernels took 5 .. 10 more VGPRs and up to twice the SGPR spills, and <HMM_TABLE, systematic> fell from
// five wavefronts a SIMD to four, for batches that never ask for the rows -- profiles/r18_notes.md, "Kernel resources".)
template <class Model, int RS, bool KEEP, bool RESUME = false, bool MASS = false>
__global__ __launch_bounds__(kThreads) void batch_smc_kernel(BatchArgs a)
{
    using V = typename Model::value_t;
    constexpr bool kCounts = Model::kWeightTable == 3;          // HMM3: prefix counts; HMM_TABLE: fixed-point masses
    extern __shared__ __attribute__((aligned(16))) double s_batch[];
    __shared__ uint64_t s_cnt[2][kWaves][2];                    // per-wavefront packed state counts (16 bits a state), by step parity
    __shared__ uint64_t s_scan[2][kWaves];                      // per-wavefront totals of a pass's scan, by pass parity
    __shared__ int32_t s_imax[2][kWaves];
    __shared__ unsigned long long s_rows[2][kTraceKeys];        // read-out (HMM3): the pair counts of hit t, then of hit T-1
    __shared__ uint64_t s_acc[2][kWaves][8];                    // read-out: per-wavefront sums of a hit
    const int tid = threadIdx.x, lane = lane_id(), wv = wave_id();
    // the problem this workgroup runs and its shape (workgroup-uniform: scalar loads and selects)
    const int b = a.order ? (int)a.order[blockIdx.x] : (int)blockIdx.x;
    const int n = a.prob ? (int)a.prob[b].n : a.n;
    const int T = a.prob ? (int)a.prob[b].T : a.T_max;
    const int t_first = RESUME ? (int)a.first[b] : 0;
    if (RESUME && (t_first < 0 || (t_first == T && (!KEEP || a.skip_readout)))) return;     // neither steps nor a read-out to do
    const int npad = (n + kTile - 1) / kTile * kTile, passes = npad / kTile;
    int32_t* A = reinterpret_cast<int32_t*>(s_batch);                                       // ancestors of the next generation (slots while the comb runs; paths in the read-out)
    uint8_t* S0 = reinterpret_cast<uint8_t*>(A + npad);
    uint8_t* S1 = S0 + npad;
    const double n_pop = (double)n;
    const int k_states = kCounts ? 3 : a.mp.hk;
    const uint64_t seed = a.seeds[b];
    const double* tab = a.tab + (int64_t)b * a.T_max * kBatchTab;
    StepCtrl* ctrl = reinterpret_cast<StepCtrl*>(a.ctrl + (int64_t)b * kBatchCtrlBytes);
    double* ess_b = a.ess + (int64_t)b * a.T_max;
    int32_t* res_b = a.resampled + (int64_t)b * a.T_max;
    double* st_b = a.stats + (int64_t)b * a.T_max * a.spp;
    // The problem's first entry in values / anc is formed where a row is addressed (a scalar load or multiply), not held across the
    // steps: held in registers, that 64-bit value made <HMM3, stratified, KEEP> reserve a 68-byte private segment
    // (profiles/r09_notes.md, "Kernel resources").
    auto store = [&]() -> int64_t { return a.prob ? a.prob[b].store : (int64_t)b * T * n; };
    int n_requant = 0;
    if (RESUME && t_first > 0) {
        const BatchSnap sn = a.snap[b];
        n_requant = sn.n_requant;
        if (tid == 0) { ctrl->lz_trace = nullptr; ctrl->first_bad = sn.first_bad; ctrl->log_z = sn.log_z; ctrl->n_resampled = sn.n_resampled; ctrl->fix_gap = sn.fix_gap; }
    } else if (tid == 0) { ctrl->lz_trace = nullptr; ctrl->first_bad = -1; ctrl->log_z = 0.0; ctrl->n_resampled = 0; ctrl->fix_gap = 0.0; }
    uint32_t q_fin[8] = {0, 0, 0, 0, 0, 0, 0, 0};              // HMM_TABLE: the final generation's weight of each state
    uint64_t S_fin = 0;
    // HMM_TABLE: the problem's 64 threshold words staged in LDS once; every draw reads its row there.  (Left in global memory
    // the same batch runs 6 % slower: profiles/r09_notes.md, "Threshold staging".)
    __shared__ uint64_t s_thr[kCounts ? 1 : 64];                // (HMM3: unused, and takes no LDS)
    if constexpr (!kCounts) { if (tid < 64) s_thr[tid] = a.thr[(int64_t)b * a.thr_stride + tid]; __syncthreads(); }
    for (int t = RESUME && t_first > 0 ? t_first - 1 : 0; t < T; ++t) {
        uint8_t* cur = (t & 1) ? S1 : S0;
        const uint8_t* prv = (t & 1) ? S0 : S1;
        // ---- draw (a resumed problem's first pass through the loop: generation first - 1 comes back from memory) ----
        uint64_t cA = 0, cB = 0;
        const bool reload = RESUME && t < t_first;
        for (int p = 0; p < passes; ++p) {
            const int i0 = p * kTile + tid * kPPT;
            if (i0 >= n) continue;
            if (reload) {
#pragma unroll
                for (int k = 0; k < kPPT; ++k) {
                    const int i = i0 + k;
                    if (i >= n) continue;
                    const int s = KEEP ? (int)a.values[store() + (int64_t)t * n + i] : (int)a.carry[store() + i];
                    cur[i] = (uint8_t)s;
                    cA += s < 4 ? 1ull << (16 * s) : 0ull;
                    cB += s >= 4 ? 1ull << (16 * (s - 4)) : 0ull;
                }
                continue;
            }
            V prev[kPPT], x[kPPT];
            int32_t an[kPPT];
#pragma unroll
            for (int k = 0; k < kPPT; ++k) {
                const int i = i0 + k;
                an[k] = (t == 0 || i >= n) ? i : A[i];
                prev[k] = (t == 0 || i >= n) ? (V)0 : (V)prv[an[k]];
            }
            typename Model::Rand r;
            Model::draw4(seed, (uint64_t)i0, t, r);
            if constexpr (!kCounts) {
                ModelParams mp_b = a.mp;                                  // the batch's parameters, hk_thr pointed at this problem's staged rows
                mp_b.hk_thr = s_thr;
                Model::apply4(mp_b, t, r, prev, x);
            } else Model::apply4(a.mp, t, r, prev, x);
#pragma unroll
            for (int k = 0; k < kPPT; ++k) {
                const int i = i0 + k;
                if (i >= n) continue;
                const int s = (int)x[k];
                cur[i] = (uint8_t)s;
                cA += s < 4 ? 1ull << (16 * s) : 0ull;
                cB += s >= 4 ? 1ull << (16 * (s - 4)) : 0ull;
                if (KEEP) { a.values[store() + (int64_t)t * n + i] = (int8_t)s; a.anc[store() + (int64_t)t * n + i] = an[k]; }
            }
        }
        // ---- count ----
        cA = wave_sum_u64(cA);
        cB = wave_sum_u64(cB);
        if (lane == 0) { s_cnt[t & 1][wv][0] = cA; s_cnt[t & 1][wv][1] = cB; }
        __syncthreads();
        uint64_t tA = 0, tB = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) { tA += s_cnt[t & 1][w][0]; tB += s_cnt[t & 1][w][1]; }
        uint32_t cnt[8];
#pragma unroll
        for (int s = 0; s < 4; ++s) { cnt[s] = (uint32_t)(tA >> (16 * s)) & 0xffffu; cnt[s + 4] = (uint32_t)(tB >> (16 * s)) & 0xffffu; }
        const bool resample = t + 1 < T;
        if (resample) for (int j = tid; j < n; j += kThreads) A[j] = -1;      // (every draw has read its ancestor: the barrier above)
        // ---- books ----
        const double* row = tab + (int64_t)t * kBatchTab;
        // the generation's row of the m table (a filtering batch that keeps it): the first eight lanes of wavefront 1, an entry each,
        // beside thread 0's books; no later phase reads it.  (A resumed problem's reloaded generation: the same values again.)
        if constexpr (MASS && !KEEP) {
            if (tid >= kWave && tid < kWave + 8) a.mass[((int64_t)b * a.T_max + t) * 8 + (tid - kWave)] = batch_mass(cnt, row, k_states, tid - kWave);
        }
        const uint64_t draw = kResampleDrawBase + (uint64_t)(t + 1);          // the resampling in front of step t + 1
        double u0 = 0.0;
        if (resample) { const u32x4 r = draw_block(seed, 0, draw); u0 = u01_53(r.x, r.y); }
        TableCdf tc;
        FixedCdf fc;
        uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (kCounts) {
            const double tot0 = (double)cnt[0], tot1 = (double)cnt[1];
            tc.e0 = row[3]; tc.e1 = row[4]; tc.e2 = row[5]; tc.n_pop = n_pop; tc.u0 = u0;
            tc.base0 = 0.0; tc.base1 = 0.0; tc.basev = 0.0;
            tc.seed = seed; tc.draw = draw; tc.uid0 = 0;
            const double W = tc.cdf(tot0, tot1, n_pop);
            tc.inv = n_pop / W;
            if (tid == 0) {
                if (resample) {
                    StepCountsArgs<Model> ca{};
                    ca.e_prev[3] = row[6]; ca.ctrl = ctrl; ca.n_pop = n_pop; ca.ess_trace = ess_b; ca.resampled = res_b;
                    ca.filter_stats = KEEP ? nullptr : st_b;
                    counts_step_bookkeep(ca, t + 1, tc, W, tot0, tot1);
                } else {
                    if (RESUME) { BatchSnap sn{}; sn.log_z = ctrl->log_z; sn.n_resampled = ctrl->n_resampled; sn.first_bad = -1; a.snap[b] = sn; }
                    CountsFinal f{};
                    f.e[0] = row[3]; f.e[1] = row[4]; f.e[2] = row[5]; f.e[3] = row[6];
                    f.n_pop = n_pop; f.T = T; f.bookkeep = 1; f.ctrl = ctrl; f.ess_trace = ess_b; f.resampled = res_b;
                    f.filter_stats = KEEP ? nullptr : st_b;
                    counts_final_bookkeep(f, tot0, tot1);
                }
            }
        } else {
            double bound = -INFINITY, M = -INFINITY;
            for (int s = 0; s < k_states; ++s) { bound = fmax(bound, row[s]); if (cnt[s]) M = fmax(M, row[s]); }
            double ref = fixed_reference(true, 0.0, bound);                   // every particle enters the step at log-weight 0
            const bool requant = ref - M > kFixGapLimit && M > -INFINITY;      // too few of the 32 bits left: weigh against the exact maximum
            if (requant) { ref = M; ++n_requant; }
            uint64_t S = 0, Q = 0;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                q[s] = s < k_states ? fix_weight(0.0 + row[s], ref) : 0u;
                S += (uint64_t)cnt[s] * q[s];
                Q += (uint64_t)cnt[s] * fix_square(q[s]);
            }
            const FixedDecision d = fixed_decide(S, Q, n_pop, a.ess_frac, resample);
            fc.inv = d.inv; fc.u0 = u0; fc.n_pop = n_pop; fc.base = 0; fc.seed = seed; fc.draw = draw; fc.uid0 = 0;
            if (tid == 0) {
                if (RESUME && !resample) {
                    BatchSnap sn{};
                    sn.log_z = ctrl->log_z; sn.fix_gap = ctrl->fix_gap; sn.n_resampled = ctrl->n_resampled; sn.first_bad = ctrl->first_bad;
                    sn.n_requant = n_requant - (requant ? 1 : 0);
                    a.snap[b] = sn;
                }
                ctrl->ref_cur = ref;
                fixed_bookkeep(ctrl, t, d, ref, n_pop, u0, ess_b, res_b, !resample, M);
                if (!KEEP) {
                    const double Sd = u64_to_double(S);
                    for (int s = 0; s < a.spp; ++s) st_b[(int64_t)t * a.spp + s] = s < k_states ? u64_to_double((uint64_t)cnt[s] * q[s]) / Sd : 0.0;
                }
            }
            if (!resample) {
#pragma unroll
                for (int s = 0; s < 8; ++s) q_fin[s] = q[s];
                S_fin = S;
            }
        }
        if (!resample) {
            if (RESUME && !KEEP && !reload) for (int j = tid; j < n; j += kThreads) a.carry[store() + j] = cur[j];   // what the next piece resumes from
            break;
        }
        // ---- comb: each source marks the first output it owns ----
        auto first_of = [&](uint64_t prefix, int upto) -> int {           // first output owned by the sources after `upto` particles
            double g;
            if constexpr (kCounts) g = tc.template first<RS>(tc.cdf((double)(uint32_t)(prefix & 0xffffu), (double)(uint32_t)(prefix >> 16), (double)upto));
            else g = fc.template first<RS>(prefix);
            return g < 0.0 ? 0 : (g > n_pop ? n : (int)g);
        };
        uint64_t carry = 0;
        for (int p = 0; p < passes; ++p) {
            const int i0 = p * kTile + tid * kPPT;
            uint64_t incl_k[kPPT];
            uint64_t run = 0;
#pragma unroll
            for (int k = 0; k < kPPT; ++k) {
                const int i = i0 + k;
                if (i < n) {
                    const int s = cur[i];
                    if constexpr (kCounts) run += s == 0 ? 1ull : (s == 1 ? 0x10000ull : 0ull);
                    else run += batch_sel8(q, s);
                }
                incl_k[k] = run;
            }
            const uint64_t incl = wave_incl_scan_u64(run);
            if (lane == kWave - 1) s_scan[p & 1][wv] = incl;
            __syncthreads();
            uint64_t off = carry, tot = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) { const uint64_t v = s_scan[p & 1][w]; if (w < wv) off += v; tot += v; }
            carry += tot;
            if (i0 < n) {
                const uint64_t excl = off + incl - run;
                int p_prev = first_of(excl, i0);
#pragma unroll
                for (int k = 0; k < kPPT; ++k) {
                    const int i = i0 + k;
                    if (i >= n) break;
                    const int pk = i + 1 == n ? n : first_of(excl + incl_k[k], i + 1);   // the population's last source owns the rest
                    if (pk > p_prev) { A[p_prev] = i; p_prev = pk; }
                }
            }
        }
        __syncthreads();
        // ---- inclusive prefix maximum over the slots: every output's ancestor ----
        int32_t carry_m = -1;
        for (int p = 0; p < passes; ++p) {
            const int i0 = p * kTile + tid * kPPT;
            int32_t v[kPPT];
#pragma unroll
            for (int k = 0; k < kPPT; ++k) v[k] = i0 + k < n ? A[i0 + k] : -1;
            lane_prefix_max(v);
            const int32_t incl = wave_incl_max_i32(v[kPPT - 1]);
            if (lane == kWave - 1) s_imax[p & 1][wv] = incl;
            int32_t excl = dpp_or_i32<0x138 /* wave_shr:1 */>(incl, -1);
            if (lane == 0) excl = -1;
            __syncthreads();
            excl = max(excl, carry_m);
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const int32_t m = s_imax[p & 1][w];
                if (w < wv) excl = max(excl, m);
                carry_m = max(carry_m, m);
            }
#pragma unroll
            for (int k = 0; k < kPPT; ++k) if (i0 + k < n) A[i0 + k] = max(v[k], excl);
        }
        __syncthreads();
    }
    if (tid == 0 && a.n_requant) a.n_requant[b] = n_requant;
    if constexpr (KEEP) {
        if (RESUME && a.skip_readout) return;
        // ---- read-out: the lineage walk, hit T-1 back to 0, integer sums per hit ----
        const uint8_t* fin = ((T - 1) & 1) ? S1 : S0;
        for (int p = 0; p < passes; ++p)
#pragma unroll
            for (int k = 0; k < kPPT; ++k) { const int i = p * kTile + tid * kPPT + k; if (i < n) A[i] = i; }
        // (each thread walks its own particles' paths: no barrier needed before the walk)
        const double* e_fin = tab + (int64_t)(T - 1) * kBatchTab + 3;
        for (int t = T - 1; t >= 0; --t) {
            uint64_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};                       // HMM3: pair counts by key; HMM_TABLE: weight sums by state
            const int8_t* vrow = a.values + store() + (int64_t)t * n;
            const int32_t* arow = a.anc + store() + (int64_t)t * n;
            for (int p = 0; p < passes; ++p) {
#pragma unroll
                for (int k = 0; k < kPPT; ++k) {
                    const int i = p * kTile + tid * kPPT + k;
                    if (i >= n) continue;
                    const int pth = A[i];
                    const int x = vrow[pth], c = fin[i];
                    if constexpr (kCounts) {
                        const int key = 3 * (x - 1) + c;                       // trace_words.hpp: x_t in {1, 2} paired with the class x_{T-1}
#pragma unroll
                        for (int j = 0; j < kTraceKeys; ++j) acc[j] += (x > 0 && key == j) ? 1ull : 0ull;
                    } else {
                        const uint64_t w = batch_sel8(q_fin, c);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j] += x == j ? w : 0ull;
                    }
                    if (t > 0) A[i] = arow[pth];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = wave_sum_u64(acc[j]);
            if (lane == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) s_acc[t & 1][wv][j] = acc[j];
            }
            __syncthreads();
            if constexpr (kCounts) {
                if (tid < kTraceKeys) {
                    unsigned long long v = 0;
#pragma unroll
                    for (int w = 0; w < kWaves; ++w) v += s_acc[t & 1][w][tid];
                    s_rows[0][tid] = v;
                    if (t == T - 1) s_rows[1][tid] = v;
                }
                __syncthreads();
                if (tid < 3) st_b[(int64_t)t * a.spp + tid] = trace_stat(&s_rows[0][0], 2, 0, tid, n_pop, e_fin, false);
            } else {
                if (tid < a.spp) {
                    uint64_t v = 0;
#pragma unroll
                    for (int w = 0; w < kWaves; ++w) v += s_acc[t & 1][w][tid < 8 ? tid : 0];
                    st_b[(int64_t)t * a.spp + tid] = tid < k_states ? u64_to_double(v) / u64_to_double(S_fin) : 0.0;
                }
            }
        }
    }
}

// {log_evidence, ess_final, log_norm, max_logw, stats[T * spp]} of every problem, side by side (cpprob_hip_batch_results_device)
__global__ void batch_pack_kernel(const char* __restrict__ ctrl, const double* __restrict__ stats, int per, int64_t B, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = 4 + per;
    if (i >= B * row) return;
    const int64_t b = i / row, j = i - b * row;
    const StepCtrl* c = reinterpret_cast<const StepCtrl*>(ctrl + b * kBatchCtrlBytes);
    double v;
    if (j == 0) v = c->log_z;
    else if (j == 1) v = c->ess;
    else if (j == 2) v = c->M + log(c->W);
    else if (j == 3) v = c->M;
    else v = stats[b * per + (j - 4)];
    out[i] = v;
}

}  // namespace cph
