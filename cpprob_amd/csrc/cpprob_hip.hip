// C ABI of the gfx950 SIS / SMC engine: context, particle store, launch sequencing.
// Declarations and the reference interfaces they replace: include/cpprob_hip.h.
#include "../../include/cpprob_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "step_counts.hpp"
#include "step_fixed.hpp"
#include "exchange.hpp"
#include "bookkeep_fixed.hpp"
#include "trace_words.hpp"
#include "device_collectives.hpp"
#include "batch_smc.hpp"
#include "batch_paths.hpp"
#include "batch_smooth.hpp"
#include "batch_suffstats.hpp"
#include "batch_trajstats.hpp"
#include "batch_onlinestats.hpp"
#include "batch_forecast.hpp"
#include "batch_decode.hpp"
#include "batch_csmc.hpp"
#include "batch_retable.hpp"
#include "batch_scale.hpp"
#include "batch_poisson.hpp"
#include "batch_learn.hpp"
#include "batch_learn_tied.hpp"
#include "batch_pass_plan.hpp"
#include "batch_buffers.hpp"
#include "batch_pool.hpp"

using namespace cph;

namespace {

thread_local std::string g_last_error;      // per thread: contexts (and the group driver's workers) live on threads of their own
thread_local hipError_t g_last_hip_error = hipSuccess;   // the HIP error behind the last CPPROB_HIP_EDEVICE of HIP_TRY (run lanes: out of memory or not)

struct EventPair { hipEvent_t a, b; int cls; int count; };

}  // namespace

namespace { struct BatchState; }   // cpprob_hip_batch_*: beside the single-run state, which it does not touch

struct cpprob_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    cpprob_hip_config cfg{};
    bool begun = false, ran = false;
    int T = 0;              // predict hits per trace
    int n_obs = 0;
    bool is_int = false;
    int K = 0;              // stats per predict
    int64_t n = 0, ld = 0;
    int64_t rs = 0;         // row stride of values[] / anc[]: ld + annex_cap
    bool grid_refs = false; // continuous-weight model: tile references on the grid {k ln 2} (kernels.hpp, grid_reference)
    size_t ssz = 8;         // bytes per element of values[] (Model::store_t; may be narrower than the model's value type)
    int nb = 0;             // tiles
    int smooth_grid = 0;
    int walk_cap = 0, walk_grid = 0, n_cu = 0;    // lineage walk: partials allocated for walk_cap workgroups; the grid of this configuration's walk (0: not chosen yet)
    ModelParams mp{};
    uint64_t run_seed = 0;
    uint64_t pop_n = 0;     // size of the population this shard is resampled with (n_global, or n for islands)

    // device buffers
    double* d_obs = nullptr;
    double* d_logw[2] = {nullptr, nullptr};
    double* d_wrel[2] = {nullptr, nullptr};
    double* d_bf = nullptr;
    bool final_from_counts = false, final_bookkeep_pending = false; int final_copy = 0;
    bool scan2_deferred = false;         // exchange scope, floating-point form: step_end left the cross-rank combine to the plan launch
    bool keep = true, cap_keep = true;   // keep_history: per-step values + ancestors (false: two rows, no ancestors, filtering statistics)
    double* d_filter_w = nullptr;        // filtering-only shards: [T] this shard's mass of generation t (the joint normaliser is their sum over ranks)
    double* d_fpart = nullptr;           // filtering-only runs, floating-point form: [T][K + 2][smooth_grid] (filter_partials_kernel)   // prefix-count form, single shard: the read-out works from the final generation's counts
    double* d_ll_tab = nullptr;     // hmm: [T][3] emission log-densities
    void* d_values = nullptr;
    int32_t* d_anc = nullptr;
    void* d_paths = nullptr;
    Partial* d_part[2] = {nullptr, nullptr};   // tile partials, ping-pong between generations
    int cur_part = 0;                          // which one holds the latest generation
    double* d_e_tab = nullptr;                 // hmm: [T][4]
    double* d_gpart = nullptr;                 // slab partials of the two-level normalisation (large populations)
    double* d_stile = nullptr;                 // SIS fused read-out: per-tile weighted sums [kMaxReadoutCols][nb]
    double* d_gstat = nullptr;                 //                     per-slab weighted sums [kMaxReadoutCols][kMaxSlabs]
    double* d_bc = nullptr;
    StepCtrl* d_ctrl = nullptr;
    double* d_ess = nullptr;
    int32_t* d_resampled = nullptr;
    double* d_stats_part = nullptr;
    double* d_stats = nullptr;
    uint32_t* d_bbf_strata = nullptr; uint32_t* d_bbf_strata_top = nullptr; size_t bbf_strata_cap = 0;     // ... of the bookkeeping protocol (cpprob_hip_smc_bookkeep_fixed_rs)
    uint32_t* d_strata = nullptr;   // multinomial, strata form: [T - 1][2^k + 1] first outputs of the strata, every step of the run
    uint32_t* d_strata_top = nullptr; int strata_phase = 0; bool strata_pending = false;   // ... [2][T][64] totals of the level-6 nodes (the set in use alternates run by run)
    size_t strata_cap_words = 0; int strata_cap_T = 0;
    // ... of one shard of a joint population (exchange scope, strata_cut.hpp): what the ranks' boundaries cut, rewritten by every exchange
    uint32_t* d_cut_tab = nullptr; CutHead* d_cut_head = nullptr; uint32_t* d_cut_srccnt = nullptr;
    double* d_cdf = nullptr;        // multinomial only
    int32_t* d_anc_pre = nullptr;   // multinomial only
    double* d_local_totals = nullptr;
    double* totals_out = nullptr;   // caller-provided {max, sum, sum of squares} of the shard (step protocol)
    bool sharded = false;           // the last run went through the step protocol: stats stay un-normalised
    bool step_protocol = false;     // a step-protocol run is in progress (the step kernel must not normalise on its own)
    int step_t = -1;                // step of the last cpprob_hip_smc_step_begin
    int cur = 0;                    // logw buffer holding the latest generation
    // exchange scope: exact global resampling, offspring of remote sources migrate in as annex columns
    bool exchange = false;
    int64_t annex_cap = 0, annex_used = 0;
    std::vector<int64_t> annex_used_before;   // (synchronising exchange calls) annex columns in use before the commit that follows step t: what a repair rewinds to
    double* d_obound = nullptr;     // [world + 2]: offspring-interval bounds per rank, then the resampling decision
    double* h_obound = nullptr;     // pinned host copy (the one host read-back per step of the exchange scope)
    // read-backs of small results go through pinned memory (a copy into pageable memory blocks the host for its own round trip: three of
    // them closed an unchanged-model run at ~25 us each) and ride ONE stream synchronisation; the caller may hang a copy of its own on it
    char* h_pin = nullptr; size_t h_pin_cap = 0; uint64_t pin_seq = 0;
    const void* ride_src = nullptr; void* ride_dst = nullptr; size_t ride_bytes = 0;
    int32_t* d_send_src = nullptr; size_t send_src_cap = 0;
    // device-resident exchange plan (exchange.hpp) and the transport geometry
    ExchangePlan* d_xplan = nullptr;
    int64_t* d_shard_begin = nullptr; int32_t* d_slot_of_rank = nullptr;
    int x_world = 0, x_rank = 0;                  // as of the last step_end
    const double* x_all_totals = nullptr;
    bool x_fixed = false; int64_t x_cap = 0; int x_mode = 0; std::vector<int> x_peers;   // fixed-capacity transport (cpprob_hip_exchange_setup)
    void* d_xsend = nullptr; void* d_xrecv = nullptr; size_t x_buf_bytes = 0;
    // direct transport: the packing kernel stores records straight into the receivers' buffers (cpprob_hip_exchange_direct)
    bool x_direct = false; void** d_peer_recv = nullptr; int32_t* d_peer_slot = nullptr;
    int64_t* d_sent = nullptr; int sent_cap = 0;  // [T] records sent after each step of the last run (traffic accounting)
    // remote lineages (cpprob_hip_exchange_remote): migrants leave their history where it is; d_origin[annex column] = (rank << 32) | slot
    bool x_remote = false; int64_t* d_origin = nullptr; int64_t origin_cap = 0; RemoteStores* d_remote = nullptr; int64_t* d_annex_all = nullptr; int annex_all_T = 0;
    std::vector<uint64_t> x_shard_begin;
    int x_plan_t = -1;                            // step whose plan sits in d_xplan
    struct { int t = -1; bool resample = false; std::vector<uint64_t> send_lo, send_cnt; uint64_t n_send = 0, n_recv = 0; int64_t l0 = 0, l1 = 0; } plan;
    size_t cap_particles = 0; int cap_T = 0; bool cap_int = false; bool cap_multinomial = false;
    // prefix-count form of the step (table-weight models on an every-step schedule; step_counts.hpp)
    uint64_t* d_hier = nullptr; size_t hier_entries = 0;   // three copies of the 64-ary count hierarchy
    HierTable hier{};                                      // host copy of the hierarchy's layout
    HierTable* d_hier_table = nullptr;                     // the same in device memory
    size_t hier_per_copy = 0;                              // 64-bit words per copy
    int hier_phase = 0;                                    // copy that step 0 of the next run reads: chosen so that the copy it adds into is clean
    int hier_phase_run = 0;                                // ... of the run in flight
    bool hier_run_open = false;                            // a run's steps are in flight (the rotation's state is known only at run boundaries)
    int64_t* d_annex_base = nullptr;                       // [T + 1] exchange scope: annex columns in use before each step's immigrants
    int32_t* d_skip = nullptr;                             // [T / 8 + 1][rs] exchange scope, long traces: skip rows (exchange.hpp: skip_rows_kernel)
    bool counts_mode = false;                              // this run's steps use smc_step_counts_kernel
    bool fixed_mode = false;                               // ... or smc_step_fixed_kernel (fixed-point weights, step_fixed.hpp)
    bool final_from_fixed = false;                         // the read-out takes its weights from the final generation's integer weights
    // The fixed-point weights are taken against a reference fixed before the generation exists (step_fixed.hpp); where some
    // generation's heaviest particle sat far below it (an observation many standard deviations from every particle) they lose bits.
    // The first call that reads a run's results checks the run's largest gap and repeats the run in the floating-point form.
    bool force_fp = false, fixed_check_pending = false, last_was_infer_run = false; uint64_t last_run_index = 0;
    double* d_lz_trace = nullptr; int n_requantised = 0;    // fixed-point form: the evidence before each generation's books (what a repair rewinds to); generations repaired in the last run
    uint32_t* d_q[2] = {nullptr, nullptr};                 // [ld] integer weights of the fixed-point form, ping-pong; the count form's trace words
    // trace words (trace_words.hpp): a single population's short discrete traces ride with the particles; the read-out streams them
    bool trace_mode = false; uint32_t* d_trace_cnt = nullptr; unsigned long long* d_trace_arrive = nullptr;
    // the run's last step with the read-out folded in (step_counts.hpp: step_fold_tail): its counter sets, then the top arrival counter
    uint32_t* d_fold = nullptr; size_t fold_cap = 0, fold_sets = 0; bool final_folded = false;
    // ... and of one shard of a joint population (remote lineages): the words by the step's parity, [rs] each -- annex columns included,
    // a migrant's word arrives with its state; trace_shard: every rank of the group has them
    uint32_t* d_tr[2] = {nullptr, nullptr}; size_t tr_cap = 0; bool trace_shard = false, trace_shard_run = false;
    std::vector<double> h_bound;                           // [T] upper bound of each step's incremental log-weight (host-evaluated)
    int hk = 0; std::vector<double> hk_mean, hk_trans;     // cpprob_hip_set_hmm: the table of CPPROB_HIP_MODEL_HMM_TABLE
    uint64_t* d_hk_thr = nullptr; double* d_hk_ll = nullptr;
    size_t hier_q0_off = 0, hier_m0_off = 0;               // the tiles' Q / M arrays inside one copy of the hierarchy
    std::vector<double> h_ll_tab, h_e_tab;                 // host copies of the table-weight model's per-step tables ([T][3], [T][4])
    double* d_wpart = nullptr;                             // bounded SIS: per-workgroup partial rows
    bool sis_bounded_ok = false;                           // this run's model / observes admit the bounded-weight SIS kernel

    // scratch for building blocks
    Partial* d_bb_part = nullptr; double* d_bb_bc = nullptr; double* d_bb_bf = nullptr; double* d_bb_wrel = nullptr; void* d_bb_col = nullptr;
    StepCtrl* d_bb_ctrl = nullptr; size_t bb_cap_nb = 0;
    double* d_bb_stats_part = nullptr; double* d_bb_stats = nullptr; double* d_bb_cdf = nullptr; size_t bb_cdf_cap = 0;
    void* d_bb_cols = nullptr; double* d_bb_cols_part = nullptr; double* d_bb_cols_stat = nullptr; size_t bb_cols_bytes = 0, bb_cols_part = 0, bb_cols_stat = 0;   // several columns at once
    int32_t* d_bb_first = nullptr; size_t bb_first_cap = 0;
    std::vector<int32_t> bb_first_host;
    // exchange scope, mailbox collectives (group.hpp): the step's shard-totals launch carries the all-gather (device_collectives.hpp)
    bool x_gather_on = false, x_gather_done = false; TotalsGather x_gather{}; unsigned long long x_gather_serial = 0;
    int x_gather_tshift = 0;                 // (a run resumed behind a repaired generation numbers its collectives from there: group.hpp)                              // what d_bb_first holds (an unchanged table is not uploaded again)

    // cpprob_hip_smc_bookkeep_fixed: two alternating copies of a mass hierarchy + the integer weights
    uint64_t* d_bbf_hier = nullptr; HierTable* d_bbf_table = nullptr; HierTable bbf_table{}; uint32_t* d_bbf_q = nullptr;
    size_t bbf_per_copy = 0, bbf_q0_off = 0, bbf_m0_off = 0; int bbf_nb = 0, bbf_phase = 0; size_t bbf_cap_nb = 0;
    // cpprob_hip_generic_*: three rotating copies of a mass hierarchy, two generations of integer weights, a control block
    uint64_t* d_gen_hier = nullptr; HierTable* d_gen_table = nullptr; HierTable gen_table{}; uint32_t* d_gen_q[2] = {nullptr, nullptr}; void* d_gen_ctrl = nullptr;
    size_t gen_per_copy = 0, gen_q0_off = 0, gen_m0_off = 0, gen_off[3] = {0, 0, 0}; int gen_nb = 0, gen_block = 0; size_t gen_cap_hier = 0, gen_cap_q = 0;

    // optional per-kernel-class timing
    bool profile = false;
    bool profile_suspended = false;   // an enclosing group scope is timing these launches
    std::vector<EventPair> ev_used, ev_free;
    double prof_ms[CPPROB_HIP_N_KERNEL_CLASSES] = {0};
    int64_t prof_calls[CPPROB_HIP_N_KERNEL_CLASSES] = {0};
    BatchState* batch = nullptr;

    // run lanes: cpprob_hip_infer_run calls that follow each other directly go round robin over up to kLaneDepth - 1 further contexts of
    // the library's own -- each a whole context: its own stream, workspace, hierarchy rotation, counters and pinned block, begun as
    // this one was -- so that independent runs overlap on the device.  Lane 0 is the context itself; reads go to the lane that ran last.
    bool is_lane = false;                                  // a lane of another context: never routes
    std::vector<cpprob_hip_ctx*> lanes; std::vector<char> lane_begun;      // [lane - 1]; begun with the configuration in force
    int lane_last = 0;                                     // lane of the last run
    bool lane_chain = false;                               // the previous entry point on this context was cpprob_hip_infer_run
    bool lanes_busy = false;                               // a further lane may have work in flight
    int lane_pin = 0;                                      // CPPROB_HIP_SERIAL_* that pinned the context serial until it is destroyed
    uint64_t lane_bytes = 0;                               // device bytes of the further lanes' population-sized arrays (a lane: of its own)
    cpprob_hip_config lane_cfg{}; std::vector<double> lane_obs;            // what cpprob_hip_infer_begin was given
    hipEvent_t lane_ev = nullptr;                          // orders cpprob_hip_infer_results_device against a lane's stream
};

namespace {

int fail(cpprob_hip_ctx* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->err = msg;
    g_last_error = msg;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                                  \
    do {                                                                                                    \
        hipError_t e__ = (expr);                                                                            \
        if (e__ != hipSuccess) {                                                                            \
            g_last_hip_error = e__;                                                                         \
            return fail(ctx, CPPROB_HIP_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e__));       \
        }                                                                                                   \
    } while (0)

template <class T>
void dfree(T*& p)
{
    if (p) { (void)hipFree(p); p = nullptr; }
}

struct ProfScope {
    cpprob_hip_ctx* c; int cls; EventPair ep{}; bool on;
    // count = launches bracketed by this pair (back-to-back launches of one class are timed as a group, so the
    // event records do not sit between them)
    ProfScope(cpprob_hip_ctx* ctx, int k, int count = 1) : c(ctx), cls(k), on(ctx->profile && !ctx->profile_suspended)
    {
        if (!on) return;
        if (!c->ev_free.empty()) { ep = c->ev_free.back(); c->ev_free.pop_back(); }
        else { (void)hipEventCreate(&ep.a); (void)hipEventCreate(&ep.b); }
        ep.cls = cls; ep.count = count;
        (void)hipEventRecord(ep.a, c->stream);
    }
    ~ProfScope()
    {
        if (!on) return;
        (void)hipEventRecord(ep.b, c->stream);
        c->ev_used.push_back(ep);
    }
};

void host_model_params(ModelParams& mp, int model)
{
    std::memset(&mp, 0, sizeof mp);
    const double pi = 3.14159265358979323846;
    if (model == CPPROB_HIP_MODEL_GAUSSIAN_UNKNOWN_MEAN) {          // models.hpp:26-30
        mp.mu0 = 1; mp.sigma0 = std::sqrt(5.0); mp.sigma = std::sqrt(2.0);
    } else if (model == CPPROB_HIP_MODEL_GAUSSIAN_README) {         // gaussian.cpp:8
        mp.mu0 = 1; mp.sigma0 = 1.5; mp.sigma = 2;
    } else if (model == CPPROB_HIP_MODEL_GAUSSIAN_2D_UNKNOWN_MEAN) { // models.hpp:42,44
        mp.nd_mean[0] = 1; mp.nd_mean[1] = 2; mp.nd_sigma[0] = std::sqrt(5.0); mp.nd_sigma[1] = std::sqrt(3.0); mp.sigma = std::sqrt(2.0);
    } else { mp.mu0 = 0; mp.sigma0 = 1; mp.sigma = 1; }
    mp.log_norm_lik = std::log(2 * pi * mp.sigma * mp.sigma);       // utils_normal_distribution.hpp:40
    mp.inv_sigma = 1.0 / mp.sigma;
    mp.log_norm_unit = std::log(2 * pi * 1.0 * 1.0);
    const double mean[3] = {-1, 0, 1};                               // models.hpp:122
    const double T[3][3] = {{0.1, 0.5, 0.4}, {0.2, 0.2, 0.6}, {0.15, 0.15, 0.7}};  // models.hpp:123-125
    for (int s = 0; s < 3; ++s) {
        mp.hmm_mean[s] = mean[s];
        double tot = 0.0;
        for (int j = 0; j < 3; ++j) tot += T[s][j];
        double acc = 0.0;
        for (int j = 0; j < 2; ++j) { acc += T[s][j]; mp.hmm_thr[s][j] = (uint64_t)std::ceil((acc / tot) * 4294967296.0); }   // u >= c  <=>  word >= ceil(c * 2^32)
    }
}

int model_T(int model, size_t n_obs)
{
    return (model == CPPROB_HIP_MODEL_GAUSSIAN_UNKNOWN_MEAN || model == CPPROB_HIP_MODEL_GAUSSIAN_README) ? 1 : (int)n_obs;
}

int ensure_bb(cpprob_hip_ctx* ctx, size_t n)
{
    const size_t nb = (n + kTile - 1) / kTile;
    if (nb > ctx->bb_cap_nb || !ctx->d_bb_ctrl) {
        dfree(ctx->d_bb_part); dfree(ctx->d_bb_bc); dfree(ctx->d_bb_bf); dfree(ctx->d_bb_wrel); dfree(ctx->d_bb_col); dfree(ctx->d_bb_stats_part);
        const size_t cap = std::max<size_t>(nb, 1024);
        HIP_TRY(ctx, hipMalloc(&ctx->d_bb_part, (size_t)part_stride((int)cap) * 3 * sizeof(double)));
        HIP_TRY(ctx, hipMalloc(&ctx->d_bb_bc, (cap + 1) * sizeof(double)));
        HIP_TRY(ctx, hipMalloc(&ctx->d_bb_bf, cap * sizeof(double)));
        HIP_TRY(ctx, hipMalloc(&ctx->d_bb_wrel, cap * kTile * sizeof(double)));
        HIP_TRY(ctx, hipMalloc(&ctx->d_bb_col, cap * kTile * sizeof(double)));
        HIP_TRY(ctx, hipMalloc(&ctx->d_bb_stats_part, 2048 * 8 * sizeof(double)));
        if (!ctx->d_bb_ctrl) HIP_TRY(ctx, hipMalloc(&ctx->d_bb_ctrl, sizeof(StepCtrl)));
        if (!ctx->d_bb_stats) HIP_TRY(ctx, hipMalloc(&ctx->d_bb_stats, 16 * sizeof(double)));
        ctx->bb_cap_nb = cap;
    }
    return 0;
}

// partials + linear weights + scan of an arbitrary logw array into the building-block scratch
int bb_normalise(cpprob_hip_ctx* ctx, const double* d_logw, size_t n, double n_total)
{
    if (int rc = ensure_bb(ctx, n)) return rc;
    const int nb = (int)((n + kTile - 1) / kTile);
    hipLaunchKernelGGL(weights_partials_kernel, dim3(nb), dim3(kThreads), 0, ctx->stream, d_logw, (int64_t)n, ctx->d_bb_part, ctx->d_bb_wrel);
    ScanArgs sa{};
    sa.part = ctx->d_bb_part; sa.nb = nb; sa.bc = ctx->d_bb_bc; sa.bf = ctx->d_bb_bf; sa.ctrl = ctx->d_bb_ctrl; sa.t = 0; sa.T = 1;
    sa.n_pop = n_total; sa.n_local = (double)n; sa.ess_frac = 0.0; sa.force_no_resample = 1; sa.phase = 0; sa.seed = 0;
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sa);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// the SIS read-out can ride the normalisation (no read-back of the particle store) when its columns are few
template <class Model>
bool sis_readout_fused(const cpprob_hip_ctx* c)
{
    return !(c->cfg.flags & CPPROB_HIP_FLAG_SIS_SEPARATE_READOUT) && c->T <= kMaxReadoutT && c->T * Model::kStats <= kMaxReadoutCols;
}

template <class Model>
void launch_sis(cpprob_hip_ctx* c, bool readout)
{
    SisArgs<Model> a{};
    a.mp = c->mp; a.obs = c->d_obs; a.T = c->T; a.n = c->n; a.ld = c->ld; a.rs = c->rs; a.seed = c->run_seed; a.pid0 = c->cfg.particle_offset;
    a.values = static_cast<typename Model::store_t*>(c->d_values); a.logw = c->d_logw[0]; a.wrel = c->d_wrel[0]; a.part = c->d_part[0];
    a.stile = c->d_stile;
    c->cur_part = 0;
    ProfScope ps(c, 4);
    if (readout) hipLaunchKernelGGL((sis_kernel<Model, true>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL((sis_kernel<Model, false>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
}

// normalisation of the final SIS weights + the weighted moments in the same two launches (slab form at every size)
template <class Model>
void launch_sis_readout(cpprob_hip_ctx* c)
{
    ScanArgs sa{};
    sa.part = c->d_part[c->cur_part]; sa.nb = c->nb; sa.bc = c->d_bc; sa.bf = c->d_bf; sa.ctrl = c->d_ctrl; sa.t = c->T - 1; sa.T = c->T;
    sa.n_pop = (double)c->pop_n; sa.n_local = (double)c->n; sa.ess_frac = c->cfg.ess_threshold; sa.seed = c->run_seed;
    sa.ess_trace = c->d_ess; sa.resampled = c->d_resampled; sa.force_no_resample = 1; sa.grid_refs = c->grid_refs ? 1 : 0; sa.phase = 0;
    const int G = (c->nb + kSlabTiles - 1) / kSlabTiles;
    const int n_col = c->T * Model::kStats;
    ProfScope ps(c, 1);
    hipLaunchKernelGGL(scan_slab_partials_kernel, dim3(G), dim3(kThreads), 0, c->stream, sa.part, c->nb, c->d_gpart, sa.grid_refs,
                       (const double*)c->d_stile, n_col, c->d_gstat);
    hipLaunchKernelGGL(scan_slab_finish_kernel, dim3(G), dim3(kThreads), 0, c->stream, sa, (const double*)c->d_gpart, G,
                       (const double*)c->d_gstat, n_col, (int)Model::kStats, Model::kIsInt ? 1 : 0, c->d_stats);
}

// Bounded-weight SIS (kernels.hpp: sis_bounded_kernel): the whole run in two launches.  CPPROB_HIP_FLAG_SIS_PER_TILE keeps the per-tile form.
template <class Model>
bool launch_sis_bounded(cpprob_hip_ctx* c)
{
    if constexpr (Model::kBounded) {
        if ((c->cfg.flags & CPPROB_HIP_FLAG_SIS_PER_TILE) || !c->sis_bounded_ok) return false;
        SisBoundedArgs<Model> a{};
        a.mp = c->mp; a.T = c->T; a.n = c->n; a.ld = c->ld; a.rs = c->rs; a.nb = c->nb; a.seed = c->run_seed; a.pid0 = c->cfg.particle_offset;
        a.values = static_cast<typename Model::store_t*>(c->d_values); a.logw = c->d_logw[0]; a.wpart = c->d_wpart;
        const int G = std::min(c->nb, (int)kSisBoundedMaxGrid);
        c->cur = 0; c->cur_part = 0;
        {
            ProfScope ps(c, 4);
            if (c->T == 1) hipLaunchKernelGGL((sis_bounded_kernel<Model, 1>), dim3(G), dim3(kThreads), 0, c->stream, a);
            else hipLaunchKernelGGL((sis_bounded_kernel<Model, 2>), dim3(G), dim3(kThreads), 0, c->stream, a);
        }
        ProfScope ps(c, 1);
        hipLaunchKernelGGL(sis_bounded_finish_kernel, dim3(1), dim3(kThreads), 0, c->stream, (const double*)c->d_wpart, G, c->T, (int)Model::kStats, c->mp.lw_ref,
                           (double)c->pop_n, c->d_ctrl, c->d_stats, c->d_ess, c->d_resampled, 1);
        return true;
    }
    return false;
}

template <class Model, int FUSED, bool COUNTS>
void launch_step_kernels(cpprob_hip_ctx* c, StepArgs<Model>& a)
{
    const size_t shm = FUSED ? (size_t)(2 * c->nb + 1) * sizeof(double) : 0;
    switch (c->cfg.resampler) {
    case CPPROB_HIP_RESAMPLE_SYSTEMATIC:
        hipLaunchKernelGGL((smc_step_kernel<Model, RS_SYSTEMATIC, FUSED, COUNTS>), dim3(c->nb), dim3(kThreads), shm, c->stream, a); break;
    case CPPROB_HIP_RESAMPLE_STRATIFIED:
        hipLaunchKernelGGL((smc_step_kernel<Model, RS_STRATIFIED, FUSED, COUNTS>), dim3(c->nb), dim3(kThreads), shm, c->stream, a); break;
    default:
        hipLaunchKernelGGL((smc_step_kernel<Model, RS_PRECOMPUTED, 0, false>), dim3(c->nb), dim3(kThreads), 0, c->stream, a); break;
    }
}

template <class Model, int FUSED>
void launch_step_impl(cpprob_hip_ctx* c, StepArgs<Model>& a)
{
    // packed-count partials exist for table-weight models in the fused form only (a.part_counts is set accordingly)
    if (Model::kWeightTable > 0 && FUSED != 0 && a.part_counts) launch_step_kernels<Model, FUSED, (Model::kWeightTable > 0 && FUSED != 0)>(c, a);
    else launch_step_kernels<Model, FUSED, false>(c, a);
}

// fused = the step kernel normalises the previous generation itself (no scan_partials launch between steps)
bool step_is_fused(const cpprob_hip_ctx* c)
{
    const int max_tiles = c->cfg.fuse_max_tiles > 0 ? std::min((int)c->cfg.fuse_max_tiles, (int)kFuseMaxTiles) : (int)kFuseMaxTiles;
    return c->nb <= max_tiles && c->cfg.resampler != CPPROB_HIP_RESAMPLE_MULTINOMIAL && !c->step_protocol;
}

template <class Model>
void launch_step(cpprob_hip_ctx* c, int t)
{
    StepArgs<Model> a{};
    a.mp = c->mp; a.obs = c->d_obs; a.t = t; a.T = c->T; a.n = c->n; a.ld = c->ld; a.seed = c->run_seed;
    a.pid0 = c->cfg.particle_offset;
    a.values = static_cast<typename Model::store_t*>(c->d_values); a.anc = c->d_anc;
    a.logw_prev = c->d_logw[c->cur]; a.logw_next = c->d_logw[c->cur ^ 1];
    a.wrel_prev = c->d_wrel[c->cur]; a.wrel_next = c->d_wrel[c->cur ^ 1];
    a.part_prev = c->d_part[c->cur_part]; a.part = c->d_part[t == 0 ? c->cur_part : c->cur_part ^ 1];
    a.bc = c->d_bc; a.bf = c->d_bf; a.nb = c->nb; a.ctrl = c->d_ctrl; a.anc_pre = c->d_anc_pre;
    a.n_pop = (double)c->pop_n; a.ess_frac = c->cfg.ess_threshold; a.ess_trace = c->d_ess; a.resampled = c->d_resampled;
    a.store_logw = (c->cfg.ess_threshold > 1.0 && c->keep) ? 0 : 1;      // ESS <= N always: threshold > 1 resamples after every step (a filtering-only run reads them after every step)
    a.rs = c->rs;
    a.row_w = c->keep ? t : (t & 1); a.row_r = t > 0 ? (c->keep ? t - 1 : ((t - 1) & 1)) : 0;
    if (!c->keep) a.anc = nullptr;
    {
        // table-weight model + every step resamples + systematic + fused: the step kernel reads states instead of wrel
        const bool enabled = !(c->cfg.flags & CPPROB_HIP_FLAG_WREL_STORED);
        // (pays from ~2.6e5 particles: below, the extra selects cost more than the halved traffic saves -- profiles/r01_ab_notes.md)
        const int min_tiles = 256;
        a.wrel_from_state = (enabled && Model::kWeightTable > 0 && c->cfg.ess_threshold > 1.0 && c->cfg.resampler == CPPROB_HIP_RESAMPLE_SYSTEMATIC &&
                             !c->step_protocol && c->nb >= min_tiles) ? 1 : 0;
        const bool counts = !(c->cfg.flags & CPPROB_HIP_FLAG_FP_TILE_PARTIALS);
        a.part_counts = (counts && a.wrel_from_state && step_is_fused(c)) ? 1 : 0;
    }
    a.exchange = (c->exchange && c->step_protocol) ? 1 : 0; a.imm_l01 = c->d_xplan ? &c->d_xplan->l0 : nullptr; a.annex_base = c->d_annex_base;
#ifdef CPPROB_STAMPS
    static unsigned long long* d_st = nullptr;
    if (!d_st) { (void)hipMalloc(&d_st, (size_t)131072 * 16 * 8); (void)hipMemset(d_st, 0, (size_t)131072 * 16 * 8); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &d_st, sizeof(d_st)); }
#endif
    if (c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL && t > 0) {
        // literal thesis Alg. 1: materialise the CDF, draw N independent positions.  Runs
        // unconditionally; the step kernel ignores the result when ctrl says "no resampling".
        ProfScope ps(c, 5);
        hipLaunchKernelGGL(cdf_kernel, dim3(c->nb), dim3(kThreads), 0, c->stream, c->d_wrel[c->cur], c->d_bc, c->d_bf, c->d_ctrl, c->d_cdf);
        hipLaunchKernelGGL(multinomial_kernel, dim3((unsigned)((c->ld + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, c->d_cdf, c->n,
                           c->d_ctrl, c->run_seed, (uint64_t)t, c->cfg.particle_offset, c->n, c->ld, c->d_anc_pre, 0);
    }
    {
        ProfScope ps(c, 0);
        if (!step_is_fused(c)) launch_step_impl<Model, 0>(c, a);
        else if (c->nb <= 2 * kThreads) launch_step_impl<Model, 2>(c, a);
        else if (c->nb <= 4 * kThreads) launch_step_impl<Model, 4>(c, a);
        else launch_step_impl<Model, 8>(c, a);
    }
#ifdef CPPROB_STAMPS
    if (t == 8 && getenv("CPPROB_STAMP_DUMP")) {
        (void)hipStreamSynchronize(c->stream);
        std::vector<unsigned long long> h((size_t)c->nb * 16);
        (void)hipMemcpy(h.data(), d_st, h.size() * 8, hipMemcpyDeviceToHost);
        unsigned long long t0 = ~0ull; for (int b2 = 0; b2 < c->nb; ++b2) t0 = std::min(t0, h[(size_t)b2 * 16]);
        fprintf(stderr, "STAMPS t=8 n=%lld (us since first workgroup start) mean/max:", (long long)c->n);
        for (int k = 0; k < 12; ++k) {
            double acc = 0, mx = 0;
            for (int b2 = 0; b2 < c->nb; ++b2) { const double v = (double)(h[(size_t)b2 * 16 + k] - t0) * 0.01; acc += v; mx = std::max(mx, v); }
            fprintf(stderr, " [%d] %.2f/%.2f", k, acc / c->nb, mx);
        }
        fprintf(stderr, "\n");
    }
#endif
    c->cur ^= 1;
    if (t > 0) c->cur_part ^= 1;
    if (!c->keep) {
        // filtering only: predict hit t's sums under the weights this step just left
        hipLaunchKernelGGL(filter_partials_kernel<Model>, dim3(c->smooth_grid), dim3(kThreads), 0, c->stream,
                           static_cast<const typename Model::store_t*>(c->d_values) + (int64_t)a.row_w * c->rs, (const double*)c->d_logw[c->cur], c->n,
                           c->d_fpart + (size_t)t * (Model::kStats + 2) * c->smooth_grid);
    }
}

// The prefix-count form serves table-weight models (three values) whose every step resamples systematically: ancestors are
// then a function of integer counts (bit-exact against the oracle at any size), no step needs a normalisation launch, and the
// per-step prologue is one wavefront reduction.  CPPROB_HIP_FLAG_FLOATING_POINT_STEP keeps the floating-point form (A/B runs).
template <class Model>
bool counts_eligible(const cpprob_hip_ctx* c)
{
    return !(c->cfg.flags & CPPROB_HIP_FLAG_FLOATING_POINT_STEP) && c->nb <= kCountsMaxTiles && Model::kWeightTable == 3 && sizeof(typename Model::store_t) == 1 && c->cfg.algorithm == CPPROB_HIP_ALG_SMC &&
           c->cfg.ess_threshold > 1.0 &&
           (c->cfg.resampler == CPPROB_HIP_RESAMPLE_SYSTEMATIC
                ? (c->cfg.resample_scope == CPPROB_HIP_SCOPE_EXCHANGE || c->cfg.n_global == c->cfg.n_particles || c->cfg.resample_scope == CPPROB_HIP_SCOPE_ISLAND)
                // (stratified resampling: the same walk with the outputs' own uniforms)
                : c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED
                ? (c->cfg.resample_scope == CPPROB_HIP_SCOPE_EXCHANGE || c->cfg.n_global == c->cfg.n_particles || c->cfg.resample_scope == CPPROB_HIP_SCOPE_ISLAND)
                // (multinomial, strata form: a population of its own or one shard of the exchange scope; the literal form runs on fixed-point masses)
                : (!(c->cfg.flags & CPPROB_HIP_FLAG_MULTINOMIAL_LITERAL) &&
                   (c->cfg.resample_scope == CPPROB_HIP_SCOPE_EXCHANGE || c->cfg.n_global == c->cfg.n_particles || c->cfg.resample_scope == CPPROB_HIP_SCOPE_ISLAND)));
}

// Philox4x32-10 on the host (cpprob/detail/rng.hpp's draw_block): the systematic offset of a resampling step is a pure function of
// (seed, step), so the launch carries it as a kernel argument instead of a device-side hand-over between consecutive kernels.
double host_resample_u0(uint64_t seed, uint64_t step)
{
    const uint64_t draw = (1ull << 40) + step, group = 0;
    uint32_t c0 = (uint32_t)draw, c1 = (uint32_t)(draw >> 32), c2 = (uint32_t)group, c3 = (uint32_t)(group >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint64_t bits = (uint64_t)c0 | ((uint64_t)(c1 >> 11) << 32);
    return (double)bits * 1.1102230246251565e-16;
}

// The launch-side view of one copy of the count hierarchy (levels not in use alias level 0: see step_counts.hpp).
static void hier_view(const cpprob_hip_ctx* c, int copy, Hier& h)
{
    for (int l = 0; l < kHierMaxLevels; ++l) {
        h.lvl[l] = l < c->hier.n_lev ? c->hier.lvl[copy][l] : c->hier.lvl[copy][0];
        h.n_ent[l] = c->hier.n_ent[l];
    }
    h.n_lev = c->hier.n_lev; h.table = c->d_hier_table; h.copy = copy;
    const int top = c->hier.n_lev - 1;
    h.top = c->hier.lvl[copy][top]; h.top_n = c->hier.n_ent[top]; h.top_stride = top == 0 ? 1 : kHierStride;
}

static void hier_rotation(cpprob_hip_ctx* c, int t, int& kp, int& kn, int& kc);
static void counts_final_view(cpprob_hip_ctx* c, CountsFinal& f, bool bookkeep);
static void launch_strata(cpprob_hip_ctx* c);
// multinomial resampling, strata form: the outputs the strata are drawn for -- the population's in the exchange scope, else this context's
static uint64_t strata_outputs(const cpprob_hip_ctx* c) { return c->exchange ? c->pop_n : (uint64_t)c->n; }
static int strata_k_of(const cpprob_hip_ctx* c) { return strata_levels((int64_t)((strata_outputs(c) + kTile - 1) / kTile)); }
static CutView cut_view(const cpprob_hip_ctx* c) { return CutView{c->d_cut_tab, c->d_cut_head, c->d_cut_srccnt}; }

template <class Model>
void launch_step_counts(cpprob_hip_ctx* c, int t, const double* all_totals, int world, int rank)
{
    if constexpr (Model::kWeightTable == 3 && sizeof(typename Model::store_t) == 1) {
        StepCountsArgs<Model> a{};
        a.mp = c->mp; a.t = t; a.T = c->T; a.n = c->n; a.ld = c->ld; a.rs = c->rs; a.seed = c->run_seed; a.pid0 = c->cfg.particle_offset;
        a.values = static_cast<typename Model::store_t*>(c->d_values); a.anc = c->d_anc;
        {
            int kp, kn, kc;
            hier_rotation(c, t, kp, kn, kc);
            hier_view(c, kp, a.h);
            a.h.to_next = (int64_t)(kn - kp) * (int64_t)c->hier_per_copy; a.h.to_clear = (int64_t)(kc - kp) * (int64_t)c->hier_per_copy;
            if (t == 0) c->final_from_counts = false;
            if (t + 1 == c->T) {
                // The last step is a step like any other (the read-out works from the counts it leaves): the copy it read and the one
                // it wrote are dirty, the one it cleared is where the next run's step 0 writes -- the next run starts its rotation
                // there, without any clearing launch.
                c->hier_phase = kn; c->final_from_counts = true; c->final_copy = kn; c->final_bookkeep_pending = true;
                c->hier_run_open = false;
            }
        }
        a.ctrl = c->d_ctrl; a.n_pop = (double)c->pop_n; a.ess_trace = c->d_ess; a.resampled = c->d_resampled;
        a.row_w = c->keep ? t : (t & 1); a.row_r = t > 0 ? (c->keep ? t - 1 : ((t - 1) & 1)) : 0;
        if (!c->keep) { a.anc = nullptr; a.filter_stats = c->d_stats; }
        a.all_totals = all_totals; a.world = world; a.rank = rank; a.annex_base = c->d_annex_base;
        a.src_shift = (c->exchange && c->x_fixed && !c->x_peers.empty() && c->d_xplan) ? &c->d_xplan->src_shift : nullptr;
        for (int k = 0; k < 4; ++k) a.e_prev[k] = t > 0 ? c->h_e_tab[(size_t)(t - 1) * 4 + k] : 0.0;
        a.u0 = t > 0 ? host_resample_u0(c->run_seed, (uint64_t)t) : 0.0;
        if (c->trace_mode && !all_totals) { a.trace_prev = c->d_q[(t + 1) & 1]; a.trace_next = c->d_q[t & 1]; }
        if (c->step_protocol && c->trace_shard_run) { a.trace_prev = c->d_tr[(t + 1) & 1]; a.trace_next = c->d_tr[t & 1]; }
        ProfScope ps(c, 0);
        // The run's last step with the read-out folded in (step_counts.hpp: step_fold_tail): a population of its own whose read-out is
        // the trace words' counts (r07: -4.5 us a run at 10^6, -13 / -9 / -17 us at 10^5 / 4e6 / 10^7).  Filtering-only runs keep
        // counts_filter_final_kernel, one wavefront: folded, their run measured 1.4 us slower at 10^6 (profiles/r07_notes.md).
        // CPPROB_HIP_FLAG_SEPARATE_TRACE_READOUT keeps the last step ordinary and the read-out a launch of its own (trace_readout_kernel).
        const bool fold = t + 1 == c->T && !all_totals && !c->step_protocol && !c->sharded && c->trace_mode && c->d_fold &&
                          !(c->cfg.flags & CPPROB_HIP_FLAG_SEPARATE_TRACE_READOUT);
        StepCountsLastArgs<Model> la{};
        if (fold) {
            static_cast<StepCountsArgs<Model>&>(la) = a;
            la.fold.cnt = c->d_fold; la.fold.arrive = reinterpret_cast<unsigned long long*>(c->d_fold + c->fold_sets * kFoldSetWords);
            la.fold.stats = c->d_stats;
            counts_final_view(c, la.fold.f, true);
            c->final_bookkeep_pending = false; c->final_folded = true;
        }
        if (c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL) {
            a.strata_k = strata_k_of(c);
            if (t == 0) launch_strata(c);
            a.strata_offs = t > 0 ? c->d_strata + (size_t)(t - 1) * (((size_t)1 << a.strata_k) + 1) : nullptr;
            a.cut = cut_view(c);
            la.strata_k = a.strata_k; la.strata_offs = a.strata_offs; la.cut = a.cut;
            if (all_totals) hipLaunchKernelGGL((smc_step_counts_kernel<Model, true, kFixMultinomial>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (fold) hipLaunchKernelGGL((smc_step_counts_kernel<Model, false, kFixMultinomial, true>), dim3(c->nb), dim3(kThreads), 0, c->stream, la);
            else hipLaunchKernelGGL((smc_step_counts_kernel<Model, false, kFixMultinomial>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
        }
        else if (c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED && all_totals) hipLaunchKernelGGL((smc_step_counts_kernel<Model, true, kFixStratified>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
        else if (c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED && fold) hipLaunchKernelGGL((smc_step_counts_kernel<Model, false, kFixStratified, true>), dim3(c->nb), dim3(kThreads), 0, c->stream, la);
        else if (c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED) hipLaunchKernelGGL((smc_step_counts_kernel<Model, false, kFixStratified>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
        else if (all_totals) hipLaunchKernelGGL((smc_step_counts_kernel<Model, true>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
        else if (fold) hipLaunchKernelGGL((smc_step_counts_kernel<Model, false, kFixSystematic, true>), dim3(c->nb), dim3(kThreads), 0, c->stream, la);
        else hipLaunchKernelGGL((smc_step_counts_kernel<Model, false>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
#ifdef CPPROB_STAMPS
        {
            // diagnostic build: the phase stamps of step 8 (kernels.hpp: CPH_STAMP; 8 .. 11 = inside the multinomial walk), CPPROB_STAMP_DUMP=1
            static unsigned long long* d_st = nullptr;
            if (!d_st) { (void)hipMalloc(&d_st, (size_t)131072 * 16 * 8); (void)hipMemset(d_st, 0, (size_t)131072 * 16 * 8); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &d_st, sizeof(d_st)); }
            if (t == 8 && getenv("CPPROB_STAMP_DUMP")) {
                (void)hipStreamSynchronize(c->stream);
                std::vector<unsigned long long> h((size_t)c->nb * 16);
                (void)hipMemcpy(h.data(), d_st, h.size() * 8, hipMemcpyDeviceToHost);
                unsigned long long t0 = ~0ull; for (int b2 = 0; b2 < c->nb; ++b2) t0 = std::min(t0, h[(size_t)b2 * 16]);
                fprintf(stderr, "STAMPS counts t=8 n=%lld rs=%d (us since first workgroup start) mean/max:", (long long)c->n, (int)c->cfg.resampler);
                for (int k : {0, 1, 2, 8, 9, 10, 11, 3, 4, 5}) {
                    double acc = 0, mx = 0;
                    for (int b2 = 0; b2 < c->nb; ++b2) { const double v = (double)(h[(size_t)b2 * 16 + k] - t0) * 0.01; acc += v; mx = std::max(mx, v); }
                    fprintf(stderr, " [%d] %.2f/%.2f", k, acc / c->nb, mx);
                }
                fprintf(stderr, "\n");
                for (int k : {0, 2, 3, 5}) {
                    std::vector<double> v((size_t)c->nb);
                    for (int b2 = 0; b2 < c->nb; ++b2) v[(size_t)b2] = (double)(h[(size_t)b2 * 16 + k] - t0) * 0.01;
                    std::sort(v.begin(), v.end());
                    fprintf(stderr, "   stamp %d percentiles 10/50/75/90/95/99/100: %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n", k, v[v.size() / 10], v[v.size() / 2], v[v.size() * 3 / 4],
                            v[v.size() * 9 / 10], v[v.size() * 95 / 100], v[v.size() * 99 / 100], v.back());
                }
                {
                    std::vector<int> order((size_t)c->nb);
                    for (int b2 = 0; b2 < c->nb; ++b2) order[(size_t)b2] = b2;
                    std::sort(order.begin(), order.end(), [&](int x, int y) { return h[(size_t)x * 16 + 5] > h[(size_t)y * 16 + 5]; });
                    for (int r = 0; r < 8 && r < c->nb; ++r) {
                        const int b2 = order[(size_t)r];
                        fprintf(stderr, "   slow workgroup %d:", b2);
                        for (int k : {0, 1, 2, 3, 4, 5}) fprintf(stderr, " [%d] %.2f", k, (double)(h[(size_t)b2 * 16 + k] - t0) * 0.01);
                        fprintf(stderr, "\n");
                    }
                }
            }
        }
#endif
        if (t + 1 == c->T) { c->cur = 0; c->cur_part = 0; }
    }
}

// The fixed-point form (step_fixed.hpp) serves what the prefix-count form does not: continuous weights and ESS-triggered schedules
// under systematic resampling, one population per context or one shard of an exchange-scope population.  Same hierarchy, same
// rotation; ancestors, decisions and evidence are integer-exact across tilings and shardings.
template <class Model>
bool fixed_eligible(const cpprob_hip_ctx* c)
{
    constexpr bool model_ok = std::is_same<Model, ModelLinearGaussian1D>::value || std::is_same<Model, ModelHmm3>::value || std::is_same<Model, ModelHmmK>::value;
    // (stratified and multinomial resampling run on the same integer masses; multinomial: one population per context)
    const bool own = c->cfg.n_global == c->cfg.n_particles || c->cfg.resample_scope == CPPROB_HIP_SCOPE_ISLAND;
    // (one interval of outputs per rank -- the strata form of multinomial resampling: one interval + the strata the ranks' boundaries cut)
    const bool systematic = c->cfg.resampler == CPPROB_HIP_RESAMPLE_SYSTEMATIC || c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED ||
                            (c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL && !(c->cfg.flags & CPPROB_HIP_FLAG_MULTINOMIAL_LITERAL));
    return model_ok && !c->force_fp && !(c->cfg.flags & CPPROB_HIP_FLAG_FLOATING_POINT_STEP) && c->nb <= kCountsMaxTiles && c->pop_n <= (1ull << 28) &&
           c->cfg.algorithm == CPPROB_HIP_ALG_SMC && !counts_eligible<Model>(c) &&
           (systematic ? (c->cfg.resample_scope == CPPROB_HIP_SCOPE_EXCHANGE || own) : (own && c->cfg.resample_scope != CPPROB_HIP_SCOPE_EXCHANGE));
}

static void fhier_view(const cpprob_hip_ctx* c, int copy, FHier& f)
{
    hier_view(c, copy, f.h);
    f.q0 = c->d_hier + (size_t)copy * c->hier_per_copy + c->hier_q0_off;
    f.m0 = c->d_hier + (size_t)copy * c->hier_per_copy + c->hier_m0_off;
}

// the copies step t reads / writes / clears (shared by both integer forms)
static void hier_rotation(cpprob_hip_ctx* c, int t, int& kp, int& kn, int& kc)
{
    if (t == 0) {
        // a run that was abandoned half-way leaves the rotation in an unknown state: start over from clean copies
        if (c->hier_run_open) { (void)hipMemsetAsync(c->d_hier, 0, c->hier_entries * sizeof(uint64_t), c->stream); c->hier_phase = 0; }
        c->hier_run_open = true; c->hier_phase_run = c->hier_phase;
    }
    kp = (t + c->hier_phase_run) % 3; kn = (kp + 1) % 3; kc = (kp + 2) % 3;
}

// Multinomial resampling, strata form (step_fixed.hpp): how many thresholds fall into each stratum does not depend on the weights --
// every step's counts in ONE launch (two above 64 tiles) in front of the run's first step.
static void launch_strata(cpprob_hip_ctx* c)
{
    if (!c->strata_pending) return;
    c->strata_pending = false;
    if (c->T < 2 || !c->d_strata) return;
    ProfScope ps(c, 5);
    StrataArgs sa{};
    // (a shard of a joint population draws the POPULATION's strata: every rank holds the whole table, a function of the seed alone)
    sa.seed = c->run_seed; sa.t0 = 1; sa.k = strata_k_of(c); sa.n_out = (uint32_t)strata_outputs(c); sa.offs = c->d_strata;
    if (sa.k <= kStrataTop) hipLaunchKernelGGL(multinomial_strata_kernel, dim3(1, c->T - 1), dim3(kThreads), 0, c->stream, sa);
    else {
        // (two sets of the steps' level-6 totals: the bottom launch clears the set the NEXT run adds into)
        sa.top = c->d_strata_top + (size_t)c->strata_phase * (size_t)c->T * 64; sa.top_clear = c->d_strata_top + (size_t)(c->strata_phase ^ 1) * (size_t)c->T * 64;
        c->strata_phase ^= 1;
        hipLaunchKernelGGL(multinomial_strata_top_kernel, dim3(strata_groups(sa.k), c->T - 1), dim3(kThreads), 0, c->stream, sa);
        hipLaunchKernelGGL(multinomial_strata_bottom_kernel, dim3(64, c->T - 1), dim3(kThreads), 0, c->stream, sa);
    }
}

template <class Model>
void launch_step_fixed(cpprob_hip_ctx* c, int t, const double* all_totals, int world, int rank)
{
    if constexpr (std::is_same<Model, ModelLinearGaussian1D>::value || std::is_same<Model, ModelHmm3>::value || std::is_same<Model, ModelHmmK>::value) {
        StepFixedArgs<Model> a{};
        a.mp = c->mp; a.obs = c->d_obs; a.t = t; a.T = c->T; a.n = c->n; a.ld = c->ld; a.rs = c->rs; a.seed = c->run_seed; a.pid0 = c->cfg.particle_offset;
        a.values = static_cast<typename Model::store_t*>(c->d_values); a.anc = c->d_anc;
        int kp, kn, kc;
        hier_rotation(c, t, kp, kn, kc);
        fhier_view(c, kp, a.f);
        a.f.h.to_next = (int64_t)(kn - kp) * (int64_t)c->hier_per_copy; a.f.h.to_clear = (int64_t)(kc - kp) * (int64_t)c->hier_per_copy;
        if (t == 0) { c->final_from_fixed = false; c->cur = 0; }
        if (t + 1 == c->T) { c->hier_phase = kn; c->final_from_fixed = true; c->final_copy = kn; c->final_bookkeep_pending = true; c->hier_run_open = false; }
        a.q_prev = c->d_q[c->cur]; a.q_next = c->d_q[c->cur ^ 1];
        a.logw_prev = c->d_logw[c->cur]; a.logw_next = c->d_logw[c->cur ^ 1];
        a.u0 = t > 0 ? host_resample_u0(c->run_seed, (uint64_t)t) : 0.0;
        a.bound = c->h_bound[(size_t)t]; a.bound_prev = t > 0 ? c->h_bound[(size_t)t - 1] : 0.0;
        a.ess_frac = c->cfg.ess_threshold; a.may_carry = c->cfg.ess_threshold > 1.0 ? 0 : 1;
        a.prefetch = a.may_carry ? 0 : 1;                        // (a schedule on which steps may not resample: the fetch is wasted on those, and costs registers on all)
        const int rs = c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED ? kFixStratified
                     : (c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL ? ((c->cfg.flags & CPPROB_HIP_FLAG_MULTINOMIAL_LITERAL) ? kFixMultinomialLiteral : kFixMultinomial) : kFixSystematic);
        if (rs == kFixMultinomial) {
            a.prefetch = 0;
            a.strata_k = strata_k_of(c);
            if (t == 0) launch_strata(c);
            a.strata_offs = t > 0 ? c->d_strata + (size_t)(t - 1) * (((size_t)1 << a.strata_k) + 1) : nullptr;
            a.cut = cut_view(c);
        }
        if (rs == kFixMultinomialLiteral) {
            // the lanes' in-tile prefixes travel with the weights (ping-pong, in the halves of the floating-point form's CDF array);
            // the tiles' prefix masses of generation t-1 come from one short launch in front of the step
            uint64_t* lp = reinterpret_cast<uint64_t*>(c->d_cdf);
            a.lane_prefix_prev = lp + (size_t)c->cur * (size_t)(c->ld / kPPT); a.lane_prefix_next = lp + (size_t)(c->cur ^ 1) * (size_t)(c->ld / kPPT);
            a.tile_prefix = reinterpret_cast<const uint64_t*>(c->d_bc);
            a.prefetch = 0;
            if (t > 0) {
                ProfScope ps(c, 5);
                hipLaunchKernelGGL(fixed_tile_prefix_kernel, dim3(1), dim3(kTilePrefixThreads), 0, c->stream, a.f.h.lvl[0], c->nb, reinterpret_cast<uint64_t*>(c->d_bc));
            }
        }
        a.ctrl = c->d_ctrl; a.n_pop = (double)c->pop_n; a.ess_trace = c->d_ess; a.resampled = c->d_resampled;
        a.all_totals = reinterpret_cast<const uint64_t*>(all_totals); a.world = world; a.rank = rank; a.annex_base = c->d_annex_base;
        a.row_w = c->keep ? t : (t & 1); a.row_r = t > 0 ? (c->keep ? t - 1 : ((t - 1) & 1)) : 0;
        if (!c->keep) a.anc = nullptr;
        {
            ProfScope ps(c, 0);
            // A/B form (CPPROB_HIP_FLAG_PAIRED_STEP_LAUNCH): on schedules where a step may not resample, the step as two launches, each ending
            // at once when the step is the other's (step_fixed.hpp: smc_step_fixed_carry_body).  Measured at configs[4]'s shard: the carry
            // launch takes 70 us where the two-form kernel's non-resampling launches take 81, and the second launch costs what that saves.
            // (the A/B form has no sharded build of the stratified / multinomial resampling launch: those shards take the one-launch step)
            const bool paired = a.may_carry && t > 0 && (c->cfg.flags & CPPROB_HIP_FLAG_PAIRED_STEP_LAUNCH) && rs != kFixMultinomialLiteral &&
                                !(all_totals != nullptr && rs != kFixSystematic);
            if (paired) {
                const bool sh = all_totals != nullptr;
                if (sh) hipLaunchKernelGGL((smc_step_fixed_carry_kernel<Model, true>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
                else hipLaunchKernelGGL((smc_step_fixed_carry_kernel<Model, false>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
                if (rs == kFixMultinomial) hipLaunchKernelGGL((smc_step_fixed_resampling_kernel<Model, false, kFixMultinomial>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
                else if (rs == kFixStratified && !sh) hipLaunchKernelGGL((smc_step_fixed_resampling_kernel<Model, false, kFixStratified>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
                else if (sh) hipLaunchKernelGGL((smc_step_fixed_resampling_kernel<Model, true, kFixSystematic>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
                else hipLaunchKernelGGL((smc_step_fixed_resampling_kernel<Model, false, kFixSystematic>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            }
            else if (rs == kFixMultinomial && all_totals) hipLaunchKernelGGL((smc_step_fixed_sharded_kernel<Model, false, kFixMultinomial>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (rs == kFixMultinomial) hipLaunchKernelGGL((smc_step_fixed_kernel<Model, false, kFixMultinomial>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (rs == kFixMultinomialLiteral) hipLaunchKernelGGL((smc_step_fixed_kernel<Model, false, kFixMultinomialLiteral>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (rs == kFixStratified && all_totals && a.prefetch) hipLaunchKernelGGL((smc_step_fixed_sharded_kernel<Model, true, kFixStratified>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (rs == kFixStratified && all_totals) hipLaunchKernelGGL((smc_step_fixed_sharded_kernel<Model, false, kFixStratified>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (rs == kFixStratified && a.prefetch) hipLaunchKernelGGL((smc_step_fixed_kernel<Model, true, kFixStratified>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (rs == kFixStratified && !Model::kIsInt) hipLaunchKernelGGL((smc_step_fixed_five_kernel<Model, kFixStratified>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (rs == kFixStratified) hipLaunchKernelGGL((smc_step_fixed_kernel<Model, false, kFixStratified>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (all_totals && a.prefetch) hipLaunchKernelGGL((smc_step_fixed_sharded_kernel<Model, true>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (all_totals) hipLaunchKernelGGL((smc_step_fixed_sharded_kernel<Model, false>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (a.prefetch) hipLaunchKernelGGL((smc_step_fixed_kernel<Model, true>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else if (!Model::kIsInt) hipLaunchKernelGGL((smc_step_fixed_five_kernel<Model>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
            else hipLaunchKernelGGL((smc_step_fixed_kernel<Model, false>), dim3(c->nb), dim3(kThreads), 0, c->stream, a);
        }
#ifdef CPPROB_STAMPS
        {
            static unsigned long long* d_st = nullptr;
            if (!d_st) { (void)hipMalloc(&d_st, (size_t)131072 * 16 * 8); (void)hipMemset(d_st, 0, (size_t)131072 * 16 * 8); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &d_st, sizeof(d_st)); }
            if (t >= 40 && t < 48 && getenv("CPPROB_STAMP_DUMP")) {
                (void)hipStreamSynchronize(c->stream);
                std::vector<unsigned long long> h((size_t)c->nb * 16);
                (void)hipMemcpy(h.data(), d_st, h.size() * 8, hipMemcpyDeviceToHost);
                int32_t rs_prev = 0; (void)hipMemcpy(&rs_prev, c->d_resampled + (t - 1), 4, hipMemcpyDeviceToHost);
                unsigned long long t0 = ~0ull; for (int b2 = 0; b2 < c->nb; ++b2) t0 = std::min(t0, h[(size_t)b2 * 16]);
                fprintf(stderr, "STAMPS fixed t=%d resampled=%d n=%lld (us since first workgroup start) mean/max:", t, rs_prev, (long long)c->n);
                for (int k = 0; k < 8; ++k) {
                    double acc = 0, mx = 0;
                    for (int b2 = 0; b2 < c->nb; ++b2) { const double v = (double)(h[(size_t)b2 * 16 + k] - t0) * 0.01; acc += v; mx = std::max(mx, v); }
                    fprintf(stderr, " [%d] %.2f/%.2f", k, acc / c->nb, mx);
                }
                fprintf(stderr, "\n");
                for (int k : {0, 7}) {
                    std::vector<double> v((size_t)c->nb);
                    for (int b2 = 0; b2 < c->nb; ++b2) v[(size_t)b2] = (double)(h[(size_t)b2 * 16 + k] - t0) * 0.01;
                    std::sort(v.begin(), v.end());
                    fprintf(stderr, "   stamp %d percentiles 10/25/50/75/80/85/90/95/99/100: %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f\n", k, v[v.size() / 10], v[v.size() / 4], v[v.size() / 2],
                            v[v.size() * 3 / 4], v[v.size() * 8 / 10], v[v.size() * 85 / 100], v[v.size() * 9 / 10], v[v.size() * 95 / 100], v[v.size() * 99 / 100], v.back());
                }
            }
        }
#endif
        c->cur ^= 1;
        if (!c->keep) {
            // filtering only: predict hit t's sums under the integer weights this step just left
            hipLaunchKernelGGL(filter_partials_fixed_kernel<Model>, dim3(c->smooth_grid), dim3(kThreads), 0, c->stream,
                               static_cast<const typename Model::store_t*>(c->d_values) + (int64_t)a.row_w * c->rs, (const uint32_t*)c->d_q[c->cur], c->n,
                               c->d_fpart + (size_t)t * (Model::kStats + 2) * c->smooth_grid);
        }
    }
}

static void fixed_final_view(cpprob_hip_ctx* c, FixedFinal& ff, bool bookkeep)
{
    fhier_view(c, c->final_copy, ff.f);
    ff.n_pop = (double)c->pop_n; ff.ess_frac = c->cfg.ess_threshold; ff.T = c->T; ff.bookkeep = bookkeep ? 1 : 0;
    ff.ctrl = c->d_ctrl; ff.ess_trace = c->d_ess; ff.resampled = c->d_resampled;
}

// The final generation's counts, as the read-out and the joint bookkeeping see them.
static void counts_final_view(cpprob_hip_ctx* c, CountsFinal& f, bool bookkeep)
{
    hier_view(c, c->final_copy, f.h);
    for (int k = 0; k < 4; ++k) f.e[k] = c->h_e_tab[(size_t)(c->T - 1) * 4 + k];
    f.n_pop = (double)c->pop_n; f.T = c->T; f.bookkeep = bookkeep ? 1 : 0; f.ctrl = c->d_ctrl; f.ess_trace = c->d_ess; f.resampled = c->d_resampled;
    f.filter_stats = c->keep ? nullptr : c->d_stats;
}

ScanArgs make_scan_args(cpprob_hip_ctx* c, int t, int phase, const double* all_totals, int world, int rank)
{
    ScanArgs sa{};
    sa.part = c->d_part[c->cur_part]; sa.nb = c->nb; sa.bc = c->d_bc; sa.bf = c->d_bf; sa.ctrl = c->d_ctrl; sa.t = t; sa.T = c->T;
    sa.n_pop = (double)c->pop_n; sa.n_local = (double)c->n; sa.ess_frac = c->cfg.ess_threshold; sa.seed = c->run_seed;
    sa.ess_trace = c->d_ess; sa.resampled = c->d_resampled;
    sa.force_no_resample = c->cfg.algorithm == CPPROB_HIP_ALG_SIS ? 1 : 0;
    sa.grid_refs = c->grid_refs ? 1 : 0;
    sa.exchange = (c->exchange && phase == 2) ? 1 : 0; sa.obound = c->d_obound;
    sa.all_totals = all_totals; sa.world = world; sa.rank = rank; sa.local_totals = c->totals_out ? c->totals_out : c->d_local_totals; sa.phase = phase;
    return sa;
}

void launch_scan(cpprob_hip_ctx* c, int t, int phase, const double* all_totals, int world, int rank)
{
    ScanArgs sa = make_scan_args(c, t, phase, all_totals, world, rank);
    ProfScope ps(c, 1);
    if (phase != 2 && c->nb > kSlabThreshold) {
        // large population: two multi-workgroup launches instead of one single-CU pass
        const int G = (c->nb + kSlabTiles - 1) / kSlabTiles;
        hipLaunchKernelGGL(scan_slab_partials_kernel, dim3(G), dim3(kThreads), 0, c->stream, sa.part, c->nb, c->d_gpart, sa.grid_refs);
        hipLaunchKernelGGL(scan_slab_finish_kernel, dim3(G), dim3(kThreads), 0, c->stream, sa, (const double*)c->d_gpart, G);
    } else {
        hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, c->stream, sa);
    }
}


// Workgroups of the trace-word read-out: each adds its counts into the shared counters (~100 atomics), so few of them while the pass
// is short -- 256 up to 4e6 particles (10^6: 12.6 us; 1024 workgroups: 21) -- and one per sixteen tiles beyond, up to 2048
// (10^8 particles: 430 -> 244 us).
static int trace_readout_grid(int64_t n)
{
    const int64_t tiles = (n + kTile - 1) / kTile;
    return (int)std::min<int64_t>(tiles, std::max<int64_t>(256, std::min<int64_t>(2048, tiles / 16)));
}

template <class Model>
void launch_smooth(cpprob_hip_ctx* c, bool with_paths)
{
    SmoothArgs<Model> a{};
    a.values = static_cast<const typename Model::store_t*>(c->d_values); a.anc = c->d_anc; a.wrel = c->d_wrel[c->cur]; a.bf = c->d_bf; a.ctrl = c->d_ctrl;
    a.resampled = c->d_resampled; a.T = c->T; a.n = c->n; a.ld = c->ld; a.rs = c->rs;
    a.identity = c->cfg.algorithm == CPPROB_HIP_ALG_SIS ? 1 : 0;
    a.stats_part = c->d_stats_part;
    a.paths = with_paths ? static_cast<typename Model::value_t*>(c->d_paths) : nullptr;
    a.rem = (c->x_remote && c->sharded) ? c->d_remote : nullptr;
    const size_t shm = (size_t)kWaves * c->T * Model::kStats * sizeof(double);
    // The walk's grid.  Its workgroups loop over tiles (kSmoothTiles at a time for one-byte states), so what a launch costs is
    // passes x rounds: a grid that is not a multiple of what the chip holds at once leaves its last round part-empty (2048 workgroups
    // at six a CU: 1536 + 512), and one that divides the tiles badly gives some workgroups a pass more than others.  Chosen once per
    // configuration: k x residency, k = 1 .. 4, with the least padded capacity (ties: the larger grid -- shorter chains per workgroup).
    // hmm<128> at 1.25e7 particles: 2048 -> 6144 workgroups, 1.38 -> 1.20 ms; linear_gaussian_1d<100> at 1e7 keeps 2048 (eight a CU).
    auto choose_grid = [&](auto kernel, int tiles_at_a_time = kSmoothTiles) -> int {
        if (c->walk_grid > 0) return c->walk_grid;
        int grid = c->smooth_grid, occ = 0;
        if (c->n_cu == 0) { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess) c->n_cu = v; }
        if (c->n_cu > 0 && hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, kThreads, shm) == hipSuccess && occ > 0) {
            const int64_t R = (int64_t)occ * c->n_cu, nt = c->nb;
            if (nt <= R) grid = (int)nt;
            else {
                double best = 1e300;
                for (int k = 1; k <= 4; ++k) {
                    const int64_t g = R * k;
                    if (g > c->walk_cap) break;
                    const int64_t per = (sizeof(typename Model::store_t) == 1 && tiles_at_a_time > 1 && nt > g) ? tiles_at_a_time : 1;
                    const int64_t passes = (nt + g * per - 1) / (g * per);
                    const double waste = (double)(passes * g * per) / (double)nt;
                    if (waste <= best * 1.01) { best = std::min(best, waste); grid = (int)std::min<int64_t>(g, nt); }
                }
            }
        }
        (void)hipGetLastError();
        c->walk_grid = grid;
        return grid;
    };
    int grid_used = c->smooth_grid;
    {
        ProfScope ps(c, 2);
        bool launched = false;
        if constexpr (Model::kWeightTable == 3 && sizeof(typename Model::store_t) == 1) {
            if (c->final_from_counts && c->sharded && c->trace_shard_run && !with_paths) {
                // one shard of a joint population: the same counting over this shard's words, un-normalised (the ranks' sums meet in the
                // run's final all-reduce); the final generation's bookkeeping came from the all-gathered totals
                TraceReadoutArgs ta{};
                ta.trace = c->d_tr[(c->T - 1) & 1]; ta.n = c->n; ta.T = c->T;
                counts_final_view(c, ta.f, false);
                ta.counters = c->d_trace_cnt; ta.arrive = c->d_trace_arrive; ta.stats = c->d_stats; ta.raw = 1; ta.n_local = (double)c->n;
                const int grid = trace_readout_grid(c->n);
                hipLaunchKernelGGL(trace_readout_kernel, dim3(grid), dim3(kThreads), 0, c->stream, ta);
                return;
            }
            if (c->final_from_counts && c->trace_mode && !with_paths) {
                // every particle carries its trace: one streaming pass, integer counts, statistics written by the last workgroup
                TraceReadoutArgs ta{};
                ta.trace = c->d_q[(c->T - 1) & 1]; ta.n = c->n; ta.T = c->T;
                counts_final_view(c, ta.f, c->final_bookkeep_pending);
                c->final_bookkeep_pending = false;
                ta.counters = c->d_trace_cnt; ta.arrive = c->d_trace_arrive; ta.stats = c->d_stats;
                const int grid = trace_readout_grid(c->n);
                hipLaunchKernelGGL(trace_readout_kernel, dim3(grid), dim3(kThreads), 0, c->stream, ta);
                return;
            }
            if (c->final_from_counts) {
                CountsFinal f{};
                counts_final_view(c, f, c->final_bookkeep_pending && !with_paths);
                if (!with_paths) c->final_bookkeep_pending = false;
                grid_used = choose_grid(smooth_counts_kernel<Model>);
                hipLaunchKernelGGL(smooth_counts_kernel<Model>, dim3(grid_used), dim3(kThreads), shm, c->stream, a, f);
                launched = true;
            }
        }
        if (!launched && c->final_from_fixed) {
            FixedFinal ff{};
            fixed_final_view(c, ff, c->final_bookkeep_pending && !with_paths);
            if (!with_paths) c->final_bookkeep_pending = false;
            bool int_walk = false;
            if constexpr (Model::kIsInt) {
                if (!a.rem) {                                            // every lineage on this device: the integer walk (step_fixed.hpp)
                    int_walk = true;
                    if (a.paths) {
                        grid_used = choose_grid(smooth_fixed_int_kernel<Model, true>, kSmoothTilesInt);
                        hipLaunchKernelGGL((smooth_fixed_int_kernel<Model, true>), dim3(grid_used), dim3(kThreads), shm, c->stream, a, ff, (const uint32_t*)c->d_q[c->cur]);
                    } else {
                        grid_used = choose_grid(smooth_fixed_int_kernel<Model, false>, kSmoothTilesInt);
                        hipLaunchKernelGGL((smooth_fixed_int_kernel<Model, false>), dim3(grid_used), dim3(kThreads), shm, c->stream, a, ff, (const uint32_t*)c->d_q[c->cur]);
                    }
                }
            }
            if (!int_walk) {
                grid_used = choose_grid(smooth_fixed_kernel<Model>);
                hipLaunchKernelGGL(smooth_fixed_kernel<Model>, dim3(grid_used), dim3(kThreads), shm, c->stream, a, ff, (const uint32_t*)c->d_q[c->cur]);
            }
            launched = true;
        }
        if (!launched) { grid_used = choose_grid(smooth_kernel<Model>); hipLaunchKernelGGL(smooth_kernel<Model>, dim3(grid_used), dim3(kThreads), shm, c->stream, a); }
    }
    if (with_paths && c->trace_mode && c->final_from_counts) return;     // (the statistics came from the trace words: the walk only materialises traces)
    ProfScope ps(c, 3);
    hipLaunchKernelGGL(finalize_kernel, dim3(c->T), dim3(kThreads), 0, c->stream,
                       c->d_stats_part, grid_used, c->T, Model::kStats, Model::kIsInt ? 1 : 0, c->d_ctrl, c->d_stats, c->sharded ? 0 : 1);
}

template <class F>
int dispatch_model(cpprob_hip_ctx* c, F&& f)
{
    switch (c->cfg.model) {
    case CPPROB_HIP_MODEL_GAUSSIAN_UNKNOWN_MEAN:
    case CPPROB_HIP_MODEL_GAUSSIAN_README: f(ModelGaussian{}); return 0;
    case CPPROB_HIP_MODEL_LINEAR_GAUSSIAN_1D: f(ModelLinearGaussian1D{}); return 0;
    case CPPROB_HIP_MODEL_HMM3: f(ModelHmm3{}); return 0;
    case CPPROB_HIP_MODEL_GAUSSIAN_2D_UNKNOWN_MEAN: f(ModelGaussianND{}); return 0;
    case CPPROB_HIP_MODEL_HMM_TABLE: f(ModelHmmK{}); return 0;
    }
    return fail(c, CPPROB_HIP_EINVAL, "unknown model id");
}

// Per-step tables of the table-weight HMMs from an observation, and the transition thresholds of CPPROB_HIP_MODEL_HMM_TABLE: ONE host
// statement of each, shared by the single-population begin and the batched begin (their draws and weights must agree bit for bit).
//   hmm3_step_table  log N(y; state_mean[s], 1) for s = 0..2 (the functor the reference applies per particle, utils_normal_distribution.hpp:20-45),
//                    e[s] = exp(ll_s - max ll) and max ll
//   hmmk_step_ll     log N(y; mean[s], 1) for s < k, -inf beyond (8 entries)
//   hmmk_thresholds  u >= c  <=>  word >= ceil(c 2^32) for the cumulative row weights, as for the three-state model ([k][8], ~0 beyond)
void hmm3_step_table(double y, const double (&mean)[3], double* ll, double* e, double& mx)
{
    for (int s2 = 0; s2 < 3; ++s2) ll[s2] = normal_logpdf(y, mean[s2], 1.0);
    mx = std::max(ll[0], std::max(ll[1], ll[2]));
    for (int s2 = 0; s2 < 3; ++s2) e[s2] = std::exp(ll[s2] - mx);
}
void hmmk_step_ll(double y, const std::vector<double>& mean, int k, double* ll)
{
    for (int s2 = 0; s2 < 8; ++s2) ll[s2] = s2 < k ? normal_logpdf(y, mean[(size_t)s2], 1.0) : -INFINITY;
}
// a scaled table's row (csrc/batch_scale.hpp): the statements the device's re-table writes it with, not normal_logpdf's logarithm
void scale_step_ll(double y, const double* mean, const double* sigma, const double* log_norm, int k, double* ll)
{
    for (int s2 = 0; s2 < 8; ++s2) ll[s2] = s2 < k ? scale_entry(y, mean[s2], sigma[s2], log_norm[s2]) : -INFINITY;
}
// a Poisson table's row (csrc/batch_poisson.hpp), with the statements the device's re-table writes it with
void poisson_step_ll(double y, const double* rate, const double* log_rate, const double* lf, int k, double* ll)
{
    for (int s2 = 0; s2 < 8; ++s2) ll[s2] = s2 < k ? poisson_entry(y, rate[s2], log_rate[s2], lf) : -INFINITY;
}
// The emission family of a table batch and of a call that hands tables over: N(mean, 1), N(mean, sigma) or Poisson(rate).
enum EmissionFamily { kFamilyUnit = 0, kFamilyScaled = 1, kFamilyPoisson = 2 };
std::vector<uint64_t> hmmk_thresholds(const std::vector<double>& trans, int k)
{
    std::vector<uint64_t> thr((size_t)k * 8, ~0ull);
    for (int s2 = 0; s2 < k; ++s2) {
        double tot = 0.0, acc = 0.0;
        for (int j = 0; j < k; ++j) tot += trans[(size_t)s2 * k + j];
        for (int j = 0; j + 1 < k; ++j) { acc += trans[(size_t)s2 * k + j]; thr[(size_t)s2 * 8 + j] = (uint64_t)std::ceil((acc / tot) * 4294967296.0); }
    }
    return thr;
}

void free_run_buffers(cpprob_hip_ctx* c)
{
    dfree(c->d_obs); dfree(c->d_logw[0]); dfree(c->d_logw[1]); dfree(c->d_wrel[0]); dfree(c->d_wrel[1]); dfree(c->d_bf); dfree(c->d_ll_tab); dfree(c->d_values); dfree(c->d_anc); dfree(c->d_paths);
    dfree(c->d_part[0]); dfree(c->d_part[1]); dfree(c->d_e_tab); dfree(c->d_gpart); dfree(c->d_stile); dfree(c->d_gstat); dfree(c->d_bc); dfree(c->d_ess); dfree(c->d_resampled); dfree(c->d_stats_part); dfree(c->d_stats);
    dfree(c->d_cdf); dfree(c->d_anc_pre); dfree(c->d_strata); dfree(c->d_strata_top); dfree(c->d_lz_trace); dfree(c->d_obound); dfree(c->d_hier); dfree(c->d_annex_base); dfree(c->d_fpart); dfree(c->d_filter_w); dfree(c->d_skip); dfree(c->d_q[0]); dfree(c->d_q[1]); dfree(c->d_trace_cnt); dfree(c->d_trace_arrive); dfree(c->d_fold); dfree(c->d_tr[0]); dfree(c->d_tr[1]);
    c->cap_particles = 0; c->cap_T = 0; c->annex_cap = 0; c->tr_cap = 0;
}

// ---- batched SMC (cpprob_hip_batch_*, csrc/batch_smc.hpp) -------------------------------------------------------------------------
// Device workspace of a batch: regions side by side, each starting on a 256-byte boundary; an empty region takes no bytes.
//   uniform    (cpprob_hip_batch_begin: T_rows = T, tables = 1, no descriptors, entries = B T n): ten regions,
//              cpprob_hip_batch_workspace_bytes states the sum
//   described  (cpprob_hip_batch_begin_problems: T_rows = T_max, tables = B, descriptors and dispatch order, entries = sum of T_b n_b,
//              the particle store packed): twelve regions, cpprob_hip_batch_problems_workspace_bytes states the sum
//   online     (cpprob_hip_batch_begin_online: a described batch of the capacities, then every problem's first step of a launch, its
//              snapshot and, filtering, its carried generation -- carry = sum of n_b): cpprob_hip_batch_online_workspace_bytes
//   masses     (CPPROB_HIP_BATCH_KEEP_MASSES, any of the three; keep_history = 0): the m table [B][T_rows][8] last, so that every
//              other region sits where it sits without the bit
struct BatchLayout { size_t tab, seeds, thr, ctrl, stats, ess, res, nreq, prob, order, values, anc, first, snap, carry, mass, total; };
size_t batch_round(size_t x) { return (x + 255) / 256 * 256; }
inline bool batch_masses(const cpprob_hip_batch_config* cfg) { return (cfg->flags & CPPROB_HIP_BATCH_KEEP_MASSES) != 0; }
BatchLayout batch_layout(uint64_t B, uint64_t T_rows, uint64_t tables, bool described, uint64_t entries, int spp, bool keep, bool online = false, uint64_t carry = 0, bool masses = false)
{
    BatchLayout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += batch_round(bytes); return at; };
    L.tab = take(B * T_rows * kBatchTab * sizeof(double));
    L.seeds = take(B * sizeof(uint64_t));
    L.thr = take(tables * 64 * sizeof(uint64_t));
    L.ctrl = take(B * kBatchCtrlBytes);
    L.stats = take(B * T_rows * (uint64_t)spp * sizeof(double));
    L.ess = take(B * T_rows * sizeof(double));
    L.res = take(B * T_rows * sizeof(int32_t));
    L.nreq = take(B * sizeof(int32_t));
    L.prob = take(described ? B * sizeof(BatchProblem) : 0);
    L.order = take(described ? B * sizeof(int32_t) : 0);
    L.values = take(keep ? entries : 0);
    L.anc = take(keep ? entries * sizeof(int32_t) : 0);
    L.first = take(online ? B * sizeof(int32_t) : 0);
    L.snap = take(online ? B * sizeof(BatchSnap) : 0);
    L.carry = take(online && !keep ? carry : 0);
    L.mass = take(masses ? B * T_rows * 8 * sizeof(double) : 0);
    L.total = o;
    return L;
}
struct BatchProblemsShape { uint64_t T_max = 0, n_max = 0, steps = 0, particles = 0; };      // steps = sum of T_b n_b, particles = sum of n_b

struct BatchState {
    cpprob_hip_batch_config cfg{};
    bool begun = false, ran = false;
    std::vector<BatchProblem> prob;            // [B]: every problem's T, n and first entry in the particle store (a uniform batch's too)
    bool described = false;                    // cpprob_hip_batch_begin_problems: descriptors, dispatch order and a threshold table a problem on the device
    int T = 0, K = 0, hk = 0;                  // T: rows a problem holds in the small regions (the longest problem's)
    BatchLayout lay{};
    std::vector<double> h_tab;                 // [B][T][kBatchTab]: the per-step tables the kernel reads (also the final log-weights' source)
    std::vector<uint64_t> h_thr;               // HMM_TABLE: the rows' thresholds at begin
    DeviceBuffer d_ws;
    char* ws() const { return d_ws.as<char>(); }
    ModelParams mp{};
    // a batch advanced in pieces (cpprob_hip_batch_begin_online): prob[b].T is the length reached, prob[b].store the problem's first
    // entry in a store sized by the capacities (keep_history = 1) or its first byte in the carry region (keep_history = 0)
    bool online = false, walked = true;        // walked: the statistics on the device are those of the lengths reached
    std::vector<char> walked_b;                // [B]: ... problem b's (keep_history = 1: the lineage walk has run over its rows)
    std::vector<uint32_t> cap_T;               // [B]
    std::vector<double> means;                 // HMM_TABLE: [tables][hk], the rows an advance evaluates its steps' tables with
    std::vector<double> trans;                 // HMM_TABLE with per-problem tables: [B][hk][hk], what cpprob_hip_batch_learn_begin uploads
    PinnedBuffer pin_tab;                      // pinned mirror of the table region: an advance writes its new rows only
    // pinned descriptors of an advance in flight, kOnlineSlots in turn: {BatchProblem[B], first[B], order[B]}; a slot is written
    // again once the copies that read it have run (its event); the ring's count is the advances since the begin
    static constexpr int kOnlineSlots = 4;
    SlotRing<kOnlineSlots> advance_ring;
    // posterior traces (cpprob_hip_batch_paths, _paths_device; csrc/batch_paths.hpp): the problems' descriptors on the device, their
    // pinned sources (kOnlineSlots in turn, as an advance's) and the host variant's device staging; none of it in the workspace
    DeviceBuffer d_pdesc;
    SlotRing<kOnlineSlots> paths_ring;
    DeviceBuffer d_stage;
    // backward smoothing (cpprob_hip_batch_smooth*, _smooth_lag*; csrc/batch_smooth.hpp): the m table ([sum of T_b][8] doubles -- an
    // online batch: of its capacities, rows never move --, grown lazily), the problems' descriptors with the HMM3 thresholds behind
    // them, and their pinned sources, kOnlineSlots in turn
    DeviceBuffer d_mass;
    // (a filtering batch with CPPROB_HIP_BATCH_KEEP_MASSES has its m table in the workspace, written by the run: none of these three)
    std::vector<uint32_t> counted;             // [B], online batch: its rows [0, counted_b) of the m table are valid (any begin: none)
    DeviceBuffer d_sdesc;                      // (as large as a slot of the ring: a call copies the whole slot)
    SlotRing<kOnlineSlots> smooth_ring;
    unsigned smooth_gy_count = 0, smooth_gy_lag = 0;        // gridDim.y of the last smoothing call's counting and lag launches (0: none)
    // of the last decode / forecast / predictive call: gridDim.x of the forward launch, gridDim.y of the trace, forecast and predictive launches (0: none)
    unsigned decode_gx_forward = 0, decode_gy_trace = 0, forecast_gy = 0, predictive_gy = 0;
    unsigned traj_stats_gy = 0;                             // gridDim.y of the last trajectory statistics launch (0: none)
    // decoding (cpprob_hip_batch_decode*; csrc/batch_decode.hpp): the step words (addressed as the m table's rows: an online batch's by
    // capacity, kept), the v rows [B][8] and the log tables ([tables][64], computed on the host at the first call after a begin and
    // uploaded once), allocations of the context's own; decoded: [B], online batch: its words [0, decoded_b) and its v row are valid
    // (any begin: none)
    DeviceBuffer d_words, d_v, d_lp;
    std::vector<double> h_lp; double lp0 = 0.0;
    bool lp_ready = false, lp_sent = false;
    std::vector<uint32_t> decoded;
    // running statistics (cpprob_hip_batch_online_stats*; csrc/batch_onlinestats.hpp): tau [B][8][88], an allocation of the context's
    // own; ostats_done: [B], online batch: the steps [0, ostats_done_b) are in its tau (any begin: none -- a problem at 0 never reads tau)
    DeviceBuffer d_tau;
    std::vector<uint32_t> ostats_done;
    // conditional runs (cpprob_hip_batch_run_conditional*; csrc/batch_csmc.hpp): conditional: the last run was one -- it keeps masses, not
    // books, and cpprob_hip_batch_results is refused until the next cpprob_hip_batch_run; a described batch's first entries in the
    // reference paths ([B] int64, the lengths are fixed at begin: written and uploaded at the first conditional run after it) with
    // their pinned source, allocations of the context's own
    bool conditional = false, cfirst_ready = false;
    DeviceBuffer d_cfirst; PinnedBuffer pin_cfirst;
    // re-tabling (cpprob_hip_batch_retable*; csrc/batch_retable.hpp): the status words [B] and the observes the host form staged, allocations
    // of the context's own; retabled: the begun batch has been re-tabled (its status words are those of the last one); robs_ready: d_robs
    // holds this begun batch's observes; tab_stale / thr_stale: the device holds rows / thresholds the host mirrors (h_tab, h_thr) do not
    DeviceBuffer d_rstatus, d_robs;
    bool retabled = false, robs_ready = false, tab_stale = false, thr_stale = false;
    unsigned retable_gy = 0;                                // gridDim.y of the last re-table launch (0: none)
    // online EM (cpprob_hip_batch_learn_*; csrc/batch_learn.hpp): own_tables: the batch was begun with per-problem tables; armed: the
    // begun online batch learns its tables -- the step sizes [n_gamma], the device-resident tables (means [B][k], transition [B][k][k]),
    // the learner's tau [B][8][88], the records [B][88], the status words [B], the first new observes of an advance ([B] int64, with
    // their pinned sources, kOnlineSlots in turn as an advance's descriptors) and the host form's copy of an advance's observes,
    // allocations of the context's own, in the order above
    // learn_tied: the armed batch's learner pools over the tie in force (cpprob_hip_batch_learn_tie; csrc/batch_learn_tied.hpp): the streams
    // of a group learn one table; arming again or any begin clears it
    bool own_tables = false, armed = false, learn_tied = false;
    uint32_t learn_t_min = 0;
    struct Learner {
        DeviceBuffer gamma, means, trans, tau, rec, obs, status, first;
        PinnedBuffer pin_first;
        DeviceBuffer pooled;                                // tied online EM (cpprob_hip_batch_learn_tie): the groups' pooled records [G][88]
        void release() { for (DeviceBuffer* b : {&gamma, &means, &trans, &tau, &rec, &obs, &status, &first, &pooled}) b->release(); pin_first.release(); }
    } learn;
    // per-state emission scales (cpprob_hip_batch_begin_problems_scaled, _begin_online_scaled; csrc/batch_scale.hpp): scaled: the begun
    // batch has them; the sigmas and log_norms in force, [B][8] (states >= k zero), on the host as the last begin or host call
    // (cpprob_hip_batch_retable_scaled, _online_tables_scaled) left them and on the device (allocations of the context's own) as the
    // last re-table or learn step left them; learn_scales / learn_floor: the armed batch's learner fits the scales
    // (cpprob_hip_batch_learn_begin_scaled) -- the host mirrors are stale from its first advance on, and nothing reads them then
    bool scaled = false, learn_scales = false;
    double learn_floor = 0.0;
    std::vector<double> sigmas, log_norms;
    DeviceBuffer d_sigma, d_lognorm;
    // Poisson emissions (cpprob_hip_batch_begin_problems_poisson, _begin_online_poisson; csrc/batch_poisson.hpp): poisson: the begun batch
    // has them, and is then not scaled.  The rates in force and their logarithms stand where a scaled batch's sigmas and log_norms stand
    // (sigmas / log_norms on the host, d_sigma / d_lognorm on the device, [B][8]), under the same mirror rules; the log-factorials
    // (lfact, kPoissonMaxCount + 1 doubles) are filled at the context's first Poisson begin and uploaded once
    bool poisson = false;
    std::vector<double> lfact;
    DeviceBuffer d_lfact;
    // a tie (cpprob_hip_batch_tie; csrc/batch_pool.hpp): tied: the begun batch's problems are partitioned into tie_groups groups; one
    // allocation of the context's own holds the members sorted by (group, problem) [B], the groups' first positions [G + 1] and the
    // map problem -> group [B]; tie_map is the host's copy of the map.  A re-table keeps it, any begin forgets it.
    bool tied = false;
    int32_t tie_groups = 0;
    std::vector<int32_t> tie_map;
    DeviceBuffer d_tie;
    const double* tab_host() const { return online ? pin_tab.as<double>() : h_tab.data(); }
};

// Disarms: the learner's allocations go (hipFree waits for the device: no kernel still reads them).
void batch_learn_free(BatchState* bs)
{
    bs->learn.release();
    bs->armed = false; bs->learn_tied = false;
}

// The state goes with everything it owns.  The workspace first: hipFree waits for the device, so no copy still reads a pinned buffer
// when the members' destructors free them.
void batch_free(cpprob_hip_ctx* c)
{
    if (!c->batch) return;
    c->batch->d_ws.release();
    delete c->batch;
    c->batch = nullptr;
}

// What a configuration and T admit, without a device: 0, or the error code with its message.
int batch_check(const cpprob_hip_batch_config* cfg, size_t T, std::string& msg)
{
    if (!cfg) { msg = "NULL argument"; return CPPROB_HIP_EINVAL; }
    if (cfg->algorithm == CPPROB_HIP_ALG_SIS) { msg = "batched runs are SMC only: SIS runs on the single-population path (cpprob_hip_infer_begin / _run)"; return CPPROB_HIP_EUNSUPPORTED; }
    if (cfg->algorithm != CPPROB_HIP_ALG_SMC) { msg = "unknown algorithm"; return CPPROB_HIP_EINVAL; }
    if (cfg->model < 0 || cfg->model > CPPROB_HIP_MODEL_HMM_TABLE) { msg = "unknown model id"; return CPPROB_HIP_EINVAL; }
    if (cfg->model != CPPROB_HIP_MODEL_HMM3 && cfg->model != CPPROB_HIP_MODEL_HMM_TABLE) {
        msg = "batched runs hold the table-weight HMMs (CPPROB_HIP_MODEL_HMM3, CPPROB_HIP_MODEL_HMM_TABLE): run this model one problem at a time on the "
              "single-population path (cpprob_hip_infer_begin / _run)";
        return CPPROB_HIP_EUNSUPPORTED;
    }
    if (cfg->resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL) { msg = "batched runs resample systematically or stratified: multinomial resampling runs on the single-population path (cpprob_hip_infer_begin / _run)"; return CPPROB_HIP_EUNSUPPORTED; }
    if (cfg->resampler != CPPROB_HIP_RESAMPLE_SYSTEMATIC && cfg->resampler != CPPROB_HIP_RESAMPLE_STRATIFIED) { msg = "unknown resampler"; return CPPROB_HIP_EINVAL; }
    if (!(cfg->ess_threshold > 1.0)) { msg = "batched runs resample after every step (ess_threshold > 1): ESS-triggered schedules run on the single-population path (cpprob_hip_infer_begin / _run)"; return CPPROB_HIP_EUNSUPPORTED; }
    if (cfg->keep_history != 0 && cfg->keep_history != 1) { msg = "keep_history must be 0 or 1"; return CPPROB_HIP_EINVAL; }
    if (cfg->flags & ~CPPROB_HIP_BATCH_KEEP_MASSES) { msg = "flags are reserved and must be 0"; return CPPROB_HIP_EINVAL; }
    if (cfg->flags && cfg->keep_history == 1) { msg = "CPPROB_HIP_BATCH_KEEP_MASSES is for filtering-only batches (keep_history = 0): a batch with keep_history = 1 is smoothed from its particle store"; return CPPROB_HIP_EINVAL; }
    if (cfg->n_particles == 0 || cfg->n_particles > (uint64_t)kBatchMaxN) { msg = "n_particles per problem must lie in 1 .. " + std::to_string(kBatchMaxN); return CPPROB_HIP_EINVAL; }
    if (cfg->n_problems == 0 || cfg->n_problems > (uint64_t)INT32_MAX) { msg = "n_problems must lie in 1 .. 2^31 - 1"; return CPPROB_HIP_EINVAL; }
    if (T == 0 || T > (size_t)INT32_MAX) { msg = "every problem needs 1 .. 2^31 - 1 observes"; return CPPROB_HIP_EINVAL; }
    const long double est = (long double)cfg->n_problems * (long double)T * (64.0L + 8 * 8 + 12 + (cfg->keep_history ? 5.0L * cfg->n_particles : 0.0L));
    if (est > 1e18L) { msg = "the batch's workspace does not fit 64-bit sizes"; return CPPROB_HIP_EINVAL; }
    return 0;
}

// The same for a batch of problems with their own shapes: batch_check first (T = the longest problem's), then every T_b and n_b.
int batch_check_problems(const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n, BatchProblemsShape& sh, std::string& msg)
{
    sh = BatchProblemsShape();
    const bool scan = cfg && h_T && h_n && cfg->n_problems <= (uint64_t)INT32_MAX;
    if (scan) for (uint64_t b = 0; b < cfg->n_problems; ++b) sh.T_max = std::max<uint64_t>(sh.T_max, h_T[b]);
    if (int rc = batch_check(cfg, scan ? (size_t)sh.T_max : 1, msg)) return rc;
    if (!h_T || !h_n) { msg = "NULL argument"; return CPPROB_HIP_EINVAL; }
    for (uint64_t b = 0; b < cfg->n_problems; ++b) {
        if (h_T[b] == 0 || h_T[b] > (uint32_t)INT32_MAX) { msg = "problem " + std::to_string(b) + ": every problem needs 1 .. 2^31 - 1 observes"; return CPPROB_HIP_EINVAL; }
        if (h_n[b] == 0 || h_n[b] > cfg->n_particles) {
            msg = "problem " + std::to_string(b) + ": its particle count must lie in 1 .. cfg->n_particles (the batch's largest)";
            return CPPROB_HIP_EINVAL;
        }
        sh.n_max = std::max<uint64_t>(sh.n_max, h_n[b]);
        sh.steps += (uint64_t)h_T[b] * h_n[b];
        sh.particles += h_n[b];
    }
    return 0;
}

// The host mirrors of a scaled batch ([B][8]): the scales in force and their logarithms, with the statements the device's re-table
// evaluates (csrc/batch_scale.hpp).
void batch_mirror_scales(BatchState* bs, size_t B, int k, const double* h_sigmas)
{
    for (size_t b = 0; b < B; ++b)
        for (size_t s = 0; s < (size_t)k; ++s) {
            bs->sigmas[b * 8 + s] = h_sigmas[b * (size_t)k + s];
            bs->log_norms[b * 8 + s] = scale_log_norm(h_sigmas[b * (size_t)k + s]);
        }
}

// The same mirrors of a Poisson batch: the rates in force and their logarithms (csrc/batch_poisson.hpp).
void batch_mirror_rates(BatchState* bs, size_t B, int k, const double* h_rates)
{
    for (size_t b = 0; b < B; ++b)
        for (size_t s = 0; s < (size_t)k; ++s) {
            bs->sigmas[b * 8 + s] = h_rates[b * (size_t)k + s];
            bs->log_norms[b * 8 + s] = table_log(h_rates[b * (size_t)k + s]);
        }
}

// Begins a checked batch.  Described (h_T, h_n given): problem b has h_T[b] observes, consecutive in h_obs, and h_n[b] particles;
// uniform (both NULL): every problem has T_max observes and cfg->n_particles particles.  HMM_TABLE of k states: problem b's own table
// (h_means [B][k], h_transition [B][k][k]) or, both NULL, the table of cpprob_hip_set_hmm.
// Online (h_T = the capacities, h_obs NULL, h_seeds given): every problem starts without observes; cpprob_hip_batch_advance evaluates
// its rows, with the statements below, as they arrive.
int batch_begin(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, size_t T_max, const uint32_t* h_T, const uint32_t* h_n, const double* h_obs,
                int k, const double* h_means, const double* h_transition, const uint64_t* h_seeds = nullptr, const double* h_sigmas = nullptr,
                EmissionFamily family = kFamilyUnit)
{
    // (a Poisson begin: h_means are the rates)
    const bool online = h_seeds != nullptr, scaled = family == kFamilyScaled, poisson = family == kFamilyPoisson;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->batch) c->batch = new BatchState();
    BatchState* bs = c->batch;
    bs->begun = false; bs->ran = false; bs->conditional = false; bs->cfirst_ready = false;
    const uint64_t B = cfg->n_problems;
    bs->counted.assign(B, 0);
    bs->decoded.assign(B, 0); bs->lp_ready = false; bs->lp_sent = false;
    bs->ostats_done.assign(B, 0);
    bs->retabled = false; bs->robs_ready = false; bs->tab_stale = false; bs->thr_stale = false; bs->retable_gy = 0;
    bs->tied = false; bs->tie_groups = 0; bs->tie_map.clear();              // (any begin forgets the tie)
    if (bs->armed) batch_learn_free(bs);
    const bool hmm3 = cfg->model == CPPROB_HIP_MODEL_HMM3, described = h_T != nullptr, own = h_means != nullptr;
    const int spp = hmm3 ? 3 : 8;
    const uint64_t tables = described ? B : 1;
    host_model_params(bs->mp, cfg->model);
    bs->mp.hk = hmm3 ? 0 : k;
    // the per-step tables and thresholds of every problem, with the single path's own host expressions (cpprob_hip_infer_begin) on the
    // problem's means / transition rows; rows t >= T_b stay zero
    bs->online = false;
    if (online) {
        // (advances of the batch this one replaces may still read the pinned buffers)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const size_t tab_bytes = (size_t)B * T_max * kBatchTab * sizeof(double);
        HIP_TRY(c, bs->pin_tab.grow(c->stream, tab_bytes));
        std::memset(bs->pin_tab.as<double>(), 0, tab_bytes);
        HIP_TRY(c, bs->advance_ring.reserve(c->stream, batch_round((size_t)B * (sizeof(BatchProblem) + 2 * sizeof(int32_t)))));
        bs->advance_ring.restart();
        bs->cap_T.assign(h_T, h_T + B);
        bs->walked_b.assign(B, 1);
        bs->means.clear(); bs->trans.clear();
        bs->h_tab.clear();
    } else bs->h_tab.assign((size_t)B * T_max * kBatchTab, 0.0);
    bs->h_thr.assign((size_t)tables * 64, ~0ull);
    bs->prob.resize(B);
    bs->scaled = false; bs->poisson = false; bs->sigmas.clear(); bs->log_norms.clear();
    if (scaled || poisson) {
        bs->sigmas.assign((size_t)B * 8, 0.0); bs->log_norms.assign((size_t)B * 8, 0.0);
        if (scaled) batch_mirror_scales(bs, (size_t)B, k, h_sigmas);
        else batch_mirror_rates(bs, (size_t)B, k, h_means);
        HIP_TRY(c, bs->d_sigma.grow(c->stream, B * 8 * sizeof(double)));
        HIP_TRY(c, bs->d_lognorm.grow(c->stream, B * 8 * sizeof(double)));
    }
    if (poisson && bs->lfact.empty()) {
        // the context's first Poisson begin: the log-factorials, once (hipMemcpy of pageable memory has read them when it returns)
        std::vector<double> lf((size_t)kPoissonMaxCount + 1);
        poisson_log_fact_table(lf.data());
        HIP_TRY(c, bs->d_lfact.grow(c->stream, lf.size() * sizeof(double)));
        HIP_TRY(c, hipMemcpyAsync(bs->d_lfact.as<double>(), lf.data(), lf.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        bs->lfact.swap(lf);
    }
    std::vector<double> mean, trans;
    if (!hmm3 && !own) { mean = c->hk_mean; trans = c->hk_trans; }
    std::vector<uint64_t> thr;
    size_t at_obs = 0;
    int64_t at_store = 0, at_carry = 0;
    if (online && !hmm3 && !own) bs->means = mean;
    for (uint64_t b = 0; b < B; ++b) {
        const size_t T_b = described ? h_T[b] : T_max, n_b = described ? h_n[b] : (size_t)cfg->n_particles;
        if (own) { mean.assign(h_means + b * (size_t)k, h_means + (b + 1) * (size_t)k); trans.assign(h_transition + b * (size_t)k * k, h_transition + (b + 1) * (size_t)k * k); }
        if (online && own) { bs->means.insert(bs->means.end(), mean.begin(), mean.end()); bs->trans.insert(bs->trans.end(), trans.begin(), trans.end()); }
        for (size_t t = 0; t < (online ? 0 : T_b); ++t) {
            const double y = h_obs[at_obs + t];
            double* row = &bs->h_tab[(b * T_max + t) * kBatchTab];
            if (hmm3) hmm3_step_table(y, bs->mp.hmm_mean, row, row + 3, row[6]);
            else if (scaled) scale_step_ll(y, mean.data(), &bs->sigmas[b * 8], &bs->log_norms[b * 8], k, row);
            else if (poisson) poisson_step_ll(y, &bs->sigmas[b * 8], &bs->log_norms[b * 8], bs->lfact.data(), k, row);
            else hmmk_step_ll(y, mean, k, row);
        }
        if (!hmm3 && b < tables) {
            if (own || b == 0) thr = hmmk_thresholds(trans, k);
            std::copy(thr.begin(), thr.end(), bs->h_thr.begin() + (size_t)b * 64);
        }
        bs->prob[b].T = online ? 0 : (int32_t)T_b; bs->prob[b].n = (int32_t)n_b;
        bs->prob[b].store = online && cfg->keep_history != 1 ? at_carry : at_store;
        at_obs += T_b;
        at_store += (int64_t)(T_b * n_b);
        at_carry += (int64_t)n_b;
    }
    bs->lay = batch_layout(B, T_max, tables, described, (uint64_t)at_store, spp, cfg->keep_history == 1, online, (uint64_t)at_carry, batch_masses(cfg));
    HIP_TRY(c, bs->d_ws.grow(c->stream, bs->lay.total));        // (the previous workspace may still be read by a batch in flight)
    if (online) HIP_TRY(c, hipMemsetAsync(bs->ws() + bs->lay.tab, 0, (size_t)B * T_max * kBatchTab * sizeof(double), c->stream));
    else HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.tab, bs->h_tab.data(), bs->h_tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.thr, bs->h_thr.data(), bs->h_thr.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    if (scaled || poisson) {
        HIP_TRY(c, hipMemcpyAsync(bs->d_sigma.as<double>(), bs->sigmas.data(), B * 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(bs->d_lognorm.as<double>(), bs->log_norms.data(), B * 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    std::vector<int32_t> order;                               // (lives until the synchronisation below)
    std::vector<char> ctrl0;
    if (online) {
        // no observes yet: a problem's summary reads as zeros (log_norm = M + log W) until its first advance
        ctrl0.assign((size_t)B * kBatchCtrlBytes, 0);
        StepCtrl z{};
        z.W = 1.0;
        for (uint64_t b = 0; b < B; ++b) std::memcpy(ctrl0.data() + b * kBatchCtrlBytes, &z, sizeof z);
        HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.ctrl, ctrl0.data(), ctrl0.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.seeds, h_seeds, B * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(bs->ws() + bs->lay.nreq, 0, B * sizeof(int32_t), c->stream));
        HIP_TRY(c, hipMemsetAsync(bs->ws() + bs->lay.snap, 0, B * sizeof(BatchSnap), c->stream));
    }
    if (described) {
        // the longest chains first (steps x LDS passes a step), ties by index: the launch's tail is made of short problems; no result
        // depends on the order
        order.resize(B);
        for (uint64_t b = 0; b < B; ++b) order[b] = (int32_t)b;
        auto cost = [&](int32_t b) { return (uint64_t)h_T[b] * ((h_n[b] + (uint64_t)kTile - 1) / kTile); };
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return cost(x) > cost(y); });
        HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.prob, bs->prob.data(), B * sizeof(BatchProblem), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.order, order.data(), B * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        // the padded rows t >= T_b are never written by a run: zero once (the workspace may have held another batch)
        HIP_TRY(c, hipMemsetAsync(bs->ws() + bs->lay.stats, 0, B * T_max * (size_t)spp * sizeof(double), c->stream));
        HIP_TRY(c, hipMemsetAsync(bs->ws() + bs->lay.ess, 0, B * T_max * sizeof(double), c->stream));
        HIP_TRY(c, hipMemsetAsync(bs->ws() + bs->lay.res, 0, B * T_max * sizeof(int32_t), c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    bs->cfg = *cfg; bs->T = (int)T_max; bs->K = spp; bs->hk = k; bs->described = described;
    bs->online = online; bs->walked = true; bs->own_tables = own; bs->scaled = scaled; bs->poisson = poisson;
    bs->begun = true; bs->ran = online;         // (an online batch has results from its begin on: those of no observes)
    return 0;
}

// The packed layout of a batch's traces (cpprob_hip_batch_paths_layout): problem b's T_b x m_b entries from first[b] on and its m_b
// weights from wfirst[b] on, m_b = n_b or min(n_b, max_particles); a problem of length 0 owns neither.  first[B] / wfirst[B]: the totals.
inline uint64_t batch_paths_m(uint64_t n, uint64_t max_particles) { return max_particles && max_particles < n ? max_particles : n; }

// The eight kernels of cpprob_hip_batch_run, and the eight of cpprob_hip_batch_advance; a filtering batch that keeps its masses
// (CPPROB_HIP_BATCH_KEEP_MASSES) has four of its own for either.
using BatchKernel = void (*)(BatchArgs);
template <class Model, bool RESUME>
BatchKernel batch_kernel(bool stratified, bool keep, bool masses)
{
    static constexpr BatchKernel k[2][2] = {{batch_smc_kernel<Model, kFixSystematic, false, RESUME>, batch_smc_kernel<Model, kFixSystematic, true, RESUME>},
                                            {batch_smc_kernel<Model, kFixStratified, false, RESUME>, batch_smc_kernel<Model, kFixStratified, true, RESUME>}};
    static constexpr BatchKernel km[2] = {batch_smc_kernel<Model, kFixSystematic, false, RESUME, true>, batch_smc_kernel<Model, kFixStratified, false, RESUME, true>};
    return masses && !keep ? km[stratified] : k[stratified][keep];
}
template <class Model>
BatchKernel batch_kernel(bool stratified, bool keep, bool resume, bool masses)
{
    return resume ? batch_kernel<Model, true>(stratified, keep, masses) : batch_kernel<Model, false>(stratified, keep, masses);
}

}  // namespace

// ---- run lanes ---------------------------------------------------------------------------------------------------------------------
// One run is a chain of dependent launches, each short next to its own latency chain (profiles/r06_notes.md section 9): it leaves
// most of the chip idle, and only independent runs can fill it.  Runs of one begun problem that differ in their run index are
// independent; they serialised because a context has one stream and one workspace.  Here cpprob_hip_infer_run calls that follow each
// other DIRECTLY go round robin over kLaneDepth lanes (the rule depends on the call sequence alone, never on timing); a caller who
// reads every run's results before the next run never leaves lane 0.  Depth and size limit: measured, profiles/r11_notes.md.
#ifndef CPPROB_LANE_DEPTH
#define CPPROB_LANE_DEPTH 3
#endif
#ifndef CPPROB_LANE_MAX_TILES
#define CPPROB_LANE_MAX_TILES 10240
#endif
namespace {
// Depth 3: 0.074-0.078 ms per hmm<16> run of 10^6 particles against 0.083-0.089 with 2 lanes and 0.092-0.095 with 4 (a process opens 4
// hardware queues and something else of the process holds one: a fourth stream shares a queue and serialises with its neighbour).
constexpr int kLaneDepth = CPPROB_LANE_DEPTH;                            // lanes of a context, lane 0 included
// Up to 10240 tiles of 1024 particles (profiles/r11_notes.md section 3): the gain is 50 % at 977 tiles, 27 % at 3907 and 3.8 % (hmm<16>) /
// 6.7 % (linear_gaussian_1d<100>) at 9766, above the spread for every workload measured.  At 12208 tiles hmm<128> on the ESS schedule
// still gains 3.6 % but hmm<16> 0.22 % against a spread of 2.7 %: lanes there would engage where a measured gain does not exceed it.
constexpr int64_t kLaneMaxTiles = CPPROB_LANE_MAX_TILES;
constexpr uint64_t kLaneMemShare = 4;                                    // the further lanes hold at most 1 / kLaneMemShare of the memory free without them
static_assert(kLaneDepth >= 1 && kLaneDepth <= 4, "a context never owns more than 4 streams");

int lanes_wait(cpprob_hip_ctx* c)                                        // every further lane's stream has drained
{
    if (!c->lanes_busy) return 0;
    for (cpprob_hip_ctx* l : c->lanes)
        if (l) HIP_TRY(c, hipStreamSynchronize(l->stream));
    c->lanes_busy = false;
    return 0;
}
// entry points that act on the context's own state: they end a sequence of back-to-back runs and find every lane idle
inline int lanes_own(cpprob_hip_ctx* c)
{
    c->lane_chain = false;
    return c->lanes_busy ? lanes_wait(c) : 0;
}
#define LANES_OWN(c)                                                       \
    do {                                                                   \
        if (c) { if (int rc__ = lanes_own(c)) return rc__; }               \
    } while (0)

int lane_serial_reason(const cpprob_hip_ctx* c)
{
    if (c->lane_pin) return c->lane_pin;
    if (c->profile) return CPPROB_HIP_SERIAL_PROFILE;                    // (the per-class events are stream-ordered)
    if (c->exchange || c->cfg.n_global != c->cfg.n_particles) return CPPROB_HIP_SERIAL_SHARD;
    if (c->cfg.flags & CPPROB_HIP_FLAG_SERIAL_RUNS) return CPPROB_HIP_SERIAL_FLAG;
    if ((int64_t)c->nb > kLaneMaxTiles) return CPPROB_HIP_SERIAL_SIZE;
    return kLaneDepth < 2 ? CPPROB_HIP_SERIAL_FLAG : 0;
}

inline cpprob_hip_ctx* lane_of_last(cpprob_hip_ctx* c) { return c->lane_last == 0 ? c : c->lanes[(size_t)c->lane_last - 1]; }

// device bytes a begin of this configuration allocates: the arrays that grow with the population, as sized for ld particles and T steps
// (the rest is a few KB; free memory as hipMemGetInfo reports it does not move for allocations the runtime serves from a chunk it holds)
uint64_t lane_estimate_bytes(const cpprob_hip_ctx* c, uint64_t ld, uint64_t T)
{
    const uint64_t rows = c->keep ? T : 2;
    uint64_t b = ld * (4 * sizeof(double) + 2 * sizeof(uint32_t)) + rows * ld * c->ssz + (c->keep ? T * ld * sizeof(int32_t) : 0);
    if (c->cfg.algorithm == CPPROB_HIP_ALG_SMC && c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL) b += ld * (sizeof(double) + sizeof(int32_t));
    b += (uint64_t)c->nb * 512 + (uint64_t)c->walk_cap * T * 8 * sizeof(double) + ((uint64_t)1 << 20);
    return b;
}

void lane_drop(cpprob_hip_ctx* c, size_t k)
{
    if (c->lanes[k]) { c->lane_bytes -= std::min(c->lane_bytes, c->lanes[k]->lane_bytes); cpprob_hip_destroy(c->lanes[k]); }
    c->lanes[k] = nullptr; c->lane_begun[k] = 0;
}

// Lane `lane` >= 1, created and begun as the context was, the first time it is needed.  *out = nullptr without an error: its memory does
// not fit -- the lane is freed and the context pinned serial.
int lane_get(cpprob_hip_ctx* c, int lane, cpprob_hip_ctx** out)
{
    *out = nullptr;
    const size_t k = (size_t)lane - 1;
    if (c->lanes.size() <= k) { c->lanes.resize(k + 1, nullptr); c->lane_begun.resize(k + 1, 0); }
    if (c->lanes[k] && c->lane_begun[k]) { *out = c->lanes[k]; return 0; }
    size_t free0 = 0, total = 0;
    HIP_TRY(c, hipMemGetInfo(&free0, &total));
    cpprob_hip_ctx* l = c->lanes[k];
    const bool fits_old = l && l->d_values && l->cap_particles >= (size_t)c->ld && l->cap_T >= c->T && l->cap_keep == c->keep && l->cap_int == c->is_int;
    const uint64_t need = fits_old ? 0 : lane_estimate_bytes(c, (uint64_t)c->ld, (uint64_t)c->T);
    if (c->lane_bytes + need > ((uint64_t)free0 + c->lane_bytes) / kLaneMemShare) {
        lane_drop(c, k);
        c->lane_pin = CPPROB_HIP_SERIAL_MEMORY;
        return 0;
    }
    int rc = 0;
    g_last_hip_error = hipSuccess;
    if (!l) {
        rc = cpprob_hip_create(c->device, &l);
        if (rc == 0) { l->is_lane = true; c->lanes[k] = l; }
    }
    if (rc == 0 && c->lane_cfg.model == CPPROB_HIP_MODEL_HMM_TABLE) rc = cpprob_hip_set_hmm(l, c->hk, c->hk_mean.data(), c->hk_trans.data());
    if (rc == 0) rc = cpprob_hip_infer_begin(l, &c->lane_cfg, c->lane_obs.data(), c->lane_obs.size());
    if (rc == CPPROB_HIP_EDEVICE && g_last_hip_error == hipErrorOutOfMemory) {
        // (an allocation failed after all: no error, the caller's runs go on one at a time; any other device error is the caller's)
        (void)hipGetLastError();
        if (c->lanes[k]) lane_drop(c, k);
        c->lane_pin = CPPROB_HIP_SERIAL_MEMORY;
        return 0;
    }
    if (rc) return fail(c, rc, l ? l->err : g_last_error);
    // what the lane holds now (its own field; allocations only grow while a begin can reuse them)
    c->lane_bytes -= std::min(c->lane_bytes, l->lane_bytes);
    l->lane_bytes = lane_estimate_bytes(l, (uint64_t)l->cap_particles, (uint64_t)l->cap_T);
    c->lane_bytes += l->lane_bytes;
    l->force_fp = c->force_fp;
    c->lane_begun[k] = 1;
    *out = l;
    return 0;
}

void lanes_invalidate(cpprob_hip_ctx* c)                                 // a new configuration: the lanes are begun again at their next use
{
    for (char& b : c->lane_begun) b = 0;
    c->lane_last = 0; c->lane_chain = false;
}

// the reads: on the lane of the last run; its error is the context's
template <class F>
int lane_read(cpprob_hip_ctx* c, F&& f)
{
    if (!c || c->is_lane) return f(c);
    c->lane_chain = false;
    cpprob_hip_ctx* l = lane_of_last(c);
    const int rc = f(l);
    if (rc && l != c) fail(c, rc, l->err);
    if (l->force_fp) {
        // (the run was repeated in the floating-point form: as on one stream, every later run of this configuration takes that form)
        c->force_fp = true;
        for (cpprob_hip_ctx* o : c->lanes) if (o) o->force_fp = true;
    }
    return rc;
}

int infer_run_impl(cpprob_hip_ctx* c, uint64_t run_index);
}  // namespace

extern "C" {

int cpprob_hip_abi_version(void) { return CPPROB_HIP_ABI_VERSION; }

#ifndef CPPROB_BUILD_ID
#define CPPROB_BUILD_ID "unknown"
#endif
const char* cpprob_hip_build_id(void) { return CPPROB_BUILD_ID; }

int cpprob_hip_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_last_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return CPPROB_HIP_EDEVICE; }
    return n;
}

const char* cpprob_hip_last_error(const cpprob_hip_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int cpprob_hip_create(int device, cpprob_hip_ctx** out)
{
    if (!out) return fail(nullptr, CPPROB_HIP_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, CPPROB_HIP_EDEVICE, std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
                                                     "); this engine has no CPU fallback");
    if (device < 0 || device >= n) return fail(nullptr, CPPROB_HIP_EINVAL, "device index out of range");
    cpprob_hip_ctx* c = new cpprob_hip_ctx();
    c->device = device;
    const int rc = [&]() -> int {
        HIP_TRY(nullptr, hipSetDevice(device));
        HIP_TRY(nullptr, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HIP_TRY(nullptr, hipMalloc(&c->d_ctrl, sizeof(StepCtrl)));
        HIP_TRY(nullptr, hipMalloc(&c->d_local_totals, 4 * sizeof(double)));
        HIP_TRY(nullptr, hipMemsetAsync(c->d_ctrl, 0, sizeof(StepCtrl), c->stream));
        return 0;
    }();
    if (rc) { cpprob_hip_destroy(c); return rc; }     // nothing leaks on a failed create
    *out = c;
    return 0;
}

void cpprob_hip_destroy(cpprob_hip_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (cpprob_hip_ctx* l : c->lanes) cpprob_hip_destroy(l);
    c->lanes.clear(); c->lane_begun.clear();
    if (c->lane_ev) { (void)hipEventDestroy(c->lane_ev); c->lane_ev = nullptr; }
    free_run_buffers(c);
    batch_free(c);
    dfree(c->d_ctrl); dfree(c->d_local_totals); dfree(c->d_cut_tab); dfree(c->d_cut_head); dfree(c->d_cut_srccnt);
    dfree(c->d_send_src); dfree(c->d_hk_thr); dfree(c->d_hk_ll); dfree(c->d_hier_table); dfree(c->d_wpart); dfree(c->d_xplan); dfree(c->d_shard_begin); dfree(c->d_slot_of_rank); dfree(c->d_xsend); dfree(c->d_xrecv); dfree(c->d_peer_recv); dfree(c->d_peer_slot); dfree(c->d_sent); dfree(c->d_origin); dfree(c->d_remote); dfree(c->d_annex_all);
    if (c->h_obound) { (void)hipHostFree(c->h_obound); c->h_obound = nullptr; }
    if (c->h_pin) { (void)hipHostFree(c->h_pin); c->h_pin = nullptr; c->h_pin_cap = 0; }
    dfree(c->d_bb_part); dfree(c->d_bb_bc); dfree(c->d_bb_bf); dfree(c->d_bb_wrel); dfree(c->d_bb_col); dfree(c->d_bb_ctrl); dfree(c->d_bb_stats_part); dfree(c->d_bb_stats); dfree(c->d_bb_cdf); dfree(c->d_bb_cols); dfree(c->d_bb_cols_part); dfree(c->d_bb_cols_stat); dfree(c->d_bb_first); dfree(c->d_bbf_hier); dfree(c->d_bbf_table); dfree(c->d_bbf_q); dfree(c->d_bbf_strata); dfree(c->d_bbf_strata_top);
    dfree(c->d_gen_hier); dfree(c->d_gen_table); dfree(c->d_gen_q[0]); dfree(c->d_gen_q[1]); dfree(c->d_gen_ctrl);
    for (auto& ep : c->ev_used) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    for (auto& ep : c->ev_free) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void* cpprob_hip_stream(cpprob_hip_ctx* c)
{
    if (!c) return nullptr;
    // a handed-out stream promises stream order to its holder: from here on every run of this context is enqueued on it
    if (lanes_own(c)) return nullptr;                  // (a lane's work failed: cpprob_hip_last_error says how)
    if (!c->is_lane) c->lane_pin = CPPROB_HIP_SERIAL_STREAM;
    return (void*)c->stream;
}

int cpprob_hip_sync(cpprob_hip_ctx* c)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return lanes_own(c);                               // (every lane)
}

int cpprob_hip_set_hmm(cpprob_hip_ctx* c, int32_t k, const double* h_means, const double* h_transition)
{
    if (!c || !h_means || !h_transition) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (k < 2 || k > 8) return fail(c, CPPROB_HIP_EINVAL, "the table model holds 2 .. 8 states");
    for (int s2 = 0; s2 < k; ++s2) {
        double tot = 0.0;
        for (int j = 0; j < k; ++j) { const double w = h_transition[(size_t)s2 * k + j]; if (!(w >= 0.0) || !std::isfinite(w)) return fail(c, CPPROB_HIP_EINVAL, "transition weights must be finite and >= 0"); tot += w; }
        if (!(tot > 0.0)) return fail(c, CPPROB_HIP_EINVAL, "a transition row without mass");
        if (!std::isfinite(h_means[s2])) return fail(c, CPPROB_HIP_EINVAL, "state means must be finite");
    }
    c->hk = k; c->hk_mean.assign(h_means, h_means + k); c->hk_trans.assign(h_transition, h_transition + (size_t)k * k);
    c->begun = false;                                   // (a run in flight keeps the tables it was begun with; the next begin takes these)
    lanes_invalidate(c);
    return 0;
}

int cpprob_hip_infer_begin(cpprob_hip_ctx* c, const cpprob_hip_config* cfg, const double* h_obs, size_t n_obs)
{
    if (!c || !cfg || !h_obs) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    LANES_OWN(c);
    if (cfg->algorithm != CPPROB_HIP_ALG_SIS && cfg->algorithm != CPPROB_HIP_ALG_SMC)
        return fail(c, CPPROB_HIP_EUNSUPPORTED, "algorithm must be sis or smc (compile/csis/dryrun are outside this engine)");
    if (cfg->model < 0 || cfg->model > CPPROB_HIP_MODEL_HMM_TABLE) return fail(c, CPPROB_HIP_EINVAL, "unknown model id");
    if (cfg->model == CPPROB_HIP_MODEL_HMM_TABLE && c->hk < 2) return fail(c, CPPROB_HIP_ESTATE, "CPPROB_HIP_MODEL_HMM_TABLE: call cpprob_hip_set_hmm first");
    if (n_obs == 0) return fail(c, CPPROB_HIP_EINVAL, "the model has to receive the observed values (cpprob.hpp:182)");
    const bool gauss = cfg->model == CPPROB_HIP_MODEL_GAUSSIAN_UNKNOWN_MEAN || cfg->model == CPPROB_HIP_MODEL_GAUSSIAN_README;
    if (gauss && n_obs != 2) return fail(c, CPPROB_HIP_EINVAL, "gaussian_unknown_mean takes exactly two observes");
    if (cfg->model == CPPROB_HIP_MODEL_GAUSSIAN_2D_UNKNOWN_MEAN && n_obs != 2) return fail(c, CPPROB_HIP_EINVAL, "gaussian_2d_unk_mean observes one vector of two values");
    if (cfg->n_particles == 0) return fail(c, CPPROB_HIP_EINVAL, "n_particles must be > 0");
    if (cfg->n_particles > (uint64_t)INT32_MAX - kTile) return fail(c, CPPROB_HIP_EINVAL, "n_particles per context must fit int32 ancestor indices");
    if (cfg->n_particles > (uint64_t)kMaxSlabs * kSlabTiles * kTile) return fail(c, CPPROB_HIP_EINVAL, "n_particles per context exceeds the two-level normalisation's capacity");
    if (cfg->n_global < cfg->n_particles || cfg->particle_offset + cfg->n_particles > cfg->n_global)
        return fail(c, CPPROB_HIP_EINVAL, "shard [particle_offset, particle_offset + n_particles) must lie inside [0, n_global)");
    if (cfg->algorithm == CPPROB_HIP_ALG_SMC) {
        if (cfg->resampler < 0 || cfg->resampler > CPPROB_HIP_RESAMPLE_MULTINOMIAL) return fail(c, CPPROB_HIP_EINVAL, "unknown resampler");
        if (!(cfg->ess_threshold >= 0.0)) return fail(c, CPPROB_HIP_EINVAL, "ess_threshold must be >= 0");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));

    if (cfg->resample_scope != CPPROB_HIP_SCOPE_GLOBAL && cfg->resample_scope != CPPROB_HIP_SCOPE_ISLAND && cfg->resample_scope != CPPROB_HIP_SCOPE_EXCHANGE)
        return fail(c, CPPROB_HIP_EINVAL, "unknown resample_scope");
    const bool exchange = cfg->resample_scope == CPPROB_HIP_SCOPE_EXCHANGE && cfg->algorithm == CPPROB_HIP_ALG_SMC;
    if (exchange && cfg->resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL && ((cfg->flags & (CPPROB_HIP_FLAG_MULTINOMIAL_LITERAL | CPPROB_HIP_FLAG_FLOATING_POINT_STEP)) || cfg->keep_history == 0))
        return fail(c, CPPROB_HIP_EUNSUPPORTED, "multinomial resampling in the exchange scope is the strata form on integer weights with histories kept: its thresholds come stratum by "
                                                 "stratum, so a rank's sources own one interval of outputs plus its share of the strata the ranks' boundaries cut (not the literal form, "
                                                 "not the floating-point step, not keep_history = 0)");
    c->cfg = *cfg;
    // (validated: from here on the old problem is gone -- the lanes are begun again at their next use, with this configuration)
    lanes_invalidate(c);
    if (!c->is_lane) {
        const cpprob_hip_config cfg_in = *cfg;          // (cfg and h_obs may be the copies themselves)
        std::vector<double> obs_in(h_obs, h_obs + n_obs);
        c->lane_cfg = cfg_in; c->lane_obs.swap(obs_in);
    }
    // a model with ONE observe statement has nothing to resample between: smc is sis (the components of its vector-valued
    // statements are rows of the particle store, not resampling points)
    if (cfg->model == CPPROB_HIP_MODEL_GAUSSIAN_2D_UNKNOWN_MEAN) c->cfg.algorithm = CPPROB_HIP_ALG_SIS;
    const bool island = cfg->resample_scope == CPPROB_HIP_SCOPE_ISLAND;
    c->pop_n = island ? cfg->n_particles : cfg->n_global;
    c->T = model_T(cfg->model, n_obs);
    c->n_obs = (int)n_obs;
    c->begun = false; c->step_protocol = false; c->step_t = -1; c->force_fp = false; c->fixed_check_pending = false;
    // the read-out keeps kWaves * T * kStats accumulators in LDS (smooth_kernel)
    c->is_int = cfg->model == CPPROB_HIP_MODEL_HMM3 || cfg->model == CPPROB_HIP_MODEL_HMM_TABLE;
    c->K = cfg->model == CPPROB_HIP_MODEL_HMM_TABLE ? 8 : (c->is_int ? 3 : 2);
    if ((size_t)kWaves * (size_t)c->T * (size_t)std::max(c->K, 3) * sizeof(double) > 64 * 1024)
        return fail(c, CPPROB_HIP_EUNSUPPORTED, "too many predict hits per trace for the read-out kernel's LDS accumulators (T x statistics per hit <= 2048)");
    c->n = (int64_t)cfg->n_particles;
    c->nb = (int)((c->n + kTile - 1) / kTile);
    c->ld = (int64_t)c->nb * kTile;                 // padded to the tile: no ragged tails in any kernel
    c->smooth_grid = std::min(c->nb, 2048);
    c->walk_cap = std::min(c->nb, 8192);
    c->walk_grid = 0;
    host_model_params(c->mp, cfg->model);
    const bool smc = c->cfg.algorithm == CPPROB_HIP_ALG_SMC;
    const bool multinomial = smc && cfg->resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL;
    // keep_history = 0: filtering only -- two rows of values, no ancestors, predict hit t's statistics under generation t's own
    // weights.  SIS traces are their own lines (nothing to drop); a joint population's migration moves lineages (nothing to move).
    c->keep = cfg->keep_history != 0 || !smc;
    // (a shard of a joint population keeps no history in the exchange scope only: its migrants are then their current state alone)
    if (!c->keep && !exchange && cfg->resample_scope != CPPROB_HIP_SCOPE_ISLAND && cfg->n_global != cfg->n_particles)
        return fail(c, CPPROB_HIP_EUNSUPPORTED, "keep_history = 0 (filtering only) serves one population per context or a shard in the exchange scope: not a locally resampled shard");

    c->exchange = exchange;
    // exchange scope: room for immigrant lineages next to every row (grown on demand by cpprob_hip_exchange_commit)
    // default: what a well-mixed run needs -- a rank's offspring interval leaves its shard by O(sqrt(N)) outputs per resampling, so
    // ~sqrt(n_global) immigrants per step and T steps of them (measured 0.5 sqrt(N) per rank-step on BASELINE configs[3]) -- and at
    // least a sixteenth of the shard; a run that needs more reports overflow and is repeated with four times as much
    // (multinomial resampling, strata form: the two strata a rank's boundaries cut hand it up to ~a tile of immigrants a step whatever N is)
    const int64_t annex_strata = (exchange && cfg->resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL) ? (int64_t)c->T * (kTile + kTile / 2) : 0;
    const int64_t annex_mixed = (int64_t)(std::sqrt((double)cfg->n_global) * (double)c->T) / kTile * kTile + annex_strata;
    const int64_t annex_want = cfg->annex_kcols > 0 ? (int64_t)cfg->annex_kcols * 1024 : std::max<int64_t>(std::max<int64_t>(4 * kTile, c->ld / 16 / kTile * kTile), annex_mixed);
    const int64_t annex0 = exchange ? std::max<int64_t>(c->annex_cap, annex_want) : 0;
    c->ssz = 8;
    dispatch_model(c, [&](auto m) { c->ssz = sizeof(typename decltype(m)::store_t); c->grid_refs = decltype(m)::kWeightTable == 0; });
    // long traces in the exchange scope: skip rows shorten the extraction of migrating lineages (exchange.hpp)
    const bool want_skip = exchange && c->keep && !(cfg->flags & CPPROB_HIP_FLAG_NO_SKIP_ROWS) && c->T >= 3 * kSkipEvery;
    const bool realloc = (size_t)c->ld > c->cap_particles || c->T > c->cap_T || c->is_int != c->cap_int || (multinomial && !c->cap_multinomial) || !c->d_values ||
                         annex0 != c->annex_cap || c->keep != c->cap_keep || want_skip != (c->d_skip != nullptr);
    if (realloc) {
        free_run_buffers(c);
        c->annex_cap = annex0;
        const size_t ld = (size_t)c->ld, T = (size_t)c->T, rs = ld + (size_t)annex0;
        const size_t vsz = c->ssz;
        HIP_TRY(c, hipMalloc(&c->d_logw[0], ld * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_logw[1], ld * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_wrel[0], ld * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_wrel[1], ld * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_bf, (size_t)c->nb * sizeof(double)));
        const size_t rows = c->keep ? T : 2;
        HIP_TRY(c, hipMalloc(&c->d_values, rows * rs * vsz));
        HIP_TRY(c, hipMemsetAsync(c->d_values, 0, rows * rs * vsz, c->stream));
        // (ancestor and skip rows start as zeros -- a valid slot: a run that overflowed its transport still walks its lineages once,
        //  through annex columns nobody committed, before the host sees the flag and repeats it)
        if (c->keep) { HIP_TRY(c, hipMalloc(&c->d_anc, T * rs * sizeof(int32_t))); HIP_TRY(c, hipMemsetAsync(c->d_anc, 0, T * rs * sizeof(int32_t), c->stream)); }
        else { HIP_TRY(c, hipMalloc(&c->d_fpart, T * (8 + 2) * (size_t)c->smooth_grid * sizeof(double))); HIP_TRY(c, hipMalloc(&c->d_filter_w, T * sizeof(double))); }
        if (want_skip) {
            HIP_TRY(c, hipMalloc(&c->d_skip, (T / kSkipEvery + 1) * rs * sizeof(int32_t)));
            HIP_TRY(c, hipMemsetAsync(c->d_skip, 0, (T / kSkipEvery + 1) * rs * sizeof(int32_t), c->stream));
        }
        HIP_TRY(c, hipMalloc(&c->d_obound, (1024 + 2) * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_part[0], (size_t)part_stride(c->nb) * 3 * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_part[1], (size_t)part_stride(c->nb) * 3 * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_bc, ((size_t)c->nb + 1) * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_gpart, (size_t)3 * kMaxSlabs * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_stile, (size_t)kMaxReadoutCols * c->nb * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_gstat, (size_t)kMaxReadoutCols * kMaxSlabs * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_ess, T * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_lz_trace, T * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_resampled, T * sizeof(int32_t)));
        HIP_TRY(c, hipMalloc(&c->d_stats_part, (size_t)c->walk_cap * T * 8 * sizeof(double)));
        HIP_TRY(c, hipMalloc(&c->d_stats, T * 8 * sizeof(double)));
        {
            // 64-ary hierarchy of per-tile state counts, three rotating copies (step_counts.hpp); levels >= 1 one line per entry
            size_t per_copy = 0; int lev = 0;
            for (size_t e = (size_t)c->nb;; e = (e + 63) / 64, ++lev) { per_copy += e * (lev == 0 ? 1 : kHierStride); if (e <= 64) break; }
            per_copy += 2 * (size_t)c->nb;                          // fixed-point form: the tiles' Q and M arrays
            c->hier_entries = 3 * per_copy;
            HIP_TRY(c, hipMalloc(&c->d_q[0], ld * sizeof(uint32_t)));
            HIP_TRY(c, hipMalloc(&c->d_q[1], ld * sizeof(uint32_t)));
            HIP_TRY(c, hipMalloc(&c->d_hier, c->hier_entries * sizeof(uint64_t)));
            HIP_TRY(c, hipMalloc(&c->d_annex_base, (T + 1) * sizeof(int64_t)));
            HIP_TRY(c, hipMemsetAsync(c->d_annex_base, 0, (T + 1) * sizeof(int64_t), c->stream));
        }
        if (multinomial) {
            HIP_TRY(c, hipMalloc(&c->d_cdf, ld * sizeof(double)));
            HIP_TRY(c, hipMalloc(&c->d_anc_pre, ld * sizeof(int32_t)));
        }
        c->cap_particles = ld; c->cap_T = c->T; c->cap_int = c->is_int; c->cap_multinomial = multinomial; c->cap_keep = c->keep;
    }
    {
        std::memset(&c->hier, 0, sizeof c->hier);
        size_t per_copy = 0; int nl = 0;
        size_t off[kHierMaxLevels] = {0, 0, 0};
        for (size_t e = (size_t)c->nb;; e = (e + 63) / 64) {
            if (nl >= kHierMaxLevels) break;                       // (more than 64^3 tiles: the prefix-count form is not eligible)
            off[nl] = per_copy; c->hier.n_ent[nl] = (int)e; per_copy += e * (nl == 0 ? 1 : kHierStride); ++nl;
            if (e <= 64) break;
        }
        c->hier_q0_off = per_copy; c->hier_m0_off = per_copy + (size_t)c->nb; per_copy += 2 * (size_t)c->nb;
        c->hier.n_lev = nl; c->hier_per_copy = per_copy;
        {
            // the folded last step's counter sets: one per level-1 block (one at <= 64 tiles), then one per level-2 block; the top
            // arrival counter on a line of its own behind them.  Zero here; every folded run leaves them zero.
            const size_t sets = nl <= 1 ? 1 : (size_t)c->hier.n_ent[1] + (nl == 3 ? (size_t)c->hier.n_ent[2] : 0);
            const size_t words = sets * kFoldSetWords + 32;
            if (!c->d_fold || words > c->fold_cap) { dfree(c->d_fold); HIP_TRY(c, hipMalloc(&c->d_fold, words * sizeof(uint32_t))); c->fold_cap = words; }
            c->fold_sets = sets;
            HIP_TRY(c, hipMemsetAsync(c->d_fold, 0, words * sizeof(uint32_t), c->stream));
        }
        for (int k = 0; k < 3; ++k)
            for (int l = 0; l < nl; ++l) c->hier.lvl[k][l] = c->d_hier + (size_t)k * per_copy + off[l];
        if (3 * per_copy > c->hier_entries) return fail(c, CPPROB_HIP_EDEVICE, "count hierarchy exceeds its allocation");
        if (!c->d_hier_table) HIP_TRY(c, hipMalloc(&c->d_hier_table, sizeof(HierTable)));
        HIP_TRY(c, hipMemcpyAsync(c->d_hier_table, &c->hier, sizeof(HierTable), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_hier, 0, c->hier_entries * sizeof(uint64_t), c->stream));     // (the layout may have changed)
        c->hier_phase = 0; c->hier_run_open = false;
    }
    if (multinomial) {
        // the strata of every step of a run ([T - 1][2^k + 1]; a shard of a joint population holds the POPULATION's) and the level-6 totals
        const size_t words = (size_t)c->T * (((size_t)1 << strata_k_of(c)) + 1);
        if (words > c->strata_cap_words || c->T > c->strata_cap_T || !c->d_strata || !c->d_strata_top) {
            dfree(c->d_strata); dfree(c->d_strata_top);
            HIP_TRY(c, hipMalloc(&c->d_strata, words * sizeof(uint32_t)));
            HIP_TRY(c, hipMalloc(&c->d_strata_top, (size_t)2 * c->T * 64 * sizeof(uint32_t)));
            c->strata_cap_words = words; c->strata_cap_T = c->T;
        }
        if (exchange && !c->d_cut_tab) {
            HIP_TRY(c, hipMalloc(&c->d_cut_tab, (size_t)kCutSlots * kCutRow * sizeof(uint32_t)));
            HIP_TRY(c, hipMalloc(&c->d_cut_head, (size_t)kCutSlots * sizeof(CutHead)));
            HIP_TRY(c, hipMalloc(&c->d_cut_srccnt, (size_t)kCutSlots * kCutSlots * sizeof(uint32_t)));
            HIP_TRY(c, hipMemsetAsync(c->d_cut_tab, 0, (size_t)kCutSlots * kCutRow * sizeof(uint32_t), c->stream));
            HIP_TRY(c, hipMemsetAsync(c->d_cut_head, 0, (size_t)kCutSlots * sizeof(CutHead), c->stream));
            HIP_TRY(c, hipMemsetAsync(c->d_cut_srccnt, 0, (size_t)kCutSlots * kCutSlots * sizeof(uint32_t), c->stream));
        }
    }
    c->rs = c->ld + c->annex_cap;
    c->annex_used = 0; c->plan.t = -1; c->x_plan_t = -1; c->x_all_totals = nullptr;
    if (!c->d_xplan) { HIP_TRY(c, hipMalloc(&c->d_xplan, sizeof(ExchangePlan))); HIP_TRY(c, hipMemsetAsync(c->d_xplan, 0, sizeof(ExchangePlan), c->stream)); }
    dfree(c->d_obs);
    HIP_TRY(c, hipMalloc(&c->d_obs, n_obs * sizeof(double)));
    HIP_TRY(c, hipMemcpyAsync(c->d_obs, h_obs, n_obs * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_resampled, 0, (size_t)c->T * sizeof(int32_t), c->stream));
    // (the trace-word read-out's counters: allocated HERE, not by the first run that needs them -- a context made for one run paid two
    //  hipMalloc and two clears inside that run's clock: ~40 us of a 150-us run through cpprob::inference)
    if (cfg->algorithm == CPPROB_HIP_ALG_SMC && cfg->model == CPPROB_HIP_MODEL_HMM3 && c->T <= kTraceMaxT && !c->d_trace_cnt) {
        HIP_TRY(c, hipMalloc(&c->d_trace_cnt, kTraceCounterWords * sizeof(uint32_t)));
        HIP_TRY(c, hipMalloc(&c->d_trace_arrive, sizeof(unsigned long long)));
        HIP_TRY(c, hipMemsetAsync(c->d_trace_cnt, 0, kTraceCounterWords * sizeof(uint32_t), c->stream));
        HIP_TRY(c, hipMemsetAsync(c->d_trace_arrive, 0, sizeof(unsigned long long), c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(&c->d_ctrl->lz_trace, &c->d_lz_trace, sizeof(double*), hipMemcpyHostToDevice, c->stream));
    if (multinomial && c->d_strata_top) {                      // (its layout follows T; a run abandoned between its two launches leaves totals behind)
        HIP_TRY(c, hipMemsetAsync(c->d_strata_top, 0, (size_t)2 * c->T * 64 * sizeof(uint32_t), c->stream));
        c->strata_phase = 0;
    }
    {
        // Gaussian models: the log-weight as a quadratic in the prior's standard-normal variate (extended precision on the host),
        // and the grid point above its maximum
        c->sis_bounded_ok = false;
        const bool g1 = gauss, g2 = cfg->model == CPPROB_HIP_MODEL_GAUSSIAN_2D_UNKNOWN_MEAN;
        bool finite = true;
        for (size_t i = 0; i < n_obs; ++i) finite = finite && std::isfinite(h_obs[i]);
        if ((g1 || g2) && finite) {
            long double lmax = 0.0L;
            const long double sg = c->mp.sigma, ln = c->mp.log_norm_lik;
            if (g1) {
                const long double b = (long double)c->mp.sigma0 / sg, a1 = ((long double)h_obs[0] - c->mp.mu0) / sg, a2 = ((long double)h_obs[1] - c->mp.mu0) / sg;
                const long double A = -b * b, B = b * (a1 + a2), C = -0.5L * (a1 * a1 + a2 * a2) - ln;
                c->mp.quad[0][0] = (double)A; c->mp.quad[0][1] = (double)B; c->mp.quad[0][2] = (double)C;
                lmax = C - B * B / (4.0L * A);
            } else {
                for (int d = 0; d < 2; ++d) {
                    const long double b = (long double)c->mp.nd_sigma[d] / sg, a = ((long double)h_obs[d] - c->mp.nd_mean[d]) / sg;
                    const long double A = -0.5L * b * b, B = a * b, C = -0.5L * a * a - 0.5L * ln;
                    c->mp.quad[d][0] = (double)A; c->mp.quad[d][1] = (double)B; c->mp.quad[d][2] = (double)C;
                    lmax += C - B * B / (4.0L * A);
                }
            }
            c->mp.lw_ref = std::ceil((double)lmax * kInvLn2) * kLn2;
            c->sis_bounded_ok = c->T <= kMaxReadoutT;
            if (!c->d_wpart) HIP_TRY(c, hipMalloc(&c->d_wpart, (size_t)(2 + kMaxReadoutT * 2) * kSisBoundedMaxGrid * sizeof(double)));
        }
    }
    dfree(c->d_ll_tab);
    c->mp.ll_tab = nullptr; c->mp.e_tab = nullptr;
    if (cfg->model == CPPROB_HIP_MODEL_HMM3) {
        // log N(y_t; state_mean[s], 1): three values per step, computed once with the same functor
        // the reference applies per particle (utils_normal_distribution.hpp:20-45)
        // (and the linear weights of the three values against their maximum: exp(ll - max), and the max itself)
        std::vector<double> tab((size_t)c->T * 3), et((size_t)c->T * 4);
        for (int t = 0; t < c->T; ++t) hmm3_step_table(h_obs[t], c->mp.hmm_mean, &tab[(size_t)t * 3], &et[(size_t)t * 4], et[(size_t)t * 4 + 3]);
        c->h_ll_tab = tab;
        HIP_TRY(c, hipMalloc(&c->d_ll_tab, tab.size() * sizeof(double)));
        HIP_TRY(c, hipMemcpy(c->d_ll_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        c->mp.ll_tab = c->d_ll_tab;
        c->h_e_tab = et;
        dfree(c->d_e_tab);
        HIP_TRY(c, hipMalloc(&c->d_e_tab, et.size() * sizeof(double)));
        HIP_TRY(c, hipMemcpy(c->d_e_tab, et.data(), et.size() * sizeof(double), hipMemcpyHostToDevice));
        c->mp.e_tab = c->d_e_tab;
    }
    c->mp.hk = 0; c->mp.hk_thr = nullptr; c->mp.hk_ll = nullptr;
    if (cfg->model == CPPROB_HIP_MODEL_HMM_TABLE) {
        // thresholds of the rows' inverse CDFs (u >= c  <=>  word >= ceil(c 2^32), as for the three-state model) and the
        // emission log-densities of every step
        const int k = c->hk;
        const std::vector<uint64_t> thr = hmmk_thresholds(c->hk_trans, k);
        std::vector<double> ll((size_t)c->T * 8);
        for (int t = 0; t < c->T; ++t) hmmk_step_ll(h_obs[t], c->hk_mean, k, &ll[(size_t)t * 8]);
        dfree(c->d_hk_thr); dfree(c->d_hk_ll);
        HIP_TRY(c, hipMalloc(&c->d_hk_thr, thr.size() * sizeof(uint64_t)));
        HIP_TRY(c, hipMalloc(&c->d_hk_ll, ll.size() * sizeof(double)));
        HIP_TRY(c, hipMemcpy(c->d_hk_thr, thr.data(), thr.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(c->d_hk_ll, ll.data(), ll.size() * sizeof(double), hipMemcpyHostToDevice));
        c->mp.hk = k; c->mp.hk_thr = c->d_hk_thr; c->mp.hk_ll = c->d_hk_ll;
        c->h_ll_tab = ll;                                   // (host copy: the bounds below)
    }
    {
        // fixed-point form: the upper bound of each step's incremental log-weight, with the very expressions the kernels evaluate
        c->h_bound.assign((size_t)c->T, 0.0);
        for (int t = 0; t < c->T; ++t) {
            if (cfg->model == CPPROB_HIP_MODEL_HMM3) c->h_bound[(size_t)t] = c->h_e_tab[(size_t)t * 4 + 3];                       // the largest table value
            else if (cfg->model == CPPROB_HIP_MODEL_LINEAR_GAUSSIAN_1D) c->h_bound[(size_t)t] = normal_logpdf_hoisted(h_obs[t], h_obs[t], 1.0, c->mp.log_norm_unit);   // the emission's density at its mode
            else if (cfg->model == CPPROB_HIP_MODEL_HMM_TABLE) { double b = -INFINITY; for (int s2 = 0; s2 < c->hk; ++s2) b = std::max(b, c->h_ll_tab[(size_t)t * 8 + s2]); c->h_bound[(size_t)t] = b; }
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->begun = true; c->ran = false;
    return 0;
}

int cpprob_hip_infer_run(cpprob_hip_ctx* c, uint64_t run_index)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (c->is_lane) return infer_run_impl(c, run_index);
    if (!c->begun) { c->lane_chain = false; return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_infer_begin has not been called"); }
    // which lane: the one that ran last; the next one, round robin, when this call directly follows another run
    int lane = c->lane_last;
    if (lane_serial_reason(c) != 0) {
        if (int rc = lanes_wait(c)) return rc;
        lane = 0;
    } else if (c->lane_chain) lane = (c->lane_last + 1) % kLaneDepth;
    cpprob_hip_ctx* l = c;
    if (lane > 0) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (int rc = lane_get(c, lane, &l)) { c->lane_chain = false; return rc; }
        if (!l) {                                       // (it did not fit: one at a time from here on)
            if (int rc = lanes_wait(c)) return rc;
            lane = 0; l = c;
        }
    }
    const int rc = infer_run_impl(l, run_index);
    if (rc && l != c) fail(c, rc, l->err);
    c->lane_last = lane; c->lane_chain = rc == 0;
    if (lane > 0) c->lanes_busy = true;
    return rc;
}

}  // extern "C"
namespace {
int infer_run_impl(cpprob_hip_ctx* c, uint64_t run_index)
{
    if (!c->begun) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_infer_begin has not been called");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->cfg.resample_scope != CPPROB_HIP_SCOPE_ISLAND && c->cfg.n_global != c->cfg.n_particles)
        return fail(c, CPPROB_HIP_ESTATE, "this context holds one shard of a joint population: drive it with cpprob_hip_smc_step_begin/_end/_finish");
    c->run_seed = c->cfg.seed + run_index;
    c->cur = 0; c->cur_part = 0;
    c->sharded = false;
    if (!c->force_fp) c->n_requantised = 0;
    c->final_from_counts = false; c->final_from_fixed = false; c->final_folded = false;
    bool readout_done = false, sis_bounded = false;
    (void)sis_bounded;
    if (c->cfg.algorithm == CPPROB_HIP_ALG_SIS) {
        dispatch_model(c, [&](auto m) {
            using M = decltype(m);
            if (launch_sis_bounded<M>(c)) { readout_done = true; sis_bounded = true; return; }
            readout_done = sis_readout_fused<M>(c);
            launch_sis<M>(c, readout_done);
            if (readout_done) launch_sis_readout<M>(c);
        });
        if (!readout_done) launch_scan(c, c->T - 1, 0, nullptr, 1, 0);
    } else {
        c->step_protocol = false;
        c->counts_mode = false; c->fixed_mode = false;
        dispatch_model(c, [&](auto m) { c->counts_mode = counts_eligible<decltype(m)>(c); c->fixed_mode = fixed_eligible<decltype(m)>(c); });
        // a population of its own, short traces of a few states: the particles carry their traces (trace_words.hpp)
        c->trace_mode = c->counts_mode && c->keep && !c->exchange && c->T <= kTraceMaxT && c->cfg.model == CPPROB_HIP_MODEL_HMM3 &&
                        !(c->cfg.flags & CPPROB_HIP_FLAG_WALK_READOUT);
        if (c->trace_mode && !c->d_trace_cnt) {
            HIP_TRY(c, hipMalloc(&c->d_trace_cnt, kTraceCounterWords * sizeof(uint32_t)));
            HIP_TRY(c, hipMalloc(&c->d_trace_arrive, sizeof(unsigned long long)));
            HIP_TRY(c, hipMemsetAsync(c->d_trace_cnt, 0, kTraceCounterWords * sizeof(uint32_t), c->stream));
            HIP_TRY(c, hipMemsetAsync(c->d_trace_arrive, 0, sizeof(unsigned long long), c->stream));
        }
        const bool fused = step_is_fused(c);
        if (c->fixed_mode) {
            c->strata_pending = c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL && !(c->cfg.flags & CPPROB_HIP_FLAG_MULTINOMIAL_LITERAL);
            launch_strata(c);
            ProfScope group(c, 0, c->T);
            c->profile_suspended = true;
            for (int t = 0; t < c->T; ++t) dispatch_model(c, [&](auto m) { launch_step_fixed<decltype(m)>(c, t, nullptr, 1, 0); });
            c->profile_suspended = false;
            // (no normalisation launch at any size: the read-out works from the final generation's masses)
        } else if (c->counts_mode) {
            c->strata_pending = c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL;
            launch_strata(c);
            {
                ProfScope group(c, 0, c->T);
                c->profile_suspended = true;
                for (int t = 0; t < c->T; ++t) dispatch_model(c, [&](auto m) { launch_step_counts<decltype(m)>(c, t, nullptr, 1, 0); });
                c->profile_suspended = false;
            }
            // (no normalisation launch: the read-out works from the final generation's counts)
        } else if (fused) {
            // the T step kernels run back to back: one event pair around the group
            {
                ProfScope group(c, 0, c->T);
                c->profile_suspended = true;
                for (int t = 0; t < c->T; ++t) dispatch_model(c, [&](auto m) { launch_step<decltype(m)>(c, t); });
                c->profile_suspended = false;
            }
            launch_scan(c, c->T - 1, 0, nullptr, 1, 0);                          // only the final generation needs the standalone pass
        } else {
            for (int t = 0; t < c->T; ++t) {
                dispatch_model(c, [&](auto m) { launch_step<decltype(m)>(c, t); });
                launch_scan(c, t, 0, nullptr, 1, 0);
            }
        }
    }
    if (!c->keep) {
        // filtering only: every step left its own statistics (count form: from the generation's totals; floating-point form:
        // filter_partials_kernel); what remains is the final generation's bookkeeping and the normalisation
        if (c->final_from_counts) {
            CountsFinal f{};
            counts_final_view(c, f, true);
            c->final_bookkeep_pending = false;
            hipLaunchKernelGGL(counts_filter_final_kernel, dim3(1), dim3(kWave), 0, c->stream, f);
        } else {
            if (c->final_from_fixed) {
                FixedFinal ff{};
                fixed_final_view(c, ff, true);
                c->final_bookkeep_pending = false;
                hipLaunchKernelGGL(fixed_filter_final_kernel, dim3(1), dim3(kWave), 0, c->stream, ff);
            }
            hipLaunchKernelGGL(filter_finalize_kernel, dim3(c->T), dim3(kThreads), 0, c->stream, (const double*)c->d_fpart, c->smooth_grid, c->K, c->is_int ? 1 : 0, c->d_stats, 1, (double*)nullptr);
        }
    } else if (!readout_done && !c->final_folded) dispatch_model(c, [&](auto m) { launch_smooth<decltype(m)>(c, false); });
    HIP_TRY(c, hipGetLastError());
    c->ran = true;
    c->fixed_check_pending = c->fixed_mode && c->cfg.algorithm == CPPROB_HIP_ALG_SMC; c->last_was_infer_run = true; c->last_run_index = run_index;
    return 0;
}
}  // namespace
extern "C" {

int cpprob_hip_infer_lanes(cpprob_hip_ctx* c, int32_t* depth, int32_t* last_lane, uint64_t* lane_bytes, int32_t* serial_reason)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    int d = 1;
    for (size_t k = 0; k < c->lanes.size(); ++k) d += (c->lanes[k] && c->lane_begun[k]) ? 1 : 0;
    if (depth) *depth = d;
    if (last_lane) *last_lane = c->lane_last;
    if (lane_bytes) *lane_bytes = c->lane_bytes;
    if (serial_reason) *serial_reason = c->begun ? lane_serial_reason(c) : c->lane_pin;
    return 0;
}

}  // extern "C"
namespace {
// A generation whose heaviest particle sat more than kFixGapLimit nats below its reference kept too few of its 32 bits (an observation
// far from EVERY particle).  Repair, in integers: the offending generation g is weighed again against its EXACT maximum -- its
// log-weights recomputed from the particle store (fixed_relogw_kernel), maximum and masses by the two order-free passes of
// bookkeep_fixed.hpp -- the books are rewound to where they stood before g (StepCtrl::lz_trace), and the steps behind g run again;
// repeated while a later generation trips (each round starts later).  The CPU restatement states the same rule (orc_smc_impl), so a
// repaired run still equals it index for index, and no floating-point CDF enters.
template <class Model>
int repair_fixed_generation(cpprob_hip_ctx* c, int g)
{
    if constexpr (std::is_same<Model, ModelLinearGaussian1D>::value || std::is_same<Model, ModelHmm3>::value || std::is_same<Model, ModelHmmK>::value) {
        std::vector<int32_t> res((size_t)c->T);
        HIP_TRY(c, hipMemcpyAsync(res.data(), c->d_resampled, res.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        int s0 = 0;
        for (int s2 = g - 1; s2 >= 0; --s2) if (res[(size_t)s2]) { s0 = s2 + 1; break; }
        c->cur = (g + 1) & 1;                                        // (where step g left its weights: the buffers alternate step by step)
        double* lw = c->d_logw[c->cur];
        uint32_t* q = c->d_q[c->cur];
        hipLaunchKernelGGL(fixed_relogw_kernel<Model>, dim3((unsigned)((c->ld + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, c->mp, (const double*)c->d_obs,
                           static_cast<const typename Model::store_t*>(c->d_values), c->rs, s0, g, c->n, c->ld, lw);
        // the hierarchy: every copy clean, generation g's masses in the copy step g + 1 reads
        HIP_TRY(c, hipMemsetAsync(c->d_hier, 0, c->hier_entries * sizeof(uint64_t), c->stream));
        const int ka = (g + 1 + c->hier_phase_run) % 3, kb = (ka + 1) % 3;
        FHier f{};
        fhier_view(c, ka, f);
        f.h.to_next = 0; f.h.to_clear = (int64_t)(kb - ka) * (int64_t)c->hier_per_copy;
        hipLaunchKernelGGL(bbf_max_kernel, dim3(c->nb), dim3(kThreads), 0, c->stream, (const double*)lw, c->n, f);
        hipLaunchKernelGGL(bbf_quantize_kernel, dim3(c->nb), dim3(kThreads), 0, c->stream, (const double*)lw, c->n, f, q);
        hipLaunchKernelGGL(fixed_repair_ctrl_kernel, dim3(1), dim3(kWave), 0, c->stream, c->d_ctrl, f, g, (const int32_t*)c->d_resampled);
        for (int t = g + 1; t < c->T; ++t) launch_step_fixed<Model>(c, t, nullptr, 1, 0);
        if (g + 1 == c->T) { c->final_from_fixed = true; c->final_copy = ka; c->final_bookkeep_pending = true; }
        launch_smooth<Model>(c, false);
        HIP_TRY(c, hipGetLastError());
        return 0;
    }
    return fail(c, CPPROB_HIP_ESTATE, "the fixed-point form serves the state-space models");
}

// Before a run's results leave the library: did the fixed-point weights keep their bits?  If not the offending generations are
// repaired as above; where that is not possible (a shard of a joint population, a filtering-only run, a generation without mass) the
// run is repeated in the floating-point form (runs the caller drives step by step cannot be repeated here: CPPROB_HIP_EPRECISION).
// Small results reach the host WITHOUT copy commands and without waiting for the stream: one short launch stores them into pinned
// (device-visible, coherent) host memory, then a sequence number behind them; the host polls that word.  (Measured on the way here,
// per read-back of a few hundred bytes: a copy into pageable memory ~35 us of host round trip, an asynchronous copy into pinned memory
// ~20 us each -- three of them closed every run -- and hipStreamSynchronize's own wake-up behind the last kernel.)
constexpr size_t kPinHeader = 64;                                       // the block's first bytes: the sequence word
struct PinSeg { const uint32_t* src; uint32_t* dst; uint32_t words; uint32_t pad; };
struct PinSegs { PinSeg s[4]; int n; };
__global__ __launch_bounds__(kThreads) void pin_pack_kernel(PinSegs a, unsigned long long* flag, unsigned long long seq)
{
    for (int k = 0; k < a.n; ++k)
        for (uint32_t i = threadIdx.x; i < a.s[k].words; i += kThreads) a.s[k].dst[i] = a.s[k].src[i];
    __threadfence_system();                                             // (every thread's stores are on their way before the flag is)
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
static int pin_reserve(cpprob_hip_ctx* c, size_t bytes)                 // bytes of data (behind the header)
{
    bytes += kPinHeader;
    if (bytes <= c->h_pin_cap) return 0;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->h_pin) { (void)hipHostFree(c->h_pin); c->h_pin = nullptr; c->h_pin_cap = 0; }
    const size_t want = std::max<size_t>(bytes + bytes / 2, (size_t)1 << 16);
    // (coherent, i.e. fine-grained: the host sees the sequence word while the stream is still busy; a runtime that refuses the flag
    //  combination still gets a correct block -- pin_wait falls back to the stream's completion)
    if (hipHostMalloc(reinterpret_cast<void**>(&c->h_pin), want, hipHostMallocCoherent | hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
        c->h_pin = nullptr;
        HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_pin), want, hipHostMallocPortable | hipHostMallocMapped));
    }
    std::memset(c->h_pin, 0, kPinHeader);
    c->h_pin_cap = want; c->pin_seq = 0;
    return 0;
}
static char* pin_data(cpprob_hip_ctx* c) { return c->h_pin + kPinHeader; }
struct PinPack {
    PinSegs segs{};
    void add(const void* d_src, void* h_dst, size_t bytes)             // (device memory -> the context's pinned block; 4-byte words)
    {
        if (bytes == 0) return;
        PinSeg& g = segs.s[segs.n++];
        g.src = static_cast<const uint32_t*>(d_src); g.dst = static_cast<uint32_t*>(h_dst); g.words = (uint32_t)((bytes + 3) / 4); g.pad = 0;
    }
    // the launch; `wait` is what the host calls when it wants the bytes
    int launch(cpprob_hip_ctx* c)
    {
        c->pin_seq += 1;
        hipLaunchKernelGGL(pin_pack_kernel, dim3(1), dim3(kThreads), 0, c->stream, segs, reinterpret_cast<unsigned long long*>(c->h_pin), (unsigned long long)c->pin_seq);
        HIP_TRY(c, hipGetLastError());
        return 0;
    }
};
// the host's side: poll the sequence word (the launch is short and last in the stream); a look at the stream every few thousand polls
// catches a failed launch, and a stream that finished without the word showing falls back to its synchronisation
static int pin_wait(cpprob_hip_ctx* c)
{
    volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(c->h_pin);
    const unsigned long long want = (unsigned long long)c->pin_seq;
    for (unsigned k = 1;; ++k) {
        if (*flag == want) break;
        if ((k & 0x3fffu) == 0) {
            const hipError_t q = hipStreamQuery(c->stream);
            if (q == hipSuccess) { if (*flag != want) HIP_TRY(c, hipStreamSynchronize(c->stream)); break; }
            if (q != hipErrorNotReady) { HIP_TRY(c, q); }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return 0;
}

int settle_fixed(cpprob_hip_ctx* c)
{
    if (!c->fixed_check_pending) return 0;
    c->fixed_check_pending = false;
    StepCtrl h{};
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(&h, c->d_ctrl, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h.fix_gap <= kFixGapLimit) return 0;
    // (the literal multinomial form keeps lane prefixes beside the weights that a requantised generation would leave stale: it repeats the run)
    const bool literal = c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL && (c->cfg.flags & CPPROB_HIP_FLAG_MULTINOMIAL_LITERAL);
    if (c->last_was_infer_run && c->keep && !c->exchange && c->d_lz_trace && !literal && !(c->cfg.flags & CPPROB_HIP_FLAG_REPEAT_IN_FLOATING_POINT)) {
        int g_prev = -1;
        for (int round = 0; round <= c->T; ++round) {
            const int g = h.first_bad;
            if (g < 0 || g >= c->T || g <= g_prev) break;                // (no progress: a generation without any mass)
            int rc = 0;
            dispatch_model(c, [&](auto m) { rc = repair_fixed_generation<decltype(m)>(c, g); });
            if (rc) return rc;
            c->n_requantised += 1;
            g_prev = g;
            HIP_TRY(c, hipMemcpyAsync(&h, c->d_ctrl, sizeof h, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (h.fix_gap <= kFixGapLimit) return 0;
        }
    }
    if (!c->last_was_infer_run)
        return fail(c, CPPROB_HIP_EPRECISION, "some generation's heaviest particle sat more than 6 nats below the fixed-point reference (an observation far from every particle): "
                                               "repair it in the run (cpprob_hip_smc_repair_begin / _end on every rank, from the first offending generation: StepCtrl::first_bad "
                                               "through cpprob_hip_smc_first_bad_generation) or repeat the run with CPPROB_HIP_FLAG_FLOATING_POINT_STEP");
    c->force_fp = true;
    return infer_run_impl(c, c->last_run_index);
}
}  // namespace
extern "C" {

static int ensure_shard_trace(cpprob_hip_ctx* c, bool& words);

int cpprob_hip_smc_step_begin(cpprob_hip_ctx* c, int32_t t, uint64_t run_index, double* d_local_totals)
{
    LANES_OWN(c);
    if (!c || !d_local_totals) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->begun) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_infer_begin has not been called");
    if (t < 0 || t >= c->T) return fail(c, CPPROB_HIP_EINVAL, "step out of range");
    c->lane_last = 0;                                   // (the step protocol runs on the context itself: its results are read there)
    HIP_TRY(c, hipSetDevice(c->device));
    const bool sis = c->cfg.algorithm == CPPROB_HIP_ALG_SIS;
    if (sis && t != c->T - 1) return fail(c, CPPROB_HIP_EINVAL, "SIS shards run in one launch: call step_begin(T-1) only");
    if (t == 0 || sis) {
        c->strata_pending = !sis && c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL && !(c->cfg.flags & CPPROB_HIP_FLAG_MULTINOMIAL_LITERAL);
        c->run_seed = c->cfg.seed + run_index; c->cur = 0; c->cur_part = 0; c->ran = false; c->annex_used = 0; c->plan.t = -1; c->x_plan_t = -1;
        c->n_requantised = 0; c->annex_used_before.clear();
        c->final_from_counts = false; c->final_from_fixed = false; c->final_folded = false;
        c->counts_mode = false; c->fixed_mode = false;
        // the integer forms serve exact joint resampling (exchange scope) and a population held by this context alone; a shard that
        // resamples locally (global scope, several ranks) keeps the floating-point form and its mass-share bookkeeping
        if (!sis && (c->exchange || c->cfg.n_global == c->cfg.n_particles))
            dispatch_model(c, [&](auto m) { c->counts_mode = counts_eligible<decltype(m)>(c); c->fixed_mode = fixed_eligible<decltype(m)>(c); });
    }
    if ((t == 0 || sis) && c->exchange && !sis && c->cfg.resampler != CPPROB_HIP_RESAMPLE_SYSTEMATIC && !c->counts_mode && !c->fixed_mode)
        return fail(c, CPPROB_HIP_EUNSUPPORTED, "stratified / multinomial resampling in the exchange scope run on the integer forms of the step (the floating-point form plans the ranks' "
                                                 "offspring intervals from the ONE systematic offset): not with CPPROB_HIP_FLAG_FLOATING_POINT_STEP, beyond 2^28 particles, or for models "
                                                 "without a fixed-point form");
    if (c->exchange && t > 0 && c->x_plan_t != t - 1)
        return fail(c, CPPROB_HIP_ESTATE, "exchange scope: the exchange of the previous step (plan / pack / commit) must run before the next step_begin");
    c->step_protocol = true; c->step_t = t; c->trace_mode = false;
    if (t == 0 || sis) {
        c->trace_shard_run = c->trace_shard && c->x_remote && c->counts_mode && c->keep && !c->x_peers.empty();
        if (c->exchange && c->x_fixed && c->x_peers.empty() && c->counts_mode && c->keep) {
            // (a shard with nobody to exchange with -- a group of one -- needs nobody's consent)
            bool words = false;
            if (int rc = ensure_shard_trace(c, words)) return rc;
            c->trace_shard_run = words;
        }
    }
    c->totals_out = d_local_totals;
    c->x_gather_done = c->x_gather_on && (c->counts_mode || c->fixed_mode);
    if (c->counts_mode) {
        // prefix-count form: the step consumes the all-gathered counts of generation t-1 itself; what leaves is this shard's
        // {n_0, n_1, particles} (exact doubles), after the last step too: the read-out works from the final generation's counts
        if (t > 0 && !c->x_all_totals) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_smc_step_end(t-1) has not run");
        dispatch_model(c, [&](auto m) { launch_step_counts<decltype(m)>(c, t, t > 0 ? c->x_all_totals : nullptr, c->x_world, c->x_rank); });
        {
            Hier h{};
            const int kn = (t + 1 + c->hier_phase_run) % 3;
            hier_view(c, kn, h);
            if (c->x_gather_on) { TotalsGather d = c->x_gather; d.parity = (t - c->x_gather_tshift) & 1; d.seq = (c->x_gather_serial << 32) | (unsigned long long)(uint32_t)(t - c->x_gather_tshift + 1);
                                  hipLaunchKernelGGL(counts_totals_gather_kernel, dim3(1), dim3(kWave), 0, c->stream, h, (double)c->n, d_local_totals, d); }
            else hipLaunchKernelGGL(counts_totals_kernel, dim3(1), dim3(kWave), 0, c->stream, h, (double)c->n, d_local_totals);
        }
    } else if (c->fixed_mode) {
        // fixed-point form: likewise; what leaves is this shard's {mass, squares, key of the largest log-weight}: 24 bytes
        if (t > 0 && !c->x_all_totals) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_smc_step_end(t-1) has not run");
        dispatch_model(c, [&](auto m) { launch_step_fixed<decltype(m)>(c, t, t > 0 ? c->x_all_totals : nullptr, c->x_world, c->x_rank); });
        {
            FHier f{};
            const int kn = (t + 1 + c->hier_phase_run) % 3;
            fhier_view(c, kn, f);
            if (c->x_gather_on) { TotalsGather d = c->x_gather; d.parity = (t - c->x_gather_tshift) & 1; d.seq = (c->x_gather_serial << 32) | (unsigned long long)(uint32_t)(t - c->x_gather_tshift + 1);
                                  hipLaunchKernelGGL(fixed_totals_gather_kernel, dim3(1), dim3(kWave), 0, c->stream, f, reinterpret_cast<uint64_t*>(d_local_totals), d); }
            else hipLaunchKernelGGL(fixed_totals_kernel, dim3(1), dim3(kWave), 0, c->stream, f, reinterpret_cast<uint64_t*>(d_local_totals));
        }
    } else {
        if (sis) dispatch_model(c, [&](auto m) { launch_sis<decltype(m)>(c, false); });
        else dispatch_model(c, [&](auto m) { launch_step<decltype(m)>(c, t); });
        launch_scan(c, t, 1, nullptr, 1, 0);
    }
    if (c->d_skip && !c->x_remote && t >= kSkipEvery && (t % kSkipEvery) == 0 && !sis) {
        // every eighth step: where each local slot's lineage sat eight generations ago
        hipLaunchKernelGGL(skip_rows_kernel, dim3((unsigned)((c->n + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, (const int32_t*)c->d_anc, c->rs, c->n,
                           (const int32_t*)c->d_resampled, t, c->d_skip + (size_t)(t / kSkipEvery) * c->rs);
    }
    HIP_TRY(c, hipGetLastError());
    c->sharded = true;
    return 0;
}

int cpprob_hip_smc_step_end(cpprob_hip_ctx* c, int32_t t, const double* d_all_totals, int32_t world, int32_t rank)
{
    LANES_OWN(c);
    if (!c || !d_all_totals) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->begun || !c->step_protocol || t != c->step_t) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_smc_step_end(t) follows cpprob_hip_smc_step_begin(t)");
    if (world < 1 || world > 1024 || rank < 0 || rank >= world) return fail(c, CPPROB_HIP_EINVAL, "bad world/rank (1 <= world <= 1024)");
    if (c->exchange && world > kMaxWorld) return fail(c, CPPROB_HIP_EUNSUPPORTED, "the exchange scope plans on one wavefront (world + 1 bounds, one per lane): world <= 63");
    HIP_TRY(c, hipSetDevice(c->device));
    c->x_all_totals = d_all_totals; c->x_world = world; c->x_rank = rank;
    if (c->fixed_mode) {
        if (t + 1 == c->T) {
            if (world > kWave) return fail(c, CPPROB_HIP_EUNSUPPORTED, "the fixed-point form sums the ranks' totals on one wavefront: world <= 64");
            FixedFinal ff{};
            fixed_final_view(c, ff, true);
            hipLaunchKernelGGL(fixed_final_ctrl_kernel, dim3(1), dim3(kWave), 0, c->stream, ff, reinterpret_cast<const uint64_t*>(d_all_totals), world);
            c->final_bookkeep_pending = false;
        }
    } else if (!c->counts_mode) {
        // floating-point form: the ranks' {max, sum, sum of squares} into ctrl.  In the exchange scope the step's plan launch follows
        // and does this on its way in (one launch less per step); the last step has no exchange
        c->scan2_deferred = c->exchange && t + 1 < c->T;
        if (!c->scan2_deferred) launch_scan(c, t, 2, d_all_totals, world, rank);
    }
    else if (t + 1 == c->T) {
        // the final generation's bookkeeping from the population's totals (the same sums a single GPU's hierarchy would hold)
        if (world > kWave) return fail(c, CPPROB_HIP_EUNSUPPORTED, "the prefix-count form sums the ranks' totals on one wavefront: world <= 64");
        CountsFinal f{};
        counts_final_view(c, f, true);
        hipLaunchKernelGGL(counts_final_ctrl_kernel, dim3(1), dim3(kWave), 0, c->stream, f, d_all_totals, world);
        c->final_bookkeep_pending = false;
    }
    HIP_TRY(c, hipGetLastError());
    return 0;
}

// ---- a shard's generation that lost its bits: repaired in the run, as a single context's is (settle_fixed) ----------------------
// Every rank finds the same first offending generation g in its books (they come from the all-gathered totals).  The repair is the
// single context's, with the POPULATION's exact maximum in place of the shard's:
//   repair_begin(g)   generation g's log-weights again from the particle store, this shard's exact maximum -> d_local3 = {key(M), 0, 0}
//   (the caller all-gathers the 24 bytes, as it does a step's totals)
//   repair_end(g)     masses against the largest of the ranks' maxima, the books rewound to where they stood before g,
//                     this shard's {S, Q, key(M)} of the requantised generation -> d_local3
//   (all-gather; cpprob_hip_smc_step_end(g); the exchange behind step g; the steps g + 1 .. T - 1 as ever; cpprob_hip_smc_finish)
}  // extern "C"
template <class Model>
static int shard_repair_begin(cpprob_hip_ctx* c, int g, double* d_local3)
{
    if constexpr (std::is_same<Model, ModelLinearGaussian1D>::value || std::is_same<Model, ModelHmm3>::value || std::is_same<Model, ModelHmmK>::value) {
        std::vector<int32_t> res((size_t)c->T);
        HIP_TRY(c, hipMemcpyAsync(res.data(), c->d_resampled, res.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        int s0 = 0;
        for (int s2 = g - 1; s2 >= 0; --s2) if (res[(size_t)s2]) { s0 = s2 + 1; break; }
        c->cur = (g + 1) & 1;
        hipLaunchKernelGGL(fixed_relogw_kernel<Model>, dim3((unsigned)((c->ld + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, c->mp, (const double*)c->d_obs,
                           static_cast<const typename Model::store_t*>(c->d_values), c->rs, s0, g, c->n, c->ld, c->d_logw[c->cur]);
        HIP_TRY(c, hipMemsetAsync(c->d_hier, 0, c->hier_entries * sizeof(uint64_t), c->stream));
        const int ka = (g + 1 + c->hier_phase_run) % 3, kb = (ka + 1) % 3;
        FHier f{};
        fhier_view(c, ka, f);
        f.h.to_next = 0; f.h.to_clear = (int64_t)(kb - ka) * (int64_t)c->hier_per_copy;
        hipLaunchKernelGGL(bbf_max_kernel, dim3(c->nb), dim3(kThreads), 0, c->stream, (const double*)c->d_logw[c->cur], c->n, f);
        hipLaunchKernelGGL(fixed_repair_max_kernel, dim3(1), dim3(kWave), 0, c->stream, f, reinterpret_cast<uint64_t*>(d_local3));
        HIP_TRY(c, hipGetLastError());
        return 0;
    }
    return fail(c, CPPROB_HIP_ESTATE, "the fixed-point form serves the state-space models");
}

extern "C" {

static int smc_first_bad_generation_impl(cpprob_hip_ctx* c, int32_t* h_generation, double* h_gap);
int cpprob_hip_smc_first_bad_generation(cpprob_hip_ctx* c, int32_t* h_generation, double* h_gap)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return smc_first_bad_generation_impl(l, h_generation, h_gap); });
}
static int smc_first_bad_generation_impl(cpprob_hip_ctx* c, int32_t* h_generation, double* h_gap)
{
    if (!c || !h_generation) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->begun) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_infer_begin has not been called");
    HIP_TRY(c, hipSetDevice(c->device));
    StepCtrl h{};
    HIP_TRY(c, hipMemcpyAsync(&h, c->d_ctrl, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *h_generation = (c->fixed_mode && !(h.fix_gap <= kFixGapLimit)) ? h.first_bad : -1;
    if (h_gap) *h_gap = c->fixed_mode ? h.fix_gap : 0.0;
    return 0;
}

int cpprob_hip_smc_repair_begin(cpprob_hip_ctx* c, int32_t g, double* d_local3)
{
    LANES_OWN(c);
    if (!c || !d_local3) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->begun || !c->step_protocol || !c->fixed_mode || !c->keep || !c->d_lz_trace) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_smc_repair_begin: a history-keeping step-protocol run on fixed-point weights");
    if (g < 0 || g >= c->T) return fail(c, CPPROB_HIP_EINVAL, "generation out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = 0;
    dispatch_model(c, [&](auto m) { rc = shard_repair_begin<decltype(m)>(c, g, d_local3); });
    return rc;
}

int cpprob_hip_smc_repair_end(cpprob_hip_ctx* c, int32_t g, const double* d_all3, int32_t world, int32_t rank, double* d_local3)
{
    LANES_OWN(c);
    if (!c || !d_all3 || !d_local3) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->begun || !c->step_protocol || !c->fixed_mode) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_smc_repair_end follows cpprob_hip_smc_repair_begin");
    if (g < 0 || g >= c->T || world < 1 || world > kWave || rank < 0 || rank >= world) return fail(c, CPPROB_HIP_EINVAL, "bad generation / world / rank");
    HIP_TRY(c, hipSetDevice(c->device));
    const int ka = (g + 1 + c->hier_phase_run) % 3, kb = (ka + 1) % 3;
    FHier f{};
    fhier_view(c, ka, f);
    f.h.to_next = 0; f.h.to_clear = (int64_t)(kb - ka) * (int64_t)c->hier_per_copy;
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(d_all3);
    hipLaunchKernelGGL(bbf_quantize_kernel, dim3(c->nb), dim3(kThreads), 0, c->stream, (const double*)c->d_logw[c->cur], c->n, f, c->d_q[c->cur], keys, (int)world);
    hipLaunchKernelGGL(fixed_repair_ctrl_kernel, dim3(1), dim3(kWave), 0, c->stream, c->d_ctrl, f, (int)g, (const int32_t*)c->d_resampled, keys, (int)world);
    hipLaunchKernelGGL(fixed_totals_kernel, dim3(1), dim3(kWave), 0, c->stream, f, reinterpret_cast<uint64_t*>(d_local3));
    HIP_TRY(c, hipGetLastError());
    // the protocol goes on as if step g had just run: its step_end, its exchange, then step g + 1
    c->step_t = g; c->x_plan_t = g - 1; c->plan.t = -1; c->x_all_totals = nullptr; c->ran = false;
    // (a caller of the synchronising exchange calls: the annex as it stood before the exchange that followed step g; a step whose
    //  exchange planned nothing left no mark -- the next marked one stands for it, the columns in use do not shrink)
    for (size_t k = (size_t)g; k < c->annex_used_before.size(); ++k) {
        if (c->annex_used_before[k] >= 0) { c->annex_used = c->annex_used_before[k]; break; }
    }
    for (size_t k = (size_t)g; k < c->annex_used_before.size(); ++k) c->annex_used_before[k] = -1;
    if (g + 1 == c->T) { c->final_from_fixed = true; c->final_copy = ka; c->final_bookkeep_pending = true; }
    c->n_requantised += 1;
    c->fixed_check_pending = false;
    return 0;
}

int cpprob_hip_smc_finish(cpprob_hip_ctx* c)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!c->begun || !c->step_protocol || c->step_t != c->T - 1) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_smc_finish follows the last step's cpprob_hip_smc_step_end");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->keep) {
        // filtering-only shard: every step left its statistics -- the count form the JOINT population's probabilities (from the
        // all-gathered totals: nothing to combine), the fixed-point form this shard's raw sums and masses (the caller adds them
        // over ranks and divides: cpprob_hip_filter_masses)
        if (c->fixed_mode) hipLaunchKernelGGL(filter_finalize_kernel, dim3(c->T), dim3(kThreads), 0, c->stream, (const double*)c->d_fpart, c->smooth_grid, c->K, c->is_int ? 1 : 0, c->d_stats, 0, c->d_filter_w);
    } else dispatch_model(c, [&](auto m) { launch_smooth<decltype(m)>(c, false); });
    HIP_TRY(c, hipGetLastError());
    c->ran = true;
    c->fixed_check_pending = c->fixed_mode; c->last_was_infer_run = false;
    return 0;
}

static int filter_masses_impl(cpprob_hip_ctx* c, double** d_masses, int32_t* joint_already);
int cpprob_hip_filter_masses(cpprob_hip_ctx* c, double** d_masses, int32_t* joint_already)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return filter_masses_impl(l, d_masses, joint_already); });
}
static int filter_masses_impl(cpprob_hip_ctx* c, double** d_masses, int32_t* joint_already)
{
    if (!c || !d_masses || !joint_already) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->begun || c->keep) return fail(c, CPPROB_HIP_ESTATE, "not a filtering-only run (keep_history = 0)");
    *d_masses = c->d_filter_w; *joint_already = c->counts_mode ? 1 : 0;
    return 0;
}

// ---- exchange scope -----------------------------------------------------------------------------
#define GRID1(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, c->stream

}  // extern "C"

namespace {

int upload_geometry(cpprob_hip_ctx* c, int world, int rank, const uint64_t* h_shard_begin)
{
    if (world < 1 || world > kMaxWorld || rank < 0 || rank >= world) return fail(c, CPPROB_HIP_EINVAL, "bad world/rank (1 <= world <= 63)");
    if (h_shard_begin[rank] != c->cfg.particle_offset || h_shard_begin[rank + 1] - h_shard_begin[rank] != (uint64_t)c->n || h_shard_begin[world] != c->cfg.n_global)
        return fail(c, CPPROB_HIP_EINVAL, "h_shard_begin does not describe this context's shard");
    std::vector<uint64_t> sb(h_shard_begin, h_shard_begin + world + 1);
    if (sb == c->x_shard_begin && c->d_shard_begin) return 0;
    if (!c->d_shard_begin) HIP_TRY(c, hipMalloc(&c->d_shard_begin, (kWorldSlots + 1) * sizeof(int64_t)));
    std::vector<int64_t> h(sb.begin(), sb.end());
    HIP_TRY(c, hipMemcpyAsync(c->d_shard_begin, h.data(), h.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));           // (h is a local)
    c->x_shard_begin = sb;
    return 0;
}

// the plan of the exchange that follows step t, on the device (no host synchronisation)
int launch_plan(cpprob_hip_ctx* c, int t, bool fixed_layout)
{
    ExchangeGeom g{};
    g.world = c->x_world; g.rank = c->x_rank; g.n = c->n; g.shard_begin = c->d_shard_begin;
    g.slot_of_rank = fixed_layout ? c->d_slot_of_rank : nullptr; g.cap = fixed_layout ? c->x_cap : (int64_t)1 << 40;
    g.annex_cap = fixed_layout ? c->annex_cap : (int64_t)1 << 40;      // (callers that synchronise grow the annex themselves)
    g.bytes_per_value = (int)(fixed_layout ? c->ssz : (c->is_int ? sizeof(int32_t) : sizeof(double))); g.sent_per_step = c->d_sent;
    g.no_history = c->keep ? 0 : 1; g.remote = (c->x_remote && c->keep && fixed_layout) ? 1 : 0;
    if (g.remote) { g.rem = c->d_remote; g.annex_all = c->d_annex_all; g.slot_of_rank = nullptr; g.cap = (int64_t)1 << 40; g.trace_words = c->trace_shard_run ? 1 : 0; }
    PlanCountsIn pc{};
    pc.all_totals = c->x_all_totals; pc.n_pop = (double)c->pop_n;
    if (c->fixed_mode) {
        PlanFixedIn pf{};
        pf.all_totals = reinterpret_cast<const uint64_t*>(c->x_all_totals); pf.u0 = host_resample_u0(c->run_seed, (uint64_t)t + 1); pf.n_pop = (double)c->pop_n;
        pf.ess_frac = c->cfg.ess_threshold;
        pf.rs = c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED ? kFixStratified : kFixSystematic; pf.seed = c->run_seed; pf.draw = kResampleDrawBase + (uint64_t)t + 1;
        hipLaunchKernelGGL(exchange_plan_fixed_kernel, dim3(1), dim3(kWave), 0, c->stream, g, pf, t, c->d_annex_base, c->d_xplan);
    } else if (c->counts_mode) {
        pc.e0 = c->h_e_tab[(size_t)t * 4]; pc.e1 = c->h_e_tab[(size_t)t * 4 + 1]; pc.e2 = c->h_e_tab[(size_t)t * 4 + 2];
        pc.u0 = host_resample_u0(c->run_seed, (uint64_t)t + 1);
        pc.rs = c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED ? kFixStratified : kFixSystematic; pc.seed = c->run_seed; pc.draw = kResampleDrawBase + (uint64_t)t + 1;
        hipLaunchKernelGGL((exchange_plan_kernel<true, false>), dim3(1), dim3(kWave), 0, c->stream, g, pc, (const double*)c->d_obound, t, c->d_annex_base, c->d_xplan, ScanArgs{});
    } else if (c->scan2_deferred) {
        const ScanArgs sa = make_scan_args(c, t, 2, c->x_all_totals, c->x_world, c->x_rank);
        hipLaunchKernelGGL((exchange_plan_kernel<false, true>), dim3(1), dim3(kWave), 0, c->stream, g, pc, (const double*)c->d_obound, t, c->d_annex_base, c->d_xplan, sa);
        c->scan2_deferred = false;
    } else {
        hipLaunchKernelGGL((exchange_plan_kernel<false, false>), dim3(1), dim3(kWave), 0, c->stream, g, pc, (const double*)c->d_obound, t, c->d_annex_base, c->d_xplan, ScanArgs{});
    }
    c->x_plan_t = t;
    return 0;
}

template <class Model, class R>
void launch_pack(cpprob_hip_ctx* c, int t, R* d_send, int grid, bool plan_inside = false)
{
    PackArgs<Model, R> a{};
    if (c->x_direct && c->x_fixed) { a.peer_recv = c->d_peer_recv; a.peer_slot = c->d_peer_slot; a.cap = c->x_cap; }
    a.geom.no_history = c->keep ? 0 : 1; a.geom.remote = (c->x_remote && c->keep && c->x_fixed) ? 1 : 0;
    if (a.geom.remote) { a.geom.rem = c->d_remote; a.geom.annex_all = c->d_annex_all; a.peer_recv = nullptr; }
    if (a.geom.remote && c->trace_shard_run) { a.trace_cur = c->d_tr[t & 1]; a.trace_par = t & 1; a.geom.trace_words = 1; }
    if (plan_inside) {
        a.geom.world = c->x_world; a.geom.rank = c->x_rank; a.geom.n = c->n; a.geom.shard_begin = c->d_shard_begin; a.geom.slot_of_rank = c->d_slot_of_rank;
        a.geom.cap = c->x_cap; a.geom.annex_cap = c->annex_cap; a.geom.bytes_per_value = (int)c->ssz; a.geom.sent_per_step = c->d_sent;
        a.annex_base = c->d_annex_base; a.plan_out = c->d_xplan;
        if (a.geom.remote) { a.geom.slot_of_rank = nullptr; a.geom.cap = (int64_t)1 << 40; }     // (no segments: straight into the receivers' annexes)
    }
    a.values = static_cast<const typename Model::store_t*>(c->d_values); a.anc = c->d_anc; a.rs = c->rs; a.n = c->n; a.nb = c->nb;
    a.resampled = c->d_resampled; a.t = t; a.plan = c->d_xplan; a.world = c->x_world; a.rank = c->x_rank; a.send = d_send;
    a.skip = (c->keep && !a.geom.remote && c->d_skip && t >= 2 * kSkipEvery) ? c->d_skip : nullptr;
    const dim3 pgrid((unsigned)grid, a.skip ? (unsigned)(t / kSkipEvery + 1) : 1u);
    a.pc.all_totals = c->x_all_totals; a.pc.n_pop = (double)c->pop_n;
    a.wrel = c->d_wrel[c->cur]; a.bc = c->d_bc; a.bf = c->d_bf; a.ctrl = c->d_ctrl; a.seed = c->run_seed; a.pid0 = c->cfg.particle_offset;
    if constexpr (Model::kWeightTable == 3 && sizeof(typename Model::store_t) == 1) {
        if (c->counts_mode) {
            const int kn = (t + 1 + c->hier_phase_run) % 3;            // the copy step t wrote = the one step t+1 reads
            hier_view(c, kn, a.h);
            a.pc.e0 = c->h_e_tab[(size_t)t * 4]; a.pc.e1 = c->h_e_tab[(size_t)t * 4 + 1]; a.pc.e2 = c->h_e_tab[(size_t)t * 4 + 2];
            a.pc.u0 = host_resample_u0(c->run_seed, (uint64_t)t + 1);
            a.pc.rs = c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED ? kFixStratified : kFixSystematic; a.pc.seed = c->run_seed; a.pc.draw = kResampleDrawBase + (uint64_t)t + 1;
            if (plan_inside) hipLaunchKernelGGL((exchange_pack_kernel<Model, R, kPackCounts, true>), pgrid, dim3(kThreads), 0, c->stream, a);
            else hipLaunchKernelGGL((exchange_pack_kernel<Model, R, kPackCounts, false>), pgrid, dim3(kThreads), 0, c->stream, a);
            return;
        }
    }
    if (c->fixed_mode) {
        const int kn = (t + 1 + c->hier_phase_run) % 3;
        fhier_view(c, kn, a.f);
        a.pf.all_totals = reinterpret_cast<const uint64_t*>(c->x_all_totals); a.pf.u0 = host_resample_u0(c->run_seed, (uint64_t)t + 1); a.pf.n_pop = (double)c->pop_n;
        a.pf.ess_frac = c->cfg.ess_threshold;
        a.pf.rs = c->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED ? kFixStratified : kFixSystematic; a.pf.seed = c->run_seed; a.pf.draw = kResampleDrawBase + (uint64_t)t + 1;
        a.q_prev = c->d_q[c->cur];                                     // the weights of the generation step t just produced
        if (plan_inside) hipLaunchKernelGGL((exchange_pack_kernel<Model, R, kPackFixed, true>), pgrid, dim3(kThreads), 0, c->stream, a);
        else hipLaunchKernelGGL((exchange_pack_kernel<Model, R, kPackFixed, false>), pgrid, dim3(kThreads), 0, c->stream, a);
        return;
    }
    hipLaunchKernelGGL((exchange_pack_kernel<Model, R, kPackFloat, false>), pgrid, dim3(kThreads), 0, c->stream, a);
}

// Multinomial resampling (strata form) in the exchange scope, remote lineages: what the ranks' boundaries cut (one workgroup per
// boundary), then the packing launch that derives the plan from it and stores every migrant into its column of the receiver's annex.
static bool strata_exchange(const cpprob_hip_ctx* c)
{
    return c->exchange && c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL && (c->counts_mode || c->fixed_mode);
}
template <class Model>
void launch_pack_strata(cpprob_hip_ctx* c, int t, int grid)
{
    const int k = strata_k_of(c);
    const uint32_t* offs = c->d_strata + (size_t)t * (((size_t)1 << k) + 1);      // the strata of the resampling in front of step t + 1
    if (c->x_world > 1) {
        CutArgs ca{};
        ca.world = c->x_world; ca.shard_begin = c->d_shard_begin; ca.offs = offs; ca.k = k; ca.seed = c->run_seed; ca.draw2 = kResampleDrawBase2 + (uint64_t)t + 1;
        ca.totals_u = reinterpret_cast<const uint64_t*>(c->x_all_totals); ca.n_pop = (double)c->pop_n; ca.ess_frac = c->cfg.ess_threshold;
        ca.totals_d = c->x_all_totals;
        if (c->counts_mode) { ca.e0 = c->h_e_tab[(size_t)t * 4]; ca.e1 = c->h_e_tab[(size_t)t * 4 + 1]; ca.e2 = c->h_e_tab[(size_t)t * 4 + 2]; }
        ca.tab = c->d_cut_tab; ca.head = c->d_cut_head; ca.srccnt = c->d_cut_srccnt;
        if (c->counts_mode) hipLaunchKernelGGL((exchange_cut_kernel<true>), dim3((unsigned)(c->x_world - 1)), dim3(kThreads), 0, c->stream, ca);
        else hipLaunchKernelGGL((exchange_cut_kernel<false>), dim3((unsigned)(c->x_world - 1)), dim3(kThreads), 0, c->stream, ca);
    }
    PackStrataArgs<Model> a{};
    a.values = static_cast<const typename Model::store_t*>(c->d_values); a.rs = c->rs; a.n = c->n; a.nb = c->nb; a.t = t;
    a.world = c->x_world; a.rank = c->x_rank; a.pid0 = c->cfg.particle_offset; a.n_pop = (double)c->pop_n;
    a.geom.world = c->x_world; a.geom.rank = c->x_rank; a.geom.n = c->n; a.geom.shard_begin = c->d_shard_begin; a.geom.slot_of_rank = nullptr;
    a.geom.cap = (int64_t)1 << 40; a.geom.annex_cap = c->annex_cap; a.geom.bytes_per_value = (int)c->ssz; a.geom.sent_per_step = c->d_sent;
    a.geom.no_history = 0; a.geom.remote = 1; a.geom.rem = c->d_remote; a.geom.annex_all = c->d_annex_all;
    a.annex_base = c->d_annex_base; a.plan_out = c->d_xplan;
    a.cut = cut_view(c); a.offs = offs; a.k = k; a.seed = c->run_seed; a.draw2 = kResampleDrawBase2 + (uint64_t)t + 1;
    if (c->trace_shard_run) { a.trace_cur = c->d_tr[t & 1]; a.trace_par = t & 1; a.geom.trace_words = 1; }
    const int kn = (t + 1 + c->hier_phase_run) % 3;                    // the copy step t wrote = the one step t + 1 reads
    if constexpr (Model::kWeightTable == 3 && sizeof(typename Model::store_t) == 1) {
        if (c->counts_mode) {
            hier_view(c, kn, a.h);
            a.totals_d = c->x_all_totals; a.e0 = c->h_e_tab[(size_t)t * 4]; a.e1 = c->h_e_tab[(size_t)t * 4 + 1]; a.e2 = c->h_e_tab[(size_t)t * 4 + 2];
            hipLaunchKernelGGL((exchange_pack_strata_kernel<Model, kPackCounts>), dim3((unsigned)grid), dim3(kThreads), 0, c->stream, a);
            return;
        }
    }
    if constexpr (std::is_same<Model, ModelLinearGaussian1D>::value || std::is_same<Model, ModelHmm3>::value || std::is_same<Model, ModelHmmK>::value) {
        fhier_view(c, kn, a.f);
        a.totals_u = reinterpret_cast<const uint64_t*>(c->x_all_totals); a.ess_frac = c->cfg.ess_threshold; a.q_prev = c->d_q[c->cur];
        hipLaunchKernelGGL((exchange_pack_strata_kernel<Model, kPackFixed>), dim3((unsigned)grid), dim3(kThreads), 0, c->stream, a);
    }
}

template <class Model, class R>
void launch_commit(cpprob_hip_ctx* c, int t, const R* d_recv, int grid)
{
    using S = typename Model::store_t;
    hipLaunchKernelGGL((exchange_commit_kernel<S, R>), dim3(grid), dim3(kThreads), 0, c->stream, (const ExchangePlan*)c->d_xplan, c->x_world, d_recv, t,
                       (const int64_t*)c->d_annex_base, static_cast<S*>(c->d_values), c->d_anc, c->rs, c->ld, c->d_skip);
}

// more annex columns: re-stride values[] / anc[] (callers that synchronise per step only)
int grow_annex(cpprob_hip_ctx* c, int64_t need)
{
    int64_t cap = std::max<int64_t>(2 * c->annex_cap, (need + kTile - 1) / kTile * kTile);
    const size_t T = (size_t)c->cap_T, vsz = c->ssz;
    const size_t ldc = c->cap_particles, rs_new = (size_t)c->ld + (size_t)cap, rs_old = (size_t)c->rs;
    void* nv = nullptr; int32_t* na = nullptr;
    HIP_TRY(c, hipMalloc(&nv, T * (ldc + (size_t)cap) * vsz));
    HIP_TRY(c, hipMalloc(&na, T * (ldc + (size_t)cap) * sizeof(int32_t)));
    HIP_TRY(c, hipMemsetAsync(nv, 0, T * (ldc + (size_t)cap) * vsz, c->stream));
    HIP_TRY(c, hipMemsetAsync(na, 0, T * (ldc + (size_t)cap) * sizeof(int32_t), c->stream));
    const size_t used = (size_t)(c->ld + c->annex_used);
    HIP_TRY(c, hipMemcpy2DAsync(nv, rs_new * vsz, c->d_values, rs_old * vsz, used * vsz, (size_t)c->T, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpy2DAsync(na, rs_new * 4, c->d_anc, rs_old * 4, used * 4, (size_t)c->T, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->d_skip) {
        int32_t* ns = nullptr;
        const size_t M = T / kSkipEvery + 1;
        HIP_TRY(c, hipMalloc(&ns, M * (ldc + (size_t)cap) * sizeof(int32_t)));
        HIP_TRY(c, hipMemsetAsync(ns, 0, M * (ldc + (size_t)cap) * sizeof(int32_t), c->stream));
        HIP_TRY(c, hipMemcpy2DAsync(ns, rs_new * 4, c->d_skip, rs_old * 4, used * 4, (size_t)c->T / kSkipEvery + 1, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        dfree(c->d_skip); c->d_skip = ns;
    }
    dfree(c->d_values); dfree(c->d_anc);
    c->d_values = nv; c->d_anc = na; c->annex_cap = cap; c->rs = c->ld + cap;
    return 0;
}

}  // namespace

extern "C" {

// ---- exchange, synchronising form: the caller sizes its buffers from host-visible counts ----
int cpprob_hip_exchange_plan(cpprob_hip_ctx* c, int32_t t, int32_t world, int32_t rank, const uint64_t* h_shard_begin, uint64_t* h_send_counts,
                             uint64_t* h_recv_counts, int32_t* h_do_resample)
{
    LANES_OWN(c);
    if (!c || !h_shard_begin || !h_send_counts || !h_recv_counts) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->exchange) return fail(c, CPPROB_HIP_ESTATE, "the context was not begun with resample_scope = CPPROB_HIP_SCOPE_EXCHANGE");
    if (c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL)
        return fail(c, CPPROB_HIP_EUNSUPPORTED, "multinomial resampling in the exchange scope moves its migrants by remote lineages (cpprob_hip_exchange_setup / _direct / _remote, "
                                                 "then cpprob_hip_exchange_pack_async): the synchronising plan / pack / commit calls serve systematic and stratified resampling");
    if (t < 0 || t >= c->T) return fail(c, CPPROB_HIP_EINVAL, "step out of range");
    if (!c->step_protocol || c->step_t != t || !c->x_all_totals || world != c->x_world || rank != c->x_rank)
        return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_exchange_plan(t) follows cpprob_hip_smc_step_end(t) with the same world / rank");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = upload_geometry(c, world, rank, h_shard_begin)) return rc;
    if (int rc = launch_plan(c, t, false)) return rc;
    HIP_TRY(c, hipGetLastError());
    ExchangePlan h;
    HIP_TRY(c, hipMemcpyAsync(&h, c->d_xplan, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    auto& p = c->plan;
    p.t = t; p.resample = h.resample != 0; p.n_send = (uint64_t)h.n_send; p.n_recv = (uint64_t)h.n_recv; p.l0 = h.l0; p.l1 = h.l1;
    for (int r = 0; r < world; ++r) { h_send_counts[r] = (uint64_t)h.send_cnt[r]; h_recv_counts[r] = (uint64_t)h.recv_cnt[r]; }
    if (h_do_resample) *h_do_resample = p.resample ? 1 : 0;
    if (p.resample && (int64_t)p.n_recv != c->n - (p.l1 - p.l0)) return fail(c, CPPROB_HIP_EDEVICE, "exchange plan does not cover the shard");
    return 0;
}

int cpprob_hip_exchange_pack(cpprob_hip_ctx* c, int32_t t, void* d_send)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    auto& p = c->plan;
    if (!c->exchange || p.t != t) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_exchange_plan(t) has not run");
    if (!p.resample || p.n_send == 0) return 0;
    if (!d_send) return fail(c, CPPROB_HIP_EINVAL, "d_send is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    const int grid = (int)std::min<uint64_t>((p.n_send + kTile - 1) / kTile + 1, 1024);
    dispatch_model(c, [&](auto m) { using M = decltype(m); launch_pack<M, typename M::value_t>(c, t, static_cast<typename M::value_t*>(d_send), grid); });
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_exchange_commit(cpprob_hip_ctx* c, int32_t t, const void* d_recv)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    auto& p = c->plan;
    if (!c->exchange || p.t != t) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_exchange_plan(t) has not run");
    if (!p.resample || p.n_recv == 0) return 0;
    if (!d_recv) return fail(c, CPPROB_HIP_EINVAL, "d_recv is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->ld + c->annex_used + (int64_t)p.n_recv + kTile > (int64_t)INT32_MAX) return fail(c, CPPROB_HIP_EINVAL, "immigrant columns exceed int32 ancestor indices");
    if (c->annex_used_before.size() < (size_t)c->T + 1) c->annex_used_before.assign((size_t)c->T + 1, -1);
    c->annex_used_before[(size_t)t] = c->annex_used;
    if (c->annex_used + (int64_t)p.n_recv > c->annex_cap) { if (int rc = grow_annex(c, c->annex_used + (int64_t)p.n_recv)) return rc; }
    const int grid = (int)std::min<uint64_t>((p.n_recv * (uint64_t)(t + 1) + kThreads - 1) / kThreads, 2048);
    dispatch_model(c, [&](auto m) { using M = decltype(m); launch_commit<M, typename M::value_t>(c, t, static_cast<const typename M::value_t*>(d_recv), grid); });
    HIP_TRY(c, hipGetLastError());
    c->annex_used += (int64_t)p.n_recv;
    return 0;
}

// ---- exchange, stream-ordered form: fixed-capacity transport segments, no host synchronisation inside a run ----
int cpprob_hip_exchange_setup(cpprob_hip_ctx* c, int32_t world, int32_t rank, const uint64_t* h_shard_begin, int32_t all_peers, uint64_t records_per_peer)
{
    LANES_OWN(c);
    if (!c || !h_shard_begin) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->begun || !c->exchange) return fail(c, CPPROB_HIP_ESTATE, "begin the context with resample_scope = CPPROB_HIP_SCOPE_EXCHANGE first");
    if (records_per_peer == 0) return fail(c, CPPROB_HIP_EINVAL, "records_per_peer must be > 0");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = upload_geometry(c, world, rank, h_shard_begin)) return rc;
    std::vector<int32_t> slot((size_t)kWorldSlots, -1);
    c->x_peers.clear();
    if (all_peers == 2 && world != 1) return fail(c, CPPROB_HIP_EINVAL, "all_peers = 2 (a rank that is its own peer) is the one-rank diagnostic");
    for (int r = 0; r < world; ++r) {
        if (r == rank && all_peers != 2) continue;
        if (all_peers || r == rank - 1 || r == rank + 1) { slot[(size_t)r] = (int32_t)c->x_peers.size(); c->x_peers.push_back(r); }
    }
    if (!c->d_slot_of_rank) HIP_TRY(c, hipMalloc(&c->d_slot_of_rank, kWorldSlots * sizeof(int32_t)));
    HIP_TRY(c, hipMemcpy(c->d_slot_of_rank, slot.data(), kWorldSlots * sizeof(int32_t), hipMemcpyHostToDevice));
    c->x_cap = (int64_t)records_per_peer; c->x_mode = all_peers ? 1 : 0; c->x_fixed = true;
    const size_t need = std::max<size_t>(1, c->x_peers.size()) * (size_t)records_per_peer * (size_t)c->T * c->ssz;
    if (need > c->x_buf_bytes) {
        dfree(c->d_xsend); dfree(c->d_xrecv);
        HIP_TRY(c, hipMalloc(&c->d_xsend, need));
        HIP_TRY(c, hipMalloc(&c->d_xrecv, need));
        c->x_buf_bytes = need;
    }
    c->x_world = world; c->x_rank = rank;
    c->x_direct = false; c->x_remote = false; c->trace_shard = false;   // (the peers' buffers may have moved: cpprob_hip_exchange_direct / _remote again)
    if (c->T > c->sent_cap) { dfree(c->d_sent); HIP_TRY(c, hipMalloc(&c->d_sent, (size_t)c->T * sizeof(int64_t))); c->sent_cap = c->T; }
    HIP_TRY(c, hipMemset(c->d_sent, 0, (size_t)c->sent_cap * sizeof(int64_t)));
    return 0;
}

int cpprob_hip_exchange_direct(cpprob_hip_ctx* c, void* const* h_peer_recv)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!c->x_fixed) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_exchange_setup has not run");
    if (!h_peer_recv) { c->x_direct = false; return 0; }
    HIP_TRY(c, hipSetDevice(c->device));
    // the slot each peer keeps for this rank: its peer list is the ranks around it (or every other rank) in rank order
    std::vector<void*> ptr((size_t)kWorldSlots, nullptr);
    std::vector<int32_t> slot((size_t)kWorldSlots, 0);
    for (int r : c->x_peers) {
        if (!h_peer_recv[r]) return fail(c, CPPROB_HIP_EINVAL, "cpprob_hip_exchange_direct: no receive buffer for a peer rank");
        ptr[(size_t)r] = h_peer_recv[r];
        if (r == c->x_rank) slot[(size_t)r] = 0;                               // (one-rank diagnostic: its own, only, slot)
        else if (c->x_mode) slot[(size_t)r] = c->x_rank < r ? c->x_rank : c->x_rank - 1;
        else slot[(size_t)r] = (c->x_rank == r - 1) ? 0 : (r - 1 >= 0 ? 1 : 0);
    }
    if (!c->d_peer_recv) HIP_TRY(c, hipMalloc(&c->d_peer_recv, kWorldSlots * sizeof(void*)));
    if (!c->d_peer_slot) HIP_TRY(c, hipMalloc(&c->d_peer_slot, kWorldSlots * sizeof(int32_t)));
    HIP_TRY(c, hipMemcpy(c->d_peer_recv, ptr.data(), kWorldSlots * sizeof(void*), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_peer_slot, slot.data(), kWorldSlots * sizeof(int32_t), hipMemcpyHostToDevice));
    c->x_direct = true;
    return 0;
}

// trace words of an exchange-scope shard (hmm<T <= 16> on the count form): the two word arrays over local + annex columns and the
// read-out's counters; `words` = this shard can carry them
static int ensure_shard_trace(cpprob_hip_ctx* c, bool& words)
{
    words = false;
    dispatch_model(c, [&](auto m) { words = counts_eligible<decltype(m)>(c); });
    words = words && c->keep && c->cfg.model == CPPROB_HIP_MODEL_HMM3 && c->T <= kTraceMaxT && !(c->cfg.flags & CPPROB_HIP_FLAG_WALK_READOUT);
    if (!words) return 0;
    if ((size_t)c->rs > c->tr_cap || !c->d_tr[0]) {
        dfree(c->d_tr[0]); dfree(c->d_tr[1]);
        HIP_TRY(c, hipMalloc(&c->d_tr[0], (size_t)c->rs * sizeof(uint32_t)));
        HIP_TRY(c, hipMalloc(&c->d_tr[1], (size_t)c->rs * sizeof(uint32_t)));
        HIP_TRY(c, hipMemset(c->d_tr[0], 0, (size_t)c->rs * sizeof(uint32_t)));
        HIP_TRY(c, hipMemset(c->d_tr[1], 0, (size_t)c->rs * sizeof(uint32_t)));
        c->tr_cap = (size_t)c->rs;
    }
    if (!c->d_trace_cnt) {
        HIP_TRY(c, hipMalloc(&c->d_trace_cnt, kTraceCounterWords * sizeof(uint32_t)));
        HIP_TRY(c, hipMalloc(&c->d_trace_arrive, sizeof(unsigned long long)));
        HIP_TRY(c, hipMemset(c->d_trace_cnt, 0, kTraceCounterWords * sizeof(uint32_t)));
        HIP_TRY(c, hipMemset(c->d_trace_arrive, 0, sizeof(unsigned long long)));
    }
    return 0;
}

int cpprob_hip_exchange_store(cpprob_hip_ctx* c, cpprob_hip_store* out)
{
    LANES_OWN(c);
    if (!c || !out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->begun || !c->exchange || !c->keep) return fail(c, CPPROB_HIP_ESTATE, "no history-keeping exchange-scope run begun");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->annex_cap > c->origin_cap || !c->d_origin) {
        dfree(c->d_origin);
        HIP_TRY(c, hipMalloc(&c->d_origin, (size_t)std::max<int64_t>(c->annex_cap, 1) * sizeof(int64_t)));
        c->origin_cap = c->annex_cap;
    }
    out->d_values = c->d_values; out->d_ancestors = c->d_anc; out->d_origin = c->d_origin; out->row_stride = (uint64_t)c->rs; out->n_local_columns = (uint64_t)c->ld;
    // short discrete traces on the count form: the particles carry their traces across ranks too (trace_words.hpp)
    out->d_trace[0] = nullptr; out->d_trace[1] = nullptr;
    bool words = false;
    if (int rc = ensure_shard_trace(c, words)) return rc;
    if (words) { out->d_trace[0] = c->d_tr[0]; out->d_trace[1] = c->d_tr[1]; }
    return 0;
}

int cpprob_hip_exchange_remote(cpprob_hip_ctx* c, const cpprob_hip_store* h_stores)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!c->x_fixed || !c->x_direct) return fail(c, CPPROB_HIP_ESTATE, "remote lineages ride the direct transport: cpprob_hip_exchange_setup and _direct first");
    if (!h_stores) { c->x_remote = false; c->trace_shard = false; return 0; }
    if (!c->keep) return 0;                                 // (a filtering-only shard has no lineages to leave anywhere)
    HIP_TRY(c, hipSetDevice(c->device));
    RemoteStores rs{};
    rs.world = c->x_world; rs.rank = c->x_rank;
    for (int r = 0; r < c->x_world; ++r) {
        if (!h_stores[r].d_values || !h_stores[r].d_ancestors || !h_stores[r].d_origin) return fail(c, CPPROB_HIP_EINVAL, "cpprob_hip_exchange_remote: a rank's store is missing");
        rs.values[r] = h_stores[r].d_values; rs.anc[r] = static_cast<const int32_t*>(h_stores[r].d_ancestors); rs.origin[r] = static_cast<const int64_t*>(h_stores[r].d_origin);
        rs.rs[r] = (int64_t)h_stores[r].row_stride; rs.ld[r] = (int64_t)h_stores[r].n_local_columns;
    }
    bool words = true;
    for (int r = 0; r < c->x_world; ++r) words = words && h_stores[r].d_trace[0] && h_stores[r].d_trace[1];
    for (int r = 0; r < c->x_world; ++r)
        for (int k = 0; k < 2; ++k) rs.trace[k][r] = words ? static_cast<uint32_t*>(const_cast<void*>(h_stores[r].d_trace[k])) : nullptr;
    c->trace_shard = words && c->d_tr[0] != nullptr;
    if (!c->d_remote) HIP_TRY(c, hipMalloc(&c->d_remote, sizeof(RemoteStores)));
    if (c->T + 1 > c->annex_all_T || !c->d_annex_all) {
        dfree(c->d_annex_all);
        HIP_TRY(c, hipMalloc(&c->d_annex_all, (size_t)(c->T + 1) * kWorldSlots * sizeof(int64_t)));
        c->annex_all_T = c->T + 1;
    }
    HIP_TRY(c, hipMemcpy(c->d_remote, &rs, sizeof rs, hipMemcpyHostToDevice));
    c->x_remote = true;
    return 0;
}

int cpprob_hip_exchange_traffic(cpprob_hip_ctx* c, int64_t* h_sent_per_step, size_t n_steps, uint64_t* h_records, uint64_t* h_bytes)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!c->exchange || !c->d_xplan || !c->d_sent) return fail(c, CPPROB_HIP_ESTATE, "no exchange-scope run on a fixed transport");
    HIP_TRY(c, hipSetDevice(c->device));
    ExchangePlan h;
    HIP_TRY(c, hipMemcpyAsync(&h, c->d_xplan, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if (h_sent_per_step) {
        if (n_steps < (size_t)c->T) return fail(c, CPPROB_HIP_EINVAL, "h_sent_per_step too small");
        HIP_TRY(c, hipMemcpyAsync(h_sent_per_step, c->d_sent, (size_t)c->T * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_records) *h_records = (uint64_t)h.run_records;
    if (h_bytes) *h_bytes = (uint64_t)h.run_bytes;
    return 0;
}

int cpprob_hip_exchange_transport(cpprob_hip_ctx* c, void** d_send, void** d_recv, int32_t* n_peers, int32_t* h_peers, uint64_t* records_per_peer,
                                  uint64_t* bytes_per_value)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!c->x_fixed) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_exchange_setup has not run");
    if (d_send) *d_send = c->d_xsend;
    if (d_recv) *d_recv = c->d_xrecv;
    if (n_peers) *n_peers = (int32_t)c->x_peers.size();
    if (h_peers) for (size_t i = 0; i < c->x_peers.size(); ++i) h_peers[i] = c->x_peers[i];
    if (records_per_peer) *records_per_peer = (uint64_t)c->x_cap;
    if (bytes_per_value) *bytes_per_value = (uint64_t)c->ssz;
    return 0;
}

int cpprob_hip_exchange_pack_async(cpprob_hip_ctx* c, int32_t t)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!c->exchange || !c->x_fixed) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_exchange_setup has not run");
    if (!c->step_protocol || c->step_t != t || !c->x_all_totals) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_exchange_pack_async(t) follows cpprob_hip_smc_step_end(t)");
    if (t < 0 || t + 1 >= c->T) return fail(c, CPPROB_HIP_EINVAL, "no exchange follows the last step");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->keep && !c->counts_mode && !c->fixed_mode) return fail(c, CPPROB_HIP_EUNSUPPORTED, "filtering-only shards run on the integer forms of the step (systematic resampling)");
    // count form: the plan is a pure function of the all-gathered totals -- every packing workgroup derives it on its first wavefront
    // and workgroup 0 stores it (one launch less per step); floating-point form: the plan launch also combines the ranks' totals
    const bool plan_inside = c->counts_mode || c->fixed_mode;
    if (c->cfg.resampler == CPPROB_HIP_RESAMPLE_MULTINOMIAL) {
        if (!strata_exchange(c)) return fail(c, CPPROB_HIP_EUNSUPPORTED, "multinomial resampling in the exchange scope runs on the integer forms of the step");
        if (c->x_peers.empty()) { c->x_plan_t = t; c->plan.t = t; return 0; }     // (a group of one: every threshold lies in its own mass)
        if (!(c->x_remote && c->keep))
            return fail(c, CPPROB_HIP_EUNSUPPORTED, "multinomial resampling in the exchange scope needs remote lineages (every rank addresses every rank's particle store: "
                                                     "cpprob_hip_exchange_remote) -- its migrants are not one interval per peer, so the segment transports do not carry them");
        c->x_plan_t = t;
        const int grid = (int)std::min<int64_t>(std::max<int64_t>(1, (c->x_cap + kTile - 1) / kTile), 256);
        dispatch_model(c, [&](auto m) { launch_pack_strata<decltype(m)>(c, t, grid); });
        HIP_TRY(c, hipGetLastError());
        c->plan.t = t;
        return 0;
    }
    if (c->x_peers.empty()) {
        // nobody to exchange with (a group of one): the count form's step derives everything it needs from the totals; the
        // floating-point form's plan launch still combines the ranks' totals into ctrl
        if (!plan_inside) { if (int rc = launch_plan(c, t, true)) return rc; HIP_TRY(c, hipGetLastError()); }
        c->x_plan_t = t; c->plan.t = t;
        return 0;
    }
    if (!plan_inside) { if (int rc = launch_plan(c, t, true)) return rc; }
    else c->x_plan_t = t;
    // enough workgroups for a full segment per peer; those beyond the planned tiles leave at once
    const int grid = (int)std::min<int64_t>(std::max<int64_t>(1, (c->x_cap + kTile - 1) / kTile), 256);
    dispatch_model(c, [&](auto m) { using M = decltype(m); launch_pack<M, typename M::store_t>(c, t, static_cast<typename M::store_t*>(c->d_xsend), grid, plan_inside); });
    HIP_TRY(c, hipGetLastError());
    c->plan.t = t;
    return 0;
}

int cpprob_hip_exchange_commit_async(cpprob_hip_ctx* c, int32_t t)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!c->exchange || !c->x_fixed || c->x_plan_t != t) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_exchange_pack_async(t) has not run");
    if (c->x_peers.empty()) return 0;
    if (c->x_remote && c->keep) return 0;                  // (remote lineages: the senders stored into this rank's annex themselves)
    HIP_TRY(c, hipSetDevice(c->device));
    dispatch_model(c, [&](auto m) { using M = decltype(m); launch_commit<M, typename M::store_t>(c, t, static_cast<const typename M::store_t*>(c->d_xrecv), 256); });
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_exchange_status(cpprob_hip_ctx* c, int32_t* h_overflow, uint64_t* h_annex_used)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!c->exchange || !c->d_xplan) return fail(c, CPPROB_HIP_ESTATE, "no exchange-scope run");
    HIP_TRY(c, hipSetDevice(c->device));
    int32_t head[2] = {0, 0};
    std::vector<int64_t> ab((size_t)c->T + 1, 0);
    HIP_TRY(c, hipMemcpyAsync(head, c->d_xplan, sizeof head, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ab.data(), c->d_annex_base, ab.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_overflow) *h_overflow = head[1];
    if (h_annex_used) *h_annex_used = (uint64_t)(c->T >= 2 ? ab[(size_t)c->T - 1] : 0);
    return 0;
}

static int infer_summary_impl(cpprob_hip_ctx* c, cpprob_hip_summary* out);
int cpprob_hip_infer_summary(cpprob_hip_ctx* c, cpprob_hip_summary* out)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return infer_summary_impl(l, out); });
}
static int infer_summary_impl(cpprob_hip_ctx* c, cpprob_hip_summary* out)
{
    if (!c || !out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished run");
    if (int rc = settle_fixed(c)) return rc;
    StepCtrl h{};
    HIP_TRY(c, hipMemcpyAsync(&h, c->d_ctrl, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out->log_evidence = h.log_z;
    out->ess_final = h.ess;
    out->log_norm = h.M + std::log(h.W);
    out->max_logw = h.M;
    out->n_predict = c->T;
    out->stats_per_predict = c->K;
    out->is_int = c->is_int ? 1 : 0;
    out->n_resampled = h.n_resampled;
    out->step_form = c->cfg.algorithm != CPPROB_HIP_ALG_SMC ? CPPROB_HIP_FORM_FLOAT : (c->fixed_mode ? CPPROB_HIP_FORM_FIXED : (c->counts_mode ? CPPROB_HIP_FORM_COUNTS : CPPROB_HIP_FORM_FLOAT));
    out->n_requantised = c->fixed_mode ? c->n_requantised : 0;
    return 0;
}

// Everything cpprob::inference reads when a run is over -- the summary, the per-predict statistics, the step trace -- behind ONE stream
// synchronisation, through pinned memory (three calls of the single-purpose functions above cost three host round trips, each
// a blocking copy into pageable memory: ~40 us on a 150-us run).
static void fill_summary(const cpprob_hip_ctx* c, const StepCtrl& h, cpprob_hip_summary* out)
{
    out->log_evidence = h.log_z;
    out->ess_final = h.ess;
    out->log_norm = h.M + std::log(h.W);
    out->max_logw = h.M;
    out->n_predict = c->T;
    out->stats_per_predict = c->K;
    out->is_int = c->is_int ? 1 : 0;
    out->n_resampled = h.n_resampled;
    out->step_form = c->cfg.algorithm != CPPROB_HIP_ALG_SMC ? CPPROB_HIP_FORM_FLOAT : (c->fixed_mode ? CPPROB_HIP_FORM_FIXED : (c->counts_mode ? CPPROB_HIP_FORM_COUNTS : CPPROB_HIP_FORM_FLOAT));
    out->n_requantised = c->fixed_mode ? c->n_requantised : 0;
}
static int infer_results_impl(cpprob_hip_ctx* c, cpprob_hip_summary* out, double* h_stats, size_t n_doubles, double* h_ess, int32_t* h_resampled);
int cpprob_hip_infer_results(cpprob_hip_ctx* c, cpprob_hip_summary* out, double* h_stats, size_t n_doubles, double* h_ess, int32_t* h_resampled)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return infer_results_impl(l, out, h_stats, n_doubles, h_ess, h_resampled); });
}
static int infer_results_impl(cpprob_hip_ctx* c, cpprob_hip_summary* out, double* h_stats, size_t n_doubles, double* h_ess, int32_t* h_resampled)
{
    if (!c || !out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished run");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t T = (size_t)c->T, need = T * (size_t)c->K;
    if (h_stats && n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "h_stats too small");
    const bool sis = c->cfg.algorithm == CPPROB_HIP_ALG_SIS;
    const size_t o_ctrl = 0, o_stats = (sizeof(StepCtrl) + 15) / 16 * 16, o_ess = o_stats + need * sizeof(double), o_res = o_ess + T * sizeof(double), total = o_res + T * sizeof(int32_t);
    if (int rc = pin_reserve(c, total)) return rc;
    for (int pass = 0; pass < 2; ++pass) {
        char* const pin = pin_data(c);
        PinPack pk;
        pk.add(c->d_ctrl, pin + o_ctrl, sizeof(StepCtrl));
        if (h_stats) pk.add(c->d_stats, pin + o_stats, need * sizeof(double));
        if (h_ess && sis) pk.add(c->d_ess + (T - 1), pin + o_ess + (T - 1) * sizeof(double), sizeof(double));
        else if (h_ess) pk.add(c->d_ess, pin + o_ess, T * sizeof(double));
        if (h_resampled && !sis) pk.add(c->d_resampled, pin + o_res, T * sizeof(int32_t));
        if (int rc = pk.launch(c)) return rc;
        if (int rc = pin_wait(c)) return rc;
        StepCtrl h;
        std::memcpy(&h, pin + o_ctrl, sizeof h);
        if (pass == 0 && c->fixed_check_pending) {
            // (a fixed-point run is settled on the same read-back: only a generation that lost its bits costs more round trips)
            if (h.fix_gap <= kFixGapLimit) c->fixed_check_pending = false;
            else { if (int rc = settle_fixed(c)) return rc; continue; }
        }
        fill_summary(c, h, out);
        if (h_stats) std::memcpy(h_stats, pin + o_stats, need * sizeof(double));
        if (h_ess) {
            std::memcpy(h_ess, pin + o_ess, T * sizeof(double));
            if (sis) for (size_t t = 0; t + 1 < T; ++t) h_ess[t] = 0.0;                  // (one weighting pass: only the final entry is defined)
        }
        if (h_resampled) {
            if (sis) for (size_t t = 0; t < T; ++t) h_resampled[t] = 0;
            else std::memcpy(h_resampled, pin + o_res, T * sizeof(int32_t));
        }
        return 0;
    }
    return fail(c, CPPROB_HIP_ESTATE, "the run did not settle");
}

static int infer_stats_impl(cpprob_hip_ctx* c, double* h_stats, size_t n_doubles);
int cpprob_hip_infer_stats(cpprob_hip_ctx* c, double* h_stats, size_t n_doubles)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return infer_stats_impl(l, h_stats, n_doubles); });
}
static int infer_stats_impl(cpprob_hip_ctx* c, double* h_stats, size_t n_doubles)
{
    if (!c || !h_stats) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished run");
    if (int rc = settle_fixed(c)) return rc;
    const size_t need = (size_t)c->T * c->K;
    if (n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "h_stats too small");
    HIP_TRY(c, hipMemcpyAsync(h_stats, c->d_stats, need * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

int cpprob_hip_infer_results_device(cpprob_hip_ctx* c, double* d_out, size_t n_doubles)
{
    if (!c || !d_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    c->lane_chain = false;
    cpprob_hip_ctx* const l = c->is_lane ? c : lane_of_last(c);       // (same configuration: T and K are the context's)
    if (!l->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished run");
    const size_t need = 4 + (size_t)c->T * c->K;
    if (n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "d_out too small");
    HIP_TRY(c, hipSetDevice(c->device));
    const int ns = c->T * c->K;
    if (l != c) {
        // the last run sits on a lane: the context's stream waits for it, and the lane's next run for this copy
        if (!c->lane_ev) HIP_TRY(c, hipEventCreateWithFlags(&c->lane_ev, hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->lane_ev, l->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->lane_ev, 0));
    }
    hipLaunchKernelGGL(pack_results_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, l->d_ctrl, l->d_stats, ns, d_out);
    HIP_TRY(c, hipGetLastError());
    if (l != c) {
        HIP_TRY(c, hipEventRecord(c->lane_ev, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(l->stream, c->lane_ev, 0));
    }
    return 0;
}

static int infer_step_trace_impl(cpprob_hip_ctx* c, double* h_ess, int32_t* h_resampled);
int cpprob_hip_infer_step_trace(cpprob_hip_ctx* c, double* h_ess, int32_t* h_resampled)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return infer_step_trace_impl(l, h_ess, h_resampled); });
}
static int infer_step_trace_impl(cpprob_hip_ctx* c, double* h_ess, int32_t* h_resampled)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!c->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished run");
    if (int rc = settle_fixed(c)) return rc;
    if (c->cfg.algorithm == CPPROB_HIP_ALG_SIS) {
        // one weighting pass: only the final entry is defined
        if (h_ess) { for (int t = 0; t < c->T; ++t) h_ess[t] = 0.0; }
        if (h_resampled) { for (int t = 0; t < c->T; ++t) h_resampled[t] = 0; }
        if (h_ess) HIP_TRY(c, hipMemcpyAsync(h_ess + (c->T - 1), c->d_ess + (c->T - 1), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    } else {
        if (h_ess) HIP_TRY(c, hipMemcpyAsync(h_ess, c->d_ess, (size_t)c->T * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (h_resampled) HIP_TRY(c, hipMemcpyAsync(h_resampled, c->d_resampled, (size_t)c->T * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int copy_rows(cpprob_hip_ctx* c, void* h, const void* d, size_t elem, size_t rows, size_t n_bytes, size_t stride)
{
    const size_t need = rows * (size_t)c->n * elem;
    if (n_bytes < need) return fail(c, CPPROB_HIP_EINVAL, "host buffer too small");
    HIP_TRY(c, hipMemcpy2DAsync(h, (size_t)c->n * elem, d, stride * elem, (size_t)c->n * elem, rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int copy_values_impl(cpprob_hip_ctx* c, void* h, size_t n_bytes);
int cpprob_hip_copy_values(cpprob_hip_ctx* c, void* h, size_t n_bytes)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return copy_values_impl(l, h, n_bytes); });
}
static int copy_values_impl(cpprob_hip_ctx* c, void* h, size_t n_bytes)
{
    if (!c || !h) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished run");
    if (int rc = settle_fixed(c)) return rc;
    if (!c->keep) return fail(c, CPPROB_HIP_ESTATE, "the run kept no history (keep_history = 0): traces and ancestors do not exist; its statistics are the filtering ones");
    const size_t vsz = c->is_int ? sizeof(int32_t) : sizeof(double);
    if (c->ssz == vsz) return copy_rows(c, h, c->d_values, vsz, (size_t)c->T, n_bytes, (size_t)c->rs);
    // narrow store: widen to the value type on the device first (d_paths doubles as the staging buffer)
    if (!c->d_paths) HIP_TRY(c, hipMalloc(&c->d_paths, (size_t)c->cap_T * c->cap_particles * vsz));
    dispatch_model(c, [&](auto m) {
        using S = typename decltype(m)::store_t; using V = typename decltype(m)::value_t;
        hipLaunchKernelGGL((widen_rows_kernel<S, V>), GRID1(c->n), static_cast<const S*>(c->d_values), c->rs, c->T, c->n, c->ld, static_cast<V*>(c->d_paths));
    });
    HIP_TRY(c, hipGetLastError());
    return copy_rows(c, h, c->d_paths, vsz, (size_t)c->T, n_bytes, (size_t)c->ld);
}

static int copy_ancestors_impl(cpprob_hip_ctx* c, int32_t* h, size_t n_bytes);
int cpprob_hip_copy_ancestors(cpprob_hip_ctx* c, int32_t* h, size_t n_bytes)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return copy_ancestors_impl(l, h, n_bytes); });
}
static int copy_ancestors_impl(cpprob_hip_ctx* c, int32_t* h, size_t n_bytes)
{
    if (!c || !h) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished run");
    if (int rc = settle_fixed(c)) return rc;
    if (!c->keep) return fail(c, CPPROB_HIP_ESTATE, "the run kept no history (keep_history = 0): traces and ancestors do not exist; its statistics are the filtering ones");
    if (c->cfg.algorithm != CPPROB_HIP_ALG_SMC) return fail(c, CPPROB_HIP_ESTATE, "SIS keeps no ancestors (every trace is its own line)");
    if (int rc = copy_rows(c, h, c->d_anc, sizeof(int32_t), (size_t)c->T, n_bytes, (size_t)c->rs)) return rc;
    if (c->final_from_fixed) {
        // the fixed-point step stores a row only where it resampled: the identity of the other rows is written here
        std::vector<int32_t> res((size_t)c->T, 0);
        HIP_TRY(c, hipMemcpy(res.data(), c->d_resampled, (size_t)c->T * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int t = 1; t < c->T; ++t)
            if (!res[(size_t)t - 1]) for (int64_t i = 0; i < c->n; ++i) h[(size_t)t * (size_t)c->n + (size_t)i] = (int32_t)i;
    }
    return 0;
}

static int copy_logw_impl(cpprob_hip_ctx* c, double* h, size_t n_bytes);
int cpprob_hip_copy_logw(cpprob_hip_ctx* c, double* h, size_t n_bytes)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return copy_logw_impl(l, h, n_bytes); });
}
static int copy_logw_impl(cpprob_hip_ctx* c, double* h, size_t n_bytes)
{
    if (!c || !h) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished run");
    if (int rc = settle_fixed(c)) return rc;
    if (c->final_from_counts) {
        // the run kept no log-weight array (they are a function of the final states): write it out now
        HIP_TRY(c, hipSetDevice(c->device));
        dispatch_model(c, [&](auto m) {
            using M = decltype(m);
            if constexpr (M::kWeightTable == 3 && sizeof(typename M::store_t) == 1) {
                const double* ll = &c->h_ll_tab[(size_t)(c->T - 1) * 3];
                hipLaunchKernelGGL(logw_from_states_kernel<M>, dim3((unsigned)((c->ld + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                                   static_cast<const typename M::store_t*>(c->d_values) + (int64_t)(c->keep ? c->T - 1 : ((c->T - 1) & 1)) * c->rs, c->n, c->ld, ll[0], ll[1], ll[2],
                                   c->d_logw[c->cur]);
            }
        });
    }
    return copy_rows(c, h, c->d_logw[c->cur], sizeof(double), 1, n_bytes, (size_t)c->ld);
}

static int copy_paths_impl(cpprob_hip_ctx* c, void* h, size_t n_bytes);
int cpprob_hip_copy_paths(cpprob_hip_ctx* c, void* h, size_t n_bytes)
{
    return lane_read(c, [&](cpprob_hip_ctx* l) { return copy_paths_impl(l, h, n_bytes); });
}
static int copy_paths_impl(cpprob_hip_ctx* c, void* h, size_t n_bytes)
{
    if (!c || !h) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!c->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished run");
    if (int rc = settle_fixed(c)) return rc;
    if (!c->keep) return fail(c, CPPROB_HIP_ESTATE, "the run kept no history (keep_history = 0): traces and ancestors do not exist; its statistics are the filtering ones");
    const size_t vsz = c->is_int ? sizeof(int32_t) : sizeof(double);
    // SIS: every trace is its own line -- the paths are the values (and a fused-read-out run keeps no linear weights to re-run the read-out on)
    if (c->cfg.algorithm == CPPROB_HIP_ALG_SIS) return copy_values_impl(c, h, n_bytes);
    if (!c->d_paths) HIP_TRY(c, hipMalloc(&c->d_paths, (size_t)c->cap_T * c->cap_particles * vsz));
    dispatch_model(c, [&](auto m) { launch_smooth<decltype(m)>(c, true); });
    HIP_TRY(c, hipGetLastError());
    return copy_rows(c, h, c->d_paths, vsz, (size_t)c->T, n_bytes, (size_t)c->ld);
}

// ---- building blocks ----------------------------------------------------------------------

#define BB_PRELUDE(c)                                                         \
    if (!(c)) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");         \
    HIP_TRY(c, hipSetDevice((c)->device));

int cpprob_hip_philox_blocks(cpprob_hip_ctx* c, uint64_t seed, uint64_t pid0, uint64_t draw, size_t n, uint32_t* d_out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (n == 0) return 0;
    hipLaunchKernelGGL(philox_blocks_kernel, GRID1(n), seed, pid0, draw, (int64_t)n, d_out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_draw_normal(cpprob_hip_ctx* c, uint64_t seed, uint64_t pid0, uint64_t draw, double mean, double sigma, size_t n, double* d_out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (n == 0) return 0;
    hipLaunchKernelGGL(draw_normal_kernel, GRID1(n), seed, pid0, draw, mean, sigma, (int64_t)n, d_out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_draw_uniform_smallint(cpprob_hip_ctx* c, uint64_t seed, uint64_t pid0, uint64_t draw, int64_t a, int64_t b, size_t n, int32_t* d_out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (b < a) return fail(c, CPPROB_HIP_EINVAL, "uniform_smallint needs a <= b");
    if (a < INT32_MIN || b > INT32_MAX) return fail(c, CPPROB_HIP_EINVAL, "uniform_smallint writes int32: a and b must fit");
    if (n == 0) return 0;
    hipLaunchKernelGGL(draw_smallint_kernel, GRID1(n), seed, pid0, draw, a, b, (int64_t)n, d_out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

// what cpprob_hip_set_hmm asks of a transition row: the generator divides by the total
static int check_weights(cpprob_hip_ctx* c, const double* w, int32_t k)
{
    double tot = 0.0;
    for (int i = 0; i < k; ++i) { if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return fail(c, CPPROB_HIP_EINVAL, "discrete: weights must be finite and >= 0"); tot += w[i]; }
    if (!(tot > 0.0) || !std::isfinite(tot)) return fail(c, CPPROB_HIP_EINVAL, "discrete: the weights' total must be positive and finite");
    return 0;
}

static int make_dw(cpprob_hip_ctx* c, const double* w, int32_t k, DiscreteW& dw)
{
    if (!w || k < 1 || k > 8) return fail(c, CPPROB_HIP_EINVAL, "discrete: need 1 <= k <= 8 weights");
    if (int rc = check_weights(c, w, k)) return rc;
    std::memset(&dw, 0, sizeof dw);
    for (int i = 0; i < k; ++i) dw.w[i] = w[i];
    dw.k = k;
    return 0;
}

int cpprob_hip_draw_discrete(cpprob_hip_ctx* c, uint64_t seed, uint64_t pid0, uint64_t draw, const double* h_w, int32_t k, size_t n, int32_t* d_out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    DiscreteW dw;
    if (int rc = make_dw(c, h_w, k, dw)) return rc;
    if (n == 0) return 0;
    hipLaunchKernelGGL(draw_discrete_kernel, GRID1(n), seed, pid0, draw, dw, (int64_t)n, d_out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_draw_uniform_real(cpprob_hip_ctx* c, uint64_t seed, uint64_t pid0, uint64_t draw, double a, double b, size_t n, double* d_out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (n == 0) return 0;
    hipLaunchKernelGGL(draw_uniform_real_kernel, GRID1(n), seed, pid0, draw, a, b, (int64_t)n, d_out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_draw_poisson(cpprob_hip_ctx* c, uint64_t seed, uint64_t pid0, uint64_t draw, double mean, size_t n, int32_t* d_out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!(mean >= 0.0 && mean <= CPPROB_HIP_POISSON_MAX_MEAN)) return fail(c, CPPROB_HIP_EINVAL, "poisson needs 0 <= mean <= CPPROB_HIP_POISSON_MAX_MEAN");
    if (n == 0) return 0;
    hipLaunchKernelGGL(draw_poisson_kernel, GRID1(n), seed, pid0, draw, mean, (int64_t)n, d_out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_logpdf_normal(cpprob_hip_ctx* c, const double* x, const double* mean, const double* sigma, size_t n, double* out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (n == 0) return 0;
    hipLaunchKernelGGL(logpdf_normal_kernel, GRID1(n), x, mean, sigma, (int64_t)n, out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_logpdf_uniform_real(cpprob_hip_ctx* c, const double* x, const double* a, const double* b, size_t n, double* out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (n == 0) return 0;
    hipLaunchKernelGGL(logpdf_uniform_real_kernel, GRID1(n), x, a, b, (int64_t)n, out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_logpdf_poisson(cpprob_hip_ctx* c, const int32_t* x, const double* mean, size_t n, double* out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (n == 0) return 0;
    hipLaunchKernelGGL(logpdf_poisson_kernel, GRID1(n), x, mean, (int64_t)n, out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_logpdf_uniform_smallint(cpprob_hip_ctx* c, const int32_t* x, int64_t a, int64_t b, size_t n, double* out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (n == 0) return 0;
    hipLaunchKernelGGL(logpdf_smallint_kernel, GRID1(n), x, a, b, (int64_t)n, out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_logpdf_discrete(cpprob_hip_ctx* c, const int32_t* x, const double* h_w, int32_t k, size_t n, double* out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    DiscreteW dw;
    if (int rc = make_dw(c, h_w, k, dw)) return rc;
    if (n == 0) return 0;
    hipLaunchKernelGGL(logpdf_discrete_kernel, GRID1(n), x, dw, (int64_t)n, out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

}  // extern "C"
namespace {
// the fixed-point weight of a log-weight x against the reference 0, as a double (cpprob/detail/fixed_mass.hpp: fix_weight)
__global__ void fix_weight_kernel(const double* __restrict__ x, int64_t n, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (double)fix_weight(x[i], 0.0);
}
}  // namespace
extern "C" {
int cpprob_hip_fastmath(cpprob_hip_ctx* c, int32_t which, const double* d_x, size_t n, double* d_out0, double* d_out1)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (which < 0 || which > 3) return fail(c, CPPROB_HIP_EINVAL, "which: 0 log01, 1 sincospi02, 2 exp_nonpos, 3 fix_weight");
    if (!d_x || !d_out0 || (which == 1 && !d_out1)) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (n == 0) return 0;
    if (which == 3) hipLaunchKernelGGL(fix_weight_kernel, GRID1(n), d_x, (int64_t)n, d_out0);
    else hipLaunchKernelGGL(fastmath_kernel, GRID1(n), (int)which, d_x, (int64_t)n, d_out0, d_out1);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

static_assert(CPPROB_HIP_POISSON_MAX_MEAN == kPoissonMaxMean, "the header documents the generator's limit");
int cpprob_hip_variate_from_bits(cpprob_hip_ctx* c, int32_t which, const double* h_params, int32_t n_params, const uint32_t* d_blocks, size_t n,
                                 double* d_out0, double* d_out1)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    static const int32_t want[5] = {2, 0, 2, 1, 0};    // parameters per generator (discrete: 1 .. 8 weights)
    if (which < 0 || which > CPPROB_HIP_VARIATE_NORMAL) return fail(c, CPPROB_HIP_EINVAL, "which: 0 uniform_smallint, 1 discrete, 2 uniform_real, 3 poisson, 4 normal");
    if (which == CPPROB_HIP_VARIATE_DISCRETE ? (n_params < 1 || n_params > 8) : n_params != want[which]) return fail(c, CPPROB_HIP_EINVAL, "wrong number of parameters");
    if ((n_params && !h_params) || !d_blocks || !d_out0 || (which == CPPROB_HIP_VARIATE_NORMAL && !d_out1)) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    VariateParams vp;
    std::memset(&vp, 0, sizeof vp);
    for (int i = 0; i < n_params; ++i) vp.p[i] = h_params[i];
    vp.k = n_params;
    if (which == CPPROB_HIP_VARIATE_SMALLINT) {
        const double a = vp.p[0], b = vp.p[1];
        if (!(std::fabs(a) <= 0x1p53 && std::fabs(b) <= 0x1p53) || a != std::floor(a) || b != std::floor(b) || b < a || b - a > 4294967295.0)
            return fail(c, CPPROB_HIP_EINVAL, "uniform_smallint needs integers a <= b with b - a < 2^32");
    }
    else if (which == CPPROB_HIP_VARIATE_DISCRETE) { if (int rc = check_weights(c, vp.p, n_params)) return rc; }
    else if (which == CPPROB_HIP_VARIATE_POISSON && !(vp.p[0] >= 0.0 && vp.p[0] <= CPPROB_HIP_POISSON_MAX_MEAN))
        return fail(c, CPPROB_HIP_EINVAL, "poisson needs 0 <= mean <= CPPROB_HIP_POISSON_MAX_MEAN");
    if (n == 0) return 0;
    hipLaunchKernelGGL(variate_from_bits_kernel, GRID1(n), (int)which, vp, d_blocks, (int64_t)n, d_out0, d_out1);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_logsumexp_ess(cpprob_hip_ctx* c, const double* d_logw, size_t n, double* h_out3)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!d_logw || !h_out3) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (n == 0) { h_out3[0] = 0; h_out3[1] = 0; h_out3[2] = 0; return 0; }   // empty: value-initialised (empirical_distribution.hpp:131-133)
    if (int rc = bb_normalise(c, d_logw, n, (double)n)) return rc;
    StepCtrl h{};
    HIP_TRY(c, hipMemcpyAsync(&h, c->d_bb_ctrl, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    h_out3[0] = h.M; h_out3[1] = h.M + std::log(h.W); h_out3[2] = h.ess;
    return 0;
}

}  // extern "C"
template <class Col>
static int column_stats(cpprob_hip_ctx* c, const typename Col::value_t* d_x, const double* d_logw, size_t n, double* h_raw, double* h_lse_ess)
{
    using V = typename Col::value_t;
    if (int rc = bb_normalise(c, d_logw, n, (double)n)) return rc;
    const int nb = (int)((n + kTile - 1) / kTile);
    const int64_t ld = (int64_t)nb * kTile;
    V* col = static_cast<V*>(c->d_bb_col);
    hipLaunchKernelGGL(pad_copy_kernel<V>, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, c->stream, d_x, (int64_t)n, ld, col);
    SmoothArgs<Col> a{};
    a.values = col; a.anc = nullptr; a.wrel = c->d_bb_wrel; a.bf = c->d_bb_bf; a.ctrl = c->d_bb_ctrl; a.resampled = nullptr; a.T = 1; a.n = (int64_t)n; a.ld = ld; a.rs = ld;
    a.identity = 1; a.stats_part = c->d_bb_stats_part; a.paths = nullptr;
    const int grid = std::min(nb, 2048);
    hipLaunchKernelGGL(smooth_kernel<Col>, dim3(grid), dim3(kThreads), (size_t)kWaves * Col::kStats * sizeof(double), c->stream, a);
    // is_int = 1 -> plain normalised sums
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(kThreads), 0, c->stream, c->d_bb_stats_part, grid, 1, Col::kStats, 1, c->d_bb_ctrl, c->d_bb_stats, 1);
    HIP_TRY(c, hipGetLastError());
    StepCtrl h{};
    HIP_TRY(c, hipMemcpyAsync(&h, c->d_bb_ctrl, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(h_raw, c->d_bb_stats, Col::kStats * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    h_lse_ess[0] = h.M + std::log(h.W); h_lse_ess[1] = h.ess;
    return 0;
}
// The same for `n_cols` columns against ONE log-weight array: one normalisation, the columns as the rows of a T = n_cols "trace" (the
// read-out kernel with identity ancestors), one finalize, one copy -- five launches and one synchronisation, whatever the number of
// predict hits (the per-column form costs six launches and a synchronisation each: 0.75 ms for the 16 hits of hmm<16>).
template <class Col>
static int columns_stats(cpprob_hip_ctx* c, const typename Col::value_t* d_x, size_t n_cols, size_t col_stride, const double* d_logw, size_t n, double* h_raw /*[n_cols][kStats]*/,
                         double* h_lse_ess)
{
    using V = typename Col::value_t;
    constexpr size_t kChunk = 64;                                  // columns per launch: LDS of the read-out = 4 waves x columns x kStats doubles
    if (int rc = bb_normalise(c, d_logw, n, (double)n)) return rc;
    const int nb = (int)((n + kTile - 1) / kTile);
    const int64_t ld = (int64_t)nb * kTile;
    const int grid = std::min(nb, 2048);
    const size_t chunk = std::min(n_cols, kChunk);
    // columns that already sit a whole number of tiles apart are read where they lie (the caller keeps the slots behind n finite: they weigh
    // nothing); others are copied into tile-padded scratch first (80 MB each way for one column of 10^7 doubles: 40 us of a 0.2 ms run)
    const bool in_place = col_stride % (size_t)kTile == 0 && col_stride >= (size_t)ld;
    const size_t col_bytes = in_place ? 0 : chunk * (size_t)ld * sizeof(V), part_doubles = chunk * Col::kStats * (size_t)grid, stat_doubles = chunk * Col::kStats;
    if (col_bytes > c->bb_cols_bytes) { dfree(c->d_bb_cols); HIP_TRY(c, hipMalloc(&c->d_bb_cols, col_bytes)); c->bb_cols_bytes = col_bytes; }
    if (part_doubles > c->bb_cols_part) { dfree(c->d_bb_cols_part); HIP_TRY(c, hipMalloc(&c->d_bb_cols_part, part_doubles * sizeof(double))); c->bb_cols_part = part_doubles; }
    if (stat_doubles > c->bb_cols_stat) { dfree(c->d_bb_cols_stat); HIP_TRY(c, hipMalloc(&c->d_bb_cols_stat, stat_doubles * sizeof(double))); c->bb_cols_stat = stat_doubles; }
    const size_t stats_bytes = n_cols * Col::kStats * sizeof(double), ride_off = (stats_bytes + sizeof(StepCtrl) + 15) / 16 * 16;
    if (int rc = pin_reserve(c, ride_off + c->ride_bytes)) return rc;
    for (size_t k0 = 0; k0 < n_cols; k0 += chunk) {
        const size_t nk = std::min(chunk, n_cols - k0);
        const V* cols = d_x + k0 * col_stride;
        const int64_t rs = in_place ? (int64_t)col_stride : ld;
        if (!in_place) {
            V* pad = static_cast<V*>(c->d_bb_cols);
            hipLaunchKernelGGL(pad_copy_cols_kernel<V>, dim3((unsigned)((ld + 255) / 256), (unsigned)nk), dim3(256), 0, c->stream, d_x + k0 * col_stride, (int64_t)n, (int64_t)col_stride, ld, pad);
            cols = pad;
        }
        SmoothArgs<Col> a{};
        a.values = const_cast<V*>(cols); a.anc = nullptr; a.wrel = c->d_bb_wrel; a.bf = c->d_bb_bf; a.ctrl = c->d_bb_ctrl; a.resampled = nullptr; a.T = (int)nk; a.n = (int64_t)n; a.ld = rs; a.rs = rs;
        a.identity = 1; a.stats_part = c->d_bb_cols_part; a.paths = nullptr;
        hipLaunchKernelGGL(smooth_kernel<Col>, dim3(grid), dim3(kThreads), (size_t)kWaves * nk * Col::kStats * sizeof(double), c->stream, a);
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)nk), dim3(kThreads), 0, c->stream, c->d_bb_cols_part, grid, (int)nk, Col::kStats, 1, c->d_bb_ctrl, c->d_bb_cols_stat, 1);
        HIP_TRY(c, hipGetLastError());
        // (results through ONE short launch into pinned memory, the caller's riding read-back with the last chunk's: see lineage_stats)
        PinPack pk;
        pk.add(c->d_bb_cols_stat, pin_data(c) + k0 * Col::kStats * sizeof(double), nk * Col::kStats * sizeof(double));
        if (k0 + chunk >= n_cols) {
            pk.add(c->d_bb_ctrl, pin_data(c) + stats_bytes, sizeof(StepCtrl));
            pk.add(c->ride_src, pin_data(c) + ride_off, c->ride_bytes);
        }
        if (int rc = pk.launch(c)) return rc;
        if (k0 + chunk < n_cols) HIP_TRY(c, hipStreamSynchronize(c->stream));     // (the scratch is reused by the next chunk)
    }
    const bool riding = c->ride_bytes != 0;
    if (int rc = pin_wait(c)) return rc;
    StepCtrl h;
    std::memcpy(h_raw, pin_data(c), stats_bytes);
    std::memcpy(&h, pin_data(c) + stats_bytes, sizeof h);
    if (riding) { std::memcpy(c->ride_dst, pin_data(c) + ride_off, c->ride_bytes); c->ride_src = nullptr; c->ride_dst = nullptr; c->ride_bytes = 0; }
    h_lse_ess[0] = h.M + std::log(h.W); h_lse_ess[1] = h.ess;
    return 0;
}
// first_row[t] .. first_row[t + 1]: the records made in generation t's slots (h_gen[h] = the generation of record h, non-decreasing)
static int upload_first_rows(cpprob_hip_ctx* c, const int32_t* h_gen, int32_t H, int32_t T)
{
    std::vector<int32_t> first((size_t)T + 1, 0);
    int32_t prev = 0;
    for (int32_t h = 0; h < H; ++h) {
        if (h_gen[h] < prev || h_gen[h] >= T) return fail(c, CPPROB_HIP_EINVAL, "h_gen must be non-decreasing and < T");
        prev = h_gen[h];
        first[(size_t)h_gen[h] + 1] += 1;
    }
    for (int t = 0; t < T; ++t) first[(size_t)t + 1] += first[(size_t)t];
    if (first == c->bb_first_host) return 0;
    c->bb_first_host.clear();
    if (first.size() > c->bb_first_cap) { dfree(c->d_bb_first); HIP_TRY(c, hipMalloc(&c->d_bb_first, first.size() * sizeof(int32_t))); c->bb_first_cap = first.size(); }
    HIP_TRY(c, hipStreamSynchronize(c->stream));                                                                       // (a launch in flight may still read the old table)
    HIP_TRY(c, hipMemcpy(c->d_bb_first, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice));     // (synchronous: `first` is a local)
    c->bb_first_host = first;
    return 0;
}

// statistics of per-step records along the final particles' lineages against the final weights (lineage_stats_kernel)
template <class Col>
static int lineage_stats(cpprob_hip_ctx* c, const int32_t* d_anc, const int32_t* d_resampled, int32_t T, size_t n, const typename Col::value_t* d_cols, const int32_t* h_gen,
                         int32_t H, const double* d_logw, double* h_raw /*[H][kStats]*/, double* h_lse_ess)
{
    constexpr int kChunk = 64;
    if (int rc = upload_first_rows(c, h_gen, H, T)) return rc;
    if (int rc = bb_normalise(c, d_logw, n, (double)n)) return rc;
    const int nb = (int)((n + kTile - 1) / kTile);
    const int grid = std::min(nb, 2048);
    const int chunk = std::min<int>(H, kChunk);
    const size_t part_doubles = (size_t)chunk * Col::kStats * (size_t)grid, stat_doubles = (size_t)chunk * Col::kStats;
    if (part_doubles > c->bb_cols_part) { dfree(c->d_bb_cols_part); HIP_TRY(c, hipMalloc(&c->d_bb_cols_part, part_doubles * sizeof(double))); c->bb_cols_part = part_doubles; }
    if (stat_doubles > c->bb_cols_stat) { dfree(c->d_bb_cols_stat); HIP_TRY(c, hipMalloc(&c->d_bb_cols_stat, stat_doubles * sizeof(double))); c->bb_cols_stat = stat_doubles; }
    const size_t stats_bytes = (size_t)H * Col::kStats * sizeof(double), ride_off = (stats_bytes + sizeof(StepCtrl) + 15) / 16 * 16;
    if (int rc = pin_reserve(c, ride_off + c->ride_bytes)) return rc;
    for (int h0 = 0; h0 < H; h0 += chunk) {
        const int nk = std::min(chunk, H - h0);
        LineageStatsArgs<Col> a{};
        a.anc = d_anc; a.resampled = d_resampled; a.T = T; a.n = (int64_t)n; a.cols = d_cols; a.first_row = c->d_bb_first; a.h0 = h0; a.h1 = h0 + nk;
        a.wrel = c->d_bb_wrel; a.bf = c->d_bb_bf; a.ctrl = c->d_bb_ctrl; a.stats_part = c->d_bb_cols_part;
        hipLaunchKernelGGL(lineage_stats_kernel<Col>, dim3(grid), dim3(kThreads), (size_t)kWaves * nk * Col::kStats * sizeof(double), c->stream, a);
        hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)nk), dim3(kThreads), 0, c->stream, c->d_bb_cols_part, grid, nk, Col::kStats, 1, c->d_bb_ctrl, c->d_bb_cols_stat, 1);
        HIP_TRY(c, hipGetLastError());
        PinPack pk;
        pk.add(c->d_bb_cols_stat, pin_data(c) + (size_t)h0 * Col::kStats * sizeof(double), (size_t)nk * Col::kStats * sizeof(double));
        if (h0 + chunk >= H) {                                              // (the last chunk's launch carries the rest)
            pk.add(c->d_bb_ctrl, pin_data(c) + stats_bytes, sizeof(StepCtrl));
            pk.add(c->ride_src, pin_data(c) + ride_off, c->ride_bytes);
        }
        if (int rc = pk.launch(c)) return rc;
        if (h0 + chunk < H) HIP_TRY(c, hipStreamSynchronize(c->stream));     // (the scratch is reused by the next chunk)
    }
    const bool riding = c->ride_bytes != 0;
    if (int rc = pin_wait(c)) return rc;
    StepCtrl h;
    std::memcpy(h_raw, pin_data(c), stats_bytes);
    std::memcpy(&h, pin_data(c) + stats_bytes, sizeof h);
    if (riding) { std::memcpy(c->ride_dst, pin_data(c) + ride_off, c->ride_bytes); c->ride_src = nullptr; c->ride_dst = nullptr; c->ride_bytes = 0; }
    h_lse_ess[0] = h.M + std::log(h.W); h_lse_ess[1] = h.ess;
    return 0;
}

// A read-back armed by cpprob_hip_readback_with_next_result rides the NEXT statistics call and no other: whatever way that call ends
// (bad arguments, a failed allocation, a device error), the caller's destination pointer does not outlive it in the context.
struct RideDisarm {
    cpprob_hip_ctx* c;
    ~RideDisarm() { if (c) { c->ride_src = nullptr; c->ride_dst = nullptr; c->ride_bytes = 0; } }
};

static int lineage_args_ok(cpprob_hip_ctx* c, const void* d_anc, const void* d_resampled, int32_t T, size_t n, const void* d_cols, const int32_t* h_gen, int32_t H,
                           const void* d_logw, const void* h_out)
{
    if (!d_anc || !d_resampled || !d_cols || !h_gen || !d_logw || !h_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (T < 1 || H < 1 || n == 0) return fail(c, CPPROB_HIP_EINVAL, "need T >= 1, H >= 1 and a non-empty population");
    if (n > (size_t)INT32_MAX - kTile) return fail(c, CPPROB_HIP_EINVAL, "population too large for int32 ancestors");
    return 0;
}

extern "C" {

int cpprob_hip_readback_with_next_result(cpprob_hip_ctx* c, const void* d_src, void* h_dst, size_t bytes)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (bytes != 0 && (!d_src || !h_dst)) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (bytes > ((size_t)1 << 20) || (bytes & 3)) return fail(c, CPPROB_HIP_EINVAL, "a read-back that rides a result's is a small one (<= 1 MiB, whole 4-byte words)");
    c->ride_src = bytes ? d_src : nullptr; c->ride_dst = bytes ? h_dst : nullptr; c->ride_bytes = bytes;
    return 0;
}

int cpprob_hip_lineage_prepare(cpprob_hip_ctx* c, const int32_t* h_gen, int32_t H, int32_t T)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!h_gen || T < 1 || H < 1) return fail(c, CPPROB_HIP_EINVAL, "need h_gen, T >= 1 and H >= 1");
    return upload_first_rows(c, h_gen, H, T);
}

int cpprob_hip_lineage_moments(cpprob_hip_ctx* c, const int32_t* d_anc, const int32_t* d_resampled, int32_t T, size_t n, const double* d_cols, const int32_t* h_gen, int32_t H,
                               const double* d_logw, double* h_out4)
{
    LANES_OWN(c);
    RideDisarm ride_guard{c};
    BB_PRELUDE(c);
    if (int rc = lineage_args_ok(c, d_anc, d_resampled, T, n, d_cols, h_gen, H, d_logw, h_out4)) return rc;
    std::vector<double> raw((size_t)H * 2);
    double le[2];
    if (int rc = lineage_stats<ColumnReal>(c, d_anc, d_resampled, T, n, d_cols, h_gen, H, d_logw, raw.data(), le)) return rc;
    for (int32_t k = 0; k < H; ++k) {
        h_out4[4 * k] = raw[2 * k];
        h_out4[4 * k + 1] = raw[2 * k + 1] - raw[2 * k] * raw[2 * k];     // variance(mean) = raw_moment(2) - mean*mean  (stats_printer.hpp:78-81)
        h_out4[4 * k + 2] = le[0]; h_out4[4 * k + 3] = le[1];
    }
    return 0;
}

int cpprob_hip_lineage_hist(cpprob_hip_ctx* c, const int32_t* d_anc, const int32_t* d_resampled, int32_t T, size_t n, const int32_t* d_cols, const int32_t* h_gen, int32_t H,
                            const double* d_logw, int32_t k, double* h_out, double* h_lse_ess)
{
    LANES_OWN(c);
    RideDisarm ride_guard{c};
    BB_PRELUDE(c);
    if (int rc = lineage_args_ok(c, d_anc, d_resampled, T, n, d_cols, h_gen, H, d_logw, h_out)) return rc;
    if (k < 1 || k > 8) return fail(c, CPPROB_HIP_EINVAL, "need 1 <= k <= 8");
    std::vector<double> raw((size_t)H * 8);
    double le[2];
    if (int rc = lineage_stats<ColumnInt8>(c, d_anc, d_resampled, T, n, d_cols, h_gen, H, d_logw, raw.data(), le)) return rc;
    for (int32_t j = 0; j < H; ++j)
        for (int s2 = 0; s2 < k; ++s2) h_out[(size_t)j * (size_t)k + s2] = raw[(size_t)j * 8 + s2];
    if (h_lse_ess) { h_lse_ess[0] = le[0]; h_lse_ess[1] = le[1]; }
    return 0;
}

int cpprob_hip_weighted_moments_columns(cpprob_hip_ctx* c, const double* d_x, size_t n_cols, size_t col_stride, const double* d_logw, size_t n, double* h_out4)
{
    LANES_OWN(c);
    RideDisarm ride_guard{c};
    BB_PRELUDE(c);
    if (!d_x || !d_logw || !h_out4) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (n == 0 || n_cols == 0 || col_stride < n) return fail(c, CPPROB_HIP_EINVAL, "empty distribution / columns closer than their length");
    std::vector<double> raw(n_cols * 2);
    double le[2];
    if (int rc = columns_stats<ColumnReal>(c, d_x, n_cols, col_stride, d_logw, n, raw.data(), le)) return rc;
    for (size_t k = 0; k < n_cols; ++k) {
        h_out4[4 * k] = raw[2 * k];
        h_out4[4 * k + 1] = raw[2 * k + 1] - raw[2 * k] * raw[2 * k];     // variance(mean) = raw_moment(2) - mean*mean  (:78-81)
        h_out4[4 * k + 2] = le[0]; h_out4[4 * k + 3] = le[1];
    }
    return 0;
}

int cpprob_hip_weighted_hist_columns(cpprob_hip_ctx* c, const int32_t* d_x, size_t n_cols, size_t col_stride, const double* d_logw, size_t n, int32_t k, double* h_out,
                                     double* h_lse_ess)
{
    LANES_OWN(c);
    RideDisarm ride_guard{c};
    BB_PRELUDE(c);
    if (!d_x || !d_logw || !h_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (k < 1 || k > 8) return fail(c, CPPROB_HIP_EINVAL, "need 1 <= k <= 8");
    if (n == 0 || n_cols == 0 || col_stride < n) return fail(c, CPPROB_HIP_EINVAL, "empty distribution / columns closer than their length");
    std::vector<double> raw(n_cols * 8);
    double le[2];
    if (int rc = columns_stats<ColumnInt8>(c, d_x, n_cols, col_stride, d_logw, n, raw.data(), le)) return rc;
    for (size_t j = 0; j < n_cols; ++j)
        for (int s2 = 0; s2 < k; ++s2) h_out[j * (size_t)k + s2] = raw[j * 8 + s2];
    if (h_lse_ess) { h_lse_ess[0] = le[0]; h_lse_ess[1] = le[1]; }
    return 0;
}

int cpprob_hip_weighted_moments(cpprob_hip_ctx* c, const double* d_x, const double* d_logw, size_t n, double* h_out4)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!d_x || !d_logw || !h_out4) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (n == 0) return fail(c, CPPROB_HIP_EINVAL, "empty distribution");
    double raw[2], le[2];
    if (int rc = column_stats<ColumnReal>(c, d_x, d_logw, n, raw, le)) return rc;
    h_out4[0] = raw[0];
    h_out4[1] = raw[1] - raw[0] * raw[0];     // variance(mean) = raw_moment(2) - mean*mean  (:78-81)
    h_out4[2] = le[0]; h_out4[3] = le[1];
    return 0;
}

int cpprob_hip_weighted_hist(cpprob_hip_ctx* c, const int32_t* d_x, const double* d_logw, size_t n, int32_t k, double* h_out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!d_x || !d_logw || !h_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (k < 1 || k > 8) return fail(c, CPPROB_HIP_EINVAL, "need 1 <= k <= 8");
    if (n == 0) return fail(c, CPPROB_HIP_EINVAL, "empty distribution");
    double raw[8], le[2];
    if (int rc = column_stats<ColumnInt8>(c, d_x, d_logw, n, raw, le)) return rc;
    for (int s = 0; s < k; ++s) h_out[s] = raw[s];
    return 0;
}

int cpprob_hip_resample(cpprob_hip_ctx* c, int32_t kind, const double* d_logw, size_t n_in, uint64_t seed, uint64_t step, uint64_t j0, size_t n_out,
                        uint64_t n_total_out, int32_t* d_anc)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!d_logw || !d_anc) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (n_in == 0) return fail(c, CPPROB_HIP_EINVAL, "cannot resample an empty population");
    if (n_in > (size_t)INT32_MAX - kTile) return fail(c, CPPROB_HIP_EINVAL, "population too large for int32 ancestors");
    if (n_total_out == 0 || j0 + n_out > n_total_out) return fail(c, CPPROB_HIP_EINVAL, "output range outside [0, n_total_out)");
    if (n_out == 0) return 0;
    if (int rc = bb_normalise(c, d_logw, n_in, (double)n_in)) return rc;
    const int nb_in = (int)((n_in + kTile - 1) / kTile);
    if (kind == CPPROB_HIP_RESAMPLE_MULTINOMIAL) {
        if ((size_t)nb_in * kTile > c->bb_cdf_cap) { dfree(c->d_bb_cdf); HIP_TRY(c, hipMalloc(&c->d_bb_cdf, (size_t)nb_in * kTile * sizeof(double))); c->bb_cdf_cap = (size_t)nb_in * kTile; }
        hipLaunchKernelGGL(cdf_kernel, dim3(nb_in), dim3(kThreads), 0, c->stream, c->d_bb_wrel, c->d_bb_bc, c->d_bb_bf, c->d_bb_ctrl, c->d_bb_cdf);
        hipLaunchKernelGGL(multinomial_kernel, GRID1(n_out), c->d_bb_cdf, (int64_t)n_in, c->d_bb_ctrl, seed, step, j0, (int64_t)n_out, (int64_t)n_out, d_anc, 0);
    } else if (kind == CPPROB_HIP_RESAMPLE_SYSTEMATIC || kind == CPPROB_HIP_RESAMPLE_STRATIFIED) {
        ResampleArgs a{};
        a.wrel = c->d_bb_wrel; a.n_in = (int64_t)n_in; a.bc = c->d_bb_bc; a.bf = c->d_bb_bf; a.nb = nb_in; a.ctrl = c->d_bb_ctrl; a.seed = seed; a.step = step; a.j0 = j0;
        a.n_total_out = n_total_out; a.n_out = (int64_t)n_out; a.anc = d_anc;
        const int nb_out = (int)((n_out + kTile - 1) / kTile);
        ProfScope ps(c, 5);
        if (kind == CPPROB_HIP_RESAMPLE_SYSTEMATIC) hipLaunchKernelGGL(resample_kernel<RS_SYSTEMATIC>, dim3(nb_out), dim3(kThreads), 0, c->stream, a);
        else hipLaunchKernelGGL(resample_kernel<RS_STRATIFIED>, dim3(nb_out), dim3(kThreads), 0, c->stream, a);
    } else {
        return fail(c, CPPROB_HIP_EINVAL, "unknown resampler");
    }
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_smc_bookkeep(cpprob_hip_ctx* c, int32_t kind, const double* d_logw, size_t n, uint64_t seed, int32_t step, int32_t last, double ess_frac,
                            double* d_ess, int32_t* d_resampled, double* d_log_z, int32_t* d_anc)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!d_logw || !d_ess || !d_resampled || !d_log_z || !d_anc) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (n == 0 || n > (size_t)INT32_MAX - kTile) return fail(c, CPPROB_HIP_EINVAL, "population size out of range");
    if (kind < CPPROB_HIP_RESAMPLE_SYSTEMATIC || kind > CPPROB_HIP_RESAMPLE_MULTINOMIAL) return fail(c, CPPROB_HIP_EINVAL, "unknown resampler");
    if (step < 0) return fail(c, CPPROB_HIP_EINVAL, "step out of range");
    if (int rc = ensure_bb(c, n)) return rc;
    const int nb = (int)((n + kTile - 1) / kTile);
    hipLaunchKernelGGL(weights_partials_kernel, dim3(nb), dim3(kThreads), 0, c->stream, d_logw, (int64_t)n, c->d_bb_part, c->d_bb_wrel);
    ScanArgs sa{};
    sa.part = c->d_bb_part; sa.nb = nb; sa.bc = c->d_bb_bc; sa.bf = c->d_bb_bf; sa.ctrl = c->d_bb_ctrl; sa.t = step; sa.T = last ? step + 1 : step + 2;
    sa.n_pop = (double)n; sa.n_local = (double)n; sa.ess_frac = ess_frac; sa.force_no_resample = 0; sa.phase = 0; sa.seed = seed;
    sa.ess_trace = d_ess; sa.resampled = d_resampled; sa.log_z_out = d_log_z;
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, c->stream, sa);
    if (!last) {
        if (kind == CPPROB_HIP_RESAMPLE_MULTINOMIAL) {
            if ((size_t)nb * kTile > c->bb_cdf_cap) { dfree(c->d_bb_cdf); HIP_TRY(c, hipMalloc(&c->d_bb_cdf, (size_t)nb * kTile * sizeof(double))); c->bb_cdf_cap = (size_t)nb * kTile; }
            hipLaunchKernelGGL(cdf_kernel, dim3(nb), dim3(kThreads), 0, c->stream, c->d_bb_wrel, c->d_bb_bc, c->d_bb_bf, c->d_bb_ctrl, c->d_bb_cdf);
            hipLaunchKernelGGL(multinomial_kernel, GRID1(n), c->d_bb_cdf, (int64_t)n, c->d_bb_ctrl, seed, (uint64_t)step + 1, (uint64_t)0, (int64_t)n, (int64_t)n, d_anc, 1);
        } else {
            ResampleArgs a{};
            a.wrel = c->d_bb_wrel; a.n_in = (int64_t)n; a.bc = c->d_bb_bc; a.bf = c->d_bb_bf; a.nb = nb; a.ctrl = c->d_bb_ctrl; a.seed = seed; a.step = (uint64_t)step + 1;
            a.j0 = 0; a.n_total_out = n; a.n_out = (int64_t)n; a.anc = d_anc; a.run_ctrl = 1; a.identity_unless_resampling = 1;
            if (kind == CPPROB_HIP_RESAMPLE_SYSTEMATIC) hipLaunchKernelGGL(resample_kernel<RS_SYSTEMATIC>, dim3(nb), dim3(kThreads), 0, c->stream, a);
            else hipLaunchKernelGGL(resample_kernel<RS_STRATIFIED>, dim3(nb), dim3(kThreads), 0, c->stream, a);
        }
    }
    HIP_TRY(c, hipGetLastError());
    return 0;
}

}  // extern "C"
namespace {
// (re)lays the two-copy hierarchy out for populations of nb tiles
int ensure_bbf(cpprob_hip_ctx* c, int nb)
{
    if (nb == c->bbf_nb && c->d_bbf_hier) return 0;
    size_t per_copy = 0, off[kHierMaxLevels] = {0, 0, 0};
    int nl = 0;
    HierTable t{};
    for (size_t e = (size_t)nb;; e = (e + 63) / 64) {
        if (nl >= kHierMaxLevels) return fail(c, CPPROB_HIP_EUNSUPPORTED, "population too large for the three-level mass hierarchy");
        off[nl] = per_copy; t.n_ent[nl] = (int)e; per_copy += e * (nl == 0 ? 1 : kHierStride); ++nl;
        if (e <= 64) break;
    }
    t.n_lev = nl;
    c->bbf_q0_off = per_copy; c->bbf_m0_off = per_copy + (size_t)nb; per_copy += 2 * (size_t)nb;
    if ((size_t)nb > c->bbf_cap_nb || !c->d_bbf_hier) {
        dfree(c->d_bbf_hier); dfree(c->d_bbf_q);
        HIP_TRY(c, hipMalloc(&c->d_bbf_hier, 2 * per_copy * sizeof(uint64_t)));
        HIP_TRY(c, hipMalloc(&c->d_bbf_q, (size_t)nb * kTile * sizeof(uint32_t)));
        c->bbf_cap_nb = (size_t)nb;
    }
    for (int k = 0; k < 3; ++k)
        for (int l = 0; l < nl; ++l) t.lvl[k][l] = c->d_bbf_hier + (size_t)(k & 1) * per_copy + off[l];
    if (!c->d_bbf_table) HIP_TRY(c, hipMalloc(&c->d_bbf_table, sizeof(HierTable)));
    HIP_TRY(c, hipMemcpyAsync(c->d_bbf_table, &t, sizeof t, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_bbf_hier, 0, 2 * per_copy * sizeof(uint64_t), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));               // (t is a local)
    c->bbf_table = t; c->bbf_per_copy = per_copy; c->bbf_nb = nb; c->bbf_phase = 0;
    return 0;
}
void bbf_view(const cpprob_hip_ctx* c, int copy, FHier& f)
{
    const HierTable& t = c->bbf_table;
    for (int l = 0; l < kHierMaxLevels; ++l) { f.h.lvl[l] = l < t.n_lev ? t.lvl[copy][l] : t.lvl[copy][0]; f.h.n_ent[l] = t.n_ent[l]; }
    f.h.n_lev = t.n_lev; f.h.table = c->d_bbf_table; f.h.copy = copy;
    const int top = t.n_lev - 1;
    f.h.top = t.lvl[copy][top]; f.h.top_n = t.n_ent[top]; f.h.top_stride = top == 0 ? 1 : kHierStride;
    f.h.to_next = 0; f.h.to_clear = (int64_t)((copy ^ 1) - copy) * (int64_t)c->bbf_per_copy;
    f.q0 = c->d_bbf_hier + (size_t)copy * c->bbf_per_copy + c->bbf_q0_off;
    f.m0 = c->d_bbf_hier + (size_t)copy * c->bbf_per_copy + c->bbf_m0_off;
}
}  // namespace
extern "C" {

int cpprob_hip_smc_bookkeep_fixed(cpprob_hip_ctx* c, const double* d_logw, size_t n, uint64_t seed, int32_t step, int32_t last, double ess_frac,
                                  double* d_ess, int32_t* d_resampled, double* d_log_z, int32_t* d_anc)
{
    LANES_OWN(c);
    return cpprob_hip_smc_bookkeep_fixed_rs(c, CPPROB_HIP_RESAMPLE_SYSTEMATIC, d_logw, n, seed, step, last, ess_frac, d_ess, d_resampled, d_log_z, d_anc);
}

int cpprob_hip_smc_bookkeep_fixed_rs(cpprob_hip_ctx* c, int32_t kind, const double* d_logw, size_t n, uint64_t seed, int32_t step, int32_t last, double ess_frac,
                                     double* d_ess, int32_t* d_resampled, double* d_log_z, int32_t* d_anc)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (kind < CPPROB_HIP_RESAMPLE_SYSTEMATIC || kind > CPPROB_HIP_RESAMPLE_MULTINOMIAL) return fail(c, CPPROB_HIP_EINVAL, "unknown resampler");
    if (!d_logw || !d_ess || !d_resampled || !d_log_z || (!last && !d_anc)) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (n == 0 || n > (size_t)(1ull << 28)) return fail(c, CPPROB_HIP_EINVAL, "population size out of range (1 .. 2^28: the squares' 64-bit sum)");
    if (step < 0) return fail(c, CPPROB_HIP_EINVAL, "step out of range");
    const int nb = (int)((n + kTile - 1) / kTile);
    if (int rc = ensure_bbf(c, nb)) return rc;
    FHier f{};
    bbf_view(c, c->bbf_phase, f);
    c->bbf_phase ^= 1;
    hipLaunchKernelGGL(bbf_max_kernel, dim3(nb), dim3(kThreads), 0, c->stream, d_logw, (int64_t)n, f);
    hipLaunchKernelGGL(bbf_quantize_kernel, dim3(nb), dim3(kThreads), 0, c->stream, d_logw, (int64_t)n, f, c->d_bbf_q);
    BbfArgs a{};
    a.f = f; a.q = c->d_bbf_q; a.n = (int64_t)n; a.nb = nb; a.u0 = host_resample_u0(seed, (uint64_t)step + 1); a.ess_frac = ess_frac; a.step = step; a.last = last ? 1 : 0;
    a.ess = d_ess; a.resampled = d_resampled; a.log_z = d_log_z; a.anc = d_anc; a.seed = seed;
    if (kind == CPPROB_HIP_RESAMPLE_MULTINOMIAL && !last) {
        // strata form: the counts of this one resampling (they do not depend on the weights: one short launch, two above 64 tiles)
        const int k = strata_levels(nb);
        const size_t words = ((size_t)1 << k) + 1;
        if (words > c->bbf_strata_cap) {
            dfree(c->d_bbf_strata); dfree(c->d_bbf_strata_top);
            HIP_TRY(c, hipMalloc(&c->d_bbf_strata, words * sizeof(uint32_t)));
            HIP_TRY(c, hipMalloc(&c->d_bbf_strata_top, 64 * sizeof(uint32_t)));
            c->bbf_strata_cap = words;
        }
        StrataArgs sa{};
        sa.seed = seed; sa.t0 = step + 1; sa.k = k; sa.n_out = (uint32_t)n; sa.offs = c->d_bbf_strata;
        if (k <= kStrataTop) hipLaunchKernelGGL(multinomial_strata_kernel, dim3(1, 1), dim3(kThreads), 0, c->stream, sa);
        else {
            HIP_TRY(c, hipMemsetAsync(c->d_bbf_strata_top, 0, 64 * sizeof(uint32_t), c->stream));
            sa.top = c->d_bbf_strata_top; sa.top_clear = nullptr;
            hipLaunchKernelGGL(multinomial_strata_top_kernel, dim3(strata_groups(k), 1), dim3(kThreads), 0, c->stream, sa);
            hipLaunchKernelGGL(multinomial_strata_bottom_kernel, dim3(64, 1), dim3(kThreads), 0, c->stream, sa);
        }
        a.strata_offs = c->d_bbf_strata; a.strata_k = k;
    }
    const dim3 grid(last ? 1 : nb);
    if (kind == CPPROB_HIP_RESAMPLE_STRATIFIED) hipLaunchKernelGGL(bbf_ancestors_kernel<kFixStratified>, grid, dim3(kThreads), 0, c->stream, a);
    else if (kind == CPPROB_HIP_RESAMPLE_MULTINOMIAL) hipLaunchKernelGGL(bbf_ancestors_kernel<kFixMultinomial>, grid, dim3(kThreads), 0, c->stream, a);
    else hipLaunchKernelGGL(bbf_ancestors_kernel<kFixSystematic>, grid, dim3(kThreads), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

// ---- the unchanged-model step with the resampling inside the model's launch (include/cpprob_hip.h; cpprob/gpu.hpp) ----
}  // extern "C"
namespace {
struct GenericCtrlBlock { double ref_cur, gap_max; };      // (= cpprob::device::StepCtrl2)

// Exact-reference form of the unchanged-model step: the hierarchy's entries are 256-particle BLOCKS (one per workgroup of the model's
// step kernel); these two passes run a 1024-particle tile per workgroup, so every wavefront owns one block and publishes it itself.
constexpr int kGenBlock = 256;
__global__ __launch_bounds__(kThreads) void generic_max_kernel(const double* __restrict__ logw, int64_t n, FHier f, int n_blocks)
{
    const int64_t j0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPPT;
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < kPPT; ++k) if (j0 + k < n) m = fmax(m, logw[j0 + k]);
    const uint64_t mw = wave_max_u64(dkey(m));
    const int blk = (int)blockIdx.x * kWaves + wave_id();
    if (lane_id() == 0 && blk < n_blocks) bbf_publish_max(f, blk, n_blocks, mw);
}

__global__ __launch_bounds__(kThreads) void generic_quantize_kernel(const double* __restrict__ logw, int64_t n, FHier f, int n_blocks, uint32_t* __restrict__ q, GenericCtrlBlock* ctrl,
                                                                int given, double ref_given)
{
    const double ref = given ? ref_given : bbf_top_max(f);              // (every wavefront: the same <= 64 words)
    if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->ref_cur = ref;
    const int64_t j0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPPT;
    U4 w;
    uint64_t s_l = 0, q_l = 0;
#pragma unroll
    for (int k = 0; k < kPPT; ++k) {
        const uint32_t v = j0 + k < n ? fix_weight(logw[j0 + k], ref) : 0u;
        w[k] = v; s_l += v; q_l += fix_square(v);
    }
    *reinterpret_cast<U4*>(q + j0) = w;
    const uint64_t sw = wave_sum_u64(s_l), qw = wave_sum_u64(q_l);
    const int blk = (int)blockIdx.x * kWaves + wave_id();
    if (lane_id() == 0 && blk < n_blocks) bbf_publish_mass(f, blk, n_blocks, sw, qw);
}

__global__ __launch_bounds__(kWave) void generic_finish_kernel(FHier f, int T, double n_pop, double gap_limit, GenericCtrlBlock* ctrl, double* ess, int32_t* resampled,
                                                               double* log_z, int32_t* flags)
{
    const FTot t = ftot(f);
    if (threadIdx.x != 0) return;
    const FixedDecision d = fixed_decide(t.S, t.Q, n_pop, 0.0, false);
    const double ref = ctrl->ref_cur;
    const double gap = d.W > 0.0 ? ref - t.M : 1e300;
    ctrl->gap_max = T == 1 ? gap : fmax(ctrl->gap_max, gap);
    if (gap < 0.0) *flags = 4;
    else if (gap > gap_limit && *flags == 0) *flags = 5;
    ess[T - 1] = d.ess;
    resampled[T - 1] = 0;
    const double lz = T == 1 ? 0.0 : *log_z;
    *log_z = lz + (ref + log(d.W / n_pop));
}

// (re)lays the three-copy hierarchy out for populations of nb 256-particle blocks
int ensure_generic(cpprob_hip_ctx* c, int nb, int block)
{
    if (nb != c->gen_nb || block != c->gen_block || !c->d_gen_hier) {
        size_t per_copy = 0, off[kHierMaxLevels] = {0, 0, 0};
        int nl = 0;
        HierTable t{};
        for (size_t e = (size_t)nb;; e = (e + 63) / 64) {
            if (nl >= kHierMaxLevels) return fail(c, CPPROB_HIP_EUNSUPPORTED, "population too large for the three-level mass hierarchy");
            off[nl] = per_copy; t.n_ent[nl] = (int)e; per_copy += e * (nl == 0 ? 1 : kHierStride); ++nl;
            if (e <= 64) break;
        }
        t.n_lev = nl;
        c->gen_q0_off = per_copy; c->gen_m0_off = per_copy + (size_t)nb; per_copy += 2 * (size_t)nb;
        // (whole tiles, and one more: the step kernel's walk reads 1024-particle chunks that start at any block)
        const size_t q_words = ((size_t)nb * (size_t)block + kTile - 1) / kTile * kTile + kTile;
        if (3 * per_copy > c->gen_cap_hier || q_words > c->gen_cap_q || !c->d_gen_hier) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            dfree(c->d_gen_hier); dfree(c->d_gen_q[0]); dfree(c->d_gen_q[1]);
            c->gen_cap_hier = 0; c->gen_cap_q = 0; c->gen_nb = 0;
            HIP_TRY(c, hipMalloc(&c->d_gen_hier, 3 * per_copy * sizeof(uint64_t)));
            for (int k = 0; k < 2; ++k) { HIP_TRY(c, hipMalloc(&c->d_gen_q[k], q_words * sizeof(uint32_t))); HIP_TRY(c, hipMemsetAsync(c->d_gen_q[k], 0, q_words * sizeof(uint32_t), c->stream)); }
            c->gen_cap_hier = 3 * per_copy; c->gen_cap_q = q_words;
        }
        for (int k = 0; k < 3; ++k)
            for (int l = 0; l < kHierMaxLevels; ++l) t.lvl[k][l] = c->d_gen_hier + (size_t)k * per_copy + off[l < nl ? l : 0];
        if (!c->d_gen_table) HIP_TRY(c, hipMalloc(&c->d_gen_table, sizeof(HierTable)));
        if (!c->d_gen_ctrl) HIP_TRY(c, hipMalloc(&c->d_gen_ctrl, sizeof(GenericCtrlBlock)));
        HIP_TRY(c, hipMemcpyAsync(c->d_gen_table, &t, sizeof t, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));               // (t is a local)
        c->gen_table = t; c->gen_per_copy = per_copy; c->gen_nb = nb; c->gen_block = block;
        for (int l = 0; l < kHierMaxLevels; ++l) c->gen_off[l] = off[l];
    }
    return 0;
}
// copy `read` as the launch's view; the copy written sits `to_next` words further, the copy cleared `to_clear`
void generic_view(const cpprob_hip_ctx* c, int read, int next, int clear, FHier& f)
{
    const HierTable& t = c->gen_table;
    for (int l = 0; l < kHierMaxLevels; ++l) { f.h.lvl[l] = t.lvl[read][l]; f.h.n_ent[l] = t.n_ent[l]; }
    f.h.n_lev = t.n_lev; f.h.table = c->d_gen_table; f.h.copy = read;
    const int top = t.n_lev - 1;
    f.h.top = t.lvl[read][top]; f.h.top_n = t.n_ent[top]; f.h.top_stride = top == 0 ? 1 : kHierStride;
    f.h.to_next = (int64_t)(next - read) * (int64_t)c->gen_per_copy; f.h.to_clear = (int64_t)(clear - read) * (int64_t)c->gen_per_copy;
    f.q0 = c->d_gen_hier + (size_t)read * c->gen_per_copy + c->gen_q0_off;
    f.m0 = c->d_gen_hier + (size_t)read * c->gen_per_copy + c->gen_m0_off;
}
}  // namespace
extern "C" {

static int generic_begin(cpprob_hip_ctx* c, size_t n, int block, cpprob_hip_generic_layout* out)
{
    if (!out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (block != kGenBlock && block != kTile) return fail(c, CPPROB_HIP_EINVAL, "the hierarchy's entries are blocks of 256 particles or tiles of 1024");
    if (n == 0 || n > (size_t)(1ull << 28)) return fail(c, CPPROB_HIP_EINVAL, "population size out of range (1 .. 2^28: the squares' 64-bit sum)");
    if (n > (size_t)kCountsMaxTiles * (size_t)block) return fail(c, CPPROB_HIP_EINVAL, "population too large for the three-level mass hierarchy (64^3 entries)");
    const int nb = (int)((n + (size_t)block - 1) / (size_t)block);
    if (int rc = ensure_generic(c, nb, block)) return rc;
    // a run starts from clean upper levels in every copy
    HIP_TRY(c, hipMemsetAsync(c->d_gen_hier, 0, 3 * c->gen_per_copy * sizeof(uint64_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_gen_ctrl, 0, sizeof(GenericCtrlBlock), c->stream));
    std::memset(out, 0, sizeof *out);
    out->hier = c->d_gen_hier; out->per_copy = c->gen_per_copy;
    for (int l = 0; l < kHierMaxLevels; ++l) { out->lvl_off[l] = c->gen_off[l < c->gen_table.n_lev ? l : 0]; out->n_ent[l] = c->gen_table.n_ent[l]; }
    out->n_lev = c->gen_table.n_lev; out->q0_off = c->gen_q0_off; out->m0_off = c->gen_m0_off;
    out->table = c->d_gen_table; out->q[0] = c->d_gen_q[0]; out->q[1] = c->d_gen_q[1]; out->ctrl = c->d_gen_ctrl; out->blocks = nb; out->block = block;
    return 0;
}
int cpprob_hip_generic_begin(cpprob_hip_ctx* c, size_t n, cpprob_hip_generic_layout* out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    return generic_begin(c, n, kGenBlock, out);
}
int cpprob_hip_generic_begin_tiles(cpprob_hip_ctx* c, size_t n, cpprob_hip_generic_layout* out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    return generic_begin(c, n, kTile, out);
}

static int generic_exact_passes(cpprob_hip_ctx* c, int32_t t, const double* d_logw, size_t n, bool max_pass, bool mass_pass, int given, double ref)
{
    if (!d_logw || t < 0) return fail(c, CPPROB_HIP_EINVAL, "bad argument");
    const int nb = (int)((n + kGenBlock - 1) / kGenBlock), nt = (int)((n + kTile - 1) / kTile);
    if (nb != c->gen_nb || c->gen_block != kGenBlock || !c->d_gen_hier) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_generic_begin was not called for this population size");
    FHier f{};
    generic_view(c, t % 3, t % 3, (t + 1) % 3, f);
    if (max_pass) hipLaunchKernelGGL(generic_max_kernel, dim3(nt), dim3(kThreads), 0, c->stream, d_logw, (int64_t)n, f, nb);
    if (mass_pass) hipLaunchKernelGGL(generic_quantize_kernel, dim3(nt), dim3(kThreads), 0, c->stream, d_logw, (int64_t)n, f, nb, c->d_gen_q[t & 1], static_cast<GenericCtrlBlock*>(c->d_gen_ctrl), given, ref);
    HIP_TRY(c, hipGetLastError());
    return 0;
}
int cpprob_hip_generic_quantize(cpprob_hip_ctx* c, int32_t t, const double* d_logw, size_t n)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    return generic_exact_passes(c, t, d_logw, n, true, true, 0, 0.0);
}
int cpprob_hip_generic_max(cpprob_hip_ctx* c, int32_t t, const double* d_logw, size_t n)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    return generic_exact_passes(c, t, d_logw, n, true, false, 0, 0.0);
}
int cpprob_hip_generic_quantize_ref(cpprob_hip_ctx* c, int32_t t, const double* d_logw, size_t n, double ref)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    return generic_exact_passes(c, t, d_logw, n, false, true, 1, ref);
}
int cpprob_hip_generic_totals(cpprob_hip_ctx* c, int32_t t, size_t n, uint64_t* d_out3)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!d_out3 || t < 0) return fail(c, CPPROB_HIP_EINVAL, "bad argument");
    const int nb = (int)((n + (size_t)c->gen_block - 1) / (size_t)c->gen_block);
    if (nb != c->gen_nb || !c->d_gen_hier) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_generic_begin was not called for this population size");
    FHier f{};
    generic_view(c, t % 3, t % 3, t % 3, f);
    hipLaunchKernelGGL(fixed_totals_kernel, dim3(1), dim3(kWave), 0, c->stream, f, d_out3);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_generic_finish(cpprob_hip_ctx* c, int32_t T, size_t n, double gap_limit, double* d_ess, int32_t* d_resampled, double* d_log_z, int32_t* d_flags)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!d_ess || !d_resampled || !d_log_z || !d_flags || T < 1) return fail(c, CPPROB_HIP_EINVAL, "bad argument");
    const int nb = (int)((n + (size_t)c->gen_block - 1) / (size_t)c->gen_block);
    if (nb != c->gen_nb || !c->d_gen_hier) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_generic_begin was not called for this population size");
    FHier f{};
    const int k = (T - 1) % 3;
    generic_view(c, k, k, k, f);
    hipLaunchKernelGGL(generic_finish_kernel, dim3(1), dim3(kWave), 0, c->stream, f, (int)T, (double)n, gap_limit, static_cast<GenericCtrlBlock*>(c->d_gen_ctrl), d_ess, d_resampled,
                       d_log_z, d_flags);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

double cpprob_hip_systematic_offset(uint64_t seed, uint64_t step) { return host_resample_u0(seed, step); }

int cpprob_hip_lineage_gather(cpprob_hip_ctx* c, const int32_t* d_anc, const int32_t* d_resampled, int32_t T, size_t n, const void* d_cols, int32_t is_int,
                              const int32_t* h_gen, int32_t H, void* d_out)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (!d_anc || !d_resampled || !d_cols || !h_gen || !d_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (T < 1 || H < 0) return fail(c, CPPROB_HIP_EINVAL, "bad T / H");
    if (n == 0 || H == 0) return 0;
    if (int rc = upload_first_rows(c, h_gen, H, T)) return rc;
    int32_t* d_first = c->d_bb_first;
    if (is_int) hipLaunchKernelGGL(lineage_gather_kernel<int32_t>, GRID1(n), d_anc, d_resampled, (int)T, (int64_t)n, static_cast<const int32_t*>(d_cols), (const int32_t*)d_first, static_cast<int32_t*>(d_out));
    else hipLaunchKernelGGL(lineage_gather_kernel<double>, GRID1(n), d_anc, d_resampled, (int)T, (int64_t)n, static_cast<const double*>(d_cols), (const int32_t*)d_first, static_cast<double*>(d_out));
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_gather_f64(cpprob_hip_ctx* c, const double* src, const int32_t* idx, size_t n, double* dst)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (n == 0) return 0;
    hipLaunchKernelGGL(gather_kernel<double>, GRID1(n), src, idx, (int64_t)n, dst);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_gather_i32(cpprob_hip_ctx* c, const int32_t* src, const int32_t* idx, size_t n, int32_t* dst)
{
    LANES_OWN(c);
    BB_PRELUDE(c);
    if (n == 0) return 0;
    hipLaunchKernelGGL(gather_kernel<int32_t>, GRID1(n), src, idx, (int64_t)n, dst);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_profile_enable(cpprob_hip_ctx* c, int32_t on)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    c->profile = on != 0;
    return 0;
}

int cpprob_hip_profile_read(cpprob_hip_ctx* c, double* h_ms, int64_t* h_calls, int32_t reset)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (auto& ep : c->ev_used) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) { c->prof_ms[ep.cls] += ms; c->prof_calls[ep.cls] += ep.count; }
        c->ev_free.push_back(ep);
    }
    c->ev_used.clear();
    for (int k = 0; k < CPPROB_HIP_N_KERNEL_CLASSES; ++k) {
        if (h_ms) h_ms[k] = c->prof_ms[k];
        if (h_calls) h_calls[k] = c->prof_calls[k];
        if (reset) { c->prof_ms[k] = 0; c->prof_calls[k] = 0; }
    }
    return 0;
}


// ---- batched SMC -----------------------------------------------------------------------------------------------------------------
int cpprob_hip_batch_workspace_bytes(const cpprob_hip_batch_config* cfg, size_t T, uint64_t* out_bytes)
{
    std::string msg;
    if (int rc = batch_check(cfg, T, msg)) return fail(nullptr, rc, msg);
    if (!out_bytes) return fail(nullptr, CPPROB_HIP_EINVAL, "NULL argument");
    const int spp = cfg->model == CPPROB_HIP_MODEL_HMM3 ? 3 : 8;
    *out_bytes = batch_layout(cfg->n_problems, T, 1, false, cfg->n_problems * T * cfg->n_particles, spp, cfg->keep_history == 1, false, 0, batch_masses(cfg)).total;
    return 0;
}

int cpprob_hip_batch_begin(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, const double* h_obs, size_t T)
{
    LANES_OWN(c);
    if (!c || !cfg || !h_obs) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    std::string msg;
    if (int rc = batch_check(cfg, T, msg)) return fail(c, rc, msg);
    if (cfg->model == CPPROB_HIP_MODEL_HMM_TABLE && c->hk < 2) return fail(c, CPPROB_HIP_ESTATE, "CPPROB_HIP_MODEL_HMM_TABLE: call cpprob_hip_set_hmm first");
    return batch_begin(c, cfg, T, nullptr, nullptr, h_obs, cfg->model == CPPROB_HIP_MODEL_HMM3 ? 3 : c->hk, nullptr, nullptr);
}

int cpprob_hip_batch_problems_workspace_bytes(const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n, uint64_t* out_bytes)
{
    std::string msg;
    BatchProblemsShape sh;
    if (int rc = batch_check_problems(cfg, h_T, h_n, sh, msg)) return fail(nullptr, rc, msg);
    if (!out_bytes) return fail(nullptr, CPPROB_HIP_EINVAL, "NULL argument");
    const int spp = cfg->model == CPPROB_HIP_MODEL_HMM3 ? 3 : 8;
    *out_bytes = batch_layout(cfg->n_problems, sh.T_max, cfg->n_problems, true, sh.steps, spp, cfg->keep_history == 1, false, 0, batch_masses(cfg)).total;
    return 0;
}

// The tables of a batch of problems (the described begins, re-table and online tables): per problem, or the context's; k = the states.
// rates: a Poisson call's, whose h_means are rates and pass what poisson_check's bit 16 demands (csrc/batch_poisson.hpp).
static int batch_check_tables(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, int32_t k_in, const double* h_means, const double* h_transition, int& k,
                              bool rates = false)
{
    const uint64_t B = cfg->n_problems;
    const bool hmm3 = cfg->model == CPPROB_HIP_MODEL_HMM3;
    const bool own = h_means || h_transition;                 // per-problem tables
    if (own && (!h_means || !h_transition)) return fail(c, CPPROB_HIP_EINVAL, "per-problem tables need both h_means and h_transition");
    if (hmm3 && own) return fail(c, CPPROB_HIP_EINVAL, "CPPROB_HIP_MODEL_HMM3 has its own table: h_means and h_transition must be NULL");
    if (!hmm3 && !own && c->hk < 2) return fail(c, CPPROB_HIP_ESTATE, "CPPROB_HIP_MODEL_HMM_TABLE: call cpprob_hip_set_hmm first, or pass per-problem tables");
    k = hmm3 ? 3 : (own ? (int)k_in : c->hk);
    if (own) {
        if (k_in < 2 || k_in > 8) return fail(c, CPPROB_HIP_EINVAL, "the table model holds 2 .. 8 states");
        // per table what cpprob_hip_set_hmm demands
        for (uint64_t b = 0; b < B; ++b) {
            const double* tr = h_transition + b * (size_t)k * k;
            const std::string at = "problem " + std::to_string(b) + ": ";
            for (int s2 = 0; s2 < k; ++s2) {
                double tot = 0.0;
                for (int j = 0; j < k; ++j) { const double w = tr[(size_t)s2 * k + j]; if (!(w >= 0.0) || !std::isfinite(w)) return fail(c, CPPROB_HIP_EINVAL, at + "transition weights must be finite and >= 0"); tot += w; }
                if (!(tot > 0.0)) return fail(c, CPPROB_HIP_EINVAL, at + "a transition row without mass");
                if (rates ? poisson_bad(h_means[b * (size_t)k + s2]) : !std::isfinite(h_means[b * (size_t)k + s2]))
                    return fail(c, CPPROB_HIP_EINVAL, at + (rates ? "emission rates must be > 0, finite and normal numbers" : "state means must be finite"));
            }
        }
    }
    return 0;
}

// The scales of a batch of problems (the scaled begins, re-table and online tables): per problem and state what scale_check's bit 8
// demands (csrc/batch_scale.hpp).
static int batch_check_scales(cpprob_hip_ctx* c, uint64_t B, int k, const double* h_sigmas)
{
    for (uint64_t b = 0; b < B; ++b)
        for (int s2 = 0; s2 < k; ++s2)
            if (scale_bad(h_sigmas[b * (size_t)k + (size_t)s2]))
                return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": emission scales must be finite and > 0, with a normal finite 2 pi sigma^2");
    return 0;
}

// The four begins over described problems (cpprob_hip_batch_begin_problems, _begin_online and their _scaled forms).  h_obs given: a begin
// over problems of h_T observes each; h_seeds given: an online begin of capacities h_T.  family: scaled: the call carries emission
// scales; Poisson: its h_means are rates (cpprob_hip_batch_begin_problems_poisson, _begin_online_poisson).  Both serve per-problem tables alone.
static int batch_begin_described(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n, const double* h_obs, int32_t k_in,
                                 const double* h_means, const double* h_transition, const double* h_sigmas, const uint64_t* h_seeds, EmissionFamily family)
{
    const bool scaled = family == kFamilyScaled, poisson = family == kFamilyPoisson;
    if (!c || !cfg || !h_T || !h_n || (!h_obs && !h_seeds) || (family != kFamilyUnit && (!h_means || !h_transition)) || (scaled && !h_sigmas)) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (scaled && cfg->model != CPPROB_HIP_MODEL_HMM_TABLE) return fail(c, CPPROB_HIP_EUNSUPPORTED, "emission scales serve CPPROB_HIP_MODEL_HMM_TABLE with per-problem tables");
    if (poisson && cfg->model != CPPROB_HIP_MODEL_HMM_TABLE) return fail(c, CPPROB_HIP_EUNSUPPORTED, "Poisson emissions serve CPPROB_HIP_MODEL_HMM_TABLE with per-problem tables");
    std::string msg;
    BatchProblemsShape sh;
    if (int rc = batch_check_problems(cfg, h_T, h_n, sh, msg)) return fail(c, rc, msg);
    int k = 0;
    if (int rc = batch_check_tables(c, cfg, k_in, h_means, h_transition, k, poisson)) return rc;
    if (scaled) if (int rc = batch_check_scales(c, cfg->n_problems, k, h_sigmas)) return rc;
    return batch_begin(c, cfg, (size_t)sh.T_max, h_T, h_n, h_obs, k, h_means, h_transition, h_seeds, h_sigmas, family);
}

int cpprob_hip_batch_begin_problems(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n,
                                    const double* h_obs, int32_t k_in, const double* h_means, const double* h_transition)
{
    LANES_OWN(c);
    return batch_begin_described(c, cfg, h_T, h_n, h_obs, k_in, h_means, h_transition, nullptr, nullptr, kFamilyUnit);
}

int cpprob_hip_batch_begin_problems_poisson(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n,
                                            const double* h_obs, int32_t k_in, const double* h_rates, const double* h_transition)
{
    LANES_OWN(c);
    return batch_begin_described(c, cfg, h_T, h_n, h_obs, k_in, h_rates, h_transition, nullptr, nullptr, kFamilyPoisson);
}

int cpprob_hip_batch_begin_problems_scaled(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n,
                                           const double* h_obs, int32_t k_in, const double* h_means, const double* h_transition, const double* h_sigmas)
{
    LANES_OWN(c);
    return batch_begin_described(c, cfg, h_T, h_n, h_obs, k_in, h_means, h_transition, h_sigmas, nullptr, kFamilyScaled);
}

// One launch over the begun batch: every problem from step 0 (cpprob_hip_batch_run), or its piece (cpprob_hip_batch_advance).
static int batch_launch(cpprob_hip_ctx* c, BatchState* bs, bool readout)
{
    const uint64_t B = bs->cfg.n_problems;
    const bool keep = bs->cfg.keep_history == 1;
    BatchArgs a{};
    if (bs->online) {
        a.first = reinterpret_cast<const int32_t*>(bs->ws() + bs->lay.first);
        a.snap = reinterpret_cast<BatchSnap*>(bs->ws() + bs->lay.snap);
        a.carry = keep ? nullptr : reinterpret_cast<uint8_t*>(bs->ws() + bs->lay.carry);
        a.skip_readout = keep && !readout ? 1 : 0;
    }
    a.mp = bs->mp;
    a.tab = reinterpret_cast<const double*>(bs->ws() + bs->lay.tab);
    a.seeds = reinterpret_cast<const uint64_t*>(bs->ws() + bs->lay.seeds);
    a.thr = reinterpret_cast<const uint64_t*>(bs->ws() + bs->lay.thr);
    a.thr_stride = bs->described ? 64 : 0;
    a.prob = bs->described ? reinterpret_cast<const BatchProblem*>(bs->ws() + bs->lay.prob) : nullptr;
    a.order = bs->described ? reinterpret_cast<const int32_t*>(bs->ws() + bs->lay.order) : nullptr;
    a.values = keep ? reinterpret_cast<int8_t*>(bs->ws() + bs->lay.values) : nullptr;
    a.anc = keep ? reinterpret_cast<int32_t*>(bs->ws() + bs->lay.anc) : nullptr;
    a.ctrl = bs->ws() + bs->lay.ctrl;
    a.stats = reinterpret_cast<double*>(bs->ws() + bs->lay.stats);
    a.ess = reinterpret_cast<double*>(bs->ws() + bs->lay.ess);
    a.resampled = reinterpret_cast<int32_t*>(bs->ws() + bs->lay.res);
    a.n_requant = reinterpret_cast<int32_t*>(bs->ws() + bs->lay.nreq);
    a.mass = batch_masses(&bs->cfg) ? reinterpret_cast<double*>(bs->ws() + bs->lay.mass) : nullptr;
    a.T_max = bs->T; a.n = (int)bs->cfg.n_particles; a.spp = bs->K; a.ess_frac = bs->cfg.ess_threshold;
    const bool strat = bs->cfg.resampler == CPPROB_HIP_RESAMPLE_STRATIFIED;
    const BatchKernel kern = bs->cfg.model == CPPROB_HIP_MODEL_HMM3 ? batch_kernel<ModelHmm3>(strat, keep, bs->online, a.mass != nullptr) : batch_kernel<ModelHmmK>(strat, keep, bs->online, a.mass != nullptr);
    hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kThreads), (size_t)batch_lds_bytes(a.n), c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_batch_run(cpprob_hip_ctx* c, const uint64_t* h_seeds)
{
    LANES_OWN(c);
    if (!c || !h_seeds) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_batch_begin has not been called");
    if (bs->online) return fail(c, CPPROB_HIP_ESTATE, "a batch begun by cpprob_hip_batch_begin_online is advanced (cpprob_hip_batch_advance), not run");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.seeds, h_seeds, bs->cfg.n_problems * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    if (int rc = batch_launch(c, bs, true)) return rc;
    bs->ran = true; bs->conditional = false;
    return 0;
}

// The device staging of a host call: front_bytes of the block in front of back_bytes (the caller rounds the former where the latter
// needs the alignment); a part of 0 bytes is nullptr.  Where the block has to grow, it waits first for the calls before it, whose
// copies and kernels may still read the block this replaces.
extern "C++" template <class F, class K> int batch_stage(cpprob_hip_ctx* c, size_t front_bytes, size_t back_bytes, F*& front, K*& back)
{
    BatchState* bs = c->batch;
    HIP_TRY(c, bs->d_stage.grow(c->stream, front_bytes + back_bytes));
    front = front_bytes ? reinterpret_cast<F*>(bs->d_stage.as<char>()) : nullptr;
    back = back_bytes ? reinterpret_cast<K*>(bs->d_stage.as<char>() + front_bytes) : nullptr;
    return 0;
}

// ---- conditional runs of a batch (csrc/batch_csmc.hpp) ----------------------------------------------------------------------------
// The state a conditional run needs and the total of its reference paths; nothing is enqueued before it has passed.
static int batch_conditional_check(cpprob_hip_ctx* c, const void* seeds, const void* ref, size_t n_entries)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!seeds || !ref) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_batch_begin has not been called");
    if (bs->online) return fail(c, CPPROB_HIP_EUNSUPPORTED, "conditional runs serve batches begun by cpprob_hip_batch_begin or _begin_problems: an online batch is advanced (cpprob_hip_batch_advance)");
    if (bs->cfg.model != CPPROB_HIP_MODEL_HMM_TABLE) return fail(c, CPPROB_HIP_EUNSUPPORTED, "conditional runs serve CPPROB_HIP_MODEL_HMM_TABLE");
    if (bs->cfg.keep_history != 0 || !batch_masses(&bs->cfg))
        return fail(c, CPPROB_HIP_ESTATE, "a conditional run keeps masses, not a particle store: begin the batch with keep_history = 0 and CPPROB_HIP_BATCH_KEEP_MASSES");
    uint64_t rows = 0;
    for (const BatchProblem& pr : bs->prob) rows += (uint64_t)pr.T;
    if ((uint64_t)n_entries != rows) return fail(c, CPPROB_HIP_EINVAL, "the reference paths hold " + std::to_string(n_entries) + " entries: the batch's lengths sum to " + std::to_string(rows));
    return 0;
}

// A described batch's first entries ([B] int64: the sums of the lengths before each problem -- where its reference path and its observes
// begin in a packed array) on the device, written and uploaded once a begin; waits for nothing, but where the buffer has to grow, for
// the calls before it.
static int batch_first_entries(cpprob_hip_ctx* c)
{
    BatchState* bs = c->batch;
    const size_t B = bs->cfg.n_problems;
    if (!bs->described || bs->cfirst_ready) return 0;
    HIP_TRY(c, bs->d_cfirst.grow(c->stream, B * sizeof(int64_t)));
    HIP_TRY(c, bs->pin_cfirst.grow(c->stream, B * sizeof(int64_t)));
    // (the pinned source is written once a begin, and a begin ends with the stream drained: no copy still reads it)
    int64_t at = 0;
    for (size_t b = 0; b < B; ++b) { bs->pin_cfirst.as<int64_t>()[b] = at; at += (int64_t)bs->prob[b].T; }
    HIP_TRY(c, hipMemcpyAsync(bs->d_cfirst.as<int64_t>(), bs->pin_cfirst.as<int64_t>(), B * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    bs->cfirst_ready = true;
    return 0;
}

// Enqueues the seeds' copy, a described batch's first entries (once a begin) and the launch; waits for nothing, but where the buffer
// of first entries has to grow, for the calls before it.
static int batch_conditional_enqueue(cpprob_hip_ctx* c, const uint64_t* h_seeds, const int8_t* d_ref)
{
    BatchState* bs = c->batch;
    const size_t B = bs->cfg.n_problems;
    if (int rc = batch_first_entries(c)) return rc;
    HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.seeds, h_seeds, B * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    BatchCsmcArgs a{};
    a.tab = reinterpret_cast<const double*>(bs->ws() + bs->lay.tab);
    a.seeds = reinterpret_cast<const uint64_t*>(bs->ws() + bs->lay.seeds);
    a.thr = reinterpret_cast<const uint64_t*>(bs->ws() + bs->lay.thr);
    a.thr_stride = bs->described ? 64 : 0;
    a.prob = bs->described ? reinterpret_cast<const BatchProblem*>(bs->ws() + bs->lay.prob) : nullptr;
    a.order = bs->described ? reinterpret_cast<const int32_t*>(bs->ws() + bs->lay.order) : nullptr;
    a.ref = d_ref;
    a.first = bs->described ? bs->d_cfirst.as<int64_t>() : nullptr;
    a.mass = reinterpret_cast<double*>(bs->ws() + bs->lay.mass);
    a.T_max = bs->T; a.n = (int)bs->cfg.n_particles; a.k = bs->hk;
    hipLaunchKernelGGL(batch_csmc_kernel, dim3((unsigned)B), dim3(kThreads), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    bs->ran = true; bs->conditional = true;
    return 0;
}

int cpprob_hip_batch_run_conditional_device(cpprob_hip_ctx* c, const uint64_t* h_seeds, const int8_t* d_ref, size_t n_entries)
{
    LANES_OWN(c);
    if (int rc = batch_conditional_check(c, h_seeds, d_ref, n_entries)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_conditional_enqueue(c, h_seeds, d_ref);
}

int cpprob_hip_batch_run_conditional(cpprob_hip_ctx* c, const uint64_t* h_seeds, const int32_t* h_ref, size_t n_entries)
{
    LANES_OWN(c);
    if (int rc = batch_conditional_check(c, h_seeds, h_ref, n_entries)) return rc;
    BatchState* bs = c->batch;
    std::vector<int8_t> v(n_entries);
    size_t at = 0;
    for (size_t b = 0; b < bs->prob.size(); ++b)
        for (int t = 0; t < bs->prob[b].T; ++t, ++at) {
            if (h_ref[at] < 0 || h_ref[at] >= bs->hk)
                return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ", step " + std::to_string(t) + ": the reference state " + std::to_string(h_ref[at]) +
                                                  " lies outside 0 .. " + std::to_string(bs->hk - 1));
            v[at] = (int8_t)h_ref[at];
        }
    HIP_TRY(c, hipSetDevice(c->device));
    int8_t *d_ref = nullptr, *none = nullptr;
    if (int rc = batch_stage(c, n_entries, 0, d_ref, none)) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_ref, v.data(), n_entries, hipMemcpyHostToDevice, c->stream));
    if (int rc = batch_conditional_enqueue(c, h_seeds, d_ref)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));               // (the staged copy has read v; a later host call may take the staging over)
    return 0;
}

int cpprob_hip_batch_online_workspace_bytes(const cpprob_hip_batch_config* cfg, const uint32_t* h_Tcap, const uint32_t* h_n, uint64_t* out_bytes)
{
    std::string msg;
    BatchProblemsShape sh;
    if (int rc = batch_check_problems(cfg, h_Tcap, h_n, sh, msg)) return fail(nullptr, rc, msg);
    if (!out_bytes) return fail(nullptr, CPPROB_HIP_EINVAL, "NULL argument");
    const int spp = cfg->model == CPPROB_HIP_MODEL_HMM3 ? 3 : 8;
    *out_bytes = batch_layout(cfg->n_problems, sh.T_max, cfg->n_problems, true, sh.steps, spp, cfg->keep_history == 1, true, sh.particles, batch_masses(cfg)).total;
    return 0;
}

int cpprob_hip_batch_begin_online(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, const uint32_t* h_Tcap, const uint32_t* h_n,
                                  int32_t k_in, const double* h_means, const double* h_transition, const uint64_t* h_seeds)
{
    LANES_OWN(c);
    return batch_begin_described(c, cfg, h_Tcap, h_n, nullptr, k_in, h_means, h_transition, nullptr, h_seeds, kFamilyUnit);
}

int cpprob_hip_batch_begin_online_poisson(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, const uint32_t* h_Tcap, const uint32_t* h_n,
                                          int32_t k_in, const double* h_rates, const double* h_transition, const uint64_t* h_seeds)
{
    LANES_OWN(c);
    return batch_begin_described(c, cfg, h_Tcap, h_n, nullptr, k_in, h_rates, h_transition, nullptr, h_seeds, kFamilyPoisson);
}

int cpprob_hip_batch_begin_online_scaled(cpprob_hip_ctx* c, const cpprob_hip_batch_config* cfg, const uint32_t* h_Tcap, const uint32_t* h_n,
                                         int32_t k_in, const double* h_means, const double* h_transition, const double* h_sigmas, const uint64_t* h_seeds)
{
    LANES_OWN(c);
    return batch_begin_described(c, cfg, h_Tcap, h_n, nullptr, k_in, h_means, h_transition, h_sigmas, h_seeds, kFamilyScaled);
}

static int batch_learn_enqueue(cpprob_hip_ctx* c, const uint32_t* before, const double* d_obs);

// One advance of the begun online batch.  Plain (cpprob_hip_batch_advance): the new rows are evaluated on the host from bs->means and
// copied.  Learning (cpprob_hip_batch_advance_learn*, learn: the batch is armed): the rows are written on the device from the
// device-resident tables and the observes (d_obs, or h_obs copied into a buffer of the context's own), and the learn step follows the
// launch (csrc/batch_learn.hpp).  Nothing changes before every check has passed.
static int batch_advance(cpprob_hip_ctx* c, const uint32_t* h_dT, const double* h_obs, const double* d_obs, size_t n_observes, int32_t readout, bool learn)
{
    if (!c || !h_dT) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun || !bs->online)
        return fail(c, CPPROB_HIP_ESTATE, std::string(learn ? "cpprob_hip_batch_advance_learn" : "cpprob_hip_batch_advance") + " serves a batch begun by cpprob_hip_batch_begin_online");
    if (learn && !bs->armed) return fail(c, CPPROB_HIP_ESTATE, "the online batch is not armed: call cpprob_hip_batch_learn_begin before its first advance");
    if (!learn && bs->armed) return fail(c, CPPROB_HIP_ESTATE, "the online batch learns its tables (cpprob_hip_batch_learn_begin): it is advanced by cpprob_hip_batch_advance_learn");
    const uint64_t B = bs->cfg.n_problems;
    uint64_t total = 0;
    for (uint64_t b = 0; b < B; ++b) {
        if ((uint64_t)bs->prob[b].T + h_dT[b] > bs->cap_T[b])
            return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": " + std::to_string(h_dT[b]) + " more observes after " + std::to_string(bs->prob[b].T) +
                                              " exceed its capacity of " + std::to_string(bs->cap_T[b]));
        total += h_dT[b];
    }
    if (total && !h_obs && !d_obs) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (learn && !h_obs && (uint64_t)n_observes != total)
        return fail(c, CPPROB_HIP_EINVAL, "n_observes = " + std::to_string(n_observes) + ", the advance hands over " + std::to_string(total) + " observes (the sum of h_dT)");
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<uint32_t> before;                              // (learning: the lengths the learn step resumes from)
    if (learn) {
        before.resize(B);
        for (uint64_t b = 0; b < B; ++b) before[b] = (uint32_t)bs->prob[b].T;
        if (h_obs) HIP_TRY(c, bs->learn.obs.grow(c->stream, (size_t)total * sizeof(double)));      // (the advance before may still read the buffer this replaces)
    }
    // this advance's descriptors: its slot is free once the copies of the advance that used it last have run
    const int slot = bs->advance_ring.slot_index();
    char* sl = nullptr;
    HIP_TRY(c, bs->advance_ring.acquire(sl));
    BatchProblem* pr = reinterpret_cast<BatchProblem*>(sl);
    int32_t* first = reinterpret_cast<int32_t*>(sl + B * sizeof(BatchProblem));
    int32_t* order = first + B;
    int64_t* ofirst = learn ? bs->learn.pin_first.as<int64_t>() + (size_t)slot * B : nullptr;
    const bool hmm3 = bs->cfg.model == CPPROB_HIP_MODEL_HMM3, keep = bs->cfg.keep_history == 1;
    const size_t hk = (size_t)bs->hk, T_max = (size_t)bs->T, row_bytes = kBatchTab * sizeof(double);
    const bool own = !hmm3 && bs->means.size() > hk;
    std::vector<double> mean;
    if (!hmm3 && !own) mean = bs->means;
    size_t at_obs = 0;
    for (uint64_t b = 0; b < B; ++b) {
        const size_t L = (size_t)bs->prob[b].T;
        if (learn) { ofirst[b] = (int64_t)at_obs; at_obs += h_dT[b]; }
        if (own && h_dT[b] && !learn) mean.assign(bs->means.begin() + (ptrdiff_t)(b * hk), bs->means.begin() + (ptrdiff_t)((b + 1) * hk));
        for (size_t t = L; !learn && t < L + h_dT[b]; ++t) {
            const double y = h_obs[at_obs++];
            double* row = bs->pin_tab.as<double>() + (b * T_max + t) * kBatchTab;
            if (hmm3) hmm3_step_table(y, bs->mp.hmm_mean, row, row + 3, row[6]);
            else if (bs->scaled) scale_step_ll(y, mean.data(), &bs->sigmas[b * 8], &bs->log_norms[b * 8], (int)hk, row);
            else if (bs->poisson) poisson_step_ll(y, &bs->sigmas[b * 8], &bs->log_norms[b * 8], bs->lfact.data(), (int)hk, row);
            else hmmk_step_ll(y, mean, (int)hk, row);
        }
        // (a problem without observes, or without new ones and with its read-out done, has nothing to do)
        const bool idle = h_dT[b] == 0 && (L == 0 || !keep || bs->walked_b[b] || !readout);
        first[b] = idle ? -1 : (int32_t)L;
        if (keep && !idle) bs->walked_b[b] = readout ? 1 : 0;
        order[b] = (int32_t)b;
        bs->prob[b].T = (int32_t)(L + h_dT[b]);
        pr[b] = bs->prob[b];
    }
    // the longest pieces first, ties by index
    auto cost = [&](int32_t b) { return (uint64_t)h_dT[b] * (((uint64_t)bs->prob[b].n + kTile - 1) / kTile); };
    std::stable_sort(order, order + B, [&](int32_t x, int32_t y) { return cost(x) > cost(y); });
    // the new rows: one strided copy per run of problems that share first step and piece length
    for (uint64_t b = 0; !learn && b < B;) {
        uint64_t e = b + 1;
        while (e < B && bs->prob[e].T == bs->prob[b].T && h_dT[e] == h_dT[b]) ++e;
        if (h_dT[b]) {
            const size_t at = ((size_t)b * T_max + (size_t)first[b]) * row_bytes;      // (h_dT[b] > 0: first[b] is its length before)
            HIP_TRY(c, hipMemcpy2DAsync(bs->ws() + bs->lay.tab + at, T_max * row_bytes, reinterpret_cast<const char*>(bs->pin_tab.as<double>()) + at, T_max * row_bytes,
                                        (size_t)h_dT[b] * row_bytes, (size_t)(e - b), hipMemcpyHostToDevice, c->stream));
        }
        b = e;
    }
    HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.prob, pr, B * sizeof(BatchProblem), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.first, first, B * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.order, order, B * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (learn) HIP_TRY(c, hipMemcpyAsync(bs->learn.first.as<int64_t>(), ofirst, B * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, bs->advance_ring.commit(c->stream));
    if (learn && total) {
        // the new rows, on the device: from the observes and the tables in force
        if (h_obs) { HIP_TRY(c, hipMemcpyAsync(bs->learn.obs.as<double>(), h_obs, (size_t)total * sizeof(double), hipMemcpyHostToDevice, c->stream)); d_obs = bs->learn.obs.as<double>(); }
        uint32_t top = 0;
        for (uint64_t b = 0; b < B; ++b) top = std::max(top, h_dT[b]);
        const dim3 grid((unsigned)B, retable_grid_y(top, (int64_t)B));
        auto common = [&](auto& r) {                            // (what the two forms' arguments share)
            r.prob = reinterpret_cast<const BatchProblem*>(bs->ws() + bs->lay.prob);
            r.first = reinterpret_cast<const int32_t*>(bs->ws() + bs->lay.first);
            r.ofirst = bs->learn.first.as<int64_t>(); r.means = bs->learn.means.as<double>(); r.obs = d_obs;
            r.tab = reinterpret_cast<double*>(bs->ws() + bs->lay.tab);
            r.T_max = bs->T; r.k = bs->hk;
        };
        if (bs->scaled) {
            BatchLearnRowsScaledArgs rs{};
            common(rs);
            rs.sigmas = bs->d_sigma.as<double>(); rs.log_norms = bs->d_lognorm.as<double>();
            hipLaunchKernelGGL(batch_learn_rows_scaled_kernel, grid, dim3(kThreads), 0, c->stream, rs);
        } else {
            BatchLearnRowsArgs ra{};
            common(ra);
            ra.log_norm = std::log(2 * kPi * 1.0 * 1.0);              // (normal_logpdf's own expression at sigma = 1.0)
            hipLaunchKernelGGL(batch_learn_rows_kernel, grid, dim3(kThreads), 0, c->stream, ra);
        }
        HIP_TRY(c, hipGetLastError());
        bs->tab_stale = true;
    }
    bool work = false, walked = true;
    for (uint64_t b = 0; b < B; ++b) { work = work || first[b] >= 0; walked = walked && bs->walked_b[b]; }
    if (work) if (int rc = batch_launch(c, bs, readout != 0)) return rc;
    bs->walked = walked;
    if (learn) return batch_learn_enqueue(c, before.data(), total ? d_obs : nullptr);
    return 0;
}

int cpprob_hip_batch_advance(cpprob_hip_ctx* c, const uint32_t* h_dT, const double* h_obs, int32_t readout)
{
    LANES_OWN(c);
    return batch_advance(c, h_dT, h_obs, nullptr, 0, readout, false);
}

int cpprob_hip_batch_advance_learn(cpprob_hip_ctx* c, const uint32_t* h_dT, const double* h_obs)
{
    LANES_OWN(c);
    return batch_advance(c, h_dT, h_obs, nullptr, 0, 1, true);
}

int cpprob_hip_batch_advance_learn_device(cpprob_hip_ctx* c, const uint32_t* h_dT, const double* d_obs, size_t n_observes)
{
    LANES_OWN(c);
    return batch_advance(c, h_dT, nullptr, d_obs, n_observes, 1, true);
}

int cpprob_hip_batch_lengths(cpprob_hip_ctx* c, uint32_t* h_L)
{
    LANES_OWN(c);
    if (!c || !h_L) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun || !bs->online) return fail(c, CPPROB_HIP_ESTATE, "cpprob_hip_batch_lengths serves a batch begun by cpprob_hip_batch_begin_online");
    for (uint64_t b = 0; b < bs->cfg.n_problems; ++b) h_L[b] = (uint32_t)bs->prob[b].T;
    return 0;
}

int cpprob_hip_batch_results(cpprob_hip_ctx* c, cpprob_hip_summary* h_out, double* h_stats, size_t n_doubles, double* h_ess, int32_t* h_resampled)
{
    LANES_OWN(c);
    if (!c || !h_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    if (!bs || !bs->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished batch run");
    if (bs->conditional) return fail(c, CPPROB_HIP_ESTATE, "a conditional run keeps masses, not books: the results wait for the next cpprob_hip_batch_run");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t B = bs->cfg.n_problems, T = (size_t)bs->T, need = B * T * (size_t)bs->K;
    if (h_stats && !bs->walked) return fail(c, CPPROB_HIP_ESTATE, "the statistics wait for an advance with readout = 1 (cpprob_hip_batch_advance)");
    if (h_stats && n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "h_stats too small");
    std::vector<char> ctrl(B * kBatchCtrlBytes);
    std::vector<int32_t> nreq(B);
    HIP_TRY(c, hipMemcpyAsync(ctrl.data(), bs->ws() + bs->lay.ctrl, ctrl.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(nreq.data(), bs->ws() + bs->lay.nreq, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (h_stats) HIP_TRY(c, hipMemcpyAsync(h_stats, bs->ws() + bs->lay.stats, need * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_ess) HIP_TRY(c, hipMemcpyAsync(h_ess, bs->ws() + bs->lay.ess, B * T * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_resampled) HIP_TRY(c, hipMemcpyAsync(h_resampled, bs->ws() + bs->lay.res, B * T * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const bool hmm3 = bs->cfg.model == CPPROB_HIP_MODEL_HMM3;
    for (size_t b = 0; b < B; ++b) {
        StepCtrl h;
        std::memcpy(&h, ctrl.data() + b * kBatchCtrlBytes, sizeof h);
        cpprob_hip_summary* o = h_out + b;
        o->log_evidence = h.log_z;
        o->ess_final = h.ess;
        o->log_norm = h.M + std::log(h.W);
        o->max_logw = h.M;
        o->n_predict = bs->prob[b].T;
        o->stats_per_predict = bs->K;
        o->is_int = 1;
        o->n_resampled = h.n_resampled;
        o->step_form = hmm3 ? CPPROB_HIP_FORM_COUNTS : CPPROB_HIP_FORM_FIXED;
        o->n_requantised = hmm3 ? 0 : nreq[b];
    }
    return 0;
}

int cpprob_hip_batch_results_device(cpprob_hip_ctx* c, double* d_out, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c || !d_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    if (!bs || !bs->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished batch run");
    if (bs->conditional) return fail(c, CPPROB_HIP_ESTATE, "a conditional run keeps masses, not books: the results wait for the next cpprob_hip_batch_run");
    if (!bs->walked) return fail(c, CPPROB_HIP_ESTATE, "the statistics wait for an advance with readout = 1 (cpprob_hip_batch_advance)");
    const int64_t B = (int64_t)bs->cfg.n_problems, per = (int64_t)bs->T * bs->K;
    if (n_doubles < (size_t)(B * (4 + per))) return fail(c, CPPROB_HIP_EINVAL, "d_out too small: n_problems * (4 + n_predict * stats_per_predict) doubles");
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t total = B * (4 + per);
    // (a batch of problems: per = T_max spp; rows t >= T_b are zero -- begin cleared them and no run writes them)
    hipLaunchKernelGGL(batch_pack_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                       (const char*)(bs->ws() + bs->lay.ctrl), (const double*)(bs->ws() + bs->lay.stats), (int)per, B, d_out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_batch_copy_store(cpprob_hip_ctx* c, uint64_t problem, int32_t* h_values, int32_t* h_anc, double* h_logw)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished batch run");
    if (bs->cfg.keep_history != 1) return fail(c, CPPROB_HIP_ESTATE, "a filtering-only batch (keep_history = 0) keeps no particle store");
    if (problem >= bs->cfg.n_problems) return fail(c, CPPROB_HIP_EINVAL, "problem index out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    // the problem's own [T_b][n_b] from its first entry in the store on; its table rows are bs->T apart
    const size_t T = (size_t)bs->prob[problem].T, n = (size_t)bs->prob[problem].n, first = (size_t)bs->prob[problem].store;
    std::vector<int8_t> v(T * n);
    double fetched[kBatchTab];                                 // a re-tabled batch's rows are on the device only: the last step's, 64 bytes
    const size_t last = ((size_t)problem * (size_t)bs->T + (T ? T - 1 : 0)) * kBatchTab;
    if (h_logw && T > 0 && bs->tab_stale)
        HIP_TRY(c, hipMemcpyAsync(fetched, bs->ws() + bs->lay.tab + last * sizeof(double), sizeof fetched, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(v.data(), bs->ws() + bs->lay.values + first, T * n, hipMemcpyDeviceToHost, c->stream));
    if (h_anc) HIP_TRY(c, hipMemcpyAsync(h_anc, bs->ws() + bs->lay.anc + first * sizeof(int32_t), T * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_values) for (size_t i = 0; i < T * n; ++i) h_values[i] = v[i];
    if (h_logw && T > 0) {
        // the final weights are table values: ll of the last step at the particle's state (what cpprob_hip_copy_logw returns)
        const double* row = bs->tab_stale ? fetched : bs->tab_host() + last;
        for (size_t i = 0; i < n; ++i) h_logw[i] = row[(int)v[(T - 1) * n + i]];
    }
    return 0;
}

int cpprob_hip_batch_copy_masses(cpprob_hip_ctx* c, uint64_t problem, double* h_out, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished batch run");
    if (!batch_masses(&bs->cfg)) return fail(c, CPPROB_HIP_ESTATE, "the batch keeps no masses: begin it with keep_history = 0 and CPPROB_HIP_BATCH_KEEP_MASSES");
    if (problem >= bs->cfg.n_problems) return fail(c, CPPROB_HIP_EINVAL, "problem index out of range");
    const size_t T = (size_t)bs->prob[problem].T;
    if (n_doubles < T * 8) return fail(c, CPPROB_HIP_EINVAL, "h_out too small: " + std::to_string(T * 8) + " doubles (8 a step of the problem)");
    if (T == 0) return 0;
    if (!h_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(h_out, bs->ws() + bs->lay.mass + (size_t)problem * (size_t)bs->T * 8 * sizeof(double), T * 8 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- posterior traces of a batch (csrc/batch_paths.hpp) ---------------------------------------------------------------------------
int cpprob_hip_batch_paths_layout(const uint32_t* h_T, const uint32_t* h_n, uint64_t n_problems, uint64_t max_particles, uint64_t* h_first, uint64_t* h_wfirst)
{
    if (!h_T || !h_n) return fail(nullptr, CPPROB_HIP_EINVAL, "NULL argument");
    if (n_problems == 0) return fail(nullptr, CPPROB_HIP_EINVAL, "n_problems must be at least 1");
    for (uint64_t b = 0; b < n_problems; ++b)
        if (h_n[b] == 0 || h_n[b] > (uint32_t)kBatchMaxN)
            return fail(nullptr, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": its particle count must lie in 1 .. " + std::to_string(kBatchMaxN));
    uint64_t first = 0, wfirst = 0;
    for (uint64_t b = 0; b < n_problems; ++b) {
        if (h_first) h_first[b] = first;
        if (h_wfirst) h_wfirst[b] = wfirst;
        const uint64_t m = batch_paths_m(h_n[b], max_particles);
        first += (uint64_t)h_T[b] * m;
        wfirst += h_T[b] ? m : 0;
    }
    if (h_first) h_first[n_problems] = first;
    if (h_wfirst) h_wfirst[n_problems] = wfirst;
    return 0;
}

// The state a batch's traces need (as cpprob_hip_batch_copy_store), then the packed totals against the caller's capacities.
static int batch_paths_check(cpprob_hip_ctx* c, uint64_t max_particles, size_t n_entries, bool with_logw, size_t n_weights, uint64_t& entries, uint64_t& weights)
{
    BatchState* bs = c->batch;
    if (!bs || !bs->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished batch run");
    if (bs->cfg.keep_history != 1) return fail(c, CPPROB_HIP_ESTATE, "a filtering-only batch (keep_history = 0) keeps no particle store");
    entries = 0; weights = 0;
    for (const BatchProblem& pr : bs->prob) {
        const uint64_t m = batch_paths_m((uint64_t)pr.n, max_particles);
        entries += (uint64_t)pr.T * m;
        weights += pr.T ? m : 0;
    }
    if (n_entries < entries) return fail(c, CPPROB_HIP_EINVAL, "the paths buffer is too small: " + std::to_string(entries) + " entries (cpprob_hip_batch_paths_layout)");
    if (with_logw && n_weights < weights) return fail(c, CPPROB_HIP_EINVAL, "the log-weight buffer is too small: " + std::to_string(weights) + " weights (cpprob_hip_batch_paths_layout)");
    return 0;
}

// Enqueues the descriptors' copy and the walk on the context's stream; waits for nothing but the pinned slot it writes (the copy
// that read it kOnlineSlots calls ago).
static int batch_paths_enqueue(cpprob_hip_ctx* c, uint64_t max_particles, int8_t* d_paths, double* d_logw)
{
    BatchState* bs = c->batch;
    const size_t B = bs->cfg.n_problems, bytes = batch_round(B * sizeof(BatchPathsProblem));
    HIP_TRY(c, bs->paths_ring.reserve(c->stream, bytes));       // (earlier calls' copies may still read the buffers these replace)
    HIP_TRY(c, bs->d_pdesc.grow(c->stream, bytes));
    char* sl = nullptr;
    HIP_TRY(c, bs->paths_ring.acquire(sl));
    BatchPathsProblem* pd = reinterpret_cast<BatchPathsProblem*>(sl);
    int64_t first = 0, wfirst = 0;
    int m_top = 0;
    for (size_t b = 0; b < B; ++b) {
        const BatchProblem& pr = bs->prob[b];
        const int m = (int)batch_paths_m((uint64_t)pr.n, max_particles);
        pd[b].T = pr.T; pd[b].n = pr.n; pd[b].m = m; pd[b].pad_ = 0;
        pd[b].store = pr.store; pd[b].first = first; pd[b].wfirst = wfirst;
        first += (int64_t)pr.T * m;
        if (pr.T) { wfirst += m; m_top = std::max(m_top, m); }
    }
    if (m_top == 0) return 0;                                  // (an online batch before its first observes: nothing to resolve)
    HIP_TRY(c, hipMemcpyAsync(bs->d_pdesc.as<char>(), pd, B * sizeof(BatchPathsProblem), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, bs->paths_ring.commit(c->stream));
    BatchPathsArgs a{};
    a.desc = reinterpret_cast<const BatchPathsProblem*>(bs->d_pdesc.as<char>());
    a.values = reinterpret_cast<const int8_t*>(bs->ws() + bs->lay.values);
    a.anc = reinterpret_cast<const int32_t*>(bs->ws() + bs->lay.anc);
    a.tab = reinterpret_cast<const double*>(bs->ws() + bs->lay.tab);
    a.paths = d_paths; a.logw = d_logw; a.T_max = bs->T;
    hipLaunchKernelGGL(batch_paths_kernel, dim3((unsigned)B, (unsigned)((m_top + kTile - 1) / kTile)), dim3(kThreads), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_batch_paths_device(cpprob_hip_ctx* c, uint64_t max_particles, int8_t* d_paths, size_t n_entries, double* d_logw, size_t n_weights)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t entries = 0, weights = 0;
    if (int rc = batch_paths_check(c, max_particles, n_entries, d_logw != nullptr, n_weights, entries, weights)) return rc;
    if (!d_paths && entries) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_paths_enqueue(c, max_particles, d_paths, d_logw);
}

// A host call's results: the int8 entries and the doubles copied back (either count may be 0), the stream waited for, the entries
// widened to int32.
static int batch_fetch(cpprob_hip_ctx* c, int32_t* h_int32, const int8_t* d_int8, size_t entries, double* h_doubles, const double* d_doubles, size_t n_doubles)
{
    std::vector<int8_t> v(entries);
    if (entries) HIP_TRY(c, hipMemcpyAsync(v.data(), d_int8, entries, hipMemcpyDeviceToHost, c->stream));
    if (n_doubles) HIP_TRY(c, hipMemcpyAsync(h_doubles, d_doubles, n_doubles * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < entries; ++i) h_int32[i] = v[i];
    return 0;
}

int cpprob_hip_batch_paths(cpprob_hip_ctx* c, uint64_t max_particles, int32_t* h_paths, size_t n_entries, double* h_logw, size_t n_weights)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t entries = 0, weights = 0;
    if (int rc = batch_paths_check(c, max_particles, n_entries, h_logw != nullptr, n_weights, entries, weights)) return rc;
    if (!h_paths && entries) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (entries == 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    // device staging: the weights (8-byte aligned) in front of the int8 entries
    const size_t n_logw = h_logw ? (size_t)weights : 0;
    double* d_logw = nullptr;
    int8_t* d_paths = nullptr;
    if (int rc = batch_stage(c, batch_round(n_logw * sizeof(double)), (size_t)entries, d_logw, d_paths)) return rc;
    if (int rc = batch_paths_enqueue(c, max_particles, d_paths, d_logw)) return rc;
    return batch_fetch(c, h_paths, d_paths, (size_t)entries, h_logw, d_logw, n_logw);
}
// ---- backward smoothing of a batch (csrc/batch_smooth.hpp) ------------------------------------------------------------------------
int cpprob_hip_batch_smooth_layout(const uint32_t* h_T, uint64_t n_problems, uint64_t n_traj, uint64_t* h_first)
{
    if (!h_T || !h_first) return fail(nullptr, CPPROB_HIP_EINVAL, "NULL argument");
    if (n_problems == 0) return fail(nullptr, CPPROB_HIP_EINVAL, "n_problems must be at least 1");
    if (n_traj > (uint64_t)kBackwardMaxTraj) return fail(nullptr, CPPROB_HIP_EINVAL, "n_traj must lie in 0 .. 2^20");
    for (uint64_t b = 0; b < n_problems; ++b)
        if (h_T[b] > (uint32_t)kBackwardMaxT) return fail(nullptr, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": backward smoothing serves lengths up to 2^24");
    uint64_t rows = 0;
    for (uint64_t b = 0; b < n_problems; ++b) { h_first[b] = n_traj * rows; rows += h_T[b]; }
    h_first[n_problems] = n_traj * rows;
    return 0;
}

// The state backward smoothing needs (as cpprob_hip_batch_copy_store), the arguments' ranges, then the totals against the capacities.
static int batch_smooth_check(cpprob_hip_ctx* c, uint64_t n_traj, uint64_t draw_index, bool with_marg, size_t n_doubles, bool with_traj, size_t n_entries, uint64_t& doubles, uint64_t& entries)
{
    BatchState* bs = c->batch;
    if (bs) bs->smooth_gy_count = bs->smooth_gy_lag = bs->decode_gx_forward = bs->decode_gy_trace = bs->forecast_gy = bs->predictive_gy = bs->traj_stats_gy = 0;
    if (!bs || !bs->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished batch run");
    if (bs->cfg.keep_history != 1 && !batch_masses(&bs->cfg)) return fail(c, CPPROB_HIP_ESTATE, "a filtering-only batch (keep_history = 0) keeps no particle store");
    if (draw_index >= (uint64_t)kBackwardMaxDraws) return fail(c, CPPROB_HIP_EINVAL, "draw_index must lie in 0 .. 2^16 - 1");
    if (n_traj > (uint64_t)kBackwardMaxTraj) return fail(c, CPPROB_HIP_EINVAL, "n_traj must lie in 0 .. 2^20");
    uint64_t rows = 0;
    for (size_t b = 0; b < bs->prob.size(); ++b) {
        if (bs->prob[b].T > kBackwardMaxT) return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": backward smoothing serves lengths up to 2^24");
        rows += (uint64_t)bs->prob[b].T;
    }
    doubles = (uint64_t)bs->cfg.n_problems * (uint64_t)bs->T * (uint64_t)bs->K;
    entries = n_traj * rows;
    if (with_marg && n_doubles < doubles) return fail(c, CPPROB_HIP_EINVAL, "the marginals buffer is too small: " + std::to_string(doubles) + " doubles (n_problems * T_max * stats_per_predict)");
    if (with_traj && n_entries < entries) return fail(c, CPPROB_HIP_EINVAL, "the trajectories buffer is too small: " + std::to_string(entries) + " entries (cpprob_hip_batch_smooth_layout)");
    return 0;
}

static_assert(kTrajStats == kSuffStats && kOnlineStats == kSuffStats, "a trajectory's record and the running record have the layout of a problem's expected statistics");
// csrc/batch_pass_plan.hpp includes no kernel header: the constants it states are the kernels'
namespace bpl = batch_pass_limits;
static_assert(bpl::kThreads == kThreads && bpl::kWaves == kWaves && bpl::kTile == kTile && bpl::kTrajStatsTile == kTrajStatsTile && bpl::kStats == kSuffStats &&
              bpl::kBackwardMaxT == kBackwardMaxT && bpl::kBackwardLdsMax == kBackwardLdsMax && bpl::kSmoothCountGroups == kSmoothCountGroups &&
              bpl::kSmoothLagGridMax == kSmoothLagGridMax && bpl::kPredictiveGridMax == kPredictiveGridMax && bpl::kDecodeTraceGridMax == kDecodeTraceGridMax, "the plan's limits are the kernels'");
static int batch_decode_prepare(cpprob_hip_ctx* c, size_t word_rows);
static bool batch_hmm3(const BatchState* bs) { return bs->cfg.model == CPPROB_HIP_MODEL_HMM3; }
static BatchPassBatch<BatchProblem> batch_pass_batch(const BatchState* bs)
{
    return {(size_t)bs->cfg.n_problems, bs->prob.data(), bs->cap_T.data(), bs->counted.data(), bs->decoded.data(), bs->ostats_done.data(), bs->online, batch_masses(&bs->cfg) != 0, bs->T, bs->K};
}

// What every pass shares, in stream order: the output memsets; the growth of the context's own buffers, each after a wait for the
// calls before it (their copies and kernels may still read what it replaces); the wait for the pinned slot (the copy that read it
// kOnlineSlots calls ago); the plan's descriptors with the HMM3 thresholds behind them, their copy and its event; the shared arguments;
// the counting pass (an online batch's m table is addressed by capacity and kept: rows [counted_b, L_b), and the watermark moves).
// (done: a learning advance's OnlineStats pass -- the steps consumed are the lengths before the advance, and tau is the learner's)
static int batch_pass_prologue(cpprob_hip_ctx* c, const BatchPass& p, BatchPassPlan& pl, BatchSmoothArgs& a, const uint32_t* done = nullptr)
{
    BatchState* bs = c->batch;
    const size_t B = bs->cfg.n_problems, thr_bytes = 64 * sizeof(uint64_t), bytes = batch_round(B * sizeof(BatchSmoothProblem)) + thr_bytes;
    const bool hmm3 = batch_hmm3(bs), kept = batch_masses(&bs->cfg);
    BatchPassBatch<BatchProblem> bt = batch_pass_batch(bs);
    if (done) bt.ostats_done = done;
    pl = batch_pass_plan(bt, p);
    if (pl.marg_bytes) HIP_TRY(c, hipMemsetAsync(p.d_marg, 0, pl.marg_bytes, c->stream));
    if (pl.stats_bytes) HIP_TRY(c, hipMemsetAsync(p.d_stats, 0, pl.stats_bytes, c->stream));
    if (pl.traj_bytes) HIP_TRY(c, hipMemsetAsync(p.d_traj, 0, pl.traj_bytes, c->stream));
    if (pl.score_bytes) HIP_TRY(c, hipMemsetAsync(p.d_score, 0, pl.score_bytes, c->stream));
    if (pl.path_bytes) HIP_TRY(c, hipMemsetAsync(p.d_path, 0xff, pl.path_bytes, c->stream));
    if (pl.done) return 0;
    bool grew = false;                                                      // (what went with a block is forgotten before a failed allocation returns)
    HIP_TRY(c, bs->smooth_ring.reserve(c->stream, bytes));
    HIP_TRY(c, bs->d_sdesc.grow(c->stream, bs->smooth_ring.stride()));      // (a call copies a whole slot)
    const hipError_t mass_grow = bs->d_mass.grow(c->stream, pl.mass_rows * 8 * sizeof(double), &grew);
    if (grew) bs->counted.assign(B, 0);                                     // (the rows counted so far went with the table)
    HIP_TRY(c, mass_grow);
    if (p.decodes()) { if (int rc = batch_decode_prepare(c, pl.word_rows)) return rc; }
    if (p.kind == BatchPass::OnlineStats && !done) {
        const hipError_t tau_grow = bs->d_tau.grow(c->stream, B * (size_t)kOnlineTau * sizeof(double), &grew);
        if (grew) bs->ostats_done.assign(B, 0);
        HIP_TRY(c, tau_grow);
    }
    // the slot's stride, the copy below and the thresholds' place are those of the ring's last growth, not of this call's bytes
    const size_t slot_bytes = bs->smooth_ring.stride(), thr_at = slot_bytes - thr_bytes;
    char* sl = nullptr;
    HIP_TRY(c, bs->smooth_ring.acquire(sl));
    batch_pass_describe(bt, p, reinterpret_cast<BatchSmoothProblem*>(sl), pl);      // (after the growth: it reads the watermarks)
    // CPPROB_HIP_MODEL_HMM3: its thresholds as a table row set of CPPROB_HIP_MODEL_HMM_TABLE ([k][8], entries 0..k-2), behind the descriptors
    uint64_t* h3 = reinterpret_cast<uint64_t*>(sl + thr_at);
    for (int i = 0; i < 64; ++i) h3[i] = ~0ull;
    for (int s2 = 0; s2 < 3; ++s2) for (int j = 0; j < 2; ++j) h3[s2 * 8 + j] = bs->mp.hmm_thr[s2][j];
    HIP_TRY(c, hipMemcpyAsync(bs->d_sdesc.as<char>(), sl, slot_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, bs->smooth_ring.commit(c->stream));
    a.desc = reinterpret_cast<const BatchSmoothProblem*>(bs->d_sdesc.as<char>());
    a.values = kept ? nullptr : reinterpret_cast<const int8_t*>(bs->ws() + bs->lay.values);
    a.tab = reinterpret_cast<const double*>(bs->ws() + bs->lay.tab);
    a.thr = hmm3 ? reinterpret_cast<const uint64_t*>(bs->d_sdesc.as<char>() + thr_at) : reinterpret_cast<const uint64_t*>(bs->ws() + bs->lay.thr);
    a.thr_stride = !hmm3 && bs->described ? 64 : 0;
    a.seeds = reinterpret_cast<const uint64_t*>(bs->ws() + bs->lay.seeds);
    a.mass = kept ? reinterpret_cast<double*>(bs->ws() + bs->lay.mass) : bs->d_mass.as<double>(); a.marg = p.d_marg; a.traj = p.with_traj() ? p.d_traj : nullptr;
    a.draw_base = kBackwardDrawBase + (p.draw_index << 24);
    a.T_max = bs->T; a.k = hmm3 ? 3 : bs->hk; a.spp = bs->K; a.n_traj = (int)p.n_traj;
    a.marg_rows = (int)pl.marg_rows; a.lag = p.lagged() ? pl.lag : 0; a.lds_bytes = pl.lds_bytes;
    if (pl.count_gy) {
        hipLaunchKernelGGL(batch_smooth_count_kernel, dim3((unsigned)B, pl.count_gy), dim3(kThreads), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        bs->smooth_gy_count = pl.count_gy;
        if (bs->online) for (size_t b = 0; b < B; ++b) bs->counted[b] = (uint32_t)bs->prob[b].T;
    }
    return 0;
}

// The launchers, one a pass family: each builds its own arguments from the shared ones, launches with the plan's grid, records the
// grid where a call reads it back (cpprob_hip_batch_smooth_grid, _traj_stats_grid, _pass_grid) and moves its watermark.
static int batch_pass_smooth(cpprob_hip_ctx* c, const BatchPass& p, const BatchPassPlan& pl, BatchSmoothArgs a)
{
    BatchState* bs = c->batch; const unsigned B = (unsigned)bs->cfg.n_problems;
    if (pl.lag_gy) {
        hipLaunchKernelGGL(batch_smooth_lag_kernel, dim3(B, pl.lag_gy), dim3(kThreads), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
        bs->smooth_gy_lag = pl.lag_gy;
    }
    if (!pl.smooth_gy) return 0;
    if (p.lagged()) a.marg = nullptr;                                       // (the pass below: the window's trajectories only)
    if (batch_hmm3(bs)) hipLaunchKernelGGL(batch_smooth_kernel<3>, dim3(B, pl.smooth_gy), dim3(kThreads), (size_t)a.lds_bytes, c->stream, a);
    else hipLaunchKernelGGL(batch_smooth_kernel<8>, dim3(B, pl.smooth_gy), dim3(kThreads), (size_t)a.lds_bytes, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

static int batch_pass_stats(cpprob_hip_ctx* c, const BatchPass& p, const BatchPassPlan& pl, const BatchSmoothArgs& a)
{
    BatchSmoothStatsArgs sa{};
    sa.desc = a.desc; sa.mass = a.mass; sa.thr = a.thr; sa.obs = p.d_obs; sa.stats = p.d_stats;
    sa.B = (int)c->batch->cfg.n_problems; sa.k = a.k; sa.thr_stride = a.thr_stride;
    hipLaunchKernelGGL(batch_smooth_stats_kernel, dim3(pl.stats_gx), dim3(kThreads), 0, c->stream, sa);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

static int batch_pass_traj_stats(cpprob_hip_ctx* c, const BatchPass& p, const BatchPassPlan& pl, const BatchSmoothArgs& a)
{
    BatchState* bs = c->batch; const unsigned B = (unsigned)bs->cfg.n_problems;
    BatchTrajStatsArgs ta{};
    ta.desc = a.desc; ta.mass = a.mass; ta.thr = a.thr; ta.seeds = a.seeds; ta.obs = p.d_obs; ta.stats = p.d_stats;
    ta.draw_base = a.draw_base; ta.k = a.k; ta.thr_stride = a.thr_stride; ta.n_traj = (int)p.n_traj; ta.lds_bytes = a.lds_bytes;
    if (batch_hmm3(bs)) hipLaunchKernelGGL(batch_traj_stats_kernel<3>, dim3(B, pl.traj_stats_gy), dim3(kThreads), (size_t)a.lds_bytes, c->stream, ta);
    else hipLaunchKernelGGL(batch_traj_stats_kernel<8>, dim3(B, pl.traj_stats_gy), dim3(kThreads), (size_t)a.lds_bytes, c->stream, ta);
    HIP_TRY(c, hipGetLastError());
    bs->traj_stats_gy = pl.traj_stats_gy;
    return 0;
}

// (a problem without new steps is read out of its tau)
static int batch_pass_online_stats(cpprob_hip_ctx* c, const BatchPass& p, const BatchPassPlan& pl, const BatchSmoothArgs& a)
{
    BatchState* bs = c->batch; const size_t B = bs->cfg.n_problems;
    BatchOnlineStatsArgs oa{};
    oa.desc = a.desc; oa.mass = a.mass; oa.thr = a.thr; oa.obs = p.d_obs; oa.tau = bs->d_tau.as<double>(); oa.stats = p.d_stats;
    oa.B = (int)B; oa.k = a.k; oa.thr_stride = a.thr_stride;
    hipLaunchKernelGGL(batch_online_stats_kernel, dim3(pl.stats_gx), dim3(kThreads), 0, c->stream, oa);
    HIP_TRY(c, hipGetLastError());
    for (size_t b = 0; b < B; ++b) bs->ostats_done[b] = (uint32_t)bs->prob[b].T;
    return 0;
}

// (a run batch counts row L - 1 -- the forecast -- or rows max(from_b, 1) - 1 .. L - 1 -- the predictive rows -- only)
static int batch_pass_forecast(cpprob_hip_ctx* c, const BatchPass& p, const BatchPassPlan& pl, const BatchSmoothArgs& a)
{
    BatchState* bs = c->batch; const unsigned B = (unsigned)bs->cfg.n_problems;
    BatchForecastArgs fa{};
    fa.desc = a.desc; fa.mass = a.mass; fa.thr = a.thr; fa.seeds = a.seeds; fa.marg = p.d_marg; fa.traj = a.traj;
    fa.draw_base = kForecastDrawBase + (p.draw_index << 24);
    fa.k = a.k; fa.spp = a.spp; fa.thr_stride = a.thr_stride; fa.n_traj = (int)p.n_traj; fa.H = (int)p.horizon; fa.rows = (int)pl.marg_rows;
    if (p.kind == BatchPass::Predictive) {
        if (!pl.predictive_gy) return 0;                                    // (nothing owed anywhere)
        hipLaunchKernelGGL(batch_predictive_kernel, dim3(B, pl.predictive_gy), dim3(kThreads), 0, c->stream, fa);
    }
    else if (batch_hmm3(bs)) hipLaunchKernelGGL(batch_forecast_kernel<3>, dim3(B, pl.forecast_gy), dim3(kThreads), 0, c->stream, fa);
    else hipLaunchKernelGGL(batch_forecast_kernel<8>, dim3(B, pl.forecast_gy), dim3(kThreads), 0, c->stream, fa);
    HIP_TRY(c, hipGetLastError());
    bs->predictive_gy = pl.predictive_gy; bs->forecast_gy = pl.forecast_gy;
    return 0;
}

// (an online batch's forward pass walks steps [decoded_b, L_b) and moves that watermark)
static int batch_pass_decode(cpprob_hip_ctx* c, const BatchPass& p, const BatchPassPlan& pl, const BatchSmoothArgs& a)
{
    BatchState* bs = c->batch; const size_t B = bs->cfg.n_problems;
    BatchDecodeArgs da{};
    da.desc = a.desc; da.mass = a.mass; da.tab = a.tab; da.lp = bs->d_lp.as<double>(); da.lp0 = bs->lp0; da.v = bs->d_v.as<double>(); da.words = bs->d_words.as<uint32_t>();
    da.score = p.d_score; da.path = p.d_path;
    da.B = (int)B; da.T_max = a.T_max; da.k = a.k; da.lp_stride = bs->h_lp.size() > 64 ? 64 : 0;
    da.full = p.kind == BatchPass::Decode ? 1 : 0; da.lag = pl.lag; da.n_rows = (int)p.n_rows;
    hipLaunchKernelGGL(batch_decode_forward_kernel, dim3(pl.decode_gx), dim3(kThreads), 0, c->stream, da);
    HIP_TRY(c, hipGetLastError());
    bs->decode_gx_forward = pl.decode_gx;
    if (bs->online) for (size_t b = 0; b < B; ++b) bs->decoded[b] = (uint32_t)bs->prob[b].T;
    if (!pl.trace_gy) return 0;
    hipLaunchKernelGGL(batch_decode_trace_kernel, dim3((unsigned)B, pl.trace_gy), dim3(kThreads), 0, c->stream, da);
    HIP_TRY(c, hipGetLastError());
    bs->decode_gy_trace = pl.trace_gy;
    return 0;
}

// Enqueues one pass of the batch on the context's stream: the prologue, then the pass's own launches.  It waits for nothing but the
// pinned slot it writes and, where a buffer of its own has to grow, for the calls before it.
static int batch_smooth_enqueue(cpprob_hip_ctx* c, const BatchPass& p)
{
    BatchPassPlan pl; BatchSmoothArgs a{};
    if (int rc = batch_pass_prologue(c, p, pl, a)) return rc;
    if (pl.done) return 0;
    switch (p.kind) {
    case BatchPass::Smooth: case BatchPass::SmoothLag: return batch_pass_smooth(c, p, pl, a);
    case BatchPass::Stats: return batch_pass_stats(c, p, pl, a);
    case BatchPass::TrajStats: return batch_pass_traj_stats(c, p, pl, a);
    case BatchPass::OnlineStats: return batch_pass_online_stats(c, p, pl, a);
    case BatchPass::Forecast: case BatchPass::Predictive: return batch_pass_forecast(c, p, pl, a);
    case BatchPass::Decode: case BatchPass::DecodeLag: return batch_pass_decode(c, p, pl, a);
    }
    return 0;
}

// The host form of a pass that leaves rows of doubles (p.d_marg) and int8 entries (p.d_traj), either count may be 0: staged on the
// device, the doubles in front of the entries, enqueued and read back.
static int batch_pass_rows_host(cpprob_hip_ctx* c, BatchPass p, double* h_doubles, size_t n_doubles, int32_t* h_entries, size_t n_entries)
{
    if (int rc = batch_stage(c, batch_round(n_doubles * sizeof(double)), n_entries, p.d_marg, p.d_traj)) return rc;
    if (int rc = batch_smooth_enqueue(c, p)) return rc;
    return batch_fetch(c, h_entries, p.d_traj, n_entries, h_doubles, p.d_marg, n_doubles);
}

int cpprob_hip_batch_smooth_device(cpprob_hip_ctx* c, uint64_t n_traj, uint64_t draw_index, double* d_marginals, size_t n_doubles, int8_t* d_traj, size_t n_entries)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t doubles = 0, entries = 0;
    if (int rc = batch_smooth_check(c, n_traj, draw_index, d_marginals != nullptr, n_doubles, d_traj != nullptr, n_entries, doubles, entries)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_smooth_enqueue(c, BatchPass::smooth(n_traj, draw_index, d_marginals, d_traj));
}

int cpprob_hip_batch_smooth(cpprob_hip_ctx* c, uint64_t n_traj, uint64_t draw_index, double* h_marginals, size_t n_doubles, int32_t* h_traj, size_t n_entries)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t doubles = 0, entries = 0;
    if (int rc = batch_smooth_check(c, n_traj, draw_index, h_marginals != nullptr, n_doubles, h_traj != nullptr, n_entries, doubles, entries)) return rc;
    const bool with_traj = h_traj && entries;
    if (!h_marginals && !with_traj) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_pass_rows_host(c, BatchPass::smooth(n_traj, draw_index, nullptr, nullptr), h_marginals, h_marginals ? (size_t)doubles : 0, h_traj, with_traj ? (size_t)entries : 0);
}

// cpprob_hip_batch_smooth_lag's arguments against the batch's state (batch_smooth_check first), then the totals against the capacities.
static int batch_smooth_lag_check(cpprob_hip_ctx* c, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, uint64_t n_traj, uint64_t draw_index,
                                  bool with_marg, size_t n_doubles, bool with_traj, size_t n_entries, uint64_t& doubles, uint64_t& entries)
{
    uint64_t full_doubles = 0, full_entries = 0;
    if (int rc = batch_smooth_check(c, n_traj, draw_index, false, 0, false, 0, full_doubles, full_entries)) return rc;
    if (lag > (uint64_t)kBackwardMaxT) return fail(c, CPPROB_HIP_EINVAL, "lag must lie in 0 .. 2^24");
    BatchState* bs = c->batch;
    uint64_t win = 0;
    for (size_t b = 0; b < bs->prob.size(); ++b) {
        const uint64_t L = (uint64_t)bs->prob[b].T, from = h_from ? h_from[b] : 0;
        if (from > L) return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": from = " + std::to_string(from) + " lies past its length of " + std::to_string(L));
        if (with_marg && L - from > n_rows)
            return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": " + std::to_string(L - from) + " rows asked for, n_rows = " + std::to_string(n_rows));
        win += std::min<uint64_t>(lag + 1, L);
    }
    doubles = (uint64_t)bs->cfg.n_problems * n_rows * (uint64_t)bs->K;
    entries = n_traj * win;
    if (with_marg && n_doubles < doubles) return fail(c, CPPROB_HIP_EINVAL, "the marginals buffer is too small: " + std::to_string(doubles) + " doubles (n_problems * n_rows * stats_per_predict)");
    if (with_traj && n_entries < entries) return fail(c, CPPROB_HIP_EINVAL, "the trajectories buffer is too small: " + std::to_string(entries) + " entries (cpprob_hip_batch_smooth_layout of the windows)");
    return 0;
}

int cpprob_hip_batch_smooth_lag_device(cpprob_hip_ctx* c, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, uint64_t n_traj, uint64_t draw_index,
                                       double* d_marginals, size_t n_doubles, int8_t* d_traj, size_t n_entries)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t doubles = 0, entries = 0;
    if (int rc = batch_smooth_lag_check(c, lag, h_from, n_rows, n_traj, draw_index, d_marginals != nullptr, n_doubles, d_traj != nullptr, n_entries, doubles, entries)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_smooth_enqueue(c, BatchPass::smooth_lag(lag, h_from, n_rows, n_traj, draw_index, d_marginals, d_traj));
}

int cpprob_hip_batch_smooth_lag(cpprob_hip_ctx* c, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, uint64_t n_traj, uint64_t draw_index,
                                double* h_marginals, size_t n_doubles, int32_t* h_traj, size_t n_entries)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t doubles = 0, entries = 0;
    if (int rc = batch_smooth_lag_check(c, lag, h_from, n_rows, n_traj, draw_index, h_marginals != nullptr, n_doubles, h_traj != nullptr, n_entries, doubles, entries)) return rc;
    const bool with_marg = h_marginals && doubles, with_traj = h_traj && entries;
    if (!with_marg && !with_traj) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_pass_rows_host(c, BatchPass::smooth_lag(lag, h_from, n_rows, n_traj, draw_index, nullptr, nullptr), h_marginals, with_marg ? (size_t)doubles : 0, h_traj,
                                with_traj ? (size_t)entries : 0);
}

// cpprob_hip_batch_smooth_stats' arguments against the batch's state (batch_smooth_check first).
static int batch_smooth_stats_check(cpprob_hip_ctx* c, bool with_obs, size_t n_observes, const double* stats, size_t n_doubles, uint64_t& rows)
{
    uint64_t doubles = 0, entries = 0;
    if (int rc = batch_smooth_check(c, 0, 0, false, 0, false, 0, doubles, entries)) return rc;
    if (!stats) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    rows = 0;
    for (const BatchProblem& pr : bs->prob) rows += (uint64_t)pr.T;
    if (with_obs && (uint64_t)n_observes != rows)
        return fail(c, CPPROB_HIP_EINVAL, "n_observes = " + std::to_string(n_observes) + ", the problems' lengths sum to " + std::to_string(rows));
    const uint64_t need = (uint64_t)bs->cfg.n_problems * (uint64_t)kSuffStats;
    if (n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "the statistics buffer is too small: " + std::to_string(need) + " doubles (88 a problem)");
    return 0;
}

// A statistics call's device staging: the records in front of the observes, which it uploads (none of them: d_obs = nullptr).
static int batch_stage_observes(cpprob_hip_ctx* c, size_t n_stats, const double* h_observes, size_t n_observes, double*& d_stats, double*& d_obs)
{
    if (int rc = batch_stage(c, n_stats * sizeof(double), (h_observes ? n_observes : 0) * sizeof(double), d_stats, d_obs)) return rc;
    if (d_obs) HIP_TRY(c, hipMemcpyAsync(d_obs, h_observes, n_observes * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return 0;
}

int cpprob_hip_batch_smooth_stats_device(cpprob_hip_ctx* c, const double* d_observes, size_t n_observes, double* d_stats, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t rows = 0;
    if (int rc = batch_smooth_stats_check(c, d_observes != nullptr, n_observes, d_stats, n_doubles, rows)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_smooth_enqueue(c, BatchPass::stats(d_observes, d_stats));
}

int cpprob_hip_batch_smooth_stats(cpprob_hip_ctx* c, const double* h_observes, size_t n_observes, double* h_stats, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t rows = 0;
    if (int rc = batch_smooth_stats_check(c, h_observes != nullptr, n_observes, h_stats, n_doubles, rows)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_stats = (size_t)c->batch->cfg.n_problems * kSuffStats;
    double *d_stats = nullptr, *d_obs = nullptr;
    if (int rc = batch_stage_observes(c, n_stats, h_observes, (size_t)rows, d_stats, d_obs)) return rc;
    if (int rc = batch_smooth_enqueue(c, BatchPass::stats(d_obs, d_stats))) return rc;
    return batch_fetch(c, nullptr, nullptr, 0, h_stats, d_stats, n_stats);
}

// ---- running statistics of an online batch (csrc/batch_onlinestats.hpp) -------------------------------------------------------------
// cpprob_hip_batch_online_stats' arguments against the batch's state; fresh: the steps the call consumes.  It writes nothing.
static int batch_online_stats_check(cpprob_hip_ctx* c, const double* observes, size_t n_observes, const double* stats, size_t n_doubles, uint64_t& fresh)
{
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "no batch is begun");
    if (!bs->online) return fail(c, CPPROB_HIP_ESTATE, "running statistics serve a batch begun by cpprob_hip_batch_begin_online");
    if (bs->cfg.keep_history != 1 && !batch_masses(&bs->cfg))
        return fail(c, CPPROB_HIP_ESTATE, "a filtering-only batch (keep_history = 0) keeps no masses: begin it with CPPROB_HIP_BATCH_KEEP_MASSES");
    if (!stats) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    fresh = 0;
    for (size_t b = 0; b < bs->prob.size(); ++b) fresh += (uint64_t)bs->prob[b].T - std::min<uint64_t>(bs->ostats_done[b], (uint64_t)bs->prob[b].T);
    if ((observes || n_observes) && (uint64_t)n_observes != fresh)
        return fail(c, CPPROB_HIP_EINVAL, "n_observes = " + std::to_string(n_observes) + ", the call consumes " + std::to_string(fresh) + " steps (the lengths reached less the steps consumed)");
    if (!observes && n_observes) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    const uint64_t need = (uint64_t)bs->cfg.n_problems * (uint64_t)kOnlineStats;
    if (n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "the statistics buffer is too small: " + std::to_string(need) + " doubles (88 a problem)");
    return 0;
}

int cpprob_hip_batch_online_stats_device(cpprob_hip_ctx* c, const double* d_observes, size_t n_observes, double* d_stats, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t fresh = 0;
    if (int rc = batch_online_stats_check(c, d_observes, n_observes, d_stats, n_doubles, fresh)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_smooth_enqueue(c, BatchPass::online_stats(fresh ? d_observes : nullptr, d_stats));
}

int cpprob_hip_batch_online_stats(cpprob_hip_ctx* c, const double* h_observes, size_t n_observes, double* h_stats, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t fresh = 0;
    if (int rc = batch_online_stats_check(c, h_observes, n_observes, h_stats, n_doubles, fresh)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_stats = (size_t)c->batch->cfg.n_problems * kOnlineStats;
    double *d_stats = nullptr, *d_obs = nullptr;
    if (int rc = batch_stage_observes(c, n_stats, h_observes, (size_t)fresh, d_stats, d_obs)) return rc;
    if (int rc = batch_smooth_enqueue(c, BatchPass::online_stats(d_obs, d_stats))) return rc;
    return batch_fetch(c, nullptr, nullptr, 0, h_stats, d_stats, n_stats);
}

int cpprob_hip_batch_online_stats_progress(cpprob_hip_ctx* c, uint32_t* h_done)
{
    LANES_OWN(c);
    if (!c || !h_done) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun || !bs->online) return fail(c, CPPROB_HIP_ESTATE, "running statistics serve a batch begun by cpprob_hip_batch_begin_online");
    for (uint64_t b = 0; b < bs->cfg.n_problems; ++b) h_done[b] = bs->ostats_done[b];
    return 0;
}

// cpprob_hip_batch_traj_stats' arguments against the batch's state (batch_smooth_check first).
static int batch_traj_stats_check(cpprob_hip_ctx* c, uint64_t n_traj, uint64_t draw_index, bool with_obs, size_t n_observes, const double* stats, size_t n_doubles,
                                  uint64_t& rows, uint64_t& need)
{
    uint64_t doubles = 0, entries = 0;
    if (int rc = batch_smooth_check(c, n_traj, draw_index, false, 0, false, 0, doubles, entries)) return rc;
    if (n_traj == 0) return fail(c, CPPROB_HIP_EINVAL, "n_traj must lie in 1 .. 2^20");
    if (!stats) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    rows = 0;
    for (const BatchProblem& pr : bs->prob) rows += (uint64_t)pr.T;
    if (with_obs && (uint64_t)n_observes != rows)
        return fail(c, CPPROB_HIP_EINVAL, "n_observes = " + std::to_string(n_observes) + ", the problems' lengths sum to " + std::to_string(rows));
    need = (uint64_t)bs->cfg.n_problems * n_traj * (uint64_t)kTrajStats;
    if (n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "the statistics buffer is too small: " + std::to_string(need) + " doubles (88 a trajectory, n_problems * n_traj of them)");
    return 0;
}

int cpprob_hip_batch_traj_stats_device(cpprob_hip_ctx* c, uint64_t n_traj, uint64_t draw_index, const double* d_observes, size_t n_observes, double* d_stats,
                                       size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t rows = 0, need = 0;
    if (int rc = batch_traj_stats_check(c, n_traj, draw_index, d_observes != nullptr, n_observes, d_stats, n_doubles, rows, need)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_smooth_enqueue(c, BatchPass::traj_stats(n_traj, draw_index, rows ? d_observes : nullptr, d_stats));
}

int cpprob_hip_batch_traj_stats(cpprob_hip_ctx* c, uint64_t n_traj, uint64_t draw_index, const double* h_observes, size_t n_observes, double* h_stats, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t rows = 0, need = 0;
    if (int rc = batch_traj_stats_check(c, n_traj, draw_index, h_observes != nullptr, n_observes, h_stats, n_doubles, rows, need)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    double *d_stats = nullptr, *d_obs = nullptr;
    if (int rc = batch_stage_observes(c, (size_t)need, h_observes, (size_t)rows, d_stats, d_obs)) return rc;
    if (int rc = batch_smooth_enqueue(c, BatchPass::traj_stats(n_traj, draw_index, d_obs, d_stats))) return rc;
    return batch_fetch(c, nullptr, nullptr, 0, h_stats, d_stats, (size_t)need);
}

// ---- forecasts of a batch (csrc/batch_forecast.hpp) ---------------------------------------------------------------------------------
// cpprob_hip_batch_forecast's arguments against the batch's state (batch_smooth_check first), then the totals against the capacities.
static int batch_forecast_check(cpprob_hip_ctx* c, uint64_t horizon, uint64_t n_traj, uint64_t draw_index, bool with_marg, size_t n_doubles, bool with_traj,
                                size_t n_entries, uint64_t& doubles, uint64_t& entries)
{
    uint64_t full_doubles = 0, full_entries = 0;
    if (int rc = batch_smooth_check(c, n_traj, draw_index, false, 0, false, 0, full_doubles, full_entries)) return rc;
    if (horizon == 0 || horizon >= (uint64_t)kForecastMaxH) return fail(c, CPPROB_HIP_EINVAL, "horizon must lie in 1 .. 2^24 - 1");
    BatchState* bs = c->batch;
    doubles = (uint64_t)bs->cfg.n_problems * horizon * (uint64_t)bs->K;
    entries = (uint64_t)bs->cfg.n_problems * (horizon + 1) * n_traj;
    if (with_marg && n_doubles < doubles) return fail(c, CPPROB_HIP_EINVAL, "the marginals buffer is too small: " + std::to_string(doubles) + " doubles (n_problems * horizon * stats_per_predict)");
    if (with_traj && n_entries < entries) return fail(c, CPPROB_HIP_EINVAL, "the trajectories buffer is too small: " + std::to_string(entries) + " entries (n_problems * (horizon + 1) * n_traj)");
    return 0;
}

int cpprob_hip_batch_forecast_device(cpprob_hip_ctx* c, uint64_t horizon, uint64_t n_traj, uint64_t draw_index, double* d_marginals, size_t n_doubles,
                                     int8_t* d_traj, size_t n_entries)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t doubles = 0, entries = 0;
    if (int rc = batch_forecast_check(c, horizon, n_traj, draw_index, d_marginals != nullptr, n_doubles, d_traj != nullptr, n_entries, doubles, entries)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_smooth_enqueue(c, BatchPass::forecast(horizon, n_traj, draw_index, d_marginals, d_traj));
}

int cpprob_hip_batch_forecast(cpprob_hip_ctx* c, uint64_t horizon, uint64_t n_traj, uint64_t draw_index, double* h_marginals, size_t n_doubles,
                              int32_t* h_traj, size_t n_entries)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t doubles = 0, entries = 0;
    if (int rc = batch_forecast_check(c, horizon, n_traj, draw_index, h_marginals != nullptr, n_doubles, h_traj != nullptr, n_entries, doubles, entries)) return rc;
    const bool with_traj = h_traj && entries;
    if (!h_marginals && !with_traj) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_pass_rows_host(c, BatchPass::forecast(horizon, n_traj, draw_index, nullptr, nullptr), h_marginals, h_marginals ? (size_t)doubles : 0, h_traj,
                                with_traj ? (size_t)entries : 0);
}

// cpprob_hip_batch_predictive's arguments against the batch's state (batch_smooth_check first).
static int batch_predictive_check(cpprob_hip_ctx* c, const uint32_t* h_from, uint64_t n_rows, const double* rows, size_t n_doubles, uint64_t& doubles)
{
    uint64_t full_doubles = 0, full_entries = 0;
    if (int rc = batch_smooth_check(c, 0, 0, false, 0, false, 0, full_doubles, full_entries)) return rc;
    if (!rows) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    for (size_t b = 0; b < bs->prob.size(); ++b) {
        const uint64_t L = (uint64_t)bs->prob[b].T, from = h_from ? h_from[b] : 0;
        if (from > L + 1) return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": from = " + std::to_string(from) + " lies past its " + std::to_string(L + 1) + " predictive rows");
        if (L + 1 - from > n_rows)
            return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": " + std::to_string(L + 1 - from) + " rows asked for, n_rows = " + std::to_string(n_rows));
    }
    doubles = (uint64_t)bs->cfg.n_problems * n_rows * (uint64_t)bs->K;
    if (n_doubles < doubles) return fail(c, CPPROB_HIP_EINVAL, "the rows buffer is too small: " + std::to_string(doubles) + " doubles (n_problems * n_rows * stats_per_predict)");
    return 0;
}

int cpprob_hip_batch_predictive_device(cpprob_hip_ctx* c, const uint32_t* h_from, uint64_t n_rows, double* d_rows, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t doubles = 0;
    if (int rc = batch_predictive_check(c, h_from, n_rows, d_rows, n_doubles, doubles)) return rc;
    if (doubles == 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_smooth_enqueue(c, BatchPass::predictive(h_from, n_rows, d_rows));
}

int cpprob_hip_batch_predictive(cpprob_hip_ctx* c, const uint32_t* h_from, uint64_t n_rows, double* h_rows, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    uint64_t doubles = 0;
    if (int rc = batch_predictive_check(c, h_from, n_rows, h_rows, n_doubles, doubles)) return rc;
    if (doubles == 0) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_pass_rows_host(c, BatchPass::predictive(h_from, n_rows, nullptr), h_rows, (size_t)doubles, nullptr, 0);
}

// ---- decoding a batch (csrc/batch_decode.hpp) ---------------------------------------------------------------------------------------
// The log tables of the batch last begun, on the host: one a problem (a described CPPROB_HIP_MODEL_HMM_TABLE batch) or one for all.
// (After a device-form re-table the thresholds are the device's: fetched once, which waits for the stream.)
static int batch_decode_table(cpprob_hip_ctx* c)
{
    BatchState* bs = c->batch;
    if (bs->lp_ready) return 0;
    if (bs->thr_stale) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipMemcpyAsync(bs->h_thr.data(), bs->ws() + bs->lay.thr, bs->h_thr.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        bs->thr_stale = false;
    }
    const bool hmm3 = bs->cfg.model == CPPROB_HIP_MODEL_HMM3;
    const size_t tables = hmm3 ? 1 : bs->h_thr.size() / 64;
    bs->h_lp.assign(tables * 64, 0.0);
    uint64_t h3[64];
    for (int i = 0; i < 64; ++i) h3[i] = ~0ull;
    for (int s2 = 0; s2 < 3; ++s2) for (int j = 0; j < 2; ++j) h3[s2 * 8 + j] = bs->mp.hmm_thr[s2][j];
    for (size_t i = 0; i < tables; ++i) decode_log_table(hmm3 ? h3 : bs->h_thr.data() + i * 64, hmm3 ? 3 : bs->hk, bs->h_lp.data() + i * 64, &bs->lp0);
    bs->lp_ready = true;
    return 0;
}

// The decode's own allocations for word_rows step words, and the log tables' upload (once a begin).  Where a buffer has to grow it
// waits for the calls before it, and the words kept so far go with it.
static int batch_decode_prepare(cpprob_hip_ctx* c, size_t word_rows)
{
    BatchState* bs = c->batch;
    const size_t B = bs->cfg.n_problems;
    if (int rc = batch_decode_table(c)) return rc;
    const size_t tables = bs->h_lp.size() / 64;
    bool grew = false;                                                      // (what went with a block is forgotten before a failed allocation returns)
    const hipError_t words_grow = bs->d_words.grow(c->stream, word_rows * sizeof(uint32_t), &grew);
    if (grew) bs->decoded.assign(B, 0);
    HIP_TRY(c, words_grow);
    const hipError_t v_grow = bs->d_v.grow(c->stream, B * 8 * sizeof(double), &grew);
    if (grew) bs->decoded.assign(B, 0);
    HIP_TRY(c, v_grow);
    const hipError_t lp_grow = bs->d_lp.grow(c->stream, tables * 64 * sizeof(double), &grew);
    if (grew) bs->lp_sent = false;
    HIP_TRY(c, lp_grow);
    if (!bs->lp_sent) {
        HIP_TRY(c, hipMemcpyAsync(bs->d_lp.as<double>(), bs->h_lp.data(), bs->h_lp.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        bs->lp_sent = true;
    }
    return 0;
}

// A decode call's arguments against the batch's state (batch_smooth_check first), then the totals against the capacities.
static int batch_decode_check(cpprob_hip_ctx* c, bool full, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, bool with_path, size_t n_entries,
                              bool with_score, size_t n_doubles, uint64_t& entries)
{
    uint64_t full_doubles = 0, full_entries = 0;
    if (int rc = batch_smooth_check(c, 0, 0, false, 0, false, 0, full_doubles, full_entries)) return rc;
    BatchState* bs = c->batch;
    entries = 0;
    if (full) {
        for (const BatchProblem& pr : bs->prob) entries += (uint64_t)pr.T;
        if (with_path && n_entries < entries) return fail(c, CPPROB_HIP_EINVAL, "the path buffer is too small: " + std::to_string(entries) + " entries (cpprob_hip_batch_smooth_layout with n_traj = 1)");
    } else {
        if (lag > (uint64_t)kBackwardMaxT) return fail(c, CPPROB_HIP_EINVAL, "lag must lie in 0 .. 2^24");
        if (n_rows > (uint64_t)INT32_MAX) return fail(c, CPPROB_HIP_EINVAL, "n_rows must lie in 0 .. 2^31 - 1");
        for (size_t b = 0; b < bs->prob.size(); ++b) {
            const uint64_t L = (uint64_t)bs->prob[b].T, from = h_from ? h_from[b] : 0;
            if (from > L) return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": from = " + std::to_string(from) + " lies past its length of " + std::to_string(L));
            if (with_path && L - from > n_rows)
                return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + ": " + std::to_string(L - from) + " rows asked for, n_rows = " + std::to_string(n_rows));
        }
        entries = (uint64_t)bs->cfg.n_problems * n_rows;
        if (with_path && n_entries < entries) return fail(c, CPPROB_HIP_EINVAL, "the states buffer is too small: " + std::to_string(entries) + " entries (n_problems * n_rows)");
    }
    if (with_score && n_doubles < (size_t)bs->cfg.n_problems) return fail(c, CPPROB_HIP_EINVAL, "the score buffer is too small: " + std::to_string(bs->cfg.n_problems) + " doubles (one a problem)");
    return 0;
}

// Both calls' device forms (dc.d_score, dc.d_path: device buffers or nullptr).
static int batch_decode_device(cpprob_hip_ctx* c, BatchPass dc, size_t n_entries, size_t n_doubles)
{
    uint64_t entries = 0;
    if (int rc = batch_decode_check(c, dc.kind == BatchPass::Decode, dc.lag, dc.from, dc.n_rows, dc.d_path != nullptr, n_entries, dc.d_score != nullptr, n_doubles, entries)) return rc;
    if (entries == 0) dc.d_path = nullptr;
    if (!dc.d_path && !dc.d_score) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_smooth_enqueue(c, dc);
}

// Both calls' host forms: staged on the device (the scores in front of the int8 entries), the entries widened.
static int batch_decode_host(cpprob_hip_ctx* c, BatchPass dc, int32_t* h_path, size_t n_entries, double* h_score, size_t n_doubles)
{
    uint64_t entries = 0;
    if (int rc = batch_decode_check(c, dc.kind == BatchPass::Decode, dc.lag, dc.from, dc.n_rows, h_path != nullptr, n_entries, h_score != nullptr, n_doubles, entries)) return rc;
    const bool with_path = h_path && entries;
    if (!with_path && !h_score) return 0;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_score = h_score ? (size_t)c->batch->cfg.n_problems : 0, n_path = with_path ? (size_t)entries : 0;
    if (int rc = batch_stage(c, batch_round(n_score * sizeof(double)), n_path, dc.d_score, dc.d_path)) return rc;
    if (int rc = batch_smooth_enqueue(c, dc)) return rc;
    return batch_fetch(c, h_path, dc.d_path, n_path, h_score, dc.d_score, n_score);
}

int cpprob_hip_batch_decode_device(cpprob_hip_ctx* c, int8_t* d_path, size_t n_entries, double* d_score, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    return batch_decode_device(c, BatchPass::decode(d_score, d_path), n_entries, n_doubles);
}

int cpprob_hip_batch_decode(cpprob_hip_ctx* c, int32_t* h_path, size_t n_entries, double* h_score, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    return batch_decode_host(c, BatchPass::decode(nullptr, nullptr), h_path, n_entries, h_score, n_doubles);
}

int cpprob_hip_batch_decode_lag_device(cpprob_hip_ctx* c, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, int8_t* d_states, size_t n_entries,
                                       double* d_score, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    return batch_decode_device(c, BatchPass::decode_lag(lag, h_from, n_rows, d_score, d_states), n_entries, n_doubles);
}

int cpprob_hip_batch_decode_lag(cpprob_hip_ctx* c, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, int32_t* h_states, size_t n_entries,
                                double* h_score, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    return batch_decode_host(c, BatchPass::decode_lag(lag, h_from, n_rows, nullptr, nullptr), h_states, n_entries, h_score, n_doubles);
}

int cpprob_hip_batch_decode_logp(cpprob_hip_ctx* c, uint64_t problem, double* h_lp, double* h_lp0)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "no batch begun");
    if (!h_lp || !h_lp0) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (problem >= bs->cfg.n_problems) return fail(c, CPPROB_HIP_EINVAL, "problem index out of range");
    if (int rc = batch_decode_table(c)) return rc;
    const size_t tables = bs->h_lp.size() / 64;
    std::memcpy(h_lp, bs->h_lp.data() + (tables > 1 ? (size_t)problem * 64 : 0), 64 * sizeof(double));
    *h_lp0 = bs->lp0;
    return 0;
}

int cpprob_hip_batch_smooth_grid(cpprob_hip_ctx* c, uint32_t* count_grid_y, uint32_t* lag_grid_y)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!count_grid_y || !lag_grid_y) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    *count_grid_y = c->batch ? c->batch->smooth_gy_count : 0u;
    *lag_grid_y = c->batch ? c->batch->smooth_gy_lag : 0u;
    return 0;
}

int cpprob_hip_batch_traj_stats_grid(cpprob_hip_ctx* c, uint32_t* grid_y)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!grid_y) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    *grid_y = c->batch ? c->batch->traj_stats_gy : 0u;
    return 0;
}

int cpprob_hip_batch_pass_grid(cpprob_hip_ctx* c, uint32_t* decode_forward_grid_x, uint32_t* decode_trace_grid_y, uint32_t* forecast_grid_y, uint32_t* predictive_grid_y)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!decode_forward_grid_x || !decode_trace_grid_y || !forecast_grid_y || !predictive_grid_y) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    const BatchState* bs = c->batch;
    *decode_forward_grid_x = bs ? bs->decode_gx_forward : 0u;
    *decode_trace_grid_y = bs ? bs->decode_gy_trace : 0u;
    *forecast_grid_y = bs ? bs->forecast_gy : 0u;
    *predictive_grid_y = bs ? bs->predictive_gy : 0u;
    return 0;
}
// ---- re-tabling a begun batch (csrc/batch_retable.hpp) -----------------------------------------------------------------------------
static_assert(kRetableStats == kSuffStats, "the M-step reads the record of cpprob_hip_batch_smooth_stats");
// What a re-table needs of the batch's state, then n_observes against the lengths; nothing is enqueued before it has passed.
static int batch_retable_check(cpprob_hip_ctx* c, size_t n_observes, EmissionFamily family)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "no batch is begun");
    if (bs->online) return fail(c, CPPROB_HIP_EUNSUPPORTED, "an online batch is not re-tabled: its advances evaluate their rows from the host's means");
    if (bs->cfg.model != CPPROB_HIP_MODEL_HMM_TABLE) return fail(c, CPPROB_HIP_EUNSUPPORTED, "re-tabling serves CPPROB_HIP_MODEL_HMM_TABLE: the table of CPPROB_HIP_MODEL_HMM3 is the model's");
    if (!bs->described) return fail(c, CPPROB_HIP_EUNSUPPORTED, "a batch begun by cpprob_hip_batch_begin shares one table: begin it with cpprob_hip_batch_begin_problems to re-table it");
    const bool scaled = family == kFamilyScaled, poisson = family == kFamilyPoisson;
    if (bs->poisson && !poisson) return fail(c, CPPROB_HIP_ESTATE, "the batch has Poisson emissions: it is re-tabled by cpprob_hip_batch_retable_poisson / _retable_poisson_device");
    if (!bs->poisson && poisson) return fail(c, CPPROB_HIP_ESTATE, "the batch has no Poisson emissions: begin it with cpprob_hip_batch_begin_problems_poisson, or re-table it with its own family's calls");
    if (bs->scaled && !scaled) return fail(c, CPPROB_HIP_ESTATE, "the batch has emission scales: it is re-tabled by cpprob_hip_batch_retable_scaled / _retable_scaled_device");
    if (!bs->scaled && scaled) return fail(c, CPPROB_HIP_ESTATE, "the batch has no emission scales: begin it with cpprob_hip_batch_begin_problems_scaled, or re-table it with cpprob_hip_batch_retable / _retable_device");
    uint64_t rows = 0;
    for (const BatchProblem& pr : bs->prob) rows += (uint64_t)pr.T;
    if ((uint64_t)n_observes != rows) return fail(c, CPPROB_HIP_EINVAL, "n_observes = " + std::to_string(n_observes) + ", the problems' lengths sum to " + std::to_string(rows));
    return 0;
}

// Enqueues the first entries (once a begin) and the launch (d_sigmas given: a scaled batch's; a Poisson batch: its own, d_means the
// rates); the batch then stands as after a begin.
// Waits for nothing but, where the status words have to grow, for the calls before it.
static int batch_retable_enqueue(cpprob_hip_ctx* c, const double* d_means, const double* d_trans, const double* d_obs, const double* d_sigmas)
{
    BatchState* bs = c->batch;
    const size_t B = bs->cfg.n_problems;
    HIP_TRY(c, bs->d_rstatus.grow(c->stream, B * sizeof(int32_t)));
    if (int rc = batch_first_entries(c)) return rc;
    const unsigned gy = retable_grid_y(bs->T, (int64_t)B);
    auto common = [&](auto& r) {                                // (what the two forms' arguments share)
        r.prob = reinterpret_cast<const BatchProblem*>(bs->ws() + bs->lay.prob);
        r.first = bs->d_cfirst.as<int64_t>();
        r.trans = d_trans; r.obs = d_obs;
        r.tab = reinterpret_cast<double*>(bs->ws() + bs->lay.tab);
        r.thr = reinterpret_cast<uint64_t*>(bs->ws() + bs->lay.thr);
        r.status = bs->d_rstatus.as<int32_t>();
        r.T_max = bs->T; r.k = bs->hk;
    };
    if (bs->poisson) {
        // (a Poisson batch: d_means are its rates; the rates and log-rates in force are the device's from here on)
        BatchRetablePoissonArgs pa{};
        common(pa);
        pa.rates = d_means; pa.lfact = bs->d_lfact.as<double>(); pa.rate_out = bs->d_sigma.as<double>(); pa.log_rate_out = bs->d_lognorm.as<double>();
        hipLaunchKernelGGL(batch_retable_poisson_kernel, dim3((unsigned)B, gy), dim3(kThreads), 0, c->stream, pa);
    } else if (d_sigmas) {
        // (a scaled batch; the sigmas and log_norms in force are the device's from here on)
        BatchRetableScaledArgs sa{};
        common(sa);
        sa.means = d_means; sa.sigmas = d_sigmas; sa.sigma_out = bs->d_sigma.as<double>(); sa.log_norm_out = bs->d_lognorm.as<double>();
        hipLaunchKernelGGL(batch_retable_scaled_kernel, dim3((unsigned)B, gy), dim3(kThreads), 0, c->stream, sa);
    } else {
        BatchRetableArgs a{};
        common(a);
        a.means = d_means;
        a.log_norm = std::log(2 * kPi * 1.0 * 1.0);               // (normal_logpdf's own expression at sigma = 1.0)
        hipLaunchKernelGGL(batch_retable_kernel, dim3((unsigned)B, gy), dim3(kThreads), 0, c->stream, a);
    }
    HIP_TRY(c, hipGetLastError());
    bs->retable_gy = gy; bs->retabled = true;
    // a begin as far as results go: the read-outs wait for the next run; the decode's log tables come from the thresholds
    bs->ran = false; bs->conditional = false;
    bs->lp_ready = false; bs->lp_sent = false;
    bs->tab_stale = true; bs->thr_stale = true;
    return 0;
}

// The three device forms (scaled: cpprob_hip_batch_retable_scaled_device, whose d_sigmas the others do not have; Poisson:
// cpprob_hip_batch_retable_poisson_device, whose d_means are rates): enqueued, no wait.  The unit and the scaled entry points pass
// their flag as they always did; the Poisson one passes poisson behind it.
static int batch_retable_device(cpprob_hip_ctx* c, const double* d_means, const double* d_transition, const double* d_sigmas, const double* d_observes, size_t n_observes,
                                bool scaled, bool poisson = false)
{
    const EmissionFamily family = poisson ? kFamilyPoisson : scaled ? kFamilyScaled : kFamilyUnit;
    if (int rc = batch_retable_check(c, n_observes, family)) return rc;
    if (!d_means || !d_transition || (scaled && !d_sigmas) || !d_observes) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_retable_enqueue(c, d_means, d_transition, d_observes, d_sigmas);
}

// The observes of a host re-table in the buffer of the context's own, where a later re-table without observes finds them.
static int batch_retable_observes(cpprob_hip_ctx* c, const double* h_observes, size_t n_observes)
{
    BatchState* bs = c->batch;
    bool grew = false;
    const hipError_t robs_grow = bs->d_robs.grow(c->stream, n_observes * sizeof(double), &grew);      // (an earlier re-table may still read the buffer this replaces)
    if (grew) bs->robs_ready = false;                          // (before a failed allocation returns: the observes went with the block)
    HIP_TRY(c, robs_grow);
    HIP_TRY(c, hipMemcpyAsync(bs->d_robs.as<double>(), h_observes, n_observes * sizeof(double), hipMemcpyHostToDevice, c->stream));
    bs->robs_ready = true;
    return 0;
}

// The three host forms (scaled: cpprob_hip_batch_retable_scaled; Poisson: cpprob_hip_batch_retable_poisson, h_means its rates): the
// tables are validated with the begin's own statements, staged -- the means, a scaled batch's sigmas behind them, in front; the
// transition rows at the back -- and re-tabled as by the device form.
static int batch_retable_host(cpprob_hip_ctx* c, const double* h_means, const double* h_transition, const double* h_sigmas, const double* h_observes, size_t n_observes,
                              bool scaled, bool poisson = false)
{
    const EmissionFamily family = poisson ? kFamilyPoisson : scaled ? kFamilyScaled : kFamilyUnit;
    if (int rc = batch_retable_check(c, n_observes, family)) return rc;
    BatchState* bs = c->batch;
    if (!h_means || !h_transition || (scaled && !h_sigmas)) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (!h_observes && !bs->robs_ready) return fail(c, CPPROB_HIP_EINVAL, "h_observes is NULL and no re-table of this begun batch has staged the observes");
    int k = 0;
    if (int rc = batch_check_tables(c, &bs->cfg, (int32_t)bs->hk, h_means, h_transition, k, poisson)) return rc;
    if (scaled) if (int rc = batch_check_scales(c, bs->cfg.n_problems, k, h_sigmas)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t B = bs->cfg.n_problems, kk = (size_t)k * k;
    if (h_observes) if (int rc = batch_retable_observes(c, h_observes, n_observes)) return rc;
    double *d_means = nullptr, *d_trans = nullptr;
    if (int rc = batch_stage(c, batch_round((scaled ? 2 : 1) * B * (size_t)k * sizeof(double)), B * kk * sizeof(double), d_means, d_trans)) return rc;
    double* d_sigmas = scaled ? d_means + B * (size_t)k : nullptr;
    HIP_TRY(c, hipMemcpyAsync(d_means, h_means, B * (size_t)k * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (scaled) HIP_TRY(c, hipMemcpyAsync(d_sigmas, h_sigmas, B * (size_t)k * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_trans, h_transition, B * kk * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (int rc = batch_retable_enqueue(c, d_means, d_trans, bs->d_robs.as<double>(), d_sigmas)) return rc;
    // the host knows the tables: the thresholds' mirror is current again (the rows' is not: cpprob_hip_batch_copy_store fetches its row)
    for (size_t b = 0; b < B; ++b) retable_thresholds(h_transition + b * kk, k, bs->h_thr.data() + b * 64);
    if (scaled) batch_mirror_scales(bs, B, k, h_sigmas);
    if (poisson) batch_mirror_rates(bs, B, k, h_means);
    bs->thr_stale = false;
    return 0;
}

int cpprob_hip_batch_retable_device(cpprob_hip_ctx* c, const double* d_means, const double* d_transition, const double* d_observes, size_t n_observes)
{
    LANES_OWN(c);
    return batch_retable_device(c, d_means, d_transition, nullptr, d_observes, n_observes, false);
}

int cpprob_hip_batch_retable_poisson_device(cpprob_hip_ctx* c, const double* d_rates, const double* d_transition, const double* d_observes, size_t n_observes)
{
    LANES_OWN(c);
    return batch_retable_device(c, d_rates, d_transition, nullptr, d_observes, n_observes, false, true);
}

int cpprob_hip_batch_retable_scaled_device(cpprob_hip_ctx* c, const double* d_means, const double* d_transition, const double* d_sigmas, const double* d_observes, size_t n_observes)
{
    LANES_OWN(c);
    return batch_retable_device(c, d_means, d_transition, d_sigmas, d_observes, n_observes, true);
}

int cpprob_hip_batch_retable(cpprob_hip_ctx* c, const double* h_means, const double* h_transition, const double* h_observes, size_t n_observes)
{
    LANES_OWN(c);
    return batch_retable_host(c, h_means, h_transition, nullptr, h_observes, n_observes, false);
}

int cpprob_hip_batch_retable_poisson(cpprob_hip_ctx* c, const double* h_rates, const double* h_transition, const double* h_observes, size_t n_observes)
{
    LANES_OWN(c);
    return batch_retable_host(c, h_rates, h_transition, nullptr, h_observes, n_observes, false, true);
}

int cpprob_hip_batch_retable_scaled(cpprob_hip_ctx* c, const double* h_means, const double* h_transition, const double* h_sigmas, const double* h_observes, size_t n_observes)
{
    LANES_OWN(c);
    return batch_retable_host(c, h_means, h_transition, h_sigmas, h_observes, n_observes, true);
}

int cpprob_hip_batch_retable_status(cpprob_hip_ctx* c, int32_t* h_status)
{
    LANES_OWN(c);
    if (!c || !h_status) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun || !bs->retabled) return fail(c, CPPROB_HIP_ESTATE, "the begun batch has not been re-tabled");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(h_status, bs->d_rstatus.as<int32_t>(), bs->cfg.n_problems * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

int cpprob_hip_batch_retable_grid(cpprob_hip_ctx* c, uint32_t* grid_y)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    if (!grid_y) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    *grid_y = c->batch ? c->batch->retable_gy : 0u;
    return 0;
}

// cpprob_hip_batch_mstep_device and -- scaled: the sigmas (and, where given, the log_norms) are fitted too, above sigma_floor --
// cpprob_hip_batch_mstep_scaled_device; Poisson: d_means are rates, kept at or above sigma_floor (the call's rate_floor), d_log_norm
// their logarithms where given -- cpprob_hip_batch_mstep_poisson_device.
static int batch_mstep_device(cpprob_hip_ctx* c, const double* d_stats, size_t n_doubles, double* d_means, double* d_transition, EmissionFamily family, double* d_sigmas,
                              double* d_log_norm, double sigma_floor)
{
    const bool scaled = family == kFamilyScaled, poisson = family == kFamilyPoisson;
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "no batch is begun");
    if (bs->cfg.model != CPPROB_HIP_MODEL_HMM_TABLE) return fail(c, CPPROB_HIP_EUNSUPPORTED, "the M-step fits the tables of CPPROB_HIP_MODEL_HMM_TABLE");
    if (bs->poisson && !poisson) return fail(c, CPPROB_HIP_ESTATE, "the batch has Poisson emissions: its M-step is cpprob_hip_batch_mstep_poisson_device");
    if (!bs->poisson && poisson) return fail(c, CPPROB_HIP_ESTATE, "the batch has no Poisson emissions: its M-step is cpprob_hip_batch_mstep_device / _mstep_scaled_device");
    if (!d_stats || !d_means || !d_transition || (scaled && !d_sigmas)) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (scaled && (!(sigma_floor > 0.0) || !std::isfinite(sigma_floor))) return fail(c, CPPROB_HIP_EINVAL, "sigma_floor must be finite and > 0");
    if (poisson && (!(sigma_floor > 0.0) || !std::isfinite(sigma_floor))) return fail(c, CPPROB_HIP_EINVAL, "rate_floor must be finite and > 0");
    const uint64_t B = bs->cfg.n_problems, need = B * (uint64_t)kRetableStats;
    if (n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "the statistics buffer is too small: " + std::to_string(need) + " doubles (88 a problem)");
    HIP_TRY(c, hipSetDevice(c->device));
    const dim3 grid((unsigned)((B * (uint64_t)bs->hk + kThreads - 1) / kThreads));
    if (scaled) {
        BatchMstepScaledArgs a{};
        a.stats = d_stats; a.means = d_means; a.trans = d_transition; a.sigmas = d_sigmas; a.log_norms = d_log_norm; a.floor = sigma_floor; a.B = (int64_t)B; a.k = bs->hk;
        hipLaunchKernelGGL(batch_mstep_scaled_kernel, grid, dim3(kThreads), 0, c->stream, a);
    } else if (poisson) {
        BatchMstepPoissonArgs a{};
        a.stats = d_stats; a.rates = d_means; a.trans = d_transition; a.log_rates = d_log_norm; a.floor = sigma_floor; a.B = (int64_t)B; a.k = bs->hk;
        hipLaunchKernelGGL(batch_mstep_poisson_kernel, grid, dim3(kThreads), 0, c->stream, a);
    } else {
        BatchMstepArgs a{};
        a.stats = d_stats; a.means = d_means; a.trans = d_transition; a.B = (int64_t)B; a.k = bs->hk;
        hipLaunchKernelGGL(batch_mstep_kernel, grid, dim3(kThreads), 0, c->stream, a);
    }
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_batch_mstep_device(cpprob_hip_ctx* c, const double* d_stats, size_t n_doubles, double* d_means, double* d_transition)
{
    return batch_mstep_device(c, d_stats, n_doubles, d_means, d_transition, kFamilyUnit, nullptr, nullptr, 0.0);
}

int cpprob_hip_batch_mstep_poisson_device(cpprob_hip_ctx* c, const double* d_stats, size_t n_doubles, double* d_rates, double* d_transition, double* d_log_rates,
                                          double rate_floor)
{
    return batch_mstep_device(c, d_stats, n_doubles, d_rates, d_transition, kFamilyPoisson, nullptr, d_log_rates, rate_floor);
}

int cpprob_hip_batch_mstep_scaled_device(cpprob_hip_ctx* c, const double* d_stats, size_t n_doubles, double* d_means, double* d_transition, double* d_sigmas,
                                         double* d_log_norm, double sigma_floor)
{
    return batch_mstep_device(c, d_stats, n_doubles, d_means, d_transition, kFamilyScaled, d_sigmas, d_log_norm, sigma_floor);
}

// ---- tied tables: a partition of the begun batch's problems and the pooled records of its groups (csrc/batch_pool.hpp) -------------
static_assert(kPoolStats == kSuffStats, "the pooling kernel sums the record of cpprob_hip_batch_smooth_stats");

int cpprob_hip_batch_tie(cpprob_hip_ctx* c, const int32_t* h_group, size_t n)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "no batch is begun");
    if (bs->learn_tied) return fail(c, CPPROB_HIP_ESTATE, "the batch's learner pools over the tie in force (cpprob_hip_batch_learn_tie): arm it again before a new tie");
    if (!h_group) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    const size_t B = bs->cfg.n_problems;
    if (n != B) return fail(c, CPPROB_HIP_EINVAL, "n = " + std::to_string(n) + ", the begun batch has " + std::to_string(B) + " problems");
    int64_t G = 0;
    for (size_t b = 0; b < B; ++b) {
        if (h_group[b] < 0) return fail(c, CPPROB_HIP_EINVAL, "problem " + std::to_string(b) + " has the negative group id " + std::to_string(h_group[b]));
        G = std::max<int64_t>(G, (int64_t)h_group[b] + 1);
    }
    if (G > (int64_t)B) return fail(c, CPPROB_HIP_EINVAL, "a group id in 0 .. " + std::to_string(G - 1) + " is unused: every id must occur");
    // a counting sort by group: within a group the members stay in ascending problem order
    std::vector<int32_t> h((size_t)B + (size_t)G + 1 + (size_t)B, 0);
    int32_t *members = h.data(), *first = h.data() + B, *map = first + G + 1;
    for (size_t b = 0; b < B; ++b) ++first[h_group[b] + 1];
    for (int64_t g = 0; g < G; ++g) {
        if (first[g + 1] == 0) return fail(c, CPPROB_HIP_EINVAL, "the group id " + std::to_string(g) + " is unused: every id in 0 .. " + std::to_string(G - 1) + " must occur");
        first[g + 1] += first[g];
    }
    std::vector<int32_t> at(first, first + G);
    for (size_t b = 0; b < B; ++b) { members[at[(size_t)h_group[b]]++] = (int32_t)b; map[b] = h_group[b]; }
    HIP_TRY(c, hipSetDevice(c->device));
    // (a pooling launch of the tie this one replaces may still read the arrays)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    bs->tied = false;
    HIP_TRY(c, bs->d_tie.grow(c->stream, h.size() * sizeof(int32_t)));
    HIP_TRY(c, hipMemcpyAsync(bs->d_tie.as<int32_t>(), h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    bs->tie_map.assign(map, map + B);
    bs->tie_groups = (int32_t)G;
    bs->tied = true;
    return 0;
}

int cpprob_hip_batch_tie_get(cpprob_hip_ctx* c, int32_t* h_group, int32_t* n_groups)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun || !bs->tied) return fail(c, CPPROB_HIP_ESTATE, "the begun batch has no tie");
    if (!n_groups) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (h_group) std::copy(bs->tie_map.begin(), bs->tie_map.end(), h_group);
    *n_groups = bs->tie_groups;
    return 0;
}

// cpprob_hip_batch_pool_stats' arguments against the batch's state; doubles: the records' size, out_doubles: the output's.  It writes nothing.
static int batch_pool_check(cpprob_hip_ctx* c, const double* records, size_t n_doubles, uint32_t per_problem, int broadcast, const double* out, size_t n_out,
                            uint64_t& doubles, uint64_t& out_doubles)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "no batch is begun");
    if (!bs->tied) return fail(c, CPPROB_HIP_ESTATE, "the begun batch has no tie: cpprob_hip_batch_tie sets one");
    if (!records || !out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (per_problem == 0) return fail(c, CPPROB_HIP_EINVAL, "per_problem must be >= 1");
    const uint64_t B = bs->cfg.n_problems, G = (uint64_t)bs->tie_groups, R = per_problem, per = (uint64_t)kPoolStats * R;
    if (G * R > (uint64_t)INT32_MAX) return fail(c, CPPROB_HIP_EINVAL, "groups x per_problem = " + std::to_string(G * R) + " is beyond one launch's grid");
    doubles = B * per;
    out_doubles = (broadcast ? B : G) * per;
    if ((uint64_t)n_doubles < doubles) return fail(c, CPPROB_HIP_EINVAL, "the records are too small: " + std::to_string(doubles) + " doubles (88 a problem and record)");
    if ((uint64_t)n_out < out_doubles) return fail(c, CPPROB_HIP_EINVAL, "the output is too small: " + std::to_string(out_doubles) + " doubles");
    if (out == records) {
        if (!broadcast) return fail(c, CPPROB_HIP_EINVAL, "the compact form does not pool in place");
    } else if (out < records + doubles && records < out + out_doubles)
        return fail(c, CPPROB_HIP_EINVAL, "the output overlaps the records: in place (d_out == d_records, broadcast) or apart");
    return 0;
}

static int batch_pool_enqueue(cpprob_hip_ctx* c, const double* d_records, uint32_t per_problem, int broadcast, double* d_out)
{
    BatchState* bs = c->batch;
    const size_t B = bs->cfg.n_problems;
    BatchPoolArgs a{};
    a.members = bs->d_tie.as<int32_t>(); a.first = bs->d_tie.as<int32_t>() + B;
    a.rec = d_records; a.out = d_out;
    a.pairs = (int64_t)bs->tie_groups * (int64_t)per_problem; a.R = (int)per_problem; a.broadcast = broadcast ? 1 : 0;
    hipLaunchKernelGGL(batch_pool_stats_kernel, dim3((unsigned)((a.pairs + kWaves - 1) / kWaves)), dim3(kThreads), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

int cpprob_hip_batch_pool_stats_device(cpprob_hip_ctx* c, const double* d_records, size_t n_doubles, uint32_t per_problem, int broadcast, double* d_out, size_t n_out)
{
    LANES_OWN(c);
    uint64_t doubles = 0, out_doubles = 0;
    if (int rc = batch_pool_check(c, d_records, n_doubles, per_problem, broadcast, d_out, n_out, doubles, out_doubles)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    return batch_pool_enqueue(c, d_records, per_problem, broadcast, d_out);
}

int cpprob_hip_batch_pool_stats(cpprob_hip_ctx* c, const double* h_records, size_t n_doubles, uint32_t per_problem, int broadcast, double* h_out, size_t n_out)
{
    LANES_OWN(c);
    uint64_t doubles = 0, out_doubles = 0;
    if (int rc = batch_pool_check(c, h_records, n_doubles, per_problem, broadcast, h_out, n_out, doubles, out_doubles)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    double *d_rec = nullptr, *d_out = nullptr;
    if (int rc = batch_stage(c, (size_t)doubles * sizeof(double), (size_t)out_doubles * sizeof(double), d_rec, d_out)) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_rec, h_records, (size_t)doubles * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (int rc = batch_pool_enqueue(c, d_rec, per_problem, broadcast, d_out)) return rc;
    return batch_fetch(c, nullptr, nullptr, 0, h_out, d_out, (size_t)out_doubles);
}

// ---- emission scales: the logarithm their tables are built with, and the scales in force (csrc/batch_scale.hpp) --------------------
double cpprob_hip_table_log(double x) { return table_log(x); }

int cpprob_hip_batch_copy_scales(cpprob_hip_ctx* c, uint64_t problem, double* h_sigmas, double* h_log_norm)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "no batch is begun");
    if (!bs->scaled) return fail(c, CPPROB_HIP_ESTATE, "the batch has no emission scales (cpprob_hip_batch_begin_problems_scaled, _begin_online_scaled)");
    if (problem >= bs->cfg.n_problems) return fail(c, CPPROB_HIP_EINVAL, "problem index out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t k = (size_t)bs->hk;
    if (h_sigmas) HIP_TRY(c, hipMemcpyAsync(h_sigmas, bs->d_sigma.as<double>() + problem * 8, k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_log_norm) HIP_TRY(c, hipMemcpyAsync(h_log_norm, bs->d_lognorm.as<double>() + problem * 8, k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

int cpprob_hip_batch_copy_rates(cpprob_hip_ctx* c, uint64_t problem, double* h_rates, double* h_log_rates)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "no batch is begun");
    if (!bs->poisson) return fail(c, CPPROB_HIP_ESTATE, "the batch has no Poisson emissions (cpprob_hip_batch_begin_problems_poisson, _begin_online_poisson)");
    if (problem >= bs->cfg.n_problems) return fail(c, CPPROB_HIP_EINVAL, "problem index out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t k = (size_t)bs->hk;
    if (h_rates) HIP_TRY(c, hipMemcpyAsync(h_rates, bs->d_sigma.as<double>() + problem * 8, k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_log_rates) HIP_TRY(c, hipMemcpyAsync(h_log_rates, bs->d_lognorm.as<double>() + problem * 8, k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- online EM of an online batch (csrc/batch_learn.hpp) ----------------------------------------------------------------------------
// What the host route and the arming share: an online CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables.
static int batch_learn_check(cpprob_hip_ctx* c, const char* who)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun || !bs->online) return fail(c, CPPROB_HIP_ESTATE, std::string(who) + " serves a batch begun by cpprob_hip_batch_begin_online");
    if (bs->cfg.model != CPPROB_HIP_MODEL_HMM_TABLE) return fail(c, CPPROB_HIP_EUNSUPPORTED, std::string(who) + " serves CPPROB_HIP_MODEL_HMM_TABLE: the table of CPPROB_HIP_MODEL_HMM3 is the model's");
    if (!bs->own_tables) return fail(c, CPPROB_HIP_EUNSUPPORTED, "the batch was begun with the context's shared table: begin it with per-problem tables to change them");
    return 0;
}

int cpprob_hip_batch_learn_begin(cpprob_hip_ctx* c, const double* h_gamma, size_t n_gamma, uint32_t t_min)
{
    LANES_OWN(c);
    if (int rc = batch_learn_check(c, "cpprob_hip_batch_learn_begin")) return rc;
    BatchState* bs = c->batch;
    if (bs->poisson) return fail(c, CPPROB_HIP_ESTATE, "the batch has Poisson emissions: online EM serves the unit and the scaled batches");
    if (bs->cfg.keep_history != 1 && !batch_masses(&bs->cfg))
        return fail(c, CPPROB_HIP_ESTATE, "a filtering-only batch (keep_history = 0) keeps no masses: begin it with CPPROB_HIP_BATCH_KEEP_MASSES");
    if (bs->advance_ring.count()) return fail(c, CPPROB_HIP_ESTATE, "the online batch has been advanced: cpprob_hip_batch_learn_begin comes before the first advance");
    if (!h_gamma) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    if (n_gamma < (size_t)bs->T) return fail(c, CPPROB_HIP_EINVAL, "n_gamma = " + std::to_string(n_gamma) + " lies below the largest capacity, " + std::to_string(bs->T));
    for (size_t t = 0; t < n_gamma; ++t)
        if (!(h_gamma[t] > 0.0) || !(h_gamma[t] <= 1.0)) return fail(c, CPPROB_HIP_EINVAL, "gamma[" + std::to_string(t) + "] lies outside (0, 1]");
    HIP_TRY(c, hipSetDevice(c->device));
    batch_learn_free(bs);
    const size_t B = bs->cfg.n_problems, k = (size_t)bs->hk;
    HIP_TRY(c, bs->learn.gamma.grow(c->stream, n_gamma * sizeof(double)));
    HIP_TRY(c, bs->learn.means.grow(c->stream, B * k * sizeof(double)));
    HIP_TRY(c, bs->learn.trans.grow(c->stream, B * k * k * sizeof(double)));
    HIP_TRY(c, bs->learn.tau.grow(c->stream, B * (size_t)kOnlineTau * sizeof(double)));
    HIP_TRY(c, bs->learn.rec.grow(c->stream, B * (size_t)kOnlineStats * sizeof(double)));
    HIP_TRY(c, bs->learn.status.grow(c->stream, B * sizeof(int32_t)));
    HIP_TRY(c, bs->learn.first.grow(c->stream, B * sizeof(int64_t)));
    HIP_TRY(c, bs->learn.pin_first.grow(c->stream, B * BatchState::kOnlineSlots * sizeof(int64_t)));
    HIP_TRY(c, hipMemcpyAsync(bs->learn.gamma.as<double>(), h_gamma, n_gamma * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(bs->learn.means.as<double>(), bs->means.data(), B * k * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(bs->learn.trans.as<double>(), bs->trans.data(), B * k * k * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(bs->learn.tau.as<double>(), 0, B * (size_t)kOnlineTau * sizeof(double), c->stream));
    HIP_TRY(c, hipMemsetAsync(bs->learn.rec.as<double>(), 0, B * (size_t)kOnlineStats * sizeof(double), c->stream));
    HIP_TRY(c, hipMemsetAsync(bs->learn.status.as<int32_t>(), 0, B * sizeof(int32_t), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));               // (h_gamma may be reused when the call returns)
    bs->learn_t_min = t_min; bs->armed = true; bs->learn_scales = false; bs->learn_floor = 0.0;
    return 0;
}

// The same arming for a batch with emission scales, whose learner then fits them: its own two checks, then cpprob_hip_batch_learn_begin's
// checks, allocations and uploads; the two words that tell the learn step to fit the scales are set once that has succeeded.  (A
// context serves one thread at a time -- include/cpprob_hip.h --, and LANES_OWN waits for the run lanes, it holds nothing.)
int cpprob_hip_batch_learn_begin_scaled(cpprob_hip_ctx* c, const double* h_gamma, size_t n_gamma, uint32_t t_min, double sigma_floor)
{
    LANES_OWN(c);
    if (int rc = batch_learn_check(c, "cpprob_hip_batch_learn_begin_scaled")) return rc;
    if (c->batch->poisson) return fail(c, CPPROB_HIP_ESTATE, "the batch has Poisson emissions: online EM serves the unit and the scaled batches");
    if (!c->batch->scaled) return fail(c, CPPROB_HIP_ESTATE, "the batch has no emission scales: begin it with cpprob_hip_batch_begin_online_scaled, or arm it with cpprob_hip_batch_learn_begin");
    if (!(sigma_floor > 0.0) || !std::isfinite(sigma_floor)) return fail(c, CPPROB_HIP_EINVAL, "sigma_floor must be finite and > 0");
    if (int rc = cpprob_hip_batch_learn_begin(c, h_gamma, n_gamma, t_min)) return rc;
    c->batch->learn_scales = true; c->batch->learn_floor = sigma_floor;
    return 0;
}

// Tied online EM: the members of every group of the tie in force hold one table bit for bit (sigmas: given on a scaled batch), or
// CPPROB_HIP_EINVAL naming the first problem that differs.  It writes nothing.
static int batch_tied_tables_check(cpprob_hip_ctx* c, const double* means, const double* trans, const double* sigmas, size_t k)
{
    BatchState* bs = c->batch;
    const size_t B = bs->cfg.n_problems;
    std::vector<size_t> lead((size_t)bs->tie_groups, B);
    for (size_t b = 0; b < B; ++b) {
        const size_t g = (size_t)bs->tie_map[b];
        if (lead[g] == B) { lead[g] = b; continue; }
        const size_t a = lead[g];
        const bool same = std::memcmp(means + a * k, means + b * k, k * sizeof(double)) == 0 &&
                          std::memcmp(trans + a * k * k, trans + b * k * k, k * k * sizeof(double)) == 0 &&
                          (!sigmas || std::memcmp(sigmas + a * k, sigmas + b * k, k * sizeof(double)) == 0);
        if (!same)
            return fail(c, CPPROB_HIP_EINVAL, "group " + std::to_string(g) + ": the table of problem " + std::to_string(b) + " differs from that of problem " + std::to_string(a) +
                                                  "; under tied online EM a group's members hold one table");
    }
    return 0;
}

// Tied online EM: the armed batch's learner pools over the tie in force from its first advance on (csrc/batch_learn_tied.hpp).
int cpprob_hip_batch_learn_tie(cpprob_hip_ctx* c)
{
    LANES_OWN(c);
    if (int rc = batch_learn_check(c, "cpprob_hip_batch_learn_tie")) return rc;
    BatchState* bs = c->batch;
    if (!bs->armed) return fail(c, CPPROB_HIP_ESTATE, "the online batch is not armed: call cpprob_hip_batch_learn_begin before cpprob_hip_batch_learn_tie");
    if (!bs->tied) return fail(c, CPPROB_HIP_ESTATE, "the begun batch has no tie: call cpprob_hip_batch_tie before cpprob_hip_batch_learn_tie");
    if (bs->advance_ring.count()) return fail(c, CPPROB_HIP_ESTATE, "the online batch has been advanced: cpprob_hip_batch_learn_tie comes before the first advance");
    const size_t B = bs->cfg.n_problems, k = (size_t)bs->hk;
    std::vector<double> sg;                                     // (the mirror keeps 8 sigmas a problem)
    if (bs->scaled) { sg.resize(B * k); for (size_t b = 0; b < B; ++b) std::copy(bs->sigmas.begin() + (ptrdiff_t)(b * 8), bs->sigmas.begin() + (ptrdiff_t)(b * 8 + k), sg.begin() + (ptrdiff_t)(b * k)); }
    if (int rc = batch_tied_tables_check(c, bs->means.data(), bs->trans.data(), bs->scaled ? sg.data() : nullptr, k)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)bs->tie_groups * kPoolStats * sizeof(double);
    HIP_TRY(c, bs->learn.pooled.grow(c->stream, bytes));
    HIP_TRY(c, hipMemsetAsync(bs->learn.pooled.as<double>(), 0, bytes, c->stream));
    bs->learn_tied = true;
    return 0;
}

// The groups' pooled records [G][88] of the last tied learning advance (none yet: zeros).  Synchronises.
int cpprob_hip_batch_learn_pooled_record(cpprob_hip_ctx* c, double* h_out, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun || !bs->armed || !bs->learn_tied) return fail(c, CPPROB_HIP_ESTATE, "the begun batch's learner does not pool: call cpprob_hip_batch_learn_tie");
    if (!h_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    const size_t need = (size_t)bs->tie_groups * kPoolStats;
    if (n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "the output is too small: " + std::to_string(need) + " doubles (88 a group)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(h_out, bs->learn.pooled.as<double>(), need * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

// The learn step of a learning advance, behind its launch: the prologue of a running-statistics pass that resumes from the lengths
// before the advance (a batch with a particle store: the counting pass over the new rows first), then batch_learn_kernel.  The
// thresholds and, through them, the decode's log tables and step words are the device's from here on.
static int batch_learn_enqueue(cpprob_hip_ctx* c, const uint32_t* before, const double* d_obs)
{
    BatchState* bs = c->batch; const size_t B = bs->cfg.n_problems;
    BatchPassPlan pl; BatchSmoothArgs a{};
    if (int rc = batch_pass_prologue(c, BatchPass::online_stats(d_obs, bs->learn.rec.as<double>()), pl, a, before)) return rc;
    if (pl.done) return 0;
    BatchLearnArgs la{};
    la.desc = a.desc; la.mass = a.mass; la.thr = reinterpret_cast<uint64_t*>(bs->ws() + bs->lay.thr); la.obs = d_obs; la.gamma = bs->learn.gamma.as<double>();
    la.tau = bs->learn.tau.as<double>(); la.stats = bs->learn.rec.as<double>(); la.means = bs->learn.means.as<double>(); la.trans = bs->learn.trans.as<double>(); la.status = bs->learn.status.as<int32_t>();
    la.B = (int)B; la.k = bs->hk; la.t_min = bs->learn_tied ? INT32_MAX : (int)std::min<uint32_t>(bs->learn_t_min, (uint32_t)INT32_MAX);
    BatchLearnScaledArgs ls{};
    ls.base = la; ls.sigmas = bs->d_sigma.as<double>(); ls.log_norms = bs->d_lognorm.as<double>(); ls.floor = bs->learn_floor; ls.fit = bs->learn_scales ? 1 : 0;
    if (bs->scaled)
        hipLaunchKernelGGL(batch_learn_scaled_kernel, dim3(pl.stats_gx), dim3(kThreads), 0, c->stream, ls);
    else
        hipLaunchKernelGGL(batch_learn_kernel, dim3(pl.stats_gx), dim3(kThreads), 0, c->stream, la);
    HIP_TRY(c, hipGetLastError());
    if (bs->learn_tied) {
        // tied: step (c) never fired above; the groups' pooled records, then one M-step a group and its broadcast (csrc/batch_learn_tied.hpp)
        if (int rc = batch_pool_enqueue(c, bs->learn.rec.as<double>(), 1, 0, bs->learn.pooled.as<double>())) return rc;
        BatchLearnTiedScaledArgs ts{};
        BatchLearnTiedArgs& ta = ts.base;
        ta.members = bs->d_tie.as<int32_t>(); ta.first = bs->d_tie.as<int32_t>() + B; ta.desc = a.desc; ta.pooled = bs->learn.pooled.as<double>();
        ta.thr = la.thr; ta.means = la.means; ta.trans = la.trans; ta.status = la.status;
        ta.t_min = (int64_t)bs->learn_t_min; ta.G = (int)bs->tie_groups; ta.k = bs->hk;
        ts.sigmas = ls.sigmas; ts.log_norms = ls.log_norms; ts.floor = ls.floor; ts.fit = ls.fit;
        const dim3 tied_grid((unsigned)((bs->tie_groups + kWaves - 1) / kWaves));
        if (bs->scaled)
            hipLaunchKernelGGL(batch_learn_tied_scaled_kernel, tied_grid, dim3(kThreads), 0, c->stream, ts);
        else
            hipLaunchKernelGGL(batch_learn_tied_kernel, tied_grid, dim3(kThreads), 0, c->stream, ta);
        HIP_TRY(c, hipGetLastError());
    }
    bs->thr_stale = true; bs->lp_ready = false; bs->lp_sent = false;
    bs->decoded.assign(B, 0);
    return 0;
}

// New tables for the begun online batch from the host (scaled: cpprob_hip_batch_online_tables_scaled, with the scales; Poisson:
// cpprob_hip_batch_online_tables_poisson, h_means its rates), validated with
// the begin's own statements before anything changes; an armed batch's device tables follow.
static int batch_online_tables(cpprob_hip_ctx* c, const double* h_means, const double* h_transition, const double* h_sigmas, bool scaled, const char* who, bool poisson = false)
{
    if (int rc = batch_learn_check(c, who)) return rc;
    BatchState* bs = c->batch;
    if (bs->poisson && !poisson) return fail(c, CPPROB_HIP_ESTATE, "the batch has Poisson emissions: its tables are replaced by cpprob_hip_batch_online_tables_poisson");
    if (!bs->poisson && poisson) return fail(c, CPPROB_HIP_ESTATE, "the batch has no Poisson emissions: begin it with cpprob_hip_batch_begin_online_poisson, or call its own family's cpprob_hip_batch_online_tables");
    if (bs->scaled && !scaled) return fail(c, CPPROB_HIP_ESTATE, "the batch has emission scales: its tables are replaced by cpprob_hip_batch_online_tables_scaled");
    if (!bs->scaled && scaled) return fail(c, CPPROB_HIP_ESTATE, "the batch has no emission scales: begin it with cpprob_hip_batch_begin_online_scaled, or call cpprob_hip_batch_online_tables");
    if (!h_means || !h_transition || (scaled && !h_sigmas)) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    int k = 0;
    if (int rc = batch_check_tables(c, &bs->cfg, (int32_t)bs->hk, h_means, h_transition, k, poisson)) return rc;
    if (scaled) if (int rc = batch_check_scales(c, bs->cfg.n_problems, k, h_sigmas)) return rc;
    if (bs->learn_tied) if (int rc = batch_tied_tables_check(c, h_means, h_transition, scaled ? h_sigmas : nullptr, (size_t)k)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t B = bs->cfg.n_problems, kk = (size_t)k * k;
    bs->means.assign(h_means, h_means + B * (size_t)k);
    bs->trans.assign(h_transition, h_transition + B * kk);
    for (size_t b = 0; b < B; ++b) retable_thresholds(h_transition + b * kk, k, bs->h_thr.data() + b * 64);
    HIP_TRY(c, hipMemcpyAsync(bs->ws() + bs->lay.thr, bs->h_thr.data(), bs->h_thr.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    if (scaled || poisson) {
        if (scaled) batch_mirror_scales(bs, B, k, h_sigmas);
        else batch_mirror_rates(bs, B, k, h_means);
        HIP_TRY(c, hipMemcpyAsync(bs->d_sigma.as<double>(), bs->sigmas.data(), B * 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(bs->d_lognorm.as<double>(), bs->log_norms.data(), B * 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    if (bs->armed) {
        HIP_TRY(c, hipMemcpyAsync(bs->learn.means.as<double>(), h_means, B * (size_t)k * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(bs->learn.trans.as<double>(), h_transition, B * kk * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    // the host knows the words again; the decode's log tables and step words follow them
    bs->thr_stale = false; bs->lp_ready = false; bs->lp_sent = false;
    bs->decoded.assign(B, 0);
    return 0;
}

int cpprob_hip_batch_online_tables(cpprob_hip_ctx* c, const double* h_means, const double* h_transition)
{
    LANES_OWN(c);
    return batch_online_tables(c, h_means, h_transition, nullptr, false, "cpprob_hip_batch_online_tables");
}

int cpprob_hip_batch_online_tables_poisson(cpprob_hip_ctx* c, const double* h_rates, const double* h_transition)
{
    LANES_OWN(c);
    return batch_online_tables(c, h_rates, h_transition, nullptr, false, "cpprob_hip_batch_online_tables_poisson", true);
}

int cpprob_hip_batch_online_tables_scaled(cpprob_hip_ctx* c, const double* h_means, const double* h_transition, const double* h_sigmas)
{
    LANES_OWN(c);
    return batch_online_tables(c, h_means, h_transition, h_sigmas, true, "cpprob_hip_batch_online_tables_scaled");
}

// The armed batch's tables, status words and -- h_sigmas given: a scaled batch -- scales to the host; waits for the stream.
static int batch_learn_tables_fetch(cpprob_hip_ctx* c, double* h_means, double* h_transition, double* h_sigmas, int32_t* h_status)
{
    BatchState* bs = c->batch;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t B = bs->cfg.n_problems, k = (size_t)bs->hk;
    if (h_sigmas) HIP_TRY(c, hipMemcpy2DAsync(h_sigmas, k * sizeof(double), bs->d_sigma.as<double>(), 8 * sizeof(double), k * sizeof(double), B, hipMemcpyDeviceToHost, c->stream));
    if (h_means) HIP_TRY(c, hipMemcpyAsync(h_means, bs->learn.means.as<double>(), B * k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_transition) HIP_TRY(c, hipMemcpyAsync(h_transition, bs->learn.trans.as<double>(), B * k * k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_status) HIP_TRY(c, hipMemcpyAsync(h_status, bs->learn.status.as<int32_t>(), B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

// What the four read-outs of the learner's tables share; scaled: the call is one of the two that read the scales.
static int batch_learn_tables_check(cpprob_hip_ctx* c, bool scaled)
{
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun || !bs->armed) return fail(c, CPPROB_HIP_ESTATE, "the begun batch is not armed (cpprob_hip_batch_learn_begin)");
    if (scaled && !bs->scaled) return fail(c, CPPROB_HIP_ESTATE, "the batch has no emission scales: call cpprob_hip_batch_learn_tables / _learn_tables_device");
    return 0;
}

int cpprob_hip_batch_learn_tables(cpprob_hip_ctx* c, double* h_means, double* h_transition, int32_t* h_status)
{
    LANES_OWN(c);
    if (int rc = batch_learn_tables_check(c, false)) return rc;
    return batch_learn_tables_fetch(c, h_means, h_transition, nullptr, h_status);
}

// The same tables and -- d_sigmas given -- scales into device buffers, stream-ordered.
static int batch_learn_tables_copy(cpprob_hip_ctx* c, double* d_means, double* d_transition, double* d_sigmas)
{
    BatchState* bs = c->batch;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t B = bs->cfg.n_problems, k = (size_t)bs->hk;
    if (d_sigmas) HIP_TRY(c, hipMemcpy2DAsync(d_sigmas, k * sizeof(double), bs->d_sigma.as<double>(), 8 * sizeof(double), k * sizeof(double), B, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_means, bs->learn.means.as<double>(), B * k * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_transition, bs->learn.trans.as<double>(), B * k * k * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int cpprob_hip_batch_learn_tables_device(cpprob_hip_ctx* c, double* d_means, double* d_transition)
{
    LANES_OWN(c);
    if (int rc = batch_learn_tables_check(c, false)) return rc;
    if (!d_means || !d_transition) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    return batch_learn_tables_copy(c, d_means, d_transition, nullptr);
}

int cpprob_hip_batch_learn_tables_scaled(cpprob_hip_ctx* c, double* h_means, double* h_transition, double* h_sigmas, int32_t* h_status)
{
    LANES_OWN(c);
    if (int rc = batch_learn_tables_check(c, true)) return rc;
    return batch_learn_tables_fetch(c, h_means, h_transition, h_sigmas, h_status);
}

int cpprob_hip_batch_learn_tables_scaled_device(cpprob_hip_ctx* c, double* d_means, double* d_transition, double* d_sigmas)
{
    LANES_OWN(c);
    if (int rc = batch_learn_tables_check(c, true)) return rc;
    if (!d_means || !d_transition || !d_sigmas) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    return batch_learn_tables_copy(c, d_means, d_transition, d_sigmas);
}

int cpprob_hip_batch_learn_record(cpprob_hip_ctx* c, double* h_stats, size_t n_doubles)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun || !bs->armed) return fail(c, CPPROB_HIP_ESTATE, "the begun batch is not armed (cpprob_hip_batch_learn_begin)");
    if (!h_stats) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    const size_t need = (size_t)bs->cfg.n_problems * kOnlineStats;
    if (n_doubles < need) return fail(c, CPPROB_HIP_EINVAL, "the statistics buffer is too small: " + std::to_string(need) + " doubles (88 a problem)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(h_stats, bs->learn.rec.as<double>(), need * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

int cpprob_hip_batch_copy_step_tables(cpprob_hip_ctx* c, uint64_t problem, double* h_rows, size_t n_doubles, uint64_t* h_thr)
{
    LANES_OWN(c);
    if (!c) return fail(nullptr, CPPROB_HIP_EINVAL, "ctx is NULL");
    BatchState* bs = c->batch;
    if (!bs || !bs->begun) return fail(c, CPPROB_HIP_ESTATE, "no batch is begun");
    if (problem >= bs->cfg.n_problems) return fail(c, CPPROB_HIP_EINVAL, "problem index out of range");
    const bool hmm3 = bs->cfg.model == CPPROB_HIP_MODEL_HMM3;
    if (hmm3 && h_thr) return fail(c, CPPROB_HIP_EINVAL, "CPPROB_HIP_MODEL_HMM3 keeps no threshold words on the device: h_thr must be NULL");
    const size_t T = (size_t)bs->prob[problem].T;
    if (n_doubles < T * kBatchTab) return fail(c, CPPROB_HIP_EINVAL, "h_rows too small: " + std::to_string(T * kBatchTab) + " doubles (8 a step of the problem)");
    if (T && !h_rows) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    if (T) HIP_TRY(c, hipMemcpyAsync(h_rows, bs->ws() + bs->lay.tab + (size_t)problem * (size_t)bs->T * kBatchTab * sizeof(double), T * kBatchTab * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h_thr) HIP_TRY(c, hipMemcpyAsync(h_thr, bs->ws() + bs->lay.thr + (bs->described ? (size_t)problem : 0) * 64 * sizeof(uint64_t), 64 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
}

int cpprob_hip_batch_summaries_device(cpprob_hip_ctx* c, double* d_out)
{
    LANES_OWN(c);
    if (!c || !d_out) return fail(c, CPPROB_HIP_EINVAL, "NULL argument");
    BatchState* bs = c->batch;
    if (!bs || !bs->ran) return fail(c, CPPROB_HIP_ESTATE, "no finished batch run");
    if (bs->conditional) return fail(c, CPPROB_HIP_ESTATE, "a conditional run keeps masses and no books: the summaries wait for the next cpprob_hip_batch_run");
    HIP_TRY(c, hipSetDevice(c->device));
    const int64_t B = (int64_t)bs->cfg.n_problems, total = B * 4;
    hipLaunchKernelGGL(batch_pack_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                       (const char*)(bs->ws() + bs->lay.ctrl), (const double*)(bs->ws() + bs->lay.stats), 0, B, d_out);
    HIP_TRY(c, hipGetLastError());
    return 0;
}
}  // extern "C"

#include "group.hpp"
