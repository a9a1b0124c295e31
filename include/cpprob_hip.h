/*
 * cpprob_hip.h -- C ABI of the MI355X (gfx950) SIS / SMC inference engine.
 *
 * Drop-in boundary for ONE path of lezcano/CPProb: cpprob::inference(StateType::sis, ...)
 * (reference include/cpprob/cpprob.hpp:173-203) and the StateType::smc mode the reference never
 * shipped.  The reference has no FFI for this path -- it is a header-level C++14 template API
 *  -- so the entry points below are what the C++14 compatibility layer
 * in cpprob_amd/include/cpprob/ binds, and what a maintainer of the reference would call from
 * cpprob::inference instead of the per-particle loop.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  No C++/torch types.
 *   - Every function returns 0 on success, a negative CPPROB_HIP_E* code otherwise;
 *     cpprob_hip_last_error(ctx) then describes the failure.  Library code never exits
 *     (the reference's exit()/terminate() paths, SURVEY section 5, are not reproduced).
 *   - A context owns one device, one HIP stream (plus those of its run lanes: cpprob_hip_infer_lanes) and all device buffers of a run.  No process
 *     globals (the reference's State::state_, StateInfer::trace_, TraceInfer::ids_predict_,
 *     src/cpprob/state.cpp:20-21,148-155, are per-context here).  One run at a time per context;
 *     contexts are independent and may live on different threads.
 *   - The context's stream is NON-blocking (no implicit ordering with the null stream or any other stream): d_* buffers the
 *     caller produced elsewhere must be complete before the call that reads them.
 *   - Pointers named d_* are DEVICE pointers valid on the context's device, h_* are host
 *     pointers.  Work is enqueued on the context's stream; functions that fill host memory
 *     synchronise that stream, all others are asynchronous.
 *   - All arithmetic is fp64 (reference: double log_w_, include/cpprob/trace.hpp:59); discrete
 *     values and ancestor indices are int32.
 */
#ifndef CPPROB_HIP_H_
#define CPPROB_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define CPPROB_HIP_ABI_VERSION 3

/* error codes */
#define CPPROB_HIP_OK 0
#define CPPROB_HIP_EINVAL (-1)     /* bad argument                                   */
#define CPPROB_HIP_EDEVICE (-2)    /* HIP runtime error (no GPU, launch failure, OOM) */
#define CPPROB_HIP_ESTATE (-3)     /* call out of order (e.g. stats before run)       */
#define CPPROB_HIP_EUNSUPPORTED (-4)
#define CPPROB_HIP_EPRECISION (-5)  /* a caller-driven sharded run (step protocol) left the fixed-point weights too few bits: repeat it
                                        with CPPROB_HIP_FLAG_FLOATING_POINT_STEP (runs the library drives itself are repeated by it) */

/* StateType -- reference include/cpprob/state.hpp:28-33 {compile, csis, sis, dryrun}; smc is new. */
#define CPPROB_HIP_ALG_SIS 2
#define CPPROB_HIP_ALG_SMC 4

/* Built-in models: hand-fused kernels for the models of namespace models on this path. */
#define CPPROB_HIP_MODEL_GAUSSIAN_UNKNOWN_MEAN 0 /* include/models/models.hpp:22-35  obs (y1,y2), predict "Mu"    */
#define CPPROB_HIP_MODEL_GAUSSIAN_README 1       /* src/models/gaussian.cpp:6-17     obs (x1,x2), predict "Mean"  */
#define CPPROB_HIP_MODEL_LINEAR_GAUSSIAN_1D 2    /* include/models/models.hpp:67-80  obs[T],      predict "State" */
#define CPPROB_HIP_MODEL_HMM3 3                  /* include/models/models.hpp:114-141 obs[T],     predict "State" */
#define CPPROB_HIP_MODEL_GAUSSIAN_2D_UNKNOWN_MEAN 4 /* include/models/models.hpp:38-49 vector-valued statements: one multivariate
                                                    normal sample, one vector observe y[2], one NDArray predict "Mu".  The D = 2
                                                    components are rows of the particle store (variable-width SoA):
                                                    n_predict = 2 = one predict hit of width 2, stats row d = component d.
                                                    One observe statement => smc runs as sis.                             */

#define CPPROB_HIP_MODEL_HMM_TABLE 5             /* the model body of include/models/models.hpp:114-141 over a caller-given table
                                                    (cpprob_hip_set_hmm before cpprob_hip_infer_begin): k states, 2 <= k <= 8, uniform
                                                    initial state, emission N(mean[s], 1), transition row s as weights; predict "State"
                                                    before every observe.  stats_per_predict = 8 (P(x_t = s), zeros beyond k)        */

/* Resamplers (thesis Alg. 1 p.36: multinomial; remark p.36: systematic / stratified).  One population per context: all three run on
 * integers inside the step launch (prefix counts or fixed-point masses), bit-identical over tilings.
 *   SYSTEMATIC   one shared offset u0: output j at j + u0;
 *   STRATIFIED   output j at j + u_j, u_j the 32-bit uniform of output j;
 *   MULTINOMIAL  a_j ~ Categorical(W) iid, evaluated in two stages so that offspring stay next to their parent (strata form): the N
 *                iid thresholds as counts per equal stratum of the total mass (K = 2^k strata, K >= four times the 1024-particle tiles;
 *                exact Binomial splits down a tree of Philox popcounts: independent of the weights, drawn once per run) and iid
 *                53-bit uniforms inside a stratum: output s of stratum w takes tau_s = B_w + floor(v_s (B_w+1 - B_w)), its ancestor
 *                is min{k : C_k > tau_s}  (CPPROB_HIP_FLAG_MULTINOMIAL_LITERAL: one threshold floor(u_j C_N) per output searched
 *                against the whole population -- the same law, N scattered searches). */
#define CPPROB_HIP_RESAMPLE_SYSTEMATIC 0
#define CPPROB_HIP_RESAMPLE_STRATIFIED 1
#define CPPROB_HIP_RESAMPLE_MULTINOMIAL 2

#define CPPROB_HIP_SCOPE_GLOBAL 0
#define CPPROB_HIP_SCOPE_ISLAND 1
#define CPPROB_HIP_SCOPE_EXCHANGE 2   /* one population, resampled jointly AND exactly: offspring of remote sources migrate (below) */

typedef struct cpprob_hip_ctx cpprob_hip_ctx;

/* Run configuration.  Replaces the arguments of cpprob::inference (cpprob.hpp:173-180):
 * algorithm <- StateType, model <- const Func& f, n_particles <- std::size_t n; the observes
 * tuple is passed flattened to cpprob_hip_infer_begin.  The reference has no seed (its RNG is
 * a random_device-seeded global, src/cpprob/utils.cpp:16-20); here runs are reproducible. */
typedef struct cpprob_hip_config {
    int32_t algorithm;        /* CPPROB_HIP_ALG_*                                              */
    int32_t model;            /* CPPROB_HIP_MODEL_*                                            */
    int32_t resampler;        /* CPPROB_HIP_RESAMPLE_* (SMC only)                              */
    int32_t resample_scope;   /* CPPROB_HIP_SCOPE_GLOBAL: one population of n_global particles,
                                 resampled jointly (sharded runs use the step_begin/step_end
                                 protocol); CPPROB_HIP_SCOPE_ISLAND: this shard is an independent
                                 population of n_particles (particle_offset only selects the
                                 RNG streams); shards are combined by their evidence estimates;
                                 CPPROB_HIP_SCOPE_EXCHANGE: like GLOBAL, with particle migration
                                 (cpprob_hip_exchange_*) so that resampling is exact over shards */
    int32_t keep_history;     /* 1: keep per-step values + ancestors: statistics over whole traces (what the reference's
                                 posterior files hold), dumps.  0 (SMC; one population per context, or a shard of a joint
                                 population in the exchange scope, whose migrants are then their current state alone): filtering only --
                                 two rows of values, no ancestors (memory O(N) instead of O(N T)); predict hit t's
                                 statistics are those of generation t under its own weights; cpprob_hip_copy_values /
                                 _ancestors / _paths return CPPROB_HIP_ESTATE                                    */
    int32_t annex_kcols;      /* exchange scope: immigrant-annex capacity in units of 1024 columns per row (0 = default: the larger of
                                 1/16 of the shard and sqrt(n_global) x T -- what a well-mixed run's O(sqrt N) immigrants per step
                                 add up to --, at least 4096); stream-ordered runs cannot grow it mid-run and report overflow instead */
    uint32_t flags;           /* CPPROB_HIP_FLAG_* below; 0 = the measured optimum.  Every switch that selects another kernel form
                                 lives HERE, in the caller's hands -- the library reads no environment variable */
    int32_t fuse_max_tiles;   /* floating-point step: largest population (in 1024-particle tiles) whose step kernel normalises the
                                 previous generation in its own prologue; 0 = default (1664), capped there */
    double ess_threshold;     /* SMC: resample after a step iff ESS < ess_threshold * N_global;
                                 > 1 resamples after every step (thesis p.37 uses 0.5)        */
    uint64_t seed;            /* Philox key                                                    */
    uint64_t n_particles;     /* particles held by THIS context (the shard)                    */
    uint64_t particle_offset; /* global id of local particle 0 (RNG counters use global ids)   */
    uint64_t n_global;        /* total particles over all shards (= n_particles for 1 GPU)     */
} cpprob_hip_config;

/* cpprob_hip_config::flags -- A/B and diagnostic forms (results agree within the stated tolerances) */
#define CPPROB_HIP_FLAG_FLOATING_POINT_STEP 1u   /* table-weight models on an every-step schedule: the floating-point step instead of the
                                                    integer prefix-count step (ancestors then agree up to CDF-boundary flips, not bit for bit) */
#define CPPROB_HIP_FLAG_NO_SKIP_ROWS 2u          /* exchange scope, long traces: extract migrating lineages hop by hop */
#define CPPROB_HIP_FLAG_SIS_PER_TILE 4u          /* SIS of bounded-weight models through the per-tile kernel */
#define CPPROB_HIP_FLAG_SIS_SEPARATE_READOUT 8u  /* SIS read-out as a pass over the particle store instead of riding the normalisation */
#define CPPROB_HIP_FLAG_WREL_STORED 16u          /* floating-point step of table-weight models: read stored linear weights, not states */
#define CPPROB_HIP_FLAG_FP_TILE_PARTIALS 32u     /* ... and fp64 tile partials instead of packed per-value counts */
#define CPPROB_HIP_FLAG_WALK_READOUT 64u         /* short discrete traces: read the posterior out by the lineage walk, not from trace words */
#define CPPROB_HIP_FLAG_PAIRED_STEP_LAUNCH 512u  /* fixed-point form, ESS-triggered schedules (A/B): a step as two launches {carry, resampling} of which one ends at once */
#define CPPROB_HIP_FLAG_REPEAT_IN_FLOATING_POINT 256u /* fixed-point form: a run with a generation that lost its bits is repeated whole in the floating-point form
                                                        (the r03 / r04 behaviour) instead of being repaired from that generation on, in integers */
#define CPPROB_HIP_FLAG_MULTINOMIAL_LITERAL 128u /* multinomial resampling: ancestor of output j = min{k : C_k > floor(u_j C_N)}, one search per output */
#define CPPROB_HIP_FLAG_SEPARATE_TRACE_READOUT 1024u /* prefix-count form, a population of its own (A/B): the read-out of the trace words (or of a
                                                        filtering-only run's final generation) as a launch after the last step, not folded into it */
#define CPPROB_HIP_FLAG_SERIAL_RUNS 2048u        /* run lanes (below, cpprob_hip_infer_lanes) off (A/B): every cpprob_hip_infer_run of this context on its one stream */

/* Posterior summary of a finished run -- what StatsPrinter prints
 * (include/cpprob/postprocess/stats_printer.hpp:42-79) plus SMC diagnostics. */
typedef struct cpprob_hip_summary {
    double log_evidence;  /* log Z-hat: logsumexp(logw) - log N for SIS; SMC product estimate     */
    double ess_final;     /* (sum W_i^2)^-1 of the final weights, thesis p.37                      */
    double log_norm;      /* logsumexp of the final log-weights (EmpiricalDistribution :117-123)  */
    double max_logw;      /* reference of the final weights: their max, or (continuous-weight models; bounded-weight SIS: an upper bound of it)
                             the smallest multiple of ln 2 above it; sums are relative to exp(max_logw) */
    int32_t n_predict;    /* predict hits per trace (T)                                           */
    int32_t stats_per_predict; /* 2 for real predicts (mean, variance); k for int predicts (P(x=s)) */
    int32_t is_int;       /* 1: predicts are integral (.int file), 0: real (.real)                */
    int32_t n_resampled;  /* number of steps after which resampling happened                      */
    int32_t step_form;    /* arithmetic the run's steps ran in: CPPROB_HIP_FORM_*                          */
    int32_t n_requantised; /* fixed-point form: generations whose weights were taken again against their exact maximum, because their heaviest
                              particle sat more than 6 nats below the reference known in advance (the steps behind such a generation ran again) */
} cpprob_hip_summary;
#define CPPROB_HIP_FORM_FLOAT 0   /* fp64 linear weights, floating-point CDF (stratified / multinomial resampling, locally resampled
                                     shards, SIS, runs repeated because the fixed-point weights lost their bits)          */
#define CPPROB_HIP_FORM_COUNTS 1  /* integer prefix counts of the states (table-weight models, every-step schedule)        */
#define CPPROB_HIP_FORM_FIXED 2   /* fixed-point weights q = rint(exp(lw - max_logw) 2^32), exact 64-bit prefix masses     */

/* ---- lifecycle ------------------------------------------------------------------------- */
int cpprob_hip_abi_version(void);
/* Hash of the sources this binary was built from (cpprob_amd/build.py embeds it; "unknown" for a hand-rolled build):
 * lets a loader refuse a stale libcpprob_hip.so that is newer than, but different from, the sources next to it. */
const char* cpprob_hip_build_id(void);
/* Number of visible HIP devices, or a negative error code (no GPU -> CPPROB_HIP_EDEVICE). */
int cpprob_hip_device_count(void);
/* Creates a context on `device` with its own stream.  Fails loudly without a GPU. */
int cpprob_hip_create(int device, cpprob_hip_ctx** out);
void cpprob_hip_destroy(cpprob_hip_ctx* ctx);
const char* cpprob_hip_last_error(const cpprob_hip_ctx* ctx); /* ctx may be NULL: global message */
/* The context's hipStream_t, for event timing / interop by the caller.  From this call on every run of the context is enqueued on
 * this stream alone (no run lanes: cpprob_hip_infer_lanes), until the context is destroyed -- also for a caller that only wanted to time
 * with events.  Waits for lanes already used; NULL (and cpprob_hip_last_error) if their work failed. */
void* cpprob_hip_stream(cpprob_hip_ctx* ctx);
int cpprob_hip_sync(cpprob_hip_ctx* ctx);

/* ---- cpprob::inference ------------------------------------------------------------------
 * begin : State::set + StateInfer::start_infer + config_file (cpprob.hpp:184-192): validates,
 *         (re)allocates the particle store in HBM and uploads the observes.
 * run   : the whole `for (i < n)` loop of cpprob.hpp:194-201 for all particles at once, plus
 *         (SMC) weight normalisation, ESS test and resampling between observes, plus the
 *         posterior read-out (stats_printer.hpp:88-120 / empirical_distribution.hpp:30-81).
 *         Asynchronous; may be called repeatedly (each call is one full run; pass run_index to
 *         decorrelate runs: the Philox key used is seed + run_index).
 * summary / stats : finish_infer + StatsPrinter: synchronise and copy results to the host.
 *         h_stats receives n_predict * stats_per_predict doubles, row t = predict hit t:
 *         real -> {mean, variance} (raw_moment(2) - mean^2, empirical_distribution.hpp:78-81);
 *         int  -> {P(x_t = 0), ..., P(x_t = k-1)} (distribution(), :30-40).
 */
/* The three read-backs below in ONE call and behind ONE stream synchronisation (pinned staging): what cpprob::inference reads when a
 * run is over.  h_stats ([n_predict * stats_per_predict], n_doubles its capacity), h_ess and h_resampled ([n_predict]) may be NULL.
 * Same values, same errors as cpprob_hip_infer_summary / _stats / _step_trace. */
int cpprob_hip_infer_results(cpprob_hip_ctx* ctx, cpprob_hip_summary* out, double* h_stats, size_t n_doubles, double* h_ess, int32_t* h_resampled);
/* The table of CPPROB_HIP_MODEL_HMM_TABLE: h_means[k], h_transition[k * k] (row s = the weights discrete_distribution{T[s]} of
 * models.hpp:135 would be built from).  Kept by the context until the next call. */
int cpprob_hip_set_hmm(cpprob_hip_ctx* ctx, int32_t k, const double* h_means, const double* h_transition);
int cpprob_hip_infer_begin(cpprob_hip_ctx* ctx, const cpprob_hip_config* cfg, const double* h_observes, size_t n_observes);
int cpprob_hip_infer_run(cpprob_hip_ctx* ctx, uint64_t run_index);
/* Run lanes.  One run is a chain of dependent launches that leaves most of the device idle; runs that differ only in run_index are
 * independent.  A context therefore owns up to 3 LANES: lane 0 is the context itself, the further ones are created and begun by the
 * library the first time they are needed, each with its own stream and its own complete workspace (same configuration, observes and
 * cpprob_hip_set_hmm table), so that runs enqueued back to back overlap on the device.  Each run computes what it computes alone.
 *   which lane   a rule of the call sequence alone (never of timing): a cpprob_hip_infer_run that DIRECTLY follows another
 *                cpprob_hip_infer_run of this context goes to the next lane, round robin; any other entry point in between (a read,
 *                cpprob_hip_sync, a building block ...; not cpprob_hip_infer_lanes and cpprob_hip_last_error) ends the sequence: the
 *                next run goes where the last one ran (lane 0 after a begin).  run -> results -> run -> results never leaves lane 0 and
 *                allocates nothing.
 *   reads        cpprob_hip_infer_summary / _stats / _results / _step_trace, cpprob_hip_copy_*, cpprob_hip_smc_first_bad_generation and
 *                cpprob_hip_filter_masses act on the lane of the LAST run (the fixed-point check and repair run there): they return the
 *                last run's results, as before; earlier runs' results are overwritten lane by lane, as they were on one stream.
 *                cpprob_hip_infer_results_device enqueues on the context's own stream, behind an event recorded after that lane's run.
 *   waits        cpprob_hip_sync waits for every lane; cpprob_hip_destroy frees them; cpprob_hip_infer_begin and cpprob_hip_set_hmm
 *                invalidate them (begun again at their next use, allocations reused where they suffice).  Every other entry point --
 *                the step protocol, cpprob_hip_generic_*, the building blocks, cpprob_hip_batch_*, cpprob_hip_exchange_*, profiling --
 *                first waits for every lane and then works on the context itself, as before.
 *   memory       every further lane holds what the context's begin allocated (*lane_bytes); together at most a quarter of the device
 *                memory that was free without them (hipMemGetInfo, asked before allocating).
 *   serial       runs stay on the context's one stream -- after waiting for lanes already used -- when (*serial_reason):
 *                STREAM  cpprob_hip_stream was called: a handed-out stream promises stream order; holds until destroy;
 *                PROFILE cpprob_hip_profile_enable is on (the per-class events are stream-ordered);
 *                SHARD   the context holds a shard of a joint population (n_global != n_particles) or is in the exchange scope;
 *                FLAG    CPPROB_HIP_FLAG_SERIAL_RUNS;
 *                MEMORY  a further lane did not fit (that lane is freed, no error is returned); holds until destroy;
 *                SIZE    more than 10240 tiles of 1024 particles (~1.05 10^7): a launch of that size fills the device by itself and the
 *                        measured gain falls inside the run-to-run spread (profiles/r11_notes.md).
 *   several contexts   a process opens four hardware queues: three lanes fill them.  Two contexts that both use lanes still gain
 *                (0.075 ms per hmm<16> run of 10^6 particles against 0.083 without); THREE OR MORE CONTEXTS KEPT IN FLIGHT AT ONCE lose
 *                about 10 % against plain ones (0.077-0.083 against 0.070): begin them with CPPROB_HIP_FLAG_SERIAL_RUNS.
 * depth = lanes begun with the configuration in force (1: the context alone), last_lane = lane of the last run, lane_bytes = device
 * bytes of the further lanes' population-sized arrays (weights, particle store, ancestors: all but a few KB of what they hold), serial_reason = 0 or CPPROB_HIP_SERIAL_*; any pointer may be NULL.  Pure introspection. */
#define CPPROB_HIP_SERIAL_STREAM 1
#define CPPROB_HIP_SERIAL_PROFILE 2
#define CPPROB_HIP_SERIAL_SHARD 3
#define CPPROB_HIP_SERIAL_FLAG 4
#define CPPROB_HIP_SERIAL_MEMORY 5
#define CPPROB_HIP_SERIAL_SIZE 6
int cpprob_hip_infer_lanes(cpprob_hip_ctx* ctx, int32_t* depth, int32_t* last_lane, uint64_t* lane_bytes, int32_t* serial_reason);
int cpprob_hip_infer_summary(cpprob_hip_ctx* ctx, cpprob_hip_summary* out);
int cpprob_hip_infer_stats(cpprob_hip_ctx* ctx, double* h_stats, size_t n_doubles);
/* The same results left ON THE DEVICE, stream-ordered, no host synchronisation: d_out (device, caller-owned, at least
 * 4 + n_predict * stats_per_predict doubles) receives {log_evidence, ess_final, log_norm, max_logw, stats...} of the
 * run that was just enqueued.  For callers that feed them to a collective (multi-GPU island combine) or batch many
 * runs before looking at any. */
int cpprob_hip_infer_results_device(cpprob_hip_ctx* ctx, double* d_out, size_t n_doubles);
/* Per-step diagnostics of the last run: ESS after weighting step t and whether resampling
 * followed it.  Arrays of n_predict entries (either may be NULL). */
int cpprob_hip_infer_step_trace(cpprob_hip_ctx* ctx, double* h_ess, int32_t* h_resampled);

/* The particle store of the last run (the in-HBM form of the reference's posterior files,
 * src/cpprob/state.cpp:193-202,262-267).  Copies to host, synchronising.
 *   values    : [n_predict][n_particles], fp64 for real models, int32 for int models:
 *               value of predict hit t in slot i of generation t
 *   ancestors : [n_predict][n_particles] int32: slot of generation t-1 that slot i of
 *               generation t extends (row 0 and non-resampled steps: identity); SMC only
 *   logw      : [n_particles] final log-weights
 *   paths     : [n_predict][n_particles]: values along the ancestral line of final particle i,
 *               i.e. the full trace the reference would have dumped for particle i */
int cpprob_hip_copy_values(cpprob_hip_ctx* ctx, void* h_values, size_t n_bytes);
int cpprob_hip_copy_ancestors(cpprob_hip_ctx* ctx, int32_t* h_anc, size_t n_bytes);
int cpprob_hip_copy_logw(cpprob_hip_ctx* ctx, double* h_logw, size_t n_bytes);
int cpprob_hip_copy_paths(cpprob_hip_ctx* ctx, void* h_paths, size_t n_bytes);

/* ---- many small problems in one launch (batched SMC) ---------------------------------------------------------------------
 * B independent problems of one table-weight HMM, each with its own observation sequence (all of length T), seed and results, run
 * as ONE launch: one workgroup per problem holds its whole population in LDS and runs every step and the read-out.  Problem b
 * computes what a one-context SMC run begun with seed h_seeds[b] (particle_offset 0, run_index 0) computes: the same states and
 * ancestors, the same evidence, ESS and resampling flags, and the same statistics up to the last bits of the final division.
 * Supported: algorithm SMC, model HMM3 (prefix counts) or HMM_TABLE (fixed-point weights; the table of cpprob_hip_set_hmm at
 * batch_begin, shared by the batch), systematic or stratified resampling after every step (ess_threshold > 1), 1 <= n <= 8192
 * particles per problem, any T >= 1 and B >= 1.  Everything else returns CPPROB_HIP_EUNSUPPORTED (multinomial resampling,
 * ESS-triggered schedules, SIS, the Gaussian models) and runs on the single-population path.  The batch state lives beside a
 * context's single-run state: infer_* runs and batch runs may interleave on one context and keep their own results. */
typedef struct cpprob_hip_batch_config {
    int32_t algorithm;      /* must be CPPROB_HIP_ALG_SMC                                                           */
    int32_t model;          /* CPPROB_HIP_MODEL_HMM3 | CPPROB_HIP_MODEL_HMM_TABLE                                   */
    int32_t resampler;      /* CPPROB_HIP_RESAMPLE_SYSTEMATIC | CPPROB_HIP_RESAMPLE_STRATIFIED                      */
    int32_t keep_history;   /* 1: smoothed statistics + a per-problem particle store; 0: filtering statistics, O(B n) */
    uint32_t flags;         /* 0 or CPPROB_HIP_BATCH_KEEP_MASSES (keep_history = 0 only); every other bit is reserved  */
    double ess_threshold;   /* must be > 1 (every-step schedule)                                                    */
    uint64_t n_particles;   /* per problem, 1 .. 8192                                                               */
    uint64_t n_problems;    /* B                                                                                    */
} cpprob_hip_batch_config;
/* cpprob_hip_batch_config::flags.  A filtering-only batch (keep_history = 0) that keeps the m table of the backward smoother: the
 * eight integer masses m_t[s] = cnt_t[s] * fix_weight(ll_t[s], M_t) of every (problem, step), written by the run itself where the
 * step's counts stand (csrc/batch_smc.hpp) into one more workspace region of 64 B T bytes (the last one; a batch of problems: 64 B T_max,
 * an online batch: of the largest capacity), rounded as the others.  cpprob_hip_batch_smooth*, _smooth_lag* and _smooth_stats* then
 * serve the batch as they serve one with keep_history = 1 -- the same bits, without a counting launch, a particle store or ancestors:
 * O(n) memory a problem plus 64 bytes a step.  The lineage read-outs (cpprob_hip_batch_copy_store, _paths*) keep returning
 * CPPROB_HIP_ESTATE: there are no lineages.  With keep_history = 1 the bit is CPPROB_HIP_EINVAL. */
#define CPPROB_HIP_BATCH_KEEP_MASSES 2u
/* Pure host function (no device, no context): validates cfg and T and returns the device bytes a batch needs.  The workspace is ten
 * regions, each rounded up to a multiple of 256 bytes: 64 B T (per-step tables), 8 B (seeds), 512 (transition rows), 256 B (control
 * blocks), 8 B T spp (statistics), 8 B T (ESS), 4 B T (resampling flags), 4 B (requantised generations), and with keep_history = 1
 * B T n (states) and 4 B T n (ancestors); spp = 3 (HMM3) or 8 (HMM_TABLE).  A context's workspace grows to the largest batch begun. */
int cpprob_hip_batch_workspace_bytes(const cpprob_hip_batch_config* cfg, size_t T, uint64_t* out_bytes);
/* h_observes[B][T].  Validates, sizes the workspace, evaluates the per-step tables and uploads them (synchronising). */
int cpprob_hip_batch_begin(cpprob_hip_ctx* ctx, const cpprob_hip_batch_config* cfg, const double* h_observes, size_t T);
/* One launch, asynchronous: problem b runs with Philox key h_seeds[b] (explicit per problem: neighbours never share streams). */
int cpprob_hip_batch_run(cpprob_hip_ctx* ctx, const uint64_t* h_seeds);
/* h_out[B] (filled as a one-problem run fills its summary), h_stats[B][T][spp] (n_doubles its capacity), h_ess[B][T] and
 * h_resampled[B][T]; the last three may be NULL.  Synchronises. */
int cpprob_hip_batch_results(cpprob_hip_ctx* ctx, cpprob_hip_summary* h_out, double* h_stats, size_t n_doubles, double* h_ess, int32_t* h_resampled);
/* The same left on the device, stream-ordered, no host synchronisation: d_out[B][4 + T spp] = {log_evidence, ess_final, log_norm,
 * max_logw, stats...} per problem, cpprob_hip_infer_results_device's layout. */
int cpprob_hip_batch_results_device(cpprob_hip_ctx* ctx, double* d_out, size_t n_doubles);
/* Problem `problem`'s particle store: h_values[T][n], h_anc[T][n] (cpprob_hip_copy_values / _ancestors' layout) and the final
 * log-weights h_logw[n]; any may be NULL.  keep_history = 1 only (else CPPROB_HIP_ESTATE).  Synchronises. */
int cpprob_hip_batch_copy_store(cpprob_hip_ctx* ctx, uint64_t problem, int32_t* h_values, int32_t* h_anc, double* h_logw);
/* Problem `problem`'s rows of the m table after a finished run (or advance): h_out[T_b][8], T_b its length (an online batch: the
 * length reached), n_doubles the capacity of h_out.  A batch begun with CPPROB_HIP_BATCH_KEEP_MASSES only (else CPPROB_HIP_ESTATE);
 * CPPROB_HIP_EINVAL: a problem index out of range or fewer than 8 T_b doubles.  Synchronises. */
int cpprob_hip_batch_copy_masses(cpprob_hip_ctx* ctx, uint64_t problem, double* h_out, size_t n_doubles);

/* A batch whose problems differ: a second way to begin, in which problem b brings its own number of observes h_T[b], its own particle
 * count h_n[b] and, for CPPROB_HIP_MODEL_HMM_TABLE, its own table -- the same sequence under many parameter settings (a likelihood
 * grid, many chains of particle-marginal Metropolis-Hastings), or a ragged collection of sequences.  Problem b still computes what a
 * one-context SMC run with that table, those observes, h_n[b] particles and seed h_seeds[b] computes.  cpprob_hip_batch_run, _results,
 * _results_device and _copy_store serve a batch begun either way; the two begins may follow each other on one context (the workspace
 * only grows).  After this begin:
 *   - the small results are padded to T_max = max h_T so they stay plain arrays: h_stats[B][T_max][spp], h_ess[B][T_max],
 *     h_resampled[B][T_max], d_out[B][4 + T_max spp]; rows t >= h_T[b] are zero; cpprob_hip_summary::n_predict of problem b is h_T[b];
 *   - the particle store is packed: cpprob_hip_batch_copy_store(problem) returns h_values / h_anc [h_T[b]][h_n[b]] and h_logw[h_n[b]].
 * cfg is as for cpprob_hip_batch_begin, with n_particles = the LARGEST per-problem particle count: it sizes every workgroup's LDS
 * (6 bytes a particle, n rounded up to 1024), so a workgroup of few particles still reserves the largest problem's share and LDS caps
 * the workgroups a compute unit holds as if all were that large (3 at 8192, 6 at 4096); a caller with a few large and many small
 * problems may prefer two batches.  Workgroups are dispatched longest problem first (h_T[b] * ceil(h_n[b] / 1024), ties by index); no
 * result depends on that order or on the other problems.
 *
 * Pure host function (no device, no context): validates cfg (as cpprob_hip_batch_workspace_bytes does, same codes), every h_T[b] >= 1
 * and 1 <= h_n[b] <= cfg->n_particles <= 8192, and returns the device bytes.  The workspace is twelve regions, each rounded up to a
 * multiple of 256 bytes: 64 B T_max (per-step tables), 8 B (seeds), 512 B (transition rows, one table a problem), 256 B (control
 * blocks), 8 B T_max spp (statistics), 8 B T_max (ESS), 4 B T_max (resampling flags), 4 B (requantised generations), 16 B (problem
 * descriptors), 4 B (dispatch order), and with keep_history = 1 S (states) and 4 S (ancestors), S = sum over b of h_T[b] h_n[b]. */
int cpprob_hip_batch_problems_workspace_bytes(const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n, uint64_t* out_bytes);
/* h_T[B], h_n[B]; h_observes packed: problem b's h_T[b] observes start at the sum of h_T[0..b).  CPPROB_HIP_MODEL_HMM_TABLE: k states
 * (2 .. 8, one k per batch), h_means[B][k] and h_transition[B][k][k] = problem b's table, validated as cpprob_hip_set_hmm validates
 * (CPPROB_HIP_EINVAL names the problem); both NULL (k ignored): the context's cpprob_hip_set_hmm table for every problem.
 * CPPROB_HIP_MODEL_HMM3: both NULL, anything else CPPROB_HIP_EINVAL.  Tables and thresholds are evaluated per problem with the host
 * statements of the single-population begin; uploads and synchronises. */
int cpprob_hip_batch_begin_problems(cpprob_hip_ctx* ctx, const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n,
                                    const double* h_observes, int32_t k, const double* h_means, const double* h_transition);

/* A batch whose observes arrive over time: a third way to begin, with capacities instead of lengths and without observes, followed by
 * any number of cpprob_hip_batch_advance calls, each of which hands every problem zero or more new observes and runs the new steps
 * only.  After any sequence of advances problem b has seen its first L_b observes, and everything the library returns for it --
 * summaries, h_stats, h_ess, h_resampled, d_out, the particle store -- is bit for bit what a batch begun by
 * cpprob_hip_batch_begin_problems with h_T[b] = L_b (same tables, particle counts and seeds) and run once returns: feeding T observes
 * one at a time costs T steps, not T^2 / 2.  (In the shorter run generation L_b - 1 was final; the next piece re-keeps its books in the
 * resampling form, resamples it with that junction's own Philox draw and goes on: csrc/batch_smc.hpp.)  A problem with L_b = 0 has no
 * results yet: its rows are zero, its summary is zero and its n_predict is 0.  cpprob_hip_batch_results, _results_device and
 * _copy_store serve the batch with lengths L_b and the padding T_max = max h_Tcap; cpprob_hip_batch_run returns CPPROB_HIP_ESTATE on
 * it, as cpprob_hip_batch_advance and _lengths do on a batch begun the other ways.  Any begin replaces it; infer_* runs may interleave.
 *
 * Pure host function (no device, no context): validates as cpprob_hip_batch_problems_workspace_bytes does (same codes, same refusals;
 * the capacities h_Tcap[b] >= 1 stand in for the lengths) and returns the device bytes.  The workspace is the twelve regions of a
 * batch of problems of lengths h_Tcap (above), then, each rounded up to a multiple of 256 bytes: 4 B (every problem's first step of
 * a launch), 32 B (the books before the last generation's final bookkeeping: what a later piece rewinds to) and, with
 * keep_history = 0, N (the last generation's states, a byte a particle), N = sum over b of h_n[b]. */
int cpprob_hip_batch_online_workspace_bytes(const cpprob_hip_batch_config* cfg, const uint32_t* h_Tcap, const uint32_t* h_n, uint64_t* out_bytes);
/* h_Tcap[B], h_n[B]; k, h_means and h_transition as for cpprob_hip_batch_begin_problems (both NULL: the context's cpprob_hip_set_hmm
 * table; CPPROB_HIP_MODEL_HMM3: both NULL); h_seeds[B]: problem b's Philox key for the life of the batch.  Every problem starts at
 * length 0.  Besides the device workspace the batch holds pinned host memory: a mirror of the per-step tables (64 B T_max bytes).
 * Uploads and synchronises. */
int cpprob_hip_batch_begin_online(cpprob_hip_ctx* ctx, const cpprob_hip_batch_config* cfg, const uint32_t* h_Tcap, const uint32_t* h_n,
                                  int32_t k, const double* h_means, const double* h_transition, const uint64_t* h_seeds);
/* Problem b receives h_dT[b] >= 0 new observes, packed in problem order in h_observes (NULL if every h_dT[b] is 0).  If some
 * L_b + h_dT[b] exceeds h_Tcap[b]: CPPROB_HIP_EINVAL naming the problem, and nothing changes.  Otherwise the new steps' table rows are
 * evaluated on the host (the begin's own statements) into the pinned mirror, copied stream-ordered, and ONE launch is enqueued; the
 * call returns without waiting (h_dT and h_observes are consumed before it returns).  Workgroups are dispatched longest piece first
 * (h_dT[b] * ceil(h_n[b] / 1024), ties by index); a problem without new observes costs a workgroup that returns at once.
 * readout (keep_history = 1 only; ignored with keep_history = 0, whose books write every statistics row as they go): 1 ends the launch
 * with the lineage walk over all L_b rows, as a one-shot run does; 0 skips it, and until an advance with readout = 1 has been
 * enqueued cpprob_hip_batch_results with a non-NULL h_stats and cpprob_hip_batch_results_device return CPPROB_HIP_ESTATE (summaries,
 * ESS, flags and the store are served).  That advance may have every h_dT[b] = 0: it then does the walk and nothing else. */
int cpprob_hip_batch_advance(cpprob_hip_ctx* ctx, const uint32_t* h_dT, const double* h_observes, int32_t readout);
/* h_L[B]: the lengths reached so far (host state: no synchronisation). */
int cpprob_hip_batch_lengths(cpprob_hip_ctx* ctx, uint32_t* h_L);

/* Posterior traces of a batch: the surviving lineages of EVERY problem of the batch last run (or last advanced), resolved by ONE
 * launch (csrc/batch_paths.hpp) -- what cpprob_hip_copy_paths delivers for a single population.  For final particle i < m_b of
 * problem b, entry [t][i] is the state at step t of the trajectory that ends in particle i, and weight [i] is its final log-weight:
 * the table double cpprob_hip_batch_copy_store returns, bit for bit.  m_b = n_b when max_particles is 0, else min(n_b, max_particles):
 * the first m_b traces only (Options::dump_max_particles), so that a few traces of many problems do not move the whole store.
 * The output is packed: problem b's [T_b][m_b] entries start at first_b = sum over b' < b of T_b' m_b' and its m_b weights at
 * wfirst_b = sum over b' < b with T_b' > 0 of m_b'; T_b = h_T[b] (a uniform batch: T), an online batch: the length
 * cpprob_hip_batch_lengths reports, served whether or not the last advance did its read-out.  A problem of length 0 owns neither
 * entries nor weights.  keep_history = 1 only, and only after a run (else CPPROB_HIP_ESTATE, as cpprob_hip_batch_copy_store).
 *
 * Pure host function (no device, no context): the packed layout.  h_first[B + 1] (entries) and h_wfirst[B + 1] (weights), the last
 * element the total; either may be NULL.  h_T[b] may be 0.  CPPROB_HIP_EINVAL: NULL h_T / h_n, n_problems == 0, an h_n[b] of 0 or
 * above 8192. */
int cpprob_hip_batch_paths_layout(const uint32_t* h_T, const uint32_t* h_n, uint64_t n_problems, uint64_t max_particles,
                                  uint64_t* h_first, uint64_t* h_wfirst);
/* Host copies: h_paths int32 (cpprob_hip_copy_paths' element type), n_entries / n_weights the capacities in elements
 * (CPPROB_HIP_EINVAL when too small, nothing written); h_logw may be NULL.  Stages int8 on the device and widens.  Synchronises. */
int cpprob_hip_batch_paths(cpprob_hip_ctx* ctx, uint64_t max_particles, int32_t* h_paths, size_t n_entries, double* h_logw, size_t n_weights);
/* The same left on the device, enqueued on the context's stream after the run / advance, no host synchronisation: d_paths int8 (the
 * store's own element), d_logw may be NULL.  (The problems' descriptors travel through pinned host memory, four calls deep: the
 * fifth call in a row waits for the first one's copy, nothing else.) */
int cpprob_hip_batch_paths_device(cpprob_hip_ctx* ctx, uint64_t max_particles, int8_t* d_paths, size_t n_entries, double* d_logw, size_t n_weights);

/* Backward smoothing of a batch (csrc/batch_smooth.hpp): the smoothed marginals P(x_t = s | y) and backward-simulated trajectories of
 * EVERY problem of the batch last run (or last advanced), from every generation's whole filtering approximation instead of the
 * lineages that survive to the end -- with resampling after every step those have coalesced to a handful of ancestors at the early
 * steps.  Generation t of problem b enters as the k integers m_t[s] = (particles in state s) * fix_weight(ll_t[s], M_t), M_t the
 * largest ll_t[s] over the states present, and the transition law as the integers P[s][s'] its thresholds realise on 32-bit words;
 * csrc/batch_smooth.hpp and DESIGN.md section 5 state the arithmetic, which contracts no product into a sum, so the trajectories are
 * a pure function of integers and IEEE operations.  Trajectory j of problem b draws the 53-bit uniform of word pair j & 1 of Philox
 * block (key: the problem's run seed -- an online batch: its seed at begin --, group j >> 1, draw 2^41 + (draw_index << 24) + t) at
 * step t: draw_index < 2^16 gives fresh, reproducible trajectories call after call.
 * Marginals: [B][T_max][stats_per_predict] doubles, the layout and padding of cpprob_hip_batch_results' h_stats (rows t >= T_b and
 * states >= k are zero).  Trajectories: problem b's [T_b][n_traj] entries from n_traj * (sum over b' < b of T_b') on, T_b as for
 * cpprob_hip_batch_paths; a problem of length 0 owns none and its marginal rows are zero.  Either output may be NULL; n_traj may be
 * 0 when the trajectories are NULL.  keep_history = 1 only, and only after a run (else CPPROB_HIP_ESTATE, as
 * cpprob_hip_batch_copy_store); CPPROB_HIP_EINVAL: a capacity too small (nothing written), draw_index >= 2^16, n_traj > 2^20, a
 * problem longer than 2^24.  The call reads the store and the per-step tables and changes nothing the other entry points return;
 * the m table (64 B a step of the batch) is an allocation of the context's own, grown when needed, not part of the batch workspace.
 *
 * Pure host function (no device, no context): h_first[B + 1], problem b's first trajectory entry, the last element the total.
 * h_T[b] may be 0.  CPPROB_HIP_EINVAL: NULL h_T / h_first, n_problems == 0, n_traj > 2^20, an h_T[b] above 2^24. */
int cpprob_hip_batch_smooth_layout(const uint32_t* h_T, uint64_t n_problems, uint64_t n_traj, uint64_t* h_first);
/* Host copies: h_marginals doubles, h_traj int32 (cpprob_hip_batch_paths' element type); n_doubles / n_entries the capacities in
 * elements.  Stages on the device and widens.  Synchronises. */
int cpprob_hip_batch_smooth(cpprob_hip_ctx* ctx, uint64_t n_traj, uint64_t draw_index, double* h_marginals, size_t n_doubles, int32_t* h_traj, size_t n_entries);
/* The same left on the device, enqueued on the context's stream after the run / advance, no host synchronisation: d_traj int8.  (The
 * problems' descriptors travel through pinned host memory, four calls deep, as cpprob_hip_batch_paths_device's do; a call that has to
 * grow the m table waits for the calls before it.) */
int cpprob_hip_batch_smooth_device(cpprob_hip_ctx* ctx, uint64_t n_traj, uint64_t draw_index, double* d_marginals, size_t n_doubles, int8_t* d_traj, size_t n_entries);

/* Fixed-lag smoothing of a batch, at the cost of the steps asked for.  With L_b problem b's length (as for cpprob_hip_batch_smooth; an
 * online batch: cpprob_hip_batch_lengths, served whether or not the last advance did its read-out) and lag >= 0:
 *   end step of t      e(t) = min(t + lag, L_b - 1)
 *   fixed-lag marginal G_t[s] = P(x_t = s | y_0 .. y_e(t)): the recursion of cpprob_hip_batch_smooth started at the end step,
 *                      g_e[s] = double(m_e[s]) / double(sum_s m_e[s]), g_u[s] = sum over s' = 0..k-1 of (a_u[s'][s] / D_u[s']) g_{u+1}[s']
 *                      for u = e - 1 .. t (terms with g_{u+1}[s'] = 0 left out, the sums in that order, every product one rounded
 *                      operation, nothing contracted), G_t = g_t
 *   lag = 0: the normalised filtering masses.  t >= L_b - 1 - lag: row t of cpprob_hip_batch_smooth's marginals, bit for bit (the
 *   same device function walks both).  t + lag <= L_b - 1: step t is FINAL -- G_t reads rows t .. t + lag alone and is the same at
 *   every later length, however an online batch was cut into advances.
 *   window             the last W_b = min(lag + 1, L_b) steps, those whose end is L_b - 1
 *   windowed trajectories: the backward simulation of cpprob_hip_batch_smooth stopped after W_b steps; the draws keep the absolute step
 *                      (2^41 + (draw_index << 24) + t, group j >> 1, word pair j & 1), so a window row is the same row of
 *                      cpprob_hip_batch_smooth with the same n_traj and draw_index.
 * Marginals: [B][n_rows][stats_per_predict] doubles; row r of problem b is G_{from_b + r} for from_b + r < L_b, every other row and
 * the states >= k are zero.  h_from: [B], or NULL for all 0.  n_rows >= max over b of (L_b - from_b).  Trajectories: problem b's
 * [W_b][n_traj] entries (row r is step L_b - W_b + r), packed as cpprob_hip_batch_smooth_layout lays out the lengths W_b.  Either
 * output may be NULL; n_traj may be 0.  keep_history = 1 only, and only after a run (else CPPROB_HIP_ESTATE).  CPPROB_HIP_EINVAL
 * (nothing written; the message names the problem where one is at fault): from_b > L_b, n_rows too small, lag > 2^24, a capacity too
 * small, draw_index >= 2^16, n_traj > 2^20, a problem longer than 2^24.
 * Cost.  An online batch's m table is addressed by capacity (64 B times the sum of the capacities, the context's own allocation, made
 * on first use, not part of the batch workspace) and kept: this call, cpprob_hip_batch_smooth and _smooth_device count only the rows
 * that arrived since the last of them, and any batch begin forgets the table.  The call's own work is the rows asked for times
 * (lag + 1) k^2, whatever length the stream has reached.  A run batch (cpprob_hip_batch_run rewrites the store) caches nothing: this
 * call counts the rows it reads, the full calls every row.  The call changes nothing any other entry point returns.
 * Host copies: h_traj int32.  Stages on the device and widens.  Synchronises. */
int cpprob_hip_batch_smooth_lag(cpprob_hip_ctx* ctx, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, uint64_t n_traj, uint64_t draw_index,
                                double* h_marginals, size_t n_doubles, int32_t* h_traj, size_t n_entries);
/* The same left on the device, enqueued on the context's stream after the run / advance, no host synchronisation: d_traj int8 (h_from
 * stays a host array, read before the call returns). */
int cpprob_hip_batch_smooth_lag_device(cpprob_hip_ctx* ctx, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, uint64_t n_traj, uint64_t draw_index,
                                       double* d_marginals, size_t n_doubles, int8_t* d_traj, size_t n_entries);
/* The grids of the context's last smoothing call (any of the four above), host only: gridDim.y of its counting launch -- a workgroup
 * walks the rows of its problem that far apart -- and of its fixed-lag launch -- a wavefront takes the end steps 4 times that far
 * apart --, 0 where the launch did not happen (or no batch is begun).  The results do not depend on either; tests read them to know
 * how many rounds and trips a shape produced. */
int cpprob_hip_batch_smooth_grid(cpprob_hip_ctx* ctx, uint32_t* count_grid_y, uint32_t* lag_grid_y);

/* Expected sufficient statistics of a batch (csrc/batch_suffstats.hpp): the E-step of an EM fit of the problems' tables, from the
 * backward smoother's own walk.  The term the recursion of cpprob_hip_batch_smooth forms for (s', s) at step t,
 * (a_t[s'][s] / D_t[s']) g_{t+1}[s'], is the two-slice posterior P(x_t = s, x_{t+1} = s' | y); with T_b problem b's length and y_t
 * its observes the call returns, a problem,
 *   xi[s][s'] = sum over t = T_b - 2 .. 0 of that term      (expected transitions s -> s')
 *   occ[s]    = sum over t = T_b - 1 .. 0 of g_t[s]         (expected visits)
 *   occ_y[s]  = sum over t of g_t[s] * y_t,   occ_yy[s] = sum over t of g_t[s] * (y_t * y_t)
 * every accumulator from 0.0, one addition a step in that order of t, every product one rounded multiplication, nothing contracted:
 * g_t are cpprob_hip_batch_smooth's marginals bit for bit and the record is a pure function of integers and IEEE operations.
 * Record: 88 doubles a problem -- xi at 8 s + s', then occ[8], occ_y[8], occ_yy[8]; states >= k are zero, a problem of length 0 is
 * all zero, a problem of length 1 has xi = 0.  n_doubles >= 88 n_problems.
 * Observes: the problems' sequences packed one after the other by the lengths reached (cpprob_hip_batch_begin_problems' layout; a
 * uniform batch: [B][T]), n_observes their total; NULL (n_observes is then not read): occ_y and occ_yy stay zero.
 * keep_history = 1 only, and only after a run (else CPPROB_HIP_ESTATE); CPPROB_HIP_EINVAL (nothing written): a capacity too small,
 * n_observes not the sum of the lengths, a problem longer than 2^24.  The call shares the m table and its counting pass with the
 * smoothing calls above (an online batch: whichever of them comes first counts the new rows, none counts a row twice) and changes
 * nothing any other entry point returns.  Synchronises. */
int cpprob_hip_batch_smooth_stats(cpprob_hip_ctx* ctx, const double* h_observes, size_t n_observes, double* h_stats, size_t n_doubles);
/* The same between device buffers, enqueued on the context's stream after the run / advance, no host synchronisation. */
int cpprob_hip_batch_smooth_stats_device(cpprob_hip_ctx* ctx, const double* d_observes, size_t n_observes, double* d_stats, size_t n_doubles);

/* Running sufficient statistics of an online batch, forward-only (csrc/batch_onlinestats.hpp): the 88 numbers of
 * cpprob_hip_batch_smooth_stats at the lengths the stream has reached, for the cost of the steps that arrived since the last call --
 * the backward walk above pays every row of the m table on every call.  The forward-only smoothing of additive functionals (Cappe
 * 2011; Del Moral, Doucet & Singh 2010): for every current state s' the batch keeps
 *   tau_t[s'][.] = E[statistics of steps 0..t | x_t = s', y_0..y_t]                 ([8][88] doubles a problem, on the device)
 * and pushes it one step with the backward kernel the smoother forms from row t - 1 of the m table.  In exact arithmetic the record
 * equals cpprob_hip_batch_smooth_stats'; in doubles the two differ by rounding (a few T 2^-52, relative to max(1, |value|)).
 * State, for the life of an online batch: tau and, a problem, done_b = the steps consumed (host state).  Any batch begin resets both.
 * Per problem (k states; m_t its rows of the m table, states >= k zero; p[s][s'] = double(P[s][s']) as above; column j of a row of tau
 * as the record's: 8 s + s'' for xi[s][s''], 64 + s occ, 72 + s occ_y, 80 + s occ_yy), consuming step t = done_b with observe y:
 *   t = 0:   tau'[s'][.] = 0.0
 *   t >= 1, m = m_{t-1}:  a[s'][s] = m[s] * p[s][s'] (one rounded product);  D[s'] = sum of a[s'][s] in the order s = 0..7 from 0.0;
 *            Dm the same sum of m[s];  w[s'][s] = m[s] / Dm where D[s'] == 0.0 (the defensive rule), else a[s'][s] / D[s']
 *            tau'[s'][j] = sum over s = 0..k-1 ascending, from 0.0, of w[s'][s] * v (one rounded product),
 *            v = tau[s][j] + 1.0 (one rounded addition) where j == 8 s + s', else tau[s][j]
 *   then     tau'[s'][64 + s'] += 1.0,  tau'[s'][72 + s'] += y,  tau'[s'][80 + s'] += y * y;  rows s' >= k stay 0.0
 * Read-out at length L_b (tau unchanged): L_b = 0: 88 zeros; else g[s'] = double(m_{L_b-1}[s']) / double(sum of m_{L_b-1}) and
 *   out[j] = sum over s' = 0..k-1 ascending, from 0.0, of g[s'] * tau[s'][j];  states >= k of the record are zero.
 * Nothing is contracted: the record is a pure function of integers and IEEE operations, the same bits however the stream was cut into
 * advances and calls.  After the call done_b = L_b; a call without new steps returns the same record again.
 * Observes: those of the steps the call consumes -- problem b's L_b - done_b values, packed in problem order; called after every
 * advance, the advance's own h_observes.  n_observes must equal that total exactly.  NULL with n_observes = 0: every consumed step
 * takes y = 0.0 (its occ_y, occ_yy terms are zero).  h_stats: [n_problems][88], n_doubles >= 88 n_problems.
 * CPPROB_HIP_ESTATE: no batch is begun; the batch was not begun by cpprob_hip_batch_begin_online; a filtering-only batch
 * (keep_history = 0) without CPPROB_HIP_BATCH_KEEP_MASSES.  CPPROB_HIP_EINVAL: n_observes not the steps consumed (or nonzero with
 * NULL observes), n_doubles < 88 n_problems, a NULL stats.  After any refusal nothing has changed: the next correct call returns the
 * bits it would have returned.  The call shares the m table and its counting pass with the smoothing calls above (none counts a row
 * twice) and changes nothing any other entry point returns.  Stages the observes and the records on the device.  Synchronises. */
int cpprob_hip_batch_online_stats(cpprob_hip_ctx* ctx, const double* h_observes, size_t n_observes, double* h_stats, size_t n_doubles);
/* The same between device buffers, enqueued on the context's stream after the advance, no host synchronisation. */
int cpprob_hip_batch_online_stats_device(cpprob_hip_ctx* ctx, const double* d_observes, size_t n_observes, double* d_stats, size_t n_doubles);
/* done_b of every problem ([n_problems]), host only: the steps the running statistics have consumed.  CPPROB_HIP_ESTATE without an
 * online batch. */
int cpprob_hip_batch_online_stats_progress(cpprob_hip_ctx* ctx, uint32_t* h_done);

/* Trajectory sufficient statistics of a batch (csrc/batch_trajstats.hpp): the complete-data statistics of backward-simulated
 * trajectories, counted on the device while they are drawn -- what a Gibbs sweep over a table, a stochastic EM step or a
 * posterior-predictive check reads of a trajectory.  Trajectory j of problem b under draw_index is exactly column j of
 * cpprob_hip_batch_smooth's trajectories for that draw_index (the same start rule, the same pick, the Philox block
 * draw_block(seed_b, j >> 1, 2^41 + (draw_index << 24) + t), word pair j & 1) and does not depend on n_traj; it is not stored.  With
 * x_0 .. x_{T-1} the trajectory, T = T_b the length reached and y_t the observes, walking t = T - 1 .. 0:
 *   xi[s][s'] = #{t < T - 1 : x_t = s, x_{t+1} = s'}          occ[s] = #{t : x_t = s}
 *   occ_y[x_t] = occ_y[x_t] + y_t,   occ_yy[x_t] = occ_yy[x_t] + (y_t * y_t)
 * every accumulator from 0.0, one addition a step in that order of t, the product one rounded multiplication, nothing contracted;
 * the counts are integers written as doubles.
 * Record: 88 doubles a trajectory in cpprob_hip_batch_smooth_stats' layout -- xi at 8 s + s', then occ[8], occ_y[8], occ_yy[8];
 * states >= k are zero, a problem of length 0 is all zero, a problem of length 1 has xi = 0.  Output [n_problems][n_traj][88],
 * uniform and not packed; n_doubles >= 88 n_problems n_traj.
 * Observes: as cpprob_hip_batch_smooth_stats takes them, packed by the lengths reached; NULL (n_observes is then not read): occ_y
 * and occ_yy stay zero.
 * keep_history = 1 or CPPROB_HIP_BATCH_KEEP_MASSES, and only after a run / advance (else CPPROB_HIP_ESTATE); CPPROB_HIP_EINVAL
 * (nothing written): n_traj = 0 or above 2^20, draw_index >= 2^16, a capacity too small, n_observes not the sum of the lengths, a
 * problem longer than 2^24.  A batch with nothing reached yet gets zeros.  The call shares the m table and its counting pass with
 * the smoothing calls above (an online batch: none counts a row twice) and changes nothing any other entry point returns.
 * Synchronises. */
int cpprob_hip_batch_traj_stats(cpprob_hip_ctx* ctx, uint64_t n_traj, uint64_t draw_index, const double* h_observes, size_t n_observes, double* h_stats,
                                size_t n_doubles);
/* The same between device buffers, enqueued on the context's stream after the run / advance, no host synchronisation. */
int cpprob_hip_batch_traj_stats_device(cpprob_hip_ctx* ctx, uint64_t n_traj, uint64_t draw_index, const double* d_observes, size_t n_observes, double* d_stats,
                                       size_t n_doubles);
/* gridDim.y of the context's last trajectory statistics launch, host only: the tiles of 256 trajectories a problem; 0 where none
 * happened since the last smoothing, forecast, decode or statistics call (or no batch is begun).  The records do not depend on it. */
int cpprob_hip_batch_traj_stats_grid(cpprob_hip_ctx* ctx, uint32_t* grid_y);

/* Conditional SMC runs of a batch (csrc/batch_csmc.hpp): the forward pass of particle Gibbs with backward sampling.  Either call
 * takes the place of cpprob_hip_batch_run on a batch begun by cpprob_hip_batch_begin or _begin_problems with model
 * CPPROB_HIP_MODEL_HMM_TABLE, keep_history = 0 and CPPROB_HIP_BATCH_KEEP_MASSES.  Problem b runs with Philox key h_seeds[b] and with
 * one particle, slot 0, pinned to its reference path r_0 .. r_{T_b - 1}: the paths are packed problem after problem, problem b's
 * entries from first[b] of cpprob_hip_batch_smooth_layout(T, B, 1) on -- what cpprob_hip_batch_smooth_device writes with
 * n_traj = 1 -- and n_entries is their total, the sum of the T_b.  The run writes the batch's m table (the counts of a row include
 * slot 0) and nothing else.  A sweep "conditional run on the previous trajectory, then one backward-simulated trajectory" leaves
 * the smoothing law invariant at every n_particles >= 1, up to the 32-bit quantisation of weights and thresholds.
 * The resampling of a conditional run is multinomial whatever cfg.resampler says: conditional SMC with multinomial resampling
 * followed by backward sampling is the form whose invariance is proven (Whiteley 2010; Lindsten & Schon 2013), and on discrete states
 * it is the cheap one -- a particle's ancestor matters through the ancestor's state alone, a draw from the k masses of the previous
 * row, so there is no comb, no ancestor array and no particle store.  Per slot i >= 1: t = 0: x = smallint_from_word(w, 0, k - 1), w
 * word i & 3 of draw_block(seed, i >> 2, 0); t >= 1: C_s the inclusive sums of the integer masses of row t - 1, S = C_{k-1},
 * W = (hi << 32) | lo from words 2 (i & 1), 2 (i & 1) + 1 of draw_block(seed, i >> 1, 2^43 + t), V = the high 64 bits of W S,
 * a = #{s < k-1 : V >= C_s}, x = #{j < k-1 : w >= c[a][j]} with w word i & 3 of draw_block(seed, i >> 2, t) and c the thresholds.
 * After a conditional run every entry point that serves a CPPROB_HIP_BATCH_KEEP_MASSES batch from its m table, tables and seeds serves
 * this one unchanged, the run's seeds its Philox keys: cpprob_hip_batch_copy_masses, _smooth*, _smooth_lag*, _smooth_stats*,
 * _traj_stats*, _forecast*, _predictive* and _decode* (none of them reads anything else of a run).  A conditional run keeps masses,
 * not books: cpprob_hip_batch_results and _results_device return CPPROB_HIP_ESTATE until the next cpprob_hip_batch_run, which
 * returns exactly what it returns without the conditional run before it.
 * The host form validates every entry (0 <= r < k) and stages the paths as int8; it synchronises.  CPPROB_HIP_ESTATE: no batch begun,
 * keep_history = 1, no CPPROB_HIP_BATCH_KEEP_MASSES; CPPROB_HIP_EUNSUPPORTED: CPPROB_HIP_MODEL_HMM3, an online batch;
 * CPPROB_HIP_EINVAL (nothing enqueued): a NULL pointer, n_entries not the sum of the T_b, an entry out of range. */
int cpprob_hip_batch_run_conditional(cpprob_hip_ctx* ctx, const uint64_t* h_seeds, const int32_t* h_ref, size_t n_entries);
/* The same with the paths in a device buffer of int8, enqueued on the context's stream, no host synchronisation.  The entries are not
 * validated: the low three bits of one count, and a value >= k is taken as k - 1.  d_ref is read by the run, in stream order; the caller
 * keeps it alive and unchanged by other streams until the run has finished. */
int cpprob_hip_batch_run_conditional_device(cpprob_hip_ctx* ctx, const uint64_t* h_seeds, const int8_t* d_ref, size_t n_entries);

/* Forecasts of a batch (csrc/batch_forecast.hpp): what lies ahead of the last observe, from the smoother's m table and the transition
 * law the device itself draws from.  Per problem b (L_b the length reached, k its states, m_t its rows of the m table, P[s][s'] the
 * integer transition masses of cpprob_hip_batch_smooth):
 *   p[s][s']           = double(P[s][s']) * 2^-32 (exact)
 *   push(f)[s']        = sum over s = 0..k-1, in that order, of f[s] * p[s][s'] (every product one rounded operation, nothing
 *                      contracted; the sum from 0.0, terms with f[s] = 0 left out)
 *   forecast marginals f_0 = the last row of cpprob_hip_batch_smooth's marginals (the normalised filtering masses of step L_b - 1, the
 *                      same device function); f_h = push(f_{h-1}) = P(x_{L_b-1+h} | y_0 .. y_{L_b-1}), h = 1 .. horizon
 *   simulated futures  trajectory j: row 0, the present state, drawn from m_{L_b-1} by the backward simulation's start rule with the
 *                      53-bit uniform of word pair j & 1 of Philox block (seed_b, group j >> 1, ordinal 2^42 + (draw_index << 24));
 *                      row h >= 1: x_h = #{i < k-1 : w >= c[x_{h-1}][i]}, c the threshold words and w the 32-bit word 2 (j & 1) of
 *                      block (seed_b, j >> 1, 2^42 + (draw_index << 24) + h): the forward draw's own statement, so the law is P
 * Marginals: [B][horizon][stats_per_predict] doubles, row h - 1 is f_h, states >= k zero.  Trajectories: [B][horizon + 1][n_traj]
 * (uniform, not packed: every problem has the same horizon).  A problem of length 0 has rows of zeros in both.  Either output may be
 * NULL; n_traj may be 0 when the trajectories are NULL.  Needs the particle store (keep_history = 1) or CPPROB_HIP_BATCH_KEEP_MASSES,
 * and a run or advance before it (else CPPROB_HIP_ESTATE).  CPPROB_HIP_EINVAL (nothing written): horizon 0 or >= 2^24,
 * draw_index >= 2^16, n_traj > 2^20, a capacity too small, a problem longer than 2^24.
 * Cost: horizon k^2 and horizon n_traj, whatever length the stream has reached.  The m table is the smoothing calls': a
 * CPPROB_HIP_BATCH_KEEP_MASSES batch reads the rows its run kept, an online batch with history counts the rows that arrived since
 * the last call that counted (none counts a row twice), a run batch counts row L_b - 1.  The call changes nothing any other entry
 * point returns.  Host copies: h_traj int32.  Stages on the device and widens.  Synchronises. */
int cpprob_hip_batch_forecast(cpprob_hip_ctx* ctx, uint64_t horizon, uint64_t n_traj, uint64_t draw_index, double* h_marginals, size_t n_doubles,
                              int32_t* h_traj, size_t n_entries);
/* The same left on the device, enqueued on the context's stream after the run / advance, no host synchronisation: d_traj int8. */
int cpprob_hip_batch_forecast_device(cpprob_hip_ctx* ctx, uint64_t horizon, uint64_t n_traj, uint64_t draw_index, double* d_marginals, size_t n_doubles,
                                     int8_t* d_traj, size_t n_entries);
/* One-step predictive rows: the law every observe was predicted from, r_t = P(x_t | y_0 .. y_{t-1}) for t = 0 .. L_b.
 *   r_0[s] = 1.0 / double(k) for s < k (the uniform initial state);  r_t = push(normalised filtering masses of step t - 1), t >= 1
 * r_{L_b} is row h = 1 of cpprob_hip_batch_forecast bit for bit; r_t reads row t - 1 of the m table alone, so it is final when it is
 * first available and the same however an online batch was cut into advances.
 * Output: [B][n_rows][stats_per_predict] doubles; row r of problem b is r_{from_b + r} for from_b + r <= L_b, every other row and the
 * states >= k are zero.  h_from: [B] (a host array, read before the call returns), or NULL for all 0.  n_rows >= max over b of
 * (L_b + 1 - from_b).  State and cost as above (a run batch counts rows max(from_b, 1) - 1 .. L_b - 1).  CPPROB_HIP_EINVAL (nothing
 * written; the message names the problem where one is at fault): from_b > L_b + 1, n_rows too small, a capacity too small, a NULL
 * output.  Synchronises. */
int cpprob_hip_batch_predictive(cpprob_hip_ctx* ctx, const uint32_t* h_from, uint64_t n_rows, double* h_rows, size_t n_doubles);
/* The same left on the device, enqueued on the context's stream after the run / advance, no host synchronisation. */
int cpprob_hip_batch_predictive_device(cpprob_hip_ctx* ctx, const uint32_t* h_from, uint64_t n_rows, double* d_rows, size_t n_doubles);

/* Decoding a batch (csrc/batch_decode.hpp): the single most probable state path of every problem given its observes, by dynamic
 * programming over the states the particles occupy (the particle form of the MAP sequence estimate: Godsill, Doucet & West 2001).
 * The per-step argmax of cpprob_hip_batch_smooth's marginals is a different estimator and may name a sequence the transition table
 * forbids; this one cannot.  It reads the smoother's m table, the per-step log-likelihood rows and the threshold words, and touches no
 * particle.  Per problem b (L_b the length reached, k its states, m_t its rows of the m table, ll_t[s] the log-likelihood of observe
 * t in state s, P[s][s'] the integer transition masses of cpprob_hip_batch_smooth):
 *   lp[s][s']  = log(double(P[s][s']) * 2^-32), -inf where P = 0;  lp0 = log(1.0 / double(k)): computed on the HOST (std::log), the
 *                table cpprob_hip_batch_decode_logp returns; the device evaluates no logarithm
 *   support      S_t = { s < k : m_t[s] > 0 }
 *   v_0[s]     = lp0 + ll_0[s] for s in S_0, else -inf;  bp_0[.] = 0
 *   t >= 1, s' < k: best = -inf, arg = 0; for s = 0 .. k-1 in that order c = v_{t-1}[s] + lp[s][s'], taken if c > best (strict: ties
 *                go to the lowest s, an all -inf column keeps arg = 0);  bp_t[s'] = arg;  v_t[s'] = best + ll_t[s'] for s' in S_t,
 *                else -inf.  Every sum is one IEEE addition.
 *   end_t      = the first s of the same strict scan over v_t[0..k)
 *   step word    w_t = sum over s' < 8 of bp_t[s'] << (3 s') | end_t << 24
 *   full decode  x_{L-1} = end_{L-1};  x_{t-1} = (w_t >> 3 x_t) & 7;  score = v_{L-1}[end_{L-1}], the log joint density of the path
 *                and the observes under the realised law
 * On a store a run wrote every supported state has a finite candidate; the -inf rules are defensive.
 * Path: problem b's L_b entries from h_first[b] on, exactly cpprob_hip_batch_smooth_layout with n_traj = 1.  h_score: [B]; a problem
 * of length 0 owns no entries and has score 0.  Either output may be NULL.  State as for the smoothing calls: the particle store
 * (keep_history = 1) or CPPROB_HIP_BATCH_KEEP_MASSES, and a run or advance before it (else CPPROB_HIP_ESTATE).  CPPROB_HIP_EINVAL
 * (nothing written): a capacity too small, a problem longer than 2^24.
 * Cost.  The step words (4 B a row of the m table, addressed as it is), a v row of 8 doubles a problem and the log tables are
 * allocations of the context's own, made on first use.  An online batch keeps its words as it keeps the m table: a call walks the
 * steps that arrived since the last decode call -- a stream fed one observe at a time does L steps of forward work in all, not
 * L^2 / 2 -- and any batch begin forgets them.  A run batch caches nothing.  The counting pass and its watermark are the smoothing
 * calls': no row is counted twice.  The call changes nothing any other entry point returns.
 * Host copies: h_path int32.  Stages on the device and widens.  Synchronises. */
int cpprob_hip_batch_decode(cpprob_hip_ctx* ctx, int32_t* h_path, size_t n_entries, double* h_score, size_t n_doubles);
/* The same left on the device, enqueued on the context's stream after the run / advance, no host synchronisation: d_path int8. */
int cpprob_hip_batch_decode_device(cpprob_hip_ctx* ctx, int8_t* d_path, size_t n_entries, double* d_score, size_t n_doubles);
/* Fixed-lag decoding on the same words: e(t) = min(t + lag, L_b - 1), X_t = the state at t of the traceback started at end_{e(t)}.
 * X_t is FINAL once lag more observes have arrived -- it reads the words t + 1 .. e(t) alone and is the same at every later length,
 * however an online batch was cut into advances; the rows with e(t) = L_b - 1 are cpprob_hip_batch_decode's.
 * States: [B][n_rows]; row r of problem b is X_{from_b + r} for from_b + r < L_b, every other row is -1 (0 is a state).  h_from: [B]
 * (a host array, read before the call returns), or NULL for all 0.  n_rows >= max over b of (L_b - from_b).  h_score as above (the
 * full decode's).  Either output may be NULL.  State and cost as above; the traceback's own work is the rows asked for times lag.
 * CPPROB_HIP_EINVAL (nothing written; the message names the problem where one is at fault): from_b > L_b, n_rows too small,
 * lag > 2^24, a capacity too small, a problem longer than 2^24.  Host copies: h_states int32.  Synchronises. */
int cpprob_hip_batch_decode_lag(cpprob_hip_ctx* ctx, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, int32_t* h_states, size_t n_entries,
                                double* h_score, size_t n_doubles);
/* The same left on the device, enqueued on the context's stream after the run / advance, no host synchronisation: d_states int8. */
int cpprob_hip_batch_decode_lag_device(cpprob_hip_ctx* ctx, uint64_t lag, const uint32_t* h_from, uint64_t n_rows, int8_t* d_states, size_t n_entries,
                                       double* d_score, size_t n_doubles);
/* The log table of `problem` in the batch last begun: h_lp[8 s + s'] = lp[s][s'] (-inf outside the k x k table), *h_lp0 = lp0 -- the
 * doubles the decode kernels were or will be given, so that a restatement of a run depends on no second logarithm.  Host state only:
 * no device work, no synchronisation -- but after cpprob_hip_batch_retable_device, whose thresholds the first call fetches (it waits
 * for the stream once).  CPPROB_HIP_ESTATE: no batch begun. */
int cpprob_hip_batch_decode_logp(cpprob_hip_ctx* ctx, uint64_t problem, double h_lp[64], double* h_lp0);
/* The grids of the context's last decode, forecast or predictive call (any form of them), host only, as cpprob_hip_batch_smooth_grid
 * reports the smoother's: gridDim.x of the decode's forward launch -- a workgroup takes 4 problems, the problems 4 times that far
 * apart --, gridDim.y of its traceback launch -- row 0 the end L - 1, a lane of the rows behind it an earlier end, the ends
 * 256 (gridDim.y - 1) apart --, gridDim.y of the forecast launch -- 1 + the tiles of 1024 trajectories -- and gridDim.y of the
 * predictive launch -- a wavefront takes the rows 4 times that far apart.  0 where the launch did not happen (or no batch is begun);
 * every batch call that smooths, forecasts or decodes resets all four.  The results do not depend on them; tests read them to know
 * how many trips a shape produced. */
int cpprob_hip_batch_pass_grid(cpprob_hip_ctx* ctx, uint32_t* decode_forward_grid_x, uint32_t* decode_trace_grid_y, uint32_t* forecast_grid_y,
                               uint32_t* predictive_grid_y);

/* Re-tabling a begun batch (csrc/batch_retable.hpp): new tables for a batch of CPPROB_HIP_MODEL_HMM_TABLE problems where it stands --
 * what a fitting loop changes between two sweeps (72 doubles a problem) without the begin's host work.  The launch rewrites, from the
 * observes and the new tables, what a begin derives from a table: the rows log N(y_t; mean[s], 1) of every step t < T_b (-inf for
 * s >= k) and the 64 threshold words of every problem.  The row's logarithm, log(2 pi), is evaluated once on the host with the begin's
 * own expression; the device performs a subtraction, a product, a sum and a product by -0.5, none contracted, and the thresholds'
 * division, product and ceil: EVERYTHING the batch returns afterwards is, bit for bit, what cpprob_hip_batch_begin_problems with these
 * tables and the same observes returns.  Lengths, particle counts, dispatch order, descriptors and workspace stay; no workspace region
 * is added (the status words, and the host form's copy of the observes, are allocations of the context's own).
 * d_means [B][k], d_transition [B][k][k], k the batch's; d_observes packed as cpprob_hip_batch_begin_problems packs them, n_observes
 * the sum of the lengths (else CPPROB_HIP_EINVAL).  A re-table is a begin as far as results go: until the next cpprob_hip_batch_run or
 * cpprob_hip_batch_run_conditional* every read-out returns CPPROB_HIP_ESTATE.
 * The tables are checked on the device (status bits: 1 a weight not finite or not >= 0, 2 a transition row without mass, 4 a mean not
 * finite): a problem with a bit set keeps its previous rows and thresholds -- its next run is the old table's run -- and
 * cpprob_hip_batch_retable_status names it.
 * Serves a batch begun by cpprob_hip_batch_begin_problems with CPPROB_HIP_MODEL_HMM_TABLE (per-problem tables or the context's),
 * keep_history 1 or 0, with or without CPPROB_HIP_BATCH_KEEP_MASSES, before or after runs.  CPPROB_HIP_EUNSUPPORTED, the message saying
 * why: CPPROB_HIP_MODEL_HMM3 (its table is the model's), a cpprob_hip_batch_begin batch (one shared table), an online batch (its
 * advances evaluate rows from host means).  CPPROB_HIP_ESTATE: no batch begun.  After any refusal nothing has changed.
 * Enqueued on the context's stream, no host synchronisation (stream contract as cpprob_hip_batch_smooth_stats_device: the caller's
 * buffers are complete before the call and live until the stream has passed it).  After this form the host's mirrors of the tables
 * are stale: cpprob_hip_batch_copy_store fetches the one row it needs, and the first decode call (or cpprob_hip_batch_decode_logp)
 * after it fetches the threshold words, which waits for the stream once. */
int cpprob_hip_batch_retable_device(cpprob_hip_ctx* ctx, const double* d_means, const double* d_transition, const double* d_observes, size_t n_observes);
/* The same from host arrays.  The tables are validated on the host as cpprob_hip_batch_begin_problems validates them (the same codes,
 * the same messages naming the problem; nothing changes on a refusal), staged on the device and enqueued; the observes are copied into
 * a buffer of the context's own.  h_observes may be NULL when the context still holds the copy a previous cpprob_hip_batch_retable of
 * THIS begun batch staged (any begin forgets it; NULL without one: CPPROB_HIP_EINVAL) -- a loop that draws its tables on the host
 * uploads the observes once.  n_observes is checked either way.  The host arrays may be reused when the call returns. */
int cpprob_hip_batch_retable(cpprob_hip_ctx* ctx, const double* h_means, const double* h_transition, const double* h_observes, size_t n_observes);
/* The status words of the last re-table of the begun batch, [n_problems]: 0, or the bits above.  Synchronises.  CPPROB_HIP_ESTATE: the
 * begun batch has not been re-tabled. */
int cpprob_hip_batch_retable_status(cpprob_hip_ctx* ctx, int32_t* h_status);
/* gridDim.y of the last re-table launch, host only, as cpprob_hip_batch_smooth_grid: a workgroup writes 32 rows a trip, the grid holds
 * min(ceil(T_max / 32), 64, max(1, 4096 / n_problems)) of them a problem and strides beyond.  0: none since the begin (or no batch). */
int cpprob_hip_batch_retable_grid(cpprob_hip_ctx* ctx, uint32_t* grid_y);
/* The M-step of particle EM on the device: from the records of cpprob_hip_batch_smooth_stats (d_stats [n_problems][88], n_doubles >=
 * 88 n_problems) d_means [B][k] and d_transition [B][k][k] are updated in place, a state s < k of a problem:
 *   row = ((0.0 + xi[s][0]) + xi[s][1]) + ... in that order;  row > 0: trans[s][j] = xi[s][j] / row;  occ[s] > 0: means[s] = occ_y[s] / occ[s]
 * a row or a state without mass keeps its value -- cpprob_amd.em.m_step and cpprob::gpu::hmm_table_fit bit for bit.  k and
 * n_problems are the begun batch's (CPPROB_HIP_MODEL_HMM_TABLE, else CPPROB_HIP_EUNSUPPORTED; none begun: CPPROB_HIP_ESTATE).
 * Enqueued on the context's stream, no host synchronisation. */
int cpprob_hip_batch_mstep_device(cpprob_hip_ctx* ctx, const double* d_stats, size_t n_doubles, double* d_means, double* d_transition);
/* Problem `problem`'s rows of the per-step table as the device holds them, h_rows [T_b][8] (n_doubles >= 8 T_b; an online batch: the
 * length reached), and its 64 threshold words (h_thr, or NULL; a cpprob_hip_batch_begin batch: the shared table's).  Any begun batch;
 * CPPROB_HIP_MODEL_HMM3 keeps no threshold words on the device: h_thr must be NULL (CPPROB_HIP_EINVAL).  Synchronises.  A test
 * compares a re-tabled batch with a freshly begun one through it. */
int cpprob_hip_batch_copy_step_tables(cpprob_hip_ctx* ctx, uint64_t problem, double* h_rows, size_t n_doubles, uint64_t* h_thr);
/* {log_evidence, ess_final, log_norm, max_logw} of every problem into d_out [n_problems][4]: the head of
 * cpprob_hip_batch_results_device's rows without the statistics behind it, so that a loop resident on the device keeps every
 * iteration's evidence for 4 doubles a problem.  State as cpprob_hip_batch_results_device.  Enqueued, no host synchronisation. */
int cpprob_hip_batch_summaries_device(cpprob_hip_ctx* ctx, double* d_out);

/* ---- online EM: an online batch whose tables are learned on the device while its observes arrive (csrc/batch_learn.hpp) --
 * The stochastic-approximation form of Cappe 2011, Alg. 1: every step discounts the running statistics by 1 - gamma[t] and adds the
 * new ones with weight gamma[t]; the M-step on the running record gives new tables; the next observes are filtered under them.
 * cpprob_hip_batch_learn_begin arms the batch begun by cpprob_hip_batch_begin_online (CPPROB_HIP_MODEL_HMM_TABLE with per-problem
 * tables; keep_history = 1, or keep_history = 0 with CPPROB_HIP_BATCH_KEEP_MASSES): the step sizes h_gamma[t], 0 < gamma <= 1,
 * indexed by a problem's absolute step (n_gamma >= the largest capacity; the host evaluates them, the device takes no power), the
 * burn-in t_min -- the length a problem must have reached before its first M-step -- and a device-resident copy of every problem's
 * table (means [B][k], transition [B][k][k]; allocations of the context's own, no workspace region is added).
 * CPPROB_HIP_ESTATE: no online batch begun, a filtering-only batch without the masses bit, or an advance has been made.
 * CPPROB_HIP_EUNSUPPORTED: CPPROB_HIP_MODEL_HMM3, or a batch begun with the context's shared table.  CPPROB_HIP_EINVAL: n_gamma below
 * the largest capacity, a gamma outside (0, 1].  Any begin disarms.  After any refusal nothing has changed. */
int cpprob_hip_batch_learn_begin(cpprob_hip_ctx* ctx, const double* h_gamma, size_t n_gamma, uint32_t t_min);
/* A learning advance: problem b receives h_dT[b] >= 0 new observes (packed problem after problem, as cpprob_hip_batch_advance takes
 * them; the capacity check and its message are that call's).  Three steps are enqueued and the call returns without waiting:
 *   rows   the rows of the steps [L_b, L_b + dT_b) from the observes and the device tables in force, the statements of a begin's
 *          rows (log(2 pi) from the host, nothing contracted); rows a problem has taken before are not touched
 *   run    the launch cpprob_hip_batch_advance makes over the new steps (keep_history = 1: with the read-out walk, readout = 1)
 *   learn  a wavefront a problem: for every new step t, with g = gamma[t] and om = 1.0 - g, the discounted forward recursion
 *            tau'[s'][j] = sum over s ascending of w[s'][s] (om tau[s][j] + g [j == 8 s + s']),  w as cpprob_hip_batch_online_stats',
 *            tau'[s'][64 + s'] += g,  tau'[s'][72 + s'] += g y,  tau'[s'][80 + s'] += g (y y)      (step 0: from zeros)
 *          on a tau of the learner's own (cpprob_hip_batch_online_stats keeps its sums); the record [88] at the new length, read out
 *          as that call reads its own; and, where dT_b > 0 and the new length is >= t_min, cpprob_hip_batch_mstep_device's M-step on
 *          the record: the new table is checked (the status bits of cpprob_hip_batch_retable_device) and either replaces the device
 *          table and the problem's 64 threshold words (status 0) or is dropped (the old table and words stay, status = the bits).
 * With gamma[t] = 1 / (t + 1) the record is the running mean of cpprob_hip_batch_online_stats' sums.
 * Tables change only between advances: the chunk is the caller's update period.  The summaries' log_evidence is the prequential
 * likelihood under the tables in force at each step.  Smoothing, forecast, decode and statistics calls read the m table with the
 * CURRENT threshold words for every row.  The host's mirrors of rows and thresholds are stale afterwards, exactly as after
 * cpprob_hip_batch_retable_device: cpprob_hip_batch_copy_store and the decode calls fetch what they need.
 * CPPROB_HIP_ESTATE: the batch is not armed.  On an armed batch a plain cpprob_hip_batch_advance returns CPPROB_HIP_ESTATE: the two
 * routes do not mix.  After any refusal nothing has changed. */
int cpprob_hip_batch_advance_learn(cpprob_hip_ctx* ctx, const uint32_t* h_dT, const double* h_observes);
/* The same with the observes in device memory (n_observes = the sum of h_dT, else CPPROB_HIP_EINVAL); stream contract as
 * cpprob_hip_batch_online_stats_device. */
int cpprob_hip_batch_advance_learn_device(cpprob_hip_ctx* ctx, const uint32_t* h_dT, const double* d_observes, size_t n_observes);
/* The host route: new tables for the FUTURE steps of an online CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables, armed or
 * not.  The tables are validated as the begin validates them (the same codes and messages naming the problem); they replace the host
 * means the next cpprob_hip_batch_advance evaluates its rows from, the threshold words are uploaded stream-ordered, and on an armed
 * batch the device tables are replaced too.  Past rows stay.  (cpprob_hip_batch_retable* keeps refusing online batches.) */
int cpprob_hip_batch_online_tables(cpprob_hip_ctx* ctx, const double* h_means, const double* h_transition);
/* The device-resident tables of an armed batch, h_means [B][k], h_transition [B][k][k], and the status words [B] (any may be NULL):
 * 0, or the bits of the last M-step that was dropped (a problem no M-step has visited: 0).  Synchronises. */
int cpprob_hip_batch_learn_tables(cpprob_hip_ctx* ctx, double* h_means, double* h_transition, int32_t* h_status);
/* The same tables into device buffers, a stream-ordered copy. */
int cpprob_hip_batch_learn_tables_device(cpprob_hip_ctx* ctx, double* d_means, double* d_transition);
/* The records [n_problems][88] of the last learning advance (n_doubles >= 88 n_problems; none yet: zeros).  Synchronises. */
int cpprob_hip_batch_learn_record(cpprob_hip_ctx* ctx, double* h_stats, size_t n_doubles);

/* ---- per-state emission scales of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables (csrc/batch_scale.hpp) --
 * State s of problem b emits N(mean[b][s], sigma[b][s]) in place of N(mean[b][s], 1).  The step kernel and every pass behind it read
 * the emission through the per-step rows alone, so a scaled batch is run, advanced, smoothed, counted, forecast and decoded by the
 * calls above as they are; what differs is who writes the rows.  Every scaled row, on the host and on the device, is
 *   r = (y - mean) / sigma;  r *= r;  r += log_norm;  r *= -0.5          (-inf for an infinite y and for s >= k)
 * with log_norm = table_log(((2 pi) sigma) sigma), and table_log is a logarithm of the library's own in uncontracted IEEE operations
 * (exponent and mantissa by bit operations, the mantissa folded to [sqrt(1/2), sqrt(2)), twelve terms of the odd series in
 * f = (m - 1) / (m + 1), e ln2_hi + (e ln2_lo + r)): host and device perform the same operations, so that a re-tabled batch is bit
 * for bit a freshly begun one.  table_log(2 pi) has the bits of the C library's log(2 pi): a scaled batch whose sigmas are all 1.0
 * returns, bit for bit, what the unit batch returns.  cpprob_hip_table_log exports the function for tests (x normal, positive,
 * finite; host only). */
double cpprob_hip_table_log(double x);
/* cpprob_hip_batch_begin_problems / _begin_online with h_sigmas [B][k] behind the tables, which must be given (k_in states, h_means,
 * h_transition: CPPROB_HIP_EINVAL where one is NULL; another model: CPPROB_HIP_EUNSUPPORTED).  Validated as those calls validate, and
 * every sigma must be finite and > 0 with a normal finite 2 pi sigma^2 (CPPROB_HIP_EINVAL naming the problem; after a refusal nothing
 * has changed).  The batch remembers that it is scaled: cpprob_hip_batch_advance writes its rows with the statements above. */
int cpprob_hip_batch_begin_problems_scaled(cpprob_hip_ctx* ctx, const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n,
                                           const double* h_observes, int32_t k, const double* h_means, const double* h_transition, const double* h_sigmas);
int cpprob_hip_batch_begin_online_scaled(cpprob_hip_ctx* ctx, const cpprob_hip_batch_config* cfg, const uint32_t* h_Tcap, const uint32_t* h_n,
                                         int32_t k, const double* h_means, const double* h_transition, const double* h_sigmas, const uint64_t* h_seeds);
/* cpprob_hip_batch_retable_device / _retable with d_sigmas / h_sigmas [B][k], for a batch begun by
 * cpprob_hip_batch_begin_problems_scaled (a batch without scales: CPPROB_HIP_ESTATE; cpprob_hip_batch_retable* likewise returns
 * CPPROB_HIP_ESTATE on a scaled batch).  The device checks the table as those calls do and sets status bit 8 where a sigma is not
 * finite, not > 0, or has a 2 pi sigma^2 that is not a normal finite number: such a problem keeps its rows, threshold words, sigmas
 * and log_norms.  The launch takes one logarithm a state (table_log) and stores the sigmas and log_norms in force in arrays of the
 * context's own; no workspace region is added.  Everything else as the unit calls. */
int cpprob_hip_batch_retable_scaled_device(cpprob_hip_ctx* ctx, const double* d_means, const double* d_transition, const double* d_sigmas,
                                           const double* d_observes, size_t n_observes);
int cpprob_hip_batch_retable_scaled(cpprob_hip_ctx* ctx, const double* h_means, const double* h_transition, const double* h_sigmas,
                                    const double* h_observes, size_t n_observes);
/* cpprob_hip_batch_mstep_device with the scales: after that call's statements, a state with occ[s] > 0 takes
 *   v = occ_yy[s] / occ[s] - means'[s] means'[s];   sigmas[s] = v >= sigma_floor sigma_floor ? sqrt(v) : sigma_floor      (a NaN v: the floor)
 * (means' the new mean; a division, a product, a subtraction and the correctly rounded square root, none contracted) -- d_sigmas
 * [B][k] updated in place, and where d_log_norm [B][k] is not NULL, log_norm[s] of the new sigma (NaN for a sigma the check above
 * refuses).  A state without mass keeps mean, sigma and log_norm.  sigma_floor finite and > 0 (else CPPROB_HIP_EINVAL).
 * cpprob_amd.em.m_step with sigmas, bit for bit.  Enqueued, no host synchronisation. */
int cpprob_hip_batch_mstep_scaled_device(cpprob_hip_ctx* ctx, const double* d_stats, size_t n_doubles, double* d_means, double* d_transition,
                                         double* d_sigmas, double* d_log_norm, double sigma_floor);
/* cpprob_hip_batch_online_tables with h_sigmas [B][k], for a batch begun by cpprob_hip_batch_begin_online_scaled, armed or not (a
 * batch without scales: CPPROB_HIP_ESTATE; cpprob_hip_batch_online_tables likewise returns CPPROB_HIP_ESTATE on a scaled batch). */
int cpprob_hip_batch_online_tables_scaled(cpprob_hip_ctx* ctx, const double* h_means, const double* h_transition, const double* h_sigmas);
/* Online EM of a scaled online batch (csrc/batch_learn.hpp).  cpprob_hip_batch_learn_begin_scaled is
 * cpprob_hip_batch_learn_begin for a batch begun by cpprob_hip_batch_begin_online_scaled (a batch without scales: CPPROB_HIP_ESTATE;
 * sigma_floor not finite or not > 0: CPPROB_HIP_EINVAL): the learner then fits the sigmas too.  cpprob_hip_batch_advance_learn* are
 * the unchanged calls; on a scaled batch the rows of the new steps are written on the device from the device-resident means, sigmas
 * and log_norms (no logarithm is taken there), and the learn step's M-step is cpprob_hip_batch_mstep_scaled_device's on the record, a
 * state with mass taking sigma' as there and log_norm' = table_log(2 pi sigma'^2); the check adds status bit 8; a table that passes
 * replaces the device table, the sigmas, the log_norms and the 64 threshold words, one that fails leaves all of them.  A plain
 * cpprob_hip_batch_learn_begin on a scaled batch learns means and transition rows and keeps the sigmas: they are read, checked and
 * never written.  cpprob_hip_batch_learn_tables_scaled / _device are cpprob_hip_batch_learn_tables / _device with the sigmas in force,
 * [B][k] (h_sigmas may be NULL); a batch without scales: CPPROB_HIP_ESTATE. */
int cpprob_hip_batch_learn_begin_scaled(cpprob_hip_ctx* ctx, const double* h_gamma, size_t n_gamma, uint32_t t_min, double sigma_floor);
int cpprob_hip_batch_learn_tables_scaled(cpprob_hip_ctx* ctx, double* h_means, double* h_transition, double* h_sigmas, int32_t* h_status);
int cpprob_hip_batch_learn_tables_scaled_device(cpprob_hip_ctx* ctx, double* d_means, double* d_transition, double* d_sigmas);
/* Problem `problem`'s sigmas and log_norms in force as the device holds them, [k] each (either may be NULL).  Synchronises.
 * CPPROB_HIP_ESTATE: no batch begun, or a batch without scales.  For tests. */
int cpprob_hip_batch_copy_scales(cpprob_hip_ctx* ctx, uint64_t problem, double* h_sigmas, double* h_log_norm);

/* ---- Poisson emissions of a CPPROB_HIP_MODEL_HMM_TABLE batch with per-problem tables (csrc/batch_poisson.hpp) --
 * State s of problem b emits Poisson(rate[b][s]); the rates stand where the means stand ([B][k]).  A batch is unit, scaled or Poisson,
 * never two of them: every call of one family on a batch of another returns CPPROB_HIP_ESTATE and leaves the batch as it was.  The
 * step kernel and every pass behind it read the emission through the per-step rows alone, so a Poisson batch is run, advanced,
 * smoothed, counted, forecast and decoded by the calls above as they are.  Every Poisson row, on the host and on the device, is
 *   r = y * log_rate;  r = r - rate;  r = r - lf[y]                      (-inf for s >= k and for a y that is no count)
 * with log_rate = table_log(rate) and lf[c] = lf[c - 1] + table_log(c), lf[0] = lf[1] = 0, a table of 4096 doubles the host fills once
 * a context and uploads (an allocation of the context's own); a count is an integer 0 .. 4095 held in a double -- NaN, infinities,
 * negatives, non-integers and larger values have the row of an infinite observe under the Gaussian routes.  The operations are not
 * contracted: host and device write the same bits.
 * The begins: cpprob_hip_batch_begin_problems / _begin_online with h_rates in place of h_means, which must be given with h_transition
 * (CPPROB_HIP_EINVAL where one is NULL; another model: CPPROB_HIP_EUNSUPPORTED).  Every rate must be > 0, finite and a normal number
 * (CPPROB_HIP_EINVAL naming the problem; after a refusal nothing has changed).  cpprob_hip_batch_advance writes a Poisson batch's rows
 * with the statements above.
 * The re-tables: cpprob_hip_batch_retable_device / _retable with rates.  The device checks the transition rows as those calls do and
 * sets status bit 16 where a rate is not > 0, not finite or not normal (bit 4 is not used): such a problem keeps its rows, threshold
 * words, rates and log-rates.
 * The M-step: cpprob_hip_batch_mstep_device's statements on d_rates (rate = occ_y / occ), then a state with occ[s] > 0 takes
 *   rates[s] = rates[s] >= rate_floor ? rates[s] : rate_floor            (a NaN: the floor)
 * and, where d_log_rates [B][k] is not NULL, log_rates[s] = table_log of it (NaN for a rate the check refuses).  A state without mass
 * keeps both.  rate_floor finite and > 0 (else CPPROB_HIP_EINVAL).  cpprob_amd.em.m_step(emission="poisson"), bit for bit.  Enqueued.
 * cpprob_hip_batch_online_tables_poisson: cpprob_hip_batch_online_tables with rates.  cpprob_hip_batch_learn_begin* on a Poisson batch:
 * CPPROB_HIP_ESTATE (online EM serves the Gaussian families).
 * cpprob_hip_batch_copy_rates: problem `problem`'s rates and log-rates in force as the device holds them, [k] each (either may be
 * NULL); synchronises; CPPROB_HIP_ESTATE: no batch begun, or no Poisson batch.  For tests. */
int cpprob_hip_batch_begin_problems_poisson(cpprob_hip_ctx* ctx, const cpprob_hip_batch_config* cfg, const uint32_t* h_T, const uint32_t* h_n,
                                            const double* h_observes, int32_t k, const double* h_rates, const double* h_transition);
int cpprob_hip_batch_begin_online_poisson(cpprob_hip_ctx* ctx, const cpprob_hip_batch_config* cfg, const uint32_t* h_Tcap, const uint32_t* h_n,
                                          int32_t k, const double* h_rates, const double* h_transition, const uint64_t* h_seeds);
int cpprob_hip_batch_retable_poisson_device(cpprob_hip_ctx* ctx, const double* d_rates, const double* d_transition, const double* d_observes, size_t n_observes);
int cpprob_hip_batch_retable_poisson(cpprob_hip_ctx* ctx, const double* h_rates, const double* h_transition, const double* h_observes, size_t n_observes);
int cpprob_hip_batch_mstep_poisson_device(cpprob_hip_ctx* ctx, const double* d_stats, size_t n_doubles, double* d_rates, double* d_transition,
                                          double* d_log_rates, double rate_floor);
int cpprob_hip_batch_online_tables_poisson(cpprob_hip_ctx* ctx, const double* h_rates, const double* h_transition);
int cpprob_hip_batch_copy_rates(cpprob_hip_ctx* ctx, uint64_t problem, double* h_rates, double* h_log_rates);

/* ---- tied tables: one table for the problems of a group, fitted to their pooled records (csrc/batch_pool.hpp) --
 * A tie is a partition of the begun batch's problems and nothing else: h_group[b] in 0 .. G-1 names problem b's group, G = the largest
 * id + 1, and every id occurs.  Any begun batch may be tied (uniform, described or online; either batch model).  The context keeps the
 * tie on the device in arrays of its own -- the members sorted by (group, problem), the groups' first positions [G + 1], the map [B] --;
 * no workspace region is added.  A re-table keeps the tie, any begin forgets it, a second call replaces it.  CPPROB_HIP_ESTATE: no
 * batch is begun; CPPROB_HIP_EINVAL with nothing changed: n is not the batch's number of problems, an id is negative, an id in
 * 0 .. G-1 is unused.  Synchronises. */
int cpprob_hip_batch_tie(cpprob_hip_ctx* ctx, const int32_t* h_group, size_t n);
/* The tie in force: h_group [B] (may be NULL) and the number of groups.  CPPROB_HIP_ESTATE without a tie.  Host only. */
int cpprob_hip_batch_tie_get(cpprob_hip_ctx* ctx, int32_t* h_group, int32_t* n_groups);
/* The groups' pooled records.  d_records [B][R][88], R = per_problem >= 1 (R = 1: the records of cpprob_hip_batch_smooth_stats and
 * _online_stats; R = n_traj: those of _traj_stats).  For a group g with the members b_0 < b_1 < ..., every r < R and entry e < 88:
 *   pooled[g][r][e] = (((0.0 + rec[b_0][r][e]) + rec[b_1][r][e]) + ...)
 * one addition a member, in ascending problem order, from 0.0, nothing contracted; all 88 entries whatever the batch's k.
 * broadcast = 0: d_out is [G][R][88]; broadcast = 1: d_out is [B][R][88] and every member of g receives pooled[g] -- the record
 * cpprob_hip_batch_mstep_device then turns into one table a group, held by every member alike.  d_out == d_records is allowed with
 * broadcast = 1 (a resident fit pools in place); any other overlap is CPPROB_HIP_EINVAL.  CPPROB_HIP_EINVAL with nothing written:
 * n_doubles < 88 B R, n_out too small, R == 0, G R beyond what one launch's grid holds.  CPPROB_HIP_ESTATE: no begun batch, or no
 * tie.  It needs no run: it reads the caller's records and the tie.  The device form is enqueued on the context's stream without a
 * host synchronisation, under cpprob_hip_batch_smooth_stats_device's stream contract; the host form stages h_records, runs the same
 * kernel and synchronises.  cpprob_amd.em.pool_stats states the sum in numpy. */
int cpprob_hip_batch_pool_stats_device(cpprob_hip_ctx* ctx, const double* d_records, size_t n_doubles, uint32_t per_problem, int broadcast,
                                       double* d_out, size_t n_out);
int cpprob_hip_batch_pool_stats(cpprob_hip_ctx* ctx, const double* h_records, size_t n_doubles, uint32_t per_problem, int broadcast,
                                double* h_out, size_t n_out);

/* ---- tied online EM: the streams of a group learn one table on the device (csrc/batch_learn_tied.hpp) --
 * cpprob_hip_batch_learn_tie tells the learner of a begun, armed (cpprob_hip_batch_learn_begin*) and tied (cpprob_hip_batch_tie) online
 * batch to pool over the tie in force, before its first advance.  A learning advance then runs, stream-ordered and without a look from
 * the host: the rows and the run as before; every problem's discounted push and record (tau and the record of
 * cpprob_hip_batch_learn_record are what an untied learner would hold under the same tables); the pooled records, compact and with R = 1
 * (pooled[g][e] = ((0.0 + rec[b_0][e]) + rec[b_1][e]) + ... over the members b_0 < b_1 < ...; a member of length 0 contributes zeros);
 * and one M-step a group.  Group g fires in an advance iff some member received observes in it AND the members' lengths reached, summed,
 * are >= t_min.  A firing group runs the M-step on pooled[g] from the table of its first member (with the sigmas on a scaled learner
 * that fits them) and checks it (the bits of cpprob_hip_batch_learn_tables): no bit set -- every member receives the new table, the
 * scales where fitted, its 64 threshold words and status 0; a bit set -- every member's status word receives the bits and nothing else
 * changes.  A group that does not fire keeps tables, words and status words.  Every stream's record is a convex running average, so the
 * streams of a group weigh equally whatever their lengths; weighting by length is not built.  With every problem its own group this is
 * the untied learner.
 * CPPROB_HIP_ESTATE, naming the missing call: the batch is not armed, has no tie, or has been advanced.  CPPROB_HIP_EINVAL naming the
 * first problem that differs: the members of a group do not hold one table (and, on a scaled batch, one set of sigmas) bit for bit.
 * While the learner pools, cpprob_hip_batch_tie is CPPROB_HIP_ESTATE and cpprob_hip_batch_online_tables* is CPPROB_HIP_EINVAL for tables
 * that differ within a group; arming again, or any begin, ends it. */
int cpprob_hip_batch_learn_tie(cpprob_hip_ctx* ctx);
/* The groups' pooled records [G][88] of the last tied learning advance (n_doubles >= 88 G; none yet: zeros).  Synchronises. */
int cpprob_hip_batch_learn_pooled_record(cpprob_hip_ctx* ctx, double* h_out, size_t n_doubles);

/* ---- one joint population sharded over several contexts (one per GPU; the caller runs the collective) --
 * cfg.resample_scope = GLOBAL with n_global > n_particles.  Per step t = 0..T-1 (SIS: t = T-1 only):
 *   step_begin(t) propagates and weighs the local shard and writes this shard's
 *                 {max logw, sum exp(logw-max), sum exp(2(logw-max))} to d_local_totals (3 doubles, device);
 *   the caller all-gathers those over ranks (RCCL) into d_all_totals[3*world];
 *   step_end(t)   combines them ON DEVICE into the joint normaliser, ESS, evidence and resampling decision.
 * Resampling itself is local to the shard -- particles never migrate; right after a resampling step the
 * shard's particles carry log(shard mean weight / population mean weight), i.e. the shard's share of the
 * mass (distributed resampling with non-proportional allocation).  With world = 1 the protocol is
 * bit-identical to cpprob_hip_infer_run.  finish() runs the posterior read-out; cpprob_hip_infer_stats then
 * returns UN-NORMALISED weighted sums relative to exp(max_logw) -- real: {sum w x, sum w x^2}, int:
 * {sum w [x = s]} -- which the caller all-reduces and divides by W = exp(log_norm - max_logw)
 * (cpprob_amd/distributed.py; DESIGN.md section "Multi-GPU").  Everything is stream-ordered: no host sync. */
int cpprob_hip_smc_step_begin(cpprob_hip_ctx* ctx, int32_t t, uint64_t run_index, double* d_local_totals);
int cpprob_hip_smc_step_end(cpprob_hip_ctx* ctx, int32_t t, const double* d_all_totals, int32_t world, int32_t rank);
int cpprob_hip_smc_finish(cpprob_hip_ctx* ctx);
/* Fixed-point form (integer masses against a reference known before the generation exists): a generation whose heaviest particle
 * sat more than 6 nats below its reference lost too many of its 32 bits.  A single context repairs it inside cpprob_hip_infer_run
 * (cpprob_hip_summary::n_requantised); the shards of a joint population do the same through the step protocol, in integers, so
 * that the sharded run stays equal to the one-GPU run bit for bit (cpprob_hip_group_* drives this itself):
 *   first_bad_generation  after cpprob_hip_smc_finish: the first offending generation g, -1 when every generation kept its bits
 *                         (every rank reads the same g: the books come from the all-gathered totals); synchronises the stream;
 *   repair_begin(g)       generation g's log-weights recomputed from the particle store; d_local3 = {key of this shard's exact
 *                         maximum, 0, 0} (three 64-bit words, device): the caller all-gathers them as it does a step's totals;
 *   repair_end(g)         d_all3 = the all-gathered words; masses of generation g against the POPULATION's exact maximum, the
 *                         books rewound to where they stood before g; d_local3 = this shard's totals of the requantised
 *                         generation.  The caller all-gathers them and goes on as if step g had just run: cpprob_hip_smc_step_end(g),
 *                         the exchange behind step g, step_begin(g + 1) ... cpprob_hip_smc_finish; repeated while a later
 *                         generation trips (each round starts later).
 * There is no reference interface here: the reference has no SMC. */
int cpprob_hip_smc_first_bad_generation(cpprob_hip_ctx* ctx, int32_t* h_generation, double* h_gap);
int cpprob_hip_smc_repair_begin(cpprob_hip_ctx* ctx, int32_t g, double* d_local3);
int cpprob_hip_smc_repair_end(cpprob_hip_ctx* ctx, int32_t g, const double* d_all3, int32_t world, int32_t rank, double* d_local3);
/* Filtering-only shards (keep_history = 0) after finish: *joint_already = 1 -- cpprob_hip_infer_stats holds the JOINT population's
 * numbers (prefix-count form: they come from the all-gathered totals), nothing to combine; 0 -- it holds this shard's raw sums of
 * weight x f(x_t) per predict hit t and *d_masses (device, n_predict doubles) this shard's mass of generation t: the caller adds both
 * over ranks and divides (real predicts: mean = sum / mass, variance = second sum / mass - mean^2). */
int cpprob_hip_filter_masses(cpprob_hip_ctx* ctx, double** d_masses, int32_t* joint_already);

/* Exchange scope (cfg.resample_scope = CPPROB_HIP_SCOPE_EXCHANGE, systematic resampling): the sharded run draws the
 * SAME ancestors a single GPU holding all n_global particles would (one shared offset u makes every
 * rank's offspring range [o_r, o_{r+1}) a function of the all-gathered rank totals).  Output j lives on the rank whose
 * shard contains j; outputs whose ancestor sits on another rank arrive as lineage records -- the ancestor's trace
 * x_0 .. x_t, (t + 1) values of the model's value type -- and become extra columns of the receiving shard's
 * particle store, so every later kernel treats them as ordinary particles.  Between step_end(t) and
 * step_begin(t + 1), for every t < T - 1:
 *   plan(t)    host-synchronising; h_shard_begin[world + 1] = first global particle id of each rank's shard.
 *              Returns the resampling decision and, per peer, how many records this rank sends / receives
 *              (both zero when the step does not resample or when the shards' masses happen to match);
 *   pack(t)    writes sum(h_send_counts) records into d_send (device, caller-owned), grouped by destination rank
 *              in rank order;
 *   the caller moves them (RCCL all-to-all-v with the counts as split sizes, times (t + 1) elements);
 *   commit(t)  takes sum(h_recv_counts) records from d_recv, grouped by source rank in rank order.
 * pack/commit may be skipped data-wise (NULL pointers) when the respective count is zero, but must be called. */
int cpprob_hip_exchange_plan(cpprob_hip_ctx* ctx, int32_t t, int32_t world, int32_t rank, const uint64_t* h_shard_begin,
                             uint64_t* h_send_counts, uint64_t* h_recv_counts, int32_t* h_do_resample);
int cpprob_hip_exchange_pack(cpprob_hip_ctx* ctx, int32_t t, void* d_send);
int cpprob_hip_exchange_commit(cpprob_hip_ctx* ctx, int32_t t, const void* d_recv);

/* The same exchange WITHOUT any host synchronisation inside a run (what the multi-GPU drivers use: RCCL send / receive counts are
 * host constants, so the transport moves fixed-capacity segments and the plan lives on the device).
 *   setup      once after cpprob_hip_infer_begin: the shards' layout, the peer set -- all_peers = 0: the two neighbouring ranks (the
 *              offspring interval of a rank's sources leaves its shard by O(sqrt(n)) outputs: neighbours are all a well-mixed run
 *              needs), all_peers = 1: every rank (2, world = 1 only: the rank itself, a diagnostic that lets one GPU run the
 *              transport) -- and records_per_peer, the capacity of one peer segment;
 *   transport  the context-owned buffers: peer slot s (peer rank h_peers[s]) owns records_per_peer * (t + 1) values of
 *              bytes_per_value bytes at byte offset s * records_per_peer * (t + 1) * bytes_per_value of d_send / d_recv
 *              during the exchange that follows step t;
 *   between step_end(t) and step_begin(t + 1), t < T - 1:
 *     pack_async(t)    plans on the device and fills d_send;
 *     the caller moves slot s of d_send to rank h_peers[s], into the slot that rank keeps for this one, stream-ordered;
 *     commit_async(t)  turns what arrived in d_recv into annex columns;
 *   status     after the run (synchronises): overflow = 0 fine; otherwise a set of bits: 1 a peer segment was too small, 2 a rank
 *              outside the peer set was needed, 4 the immigrant annex was too small.  A non-zero value invalidates the run on
 *              EVERY rank of the group (ranks must agree on it -- all-reduce the bits): repeat it with what overflowed enlarged
 *              (records_per_peer / all_peers = 1 / cpprob_hip_config::annex_kcols).  Results do not depend on the transport parameters. */
int cpprob_hip_exchange_setup(cpprob_hip_ctx* ctx, int32_t world, int32_t rank, const uint64_t* h_shard_begin, int32_t all_peers, uint64_t records_per_peer);
int cpprob_hip_exchange_transport(cpprob_hip_ctx* ctx, void** d_send, void** d_recv, int32_t* n_peers, int32_t* h_peers, uint64_t* records_per_peer,
                                  uint64_t* bytes_per_value);
/*   direct     (optional, after setup) h_peer_recv[world]: for every peer rank r, rank r's d_recv (cpprob_hip_exchange_transport) as
 *              THIS context's device addresses it -- the same pointer when both contexts share a device, a peer-access pointer
 *              inside one process, a hipIpcOpenMemHandle mapping across processes; NULL elsewhere.  pack_async then stores every
 *              record straight into the receiver's slot for this rank and d_send is not used: the caller moves nothing, it only
 *              orders the receiver's commit_async(t) behind the senders' pack_async(t) (any collective every rank enters after its
 *              pack_async will do).  NULL switches back.  setup() resets it (the buffers may move).
 *   traffic    after the run (synchronises): lineage records this rank sent after each step (h_sent_per_step[n_predict], may be NULL),
 *              their total and their bytes -- records x (t + 1) x bytes_per_value: what the direct transport puts on the links. */
/*   remote     (optional, after direct) REMOTE LINEAGES: with every rank's particle store addressable from this device, a migrating
 *              particle takes only its current state and the slot it leaves along -- value + 8 bytes per record (+ 4 where the particles carry
 *              trace words: short discrete traces) -- and pack_async
 *              stores both straight into the RECEIVING rank's annex column and origin table: every rank keeps every rank's annex
 *              fill (a function of the all-gathered totals), so there is no receive buffer, no segment capacity, no peer set and
 *              commit_async launches nothing (what remains of the overflow bits is 4: an annex too small).  The particle's history
 *              stays where it is, and whoever walks the lineage later -- the read-out, cpprob_hip_copy_paths -- continues in that
 *              rank's store.  store() fills this context's own entry (and sizes its origin table); remote() takes h_stores[world],
 *              entry r = rank r's store as THIS device addresses it (peer access / hipIpcOpenMemHandle of the three arrays: they
 *              are written AND read through the mapping).  Every rank of the group must be in the same mode, and the caller still
 *              orders step_begin(t + 1) of every rank behind pack_async(t) of every rank.  No lineage is extracted, shipped or
 *              committed any more: the exchange of a step costs what its migrants' states cost. */
typedef struct cpprob_hip_store {
    const void* d_values; const void* d_ancestors; const void* d_origin;     /* [T][row_stride] values, [T][row_stride] int32, [annex] int64 */
    uint64_t row_stride, n_local_columns;
    const void* d_trace[2];    /* short discrete traces (hmm<T <= 16>): the particles' trace words, [row_stride] uint32 each, by the step's
                                  parity -- a migrant's word is stored into the receiving rank's with its state; NULL where not in use */
} cpprob_hip_store;
int cpprob_hip_exchange_store(cpprob_hip_ctx* ctx, cpprob_hip_store* out);
int cpprob_hip_exchange_remote(cpprob_hip_ctx* ctx, const cpprob_hip_store* h_stores);
int cpprob_hip_exchange_direct(cpprob_hip_ctx* ctx, void* const* h_peer_recv);
int cpprob_hip_exchange_traffic(cpprob_hip_ctx* ctx, int64_t* h_sent_per_step, size_t n_steps, uint64_t* h_records, uint64_t* h_bytes);
int cpprob_hip_exchange_pack_async(cpprob_hip_ctx* ctx, int32_t t);
int cpprob_hip_exchange_commit_async(cpprob_hip_ctx* ctx, int32_t t);
int cpprob_hip_exchange_status(cpprob_hip_ctx* ctx, int32_t* h_overflow, uint64_t* h_annex_used);

/* ---- one joint population over several GPUs, driven from the host side of this library ------------------------------------
 * A group = one context per GPU + collectives + a transport; cpprob_hip_group_run enqueues a WHOLE exchange-scope run on every local
 * rank -- per step: propagate / weigh, all-gather of 3 doubles per rank, device-side plan, the migrating lineages, commit -- with no
 * host synchronisation inside (cpprob_amd/csrc/group.hpp).  Replaces what a caller of the reference would have to build around
 * cpprob::inference to use more than one device (the reference is single-process, src/cpprob/state.cpp:20-21).
 *   create   world == n_local: every rank in this process.  Distinct devices: RCCL over xGMI, one communicator and one host
 *            thread per GPU.  All devices equal: "loopback" -- every rank's context on that one device and one stream, program
 *            order instead of collectives (how a one-GPU machine exercises the protocol; RCCL refuses duplicate devices).
 *            world > n_local: one rank (n_local = 1) of a group spread over processes; unique_id = the 128 bytes rank 0 got from
 *            cpprob_hip_group_unique_id and handed to every rank (the launcher's job: torchrun, MPI, a file).
 *   create_external   one rank of a group whose collectives are the CALLER's (MPI, gloo, ...): allgather(user, h_in, h_out,
 *            bytes_per_rank) gathers host bytes of every rank in rank order and returns 0; it is called from cpprob_hip_group_begin /
 *            _run / _results, which synchronise the stream around it.  The lineages move by direct stores (below); nothing else is
 *            asked of the caller.
 *   transport (before begin) records_per_peer = capacity of one peer segment (0: the default, 8 sqrt(N) + 4096); all_peers = 1: every
 *            rank is a peer, 0: the two neighbouring ranks, < 0: the default (neighbours); flags = CPPROB_HIP_GROUP_*.  Results never
 *            depend on any of them; a run they prove too small for is repeated with larger ones (results).
 *            How the lineages move: DIRECT -- the sending rank's packing kernel stores every record into the receiving rank's buffer
 *            (peer access inside a process, hipIpc mappings between processes), ordered by a one-double all-gather per step, so that
 *            what crosses xGMI is records x (t + 1) x value size and nothing on a step that does not resample -- wherever every rank
 *            can map its peers' buffers; otherwise SENDRECV -- ncclSend / ncclRecv of the fixed-capacity segments.
 *            The per-step collectives (24 bytes of totals per rank; the ordering of the direct stores): MAILBOXES wherever the ranks
 *            can map each other's memory -- a rank stores its words and the step's sequence number into every peer's mailbox and spins
 *            on its own, one short launch, no library call and no host inside a run (csrc/device_collectives.hpp); proven by a round
 *            trip at the first begin, and a wait that times out (5 s) makes results() repeat the run on the library's collectives.
 *            Otherwise RCCL calls / the caller's all-gather.  The collectives flags are read at the first begin (LIBRARY_COLLECTIVES at
 *            any later begin still switches the mailboxes off).
 *   begin    cfg as for cpprob_hip_infer_begin with n_particles = the WHOLE population (particle_offset / n_global / scope are
 *            set per rank by the group); shards are contiguous and equal unless h_shard_sizes[world] names them.  Systematic SMC
 *            runs in the exchange scope (exact global resampling); other resamplers and SIS in the global scope.  COLLECTIVE.
 *   run      asynchronous (RCCL / loopback).
 *   results  COLLECTIVE: every rank of the group calls it.  Synchronises, all-reduces and normalises: h_stats as
 *            cpprob_hip_infer_stats of ONE GPU holding the whole population would return.  If a transport segment or the annex
 *            overflowed -- every rank sees the same all-reduced flags -- it first repeats the LAST run with a larger transport
 *            (h_reruns counts those since begin): the numbers never depend on the transport.  Runs enqueued before the last one are
 *            not repeated: a caller that pipelines runs should settle the transport with one run + results first.
 *   traffic  of the run results last collected.
 *   context  the rank's context, e.g. for cpprob_hip_copy_paths of its shard. */
typedef struct cpprob_hip_group cpprob_hip_group;
typedef struct cpprob_hip_collectives {
    void* user;
    int (*allgather)(void* user, const void* h_in, void* h_out, size_t bytes_per_rank);
} cpprob_hip_collectives;
#define CPPROB_HIP_GROUP_SENDRECV 1u            /* never map peers' buffers: ncclSend / ncclRecv of fixed-capacity segments */
#define CPPROB_HIP_GROUP_WORLD1_COLLECTIVES 2u  /* diagnostic, world = 1: issue every collective of the multi-GPU path anyway and exchange
                                                   (zero records) with the rank itself, so that one GPU runs all of the transport's calls */
#define CPPROB_HIP_GROUP_SHIP_LINEAGES 4u      /* direct transport: migrants still take their whole lineage along (records of t + 1 values)
                                                   instead of leaving it on the rank they come from (remote lineages, the default where
                                                   every rank can address every rank's particle store) */
#define CPPROB_HIP_GROUP_LIBRARY_COLLECTIVES 8u /* the per-step collectives through RCCL / the caller's all-gather even where the ranks can map
                                                   each other's memory (default there: stores into the peers' mailboxes, no call inside a run) */
#define CPPROB_HIP_GROUP_MAILBOX_COLLECTIVES 16u /* loopback groups too (they gather for every rank in one launch by default) */
#define CPPROB_HIP_TRANSPORT_NONE 0
#define CPPROB_HIP_TRANSPORT_DIRECT 1
#define CPPROB_HIP_TRANSPORT_SENDRECV 2
typedef struct cpprob_hip_traffic {
    uint64_t records;          /* lineage records that changed rank, all ranks, all steps of the run                           */
    uint64_t payload_bytes;    /* sum over steps of records x (t + 1) x value size                                             */
    uint64_t wire_bytes;       /* what the transport put on the links for them: = payload_bytes (direct), capacity (send/recv)  */
    uint64_t collective_bytes; /* the small collectives: all-gathers of 3 doubles (+ 1 ordering the direct stores) per step, the final all-reduce */
    int32_t transport;         /* CPPROB_HIP_TRANSPORT_*                                                                       */
    int32_t remote_lineages;   /* 1: migrants left their history on the rank they came from (records of value + 8 bytes)           */
    int32_t mailbox_collectives; /* 1: the per-step collectives were stores into the peers' mailboxes, not library calls            */
    int32_t reserved;
} cpprob_hip_traffic;
int cpprob_hip_group_unique_id(void* out128, size_t n_bytes);
int cpprob_hip_group_create(const int32_t* devices, int32_t n_local, int32_t world, int32_t first_rank, const void* unique_id, cpprob_hip_group** out);
int cpprob_hip_group_create_external(int32_t device, int32_t world, int32_t rank, const cpprob_hip_collectives* collectives, cpprob_hip_group** out);
void cpprob_hip_group_destroy(cpprob_hip_group* group);
const char* cpprob_hip_group_last_error(const cpprob_hip_group* group);
int cpprob_hip_group_transport(cpprob_hip_group* group, uint64_t records_per_peer, int32_t all_peers, uint32_t flags);
int cpprob_hip_group_begin(cpprob_hip_group* group, const cpprob_hip_config* cfg, const double* h_observes, size_t n_observes, const uint64_t* h_shard_sizes);
int cpprob_hip_group_run(cpprob_hip_group* group, uint64_t run_index);
int cpprob_hip_group_sync(cpprob_hip_group* group);
int cpprob_hip_group_size(const cpprob_hip_group* group, int32_t* world, int32_t* n_local, int32_t* first_rank);
cpprob_hip_ctx* cpprob_hip_group_context(cpprob_hip_group* group, int32_t local_index);
int cpprob_hip_group_results(cpprob_hip_group* group, cpprob_hip_summary* out, double* h_stats, size_t n_doubles, int32_t* h_reruns);
int cpprob_hip_group_traffic(cpprob_hip_group* group, cpprob_hip_traffic* out);
/* Where a rank-step's time goes (what the first run over real links has to explain).  profile(on): HIP events between the launches of
 * every step of the following runs, on every local rank's stream.  profile_read: of the last run, microseconds per rank-step (mean over
 * the steps that run every phase, the slowest local rank; a loopback group: the SUM over its ranks, which share one stream):
 * [0] step kernel + shard totals (+ the mailbox all-gather where the totals launch carries it), [1] a separate all-gather (mailbox
 * launch or library call), [2] the hand-over of the gathered totals, [3] the packing launch, [4] the barrier that orders the commits
 * behind every rank's stores, [5] the commit, [6] of all that, the time mailbox waits spun (device wall clock), [7] steps timed. */
int cpprob_hip_group_profile(cpprob_hip_group* group, int32_t on);
int cpprob_hip_group_profile_read(cpprob_hip_group* group, double* h_out8);
/* Which collectives and which migrant transport the group settled on, and why (fall-back rungs included), as one line of text; valid
 * until the calling thread's next call. */
const char* cpprob_hip_group_note(const cpprob_hip_group* group);

/* ---- building blocks (also the unit-parity surface) --------------------------------------
 * All pointers are device pointers; n is the element count. */

/* Raw Philox4x32-10 blocks: d_out[4*i..4*i+3] = block(seed, group0 + i, draw)
 * (= rocrand_init(seed, subsequence = group, offset = 4*draw); rocrand4()). */
int cpprob_hip_philox_blocks(cpprob_hip_ctx* ctx, uint64_t seed, uint64_t group0, uint64_t draw, size_t n, uint32_t* d_out);
/* Variate generators standing in for boost::random::*::operator()(get_rng()) (cpprob.hpp:34):
 * element i is the draw of global particle pid0+i at statement ordinal `draw`.  Neighbouring
 * particles share Philox blocks: 32-bit variates (uniform_smallint, discrete) take word pid&3 of
 * block(group pid>>2); normal variates take component pid&1 of rocRAND's box_muller_double of
 * block(group pid>>1); 53-bit uniforms (uniform_real) take word pair pid&1 of block(pid>>1). */
int cpprob_hip_draw_normal(cpprob_hip_ctx* ctx, uint64_t seed, uint64_t pid0, uint64_t draw, double mean, double sigma, size_t n, double* d_out);
int cpprob_hip_draw_uniform_smallint(cpprob_hip_ctx* ctx, uint64_t seed, uint64_t pid0, uint64_t draw, int64_t a, int64_t b, size_t n, int32_t* d_out);
int cpprob_hip_draw_discrete(cpprob_hip_ctx* ctx, uint64_t seed, uint64_t pid0, uint64_t draw, const double* h_weights, int32_t k, size_t n, int32_t* d_out);
int cpprob_hip_draw_uniform_real(cpprob_hip_ctx* ctx, uint64_t seed, uint64_t pid0, uint64_t draw, double a, double b, size_t n, double* d_out);
/* The laws are pinned to the exact quantile functions at the particle's exact uniform (tests/test_gpu_variates.py): uniform_smallint
 * (a and b must fit int32) and discrete (weights finite and >= 0, total positive and finite; CPPROB_HIP_EINVAL otherwise) are the exact
 * quantile; uniform_real is one of the two doubles next to a + (b - a) u and always in [a, b); normal is within 3 2^-52 relative of
 * sqrt(-2 ln u) sin / cos(pi w).
 * poisson: inversion of the particle's 53-bit uniform u, summed outwards from the mode in O(sqrt(mean)) terms.  For 0 <= mean <=
 * CPPROB_HIP_POISSON_MAX_MEAN the result is the exact quantile at some u' within (2 W + 8 sqrt(mean) + 16) 2^-53 of u, W the number of
 * terms summed (about 18 sqrt(mean); 1762 at 10^4): below 2^-40; it never exceeds the exact quantile of 1 - 2^-54.  A mean above the
 * limit, negative or NaN is refused with CPPROB_HIP_EINVAL (the device function clamps it and terminates; its law there is unspecified). */
#define CPPROB_HIP_POISSON_MAX_MEAN 1.0e4
int cpprob_hip_draw_poisson(cpprob_hip_ctx* ctx, uint64_t seed, uint64_t pid0, uint64_t draw, double mean, size_t n, int32_t* d_out);

/* logpdf functors (include/cpprob/distributions/utils_*.hpp), elementwise. */
int cpprob_hip_logpdf_normal(cpprob_hip_ctx* ctx, const double* d_x, const double* d_mean, const double* d_sigma, size_t n, double* d_out);
int cpprob_hip_logpdf_uniform_real(cpprob_hip_ctx* ctx, const double* d_x, const double* d_a, const double* d_b, size_t n, double* d_out);
int cpprob_hip_logpdf_poisson(cpprob_hip_ctx* ctx, const int32_t* d_x, const double* d_mean, size_t n, double* d_out);
int cpprob_hip_logpdf_uniform_smallint(cpprob_hip_ctx* ctx, const int32_t* d_x, int64_t a, int64_t b, size_t n, double* d_out);
int cpprob_hip_logpdf_discrete(cpprob_hip_ctx* ctx, const int32_t* d_x, const double* h_weights, int32_t k, size_t n, double* d_out);

/* The range-specific fp64 elementary functions the variate generators and the weight kernels use in place of the device library's
 * (cpprob_amd/include/cpprob/detail/fastmath.hpp; they stand where the reference calls std::log / std::exp through Boost.Random and
 * include/cpprob/distributions/utils_normal_distribution.hpp:38-41), elementwise: which = 0 log01 on [2^-53, 1], 1 sincospi02 on
 * (0, 2] (d_out0 = sin(pi x), d_out1 = cos(pi x)), 2 exp_nonpos on [-745, 0]; 3: the fixed-point weight min(rint(exp(x) 2^32), 2^32 - 1)
 * of a log-weight x <= 0 against the reference 0 (fixed_mass.hpp: fix_weight), as a double.  Unit-parity surface: tests sweep the domain edges. */
int cpprob_hip_fastmath(cpprob_hip_ctx* ctx, int32_t which, const double* d_x, size_t n, double* d_out0, double* d_out1);

/* The variate generators above on chosen bits: element i applies the library's own generator function to the Philox block
 * d_blocks[4*i .. 4*i+3] instead of the block of (seed, particle, ordinal), so that tests reach inputs no seed does (the top uniform has
 * probability 2^-53).  h_params (host, n_params doubles): SMALLINT {a, b} (integers, b - a < 2^32) on word 0; DISCRETE 1 .. 8 weights on
 * word 0; UNIFORM_REAL {a, b} and POISSON {mean} on the 53 bits of words 0 and 1 (lo | (hi >> 11) << 32); NORMAL none, all four words,
 * d_out0 = s sin(pi w), d_out1 = s cos(pi w) (d_out1 is used by NORMAL alone).  Integer results are written as doubles.  Weights and
 * means are refused as by the draw entries.  Unit-parity surface: the draw entries and the models do not go through it. */
#define CPPROB_HIP_VARIATE_SMALLINT 0
#define CPPROB_HIP_VARIATE_DISCRETE 1
#define CPPROB_HIP_VARIATE_UNIFORM_REAL 2
#define CPPROB_HIP_VARIATE_POISSON 3
#define CPPROB_HIP_VARIATE_NORMAL 4
int cpprob_hip_variate_from_bits(cpprob_hip_ctx* ctx, int32_t which, const double* h_params, int32_t n_params, const uint32_t* d_blocks, size_t n,
                                 double* d_out0, double* d_out1);

/* EmpiricalDistribution (include/cpprob/postprocess/empirical_distribution.hpp):
 * h_out[0] = max, [1] = logsumexp (:125-143), [2] = ESS = (sum W^2)^-1. */
int cpprob_hip_logsumexp_ess(cpprob_hip_ctx* ctx, const double* d_logw, size_t n, double* h_out3);
/* h_out[0] = mean (:68-71), [1] = variance (:78-81), [2] = logsumexp, [3] = ESS. */
int cpprob_hip_weighted_moments(cpprob_hip_ctx* ctx, const double* d_x, const double* d_logw, size_t n, double* h_out4);
/* h_out[s] = sum_i W_i [x_i == s], s < k <= 8  (distribution(), :30-40). */
int cpprob_hip_weighted_hist(cpprob_hip_ctx* ctx, const int32_t* d_x, const double* d_logw, size_t n, int32_t k, double* h_out);
/* ... and of n_cols columns (column j at d_x + j * col_stride, col_stride >= n) against ONE log-weight array: one normalisation, one
 * read-out launch, one synchronisation for all of them.  h_out4: [n_cols][4] as cpprob_hip_weighted_moments; h_out: [n_cols][k].
 * Columns whose stride is a whole number of 1024-particle tiles (col_stride % 1024 == 0, col_stride >= n rounded up to a tile) are read
 * WHERE THEY LIE: their slots [n, col_stride) must be readable and hold finite numbers (they weigh nothing); any other stride is
 * copied into tile-padded scratch first.  A read-back hung on the context (cpprob_hip_readback_with_next_result) rides these calls too. */
int cpprob_hip_weighted_moments_columns(cpprob_hip_ctx* ctx, const double* d_x, size_t n_cols, size_t col_stride, const double* d_logw, size_t n, double* h_out4);
int cpprob_hip_weighted_hist_columns(cpprob_hip_ctx* ctx, const int32_t* d_x, size_t n_cols, size_t col_stride, const double* d_logw, size_t n, int32_t k, double* h_out,
                                     double* h_lse_ess /* may be NULL: {logsumexp of the weights, ESS} */);

/* Resampling: d_anc[jj] = ancestor (index into d_logw[0..n_in)) of output j0 + jj, for n_out
 * consecutive outputs of a population of n_total_out positions.  Uniforms come from
 * draw index (1<<40) + step: systematic one 53-bit uniform of group 0; stratified the 32-bit
 * uniform of id j; multinomial the 53-bit uniform of id j. */
int cpprob_hip_resample(cpprob_hip_ctx* ctx, int32_t kind, const double* d_logw, size_t n_in, uint64_t seed, uint64_t step,
                        uint64_t j0, size_t n_out, uint64_t n_total_out, int32_t* d_anc);
/* One step of SMC bookkeeping ON THE DEVICE, stream-ordered, no host synchronisation (what the generic model path runs
 * between two launches of the model body): normalises d_logw[0..n), stores the ESS in d_ess[step], decides
 * (ESS < ess_frac * n, never at the last step) into d_resampled[step], keeps the running log evidence in *d_log_z
 * (reset at step 0; + log mean weight whenever the step resamples or is the last), and fills d_anc[0..n) with the next
 * generation's ancestors -- the identity when the step does not resample.  Uniforms: draw index (1<<40) + step + 1,
 * as cpprob_hip_resample(seed, step + 1). */
int cpprob_hip_smc_bookkeep(cpprob_hip_ctx* ctx, int32_t kind, const double* d_logw, size_t n, uint64_t seed, int32_t step, int32_t last,
                            double ess_frac, double* d_ess, int32_t* d_resampled, double* d_log_z, int32_t* d_anc);
/* The same bookkeeping for SYSTEMATIC resampling on fixed-point weights (cpprob_amd/csrc/step_fixed.hpp, bookkeep_fixed.hpp): the
 * weights become integers q_i = min(rint(exp(logw_i - max logw) 2^32), 2^32 - 1), sums and the resampling comb run on exact 64-bit
 * masses -- three short launches, no floating-point CDF; uniforms as above.  d_anc may be NULL when last != 0.  n <= 2^28. */
int cpprob_hip_smc_bookkeep_fixed(cpprob_hip_ctx* ctx, const double* d_logw, size_t n, uint64_t seed, int32_t step, int32_t last, double ess_frac,
                                  double* d_ess, int32_t* d_resampled, double* d_log_z, int32_t* d_anc);
/* ... and for any resampler: kind = CPPROB_HIP_RESAMPLE_* -- stratified (output j at j + u_j against the same masses) and multinomial
 * (strata form: the counts of this resampling's thresholds per stratum in one or two short launches in front of the ancestors' launch),
 * the arithmetic of the built-in models' step kernels.  cpprob_hip_smc_bookkeep_fixed = kind SYSTEMATIC. */
int cpprob_hip_smc_bookkeep_fixed_rs(cpprob_hip_ctx* ctx, int32_t kind, const double* d_logw, size_t n, uint64_t seed, int32_t step, int32_t last, double ess_frac,
                                     double* d_ess, int32_t* d_resampled, double* d_log_z, int32_t* d_anc);
/* ---- SMC step of an UNCHANGED model with the resampling inside the model's own launch (cpprob_amd/include/cpprob/gpu.hpp:
 * model_step_kernel; replaces the loop body of reference include/cpprob/cpprob.hpp:194-201 for StateType::smc) ----------------------
 * The model translation unit owns the kernel (it is a template over the model function); the library owns what the kernel's
 * prologue and epilogue work on: three rotating copies of the 64-ary mass hierarchy (cpprob_amd/include/cpprob/detail/fixed_mass.hpp),
 * the integer weights of two generations and a small control block.  cpprob_hip_generic_begin sizes them for a population of n
 * particles (one hierarchy entry per 256-particle block = per workgroup of the step kernel; first call and growth allocate), clears
 * them on the context's stream and describes them in *out; step t of the run reads copy (t + 2) % 3 of the hierarchy, publishes
 * into copy t % 3 and clears the upper levels of copy (t + 1) % 3; integer weights: generation t in q[t & 1].  n <= 64^3 * 256. */
typedef struct cpprob_hip_generic_layout {
    uint64_t* hier;            /* [3][per_copy] 64-bit words */
    uint64_t per_copy;
    uint64_t lvl_off[3];       /* word offset of each level inside a copy */
    int32_t n_ent[3];          /* entries per level (n_ent[0] = blocks) */
    int32_t n_lev;
    uint64_t q0_off, m0_off;   /* the blocks' squares / maxima inside a copy */
    void* table;               /* the same layout in device memory (fixed_mass.hpp: HierTable) */
    uint32_t* q[2];            /* integer weights, by the step's parity: padded to whole 1024-particle tiles, and one tile more */
    void* ctrl;                /* device_trace.hpp: StepCtrl2 */
    int32_t blocks;
    int32_t block;             /* particles per hierarchy entry: 256 (cpprob_hip_generic_begin) or 1024 (cpprob_hip_generic_begin_tiles) */
} cpprob_hip_generic_layout;
int cpprob_hip_generic_begin(cpprob_hip_ctx* ctx, size_t n, cpprob_hip_generic_layout* out);
/* The same with one hierarchy entry per 1024-particle TILE: the layout of model_step_kernel_quad, whose workgroups run the model body
 * for four particles a lane behind ONE ancestor search (cpprob/gpu.hpp).  n <= 64^3 * 1024 (and 2^28).  The exact-reference passes
 * below work on 256-particle blocks only. */
int cpprob_hip_generic_begin_tiles(cpprob_hip_ctx* ctx, size_t n, cpprob_hip_generic_layout* out);
/* Exact-reference form (no host-known bound of a step's log-likelihood): the step's launch stored the log-weights only; two short
 * launches find the generation's exact maximum, quantise d_logw[0..n) against it into q[t & 1] and publish maxima and masses into
 * copy t % 3. */
int cpprob_hip_generic_quantize(cpprob_hip_ctx* ctx, int32_t t, const double* d_logw, size_t n);
/* The same in two halves, for one shard of a JOINT population whose host threads combine the ranks' numbers between the launches:
 * the maximum pass alone (into copy t % 3), and the masses against a reference the caller supplies (the population's exact maximum). */
int cpprob_hip_generic_max(cpprob_hip_ctx* ctx, int32_t t, const double* d_logw, size_t n);
int cpprob_hip_generic_quantize_ref(cpprob_hip_ctx* ctx, int32_t t, const double* d_logw, size_t n, double ref);
/* {mass, squares, order key of the maximum} of generation t as copy t % 3 holds them: 24 bytes into d_out3 (device memory; stream-ordered):
 * what a shard of a joint population contributes to the generation's totals. */
int cpprob_hip_generic_totals(cpprob_hip_ctx* ctx, int32_t t, size_t n, uint64_t* d_out3);
/* Bookkeeping of the run's LAST generation (T - 1: the copy (T - 1) % 3): d_ess[T-1], d_resampled[T-1] = 0, the final term of
 * *d_log_z; *d_flags gets 4 / 5 where the generation's heaviest particle sat above / more than gap_limit below its reference. */
int cpprob_hip_generic_finish(cpprob_hip_ctx* ctx, int32_t T, size_t n, double gap_limit, double* d_ess, int32_t* d_resampled, double* d_log_z, int32_t* d_flags);
/* The systematic offset in [0, 1) of the resampling that precedes step `step`: Philox draw (1 << 40) + step of group 0 --
 * a pure function of (seed, step), evaluated on the host so that launches carry it as an argument. */
double cpprob_hip_systematic_offset(uint64_t seed, uint64_t step);
/* Traces from per-step records: d_anc [T][n] (row t: slot of generation t-1 that slot i of generation t extends; a row counts only where
 * d_resampled[t-1] != 0), d_cols [H][n] with row h recorded in the slots of generation h_gen[h] (non-decreasing in h).  d_out[h][i] =
 * d_cols[h][slot of generation h_gen[h] on the ancestral line of FINAL particle i]: the value particle i's trace holds for that row.
 * is_int = 0: fp64 rows, 1: int32 rows.  Stream-ordered; what the unchanged-model SMC path reads its predicts out with. */
int cpprob_hip_lineage_gather(cpprob_hip_ctx* ctx, const int32_t* d_anc, const int32_t* d_resampled, int32_t T, size_t n, const void* d_cols,
                              int32_t is_int, const int32_t* h_gen, int32_t H, void* d_out);
/* The same walk with the rows' statistics taken on the way -- what cpprob_hip_lineage_gather followed by cpprob_hip_weighted_moments_columns /
 * _hist_columns against d_logw (the FINAL generation's log-weights, n of them) returns, bit for bit, without the traces' round trip through
 * memory (StatsPrinter's numbers, reference stats_printer.hpp:68-120, when nobody asked for the traces themselves).  h_out4: [H][4] =
 * {mean, variance, logsumexp, ess}; h_out: [H][k] probabilities, 1 <= k <= 8; h_lse_ess (may be NULL): {logsumexp, ess}.  Synchronises. */
/* Hangs ONE read-back of the caller's on the next cpprob_hip_lineage_moments / cpprob_hip_lineage_hist call of this context: bytes
 * [d_src, d_src + bytes) are stored into pinned host memory by the launch that stores the call's own result, and are in h_dst when
 * the call returns -- the call's own stream synchronisation is the only one (cpprob/gpu.hpp: the run's ESS / evidence / flag tail
 * rides the read-out's result instead of a host round trip of its own).  bytes = 0 cancels.  <= 1 MiB, a multiple of 4. */
int cpprob_hip_readback_with_next_result(cpprob_hip_ctx* ctx, const void* d_src, void* h_dst, size_t bytes);
/* Optional: uploads the records' generation table of the three calls above / below ahead of time (it is uploaded at their first use
 * otherwise, with a synchronisation; an unchanged table is never uploaded twice). */
int cpprob_hip_lineage_prepare(cpprob_hip_ctx* ctx, const int32_t* h_gen, int32_t H, int32_t T);
int cpprob_hip_lineage_moments(cpprob_hip_ctx* ctx, const int32_t* d_anc, const int32_t* d_resampled, int32_t T, size_t n, const double* d_cols,
                               const int32_t* h_gen, int32_t H, const double* d_logw, double* h_out4);
int cpprob_hip_lineage_hist(cpprob_hip_ctx* ctx, const int32_t* d_anc, const int32_t* d_resampled, int32_t T, size_t n, const int32_t* d_cols,
                            const int32_t* h_gen, int32_t H, const double* d_logw, int32_t k, double* h_out, double* h_lse_ess);
/* d_dst[i] = d_src[d_idx[i]] */
int cpprob_hip_gather_f64(cpprob_hip_ctx* ctx, const double* d_src, const int32_t* d_idx, size_t n, double* d_dst);
int cpprob_hip_gather_i32(cpprob_hip_ctx* ctx, const int32_t* d_src, const int32_t* d_idx, size_t n, int32_t* d_dst);

/* Kernel timing of the last cpprob_hip_infer_run, measured with HIP events on the context's
 * stream when enabled (adds two event records per kernel class; off by default).
 * h_ms[k] = accumulated milliseconds, h_calls[k] = launches of kernel class k since the last
 * reset; classes: 0 propagate/step, 1 scan-partials, 2 smoothing read-out, 3 finalize,
 * 4 sis, 5 resample-only.  Synchronises. */
#define CPPROB_HIP_N_KERNEL_CLASSES 6
int cpprob_hip_profile_enable(cpprob_hip_ctx* ctx, int32_t on);
int cpprob_hip_profile_read(cpprob_hip_ctx* ctx, double* h_ms, int64_t* h_calls, int32_t reset);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* CPPROB_HIP_H_ */
