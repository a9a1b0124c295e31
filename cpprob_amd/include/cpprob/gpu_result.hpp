// Host-visible results and options of a device inference run (additions to the reference API; the
// reference returns nothing and leaves everything in files).
#ifndef CPPROB_COMPAT_GPU_RESULT_HPP
#define CPPROB_COMPAT_GPU_RESULT_HPP
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "cpprob_hip.h"

namespace cpprob {
namespace gpu {

struct Options {
    int device = 0;
    std::vector<int> devices;                         // more than one entry: ONE joint population sharded over these GPUs, resampled exactly as
                                                      // one GPU holding every particle would (exchange scope: per step an RCCL all-gather of the
                                                      // rank totals and the redistribution of offspring over xGMI; cpprob_hip_group_*).  All
                                                      // entries equal: every rank on that one GPU (loopback transport; a one-GPU machine's way
                                                      // to run the protocol).  Built-in models; unchanged models (CPPROB_REGISTER_MODEL): under
                                                      // StateType::sis the shards need no communication until their sums are combined (the
                                                      // one-device run, exactly); under StateType::smc every device runs an ISLAND of its own
                                                      // and the islands are combined by their evidence estimates.
    std::uint64_t seed = 12345;
    int resampler = CPPROB_HIP_RESAMPLE_SYSTEMATIC;   // smc
    double ess_threshold = 0.5;                       // smc: resample when ESS < threshold * N (thesis p.37); > 1: every step
    bool dump = true;                                 // write <file>.real/.int/.ids like the reference (state.cpp:193-202)
    std::size_t dump_max_particles = 0;               // 0 = all particles
    std::string batch_dump_file;                      // batched runs (inference_batch, hmm_table_batch): not empty = write problem b's posterior as
                                                      // <batch_dump_file>_<b>.int / .ids, the first dump_max_particles traces (0 = all) resolved on
                                                      // the device in one launch (cpprob_hip_batch_paths); empty: no files
    bool backward_smoothing = false;                  // batched runs (inference_batch, hmm_table_batch, HmmTableStream; keep_history only): the results'
                                                      // statistics are the backward smoother's marginals (cpprob_hip_batch_smooth: every generation's
                                                      // whole filtering approximation) instead of the surviving lineages'
    std::size_t backward_trajectories = 0;            // ... and, not 0, with batch_dump_file: problem b's files hold this many backward-simulated
                                                      // trajectories with equal weights in place of the lineages
    long smoothing_lag = -1;                          // batched runs, keep_history only; >= 0: the results' statistics are the fixed-lag marginals
                                                      // P(x_t | y_0 .. y_min(t + lag, L - 1)) (cpprob_hip_batch_smooth_lag; it takes precedence over
                                                      // backward_smoothing).  HmmTableStream asks for the steps not yet final only: an advance costs its
                                                      // new steps, whatever length the stream has reached.  Negative: off
    std::size_t forecast_horizon = 0;                 // batched runs (keep_history, or keep_masses): not 0 = every result carries Result::forecast, the laws of
                                                      // the state 1 .. forecast_horizon steps past the last observe, P(x_{L-1+h} | y_0 .. y_{L-1})
                                                      // (cpprob_hip_batch_forecast); HmmTableStream: after every advance.  0: off
    std::size_t forecast_trajectories = 0;            // ... and, not 0, Result::forecast_trajectories: this many simulated futures (draw_index 0)
    std::size_t trajectory_stats = 0;                 // batched runs (keep_history, or keep_masses): not 0 = every result carries Result::trajectory_stats, the
                                                      // complete-data sufficient statistics of this many backward-simulated trajectories, counted on the
                                                      // device (cpprob_hip_batch_traj_stats); HmmTableStream: after every advance.  0: off
    std::uint64_t trajectory_stats_draw_index = 0;    // ... under this draw_index (< 2^16): the trajectories are cpprob_hip_batch_smooth's for it
    bool running_stats = false;                       // HmmTableStream (keep_history, or keep_masses): every advance's results carry Result::running_stats, the
                                                      // expected sufficient statistics of the lengths reached, kept forward-only on the device
                                                      // (cpprob_hip_batch_online_stats): an advance costs its new steps, whatever length the stream has reached
    bool learn_tables = false;                        // HmmTableStream (keep_history, or keep_masses): online EM -- the stream learns its tables on the device while
                                                      // its observes arrive (cpprob_hip_batch_learn_begin, _advance_learn): after every advance the M-step on the
                                                      // discounted running statistics gives the tables the next observes are filtered under; tables() reads them
    double learn_step_exponent = 0.6;                 // ... with the step sizes gamma[t] = (t + 1) ^ -this, evaluated on the host (0.5 < exponent <= 1)
    bool learn_scales = false;                        // hmm_table_fit and HmmTableStream with learn_tables, tables with HmmTable::sigmas: the per-state emission
                                                      // scales are fitted too (the M-step's sigma' = sqrt(occ_yy / occ - mean'^2)), none below scale_floor
    double scale_floor = 1e-3;                        // ... finite and > 0
    double rate_floor = 1e-6;                         // hmm_table_fit, tables with HmmTable::emission = Emission::poisson: no rate is fitted below it; finite and > 0
    std::size_t learn_burn_in = 20;                   // ... and no M-step before a problem has reached this length
    bool learn_tied = false;                          // HmmTableStream with learn_tables: tied online EM -- tie_groups (then required) partitions the streams,
                                                      // and the streams of a group learn ONE table on the device from their pooled records
                                                      // (cpprob_hip_batch_learn_tie); learn_burn_in then counts the observes a group has seen.  A
                                                      // non-empty tie_groups asks for the same
    bool map_decode = false;                          // batched runs (keep_history, or keep_masses): every result carries Result::map_path, the single most
                                                      // probable state sequence given the observes over the states the particles occupy, and
                                                      // Result::map_score (cpprob_hip_batch_decode); hmm_table_fit decodes under the fitted tables
    long decode_lag = -1;                             // ... not negative: Result::map_path holds the fixed-lag rows instead, row t the state at t of the
                                                      // best path of steps 0 .. min(t + lag, L - 1) (cpprob_hip_batch_decode_lag): what a stream labels
                                                      // with that delay.  HmmTableStream asks for the rows not yet final only
    bool markov_probe = true;                         // smc, unchanged-model path: test on the host whether a step depends on more than the last few
                                                      // sampled values; a model that does not is replayed from that window only (O(T) instead of O(T^2))
    bool markov_crosscheck = true;                    // ... and certify the probe's window on the device before using it: a pilot population under windowed
                                                      // and under full replay must agree bit for bit (once per model and trace shape), else full replay
    bool prefer_builtin = true;                       // use the hand-fused kernels when the model is one of the built-ins
    bool keep_history = true;                         // smc, built-in models on one GPU: false = filtering only -- O(N) particle store instead of O(N T),
                                                      // every predict hit's numbers under its own generation's weights, no posterior files
                                                      // (cpprob_hip_config::keep_history)
    bool keep_masses = false;                         // batched runs with keep_history = false: the run keeps the backward smoother's masses (64 bytes a
                                                      // problem and step, CPPROB_HIP_BATCH_KEEP_MASSES), so backward_smoothing, backward_trajectories,
                                                      // smoothing_lag and hmm_table_fit serve the filtering-only batch; lineage dumps stay refused
    bool fit_on_device = false;                       // hmm_table_fit: the batch is begun once and every later iteration gives it its new tables
                                                      // where it stands on the device (cpprob_hip_batch_retable: rows and thresholds rewritten by a
                                                      // kernel, the observes uploaded once) in place of a fresh begin; the same HmmTableFit bit for
                                                      // bit.  This host layer owns no device memory, so an iteration's record (88 doubles a problem)
                                                      // and its M-step still cross the host; cpprob_amd.hmm_table_em(resident=True) keeps both on the
                                                      // device (cpprob_hip_batch_mstep_device, _retable_device)
    std::vector<std::int32_t> tie_groups;             // hmm_table_fit: not empty = tied tables -- tie_groups[b] in 0 .. G-1 is problem b's group (every id
                                                      // used), the problems of a group share one table fitted to all of their observes: an iteration's
                                                      // records are pooled over each group on the device (cpprob_hip_batch_tie, _pool_stats) in front of
                                                      // the unchanged M-step.  A group's members must start from one table, bit for bit.  Empty: off
    std::vector<std::vector<int>> conditional_paths;  // hmm_table_batch with keep_history = false and keep_masses: not empty = the run is the conditional
                                                      // SMC run (cpprob_hip_batch_run_conditional), problem b's retained particle following
                                                      // conditional_paths[b] (one state a step).  It keeps masses, not books: what comes from
                                                      // cpprob_hip_batch_results stays default in the results; the smoothing, trajectory statistics,
                                                      // forecast and decode outputs asked for are filled as usual.  Empty: off
    std::uint64_t particle_offset = 0;                // (set by the engine when it shards a population: global id of this shard's first particle)
    bool progress = false;
    bool islands = false;                             // smc over several ranks, unchanged models: independent SMC runs combined by their evidence instead of
                                                      // the joint population (the default wherever the model has a joint form)
    int step_form_override = -1;                      // smc, unchanged-model path: -1 the engine chooses; 0 model launch + separate bookkeeping launches,
                                                      // 1 the resampling inside the model's launch against the dry run's bounds, 2 ... against exact maxima
    bool step_builds = true;                          // smc, unchanged-model path: launch the step kernels built per step (CPPROB_REGISTER_MODEL_STEPS) where the model
                                                      // unit holds them for a step's thresholds (false: always the run-time kernel -- the A/B switch)
    int replicates = 1;                               // built-in models: R independent runs (seeds seed .. seed + R - 1), up to three in
                                                      // flight on separate contexts; Result then carries their spread (error bars)
    bool joint_across_devices = false;                // smc, unchanged models, `devices` naming DIFFERENT GPUs: run the joint population (its peer reads have
                                                      // only ever run between loopback ranks of one device) instead of islands; Result::joint_note says so
};

struct PredictStats {            // one per predict hit, StatsPrinter's numbers
    std::string address;
    bool is_int = false;
    double mean = 0, variance = 0;            // real predicts (vector-valued: component 0)
    std::vector<double> mean_nd, variance_nd; // real predicts: one entry per component (size 1 for a scalar)
    std::vector<double> probabilities;        // int predicts: P(x = s), s = 0..k-1
};

struct Result {
    std::size_t n_particles = 0;
    double log_evidence = 0, ess = 0, log_norm = 0;
    int n_resampled = 0;
    bool used_builtin = false;
    int n_gpus = 1;                           // ranks the population was sharded over
    int exchange_reruns = 0;
    int markov_crosscheck = 0;                // unchanged-model smc: 1 the device pilot certified the probe's window, -1 it refuted it (full replay), 0 not run
    int replay_window = -1;                   // unchanged-model smc: samples of the ancestor a step replays (-1: the whole trace)                  // multi-GPU: runs repeated with a larger lineage transport (results never depend on it)
    bool joint = false;                       // unchanged-model smc over several ranks: ONE joint population (false: islands combined by their evidence)
    int joint_flag = 0;                       // (a rank's share of a joint run: the flag its generations raised)
    std::string joint_note;                   // why a multi-device smc call of an unchanged model ran islands, or that its joint run is unvalidated on real links
    int step_form = 0;                        // unchanged-model smc: 0 separate bookkeeping launches, 1 fused step on bounded references, 2 fused step + exact-maximum pass,
                                              // 3 = 1 with four particles a lane behind one ancestor search (chosen for large populations of models with <= 32 observes)
    int launches_per_step = 0;                // unchanged-model smc: dependent launches per observe
    int step_builds_used = 0;                 // unchanged-model smc: launches of the last attempt that ran a step kernel built for its step (model_step_kernel_at)
    double setup_seconds = 0;                 // unchanged-model path: context / workspace / scratch set-up and the Markov pilot of THIS call (0.0x ms once the workspace is warm)
    bool workspace_grown = false;             // ... this call created or enlarged its device workspace
    double run_seconds = 0;                   // device work of the run (launch to synchronise), excluding allocation and dumps
    std::vector<PredictStats> predicts;       // real hits first (in trace order), then int hits
    std::vector<double> step_ess;             // smc: ESS after each observe
    std::vector<std::vector<double>> forecast;                      // Options::forecast_horizon: [h - 1][s] = P(x_{L-1+h} = s | y_0 .. y_{L-1}), h = 1 .. horizon
    std::vector<std::vector<std::int32_t>> forecast_trajectories;   // Options::forecast_trajectories: [j][h], future j's states; h = 0 is the present state
    std::vector<std::vector<double>> trajectory_stats;              // Options::trajectory_stats: [j] = trajectory j's record of 88 doubles -- xi at 8 s + s' (transitions
                                                                    // s -> s'), then occ[8], occ_y[8], occ_yy[8]
    std::vector<double> running_stats;                              // Options::running_stats: the problem's record of 88 doubles in that layout, the expected statistics
    bool map_decoded = false;                 // Options::map_decode: the two fields below are set
    std::vector<std::int32_t> map_path;       // [t]: the most probable state path (Options::decode_lag >= 0: the fixed-lag rows)
    double map_score = 0;                     // the log joint density of the full decode's path and the observes; 0 without observes
    // Options::replicates > 1: replicate 0 is what the fields above (and the dump) describe; across replicates:
    int n_replicates = 1;
    double log_evidence_mean = 0, log_evidence_sd = 0;        // log of the mean evidence (unbiased in Z); sd of the log estimates
    std::vector<std::vector<double>> replicate_values;        // [predict hit][replicate]: mean (real, component 0) or P(x = 0) (int)
    std::vector<double> predict_mean, predict_sd;             // per predict hit over the replicates
    double replicates_seconds = 0;                            // device time of all replicates together
};

inline Options& options() { static thread_local Options o; return o; }
inline Result& last_result() { static thread_local Result r; return r; }

}  // namespace gpu
}  // namespace cpprob
#endif
