// Host driver in plain C++14 with the command-line surface of the reference's src/main.cpp for the
// sis path (flags :145-170, flow :69-107), plus --smc:
//     cpprob_main --model hmm16 --smc --n_samples 100000 --observes "[0.3 -1 ...]" --estimate
// Flags: --model {gaussian_unknown_mean, gaussian_readme, linear_gaussian_1d25, linear_gaussian_1d100, hmm16, hmm128, poisson_rate, gaussian_2d_unk_mean, ...}
//        --sis | --smc        --n_samples N (default 10000)    --observes "…" | --observes_file F
//        --generated_file NAME (default "post")   --model_folder DIR (default ".")   --estimate
//        additions: --seed S  --resampler {systematic,stratified,multinomial}  --ess_threshold X
//                   --generic (run the unchanged model body on the GPU instead of the fused kernels)
//                   --gpus N | --devices a,b,...  (one joint population sharded over several GPUs: exact global resampling, RCCL over xGMI;
//                                                  equal entries, e.g. 0,0,0: every rank on that GPU)
//                   --filtering_only (smc, built-in models: O(N) particle store, filtering statistics, no posterior files)
//                   --keep_masses (the batch modes and --stream_chunk, with --filtering_only: the runs keep the backward smoother's masses,
//                   64 bytes a problem and step, so --backward_smoothing, --backward_trajectories, --smoothing_lag and --em_iterations
//                   serve the filtering-only batch; same output as without the two flags)
//                   --no_dump  --dump_max_particles M  --json (print the in-memory result as one JSON line)
//                   --batch_observes_file F (smc, built-in HMMs: one observation sequence a line, all in one batched launch; seeds --seed + line
//                   index; one estimate a line, one JSON object a line under --json)
//                   --batch_tables_file F (smc, no --model: one table-weight HMM problem a line, "[means...] [transition, row-major...]
//                   [observes...]"; tables and lengths may differ from line to line; all in one batched launch, seeds and output as above)
//                   --stream_chunk K (with --batch_tables_file: the observes are fed K a problem at a time, one launch a chunk; same output)
//                   --batch_dump (both batch modes and --stream_chunk: problem b's posterior traces as <model_folder>/<generated_file>_smc_<b>.int / .ids,
//                   the files of a single run of that problem; resolved on the device in one launch)
//                   --backward_smoothing (the batch modes: the printed P(x_t = s) are the backward smoother's marginals -- every generation's
//                   whole filtering approximation -- instead of the surviving lineages')   --backward_trajectories M (with --batch_dump: the
//                   files hold M backward-simulated trajectories a problem, equal weights, in the lineages' place)
//                   --smoothing_lag L (the batch modes and --stream_chunk: the printed P(x_t = s) are the fixed-lag marginals
//                   P(x_t | y_0 .. y_min(t + L, T - 1)); with --stream_chunk every chunk costs its own steps; same output)
//                   --em_iterations N (with --batch_tables_file, not with --stream_chunk: particle EM -- N runs, each followed by the
//                   backward smoother's expected sufficient statistics and an M-step on every problem's table; the usual output is the
//                   last run's, then the fitted tables follow, one "[means] [transition]" line a problem in the input's grammar)
//                   --em_on_device (with --em_iterations: the batch is begun once and re-tabled on the device between the iterations,
//                   cpprob::gpu::Options::fit_on_device; the same output)
//                   --decode (the batch modes and --stream_chunk, not with --filtering_only unless --keep_masses: after the statistics, a
//                   line "decode b score x_0 .. x_{T-1}" a problem -- the single most probable state path given the observes, over the
//                   states the particles occupy, and its log joint density; --json carries "map_path" and "map_score" instead; with
//                   --em_iterations the decode is that of the fitted tables)   --decode_lag L (with --decode: x_t is the state at t of the
//                   best path of steps 0 .. min(t + L, T - 1), what a stream would have labelled L observes later)
//                   --conditional_paths FILE (with --batch_tables_file --filtering_only --keep_masses: the run is the conditional SMC run,
//                   problem b's retained particle following line b of FILE, T_b states; the estimates print as 0 -- such a run keeps
//                   masses, not books -- and --trajectory_stats, --backward_smoothing, --forecast and --decode read its masses as usual)
//                   --online_em [--em_step_exponent A] [--em_burn_in T] (with --batch_tables_file --stream_chunk K: online EM -- after every
//                   chunk the stream's tables are refitted on the device from the discounted running statistics, step sizes (t + 1)^-A
//                   (0.6), no M-step before T observes (20), and the next chunk is filtered under them; the final tables are printed as
//                   --em_iterations prints them)
//                   --emission_scales (with --batch_tables_file: every line carries four lists, [means] [sigmas] [transition] [observes]:
//                   state s emits N(means[s], sigmas[s]); the fitted tables are printed with their sigmas as a third list)
//                   --learn_scales [--scale_floor F] (with --emission_scales and --em_iterations or --online_em: the sigmas are fitted
//                   too, none below F (0.001); without it they stay)
//                   --poisson_emissions [--rate_floor F] (with --batch_tables_file: state s emits Poisson(rate[s]) -- every line carries
//                   the rates where it carries the means, [rates] [transition] [observes], and the observes are counts 0 .. 4095; with
//                   --em_iterations, --em_on_device, --tie_tables / --tie_groups and --stream_chunk, not with --emission_scales or
//                   --online_em; no rate is fitted below F (1e-6); the fitted rates are printed where the means are)
//                   --tie_tables / --tie_groups "[g_0 g_1 ..]" (with --em_iterations: tied tables -- all problems, or the problems with
//                   one group id (ids 0 .. G-1, every id used, one a problem), share one table fitted to all of their observes,
//                   cpprob::gpu::Options::tie_groups; their input tables must be equal; the output format is unchanged, the members of
//                   a group print the same fitted table; with --online_em --stream_chunk K: tied online EM -- the streams of a group
//                   learn one table on the device from their pooled records, cpprob::gpu::Options::learn_tied, and --em_burn_in counts
//                   the observes a group has seen)
//                   --running_stats (with --batch_tables_file --stream_chunk K: every chunk is followed by the forward-only update of the
//                   expected sufficient statistics, at the cost of the chunk's steps; after everything else one line a problem, the
//                   record of the lengths reached in --trajectory_stats' format)
// This file never touches HIP: it calls cpprob::inference exactly as the reference's main does.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "cpprob/cpprob.hpp"
#include "cpprob/postprocess/stats_printer.hpp"
#include "cpprob/serialization.hpp"
#include "registered_models.hpp"

namespace {

struct Args {
    std::string model, model_folder = ".", observes, observes_file, generated_file = "post", batch_observes_file, batch_tables_file;
    bool sis = false, smc = false, estimate = false, json = false, batch_dump = false;
    int repeat = 1;
    std::size_t n_samples = 10000;            // src/main.cpp:166
    std::size_t stream_chunk = 0;             // --batch_tables_file: feed every problem's observes this many at a time (0: all at once)
    std::size_t em_iterations = 0;            // --batch_tables_file: fit the tables by this many iterations of particle EM (0: none)
    bool emission_scales = false;             // --batch_tables_file: every line carries [sigmas] behind [means]: per-state emission scales
    bool poisson_emissions = false;           // --batch_tables_file: the first list of every line holds the rates of Poisson emissions
    std::string conditional_paths_file;       // --batch_tables_file: the reference paths of a conditional run, one line a problem (empty: none)
    bool tie_tables = false;                  // --em_iterations: all problems share one fitted table
    std::string tie_groups;                   // --em_iterations: "[g_0 g_1 ..]", the problems with one id share one fitted table (empty: none)
};

void print_json(const cpprob::gpu::Result& r)
{
    std::cout.precision(17);
    std::cout << "{\"n\": " << r.n_particles << ", \"log_evidence\": " << r.log_evidence << ", \"ess\": " << r.ess
              << ", \"n_resampled\": " << r.n_resampled << ", \"run_seconds\": " << r.run_seconds << ", \"builtin\": " << (r.used_builtin ? "true" : "false")
              << ", \"n_gpus\": " << r.n_gpus << ", \"exchange_reruns\": " << r.exchange_reruns << ", \"replay_window\": " << r.replay_window << ", \"markov_crosscheck\": " << r.markov_crosscheck
              << ", \"joint\": " << (r.joint ? "true" : "false") << ", \"joint_note\": \"" << r.joint_note << "\"" << ", \"step_form\": " << r.step_form << ", \"launches_per_step\": " << r.launches_per_step << ", \"step_builds_used\": " << r.step_builds_used << ", \"setup_seconds\": " << r.setup_seconds
              << ", \"workspace_grown\": " << (r.workspace_grown ? "true" : "false") << ", \"predicts\": [";
    for (std::size_t i = 0; i < r.predicts.size(); ++i) {
        const auto& p = r.predicts[i];
        if (i) std::cout << ", ";
        std::cout << "{\"address\": \"" << p.address << "\", ";
        if (p.is_int) {
            std::cout << "\"p\": [";
            for (std::size_t s = 0; s < p.probabilities.size(); ++s) std::cout << (s ? ", " : "") << p.probabilities[s];
            std::cout << "]}";
        } else {
            std::cout << "\"mean\": " << p.mean << ", \"variance\": " << p.variance;
            if (p.mean_nd.size() > 1) {                      // vector-valued predict: one entry per component
                std::cout << ", \"mean_nd\": [";
                for (std::size_t d = 0; d < p.mean_nd.size(); ++d) std::cout << (d ? ", " : "") << p.mean_nd[d];
                std::cout << "], \"variance_nd\": [";
                for (std::size_t d = 0; d < p.variance_nd.size(); ++d) std::cout << (d ? ", " : "") << p.variance_nd[d];
                std::cout << "]";
            }
            std::cout << "}";
        }
    }
    std::cout << "]";
    if (!r.forecast.empty()) {                                   // --forecast: row h - 1 the law of the state h steps past the last observe
        std::cout << ", \"forecast\": [";
        for (std::size_t h = 0; h < r.forecast.size(); ++h) {
            std::cout << (h ? ", [" : "[");
            for (std::size_t s = 0; s < r.forecast[h].size(); ++s) std::cout << (s ? ", " : "") << r.forecast[h][s];
            std::cout << "]";
        }
        std::cout << "], \"futures\": [";
        for (std::size_t j = 0; j < r.forecast_trajectories.size(); ++j) {
            std::cout << (j ? ", [" : "[");
            for (std::size_t h = 0; h < r.forecast_trajectories[j].size(); ++h) std::cout << (h ? ", " : "") << r.forecast_trajectories[j][h];
            std::cout << "]";
        }
        std::cout << "]";
    }
    if (r.map_decoded) {                                         // --decode: the most probable state path and its log joint density
        std::cout << ", \"map_score\": ";
        if (std::isfinite(r.map_score)) std::cout << r.map_score; else std::cout << "null";
        std::cout << ", \"map_path\": [";
        for (std::size_t t = 0; t < r.map_path.size(); ++t) std::cout << (t ? ", " : "") << r.map_path[t];
        std::cout << "]";
    }
    if (r.n_replicates > 1) {
        std::cout << ", \"replicates\": " << r.n_replicates << ", \"log_evidence_mean\": " << r.log_evidence_mean << ", \"log_evidence_sd\": " << r.log_evidence_sd
                  << ", \"replicates_seconds\": " << r.replicates_seconds << ", \"predict_mean\": [";
        for (std::size_t h = 0; h < r.predict_mean.size(); ++h) std::cout << (h ? ", " : "") << r.predict_mean[h];
        std::cout << "], \"predict_sd\": [";
        for (std::size_t h = 0; h < r.predict_sd.size(); ++h) std::cout << (h ? ", " : "") << r.predict_sd[h];
        std::cout << "]";
    }
    std::cout << "}" << std::endl;
}

// --forecast H [--forecast_trajectories M], after the statistics of the batch: problem b's rows "forecast b h p_0 .. p_{k-1}", the law
// of the state h = 1 .. H steps past its last observe, then "future b j x_0 .. x_H", simulated future j from the present state x_0 on
// (--json carries both inside the problem's object instead)
void print_forecasts(const std::vector<cpprob::gpu::Result>& res)
{
    for (std::size_t b = 0; b < res.size(); ++b) {
        for (std::size_t h = 0; h < res[b].forecast.size(); ++h) {
            std::cout << "forecast " << b << " " << h + 1;
            for (double v : res[b].forecast[h]) std::cout << " " << v;
            std::cout << std::endl;
        }
        for (std::size_t j = 0; j < res[b].forecast_trajectories.size(); ++j) {
            std::cout << "future " << b << " " << j;
            for (std::int32_t x : res[b].forecast_trajectories[j]) std::cout << " " << x;
            std::cout << std::endl;
        }
    }
}

// --decode [--decode_lag L], after the statistics (and the forecasts) of the batch: problem b's row "decode b score x_0 .. x_{T-1}"
// (--json carries both inside the problem's object instead)
void print_decodes(const std::vector<cpprob::gpu::Result>& res)
{
    for (std::size_t b = 0; b < res.size(); ++b) {
        if (!res[b].map_decoded) continue;
        std::cout << "decode " << b << " " << res[b].map_score;
        for (std::int32_t x : res[b].map_path) std::cout << " " << x;
        std::cout << std::endl;
    }
}

// --trajectory_stats M [--draw_index D], after everything else of the batch (in --json mode too): M lines a problem in problem order,
// line j the record of its backward-simulated trajectory j, "[xi k x k row-major] [occ] [occ_y] [occ_yy]" over the first k states
void print_stats_record(const std::vector<double>& rec, std::size_t k)
{
    std::cout << "[";
    for (std::size_t s = 0; s < k; ++s)
        for (std::size_t j = 0; j < k; ++j) std::cout << (s + j ? " " : "") << rec[8 * s + j];
    for (std::size_t part = 0; part < 3; ++part) {
        std::cout << "] [";
        for (std::size_t s = 0; s < k; ++s) std::cout << (s ? " " : "") << rec[64 + 8 * part + s];
    }
    std::cout << "]" << std::endl;
}

void print_trajectory_stats(const std::vector<cpprob::gpu::Result>& res, std::size_t k)
{
    for (const cpprob::gpu::Result& r : res)
        for (const std::vector<double>& rec : r.trajectory_stats) print_stats_record(rec, k);
}

// --running_stats (with --stream_chunk), after the trajectory statistics (in --json mode too): one line a problem in problem order,
// its running record of the lengths reached in the same format
void print_running_stats(const std::vector<cpprob::gpu::Result>& res, std::size_t k)
{
    for (const cpprob::gpu::Result& r : res)
        if (!r.running_stats.empty()) print_stats_record(r.running_stats, k);
}

// --batch_observes_file F: one observation sequence a line, all run as ONE batch (cpprob::gpu::inference_batch, smc, built-in HMMs);
// problem i (line i) runs with seed --seed + i; one estimate a line: log-evidence, then P(x_t = s) row by row (--json: one JSON object a line)
template <class F>
int execute_batch(const F& model, const Args& a)
{
    if (!a.smc) { std::cerr << "--batch_observes_file runs SMC: set --smc" << std::endl; return EXIT_FAILURE; }
    std::ifstream in(a.model_folder + "/" + a.batch_observes_file);
    if (!in) { std::cerr << "cannot open " << a.model_folder << "/" << a.batch_observes_file << std::endl; return EXIT_FAILURE; }
    std::vector<cpprob::tuple_observes_t<F>> observes;
    std::vector<std::uint64_t> seeds;
    std::string line;
    while (std::getline(in, line)) {
        cpprob::tuple_observes_t<F> o;
        if (!cpprob::parse_string(line, o)) { std::cerr << "Could not parse the observations of line " << observes.size() << "." << std::endl; return EXIT_FAILURE; }
        seeds.push_back(cpprob::gpu::options().seed + observes.size());
        observes.push_back(o);
    }
    if (a.batch_dump) cpprob::gpu::options().batch_dump_file = a.model_folder + "/" + a.generated_file + "_smc";
    const std::vector<cpprob::gpu::Result> res = cpprob::gpu::inference_batch(cpprob::StateType::smc, model, observes, a.n_samples, seeds);
    std::cout.precision(17);
    for (const cpprob::gpu::Result& r : res) {
        if (a.json) { print_json(r); continue; }
        std::cout << r.log_evidence;
        for (const auto& p : r.predicts)
            for (double v : p.probabilities) std::cout << " " << v;
        std::cout << std::endl;
    }
    if (!a.json) print_forecasts(res);
    if (!a.json) print_decodes(res);
    print_trajectory_stats(res, res.empty() || res[0].predicts.empty() ? 8 : res[0].predicts[0].probabilities.size());
    cpprob::gpu::release_device_resources();
    return EXIT_SUCCESS;
}

// --batch_tables_file F: one problem of the k-state table HMM a line -- its means (k numbers), its transition weights (k x k, row-major)
// and its observes (any number), three lists in the grammar of --observes; k is the length of the first list of the first line.  All
// lines run as ONE batch (cpprob::gpu::hmm_table_batch) with --n_samples particles each; output as for --batch_observes_file.
int execute_batch_tables(const Args& a)
{
    if (!a.smc) { std::cerr << "--batch_tables_file runs SMC: set --smc" << std::endl; return EXIT_FAILURE; }
    std::ifstream in(a.model_folder + "/" + a.batch_tables_file);
    if (!in) { std::cerr << "cannot open " << a.model_folder << "/" << a.batch_tables_file << std::endl; return EXIT_FAILURE; }
    std::vector<cpprob::gpu::HmmTable> tables;
    std::vector<std::vector<double>> observes;
    std::vector<std::uint64_t> seeds;
    std::string line;
    std::size_t k = 0;
    while (std::getline(in, line)) {
        const std::size_t at = tables.size();
        std::tuple<std::vector<double>, std::vector<double>, std::vector<double>> p;
        std::vector<double> sigmas;
        if (a.emission_scales) {
            // --emission_scales: four lists a line, [means] [sigmas] [transition] [observes]
            std::tuple<std::vector<double>, std::vector<double>, std::vector<double>, std::vector<double>> q;
            if (!cpprob::parse_string(line, q)) { std::cerr << "Could not parse line " << at << ": expected [means] [sigmas] [transition] [observes]." << std::endl; return EXIT_FAILURE; }
            sigmas = std::get<1>(q);
            if (sigmas.size() != std::get<0>(q).size()) { std::cerr << "line " << at << ": " << sigmas.size() << " sigmas for " << std::get<0>(q).size() << " means." << std::endl; return EXIT_FAILURE; }
            p = std::make_tuple(std::get<0>(q), std::get<2>(q), std::get<3>(q));
        }
        else if (!cpprob::parse_string(line, p)) { std::cerr << "Could not parse line " << at << ": expected [means] [transition] [observes]." << std::endl; return EXIT_FAILURE; }
        if (at == 0) k = std::get<0>(p).size();
        if (std::get<0>(p).size() != k) { std::cerr << "line " << at << ": " << std::get<0>(p).size() << " means, but the first line has " << k << "." << std::endl; return EXIT_FAILURE; }
        if (std::get<1>(p).size() != k * k) { std::cerr << "line " << at << ": the transition list holds " << std::get<1>(p).size() << " weights, not k x k = " << k * k << "." << std::endl; return EXIT_FAILURE; }
        if (std::get<2>(p).empty()) { std::cerr << "line " << at << ": no observes." << std::endl; return EXIT_FAILURE; }
        tables.push_back(cpprob::gpu::HmmTable{std::get<0>(p), std::get<1>(p), sigmas});
        if (a.poisson_emissions) tables.back().emission = cpprob::gpu::Emission::poisson;
        observes.push_back(std::get<2>(p));
        seeds.push_back(cpprob::gpu::options().seed + at);
    }
    if (tables.empty()) { std::cerr << "no problems in " << a.batch_tables_file << std::endl; return EXIT_FAILURE; }
    if (!a.conditional_paths_file.empty()) {
        if (a.em_iterations || a.stream_chunk) { std::cerr << "--conditional_paths replaces the run of one batch: not with --em_iterations or --stream_chunk" << std::endl; return EXIT_FAILURE; }
        std::ifstream pin(a.model_folder + "/" + a.conditional_paths_file);
        if (!pin) { std::cerr << "cannot open " << a.model_folder << "/" << a.conditional_paths_file << std::endl; return EXIT_FAILURE; }
        std::vector<std::vector<int>>& paths = cpprob::gpu::options().conditional_paths;
        paths.clear();
        while (std::getline(pin, line)) {
            std::istringstream ls(line);
            std::vector<int> path;
            for (int s2; ls >> s2;) path.push_back(s2);
            if (!ls.eof()) { std::cerr << "--conditional_paths: line " << paths.size() << " holds something that is no integer." << std::endl; return EXIT_FAILURE; }
            paths.push_back(path);
        }
        if (paths.size() != tables.size()) { std::cerr << "--conditional_paths: " << paths.size() << " lines for " << tables.size() << " problems." << std::endl; return EXIT_FAILURE; }
    }
    if (a.em_iterations && a.stream_chunk) { std::cerr << "--em_iterations begins a fresh batch an iteration: not with --stream_chunk" << std::endl; return EXIT_FAILURE; }
    std::vector<cpprob::gpu::Result> res;
    std::vector<cpprob::gpu::HmmTable> fitted;
    const std::string dump_prefix = a.model_folder + "/" + a.generated_file + "_smc";
    if (a.batch_dump && a.stream_chunk == 0) cpprob::gpu::options().batch_dump_file = dump_prefix;
    if (a.tie_tables) cpprob::gpu::options().tie_groups.assign(tables.size(), 0);
    else if (!a.tie_groups.empty()) {
        std::string ids = a.tie_groups;
        for (char& ch : ids) if (ch == '[' || ch == ']' || ch == ',') ch = ' ';
        std::istringstream gs(ids);
        std::vector<std::int32_t>& tie = cpprob::gpu::options().tie_groups;
        tie.clear();
        for (long g; gs >> g;) tie.push_back(static_cast<std::int32_t>(g));
        if (!gs.eof()) { std::cerr << "--tie_groups: the list holds something that is no integer." << std::endl; return EXIT_FAILURE; }
        if (tie.size() != tables.size()) { std::cerr << "--tie_groups: " << tie.size() << " ids for " << tables.size() << " problems." << std::endl; return EXIT_FAILURE; }
    }
    if (a.em_iterations) {
        cpprob::gpu::HmmTableFit fit = cpprob::gpu::hmm_table_fit(tables, observes, std::vector<std::size_t>{a.n_samples}, seeds, a.em_iterations);
        res = std::move(fit.results);
        fitted = std::move(fit.tables);
    }
    else if (a.stream_chunk == 0) res = cpprob::gpu::hmm_table_batch(tables, observes, std::vector<std::size_t>{a.n_samples}, seeds);
    else {
        // --stream_chunk K: the same batch fed K observes a problem at a time (cpprob::gpu::HmmTableStream); the last chunk may be
        // shorter, a problem that has run out gets none, and only the last advance does the read-out.  The output is the same.
        std::vector<std::size_t> cap;
        std::size_t longest = 0;
        for (const auto& o : observes) { cap.push_back(o.size()); longest = std::max(longest, o.size()); }
        cpprob::gpu::HmmTableStream stream(tables, cap, std::vector<std::size_t>{a.n_samples}, seeds);
        for (std::size_t at = 0; at < longest; at += a.stream_chunk) {
            std::vector<std::vector<double>> piece(observes.size());
            for (std::size_t b = 0; b < observes.size(); ++b) {
                const std::size_t lo = std::min(at, observes[b].size()), hi = std::min(at + a.stream_chunk, observes[b].size());
                piece[b].assign(observes[b].begin() + static_cast<std::ptrdiff_t>(lo), observes[b].begin() + static_cast<std::ptrdiff_t>(hi));
            }
            res = stream.advance(piece, at + a.stream_chunk >= longest);
        }
        if (a.batch_dump) stream.dump(dump_prefix);
        if (cpprob::gpu::options().learn_tables) fitted = stream.tables();      // --online_em: the tables the stream has learned
    }
    std::cout.precision(17);
    for (const cpprob::gpu::Result& r : res) {
        if (a.json) { print_json(r); continue; }
        std::cout << r.log_evidence;
        for (const auto& p : r.predicts)
            for (double v : p.probabilities) std::cout << " " << v;
        std::cout << std::endl;
    }
    if (!a.json) print_forecasts(res);
    if (!a.json) print_decodes(res);
    for (const cpprob::gpu::HmmTable& t : fitted) {
        std::cout << "[";
        for (std::size_t s = 0; s < t.means.size(); ++s) std::cout << (s ? " " : "") << t.means[s];
        std::cout << "] [";
        for (std::size_t i = 0; i < t.transition.size(); ++i) std::cout << (i ? " " : "") << t.transition[i];
        std::cout << "]";
        if (!t.sigmas.empty()) {
            // (tables with emission scales: the fitted sigmas behind the table)
            std::cout << " [";
            for (std::size_t s = 0; s < t.sigmas.size(); ++s) std::cout << (s ? " " : "") << t.sigmas[s];
            std::cout << "]";
        }
        std::cout << std::endl;
    }
    print_trajectory_stats(res, k);
    print_running_stats(res, k);
    cpprob::gpu::release_device_resources();
    return EXIT_SUCCESS;
}

template <class F>
int execute(const F& model, const Args& a)
{
    if (!a.batch_observes_file.empty()) return execute_batch(model, a);
    if (a.observes_file.empty() == a.observes.empty()) {
        std::cerr << R"(In SIS or SMC mode exactly one of the options "--observes" or "--observes_file" has to be set)" << std::endl;   // main.cpp:72-75
        return EXIT_FAILURE;
    }
    cpprob::tuple_observes_t<F> observes;
    const bool ok = a.observes_file.empty() ? cpprob::parse_string(a.observes, observes)
                                            : cpprob::parse_file(a.model_folder + "/" + a.observes_file, observes);
    if (!ok) {
        std::cerr << "Could not parse the observations.\n"
                  << "Please use spaces to separate the observations and elements of an aggregate type instead of commas.\n";   // main.cpp:87-92
        return EXIT_FAILURE;
    }
    const std::string post = a.model_folder + "/" + a.generated_file + (a.smc ? "_smc" : "_sis");                            // main.cpp:49-53
    if (a.smc) std::cout << "Sequential Monte Carlo (SMC)" << std::endl;
    else std::cout << "Sequential Importance Sampling (SIS)" << std::endl;                                                   // main.cpp:99
    for (int rep = 0; rep < a.repeat; ++rep) {                       // --repeat: the first call pays code loading; later ones show the warm rate
        if (rep) cpprob::gpu::options().seed += 1;
        cpprob::inference(a.smc ? cpprob::StateType::smc : cpprob::StateType::sis, model, observes, a.n_samples, post);
        if (a.repeat > 1) std::cout << "run " << rep << ": " << cpprob::gpu::last_result().run_seconds * 1e3 << " ms (set-up " << cpprob::gpu::last_result().setup_seconds * 1e3 << " ms)" << std::endl;
    }
    if (a.json) print_json(cpprob::gpu::last_result());
    if (a.estimate) {
        std::cout << "Posterior Distribution Estimators" << std::endl;                                                      // main.cpp:104
        std::cout << cpprob::StatsPrinter{post};
    }
    cpprob::gpu::release_device_resources();                         // (contexts and workspaces kept between calls: freed while the runtime is alive)
    return EXIT_SUCCESS;
}

}  // namespace

int main(int argc, char** argv)
{
    Args a;
    auto& opt = cpprob::gpu::options();
    for (int i = 1; i < argc; ++i) {
        const std::string f = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { std::cerr << "missing value for " << f << std::endl; std::exit(EXIT_FAILURE); } return argv[++i]; };
        if (f == "--model" || f == "-m") a.model = next();
        else if (f == "--model_folder") a.model_folder = next();
        else if (f == "--sis") a.sis = true;
        else if (f == "--smc") a.smc = true;
        else if (f == "--estimate" || f == "-e") a.estimate = true;
        else if (f == "--n_samples" || f == "-n") a.n_samples = std::stoull(next());
        else if (f == "--observes" || f == "-o") a.observes = next();
        else if (f == "--observes_file") a.observes_file = next();
        else if (f == "--batch_observes_file") a.batch_observes_file = next();   // one problem a line, one batched launch (built-in HMMs, smc)
        else if (f == "--batch_tables_file") a.batch_tables_file = next();       // one table-HMM problem a line: [means] [transition] [observes]
        else if (f == "--stream_chunk") a.stream_chunk = std::stoull(next());    // --batch_tables_file: the observes arrive this many at a time
        else if (f == "--em_on_device") opt.fit_on_device = true;                  // --em_iterations: one begin, then cpprob_hip_batch_retable an iteration
        else if (f == "--em_iterations") a.em_iterations = std::stoull(next());  // --batch_tables_file: particle EM on the tables (cpprob::gpu::hmm_table_fit)
        else if (f == "--tie_tables") a.tie_tables = true;                         // --em_iterations: every problem in one group (cpprob::gpu::Options::tie_groups)
        else if (f == "--tie_groups") a.tie_groups = next();                       // --em_iterations: "[0 0 1 1]", one group id a problem
        else if (f == "--batch_dump") a.batch_dump = true;                         // the batch modes: problem b's traces as <generated_file>_smc_<b>.int / .ids
        else if (f == "--backward_smoothing") opt.backward_smoothing = true;      // the batch modes: statistics from the backward smoother (cpprob_hip_batch_smooth)
        else if (f == "--smoothing_lag") opt.smoothing_lag = std::stol(next());    // the batch modes: fixed-lag marginals (cpprob_hip_batch_smooth_lag)
        else if (f == "--decode") opt.map_decode = true;                           // the batch modes: the most probable state path (cpprob_hip_batch_decode)
        else if (f == "--decode_lag") opt.decode_lag = std::stol(next());          // ... its fixed-lag rows instead (cpprob_hip_batch_decode_lag)
        else if (f == "--trajectory_stats") opt.trajectory_stats = std::stoull(next());   // the batch modes: the records of this many backward-simulated trajectories a problem (cpprob_hip_batch_traj_stats)
        else if (f == "--online_em") opt.learn_tables = true;                      // --batch_tables_file --stream_chunk: the stream learns its tables on the device (cpprob_hip_batch_advance_learn)
        else if (f == "--em_step_exponent") opt.learn_step_exponent = std::stod(next());   // ... with the step sizes (t + 1) ^ -A
        else if (f == "--emission_scales") a.emission_scales = true;              // --batch_tables_file: every line is [means] [sigmas] [transition] [observes]
        else if (f == "--poisson_emissions") a.poisson_emissions = true;          // --batch_tables_file: every line is [rates] [transition] [observes], the observes counts
        else if (f == "--rate_floor") opt.rate_floor = std::stod(next());          // ... --em_iterations fits no rate below this
        else if (f == "--learn_scales") opt.learn_scales = true;                   // --em_iterations / --online_em with --emission_scales: the sigmas are fitted too
        else if (f == "--scale_floor") opt.scale_floor = std::stod(next());        // ... none below this
        else if (f == "--em_burn_in") opt.learn_burn_in = std::stoull(next());      // ... and no M-step before a problem has this many observes
        else if (f == "--running_stats") opt.running_stats = true;                 // --batch_tables_file --stream_chunk: the expected statistics kept forward-only (cpprob_hip_batch_online_stats)
        else if (f == "--draw_index") opt.trajectory_stats_draw_index = std::stoull(next());   // ... under this draw index
        else if (f == "--forecast") opt.forecast_horizon = std::stoull(next());   // the batch modes: the state's laws this many steps ahead (cpprob_hip_batch_forecast)
        else if (f == "--forecast_trajectories") opt.forecast_trajectories = std::stoull(next());   // ... and this many simulated futures a problem
        else if (f == "--backward_trajectories") opt.backward_trajectories = std::stoull(next());   // ... and --batch_dump writes this many backward-simulated trajectories
        else if (f == "--dump_max_particles") opt.dump_max_particles = std::stoull(next());   // the posterior files hold the first M traces only (0: all)
        else if (f == "--generated_file") a.generated_file = next();
        else if (f == "--seed") opt.seed = std::stoull(next());
        else if (f == "--ess_threshold") opt.ess_threshold = std::stod(next());
        else if (f == "--resampler") { const std::string r = next(); opt.resampler = r == "multinomial" ? 2 : (r == "stratified" ? 1 : 0); }
        else if (f == "--generic") opt.prefer_builtin = false;
        else if (f == "--conditional_paths") a.conditional_paths_file = next();     // --batch_tables_file --filtering_only --keep_masses: the run is the conditional SMC run; FILE: one line of T_b states a problem
        else if (f == "--keep_masses") opt.keep_masses = true;                     // the batch modes, with --filtering_only: CPPROB_HIP_BATCH_KEEP_MASSES
        else if (f == "--filtering_only") { opt.keep_history = false; opt.dump = false; }   // smc, built-in models: O(N) particle store, filtering statistics
        else if (f == "--islands") opt.islands = true;                          // unchanged-model smc over several ranks: independent runs combined by evidence
        else if (f == "--joint_across_devices") opt.joint_across_devices = true; // ... or the joint population even across physical GPUs (unvalidated on real links)
        else if (f == "--step_form") opt.step_form_override = std::stoi(next());   // unchanged-model smc: 0 separate bookkeeping launches, 1 fused (bounds), 2 fused (exact maxima)
        else if (f == "--no_markov_probe") opt.markov_probe = false;          // unchanged-model smc: replay the whole trace every step
        else if (f == "--no_markov_crosscheck") opt.markov_crosscheck = false; // ... trust the host probe's window without the device pilot
        else if (f == "--gpus") { const int k = std::stoi(next()); opt.devices.clear(); for (int d = 0; d < k; ++d) opt.devices.push_back(d); }
        else if (f == "--devices") {                        // e.g. 0,1,2,3 -- or 0,0 for two ranks on one GPU (loopback transport)
            const std::string v = next(); opt.devices.clear();
            std::size_t p0 = 0;
            while (p0 <= v.size()) { const std::size_t q = v.find(',', p0); opt.devices.push_back(std::stoi(v.substr(p0, q == std::string::npos ? q : q - p0))); if (q == std::string::npos) break; p0 = q + 1; }
        }
        else if (f == "--repeat") a.repeat = std::stoi(next());
        else if (f == "--no_step_builds") opt.step_builds = false;          // unchanged-model smc: the run-time step kernel at every step (A/B against the per-step builds)
        else if (f == "--replicates") opt.replicates = std::stoi(next());
        else if (f == "--no_dump") opt.dump = false;
        else if (f == "--json") a.json = true;
        else { std::cerr << "unknown option " << f << std::endl; return EXIT_FAILURE; }
    }
    if (a.sis == a.smc) { std::cerr << "exactly one of --sis / --smc has to be set" << std::endl; return EXIT_FAILURE; }
    if (a.poisson_emissions && a.batch_tables_file.empty()) { std::cerr << "--poisson_emissions reads the rates of --batch_tables_file" << std::endl; return EXIT_FAILURE; }
    if (a.poisson_emissions && a.emission_scales) { std::cerr << "--poisson_emissions and --emission_scales name two emission families: a batch has one" << std::endl; return EXIT_FAILURE; }
    if (a.poisson_emissions && opt.learn_tables) { std::cerr << "--online_em serves Gaussian emissions: fit Poisson tables with --em_iterations" << std::endl; return EXIT_FAILURE; }
    if (a.emission_scales && a.batch_tables_file.empty()) { std::cerr << "--emission_scales reads the sigmas of --batch_tables_file" << std::endl; return EXIT_FAILURE; }
    if (opt.learn_scales && (!a.emission_scales || (a.em_iterations == 0 && !opt.learn_tables))) {
        std::cerr << "--learn_scales fits the sigmas of --emission_scales: set it with --em_iterations or --online_em" << std::endl;
        return EXIT_FAILURE;
    }
    if ((a.tie_tables || !a.tie_groups.empty()) && a.em_iterations == 0 && !opt.learn_tables) {
        std::cerr << "--tie_tables / --tie_groups tie the tables of a fit: set --em_iterations, or --online_em with --stream_chunk" << std::endl;
        return EXIT_FAILURE;
    }
    if ((a.tie_tables || !a.tie_groups.empty()) && opt.learn_tables) opt.learn_tied = true;      // --online_em: the streams of a group learn one table
    if (a.tie_tables && !a.tie_groups.empty()) { std::cerr << "--tie_tables is --tie_groups of all zeros: set one of them" << std::endl; return EXIT_FAILURE; }
    if (opt.fit_on_device && a.em_iterations == 0) { std::cerr << "--em_on_device re-tables the batch of a fit: set --em_iterations" << std::endl; return EXIT_FAILURE; }
    if ((opt.forecast_horizon || opt.forecast_trajectories) && a.batch_tables_file.empty() && a.batch_observes_file.empty()) {
        std::cerr << "--forecast serves the batch modes: set --batch_observes_file or --batch_tables_file" << std::endl;
        return EXIT_FAILURE;
    }
    if ((opt.map_decode || opt.decode_lag >= 0) && a.batch_tables_file.empty() && a.batch_observes_file.empty()) {
        std::cerr << "--decode serves the batch modes: set --batch_observes_file or --batch_tables_file" << std::endl;
        return EXIT_FAILURE;
    }
    if (opt.trajectory_stats && a.batch_tables_file.empty() && a.batch_observes_file.empty()) {
        std::cerr << "--trajectory_stats serves the batch modes: set --batch_observes_file or --batch_tables_file" << std::endl;
        return EXIT_FAILURE;
    }
    if (opt.trajectory_stats && !opt.keep_history && !opt.keep_masses) {
        std::cerr << "--trajectory_stats reads the smoother's masses: with --filtering_only set --keep_masses" << std::endl;
        return EXIT_FAILURE;
    }
    if (opt.running_stats && (a.batch_tables_file.empty() || a.stream_chunk == 0)) {
        std::cerr << "--running_stats follows a stream: set --batch_tables_file and --stream_chunk" << std::endl;
        return EXIT_FAILURE;
    }
    if (opt.learn_tables && (a.batch_tables_file.empty() || a.stream_chunk == 0)) {
        std::cerr << "--online_em learns the tables of a stream: set --batch_tables_file and --stream_chunk" << std::endl;
        return EXIT_FAILURE;
    }
    if (opt.learn_tables && !opt.keep_history && !opt.keep_masses) {
        std::cerr << "--online_em reads the smoother's masses: with --filtering_only set --keep_masses" << std::endl;
        return EXIT_FAILURE;
    }
    if (opt.running_stats && !opt.keep_history && !opt.keep_masses) {
        std::cerr << "--running_stats reads the smoother's masses: with --filtering_only set --keep_masses" << std::endl;
        return EXIT_FAILURE;
    }
    if (opt.decode_lag >= 0 && !opt.map_decode) { std::cerr << "--decode_lag delays a decode: set --decode" << std::endl; return EXIT_FAILURE; }
    if (opt.map_decode && !opt.keep_history && !opt.keep_masses) {
        std::cerr << "--decode reads the smoother's masses: with --filtering_only set --keep_masses" << std::endl;
        return EXIT_FAILURE;
    }
    try {
        if (!a.batch_tables_file.empty()) return execute_batch_tables(a);     // (the model is the table HMM: --model is not read)
        if (a.model == "gaussian_unknown_mean") return execute(models::gaussian_unknown_mean<double>, a);     // main.cpp:123-130
        if (a.model == "gaussian_readme") return execute(models::gaussian_readme<double>, a);
        if (a.model == "linear_gaussian_1d25") return execute(models::linear_gaussian_1d<25>, a);
        if (a.model == "linear_gaussian_1d100") return execute(models::linear_gaussian_1d<100>, a);
        if (a.model == "hmm16") return execute(models::hmm<16>, a);
        if (a.model == "hmm128") return execute(models::hmm<128>, a);
        if (a.model == "poisson_rate") return execute(models::poisson_rate<double>, a);
        if (a.model == "gaussian_2d_unk_mean") return execute(models::gaussian_2d_unk_mean<double>, a);       // observes: "[y0 y1]"
        if (a.model == "gauss_functor") return execute(models::GaussFunctor<double>{}, a);
        if (a.model == "gaussian_by_rejection") return execute(models::gaussian_by_rejection<double>, a);
        if (a.model == "second_order12") return execute(models::second_order<12>, a);
        if (a.model == "running_mean12") return execute(models::running_mean<12>, a);
        if (a.model == "rare_memory12") return execute(models::rare_memory<12>, a);
        if (a.model == "random_scale12") return execute(models::random_scale<12>, a);
        if (a.model == "all_distr") return execute(models::all_distr<int>, a);                                   // src/models/models.cpp:13-47; observes: any two ints
        std::cerr << "unknown model " << a.model << std::endl;
        return EXIT_FAILURE;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 2;
    }
}
