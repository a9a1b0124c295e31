// Host driver of a device inference run: RAII over the C ABI (include/cpprob_hip.h), the built-in-model
// path, the posterior file dump in the reference grammar, and the glue cpprob::inference uses.
// Plain C++14.  Errors from the C ABI become std::runtime_error (the reference has no error returns
// on this path: SURVEY section 8(b)).
#ifndef CPPROB_COMPAT_DETAIL_HOST_ENGINE_HPP
#define CPPROB_COMPAT_DETAIL_HOST_ENGINE_HPP
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <limits>
#include <memory>
#include <algorithm>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "cpprob/detail/registry.hpp"
#include "cpprob/detail/traits.hpp"
#include "cpprob_hip.h"

namespace cpprob {
namespace gpu {

class Context {
public:
    explicit Context(int device)
    {
        const int rc = cpprob_hip_create(device, &h_);
        if (rc) throw std::runtime_error(std::string("cpprob_hip_create: ") + cpprob_hip_last_error(nullptr));
    }
    ~Context() { if (h_) cpprob_hip_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    cpprob_hip_ctx* get() const { return h_; }
    void check(int rc, const char* what) const
    {
        if (rc) throw std::runtime_error(std::string(what) + ": " + cpprob_hip_last_error(h_));
    }
private:
    cpprob_hip_ctx* h_ = nullptr;
};

// Contexts are kept between two cpprob::inference calls (the reference's call is `inference(...)` again and again, src/main.cpp:96-100):
// a context made per call cost 1.6-2.2 ms of stream and buffer creation around a 0.2 ms run of 10^6 HMM particles.  A call leases one
// for its device (concurrent calls get contexts of their own); cpprob::gpu::release_device_resources() destroys the idle ones -- they
// are deliberately not torn down by static destructors, which run when the HIP runtime may already be gone.
struct ContextPool { std::mutex mu; std::vector<std::pair<int, std::unique_ptr<Context>>> idle; };
CPPROB_REGISTRY_VISIBLE inline ContextPool& context_pool() { static ContextPool* p = new ContextPool; return *p; }
inline void release_contexts()
{
    ContextPool& p = context_pool();
    std::lock_guard<std::mutex> lock(p.mu);
    p.idle.clear();
}
class ContextLease {
public:
    explicit ContextLease(int device) : device_(device)
    {
        ContextPool& p = context_pool();
        {
            std::lock_guard<std::mutex> lock(p.mu);
            for (auto it = p.idle.begin(); it != p.idle.end(); ++it)
                if (it->first == device) { c_ = std::move(it->second); p.idle.erase(it); break; }
        }
        if (!c_) { c_.reset(new Context(device)); add_release_hook(&release_contexts); }
    }
    ~ContextLease()
    {
        // (a call that threw leaves its context in an unknown state: destroyed, not returned)
        if (!ok_) return;
        ContextPool& p = context_pool();
        std::lock_guard<std::mutex> lock(p.mu);
        p.idle.emplace_back(device_, std::move(c_));
    }
    Context& operator*() const { return *c_; }
    Context* operator->() const { return c_.get(); }
    void done() { ok_ = true; }
private:
    int device_;
    std::unique_ptr<Context> c_;
    bool ok_ = false;
};

// ---- flatten the observes tuple into doubles (scalars and std::array<double, N>) -----------------
template <class T, std::enable_if_t<std::is_arithmetic<T>::value, int> = 0>
void flatten_one(std::vector<double>& out, T x) { out.push_back(static_cast<double>(x)); }
template <class T, std::size_t N> void flatten_one(std::vector<double>& out, const std::array<T, N>& a) { for (const auto& x : a) out.push_back(static_cast<double>(x)); }
template <class T> void flatten_one(std::vector<double>& out, const std::vector<T>& a) { for (const auto& x : a) out.push_back(static_cast<double>(x)); }
template <class Tuple, std::size_t... I>
void flatten_impl(std::vector<double>& out, const Tuple& t, std::index_sequence<I...>) { (void)std::initializer_list<int>{(flatten_one(out, std::get<I>(t)), 0)...}; }
template <class... A>
std::vector<double> flatten(const std::tuple<A...>& t) { std::vector<double> out; flatten_impl(out, t, std::index_sequence_for<A...>{}); return out; }

// ---- posterior files: StateInfer::dump_predicts / dump_ids (src/cpprob/state.cpp:250-267) -----------
// line i of <file>.real / .int:  ([(id v) (id v) ...] logw)   scientific, precision digits10 = 15
inline void dump_posterior(const std::string& file, const detail::TraceStructure& st, const HostStore& hs, std::size_t max_particles)
{
    const std::size_t n = (max_particles && max_particles < hs.n) ? max_particles : hs.n;
    auto write = [&](const std::string& path, const std::vector<std::size_t>& ids, bool is_int) {
        if (ids.empty()) { std::remove(path.c_str()); return; }          // all-empty files are removed (state.cpp:166-174)
        std::ofstream f(path.c_str(), std::ios::app);                     // append mode, as the reference (state.cpp:264)
        f.precision(std::numeric_limits<double>::digits10);
        f << std::scientific;
        for (std::size_t i = 0; i < n; ++i) {
            f << "([";
            std::size_t row = 0;
            for (std::size_t k = 0; k < ids.size(); ++k) {
                if (k) f << ' ';
                f << '(' << ids[k] << ' ';
                if (is_int) f << hs.ints[k * hs.n + i];
                else {
                    const std::size_t w = st.real_width[k];          // an NDArray prints as [v0 v1 ...] (ndarray.hpp:273-288)
                    if (w != 1) f << '[';
                    for (std::size_t d = 0; d < w; ++d) { if (d) f << ' '; f << hs.real[(row + d) * hs.n + i]; }
                    if (w != 1) f << ']';
                    row += w;
                }
                f << ')';
            }
            f << "] " << hs.logw[i] << ")\n";
        }
    };
    write(file + ".int", st.int_ids, true);
    write(file + ".real", st.real_ids, false);
    std::remove((file + ".any").c_str());
    std::ofstream ids((file + ".ids").c_str());
    for (const auto& a : st.addresses) ids << a << std::endl;
}

inline void fill_predict_names(Result& res, const detail::TraceStructure& st)
{
    res.predicts.clear();
    for (std::size_t id : st.real_ids) { PredictStats p; p.address = st.addresses[id]; p.is_int = false; res.predicts.push_back(p); }
    for (std::size_t id : st.int_ids) { PredictStats p; p.address = st.addresses[id]; p.is_int = true; res.predicts.push_back(p); }
}

// ---- built-in models over several GPUs: cpprob_hip_group_* (one joint population, exact global resampling) -------------------
class Group {
public:
    explicit Group(const std::vector<int>& devices)
    {
        std::vector<std::int32_t> d(devices.begin(), devices.end());
        const int rc = cpprob_hip_group_create(d.data(), static_cast<std::int32_t>(d.size()), static_cast<std::int32_t>(d.size()), 0, nullptr, &h_);
        if (rc) throw std::runtime_error(std::string("cpprob_hip_group_create: ") + cpprob_hip_group_last_error(nullptr));
    }
    ~Group() { if (h_) cpprob_hip_group_destroy(h_); }
    Group(const Group&) = delete;
    Group& operator=(const Group&) = delete;
    cpprob_hip_group* get() const { return h_; }
    void check(int rc, const char* what) const
    {
        if (rc) throw std::runtime_error(std::string(what) + ": " + cpprob_hip_group_last_error(h_));
    }
private:
    cpprob_hip_group* h_ = nullptr;
};

inline void run_builtin_group(StateType algorithm, int model_id, const std::vector<double>& obs, std::size_t n, const detail::TraceStructure& st,
                              const Options& opt, Result& res, HostStore* store)
{
    const std::size_t world = opt.devices.size();
    Group grp(opt.devices);
    cpprob_hip_config cfg{};
    cfg.algorithm = algorithm == StateType::smc ? CPPROB_HIP_ALG_SMC : CPPROB_HIP_ALG_SIS;
    cfg.model = model_id;
    cfg.resampler = opt.resampler;
    cfg.resample_scope = CPPROB_HIP_SCOPE_EXCHANGE;
    cfg.keep_history = 1;
    cfg.ess_threshold = opt.ess_threshold;
    cfg.seed = opt.seed;
    cfg.n_particles = n; cfg.particle_offset = 0; cfg.n_global = n;
    grp.check(cpprob_hip_group_begin(grp.get(), &cfg, obs.data(), obs.size(), nullptr), "cpprob_hip_group_begin");
    grp.check(cpprob_hip_group_sync(grp.get()), "cpprob_hip_group_sync");   // (begin's buffer clears are allocation: not the run's time)
    const auto t0 = std::chrono::steady_clock::now();
    grp.check(cpprob_hip_group_run(grp.get(), 0), "cpprob_hip_group_run");
    cpprob_hip_summary s{};
    std::int32_t reruns = 0;
    // (sizes from the model structure: results() fills exactly n_predict * stats_per_predict doubles)
    const std::size_t K_guess = st.int_ids.empty() ? 2 : 3;
    const std::size_t T_guess = st.int_ids.empty() ? st.real_rows() : st.int_ids.size();
    std::vector<double> stats(T_guess * K_guess);
    grp.check(cpprob_hip_group_results(grp.get(), &s, stats.data(), stats.size(), &reruns), "cpprob_hip_group_results");
    res.run_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const std::size_t T = static_cast<std::size_t>(s.n_predict), K = static_cast<std::size_t>(s.stats_per_predict);
    if ((s.is_int ? st.int_ids.size() : st.real_rows()) != T || T * K != stats.size())
        throw std::runtime_error("built-in model kernel and the model function disagree on the number of predict statements");
    res.n_particles = n; res.log_evidence = s.log_evidence; res.ess = s.ess_final; res.log_norm = s.log_norm; res.n_resampled = s.n_resampled;
    res.used_builtin = true; res.n_gpus = static_cast<int>(world); res.exchange_reruns = reruns;
    fill_predict_names(res, st);
    if (s.is_int) {
        for (std::size_t t = 0; t < T; ++t) res.predicts[t].probabilities.assign(stats.begin() + t * K, stats.begin() + (t + 1) * K);
    } else {
        std::size_t row = 0;
        for (std::size_t k = 0; k < st.real_ids.size(); ++k) {
            PredictStats& p = res.predicts[k];
            for (std::size_t d = 0; d < st.real_width[k]; ++d, ++row) { p.mean_nd.push_back(stats[row * K]); p.variance_nd.push_back(stats[row * K + 1]); }
            p.mean = p.mean_nd[0]; p.variance = p.variance_nd[0];
        }
    }
    res.step_ess.assign(T, 0.0);
    cpprob_hip_ctx* c0 = cpprob_hip_group_context(grp.get(), 0);
    if (cpprob_hip_infer_step_trace(c0, res.step_ess.data(), nullptr)) throw std::runtime_error(std::string("cpprob_hip_infer_step_trace: ") + cpprob_hip_last_error(c0));
    if (store) {
        // the shards' traces side by side: particle i of the population lives on rank floor(i * world / n) (contiguous, equal shards)
        store->n = n;
        store->logw.resize(n);
        if (s.is_int) store->ints.resize(T * n); else store->real.resize(T * n);
        std::size_t begin = 0;
        for (std::size_t r = 0; r < world; ++r) {
            const std::size_t nr = n / world + (r < n % world ? 1 : 0);
            cpprob_hip_ctx* c = cpprob_hip_group_context(grp.get(), static_cast<std::int32_t>(r));
            auto chk = [&](int rc, const char* what) { if (rc) throw std::runtime_error(std::string(what) + ": " + cpprob_hip_last_error(c)); };
            chk(cpprob_hip_copy_logw(c, store->logw.data() + begin, nr * sizeof(double)), "cpprob_hip_copy_logw");
            if (s.is_int) {
                std::vector<std::int32_t> part(T * nr);
                chk(cpprob_hip_copy_paths(c, part.data(), part.size() * sizeof(std::int32_t)), "cpprob_hip_copy_paths");
                for (std::size_t t = 0; t < T; ++t) std::copy(part.begin() + t * nr, part.begin() + (t + 1) * nr, store->ints.begin() + t * n + begin);
            } else {
                std::vector<double> part(T * nr);
                chk(cpprob_hip_copy_paths(c, part.data(), part.size() * sizeof(double)), "cpprob_hip_copy_paths");
                for (std::size_t t = 0; t < T; ++t) std::copy(part.begin() + t * nr, part.begin() + (t + 1) * nr, store->real.begin() + t * n + begin);
            }
            begin += nr;
        }
    }
}

// ---- built-in models: the hand-fused kernels behind cpprob_hip_infer_* ---------------------------
inline void run_builtin(StateType algorithm, int model_id, const std::vector<double>& obs, std::size_t n, const detail::TraceStructure& st,
                        const Options& opt, Result& res, HostStore* store)
{
    const auto t_setup = std::chrono::steady_clock::now();
    ContextLease lease(opt.device);
    Context& ctx = *lease;
    cpprob_hip_config cfg{};
    cfg.algorithm = algorithm == StateType::smc ? CPPROB_HIP_ALG_SMC : CPPROB_HIP_ALG_SIS;
    cfg.model = model_id;
    cfg.resampler = opt.resampler;
    cfg.resample_scope = CPPROB_HIP_SCOPE_GLOBAL;
    cfg.keep_history = (opt.keep_history || algorithm != StateType::smc) ? 1 : 0;
    if (!cfg.keep_history && store) throw std::runtime_error("cpprob::inference: a filtering-only run (options().keep_history = false) keeps no traces to dump: set options().dump = false");
    cfg.ess_threshold = opt.ess_threshold;
    cfg.seed = opt.seed;
    cfg.n_particles = n; cfg.particle_offset = 0; cfg.n_global = n;
    ctx.check(cpprob_hip_infer_begin(ctx.get(), &cfg, obs.data(), obs.size()), "cpprob_hip_infer_begin");
    ctx.check(cpprob_hip_sync(ctx.get()), "cpprob_hip_sync");          // (begin's buffer clears are allocation: not the run's time)
    const auto t0 = std::chrono::steady_clock::now();
    res.setup_seconds = std::chrono::duration<double>(t0 - t_setup).count();      // (context, buffers, clears: what a call adds to its run)
    ctx.check(cpprob_hip_infer_run(ctx.get(), 0), "cpprob_hip_infer_run");
    // (everything the result holds in ONE read-back behind one stream synchronisation; sizes from the model structure: the engine
    //  fills exactly n_predict * stats_per_predict doubles -- histograms of up to 8 bins, or {mean, variance})
    cpprob_hip_summary s{};
    const std::size_t T_guess = st.int_ids.empty() ? st.real_rows() : st.int_ids.size();
    const std::size_t T_cap = std::max<std::size_t>(std::max(T_guess, obs.size()), 1);     // (the engine's rows: one per observation at most)
    std::vector<double> stats(T_cap * 8);
    res.step_ess.assign(T_cap, 0.0);
    ctx.check(cpprob_hip_infer_results(ctx.get(), &s, stats.data(), stats.size(), res.step_ess.data(), nullptr), "cpprob_hip_infer_results");
    res.run_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const std::size_t T = static_cast<std::size_t>(s.n_predict), K = static_cast<std::size_t>(s.stats_per_predict);
    if ((s.is_int ? st.int_ids.size() : st.real_rows()) != T || T != T_guess)
        throw std::runtime_error("built-in model kernel and the model function disagree on the number of predict statements");
    stats.resize(T * K); res.step_ess.resize(T);
    res.n_particles = n; res.log_evidence = s.log_evidence; res.ess = s.ess_final; res.log_norm = s.log_norm; res.n_resampled = s.n_resampled;
    res.used_builtin = true;
    fill_predict_names(res, st);
    if (s.is_int) {
        for (std::size_t t = 0; t < T; ++t) res.predicts[t].probabilities.assign(stats.begin() + t * K, stats.begin() + (t + 1) * K);
    } else {
        std::size_t row = 0;                                         // a vector-valued hit owns one engine row per component
        for (std::size_t k = 0; k < st.real_ids.size(); ++k) {
            PredictStats& p = res.predicts[k];
            for (std::size_t d = 0; d < st.real_width[k]; ++d, ++row) { p.mean_nd.push_back(stats[row * K]); p.variance_nd.push_back(stats[row * K + 1]); }
            p.mean = p.mean_nd[0]; p.variance = p.variance_nd[0];
        }
    }
    if (store) {
        store->n = n;
        store->logw.resize(n);
        ctx.check(cpprob_hip_copy_logw(ctx.get(), store->logw.data(), n * sizeof(double)), "cpprob_hip_copy_logw");
        if (s.is_int) { store->ints.resize(T * n); ctx.check(cpprob_hip_copy_paths(ctx.get(), store->ints.data(), T * n * sizeof(std::int32_t)), "cpprob_hip_copy_paths"); }
        else { store->real.resize(T * n); ctx.check(cpprob_hip_copy_paths(ctx.get(), store->real.data(), T * n * sizeof(double)), "cpprob_hip_copy_paths"); }
    }
    // ---- replicates (error bars): further seeds, up to three runs in flight on contexts of their own ----
    const int R = opt.replicates;
    if (R > 1) {
        const std::size_t H = res.predicts.size();
        res.n_replicates = R;
        res.replicate_values.assign(H, std::vector<double>(static_cast<std::size_t>(R), 0.0));
        std::vector<double> lz(static_cast<std::size_t>(R), 0.0);
        auto value_of = [&](const std::vector<double>& stv, std::size_t hit) {          // mean of component 0 / P(x = 0)
            if (s.is_int) return stv[hit * K];
            std::size_t row = 0;
            for (std::size_t k = 0; k < hit; ++k) row += st.real_width[k];
            return stv[row * K];
        };
        for (std::size_t h = 0; h < H; ++h) res.replicate_values[h][0] = value_of(stats, h);
        lz[0] = s.log_evidence;
        const int lanes = R - 1 < 3 ? R - 1 : 3;
        std::vector<std::unique_ptr<Context>> extra;
        for (int l = 0; l < lanes; ++l) {
            extra.emplace_back(new Context(opt.device));
            extra.back()->check(cpprob_hip_infer_begin(extra.back()->get(), &cfg, obs.data(), obs.size()), "cpprob_hip_infer_begin");
        }
        std::vector<int> pending(static_cast<std::size_t>(lanes), -1);
        auto harvest = [&](int l) {
            const int r = pending[static_cast<std::size_t>(l)];
            if (r < 0) return;
            cpprob_hip_summary sr{};
            std::vector<double> str(T * K);
            extra[l]->check(cpprob_hip_infer_summary(extra[l]->get(), &sr), "cpprob_hip_infer_summary");
            extra[l]->check(cpprob_hip_infer_stats(extra[l]->get(), str.data(), str.size()), "cpprob_hip_infer_stats");
            lz[static_cast<std::size_t>(r)] = sr.log_evidence;
            for (std::size_t h = 0; h < H; ++h) res.replicate_values[h][static_cast<std::size_t>(r)] = value_of(str, h);
            pending[static_cast<std::size_t>(l)] = -1;
        };
        const auto tr0 = std::chrono::steady_clock::now();
        for (int r = 1; r < R; ++r) {
            const int l = (r - 1) % lanes;
            harvest(l);                                               // synchronises that context only; the others keep running
            extra[l]->check(cpprob_hip_infer_run(extra[l]->get(), static_cast<std::uint64_t>(r)), "cpprob_hip_infer_run");
            pending[static_cast<std::size_t>(l)] = r;
        }
        for (int l = 0; l < lanes; ++l) harvest(l);
        res.replicates_seconds = res.run_seconds + std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count();
        res.predict_mean.assign(H, 0.0); res.predict_sd.assign(H, 0.0);
        for (std::size_t h = 0; h < H; ++h) {
            double m = 0, v = 0;
            for (double x : res.replicate_values[h]) m += x;
            m /= R;
            for (double x : res.replicate_values[h]) v += (x - m) * (x - m);
            res.predict_mean[h] = m; res.predict_sd[h] = std::sqrt(v / (R - 1));
        }
        double mx = lz[0], acc = 0, ml = 0, vl = 0;
        for (double x : lz) { mx = std::max(mx, x); ml += x; }
        for (double x : lz) acc += std::exp(x - mx);
        ml /= R;
        for (double x : lz) vl += (x - ml) * (x - ml);
        res.log_evidence_mean = mx + std::log(acc / R);
        res.log_evidence_sd = std::sqrt(vl / (R - 1));
    }
    lease.done();                                                     // (the context goes back to the pool)
}

// ---- unchanged models over several GPUs ----------------------------------------------------------------------------------------
// Importance sampling needs no communication until the shards' sums meet: every device runs the model body for its
// contiguous block of particles -- global particle ids select the random streams, so the traces are those ONE device would have
// drawn -- on a host thread of its own, and the shards' self-normalised numbers are combined by their evidence:
//   w_r = exp(L_r - L), L = logsumexp_r L_r;  mean = sum w_r mean_r;  E[x^2] = sum w_r (var_r + mean_r^2);  P = sum w_r P_r;
//   ESS = 1 / sum_r w_r^2 / ESS_r;  log evidence = L - log N.
// StateType::smc: every shard is an ISLAND -- an independent SMC run of its own particles, resampled among themselves -- and the
// islands are combined the same way with L_r = log(n_r Z_r), Z_r the island's evidence estimate: a consistent estimator of the same
// posterior, but not the joint population's resampling (that needs the replayed traces to migrate: not built; the built-in models
// have it, cpprob_hip_group_*).
inline void combine_shards(std::vector<Result>& rr, const std::vector<HostStore>* hs, const std::vector<std::size_t>& begin, std::size_t n,
                           const detail::TraceStructure& st, bool islands, Result& res, HostStore* store);
inline void run_generic_sharded(StateType algorithm, const Entry& e, const void* observes_v, std::size_t n, const detail::TraceStructure& st, const Options& opt,
                                Result& res, HostStore* store)
{
    const bool smc = algorithm == StateType::smc;
    const std::size_t world = opt.devices.size();
    std::vector<Result> rr(world);
    std::vector<HostStore> hs(world);
    std::vector<std::string> errs(world);
    std::vector<std::size_t> begin(world + 1, 0);
    for (std::size_t r = 0; r < world; ++r) begin[r + 1] = begin[r] + n / world + (r < n % world ? 1 : 0);
    std::vector<std::thread> th;
    for (std::size_t r = 0; r < world; ++r)
        th.emplace_back([&, r] {
            try {
                Options o = opt;
                o.device = opt.devices[r]; o.devices.clear(); o.particle_offset = begin[r]; o.dump = false;
                e.generic(algorithm, observes_v, begin[r + 1] - begin[r], st, o, rr[r], store ? &hs[r] : nullptr);
            } catch (const std::exception& ex) { errs[r] = ex.what(); }
        });
    for (auto& t : th) t.join();
    for (std::size_t r = 0; r < world; ++r)
        if (!errs[r].empty()) throw std::runtime_error("cpprob::inference (shard " + std::to_string(r) + "): " + errs[r]);
    combine_shards(rr, store ? &hs : nullptr, begin, n, st, smc, res, store);
    if (smc && store) {
        // an island's log-weights are relative to ITS last resampling: on the population's common scale island r's particles carry
        // log(n_r Z_r) - logsumexp(its weights) more -- what the combined statistics above weigh it by, so that the files say what Result says
        for (std::size_t r = 0; r < world; ++r) {
            double mx = -std::numeric_limits<double>::infinity(), acc = 0;
            for (double v : hs[r].logw) mx = std::max(mx, v);
            for (double v : hs[r].logw) acc += std::exp(v - mx);
            const double shift = rr[r].log_norm - (mx + std::log(acc));
            for (std::size_t i = begin[r]; i < begin[r + 1]; ++i) store->logw[i] += shift;
        }
    }
}

// The shards' self-normalised numbers combined by their masses (log_norm = log of the shard's weight sum on the population's common
// scale): w_r = exp(L_r - L), L = logsumexp_r L_r;  mean = sum w_r mean_r;  E[x^2] = sum w_r (var_r + mean_r^2);  P = sum w_r P_r;
// ESS = 1 / sum_r w_r^2 / ESS_r.  islands: the shards are independent SMC runs, L_r = log(n_r Z_r) and the evidence is the combination's;
// otherwise (SIS shards; the shards of a joint SMC population, whose evidence the caller holds) the shards' weights already share a scale.
inline void combine_shards(std::vector<Result>& rr, const std::vector<HostStore>* hs, const std::vector<std::size_t>& begin, std::size_t n,
                           const detail::TraceStructure& st, bool islands, Result& res, HostStore* store)
{
    const std::size_t world = rr.size();
    const bool smc = islands;
    // (an island's mass: its particles times its evidence estimate; an SIS shard's: the sum of its weights -- the same thing)
    if (smc)
        for (std::size_t r = 0; r < world; ++r) rr[r].log_norm = rr[r].log_evidence + std::log(static_cast<double>(begin[r + 1] - begin[r]));
    double L = -std::numeric_limits<double>::infinity();
    for (const auto& x : rr) L = std::max(L, x.log_norm);
    double acc = 0;
    for (const auto& x : rr) acc += std::exp(x.log_norm - L);
    L += std::log(acc);
    res = rr[0];
    if (smc) { res.n_resampled = 0; for (const auto& x : rr) res.n_resampled = std::max(res.n_resampled, x.n_resampled); res.step_ess.clear(); }
    res.n_particles = n; res.log_norm = L; res.log_evidence = L - std::log(static_cast<double>(n)); res.n_gpus = static_cast<int>(world);
    double inv_ess = 0, secs = 0;
    for (const auto& x : rr) { const double w = std::exp(x.log_norm - L); inv_ess += w * w / x.ess; secs = std::max(secs, x.run_seconds); }
    res.ess = 1.0 / inv_ess; res.run_seconds = secs;
    for (std::size_t k = 0; k < res.predicts.size(); ++k) {
        PredictStats& p = res.predicts[k];
        if (p.is_int) {
            std::size_t top = 0;
            for (const auto& x : rr) top = std::max(top, x.predicts[k].probabilities.size());
            p.probabilities.assign(top, 0.0);
            for (const auto& x : rr) { const double w = std::exp(x.log_norm - L); for (std::size_t s2 = 0; s2 < x.predicts[k].probabilities.size(); ++s2) p.probabilities[s2] += w * x.predicts[k].probabilities[s2]; }
            while (p.probabilities.size() > 1 && p.probabilities.back() == 0.0) p.probabilities.pop_back();
        } else {
            const std::size_t D = p.mean_nd.size();
            std::vector<double> m1(D, 0.0), m2(D, 0.0);
            for (const auto& x : rr) {
                const double w = std::exp(x.log_norm - L);
                for (std::size_t d = 0; d < D; ++d) { const double m = x.predicts[k].mean_nd[d]; m1[d] += w * m; m2[d] += w * (x.predicts[k].variance_nd[d] + m * m); }
            }
            for (std::size_t d = 0; d < D; ++d) { p.mean_nd[d] = m1[d]; p.variance_nd[d] = m2[d] - m1[d] * m1[d]; }
            p.mean = p.mean_nd[0]; p.variance = p.variance_nd[0];
        }
    }
    if (store && hs) {
        // the shards' traces side by side, in global particle order
        const std::size_t n_real = st.real_rows(), n_int = st.int_ids.size();
        store->n = n; store->logw.resize(n); store->real.resize(n_real * n); store->ints.resize(n_int * n);
        for (std::size_t r = 0; r < world; ++r) {
            const std::size_t nr = begin[r + 1] - begin[r];
            std::copy((*hs)[r].logw.begin(), (*hs)[r].logw.end(), store->logw.begin() + begin[r]);
            for (std::size_t row = 0; row < n_real; ++row) std::copy((*hs)[r].real.begin() + row * nr, (*hs)[r].real.begin() + (row + 1) * nr, store->real.begin() + row * n + begin[r]);
            for (std::size_t row = 0; row < n_int; ++row) std::copy((*hs)[r].ints.begin() + row * nr, (*hs)[r].ints.begin() + (row + 1) * nr, store->ints.begin() + row * n + begin[r]);
        }
    }
}

// ---- Markov probe (cpprob/detail/host_trace.hpp: ProbeState): the smallest window of past samples a step depends on, or -1 ------
template <class Func, class ObsTuple>
int probe_markov_window(const Func& f, const ObsTuple& obs, const detail::TraceStructure& st)
{
    const std::size_t T = st.n_observe;
    if (T < 2 || st.vector_statements || st.samples_before_observe.size() != T || st.n_sample == 0) return -1;
    auto run = [&](const detail::ProbeState& cfg) -> bool {
        detail::ProbeState& p = detail::probe();
        p = cfg; p.active = true; p.failed = false; p.ordinal = 0; p.n_obs = 0; p.log.clear();
        // (whatever the model throws on substituted values -- its own checks, a distribution's parameter check -- means "this model
        //  does look at old samples": not Markov, full replay; never an error of a valid inference)
        try { call_f_tuple(f, obs); }
        catch (...) { detail::probe().active = false; return false; }
        p.active = false;
        return !p.failed;
    };
    detail::BoundProbe& bp = detail::bound_probe();
    bp.expected = &st.observe_bound; bp.varies = false;
    struct BoundGuard { detail::BoundProbe& b; ~BoundGuard() { b.expected = nullptr; } } guard{bp};
    const int windows[] = {1, 2, 4, 8};
    for (int w : windows) {
        bool ok = true;
        for (std::uint32_t rep = 0; rep < 8 && ok; ++rep) {
            detail::ProbeState a;
            a.base_seed = 1000003u * (rep + 1); a.n_steps = T; a.record_all = true; a.ordinal_cap = 64 * st.n_sample + 1024;
            if (!run(a)) return -1;
            const std::vector<std::vector<double>> ref = detail::probe().log;
            const std::vector<double> values = detail::probe().values;
            if (detail::probe().ordinal != st.n_sample || detail::probe().n_obs != T) return -1;      // sample / observe counts depend on sampled values
            for (std::size_t step = 1; step < T && ok; ++step) {
                const std::size_t fresh_lo = st.samples_before_observe[step - 1];
                if (fresh_lo <= static_cast<std::size_t>(w)) continue;                                // nothing older than the window yet
                detail::ProbeState b = a;
                b.record_all = false; b.step = step; b.dummy_below = fresh_lo - static_cast<std::size_t>(w); b.replay_below = fresh_lo; b.values = values;
                if (!run(b)) { ok = false; break; }
                const auto& lg = detail::probe().log;
                if (detail::probe().n_obs != T || lg.size() <= step || ref.size() <= step || lg[step] != ref[step]) ok = false;
            }
        }
        if (ok) return w;
    }
    return -1;
}

// ---- structural dry run on the host (one trace): statement counts, predict types and addresses -------------------------------
template <class Func, class ObsTuple>
void dry_run(StateType algorithm, const Func& f, const ObsTuple& obs, detail::TraceStructure& st)
{
    const StateType saved = algorithm;
    State::set(StateType::dryrun);
    detail::recorder() = &st;
    try { call_f_tuple(f, obs); } catch (...) { detail::recorder() = nullptr; State::set(saved); throw; }
    detail::recorder() = nullptr;
    State::set(saved);
}

// ---- the body of cpprob::inference -------------------------------------------------------------------
template <class Func, class... Args>
void run_inference(StateType algorithm, const Func& f, const std::tuple<Args...>& observes, std::size_t n, const std::string& file)
{
    using ObsTuple = tuple_observes_t<Func>;
    static_assert(std::tuple_size<ObsTuple>::value == sizeof...(Args), "the observes tuple must have one element per model argument");
    const ObsTuple obs(observes);                                   // implicit conversions, as call_f_tuple's forwarding does

    // structural dry run on the host (one trace): statement counts, predict types and addresses
    detail::TraceStructure st;
    dry_run(algorithm, f, obs, st);
    if (st.n_observe == 0) throw std::runtime_error("cpprob::inference: the model executes no observe statement");
    if (algorithm == StateType::smc && options().markov_probe) {
        st.window = probe_markov_window(f, obs, st);
        bool known = st.observe_bound.size() == st.n_observe;
        for (double b : st.observe_bound) if (!(b == b) || b == std::numeric_limits<double>::infinity() || b == -std::numeric_limits<double>::infinity()) known = false;
        st.bounds_fixed = st.window >= 0 && known && !detail::bound_probe().varies;
    }
    if (st.n_other_predicts) throw std::runtime_error("cpprob::inference: non-scalar predicts (.any file) are not supported by the device engine");

    const Key key = key_of(f, std::integral_constant<bool, detail::fn_traits<std::remove_cv_t<std::remove_reference_t<Func>>>::is_function>{});
    const Entry* e = find_entry(key);
    if (!e) throw std::runtime_error("cpprob::inference: this model has no device code: compile its source with hipcc and add "
                                     "CPPROB_REGISTER_MODEL(<model>) (or CPPROB_REGISTER_BUILTIN) -- there is no CPU fallback");
    if (st.vector_statements && e->builtin_model < 0 && !e->generic_vectors)
        throw std::runtime_error("cpprob::inference: vector-valued statements (multivariate_normal_distribution / NDArray) need the model's device "
                                 "view (CPPROB_REGISTER_MODEL_VIEW, cpprob/device_view_begin.hpp) or a built-in kernel: std::vector cannot live in device code");
    const Options& opt = options();
    Result& res = last_result();
    res = Result();
    HostStore hs;
    HostStore* store = opt.dump ? &hs : nullptr;
    if (opt.devices.size() > 1) {
        const bool builtin = e->builtin_model >= 0 && (opt.prefer_builtin || !e->generic);
        if (builtin) run_builtin_group(algorithm, e->builtin_model, flatten(obs), n, st, opt, res, store);
        else if (e->generic) {
            // smc: ONE joint population where the model has a joint form (a replay window, systematic resampling: cpprob/gpu.hpp,
            // generic_joint_launcher); otherwise islands -- a different estimator, reported as such (Result::joint)
            bool joint = false;
            if (algorithm == StateType::smc && e->generic_joint && !opt.islands) joint = e->generic_joint(algorithm, &obs, n, st, opt, res, store);
            if (!joint) run_generic_sharded(algorithm, *e, &obs, n, st, opt, res, store);
        }
        else throw std::runtime_error("cpprob::inference: registry entry without a launcher");
    }
    else if (e->builtin_model >= 0 && (opt.prefer_builtin || !e->generic || (st.vector_statements && !e->generic_vectors)))
        run_builtin(algorithm, e->builtin_model, flatten(obs), n, st, opt, res, store);
    else if (e->generic) e->generic(algorithm, &obs, n, st, opt, res, store);
    else throw std::runtime_error("cpprob::inference: registry entry without a launcher");
    if (opt.dump) dump_posterior(file, st, hs, opt.dump_max_particles);      // finish_trace() x n + finish_infer()
}

// ---- posterior files of a batch: problem b's traces as <prefix>_<b>.int / .ids --------------------------------------------------
// One cpprob_hip_batch_paths call resolves every problem's first m_b = min(n_b, max_particles) lineages on the device; problem b's
// share of the packed result fills a HostStore and goes through dump_posterior with structure(b)'s addresses.  T[b], n[b]: the
// lengths and particle counts of the batch last run on ctx.  A problem without observes writes no .int file.
template <class Structure>
void dump_batch_posterior(Context& ctx, const std::string& prefix, const std::vector<std::uint32_t>& T, const std::vector<std::uint32_t>& n,
                          std::size_t max_particles, const Structure& structure)
{
    const std::size_t B = T.size();
    std::vector<std::uint64_t> first(B + 1), wfirst(B + 1);
    if (cpprob_hip_batch_paths_layout(T.data(), n.data(), B, max_particles, first.data(), wfirst.data()))
        throw std::runtime_error(std::string("cpprob_hip_batch_paths_layout: ") + cpprob_hip_last_error(nullptr));
    std::vector<std::int32_t> paths(static_cast<std::size_t>(first[B]));
    std::vector<double> logw(static_cast<std::size_t>(wfirst[B]));
    ctx.check(cpprob_hip_batch_paths(ctx.get(), max_particles, paths.data(), paths.size(), logw.data(), logw.size()), "cpprob_hip_batch_paths");
    for (std::size_t b = 0; b < B; ++b) {
        const std::size_t m = (max_particles && max_particles < n[b]) ? max_particles : n[b];
        HostStore hs;
        hs.n = T[b] ? m : 0;
        hs.ints.assign(paths.begin() + static_cast<std::ptrdiff_t>(first[b]), paths.begin() + static_cast<std::ptrdiff_t>(first[b + 1]));
        hs.logw.assign(logw.begin() + static_cast<std::ptrdiff_t>(wfirst[b]), logw.begin() + static_cast<std::ptrdiff_t>(wfirst[b + 1]));
        dump_posterior(prefix + "_" + std::to_string(b), structure(b), hs, 0);
    }
}

// ---- backward smoothing of a batch (cpprob_hip_batch_smooth): Options::backward_smoothing, ::backward_trajectories ----------------
// The statistics of the batch last run on ctx -- [B][T_max][K], the layout of cpprob_hip_batch_results' h_stats -- replaced by the
// backward smoother's marginals.
inline void batch_backward_marginals(Context& ctx, std::vector<double>& stats)
{
    ctx.check(cpprob_hip_batch_smooth(ctx.get(), 0, 0, stats.data(), stats.size(), nullptr, 0), "cpprob_hip_batch_smooth");
}

// Options::smoothing_lag: the fixed-lag marginals of the steps from[b] on (nullptr: every problem from step 0) of the batch last run
// or advanced on ctx, [B][n_rows][K] (cpprob_hip_batch_smooth_lag).
inline void batch_lag_marginals(Context& ctx, std::size_t lag, const std::uint32_t* from, std::size_t n_rows, std::vector<double>& rows)
{
    if (rows.empty()) return;
    ctx.check(cpprob_hip_batch_smooth_lag(ctx.get(), lag, from, n_rows, 0, 0, rows.data(), rows.size(), nullptr, 0), "cpprob_hip_batch_smooth_lag");
}

// dump_batch_posterior with problem b's M backward-simulated trajectories (draw_index 0) in the lineages' place: equal weights.
template <class Structure>
void dump_batch_backward(Context& ctx, const std::string& prefix, const std::vector<std::uint32_t>& T, std::size_t M, const Structure& structure)
{
    const std::size_t B = T.size();
    std::vector<std::uint64_t> first(B + 1);
    if (cpprob_hip_batch_smooth_layout(T.data(), B, M, first.data()))
        throw std::runtime_error(std::string("cpprob_hip_batch_smooth_layout: ") + cpprob_hip_last_error(nullptr));
    std::vector<std::int32_t> traj(static_cast<std::size_t>(first[B]));
    ctx.check(cpprob_hip_batch_smooth(ctx.get(), M, 0, nullptr, 0, traj.data(), traj.size()), "cpprob_hip_batch_smooth");
    for (std::size_t b = 0; b < B; ++b) {
        HostStore hs;
        hs.n = T[b] ? M : 0;
        hs.ints.assign(traj.begin() + static_cast<std::ptrdiff_t>(first[b]), traj.begin() + static_cast<std::ptrdiff_t>(first[b + 1]));
        hs.logw.assign(hs.n, 0.0);
        dump_posterior(prefix + "_" + std::to_string(b), structure(b), hs, 0);
    }
}

// ---- forecasts of a batch (cpprob_hip_batch_forecast): Options::forecast_horizon, ::forecast_trajectories -----------------------------
// What the C ABI would refuse, refused before a batch is begun.  stored: the batch keeps its history or its masses.
inline void check_forecast_options(const std::string& who, std::size_t H, std::size_t M, bool stored)
{
    if (M && !H) throw std::runtime_error(who + ": options().forecast_trajectories simulates the steps of a forecast: set options().forecast_horizon");
    if (!H) return;
    if (H >= (std::size_t(1) << 24)) throw std::runtime_error(who + ": options().forecast_horizon must lie below 2^24");
    if (M > (std::size_t(1) << 20)) throw std::runtime_error(who + ": options().forecast_trajectories must lie in 0 .. 2^20");
    if (!stored)
        throw std::runtime_error(who + ": a forecast reads the smoother's masses: a filtering-only run (options().keep_history = false) keeps none without options().keep_masses");
}

// The forecast of the batch last run or advanced on ctx into its results: H rows of the first k of K states, M futures a problem.
inline void batch_forecast_results(Context& ctx, std::size_t H, std::size_t M, std::size_t K, std::size_t k, std::vector<Result>& out)
{
    if (!H) return;
    const std::size_t B = out.size();
    std::vector<double> marg(B * H * K);
    std::vector<std::int32_t> traj(B * (H + 1) * M);
    ctx.check(cpprob_hip_batch_forecast(ctx.get(), H, M, 0, marg.data(), marg.size(), M ? traj.data() : nullptr, traj.size()), "cpprob_hip_batch_forecast");
    for (std::size_t b = 0; b < B; ++b) {
        Result& r = out[b];
        r.forecast.resize(H);
        for (std::size_t h = 0; h < H; ++h)
            r.forecast[h].assign(marg.begin() + static_cast<std::ptrdiff_t>((b * H + h) * K), marg.begin() + static_cast<std::ptrdiff_t>((b * H + h) * K + k));
        r.forecast_trajectories.assign(M, std::vector<std::int32_t>(H + 1));
        for (std::size_t h = 0; h <= H; ++h)
            for (std::size_t j = 0; j < M; ++j) r.forecast_trajectories[j][h] = traj[(b * (H + 1) + h) * M + j];
    }
}

// ---- trajectory sufficient statistics of a batch (cpprob_hip_batch_traj_stats): Options::trajectory_stats, ::trajectory_stats_draw_index ----
// What the C ABI would refuse, refused before a batch is begun.  stored: the batch keeps its history or its masses.
inline void check_trajectory_stats_options(const std::string& who, std::size_t M, std::uint64_t draw_index, bool stored)
{
    if (!M) return;
    if (M > (std::size_t(1) << 20)) throw std::runtime_error(who + ": options().trajectory_stats must lie in 0 .. 2^20");
    if (draw_index >= (std::uint64_t(1) << 16)) throw std::runtime_error(who + ": options().trajectory_stats_draw_index must lie below 2^16");
    if (!stored)
        throw std::runtime_error(who + ": options().trajectory_stats reads the smoother's masses: a filtering-only run (options().keep_history = false) keeps none without options().keep_masses");
}

// The records of M trajectories a problem of the batch last run or advanced on ctx into its results; observes: the problems'
// sequences packed by the lengths reached.
inline void batch_trajectory_stats_results(Context& ctx, std::size_t M, std::uint64_t draw_index, const std::vector<double>& observes, std::vector<Result>& out)
{
    if (!M) return;
    const std::size_t B = out.size(), R = 88;
    std::vector<double> rec(B * M * R);
    ctx.check(cpprob_hip_batch_traj_stats(ctx.get(), M, draw_index, observes.empty() ? nullptr : observes.data(), observes.size(), rec.data(), rec.size()),
              "cpprob_hip_batch_traj_stats");
    for (std::size_t b = 0; b < B; ++b) {
        out[b].trajectory_stats.resize(M);
        for (std::size_t j = 0; j < M; ++j)
            out[b].trajectory_stats[j].assign(rec.begin() + static_cast<std::ptrdiff_t>((b * M + j) * R), rec.begin() + static_cast<std::ptrdiff_t>((b * M + j + 1) * R));
    }
}

// ---- decoding a batch (cpprob_hip_batch_decode, _decode_lag): Options::map_decode, ::decode_lag ---------------------------------------
// What the C ABI would refuse, refused before a batch is begun.  stored: the batch keeps its history or its masses.
inline void check_decode_options(const std::string& who, bool decode, long lag, bool stored)
{
    if (!decode) {
        if (lag >= 0) throw std::runtime_error(who + ": options().decode_lag delays a decode: set options().map_decode");
        return;
    }
    if (lag > (1l << 24)) throw std::runtime_error(who + ": options().decode_lag must lie in 0 .. 2^24");
    if (!stored)
        throw std::runtime_error(who + ": decoding reads the smoother's masses: a filtering-only run (options().keep_history = false) keeps none without options().keep_masses");
}

// The decode of the batch last run or advanced on ctx into its results (L: the lengths reached): Result::map_path the most probable
// state path, or (lag >= 0) the fixed-lag rows from step 0 on, and Result::map_score.
inline void batch_decode_results(Context& ctx, bool decode, long lag, const std::vector<std::uint32_t>& L, std::vector<Result>& out)
{
    if (!decode) return;
    const std::size_t B = out.size();
    std::vector<double> score(B);
    std::size_t total = 0, n_rows = 0;
    for (std::size_t b = 0; b < B; ++b) { total += L[b]; n_rows = std::max<std::size_t>(n_rows, L[b]); }
    if (lag < 0) {
        std::vector<std::int32_t> path(total);
        ctx.check(cpprob_hip_batch_decode(ctx.get(), total ? path.data() : nullptr, path.size(), score.data(), score.size()), "cpprob_hip_batch_decode");
        std::size_t at = 0;
        for (std::size_t b = 0; b < B; ++b) {
            out[b].map_path.assign(path.begin() + static_cast<std::ptrdiff_t>(at), path.begin() + static_cast<std::ptrdiff_t>(at + L[b]));
            at += L[b];
        }
    } else {
        std::vector<std::int32_t> st(B * n_rows);
        ctx.check(cpprob_hip_batch_decode_lag(ctx.get(), static_cast<std::uint64_t>(lag), nullptr, n_rows, n_rows ? st.data() : nullptr, st.size(), score.data(), score.size()),
                  "cpprob_hip_batch_decode_lag");
        for (std::size_t b = 0; b < B; ++b)
            out[b].map_path.assign(st.begin() + static_cast<std::ptrdiff_t>(b * n_rows), st.begin() + static_cast<std::ptrdiff_t>(b * n_rows + L[b]));
    }
    for (std::size_t b = 0; b < B; ++b) { out[b].map_decoded = true; out[b].map_score = score[b]; }
}

// The trace structure of a table-HMM problem of T observes: one int predict per observe, "state[t]".
inline detail::TraceStructure hmm_table_structure(std::size_t T)
{
    detail::TraceStructure st;
    for (std::size_t t = 0; t < T; ++t) st.int_ids.push_back(st.id_of("state[" + std::to_string(t) + "]"));
    return st;
}

// ---- many problems of one model in ONE launch (cpprob_hip_batch_*): models bound by CPPROB_REGISTER_BUILTIN to the table-weight HMMs ----
// observes[b] is problem b's observes tuple (all of one length), seeds[b] its Philox key: result b is what cpprob::inference with
// options().seed = seeds[b] computes (posterior files: options().batch_dump_file, problem b's as <batch_dump_file>_<b>.int / .ids).  Resampler, keep_history (false: filtering statistics), ess_threshold (must
// be > 1: every step) and device come from options(), as for cpprob::inference.
template <class Func, class... Args>
std::vector<Result> inference_batch(StateType algorithm, const Func& f, const std::vector<std::tuple<Args...>>& observes, std::size_t n,
                                    const std::vector<std::uint64_t>& seeds)
{
    using ObsTuple = tuple_observes_t<Func>;
    static_assert(std::tuple_size<ObsTuple>::value == sizeof...(Args), "the observes tuple must have one element per model argument");
    if (algorithm != StateType::smc)
        throw std::runtime_error("cpprob::gpu::inference_batch: batched runs are StateType::smc only -- run SIS with cpprob::inference");
    if (observes.empty()) throw std::runtime_error("cpprob::gpu::inference_batch: no problems");
    if (seeds.size() != observes.size()) throw std::runtime_error("cpprob::gpu::inference_batch: one seed per problem");
    const ObsTuple obs0(observes[0]);
    detail::TraceStructure st;
    dry_run(algorithm, f, obs0, st);
    const Key key = key_of(f, std::integral_constant<bool, detail::fn_traits<std::remove_cv_t<std::remove_reference_t<Func>>>::is_function>{});
    const Entry* e = find_entry(key);
    if (!e || (e->builtin_model != CPPROB_HIP_MODEL_HMM3 && e->builtin_model != CPPROB_HIP_MODEL_HMM_TABLE))
        throw std::runtime_error("cpprob::gpu::inference_batch: batched runs need a model bound by CPPROB_REGISTER_BUILTIN to CPPROB_HIP_MODEL_HMM3 or "
                                 "CPPROB_HIP_MODEL_HMM_TABLE -- run this model one problem at a time with cpprob::inference");
    std::vector<double> flat;
    std::size_t T = 0;
    for (std::size_t b = 0; b < observes.size(); ++b) {
        const std::vector<double> o = flatten(ObsTuple(observes[b]));
        if (b == 0) T = o.size();
        else if (o.size() != T) throw std::runtime_error("cpprob::gpu::inference_batch: every problem needs the same number of observes");
        flat.insert(flat.end(), o.begin(), o.end());
    }
    if (st.int_ids.size() != T) throw std::runtime_error("built-in model kernel and the model function disagree on the number of predict statements");
    const Options& opt = options();
    const bool masses = !opt.keep_history && opt.keep_masses;      // (a filtering-only batch that keeps the smoother's masses)
    if (!opt.keep_history && !opt.batch_dump_file.empty() && !(masses && opt.backward_trajectories))
        throw std::runtime_error("cpprob::gpu::inference_batch: a filtering-only run (options().keep_history = false) keeps no traces to dump: clear options().batch_dump_file");
    if (!opt.keep_history && !masses && opt.backward_smoothing)
        throw std::runtime_error("cpprob::gpu::inference_batch: backward smoothing reads the particle store: a filtering-only run (options().keep_history = false) keeps none");
    if (!opt.keep_history && !masses && opt.smoothing_lag >= 0)
        throw std::runtime_error("cpprob::gpu::inference_batch: fixed-lag smoothing reads the particle store: a filtering-only run (options().keep_history = false) keeps none");
    check_forecast_options("cpprob::gpu::inference_batch", opt.forecast_horizon, opt.forecast_trajectories, opt.keep_history || masses);
    check_decode_options("cpprob::gpu::inference_batch", opt.map_decode, opt.decode_lag, opt.keep_history || masses);
    check_trajectory_stats_options("cpprob::gpu::inference_batch", opt.trajectory_stats, opt.trajectory_stats_draw_index, opt.keep_history || masses);
    ContextLease lease(opt.device);
    Context& ctx = *lease;
    cpprob_hip_batch_config bc{};
    bc.algorithm = CPPROB_HIP_ALG_SMC;
    bc.model = e->builtin_model;
    bc.resampler = opt.resampler;
    bc.keep_history = opt.keep_history ? 1 : 0;
    bc.flags = masses ? CPPROB_HIP_BATCH_KEEP_MASSES : 0;
    bc.ess_threshold = opt.ess_threshold;
    bc.n_particles = n;
    bc.n_problems = observes.size();
    const std::size_t B = observes.size();
    const auto t0 = std::chrono::steady_clock::now();
    ctx.check(cpprob_hip_batch_begin(ctx.get(), &bc, flat.data(), T), "cpprob_hip_batch_begin");
    ctx.check(cpprob_hip_batch_run(ctx.get(), seeds.data()), "cpprob_hip_batch_run");
    std::vector<cpprob_hip_summary> sums(B);
    const std::size_t K = e->builtin_model == CPPROB_HIP_MODEL_HMM3 ? 3 : 8;
    std::vector<double> stats(B * T * K), ess(B * T);
    ctx.check(cpprob_hip_batch_results(ctx.get(), sums.data(), stats.data(), stats.size(), ess.data(), nullptr), "cpprob_hip_batch_results");
    if (opt.smoothing_lag >= 0) batch_lag_marginals(ctx, static_cast<std::size_t>(opt.smoothing_lag), nullptr, T, stats);
    else if (opt.backward_smoothing) batch_backward_marginals(ctx, stats);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!opt.batch_dump_file.empty() && opt.backward_trajectories)
        dump_batch_backward(ctx, opt.batch_dump_file, std::vector<std::uint32_t>(B, static_cast<std::uint32_t>(T)), opt.backward_trajectories,
                            [&st](std::size_t) -> const detail::TraceStructure& { return st; });
    else if (!opt.batch_dump_file.empty())
        dump_batch_posterior(ctx, opt.batch_dump_file, std::vector<std::uint32_t>(B, static_cast<std::uint32_t>(T)), std::vector<std::uint32_t>(B, static_cast<std::uint32_t>(n)),
                             opt.dump_max_particles, [&st](std::size_t) -> const detail::TraceStructure& { return st; });
    std::vector<Result> out(B);
    batch_forecast_results(ctx, opt.forecast_horizon, opt.forecast_trajectories, K, K, out);
    batch_decode_results(ctx, opt.map_decode, opt.decode_lag, std::vector<std::uint32_t>(B, static_cast<std::uint32_t>(T)), out);
    batch_trajectory_stats_results(ctx, opt.trajectory_stats, opt.trajectory_stats_draw_index, flat, out);
    lease.done();
    for (std::size_t b = 0; b < B; ++b) {
        Result& r = out[b];
        const cpprob_hip_summary& s = sums[b];
        r.n_particles = n; r.log_evidence = s.log_evidence; r.ess = s.ess_final; r.log_norm = s.log_norm; r.n_resampled = s.n_resampled;
        r.used_builtin = true; r.step_form = s.step_form; r.run_seconds = seconds;
        fill_predict_names(r, st);
        for (std::size_t t = 0; t < T; ++t) r.predicts[t].probabilities.assign(stats.begin() + (b * T + t) * K, stats.begin() + (b * T + t + 1) * K);
        r.step_ess.assign(ess.begin() + b * T, ess.begin() + (b + 1) * T);
    }
    return out;
}

// ---- one table-weight HMM under many parameter settings, ragged sequences, per-problem particle counts (cpprob_hip_batch_begin_problems) ----
// Problem b is CPPROB_HIP_MODEL_HMM_TABLE with tables[b] (k = means.size() states, the same k for all; transition row-major k x k, rows
// of weights), observes[b] (any length >= 1), n[b] particles and Philox key seeds[b]; result b is what a one-problem run with that
// table computes: log_evidence, ess, one predict per observe ("state[t]": P(x_t = s), s < k) and the per-step ESS.  tables, observes
// and n of size 1 are shared by all problems; the number of problems is seeds.size().  Resampler, keep_history (false: filtering
// statistics), ess_threshold (must be > 1: every step) and device come from options(), as for inference_batch.
// sigmas: empty (the emission of state s is N(means[s], 1)) or k per-state emission scales (N(means[s], sigmas[s]); include/cpprob_hip.h:
// cpprob_hip_batch_begin_problems_scaled) -- every table of a call with them, or none.
// emission: the family -- Emission::poisson: state s emits Poisson(means[s]), the means are rates and the observes counts 0 .. 4095
// (cpprob_hip_batch_begin_problems_poisson); such a table has no sigmas, and every table of a call has the first one's family.
enum class Emission { normal, poisson };
struct HmmTable {
    std::vector<double> means, transition, sigmas;
    Emission emission = Emission::normal;
    HmmTable() = default;
    HmmTable(std::vector<double> m, std::vector<double> t, std::vector<double> s = std::vector<double>()) : means(std::move(m)), transition(std::move(t)), sigmas(std::move(s)) {}
};

// The problems of hmm_table_batch / hmm_table_fit as cpprob_hip_batch_begin_problems takes them.
struct HmmTableProblems {
    std::size_t k = 0, T_max = 0, n_max = 0;
    std::vector<double> means, trans, flat;     // [B][k], [B][k][k], the observes packed problem after problem
    std::vector<double> sigmas;                 // [B][k], or empty: the tables carry no emission scales
    bool poisson = false;                       // the tables' emission is Poisson: means holds the rates
    std::vector<std::uint32_t> T, np;           // [B]
};

inline HmmTableProblems pack_hmm_table_problems(const std::string& who, const std::vector<HmmTable>& tables, const std::vector<std::vector<double>>& observes,
                                                const std::vector<std::size_t>& n, std::size_t B)
{
    if (B == 0) throw std::runtime_error(who + ": no problems (one seed per problem)");
    auto fits = [B](std::size_t have) { return have == B || have == 1; };
    if (!fits(tables.size()) || !fits(observes.size()) || !fits(n.size()))
        throw std::runtime_error(who + ": tables, observes and n hold one entry per seed, or one entry shared by all problems");
    HmmTableProblems pk;
    pk.k = tables[0].means.size();
    pk.poisson = tables[0].emission == Emission::poisson;
    pk.T.resize(B); pk.np.resize(B);
    for (std::size_t b = 0; b < B; ++b) {
        const HmmTable& tb = tables[tables.size() == 1 ? 0 : b];
        if (tb.means.size() != pk.k || tb.transition.size() != pk.k * pk.k)
            throw std::runtime_error(who + ": problem " + std::to_string(b) + ": every table holds k means and k x k transition weights, k that of the first table");
        if (tb.sigmas.size() != (tables[0].sigmas.empty() ? 0 : pk.k))
            throw std::runtime_error(who + ": problem " + std::to_string(b) + ": every table holds k emission scales, or none does");
        if ((tb.emission == Emission::poisson) != pk.poisson || (pk.poisson && !tb.sigmas.empty()))
            throw std::runtime_error(who + ": problem " + std::to_string(b) + ": every table has one emission family, and a Poisson table has no emission scales");
        pk.means.insert(pk.means.end(), tb.means.begin(), tb.means.end());
        pk.trans.insert(pk.trans.end(), tb.transition.begin(), tb.transition.end());
        pk.sigmas.insert(pk.sigmas.end(), tb.sigmas.begin(), tb.sigmas.end());
        const std::vector<double>& o = observes[observes.size() == 1 ? 0 : b];
        pk.flat.insert(pk.flat.end(), o.begin(), o.end());
        const std::size_t nb = n[n.size() == 1 ? 0 : b];
        if (o.size() > 0x7fffffffu || nb > 0x7fffffffu) throw std::runtime_error(who + ": problem " + std::to_string(b) + ": too large for a batch");
        pk.T[b] = static_cast<std::uint32_t>(o.size()); pk.np[b] = static_cast<std::uint32_t>(nb);
        pk.T_max = std::max(pk.T_max, o.size()); pk.n_max = std::max(pk.n_max, nb);
    }
    const Options& opt = options();
    const bool masses = !opt.keep_history && opt.keep_masses;      // (a filtering-only batch that keeps the smoother's masses)
    if (!opt.keep_history && !opt.batch_dump_file.empty() && !(masses && opt.backward_trajectories))
        throw std::runtime_error(who + ": a filtering-only run (options().keep_history = false) keeps no traces to dump: clear options().batch_dump_file");
    if (!opt.keep_history && !masses && opt.backward_smoothing)
        throw std::runtime_error(who + ": backward smoothing reads the particle store: a filtering-only run (options().keep_history = false) keeps none");
    if (!opt.keep_history && !masses && opt.smoothing_lag >= 0)
        throw std::runtime_error(who + ": fixed-lag smoothing reads the particle store: a filtering-only run (options().keep_history = false) keeps none");
    check_forecast_options(who, opt.forecast_horizon, opt.forecast_trajectories, opt.keep_history || masses);
    check_decode_options(who, opt.map_decode, opt.decode_lag, opt.keep_history || masses);
    check_trajectory_stats_options(who, opt.trajectory_stats, opt.trajectory_stats_draw_index, opt.keep_history || masses);
    return pk;
}

// One batch of the packed problems on ctx: begin, run, results (options().backward_smoothing / ::smoothing_lag as hmm_table_batch
// states them) and, where dump is set, options().batch_dump_file; decode: options().map_decode is served.  The batch stays on ctx for
// the calls that read it.
// conditional: the run is cpprob_hip_batch_run_conditional on these paths (one a problem); what cpprob_hip_batch_results returns stays default.
// retable: ctx holds this batch begun with other tables -- it is given pk's tables where it stands (cpprob_hip_batch_retable; with_observes:
// the first such call of the batch, which uploads them) in place of a begin.
inline std::vector<Result> run_hmm_table_problems(Context& ctx, const HmmTableProblems& pk, const std::vector<std::uint64_t>& seeds, bool dump, bool decode = true,
                                                  const std::vector<std::vector<int>>* conditional = nullptr, bool retable = false, bool with_observes = true)
{
    const Options& opt = options();
    const std::size_t B = seeds.size(), k = pk.k, T_max = pk.T_max;
    const std::vector<std::uint32_t>& T = pk.T;
    cpprob_hip_batch_config bc{};
    bc.algorithm = CPPROB_HIP_ALG_SMC;
    bc.model = CPPROB_HIP_MODEL_HMM_TABLE;
    bc.resampler = opt.resampler;
    bc.keep_history = opt.keep_history ? 1 : 0;
    bc.flags = !opt.keep_history && opt.keep_masses ? CPPROB_HIP_BATCH_KEEP_MASSES : 0;
    bc.ess_threshold = opt.ess_threshold;
    bc.n_particles = pk.n_max;
    bc.n_problems = B;
    const auto t0 = std::chrono::steady_clock::now();
    const bool scaled = !pk.sigmas.empty();
    if (retable && pk.poisson)
        ctx.check(cpprob_hip_batch_retable_poisson(ctx.get(), pk.means.data(), pk.trans.data(), with_observes ? pk.flat.data() : nullptr, pk.flat.size()), "cpprob_hip_batch_retable_poisson");
    else if (pk.poisson)
        ctx.check(cpprob_hip_batch_begin_problems_poisson(ctx.get(), &bc, T.data(), pk.np.data(), pk.flat.data(), static_cast<std::int32_t>(k), pk.means.data(), pk.trans.data()),
                  "cpprob_hip_batch_begin_problems_poisson");
    else if (retable && scaled)
        ctx.check(cpprob_hip_batch_retable_scaled(ctx.get(), pk.means.data(), pk.trans.data(), pk.sigmas.data(), with_observes ? pk.flat.data() : nullptr, pk.flat.size()),
                  "cpprob_hip_batch_retable_scaled");
    else if (retable)
        ctx.check(cpprob_hip_batch_retable(ctx.get(), pk.means.data(), pk.trans.data(), with_observes ? pk.flat.data() : nullptr, pk.flat.size()), "cpprob_hip_batch_retable");
    else if (scaled)
        ctx.check(cpprob_hip_batch_begin_problems_scaled(ctx.get(), &bc, T.data(), pk.np.data(), pk.flat.data(), static_cast<std::int32_t>(k), pk.means.data(), pk.trans.data(),
                                                         pk.sigmas.data()), "cpprob_hip_batch_begin_problems_scaled");
    else
        ctx.check(cpprob_hip_batch_begin_problems(ctx.get(), &bc, T.data(), pk.np.data(), pk.flat.data(), static_cast<std::int32_t>(k), pk.means.data(), pk.trans.data()),
                  "cpprob_hip_batch_begin_problems");
    std::vector<cpprob_hip_summary> sums(B);
    const std::size_t K = 8;
    std::vector<double> stats(B * T_max * K), ess(B * T_max);
    if (conditional) {
        std::vector<std::int32_t> ref;
        for (const std::vector<int>& path : *conditional) ref.insert(ref.end(), path.begin(), path.end());
        ctx.check(cpprob_hip_batch_run_conditional(ctx.get(), seeds.data(), ref.data(), ref.size()), "cpprob_hip_batch_run_conditional");
    } else {
        ctx.check(cpprob_hip_batch_run(ctx.get(), seeds.data()), "cpprob_hip_batch_run");
        ctx.check(cpprob_hip_batch_results(ctx.get(), sums.data(), stats.data(), stats.size(), ess.data(), nullptr), "cpprob_hip_batch_results");
    }
    if (opt.smoothing_lag >= 0) batch_lag_marginals(ctx, static_cast<std::size_t>(opt.smoothing_lag), nullptr, T_max, stats);
    else if (opt.backward_smoothing) batch_backward_marginals(ctx, stats);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (dump && !opt.batch_dump_file.empty() && opt.backward_trajectories)
        dump_batch_backward(ctx, opt.batch_dump_file, T, opt.backward_trajectories, [&T](std::size_t b) { return hmm_table_structure(T[b]); });
    else if (dump && !opt.batch_dump_file.empty())
        dump_batch_posterior(ctx, opt.batch_dump_file, T, pk.np, opt.dump_max_particles, [&T](std::size_t b) { return hmm_table_structure(T[b]); });
    std::vector<Result> out(B);
    for (std::size_t b = 0; b < B; ++b) {
        Result& r = out[b];
        const cpprob_hip_summary& s = sums[b];
        r.n_particles = pk.np[b]; r.log_evidence = s.log_evidence; r.ess = s.ess_final; r.log_norm = s.log_norm; r.n_resampled = s.n_resampled;
        r.used_builtin = true; r.step_form = s.step_form; r.run_seconds = seconds;
        // (a conditional run: the predicts hold the smoother's marginals where they were asked for, else nothing)
        if (conditional) { r = Result(); r.n_particles = pk.np[b]; r.used_builtin = true; r.run_seconds = seconds; }
        if (conditional && opt.smoothing_lag < 0 && !opt.backward_smoothing) continue;
        r.predicts.resize(T[b]);
        for (std::size_t t = 0; t < T[b]; ++t) {
            PredictStats& p = r.predicts[t];
            p.address = "state[" + std::to_string(t) + "]";
            p.is_int = true;
            p.probabilities.assign(stats.begin() + (b * T_max + t) * K, stats.begin() + (b * T_max + t) * K + k);
        }
        if (!conditional) r.step_ess.assign(ess.begin() + b * T_max, ess.begin() + b * T_max + T[b]);
    }
    batch_forecast_results(ctx, opt.forecast_horizon, opt.forecast_trajectories, K, k, out);
    batch_decode_results(ctx, decode && opt.map_decode, opt.decode_lag, T, out);
    batch_trajectory_stats_results(ctx, opt.trajectory_stats, opt.trajectory_stats_draw_index, pk.flat, out);
    return out;
}

inline std::vector<Result> hmm_table_batch(const std::vector<HmmTable>& tables, const std::vector<std::vector<double>>& observes,
                                           const std::vector<std::size_t>& n, const std::vector<std::uint64_t>& seeds)
{
    const std::string who = "cpprob::gpu::hmm_table_batch";
    const HmmTableProblems pk = pack_hmm_table_problems(who, tables, observes, n, seeds.size());
    const Options& opt = options();
    const std::vector<std::vector<int>>* conditional = opt.conditional_paths.empty() ? nullptr : &opt.conditional_paths;
    if (conditional) {
        if (opt.keep_history || !opt.keep_masses)
            throw std::runtime_error(who + ": a conditional run (options().conditional_paths) keeps masses, not a particle store: set options().keep_history = false and options().keep_masses");
        if (conditional->size() != seeds.size()) throw std::runtime_error(who + ": options().conditional_paths holds one path per problem");
        for (std::size_t b = 0; b < seeds.size(); ++b) {
            if ((*conditional)[b].size() != pk.T[b])
                throw std::runtime_error(who + ": problem " + std::to_string(b) + ": options().conditional_paths holds one state per observe");
            for (int s : (*conditional)[b])
                if (s < 0 || static_cast<std::size_t>(s) >= pk.k)
                    throw std::runtime_error(who + ": problem " + std::to_string(b) + ": options().conditional_paths holds states 0 .. k - 1");
        }
    }
    ContextLease lease(options().device);
    std::vector<Result> out = run_hmm_table_problems(*lease, pk, seeds, true, true, conditional);
    lease.done();
    return out;
}

// ---- particle EM for the tables (cpprob_hip_batch_smooth_stats) ----
// Fits every problem's table to its observes: iteration i runs the batch of hmm_table_batch with the current tables and the keys
// seeds[b] + i, takes the backward smoother's expected sufficient statistics (the E-step, on the device) and sets
//   transition[s][s'] = xi[s][s'] / (xi[s][0] + .. + xi[s][k-1]),   means[s] = occ_y[s] / occ[s]
// (the M-step; a row or a state without mass keeps its value; the emission's sigma is 1 and not fitted).  Returns the fitted tables
// and the results of the last run -- those of the tables that run began with.  options().keep_history must be set, or options().keep_masses
// with it (the statistics then come from the masses the filtering-only runs keep);
// options().batch_dump_file is written by the last run.  options().map_decode: one more run, with the keys seeds[b] + iterations,
// under the FITTED tables, and its decode (Result::map_path, ::map_score) in the results -- the labels a fit is made for.
// options().fit_on_device: the first run begins the batch, every later one re-tables it on the device (cpprob_hip_batch_retable) -- the
// same HmmTableFit bit for bit without a begin's host work an iteration.
// Tables with emission scales (HmmTable::sigmas): the batches are scaled; options().learn_scales: the M-step fits the scales too -- a
// state with mass takes v = occ_yy[s] / occ[s] - means[s] means[s] (its new mean) and sigmas[s] = sqrt(v) where v >= scale_floor^2, else
// options().scale_floor (a NaN v too), the statements of cpprob_hip_batch_mstep_scaled_device.  Without it the scales stay.
// Poisson tables (HmmTable::emission): the batches are Poisson ones and the M-step's means[s] = occ_y[s] / occ[s] is the rate's, kept at or
// above options().rate_floor (a NaN too), the statements of cpprob_hip_batch_mstep_poisson_device.
// options().tie_groups (one group id a problem): tied tables -- every begun batch is tied (cpprob_hip_batch_tie; once with
// fit_on_device, a re-table keeps the tie) and an iteration's records go through cpprob_hip_batch_pool_stats (broadcast) in front of
// the M-step's statements, which are unchanged: the members of a group, which must start from one table bit for bit (else
// std::runtime_error naming the group), hold one table throughout, fitted to all of their observes.
struct HmmTableFit { std::vector<HmmTable> tables; std::vector<Result> results; };

inline HmmTableFit hmm_table_fit(const std::vector<HmmTable>& tables, const std::vector<std::vector<double>>& observes, const std::vector<std::size_t>& n,
                                 const std::vector<std::uint64_t>& seeds, std::size_t iterations)
{
    const std::size_t B = seeds.size();
    HmmTableProblems pk = pack_hmm_table_problems("cpprob::gpu::hmm_table_fit", tables, observes, n, B);
    if (!options().keep_history && !options().keep_masses)
        throw std::runtime_error("cpprob::gpu::hmm_table_fit: the statistics read the particle store: a filtering-only run (options().keep_history = false) keeps none");
    const std::size_t k = pk.k, R = 88;
    HmmTableFit fit;
    ContextLease lease(options().device);
    Context& ctx = *lease;
    std::vector<double> rec(B * R), pooled(options().tie_groups.empty() ? 0 : B * R);
    std::vector<std::uint64_t> keys(B);
    const bool kept = options().fit_on_device;                 // the batch of iteration 0 is re-tabled from then on
    const bool fit_scales = options().learn_scales;
    const double floor = options().scale_floor;
    if (fit_scales && pk.sigmas.empty()) throw std::runtime_error("cpprob::gpu::hmm_table_fit: options().learn_scales fits emission scales: give every table its sigmas");
    if (fit_scales && (!(floor > 0.0) || !std::isfinite(floor))) throw std::runtime_error("cpprob::gpu::hmm_table_fit: options().scale_floor must be finite and > 0");
    const double rate_floor = options().rate_floor;
    if (pk.poisson && fit_scales) throw std::runtime_error("cpprob::gpu::hmm_table_fit: options().learn_scales fits emission scales: a Poisson table has none");
    if (pk.poisson && (!(rate_floor > 0.0) || !std::isfinite(rate_floor))) throw std::runtime_error("cpprob::gpu::hmm_table_fit: options().rate_floor must be finite and > 0");
    const std::vector<std::int32_t>& tie = options().tie_groups;
    if (!tie.empty()) {
        // a group's members start from one table, bit for bit; lead[g]: the group's first member
        if (tie.size() != B) throw std::runtime_error("cpprob::gpu::hmm_table_fit: options().tie_groups holds " + std::to_string(tie.size()) + " ids for " + std::to_string(B) + " problems");
        std::vector<std::size_t> lead;
        for (std::size_t b = 0; b < B; ++b) {
            if (tie[b] < 0) throw std::runtime_error("cpprob::gpu::hmm_table_fit: options().tie_groups: the group id of problem " + std::to_string(b) + " is negative");
            const std::size_t g = static_cast<std::size_t>(tie[b]);
            if (g >= lead.size()) lead.resize(g + 1, B);
            if (lead[g] == B) { lead[g] = b; continue; }
            const std::size_t a = lead[g];
            const bool same = std::memcmp(&pk.means[a * k], &pk.means[b * k], k * sizeof(double)) == 0 &&
                              std::memcmp(&pk.trans[a * k * k], &pk.trans[b * k * k], k * k * sizeof(double)) == 0 &&
                              (pk.sigmas.empty() || std::memcmp(&pk.sigmas[a * k], &pk.sigmas[b * k], k * sizeof(double)) == 0);
            if (!same)
                throw std::runtime_error("cpprob::gpu::hmm_table_fit: group " + std::to_string(g) + ": the initial table of problem " + std::to_string(b) +
                                         " differs from that of problem " + std::to_string(a) + "; a group's members start from one table");
        }
    }
    std::size_t runs = 0;
    for (std::size_t it = 0; it < iterations; ++it) {
        for (std::size_t b = 0; b < B; ++b) keys[b] = seeds[b] + it;
        fit.results = run_hmm_table_problems(ctx, pk, keys, it + 1 == iterations, false, nullptr, kept && runs > 0, runs == 1);
        // (a fresh begin has forgotten the tie, a re-table keeps it)
        if (!tie.empty() && (!kept || runs == 0)) ctx.check(cpprob_hip_batch_tie(ctx.get(), tie.data(), tie.size()), "cpprob_hip_batch_tie");
        ++runs;
        ctx.check(cpprob_hip_batch_smooth_stats(ctx.get(), pk.flat.empty() ? nullptr : pk.flat.data(), pk.flat.size(), rec.data(), rec.size()),
                  "cpprob_hip_batch_smooth_stats");
        if (!tie.empty()) {
            // every member's record becomes its group's pooled record: the M-step below then gives the members one table
            ctx.check(cpprob_hip_batch_pool_stats(ctx.get(), rec.data(), rec.size(), 1, 1, pooled.data(), pooled.size()), "cpprob_hip_batch_pool_stats");
            rec.swap(pooled);
        }
        for (std::size_t b = 0; b < B; ++b) {
            const double* r = rec.data() + b * R;
            for (std::size_t s = 0; s < k; ++s) {
                double row = 0.0;
                for (std::size_t j = 0; j < k; ++j) row = row + r[8 * s + j];
                if (row > 0.0)
                    for (std::size_t j = 0; j < k; ++j) pk.trans[(b * k + s) * k + j] = r[8 * s + j] / row;
                if (r[64 + s] > 0.0) pk.means[b * k + s] = r[72 + s] / r[64 + s];
                if (pk.poisson && r[64 + s] > 0.0 && !(pk.means[b * k + s] >= rate_floor)) pk.means[b * k + s] = rate_floor;
                if (fit_scales && r[64 + s] > 0.0) {
                    const double mean = pk.means[b * k + s], mm = mean * mean, ff = floor * floor;
                    double v = r[80 + s] / r[64 + s];
                    v = v - mm;
                    pk.sigmas[b * k + s] = v >= ff ? std::sqrt(v) : floor;
                }
            }
        }
    }
    if (options().map_decode) {
        for (std::size_t b = 0; b < B; ++b) keys[b] = seeds[b] + iterations;
        std::vector<Result> fin = run_hmm_table_problems(ctx, pk, keys, false, true, nullptr, kept && runs > 0, runs == 1);
        if (fit.results.empty()) fit.results = fin;
        for (std::size_t b = 0; b < B; ++b) { fit.results[b].map_decoded = true; fit.results[b].map_path = fin[b].map_path; fit.results[b].map_score = fin[b].map_score; }
    }
    lease.done();
    fit.tables.resize(B);
    for (std::size_t b = 0; b < B; ++b) {
        fit.tables[b].means.assign(pk.means.begin() + static_cast<std::ptrdiff_t>(b * k), pk.means.begin() + static_cast<std::ptrdiff_t>((b + 1) * k));
        fit.tables[b].transition.assign(pk.trans.begin() + static_cast<std::ptrdiff_t>(b * k * k), pk.trans.begin() + static_cast<std::ptrdiff_t>((b + 1) * k * k));
        if (!pk.sigmas.empty()) fit.tables[b].sigmas.assign(pk.sigmas.begin() + static_cast<std::ptrdiff_t>(b * k), pk.sigmas.begin() + static_cast<std::ptrdiff_t>((b + 1) * k));
        if (pk.poisson) fit.tables[b].emission = Emission::poisson;
    }
    return fit;
}

// ---- the same problems with observes that arrive over time (cpprob_hip_batch_begin_online / _advance) ----
// Constructed from what hmm_table_batch takes, with capacities (the most observes a problem may reach) in the observes' place; the
// number of problems is seeds.size(), and tables, capacities and n of size 1 are shared by all.  advance() hands problem b its new
// observes (new_observes[b], possibly empty; one entry per problem), runs the new steps only and returns every problem's result so
// far: bit for bit what hmm_table_batch returns for the observes seen so far.  A problem without observes has no predicts yet.
// readout = false (keep_history only) leaves the smoothed predicts to a later advance and returns results without predicts; an
// advance of empty sequences with readout = true then returns them.  dump(prefix) writes every problem's posterior traces for the
// lengths reached, as hmm_table_batch does for options().batch_dump_file (whether or not the last advance did its read-out).
// options().backward_smoothing: the predicts are the backward smoother's marginals, after every advance whatever its readout;
// options().backward_trajectories = M > 0: dump() writes M backward-simulated trajectories a problem in the lineages' place.
// options().smoothing_lag = lag >= 0: the predicts are the fixed-lag marginals P(x_t | y_0 .. y_min(t + lag, L - 1)), after every
// advance whatever its readout.  An advance asks the device for the steps from max(0, L_before - lag) on -- those whose estimate the
// new observes can still change -- and the object keeps the final rows on the host: the work of an advance is that of its new steps,
// and the predicts depend on the lengths reached alone, never on how the observes were cut into advances.
// options().forecast_horizon = H > 0: every advance's results carry the forecast from the lengths reached (Result::forecast, and
// Result::forecast_trajectories for options().forecast_trajectories > 0); a problem without observes has rows of zeros.
// options().map_decode: every advance's results carry the most probable state path of the lengths reached (Result::map_path,
// ::map_score); with options().decode_lag = lag >= 0 the path holds the fixed-lag rows instead -- row t is final once lag more
// observes have arrived --, an advance asks for the rows from max(0, L_before - lag) on and the object keeps the final ones.  The
// forward work of an advance is that of its new steps either way.
// options().trajectory_stats = M > 0: every advance's results carry the records of M backward-simulated trajectories of the lengths
// reached (Result::trajectory_stats; the object keeps the observes seen so far for their occ_y and occ_yy); a problem without
// observes has zero records.
// options().running_stats: every advance's results carry the expected sufficient statistics of the lengths reached
// (Result::running_stats), kept forward-only on the device (cpprob_hip_batch_online_stats): the call consumes the advance's own
// observes and costs its new steps, whatever length the stream has reached; a problem without observes has a zero record.
// options().learn_tables: online EM -- the stream is armed (cpprob_hip_batch_learn_begin, step sizes (t + 1) ^ -options().learn_step_exponent,
// burn-in options().learn_burn_in) and every advance is a learning advance (cpprob_hip_batch_advance_learn, with the read-out walk):
// the tables change between advances, the chunk is the update period, log_evidence is the prequential likelihood under the tables in
// force at each step; tables() reads what the stream has learned.
// Tables with emission scales (HmmTable::sigmas): the stream is a scaled one (cpprob_hip_batch_begin_online_scaled); with
// options().learn_tables and options().learn_scales the learner fits the scales too, none below options().scale_floor
// (cpprob_hip_batch_learn_begin_scaled) -- without learn_scales it learns means and transition rows and keeps them; tables() returns them.
// Poisson tables (HmmTable::emission): the stream is a Poisson one (cpprob_hip_batch_begin_online_poisson); options().learn_tables is
// refused for it (std::runtime_error): online EM serves the Gaussian families.
// options().learn_tables with options().tie_groups (one group id a problem; options().learn_tied asks for them): tied online EM -- the
// stream is tied and its learner pools over the tie (cpprob_hip_batch_tie, _learn_tie): the streams of a group, which must start from one
// table bit for bit, learn ONE table from their pooled records, every stream weighing equally whatever its length; the burn-in counts the
// observes the group has seen; tables() returns equal tables for the members of a group.
// Options are read once, by the constructor.  The object holds
// one context until it is destroyed.
class HmmTableStream {
public:
    HmmTableStream(const std::vector<HmmTable>& tables, const std::vector<std::size_t>& capacities, const std::vector<std::size_t>& n,
                   const std::vector<std::uint64_t>& seeds)
        : B_(seeds.size()), k_(tables.empty() ? 0 : tables[0].means.size()), keep_(options().keep_history), masses_(!options().keep_history && options().keep_masses), lease_(options().device)
    {
        if (B_ == 0) throw std::runtime_error("cpprob::gpu::HmmTableStream: no problems (one seed per problem)");
        check_forecast_options("cpprob::gpu::HmmTableStream", forecast_H_, forecast_M_, keep_ || masses_);
        check_decode_options("cpprob::gpu::HmmTableStream", decode_, decode_lag_, keep_ || masses_);
        check_trajectory_stats_options("cpprob::gpu::HmmTableStream", traj_stats_M_, traj_stats_draw_, keep_ || masses_);
        if (!keep_ && !masses_ && running_stats_)
            throw std::runtime_error("cpprob::gpu::HmmTableStream: options().running_stats reads the smoother's masses: a filtering-only run (options().keep_history = false) keeps none without options().keep_masses");
        if (!keep_ && !masses_ && learn_)
            throw std::runtime_error("cpprob::gpu::HmmTableStream: options().learn_tables reads the smoother's masses: a filtering-only run (options().keep_history = false) keeps none without options().keep_masses");
        if (!keep_ && !masses_ && backward_)
            throw std::runtime_error("cpprob::gpu::HmmTableStream: backward smoothing reads the particle store: a filtering-only run (options().keep_history = false) keeps none");
        if (!keep_ && !masses_ && lag_ >= 0)
            throw std::runtime_error("cpprob::gpu::HmmTableStream: fixed-lag smoothing reads the particle store: a filtering-only run (options().keep_history = false) keeps none");
        const std::size_t B = B_;
        auto fits = [B](std::size_t have) { return have == B || have == 1; };
        if (!fits(tables.size()) || !fits(capacities.size()) || !fits(n.size()))
            throw std::runtime_error("cpprob::gpu::HmmTableStream: tables, capacities and n hold one entry per seed, or one entry shared by all problems");
        std::vector<double> means, trans, sigmas;
        scaled_ = !tables[0].sigmas.empty();
        poisson_ = tables[0].emission == Emission::poisson;
        if (poisson_ && learn_)
            throw std::runtime_error("cpprob::gpu::HmmTableStream: options().learn_tables (online EM) serves Gaussian emissions: a Poisson stream is fitted by cpprob::gpu::hmm_table_fit");
        if (options().learn_scales && learn_ && !scaled_)
            throw std::runtime_error("cpprob::gpu::HmmTableStream: options().learn_scales fits emission scales: give every table its sigmas");
        std::vector<std::uint32_t> cap(B_);
        np_.resize(B_);
        std::size_t n_max = 0;
        for (std::size_t b = 0; b < B_; ++b) {
            const HmmTable& tb = tables[tables.size() == 1 ? 0 : b];
            if (tb.means.size() != k_ || tb.transition.size() != k_ * k_)
                throw std::runtime_error("cpprob::gpu::HmmTableStream: problem " + std::to_string(b) + ": every table holds k means and k x k transition weights, k that of the first table");
            if (tb.sigmas.size() != (scaled_ ? k_ : 0))
                throw std::runtime_error("cpprob::gpu::HmmTableStream: problem " + std::to_string(b) + ": every table holds k emission scales, or none does");
            if ((tb.emission == Emission::poisson) != poisson_ || (poisson_ && scaled_))
                throw std::runtime_error("cpprob::gpu::HmmTableStream: problem " + std::to_string(b) + ": every table has one emission family, and a Poisson table has no emission scales");
            means.insert(means.end(), tb.means.begin(), tb.means.end());
            trans.insert(trans.end(), tb.transition.begin(), tb.transition.end());
            sigmas.insert(sigmas.end(), tb.sigmas.begin(), tb.sigmas.end());
            const std::size_t cb = capacities[capacities.size() == 1 ? 0 : b], nb = n[n.size() == 1 ? 0 : b];
            if (cb > 0x7fffffffu || nb > 0x7fffffffu) throw std::runtime_error("cpprob::gpu::HmmTableStream: problem " + std::to_string(b) + ": too large for a batch");
            cap[b] = static_cast<std::uint32_t>(cb); np_[b] = static_cast<std::uint32_t>(nb);
            T_max_ = std::max(T_max_, cb); n_max = std::max(n_max, nb);
        }
        const Options& opt = options();
        cpprob_hip_batch_config bc{};
        bc.algorithm = CPPROB_HIP_ALG_SMC;
        bc.model = CPPROB_HIP_MODEL_HMM_TABLE;
        bc.resampler = opt.resampler;
        bc.keep_history = keep_ ? 1 : 0;
        bc.flags = masses_ ? CPPROB_HIP_BATCH_KEEP_MASSES : 0;
        bc.ess_threshold = opt.ess_threshold;
        bc.n_particles = n_max;
        bc.n_problems = B_;
        Context& ctx = *lease_;
        if (poisson_)
            ctx.check(cpprob_hip_batch_begin_online_poisson(ctx.get(), &bc, cap.data(), np_.data(), static_cast<std::int32_t>(k_), means.data(), trans.data(), seeds.data()),
                      "cpprob_hip_batch_begin_online_poisson");
        else if (scaled_)
            ctx.check(cpprob_hip_batch_begin_online_scaled(ctx.get(), &bc, cap.data(), np_.data(), static_cast<std::int32_t>(k_), means.data(), trans.data(), sigmas.data(),
                                                           seeds.data()), "cpprob_hip_batch_begin_online_scaled");
        else
            ctx.check(cpprob_hip_batch_begin_online(ctx.get(), &bc, cap.data(), np_.data(), static_cast<std::int32_t>(k_), means.data(), trans.data(), seeds.data()),
                      "cpprob_hip_batch_begin_online");
        if (learn_) {
            // the step sizes, evaluated here: the device takes no power
            std::vector<double> gamma(T_max_);
            for (std::size_t t = 0; t < T_max_; ++t) gamma[t] = std::pow(static_cast<double>(t) + 1.0, -opt.learn_step_exponent);
            const std::uint32_t burn_in = static_cast<std::uint32_t>(std::min<std::size_t>(opt.learn_burn_in, 0xffffffffu));
            if (scaled_ && opt.learn_scales)
                ctx.check(cpprob_hip_batch_learn_begin_scaled(ctx.get(), gamma.data(), gamma.size(), burn_in, opt.scale_floor), "cpprob_hip_batch_learn_begin_scaled");
            else
                ctx.check(cpprob_hip_batch_learn_begin(ctx.get(), gamma.data(), gamma.size(), burn_in), "cpprob_hip_batch_learn_begin");
            if (opt.learn_tied || !opt.tie_groups.empty()) {
                // tied online EM: the streams of a group learn one table (the library checks that they start from one, bit for bit)
                if (opt.tie_groups.size() != B_)
                    throw std::runtime_error("cpprob::gpu::HmmTableStream: options().tie_groups holds " + std::to_string(opt.tie_groups.size()) + " ids for " + std::to_string(B_) + " problems");
                ctx.check(cpprob_hip_batch_tie(ctx.get(), opt.tie_groups.data(), opt.tie_groups.size()), "cpprob_hip_batch_tie");
                ctx.check(cpprob_hip_batch_learn_tie(ctx.get()), "cpprob_hip_batch_learn_tie");
            }
        }
        lease_.done();
        if (lag_ >= 0) { lagged_.assign(B_ * T_max_ * 8, 0.0); L_prev_.assign(B_, 0); }
        if (decode_ && decode_lag_ >= 0) { decoded_.assign(B_ * T_max_, -1); dec_prev_.assign(B_, 0); }
        if (traj_stats_M_) seen_.resize(B_);
    }
    HmmTableStream(const HmmTableStream&) = delete;
    HmmTableStream& operator=(const HmmTableStream&) = delete;

    std::vector<Result> advance(const std::vector<std::vector<double>>& new_observes, bool readout = true)
    {
        if (new_observes.size() != B_) throw std::runtime_error("cpprob::gpu::HmmTableStream: one (possibly empty) sequence of new observes per problem");
        std::vector<std::uint32_t> dT(B_), L(B_);
        std::vector<double> flat;
        for (std::size_t b = 0; b < B_; ++b) {
            if (new_observes[b].size() > 0x7fffffffu) throw std::runtime_error("cpprob::gpu::HmmTableStream: problem " + std::to_string(b) + ": too large for a batch");
            dT[b] = static_cast<std::uint32_t>(new_observes[b].size());
            flat.insert(flat.end(), new_observes[b].begin(), new_observes[b].end());
        }
        Context& ctx = *lease_;
        const auto t0 = std::chrono::steady_clock::now();
        // (a learning stream's advance does the read-out walk every time)
        if (learn_) ctx.check(cpprob_hip_batch_advance_learn(ctx.get(), dT.data(), flat.empty() ? nullptr : flat.data()), "cpprob_hip_batch_advance_learn");
        else ctx.check(cpprob_hip_batch_advance(ctx.get(), dT.data(), flat.empty() ? nullptr : flat.data(), readout ? 1 : 0), "cpprob_hip_batch_advance");
        ctx.check(cpprob_hip_batch_lengths(ctx.get(), L.data()), "cpprob_hip_batch_lengths");
        // (the backward smoother reads the store, not the read-out: its marginals are there after every advance)
        const bool lagged = lag_ >= 0, with_stats = readout || !keep_ || backward_ || lagged;
        const std::size_t K = 8;
        std::vector<cpprob_hip_summary> sums(B_);
        std::vector<double> stats(with_stats && !lagged ? B_ * T_max_ * K : 0), ess(B_ * T_max_);
        ctx.check(cpprob_hip_batch_results(ctx.get(), sums.data(), with_stats && !backward_ && !lagged ? stats.data() : nullptr, stats.size(), ess.data(), nullptr), "cpprob_hip_batch_results");
        if (lagged) {
            // the steps the new observes can still change: from max(0, L_before - lag) on; the rows before them are final and kept
            std::vector<std::uint32_t> from(B_);
            std::size_t n_rows = 0;
            for (std::size_t b = 0; b < B_; ++b) {
                from[b] = L_prev_[b] > static_cast<std::size_t>(lag_) ? static_cast<std::uint32_t>(L_prev_[b] - static_cast<std::size_t>(lag_)) : 0u;
                n_rows = std::max<std::size_t>(n_rows, L[b] - from[b]);
            }
            std::vector<double> rows(B_ * n_rows * K);
            batch_lag_marginals(ctx, static_cast<std::size_t>(lag_), from.data(), n_rows, rows);
            for (std::size_t b = 0; b < B_; ++b) {
                std::copy(rows.begin() + static_cast<std::ptrdiff_t>(b * n_rows * K), rows.begin() + static_cast<std::ptrdiff_t>((b * n_rows + (L[b] - from[b])) * K),
                          lagged_.begin() + static_cast<std::ptrdiff_t>((b * T_max_ + from[b]) * K));
                L_prev_[b] = L[b];
            }
        } else if (backward_) batch_backward_marginals(ctx, stats);
        const std::vector<double>& shown = lagged ? lagged_ : stats;
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::vector<Result> out(B_);
        for (std::size_t b = 0; b < B_; ++b) {
            Result& r = out[b];
            const cpprob_hip_summary& s = sums[b];
            r.n_particles = np_[b]; r.log_evidence = s.log_evidence; r.ess = s.ess_final; r.log_norm = s.log_norm; r.n_resampled = s.n_resampled;
            r.used_builtin = true; r.step_form = s.step_form; r.run_seconds = seconds;
            r.predicts.resize(with_stats ? L[b] : 0);
            for (std::size_t t = 0; t < r.predicts.size(); ++t) {
                PredictStats& p = r.predicts[t];
                p.address = "state[" + std::to_string(t) + "]";
                p.is_int = true;
                p.probabilities.assign(shown.begin() + (b * T_max_ + t) * K, shown.begin() + (b * T_max_ + t) * K + k_);
            }
            r.step_ess.assign(ess.begin() + b * T_max_, ess.begin() + b * T_max_ + L[b]);
        }
        batch_forecast_results(ctx, forecast_H_, forecast_M_, K, k_, out);      // (after every advance, whatever its readout)
        if (decode_ && decode_lag_ >= 0) {
            // the rows the new observes can still change: from max(0, L_before - lag) on; the rows before them are final and kept
            std::vector<std::uint32_t> from(B_);
            std::size_t n_rows = 0;
            for (std::size_t b = 0; b < B_; ++b) {
                from[b] = dec_prev_[b] > static_cast<std::size_t>(decode_lag_) ? static_cast<std::uint32_t>(dec_prev_[b] - static_cast<std::size_t>(decode_lag_)) : 0u;
                n_rows = std::max<std::size_t>(n_rows, L[b] - from[b]);
            }
            std::vector<std::int32_t> st(B_ * n_rows);
            std::vector<double> score(B_);
            ctx.check(cpprob_hip_batch_decode_lag(ctx.get(), static_cast<std::uint64_t>(decode_lag_), from.data(), n_rows, n_rows ? st.data() : nullptr, st.size(),
                                                  score.data(), score.size()), "cpprob_hip_batch_decode_lag");
            for (std::size_t b = 0; b < B_; ++b) {
                std::copy(st.begin() + static_cast<std::ptrdiff_t>(b * n_rows), st.begin() + static_cast<std::ptrdiff_t>(b * n_rows + (L[b] - from[b])),
                          decoded_.begin() + static_cast<std::ptrdiff_t>(b * T_max_ + from[b]));
                dec_prev_[b] = L[b];
                out[b].map_decoded = true; out[b].map_score = score[b];
                out[b].map_path.assign(decoded_.begin() + static_cast<std::ptrdiff_t>(b * T_max_), decoded_.begin() + static_cast<std::ptrdiff_t>(b * T_max_ + L[b]));
            }
        } else batch_decode_results(ctx, decode_, -1, L, out);
        if (traj_stats_M_) {
            std::vector<double> seen;
            for (std::size_t b = 0; b < B_; ++b) {
                seen_[b].insert(seen_[b].end(), new_observes[b].begin(), new_observes[b].end());
                seen.insert(seen.end(), seen_[b].begin(), seen_[b].end());
            }
            batch_trajectory_stats_results(ctx, traj_stats_M_, traj_stats_draw_, seen, out);
        }
        if (running_stats_) {
            // (the steps the call consumes are this advance's: every advance is followed by the call)
            const std::size_t R = 88;
            std::vector<double> rec(B_ * R);
            ctx.check(cpprob_hip_batch_online_stats(ctx.get(), flat.empty() ? nullptr : flat.data(), flat.size(), rec.data(), rec.size()), "cpprob_hip_batch_online_stats");
            for (std::size_t b = 0; b < B_; ++b) out[b].running_stats.assign(rec.begin() + static_cast<std::ptrdiff_t>(b * R), rec.begin() + static_cast<std::ptrdiff_t>((b + 1) * R));
        }
        return out;
    }

    // options().learn_tables: the tables the stream has learned so far, one a problem, as the device holds them (synchronises).
    std::vector<HmmTable> tables()
    {
        if (!learn_) throw std::runtime_error("cpprob::gpu::HmmTableStream: tables() reads the tables of a learning stream: set options().learn_tables");
        Context& ctx = *lease_;
        std::vector<double> means(B_ * k_), trans(B_ * k_ * k_), sigmas(scaled_ ? B_ * k_ : 0);
        if (scaled_)
            ctx.check(cpprob_hip_batch_learn_tables_scaled(ctx.get(), means.data(), trans.data(), sigmas.data(), nullptr), "cpprob_hip_batch_learn_tables_scaled");
        else
            ctx.check(cpprob_hip_batch_learn_tables(ctx.get(), means.data(), trans.data(), nullptr), "cpprob_hip_batch_learn_tables");
        std::vector<HmmTable> out(B_);
        for (std::size_t b = 0; b < B_; ++b) {
            if (scaled_) out[b].sigmas.assign(sigmas.begin() + static_cast<std::ptrdiff_t>(b * k_), sigmas.begin() + static_cast<std::ptrdiff_t>((b + 1) * k_));
            out[b].means.assign(means.begin() + static_cast<std::ptrdiff_t>(b * k_), means.begin() + static_cast<std::ptrdiff_t>((b + 1) * k_));
            out[b].transition.assign(trans.begin() + static_cast<std::ptrdiff_t>(b * k_ * k_), trans.begin() + static_cast<std::ptrdiff_t>((b + 1) * k_ * k_));
        }
        return out;
    }

    // Problem b's posterior as <prefix>_<b>.int / .ids for the lengths reached: the first dump_max_ traces (0 = all).
    void dump(const std::string& prefix)
    {
        if (!keep_ && !(masses_ && backward_traj_)) throw std::runtime_error("cpprob::gpu::HmmTableStream: a filtering-only run (options().keep_history = false) keeps no traces to dump");
        Context& ctx = *lease_;
        std::vector<std::uint32_t> L(B_);
        ctx.check(cpprob_hip_batch_lengths(ctx.get(), L.data()), "cpprob_hip_batch_lengths");
        if (backward_traj_) dump_batch_backward(ctx, prefix, L, backward_traj_, [&L](std::size_t b) { return hmm_table_structure(L[b]); });
        else dump_batch_posterior(ctx, prefix, L, np_, dump_max_, [&L](std::size_t b) { return hmm_table_structure(L[b]); });
    }

private:
    std::size_t B_, k_, T_max_ = 0;
    bool keep_, masses_;                       // masses_: a filtering-only batch that keeps the smoother's masses (options().keep_masses)
    bool backward_ = options().backward_smoothing;
    std::size_t backward_traj_ = options().backward_trajectories;
    long lag_ = options().smoothing_lag;
    std::size_t forecast_H_ = options().forecast_horizon, forecast_M_ = options().forecast_trajectories;
    std::vector<double> lagged_;               // smoothing_lag: [B][T_max][8], the fixed-lag rows so far (rows below L - lag are final)
    std::vector<std::size_t> L_prev_;          // ... and the lengths they stand for
    bool decode_ = options().map_decode;
    long decode_lag_ = options().decode_lag;
    std::vector<std::int32_t> decoded_;        // decode_lag: [B][T_max], the fixed-lag rows so far (rows below L - lag are final)
    std::vector<std::size_t> dec_prev_;        // ... and the lengths they stand for
    std::size_t traj_stats_M_ = options().trajectory_stats;
    std::uint64_t traj_stats_draw_ = options().trajectory_stats_draw_index;
    std::vector<std::vector<double>> seen_;    // trajectory_stats: [b] = problem b's observes so far
    bool running_stats_ = options().running_stats;
    bool learn_ = options().learn_tables;
    bool scaled_ = false;                      // the tables carry emission scales
    bool poisson_ = false;                     // the tables' emission is Poisson
    std::size_t dump_max_ = options().dump_max_particles;
    std::vector<std::uint32_t> np_;
    ContextLease lease_;
};

}  // namespace gpu
}  // namespace cpprob
#endif
