// The plan of one batch pass (batch_smooth_enqueue in cpprob_hip.hip): what a call asks for (BatchPass) and, from the batch's lengths,
// capacities and watermarks, everything the enqueue decides on the host -- the output memsets, the early return, the table sizes, the
// problems' descriptors and every grid.  Plain C++17 without HIP and without the context: tests/test_batch_pass_plan_host.py builds
// it as a host program and compares it with tests/pass_plan_ref.py.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

// One call's pass and its own arguments; the pointers are device buffers (an output not asked for, or no observes: nullptr).
struct BatchPass {
    enum Kind { Smooth, SmoothLag, Stats, TrajStats, OnlineStats, Forecast, Predictive, Decode, DecodeLag } kind;
    const uint32_t* from = nullptr;            // [B], the first rows wanted (SmoothLag, Predictive, DecodeLag; nullptr: 0)
    uint64_t lag = 0, n_rows = 0, horizon = 0, n_traj = 0, draw_index = 0;      // n_rows: the rows a problem of the output, where from is taken
    double* d_marg = nullptr; int8_t* d_traj = nullptr; const double* d_obs = nullptr; double* d_stats = nullptr; double* d_score = nullptr; int8_t* d_path = nullptr;

    static BatchPass smooth(uint64_t n_traj, uint64_t draw_index, double* d_marg, int8_t* d_traj)
    { BatchPass p{Smooth}; p.n_traj = n_traj; p.draw_index = draw_index; p.d_marg = d_marg; p.d_traj = d_traj; return p; }
    static BatchPass smooth_lag(uint64_t lag, const uint32_t* from, uint64_t n_rows, uint64_t n_traj, uint64_t draw_index, double* d_marg, int8_t* d_traj)
    { BatchPass p = smooth(n_traj, draw_index, d_marg, d_traj); p.kind = SmoothLag; p.lag = lag; p.from = from; p.n_rows = n_rows; return p; }
    static BatchPass stats(const double* d_obs, double* d_stats) { BatchPass p{Stats}; p.d_obs = d_obs; p.d_stats = d_stats; return p; }
    static BatchPass traj_stats(uint64_t n_traj, uint64_t draw_index, const double* d_obs, double* d_stats)
    { BatchPass p = stats(d_obs, d_stats); p.kind = TrajStats; p.n_traj = n_traj; p.draw_index = draw_index; return p; }
    static BatchPass online_stats(const double* d_obs, double* d_stats) { BatchPass p = stats(d_obs, d_stats); p.kind = OnlineStats; return p; }
    static BatchPass forecast(uint64_t horizon, uint64_t n_traj, uint64_t draw_index, double* d_marg, int8_t* d_traj)
    { BatchPass p = smooth(n_traj, draw_index, d_marg, d_traj); p.kind = Forecast; p.horizon = horizon; return p; }
    static BatchPass predictive(const uint32_t* from, uint64_t n_rows, double* d_rows)
    { BatchPass p{Predictive}; p.from = from; p.n_rows = n_rows; p.d_marg = d_rows; return p; }
    static BatchPass decode(double* d_score, int8_t* d_path) { BatchPass p{Decode}; p.d_score = d_score; p.d_path = d_path; return p; }
    static BatchPass decode_lag(uint64_t lag, const uint32_t* from, uint64_t n_rows, double* d_score, int8_t* d_path)
    { BatchPass p = decode(d_score, d_path); p.kind = DecodeLag; p.lag = lag; p.from = from; p.n_rows = n_rows; return p; }

    bool lagged() const { return kind == SmoothLag; }                       bool forecasts() const { return kind == Forecast || kind == Predictive; }
    bool decodes() const { return kind == Decode || kind == DecodeLag; }    bool with_traj() const { return d_traj && n_traj; }
};

// The kernels' constants the plan reckons with; cpprob_hip.hip asserts each against the kernel headers' own.
namespace batch_pass_limits {
constexpr int kThreads = 256, kWaves = 4, kTile = 1024, kTrajStatsTile = 256, kStats = 88, kBackwardMaxT = 1 << 24, kBackwardLdsMax = 32768,
              kSmoothCountGroups = 8192, kSmoothLagGridMax = 4096, kPredictiveGridMax = 4096, kDecodeTraceGridMax = 4096;
}

// The batch as the plan reads it.  prob: [B] of {T (the length reached), n, store}; cap_T: [B], an online batch's capacities; counted,
// decoded, ostats_done: [B], an online batch's watermarks (rows of the m table counted, step words written, steps in tau); kept: the
// run left the m table in the workspace (batch_masses); spp: the doubles a row of marginals.
template <class Prob> struct BatchPassBatch {
    size_t B; const Prob* prob; const uint32_t* cap_T; const uint32_t* counted; const uint32_t* decoded; const uint32_t* ostats_done; bool online, kept; int T_max, spp;
};

struct BatchPassPlan {
    // batch_pass_plan: the memsets in their stream order (bytes, 0: none; path_bytes of 0xff, the others of 0), the rows of the context's
    // m table and of the word table; done: the call ends after the memsets, no launch
    size_t marg_rows = 0, marg_bytes = 0, stats_bytes = 0, traj_bytes = 0, score_bytes = 0, path_bytes = 0, mass_rows = 0, word_rows = 0;
    bool done = false;
    // batch_pass_describe: the observes an OnlineStats pass consumes, the kernels' lag and dynamic LDS, the grids (0: no launch)
    size_t fresh = 0; int lag = 0, lds_bytes = 0;
    unsigned count_gy = 0, lag_gy = 0, smooth_gy = 0, stats_gx = 0, traj_stats_gy = 0, forecast_gy = 0, predictive_gy = 0, decode_gx = 0, trace_gy = 0;
};

// What needs no descriptor, so that the enqueue can set its outputs, leave or grow its tables before it owns a pinned slot.
template <class Prob> BatchPassPlan batch_pass_plan(const BatchPassBatch<Prob>& bt, const BatchPass& p)
{
    using namespace batch_pass_limits;
    BatchPassPlan pl;
    const size_t B = bt.B; const bool predictive = p.kind == BatchPass::Predictive;
    pl.marg_rows = p.forecasts() ? (size_t)(predictive ? p.n_rows : p.horizon) : p.lagged() ? (size_t)p.n_rows : (size_t)bt.T_max;
    if (p.d_marg && pl.marg_rows) pl.marg_bytes = B * pl.marg_rows * (size_t)bt.spp * sizeof(double);   // rows past the problem's, states >= k
    size_t rows = 0, reached = 0;
    for (size_t b = 0; b < B; ++b) { reached += (size_t)bt.prob[b].T; rows += bt.online ? (size_t)bt.cap_T[b] : (size_t)bt.prob[b].T; }
    if ((p.kind == BatchPass::Stats || p.kind == BatchPass::OnlineStats) && reached == 0) pl.stats_bytes = B * (size_t)kStats * sizeof(double);
    if (p.kind == BatchPass::TrajStats && reached == 0) pl.stats_bytes = B * (size_t)p.n_traj * (size_t)kStats * sizeof(double);
    // a forecast before the first observes: rows of zeros; the predictive row 0 needs no row of the table and goes on
    if (p.kind == BatchPass::Forecast && reached == 0 && p.with_traj()) pl.traj_bytes = B * (size_t)(p.horizon + 1) * (size_t)p.n_traj;
    // a decode: a problem of length 0 has score 0; the fixed-lag rows no step owns are -1 (0 is a state)
    if (p.decodes() && p.d_score) pl.score_bytes = B * sizeof(double);
    if (p.kind == BatchPass::DecodeLag && p.d_path && p.n_rows) pl.path_bytes = B * (size_t)p.n_rows;
    // an online batch before its first observes, or nothing asked for (Stats, TrajStats, OnlineStats, Decode and DecodeLag always have an output)
    pl.done = (reached == 0 && !predictive) || ((p.kind == BatchPass::Smooth || p.lagged() || p.forecasts()) && !p.d_marg && !p.with_traj());
    // kept: the run wrote the m table into the workspace, rows by T_max as the per-step tables'; nothing to count, no table of the context's own
    pl.word_rows = bt.kept ? B * (size_t)bt.T_max : rows; pl.mass_rows = bt.kept ? 0 : rows;
    return pl;
}

// The problems' descriptors into pd ([B] of BatchSmoothProblem's fields) and what follows from them: the grids.
template <class Prob, class Desc> void batch_pass_describe(const BatchPassBatch<Prob>& bt, const BatchPass& p, Desc* pd, BatchPassPlan& pl)
{
    using namespace batch_pass_limits;
    const size_t B = bt.B;
    const bool lg = p.lagged(), fc = p.forecasts(), dc = p.decodes(), os = p.kind == BatchPass::OnlineStats, predictive = p.kind == BatchPass::Predictive;
    pl.lag = lg ? (int)p.lag : dc ? (int)std::min<uint64_t>(p.lag, (uint64_t)kBackwardMaxT) : 0;
    int64_t at = 0, at_traj = 0, at_fresh = 0, items_top = 0, lane_items = 0, owed = 0;
    int range_top = 0, W_top = 0;
    for (size_t b = 0; b < B; ++b) {
        const Prob& pr = bt.prob[b];
        const int L = pr.T, W = lg ? (int)std::min<uint64_t>(p.lag + 1, (uint64_t)L) : L;
        const int mfrom = p.from ? (int)p.from[b] : 0;
        pd[b].T = L; pd[b].n = pr.n; pd[b].store = pr.store; pd[b].rows = at; pd[b].trows = at_traj;
        pd[b].lo = L - W; pd[b].mfrom = mfrom; pd[b].cto = L;
        // lo's second meaning, under Decode, DecodeLag and OnlineStats: the first step the forward pass walks (the words, or tau, hold
        // the steps before it).  trows' second meaning, under OnlineStats: the problem's first observe among the fresh ones, packed.
        if (dc) pd[b].lo = bt.online ? (int)std::min<uint32_t>(bt.decoded[b], (uint32_t)L) : 0;
        if (os) {
            pd[b].lo = (int)std::min<uint32_t>(bt.ostats_done[b], (uint32_t)L);
            pd[b].trows = at_fresh;
            at_fresh += L - pd[b].lo;
        }
        // the rows the pass owes: an online batch's new ones; a run batch's -- nothing is kept -- those this call reads
        if (bt.kept) { pd[b].rows = (int64_t)b * bt.T_max; pd[b].store = 0; pd[b].cfrom = L; }
        else if (bt.online) pd[b].cfrom = (int)bt.counted[b];
        else if (fc) pd[b].cfrom = predictive ? std::min(std::max(mfrom, 1) - 1, L) : std::max(L - 1, 0);
        else pd[b].cfrom = lg ? std::min(p.d_marg ? mfrom : L, p.with_traj() ? L - W : L) : 0;
        at += bt.online ? (int64_t)bt.cap_T[b] : (int64_t)L;
        at_traj += W;
        range_top = std::max(range_top, pd[b].cto - pd[b].cfrom);
        W_top = std::max(W_top, W);
        if (lg && mfrom < L) items_top = std::max<int64_t>(items_top, std::max<int64_t>(1, (int64_t)L - mfrom - (int64_t)p.lag));
        if (p.kind == BatchPass::DecodeLag) lane_items = std::max<int64_t>(lane_items, (int64_t)L - 1 - (int64_t)mfrom - (int64_t)pl.lag);
        if (predictive) owed = std::max<int64_t>(owed, (int64_t)L + 1 - (int64_t)mfrom);
    }
    pl.fresh = (size_t)at_fresh;
    pl.lds_bytes = (int)std::min<int64_t>((int64_t)W_top * 64, kBackwardLdsMax);
    const unsigned waves = (unsigned)((B + kWaves - 1) / kWaves), tiles = p.with_traj() ? (unsigned)((p.n_traj + kTile - 1) / kTile) : 0u;
    // the counting pass: at least ~kSmoothCountGroups workgroups where the batch owes that many rows, a workgroup walking the rows gridDim.y apart
    if (range_top > 0 && !bt.kept) pl.count_gy = (unsigned)std::min<uint64_t>((uint64_t)range_top, std::max<uint64_t>(8, ((uint64_t)kSmoothCountGroups + B - 1) / B));
    // SmoothLag: (problem, end step) a wavefront, the ends gridDim.y * kWaves apart where a problem has more than the grid holds; then
    // the window's trajectories only.  Predictive: (problem, step) a wavefront, strided likewise where a problem owes more rows.
    if (lg && p.d_marg && items_top > 0) pl.lag_gy = (unsigned)std::min<int64_t>((items_top + kWaves - 1) / kWaves, kSmoothLagGridMax);
    if (p.kind == BatchPass::Smooth || (lg && tiles)) pl.smooth_gy = 1 + tiles;
    if (p.kind == BatchPass::Forecast) pl.forecast_gy = 1 + tiles;
    if (predictive && owed > 0) pl.predictive_gy = (unsigned)std::min<int64_t>((owed + kWaves - 1) / kWaves, kPredictiveGridMax);
    if (p.kind == BatchPass::Stats || os) pl.stats_gx = waves;              // a wavefront a problem
    // a lane a trajectory: the tiles cover n_traj, a problem of length 0 writes its zero records
    if (p.kind == BatchPass::TrajStats) pl.traj_stats_gy = (unsigned)((p.n_traj + kTrajStatsTile - 1) / kTrajStatsTile);
    // the forward pass: a wavefront a problem; it also leaves the score, so it runs where no step is new.  The trace, row 0 of the
    // grid: the item of end L - 1; the ends before it a lane each, (gridDim.y - 1) * kThreads apart
    if (dc) pl.decode_gx = waves;
    if (dc && p.d_path) pl.trace_gy = 1u + (unsigned)std::min<int64_t>((lane_items + kThreads - 1) / kThreads, kDecodeTraceGridMax);
}
