// csrc/batch_pass_plan.hpp as a host program: reads cases (tests/test_batch_pass_plan_host.py writes them and states the format),
// builds each BatchPass through its named constructor, calls batch_pass_plan and -- unless the plan says the call is done --
// batch_pass_describe, and prints what they decided.  Every array is a heap block of exactly the problems' number, so that a read or
// a descriptor written past it is the sanitizers' to report.  The output pointers are never read through: the plan asks only
// whether one is there.
#include "batch_pass_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
struct Problem { int32_t T, n; int64_t store; };
struct Desc { int32_t T, n; int64_t store, rows, trows; int32_t cfrom, cto, lo, mfrom; };

void need(bool ok, const char* what)
{
    if (!ok) { std::fprintf(stderr, "case file: %s\n", what); std::exit(2); }
}
long long get(std::FILE* f)
{
    long long v = 0;
    need(std::fscanf(f, "%lld", &v) == 1, "short read");
    return v;
}
template <class T> T* exact_block(size_t n) { return static_cast<T*>(std::calloc(n, sizeof(T))); }
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 2, "usage: batch_pass_plan_host CASES");
    std::FILE* f = std::fopen(argv[1], "r");
    need(f != nullptr, "cannot open the cases");
    static double some_doubles[1];
    static int8_t some_entries[1];
    const long long cases = get(f);
    for (long long i = 0; i < cases; ++i) {
        const int kind = (int)get(f);
        const size_t B = (size_t)get(f);
        const bool online = get(f) != 0, kept = get(f) != 0;
        const int T_max = (int)get(f), spp = (int)get(f);
        const uint64_t lag = (uint64_t)get(f);
        const bool with_from = get(f) != 0;
        const uint64_t n_rows = (uint64_t)get(f), horizon = (uint64_t)get(f), n_traj = (uint64_t)get(f);
        double* const doubles = get(f) ? some_doubles : nullptr;              // d_marg, or d_score
        int8_t* const entries = get(f) ? some_entries : nullptr;              // d_traj, or d_path
        need(B >= 1 && kind >= BatchPass::Smooth && kind <= BatchPass::DecodeLag, "header out of range");
        Problem* prob = exact_block<Problem>(B);
        uint32_t* cap_T = exact_block<uint32_t>(B);
        uint32_t* counted = exact_block<uint32_t>(B);
        uint32_t* decoded = exact_block<uint32_t>(B);
        uint32_t* ostats_done = exact_block<uint32_t>(B);
        uint32_t* from = exact_block<uint32_t>(B);
        Desc* pd = exact_block<Desc>(B);
        for (size_t b = 0; b < B; ++b) {
            prob[b].T = (int32_t)get(f); prob[b].n = (int32_t)get(f); prob[b].store = (int64_t)get(f);
            cap_T[b] = (uint32_t)get(f); counted[b] = (uint32_t)get(f); decoded[b] = (uint32_t)get(f); ostats_done[b] = (uint32_t)get(f); from[b] = (uint32_t)get(f);
        }
        const uint32_t* fr = with_from ? from : nullptr;
        BatchPass p{};
        switch (kind) {
        case BatchPass::Smooth: p = BatchPass::smooth(n_traj, 5, doubles, entries); break;
        case BatchPass::SmoothLag: p = BatchPass::smooth_lag(lag, fr, n_rows, n_traj, 5, doubles, entries); break;
        case BatchPass::Stats: p = BatchPass::stats(some_doubles, some_doubles); break;
        case BatchPass::TrajStats: p = BatchPass::traj_stats(n_traj, 5, some_doubles, some_doubles); break;
        case BatchPass::OnlineStats: p = BatchPass::online_stats(some_doubles, some_doubles); break;
        case BatchPass::Forecast: p = BatchPass::forecast(horizon, n_traj, 5, doubles, entries); break;
        case BatchPass::Predictive: p = BatchPass::predictive(fr, n_rows, doubles); break;
        case BatchPass::Decode: p = BatchPass::decode(doubles, entries); break;
        default: p = BatchPass::decode_lag(lag, fr, n_rows, doubles, entries); break;
        }
        need((int)p.kind == kind, "the constructor names another pass");
        // an online batch alone has capacities and the watermarks of its tables (the running statistics serve no other, but read theirs)
        const BatchPassBatch<Problem> bt{B, prob, online ? cap_T : nullptr, online ? counted : nullptr, online ? decoded : nullptr, ostats_done, online, kept, T_max, spp};
        BatchPassPlan pl = batch_pass_plan(bt, p);
        std::printf("case %lld\nhead %zu %zu %zu %zu %zu %zu %zu %zu %d\n", i, pl.marg_rows, pl.marg_bytes, pl.stats_bytes, pl.traj_bytes, pl.score_bytes, pl.path_bytes,
                    pl.mass_rows, pl.word_rows, pl.done ? 1 : 0);
        if (!pl.done) {
            batch_pass_describe(bt, p, pd, pl);
            std::printf("tail %zu %d %d %u %u %u %u %u %u %u %u %u\n", pl.fresh, pl.lag, pl.lds_bytes, pl.count_gy, pl.lag_gy, pl.smooth_gy, pl.stats_gx, pl.traj_stats_gy,
                        pl.forecast_gy, pl.predictive_gy, pl.decode_gx, pl.trace_gy);
            for (size_t b = 0; b < B; ++b)
                std::printf("desc %d %d %lld %lld %lld %d %d %d %d\n", pd[b].T, pd[b].n, (long long)pd[b].store, (long long)pd[b].rows, (long long)pd[b].trows, pd[b].cfrom, pd[b].cto,
                            pd[b].lo, pd[b].mfrom);
        }
        std::free(prob); std::free(cap_T); std::free(counted); std::free(decoded); std::free(ostats_done); std::free(from); std::free(pd);
    }
    std::fclose(f);
    return 0;
}
