// batch_traj_stats_kernel (csrc/batch_trajstats.hpp) run as host code over a grid given in a case file
// (tests/test_batch_trajstats_kernel_text_host.py writes it and states the format): every buffer is a heap block of exactly the size the
// host code would hand the kernel, the launch is a loop over its blocks, a block 256 threads, a workgroup's dynamic LDS a fresh heap
// block of the launch's size.  "batch_trajstats_host.hpp" is the kernel's text on top of batch_smooth.hpp's, with the shim in place of
// batch_smc.hpp.
#include "batch_trajstats_host.hpp"

#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b54524a53543031;      // "10TSJRTK"
struct Header {
    int64_t magic, B, k, thr_stride, n_traj, lds_bytes, grid_y, mass_rows, thr_words, n_obs, with_obs, hmm3;
    uint64_t draw_base;
};

template <class T> T* exact_block(size_t n)
{
    // exactly n elements, so that the first element past the end is poisoned
    return n ? static_cast<T*>(std::calloc(n, sizeof(T))) : nullptr;
}

void need(bool ok, const char* what)
{
    if (!ok) { std::fprintf(stderr, "case file: %s\n", what); std::exit(2); }
}
template <class T> void get(std::FILE* f, T* p, size_t n) { need(n == 0 || std::fread(p, sizeof(T), n, f) == n, "short read"); }
template <class T> void put(std::FILE* f, const T* p, size_t n) { need(n == 0 || std::fwrite(p, sizeof(T), n, f) == n, "short write"); }

cph::BatchTrajStatsArgs g_args;
unsigned g_grid_x = 0, g_grid_y = 0;
bool g_hmm3 = false;

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    gridDim.x = g_grid_x; gridDim.y = g_grid_y; gridDim.z = 1;
    for (unsigned by = 0; by < g_grid_y; ++by)
        for (unsigned bx = 0; bx < g_grid_x; ++bx) {
            if (threadIdx.x == 0) {
                std::free(hostk::g_group.dynamic_lds);
                hostk::g_group.dynamic_lds = exact_block<double>((size_t)g_args.lds_bytes / sizeof(double));
            }
            pthread_barrier_wait(&hostk::g_group.all);
            blockIdx.x = bx; blockIdx.y = by; blockIdx.z = 0;
            if (g_hmm3) cph::batch_traj_stats_kernel<3>(g_args);
            else cph::batch_traj_stats_kernel<8>(g_args);
            pthread_barrier_wait(&hostk::g_group.all);         // the workgroup is done: the statics stand for the next one's LDS
        }
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_trajstats_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.k >= 1 && h.k <= 8 && h.n_traj >= 1 && h.grid_y >= 1 && h.lds_bytes >= 0 && h.lds_bytes % 8 == 0, "header out of range");
    need(h.grid_y * cph::kTrajStatsTile >= h.n_traj, "the grid does not cover the trajectories");
    const size_t B = (size_t)h.B, n_stats = B * (size_t)h.n_traj * cph::kTrajStats;
    cph::BatchSmoothProblem* desc = exact_block<cph::BatchSmoothProblem>(B);
    uint64_t* thr = exact_block<uint64_t>((size_t)h.thr_words);
    uint64_t* seeds = exact_block<uint64_t>(B);
    double* mass = exact_block<double>((size_t)h.mass_rows * 8);
    double* obs = exact_block<double>((size_t)h.n_obs);
    double* stats = exact_block<double>(n_stats);
    get(f, desc, B);
    get(f, thr, (size_t)h.thr_words);
    get(f, seeds, B);
    get(f, mass, (size_t)h.mass_rows * 8);
    get(f, obs, (size_t)h.n_obs);
    std::fclose(f);
    for (size_t i = 0; i < n_stats; ++i) stats[i] = -7.0;                               // an entry nobody wrote shows

    g_args.desc = desc; g_args.mass = mass; g_args.thr = thr; g_args.seeds = seeds; g_args.obs = h.with_obs ? obs : nullptr; g_args.stats = stats;
    g_args.draw_base = h.draw_base;
    g_args.k = (int)h.k; g_args.thr_stride = (int)h.thr_stride; g_args.n_traj = (int)h.n_traj; g_args.lds_bytes = (int)h.lds_bytes;
    g_grid_x = (unsigned)B; g_grid_y = (unsigned)h.grid_y; g_hmm3 = h.hmm3 != 0;

    hostk::group_init();
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);
    std::free(hostk::g_group.dynamic_lds);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, stats, n_stats);
    need(std::fclose(o) == 0, "close");
    std::free(desc); std::free(thr); std::free(seeds); std::free(mass); std::free(obs); std::free(stats);
    return 0;
}
