// batch_online_stats_kernel (csrc/batch_onlinestats.hpp) run as host code over a grid given in a case file
// (tests/test_batch_onlinestats_kernel_text_host.py writes it and states the format): every buffer is a heap block of exactly the size
// the host code would hand the kernel, the launch is a loop over its blocks, a block 256 threads.  "batch_onlinestats_host.hpp" is the
// kernel's text on top of batch_smooth.hpp's, with the shim in place of batch_smc.hpp.
#include "batch_onlinestats_host.hpp"

#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b4f4e4c494e3031;      // "10NILNOK"
struct Header { int64_t magic, B, k, thr_stride, grid_x, mass_rows, thr_words, n_obs, with_obs; };

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

cph::BatchOnlineStatsArgs g_args;
unsigned g_grid_x = 0;

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    gridDim.x = g_grid_x; gridDim.y = 1; gridDim.z = 1;
    for (unsigned bx = 0; bx < g_grid_x; ++bx) {
        pthread_barrier_wait(&hostk::g_group.all);
        blockIdx.x = bx; blockIdx.y = 0; blockIdx.z = 0;
        cph::batch_online_stats_kernel(g_args);
        pthread_barrier_wait(&hostk::g_group.all);             // the workgroup is done
    }
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_onlinestats_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.k >= 1 && h.k <= 8 && h.grid_x >= 1, "header out of range");
    const size_t B = (size_t)h.B;
    cph::BatchSmoothProblem* desc = exact_block<cph::BatchSmoothProblem>(B);
    uint64_t* thr = exact_block<uint64_t>((size_t)h.thr_words);
    double* mass = exact_block<double>((size_t)h.mass_rows * 8);
    double* obs = exact_block<double>((size_t)h.n_obs);
    double* tau = exact_block<double>(B * cph::kOnlineTau);
    double* stats = exact_block<double>(B * cph::kOnlineStats);
    get(f, desc, B);
    get(f, thr, (size_t)h.thr_words);
    get(f, mass, (size_t)h.mass_rows * 8);
    get(f, obs, (size_t)h.n_obs);
    get(f, tau, B * cph::kOnlineTau);
    std::fclose(f);
    for (size_t i = 0; i < B * cph::kOnlineStats; ++i) stats[i] = -7.0;             // an entry nobody wrote shows

    g_args.desc = desc; g_args.mass = mass; g_args.thr = thr; g_args.obs = h.with_obs ? obs : nullptr; g_args.tau = tau; g_args.stats = stats;
    g_args.B = (int)h.B; g_args.k = (int)h.k; g_args.thr_stride = (int)h.thr_stride;
    g_grid_x = (unsigned)h.grid_x;

    hostk::group_init();
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, stats, B * cph::kOnlineStats);
    put(o, tau, B * cph::kOnlineTau);
    need(std::fclose(o) == 0, "close");
    std::free(desc); std::free(thr); std::free(mass); std::free(obs); std::free(tau); std::free(stats);
    return 0;
}
