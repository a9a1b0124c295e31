// batch_forecast_kernel and batch_predictive_kernel (csrc/batch_forecast.hpp) run as host code over a grid given in a case file
// (tests/test_batch_forecast_kernel_text_host.py writes it and states the format): every buffer is a heap block of exactly the size the
// host code would hand the kernel, the launch is a loop over its blocks, a block 256 threads.  "batch_forecast_host.hpp" is the
// kernels' text on top of batch_smooth.hpp's, with the shim in place of batch_smc.hpp.
#include "batch_forecast_host.hpp"

#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b46434153543031;      // "10TSACFK"
struct Header { int64_t magic, B, k, spp, thr_stride, hmm3, predictive, grid_y, mass_rows, thr_words, H, n_traj, rows, draw_index; };

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

cph::BatchForecastArgs g_args;
unsigned g_grid_x = 0, g_grid_y = 0;
bool g_hmm3 = false, g_predictive = false;

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    gridDim.x = g_grid_x; gridDim.y = g_grid_y; gridDim.z = 1;
    for (unsigned bx = 0; bx < g_grid_x; ++bx) {
        for (unsigned by = 0; by < g_grid_y; ++by) {
            pthread_barrier_wait(&hostk::g_group.all);
            blockIdx.x = bx; blockIdx.y = by; blockIdx.z = 0;
            if (g_predictive) cph::batch_predictive_kernel(g_args);
            else if (g_hmm3) cph::batch_forecast_kernel<3>(g_args);
            else cph::batch_forecast_kernel<8>(g_args);
            pthread_barrier_wait(&hostk::g_group.all);         // the workgroup is done
        }
    }
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_forecast_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.k >= 2 && h.k <= 8 && h.spp >= 1 && h.spp <= 8 && h.grid_y >= 1 && h.H >= 0 && h.n_traj >= 0 && h.rows >= 0, "header out of range");
    const size_t B = (size_t)h.B;
    const size_t n_marg = B * (size_t)h.rows * (size_t)h.spp, n_traj = h.predictive ? 0 : B * (size_t)(h.H + 1) * (size_t)h.n_traj;
    cph::BatchSmoothProblem* desc = exact_block<cph::BatchSmoothProblem>(B);
    uint64_t* thr = exact_block<uint64_t>((size_t)h.thr_words);
    double* mass = exact_block<double>((size_t)h.mass_rows * 8);
    uint64_t* seeds = exact_block<uint64_t>(B);
    double* marg = exact_block<double>(n_marg);                                     // (zeroed, as the caller hands it over)
    int8_t* traj = exact_block<int8_t>(n_traj);
    get(f, desc, B);
    get(f, thr, (size_t)h.thr_words);
    get(f, mass, (size_t)h.mass_rows * 8);
    get(f, seeds, B);
    std::fclose(f);
    for (size_t i = 0; i < n_traj; ++i) traj[i] = -7;                               // an entry nobody wrote shows

    g_args.desc = desc; g_args.mass = mass; g_args.thr = thr; g_args.seeds = seeds; g_args.marg = marg; g_args.traj = traj;
    g_args.draw_base = cph::kForecastDrawBase + ((uint64_t)h.draw_index << 24);
    g_args.k = (int)h.k; g_args.spp = (int)h.spp; g_args.thr_stride = (int)h.thr_stride; g_args.n_traj = (int)h.n_traj;
    g_args.H = (int)h.H; g_args.rows = (int)h.rows;
    g_grid_x = (unsigned)B; g_grid_y = (unsigned)h.grid_y;
    g_hmm3 = h.hmm3 != 0; g_predictive = h.predictive != 0;

    hostk::group_init();
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, marg, n_marg);
    put(o, traj, n_traj);
    need(std::fclose(o) == 0, "close");
    std::free(desc); std::free(thr); std::free(mass); std::free(seeds); std::free(marg); std::free(traj);
    return 0;
}
