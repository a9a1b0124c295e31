// batch_learn_rows_scaled_kernel and batch_learn_scaled_kernel (csrc/batch_learn.hpp) run as host code over grids given in a
// case file (tests/test_batch_learn_scaled_kernel_text_host.py writes it and states the format): every buffer is a heap block of
// exactly the size the host code would hand the kernels, a launch is a loop over its blocks, a block 256 threads.
// "batch_learn_host.hpp" is the kernels' text on top of batch_onlinestats.hpp's and batch_scale.hpp's, with the shims in place of
// batch_smc.hpp.  batch_learn_main.cpp with the scales: the sigmas and log_norms [B][8] in and out, the floor and the fit flag.
#include "batch_learn_host.hpp"

#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b4c524e53433031;      // "10CSNRLK"
struct Header { int64_t magic, B, k, t_min, grid_x, mass_rows, n_obs, n_gamma, T_max, rows_grid_y, fit; };

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

cph::BatchLearnScaledArgs g_args;
cph::BatchLearnRowsScaledArgs g_rows;
unsigned g_grid_x = 0, g_rows_gy = 0, g_B = 0;

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    // the rows launch: blockIdx.x the problem, blockIdx.y the tile
    gridDim.x = g_B; gridDim.y = g_rows_gy; gridDim.z = 1;
    for (unsigned bx = 0; bx < g_B; ++bx)
        for (unsigned by = 0; by < g_rows_gy; ++by) {
            pthread_barrier_wait(&hostk::g_group.all);
            blockIdx.x = bx; blockIdx.y = by; blockIdx.z = 0;
            cph::batch_learn_rows_scaled_kernel(g_rows);
            pthread_barrier_wait(&hostk::g_group.all);         // the workgroup is done
        }
    gridDim.x = g_grid_x; gridDim.y = 1; gridDim.z = 1;
    for (unsigned bx = 0; bx < g_grid_x; ++bx) {
        pthread_barrier_wait(&hostk::g_group.all);
        blockIdx.x = bx; blockIdx.y = 0; blockIdx.z = 0;
        cph::batch_learn_scaled_kernel(g_args);
        pthread_barrier_wait(&hostk::g_group.all);
    }
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_learn_scaled_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.k >= 2 && h.k <= 8 && h.grid_x >= 1 && h.rows_grid_y >= 1 && h.T_max >= 1, "header out of range");
    const size_t B = (size_t)h.B, k = (size_t)h.k, n_tab = B * (size_t)h.T_max * 8;
    cph::BatchSmoothProblem* desc = exact_block<cph::BatchSmoothProblem>(B);
    cph::BatchProblem* prob = exact_block<cph::BatchProblem>(B);
    int32_t* first = exact_block<int32_t>(B);
    int64_t* ofirst = exact_block<int64_t>(B);
    uint64_t* thr = exact_block<uint64_t>(B * 64);
    double* mass = exact_block<double>((size_t)h.mass_rows * 8);
    double* obs = exact_block<double>((size_t)h.n_obs);
    double* gamma = exact_block<double>((size_t)h.n_gamma);
    double* tau = exact_block<double>(B * cph::kOnlineTau);
    double* means = exact_block<double>(B * k);
    double* trans = exact_block<double>(B * k * k);
    int32_t* status = exact_block<int32_t>(B);
    double* tab = exact_block<double>(n_tab);
    double* stats = exact_block<double>(B * cph::kOnlineStats);
    double* sigmas = exact_block<double>(B * 8);
    double* log_norms = exact_block<double>(B * 8);
    double floor = 0.0;
    get(f, desc, B); get(f, prob, B); get(f, first, B); get(f, ofirst, B);
    get(f, thr, B * 64);
    get(f, mass, (size_t)h.mass_rows * 8);
    get(f, obs, (size_t)h.n_obs);
    get(f, gamma, (size_t)h.n_gamma);
    get(f, tau, B * cph::kOnlineTau);
    get(f, means, B * k); get(f, trans, B * k * k);
    get(f, status, B);
    get(f, tab, n_tab);
    get(f, sigmas, B * 8); get(f, log_norms, B * 8);
    get(f, &floor, 1);
    std::fclose(f);
    for (size_t i = 0; i < B * cph::kOnlineStats; ++i) stats[i] = -7.0;             // an entry nobody wrote shows

    g_rows.prob = prob; g_rows.first = first; g_rows.ofirst = ofirst; g_rows.means = means; g_rows.obs = obs; g_rows.tab = tab;
    g_rows.sigmas = sigmas; g_rows.log_norms = log_norms; g_rows.T_max = (int)h.T_max; g_rows.k = (int)h.k;
    cph::BatchLearnArgs& la = g_args.base;
    la.desc = desc; la.mass = mass; la.thr = thr; la.obs = obs; la.gamma = gamma; la.tau = tau; la.stats = stats;
    la.means = means; la.trans = trans; la.status = status;
    la.B = (int)h.B; la.k = (int)h.k; la.t_min = (int)h.t_min;
    g_args.sigmas = sigmas; g_args.log_norms = log_norms; g_args.floor = floor; g_args.fit = (int)h.fit;
    g_grid_x = (unsigned)h.grid_x; g_rows_gy = (unsigned)h.rows_grid_y; g_B = (unsigned)h.B;

    hostk::group_init();
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, stats, B * cph::kOnlineStats);
    put(o, tau, B * cph::kOnlineTau);
    put(o, means, B * k); put(o, trans, B * k * k);
    put(o, thr, B * 64);
    put(o, status, B);
    put(o, tab, n_tab);
    put(o, sigmas, B * 8); put(o, log_norms, B * 8);
    need(std::fclose(o) == 0, "close");
    std::free(desc); std::free(prob); std::free(first); std::free(ofirst); std::free(thr); std::free(mass); std::free(obs); std::free(gamma);
    std::free(tau); std::free(means); std::free(trans); std::free(status); std::free(tab); std::free(stats); std::free(sigmas); std::free(log_norms);
    return 0;
}
