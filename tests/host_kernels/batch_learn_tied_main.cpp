// The three launches of a tied learning advance behind its run -- batch_learn_kernel or batch_learn_scaled_kernel with t_min = INT32_MAX
// (csrc/batch_learn.hpp), batch_pool_stats_kernel in compact form with R = 1 (csrc/batch_pool.hpp), batch_learn_tied_kernel or
// batch_learn_tied_scaled_kernel (csrc/batch_learn_tied.hpp) -- run as host code over a case file
// (tests/test_batch_learn_tied_kernel_text_host.py writes it and states the format): every buffer is a heap block of exactly the size
// the host code would hand the kernels, a launch is a loop over its blocks, a block 256 threads.  "batch_learn_tied_host.hpp" is the
// new header's text on top of batch_learn.hpp's and batch_pool.hpp's, with the shims in place of batch_smc.hpp.
#include "batch_learn_tied_host.hpp"

#include <climits>
#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b4c544945443031;      // "10DEITLK"
struct Header { int64_t magic, B, k, t_min, G, mass_rows, n_obs, n_gamma, scaled, fit, learn_grid_x; };

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

cph::BatchLearnScaledArgs g_learn;
cph::BatchPoolArgs g_pool;
cph::BatchLearnTiedScaledArgs g_tied;
unsigned g_learn_gx = 0, g_groups_gx = 0;
bool g_scaled = false;

template <class Launch> void launch(unsigned grid_x, Launch one)
{
    gridDim.x = grid_x; gridDim.y = 1; gridDim.z = 1;
    for (unsigned bx = 0; bx < grid_x; ++bx) {
        pthread_barrier_wait(&hostk::g_group.all);
        blockIdx.x = bx; blockIdx.y = 0; blockIdx.z = 0;
        one();
        pthread_barrier_wait(&hostk::g_group.all);             // the workgroup is done
    }
}

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    // the order of batch_learn_enqueue's tied branch: learn, pool, tied; the grids ceil(G / kWaves) are the library's
    launch(g_learn_gx, [] { if (g_scaled) cph::batch_learn_scaled_kernel(g_learn); else cph::batch_learn_kernel(g_learn.base); });
    launch(g_groups_gx, [] { cph::batch_pool_stats_kernel(g_pool); });
    launch(g_groups_gx, [] { if (g_scaled) cph::batch_learn_tied_scaled_kernel(g_tied); else cph::batch_learn_tied_kernel(g_tied.base); });
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_learn_tied_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.k >= 2 && h.k <= 8 && h.G >= 1 && h.G <= h.B && h.learn_grid_x >= 1 && h.t_min >= 0, "header out of range");
    const size_t B = (size_t)h.B, k = (size_t)h.k, G = (size_t)h.G;
    cph::BatchSmoothProblem* desc = exact_block<cph::BatchSmoothProblem>(B);
    int32_t* members = exact_block<int32_t>(B);
    int32_t* first = exact_block<int32_t>(G + 1);
    uint64_t* thr = exact_block<uint64_t>(B * 64);
    double* mass = exact_block<double>((size_t)h.mass_rows * 8);
    double* obs = exact_block<double>((size_t)h.n_obs);
    double* gamma = exact_block<double>((size_t)h.n_gamma);
    double* tau = exact_block<double>(B * cph::kOnlineTau);
    double* means = exact_block<double>(B * k);
    double* trans = exact_block<double>(B * k * k);
    int32_t* status = exact_block<int32_t>(B);
    double* stats = exact_block<double>(B * cph::kOnlineStats);
    double* pooled = exact_block<double>(G * cph::kPoolStats);
    double* sigmas = h.scaled ? exact_block<double>(B * 8) : nullptr;               // (a unit batch hands the kernels no scales)
    double* log_norms = h.scaled ? exact_block<double>(B * 8) : nullptr;
    double floor = 0.0;
    get(f, desc, B); get(f, members, B); get(f, first, G + 1);
    get(f, thr, B * 64);
    get(f, mass, (size_t)h.mass_rows * 8);
    get(f, obs, (size_t)h.n_obs);
    get(f, gamma, (size_t)h.n_gamma);
    get(f, tau, B * cph::kOnlineTau);
    get(f, means, B * k); get(f, trans, B * k * k);
    get(f, status, B);
    if (h.scaled) { get(f, sigmas, B * 8); get(f, log_norms, B * 8); }
    get(f, &floor, 1);
    std::fclose(f);
    for (size_t i = 0; i < B * cph::kOnlineStats; ++i) stats[i] = -7.0;             // an entry nobody wrote shows
    for (size_t i = 0; i < G * cph::kPoolStats; ++i) pooled[i] = -9.0;

    cph::BatchLearnArgs& la = g_learn.base;
    la.desc = desc; la.mass = mass; la.thr = thr; la.obs = obs; la.gamma = gamma; la.tau = tau; la.stats = stats;
    la.means = means; la.trans = trans; la.status = status;
    la.B = (int)h.B; la.k = (int)h.k; la.t_min = INT_MAX;
    g_learn.sigmas = sigmas; g_learn.log_norms = log_norms; g_learn.floor = floor; g_learn.fit = (int)h.fit;
    g_pool.members = members; g_pool.first = first; g_pool.rec = stats; g_pool.out = pooled; g_pool.pairs = h.G; g_pool.R = 1; g_pool.broadcast = 0;
    cph::BatchLearnTiedArgs& ta = g_tied.base;
    ta.members = members; ta.first = first; ta.desc = desc; ta.pooled = pooled; ta.thr = thr; ta.means = means; ta.trans = trans; ta.status = status;
    ta.t_min = h.t_min; ta.G = (int)h.G; ta.k = (int)h.k;
    g_tied.sigmas = sigmas; g_tied.log_norms = log_norms; g_tied.floor = floor; g_tied.fit = (int)h.fit;
    g_learn_gx = (unsigned)h.learn_grid_x; g_groups_gx = (unsigned)((h.G + cph::kWaves - 1) / cph::kWaves); g_scaled = h.scaled != 0;

    hostk::group_init();
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, stats, B * cph::kOnlineStats);
    put(o, pooled, G * cph::kPoolStats);
    put(o, tau, B * cph::kOnlineTau);
    put(o, means, B * k); put(o, trans, B * k * k);
    put(o, thr, B * 64);
    put(o, status, B);
    if (h.scaled) { put(o, sigmas, B * 8); put(o, log_norms, B * 8); }
    need(std::fclose(o) == 0, "close");
    std::free(desc); std::free(members); std::free(first); std::free(thr); std::free(mass); std::free(obs); std::free(gamma);
    std::free(tau); std::free(means); std::free(trans); std::free(status); std::free(stats); std::free(pooled); std::free(sigmas); std::free(log_norms);
    return 0;
}
