// batch_retable_poisson_kernel and batch_mstep_poisson_kernel (csrc/batch_poisson.hpp) run as host code over a grid given in a case file
// (tests/test_batch_poisson_kernel_text_host.py writes it and states the format): every buffer is a heap block of exactly the size the
// host code would hand the kernel, a launch is a loop over its blocks, a block 256 threads.  "batch_poisson.hpp", "batch_scale.hpp" and
// "batch_retable.hpp" are the headers' own text, the last with the shim in place of batch_smc.hpp.  The log-factorials are filled by
// poisson_log_fact_table, as the library fills them, into a block of exactly kPoissonMaxCount + 1 doubles.
#include "batch_poisson.hpp"

#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b504f4953533031;      // "10SSIOPK"
struct Header { int64_t magic, B, k, T_max, grid_y, n_obs; };

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

cph::BatchRetablePoissonArgs g_args;
cph::BatchMstepPoissonArgs g_mstep;
unsigned g_grid_x = 0, g_grid_y = 0, g_mstep_grid = 0;

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    gridDim.x = g_grid_x; gridDim.y = g_grid_y; gridDim.z = 1;
    for (unsigned by = 0; by < g_grid_y; ++by)
        for (unsigned bx = 0; bx < g_grid_x; ++bx) {
            pthread_barrier_wait(&hostk::g_group.all);
            blockIdx.x = bx; blockIdx.y = by; blockIdx.z = 0;
            cph::batch_retable_poisson_kernel(g_args);
            pthread_barrier_wait(&hostk::g_group.all);         // the workgroup is done
        }
    gridDim.x = g_mstep_grid; gridDim.y = 1;
    for (unsigned bx = 0; bx < g_mstep_grid; ++bx) {
        pthread_barrier_wait(&hostk::g_group.all);
        blockIdx.x = bx; blockIdx.y = 0;
        cph::batch_mstep_poisson_kernel(g_mstep);
        pthread_barrier_wait(&hostk::g_group.all);
    }
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_poisson_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.k >= 2 && h.k <= 8 && h.grid_y >= 1 && h.T_max >= 1 && h.n_obs >= 0, "header out of range");
    const size_t B = (size_t)h.B, k = (size_t)h.k, n_tab = B * (size_t)h.T_max * cph::kBatchTab;
    cph::BatchProblem* prob = exact_block<cph::BatchProblem>(B);
    int64_t* first = exact_block<int64_t>(B);
    double* rates = exact_block<double>(B * k);
    double* trans = exact_block<double>(B * k * k);
    double* obs = exact_block<double>((size_t)h.n_obs);
    double* lfact = exact_block<double>((size_t)cph::kPoissonMaxCount + 1);
    double* tab = exact_block<double>(n_tab);
    uint64_t* thr = exact_block<uint64_t>(B * 64);
    int32_t* status = exact_block<int32_t>(B);
    double* rate_out = exact_block<double>(B * 8);
    double* lograte_out = exact_block<double>(B * 8);
    double* stats = exact_block<double>(B * cph::kRetableStats);
    double floor = 0.0;
    get(f, prob, B);
    get(f, first, B);
    get(f, rates, B * k);
    get(f, trans, B * k * k);
    get(f, obs, (size_t)h.n_obs);
    get(f, tab, n_tab);
    get(f, thr, B * 64);
    get(f, rate_out, B * 8);
    get(f, lograte_out, B * 8);
    get(f, stats, B * cph::kRetableStats);
    get(f, &floor, 1);
    std::fclose(f);
    cph::poisson_log_fact_table(lfact);
    for (size_t b = 0; b < B; ++b) status[b] = -7;             // a word nobody wrote shows
    // the M-step runs on copies: the re-table's inputs stay as the case gave them
    double* m_rates = exact_block<double>(B * k);
    double* m_lograte = exact_block<double>(B * k);
    double* m_trans = exact_block<double>(B * k * k);
    std::memcpy(m_rates, rates, B * k * sizeof(double));
    std::memcpy(m_trans, trans, B * k * k * sizeof(double));
    for (size_t i = 0; i < B * k; ++i) m_lograte[i] = -7.0;

    g_args.prob = prob; g_args.first = first; g_args.rates = rates; g_args.trans = trans; g_args.obs = obs; g_args.lfact = lfact;
    g_args.tab = tab; g_args.thr = thr; g_args.status = status; g_args.rate_out = rate_out; g_args.log_rate_out = lograte_out;
    g_args.T_max = (int)h.T_max; g_args.k = (int)h.k;
    g_grid_x = (unsigned)h.B; g_grid_y = (unsigned)h.grid_y;
    g_mstep.stats = stats; g_mstep.rates = m_rates; g_mstep.trans = m_trans; g_mstep.log_rates = m_lograte;
    g_mstep.floor = floor; g_mstep.B = h.B; g_mstep.k = (int)h.k;
    g_mstep_grid = (unsigned)((B * k + cph::kThreads - 1) / cph::kThreads);

    hostk::group_init();
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, tab, n_tab);
    put(o, thr, B * 64);
    put(o, status, B);
    put(o, rate_out, B * 8);
    put(o, lograte_out, B * 8);
    put(o, m_rates, B * k);
    put(o, m_trans, B * k * k);
    put(o, m_lograte, B * k);
    put(o, lfact, (size_t)cph::kPoissonMaxCount + 1);
    need(std::fclose(o) == 0, "close");
    std::free(prob); std::free(first); std::free(rates); std::free(trans); std::free(obs); std::free(lfact); std::free(tab); std::free(thr); std::free(status);
    std::free(rate_out); std::free(lograte_out); std::free(stats); std::free(m_rates); std::free(m_lograte); std::free(m_trans);
    return 0;
}
