// batch_csmc_kernel (csrc/batch_csmc.hpp) run as host code over a batch given in a case file
// (tests/test_batch_csmc_kernel_text_host.py writes it and states the format): every buffer is a heap block of exactly the size the
// host code would hand the kernel, the launch is a loop over its blocks, a block 256 threads.  "batch_csmc_host.hpp" is the kernel's
// text with batch_csmc_pre.hpp in place of batch_smc.hpp: the shim, BatchProblem and batch_mass_row cut out of csrc/batch_smc.hpp.
#include "batch_csmc_host.hpp"

#include <limits>
#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b43534d43303031;
struct Header { int64_t magic, B, k, thr_stride, T_max, n, described, skew_us, thr_words, ref_entries; };

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

cph::BatchCsmcArgs g_args;
unsigned g_grid_x = 0;

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    gridDim.x = g_grid_x; gridDim.y = 1; gridDim.z = 1;
    for (unsigned bx = 0; bx < g_grid_x; ++bx) {
        blockIdx.x = bx; blockIdx.y = 0; blockIdx.z = 0;
        cph::batch_csmc_kernel(g_args);
        pthread_barrier_wait(&hostk::g_group.all);             // the workgroup is done: the statics stand for the next one's LDS
    }
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_csmc_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.k >= 2 && h.k <= 8 && h.T_max >= 1 && h.n >= 1 && h.n <= 8192 && (h.thr_stride == 0 || h.thr_stride == 64) && h.skew_us >= 0, "header out of range");
    need(h.thr_words == (h.thr_stride ? 64 * h.B : 64), "the thresholds: 64 words a table");
    const size_t B = (size_t)h.B, rows = B * (size_t)h.T_max;
    cph::BatchProblem* prob = exact_block<cph::BatchProblem>(h.described ? B : 0);
    int32_t* order = exact_block<int32_t>(h.described ? B : 0);
    int64_t* first = exact_block<int64_t>(h.described ? B : 0);
    uint64_t* thr = exact_block<uint64_t>((size_t)h.thr_words);
    uint64_t* seeds = exact_block<uint64_t>(B);
    double* tab = exact_block<double>(rows * cph::kBatchTab);
    int8_t* ref = exact_block<int8_t>((size_t)h.ref_entries);
    double* mass = exact_block<double>(rows * 8);
    if (h.described) { get(f, prob, B); get(f, order, B); get(f, first, B); }
    get(f, thr, (size_t)h.thr_words);
    get(f, seeds, B);
    get(f, tab, rows * cph::kBatchTab);
    get(f, ref, (size_t)h.ref_entries);
    std::fclose(f);
    // what the host code's launch may rely on: every problem's path lies inside ref, its shape inside the batch's
    for (size_t b = 0; b < B; ++b) {
        const int64_t T = h.described ? prob[b].T : h.T_max, at = h.described ? first[b] : (int64_t)b * h.T_max;
        need(T >= 1 && T <= h.T_max && at >= 0 && at + T <= h.ref_entries, "a reference path outside the buffer");
        need(!h.described || (prob[b].n >= 1 && prob[b].n <= h.n && order[b] >= 0 && order[b] < h.B), "a descriptor out of range");
    }
    for (size_t i = 0; i < rows * 8; ++i) mass[i] = std::numeric_limits<double>::quiet_NaN();     // a row nobody owns stays NaN

    g_args.tab = tab; g_args.seeds = seeds; g_args.thr = thr; g_args.prob = h.described ? prob : nullptr; g_args.order = h.described ? order : nullptr;
    g_args.ref = ref; g_args.first = h.described ? first : nullptr; g_args.mass = mass;
    g_args.T_max = (int)h.T_max; g_args.n = (int)h.n; g_args.k = (int)h.k; g_args.thr_stride = (int)h.thr_stride;
    g_grid_x = (unsigned)B;

    hostk::group_init();
    hostk::g_group.skew_us = (long)h.skew_us;
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, mass, rows * 8);
    need(std::fclose(o) == 0, "close");
    std::free(prob); std::free(order); std::free(first); std::free(thr); std::free(seeds); std::free(tab); std::free(ref); std::free(mass);
    return 0;
}
