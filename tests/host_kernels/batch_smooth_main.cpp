// The three kernels of csrc/batch_smooth.hpp run as host code over a grid given in a case file (tests/test_batch_smooth_kernel_text_host.py
// writes it and states the format): every buffer is a heap block of exactly the size the host code would hand the kernels, a launch
// is a loop over its blocks, a block 256 threads.  "batch_smooth_host.hpp" is the kernels' text with the shim in place of batch_smc.hpp.
#include "batch_smooth_host.hpp"

#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b534d4f4f544831;      // "1HTOOMSK"
enum Flag : int64_t { kLagMarg = 1, kSmoothMarg = 2, kSmoothTraj = 4, kHmm3 = 8, kSmooth = 16 };
struct Header {
    int64_t magic, B, T_max, k, spp, thr_stride, n_traj, lds_bytes, marg_rows, lag, count_gy, lag_gy, flags, n_values, mass_rows, thr_words,
        traj_entries, skew_us;
    uint64_t draw_base;
};

template <class T> T* block(size_t n) { return static_cast<T*>(std::calloc(n ? n : 1, n ? sizeof(T) : 1)); }   // (n = 0: one byte nobody may touch twice)
template <class T> T* exact_block(size_t n)
{
    // calloc(0) may return a block with room: ask for exactly n elements so that the first element past the end is poisoned
    return n ? static_cast<T*>(std::calloc(n, sizeof(T))) : nullptr;
}

void need(bool ok, const char* what)
{
    if (!ok) { std::fprintf(stderr, "case file: %s\n", what); std::exit(2); }
}
template <class T> void get(std::FILE* f, T* p, size_t n) { need(n == 0 || std::fread(p, sizeof(T), n, f) == n, "short read"); }
template <class T> void put(std::FILE* f, const T* p, size_t n) { need(n == 0 || std::fwrite(p, sizeof(T), n, f) == n, "short write"); }

struct Launch { void (*kernel)(cph::BatchSmoothArgs); cph::BatchSmoothArgs args; unsigned gx, gy; size_t lds_bytes; long skew_us; };
std::vector<Launch> g_launches;

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    for (const Launch& l : g_launches) {
        gridDim.x = l.gx; gridDim.y = l.gy; gridDim.z = 1;
        for (unsigned by = 0; by < l.gy; ++by)
            for (unsigned bx = 0; bx < l.gx; ++bx) {
                if (threadIdx.x == 0) {
                    // a workgroup's dynamic LDS is its own: a fresh block of the launch's size, nothing of the workgroup before it
                    std::free(hostk::g_group.dynamic_lds);
                    hostk::g_group.dynamic_lds = exact_block<double>(l.lds_bytes / sizeof(double));
                    hostk::g_group.skew_us = l.skew_us;
                }
                pthread_barrier_wait(&hostk::g_group.all);
                blockIdx.x = bx; blockIdx.y = by; blockIdx.z = 0;
                l.kernel(l.args);
                pthread_barrier_wait(&hostk::g_group.all);     // the workgroup is done: the statics stand for the next one's LDS
            }
    }
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_smooth_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.k >= 1 && h.k <= 8 && h.spp >= 1 && h.spp <= 8 && h.lds_bytes >= 0 && h.lds_bytes % 8 == 0, "header out of range");
    const size_t B = (size_t)h.B;
    cph::BatchSmoothProblem* desc = exact_block<cph::BatchSmoothProblem>(B);
    int8_t* values = exact_block<int8_t>((size_t)h.n_values);
    double* tab = exact_block<double>(B * (size_t)h.T_max * cph::kBatchTab);
    uint64_t* thr = exact_block<uint64_t>((size_t)h.thr_words);
    uint64_t* seeds = exact_block<uint64_t>(B);
    double* mass = exact_block<double>((size_t)h.mass_rows * 8);
    double* marg = exact_block<double>(B * (size_t)h.marg_rows * (size_t)h.spp);       // zeroed, as the host's memset leaves it
    int8_t* traj = exact_block<int8_t>((size_t)h.traj_entries);
    get(f, desc, B);
    get(f, values, (size_t)h.n_values);
    get(f, tab, B * (size_t)h.T_max * cph::kBatchTab);
    get(f, thr, (size_t)h.thr_words);
    get(f, seeds, B);
    get(f, mass, (size_t)h.mass_rows * 8);
    std::fclose(f);
    if (traj) std::memset(traj, -7, (size_t)h.traj_entries);                            // an entry nobody wrote shows

    cph::BatchSmoothArgs a{};
    a.desc = desc; a.values = values; a.tab = tab; a.thr = thr; a.seeds = seeds; a.mass = mass;
    a.draw_base = h.draw_base;
    a.T_max = (int)h.T_max; a.k = (int)h.k; a.spp = (int)h.spp; a.thr_stride = (int)h.thr_stride; a.n_traj = (int)h.n_traj;
    a.lds_bytes = (int)h.lds_bytes; a.marg_rows = (int)h.marg_rows; a.lag = (int)h.lag;
    // the launches of batch_smooth_enqueue, in its order
    if (h.count_gy > 0) g_launches.push_back(Launch{cph::batch_smooth_count_kernel, a, (unsigned)B, (unsigned)h.count_gy, 0, (long)h.skew_us});
    if (h.lag_gy > 0) {
        need((h.flags & kLagMarg) && marg, "a lag launch without marginals");
        cph::BatchSmoothArgs l = a;
        l.marg = marg;
        g_launches.push_back(Launch{cph::batch_smooth_lag_kernel, l, (unsigned)B, (unsigned)h.lag_gy, 0, 0});
    }
    if (h.flags & kSmooth) {
        cph::BatchSmoothArgs s = a;
        s.marg = (h.flags & kSmoothMarg) ? marg : nullptr;
        s.traj = (h.flags & kSmoothTraj) ? traj : nullptr;
        const unsigned tiles = s.traj ? (unsigned)((h.n_traj + cph::kTile - 1) / cph::kTile) : 0u;
        g_launches.push_back(Launch{(h.flags & kHmm3) ? cph::batch_smooth_kernel<3> : cph::batch_smooth_kernel<8>, s, (unsigned)B, 1 + tiles, (size_t)h.lds_bytes, 0});
    }

    hostk::group_init();
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);
    std::free(hostk::g_group.dynamic_lds);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, mass, (size_t)h.mass_rows * 8);
    put(o, marg, B * (size_t)h.marg_rows * (size_t)h.spp);
    put(o, traj, (size_t)h.traj_entries);
    need(std::fclose(o) == 0, "close");
    std::free(desc); std::free(values); std::free(tab); std::free(thr); std::free(seeds); std::free(mass); std::free(marg); std::free(traj);
    return 0;
}
