// batch_pool_stats_kernel (csrc/batch_pool.hpp) run as host code over a case file (tests/test_batch_pool_kernel_text_host.py writes it
// and states the format): every buffer is a heap block of exactly the size the host code hands the kernel, the launch is a loop over
// the blocks of the host's own grid, a block 256 threads.  "batch_pool_host.hpp" is the kernel's text with the shim in place of
// batch_smc.hpp.  The output is NaN on the way in; in place, the output is the records' block itself.
#include "batch_pool_host.hpp"

#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b504f4f4c303031;      // "100LOOPK"
struct Header { int64_t magic, B, G, R, broadcast, in_place; };

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

cph::BatchPoolArgs g_args;
unsigned g_grid = 0;

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    gridDim.x = g_grid; gridDim.y = 1; gridDim.z = 1;
    for (unsigned bx = 0; bx < g_grid; ++bx) {
        pthread_barrier_wait(&hostk::g_group.all);
        blockIdx.x = bx; blockIdx.y = 0; blockIdx.z = 0;
        cph::batch_pool_stats_kernel(g_args);
        pthread_barrier_wait(&hostk::g_group.all);             // the workgroup is done
    }
    return nullptr;
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_pool_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.G >= 1 && h.G <= h.B && h.R >= 1 && (h.in_place == 0 || h.broadcast == 1), "header out of range");
    const size_t B = (size_t)h.B, G = (size_t)h.G, R = (size_t)h.R;
    const size_t n_rec = B * R * cph::kPoolStats, n_out = (h.broadcast ? B : G) * R * cph::kPoolStats;
    int32_t* members = exact_block<int32_t>(B);
    int32_t* first = exact_block<int32_t>(G + 1);
    double* rec = exact_block<double>(n_rec);
    get(f, members, B);
    get(f, first, G + 1);
    get(f, rec, n_rec);
    std::fclose(f);
    double* out = rec;
    if (!h.in_place) {
        out = exact_block<double>(n_out);
        for (size_t i = 0; i < n_out; ++i) out[i] = std::nan("");   // an entry nobody wrote shows
    }

    g_args.members = members; g_args.first = first; g_args.rec = rec; g_args.out = out;
    g_args.pairs = (int64_t)(G * R); g_args.R = (int)h.R; g_args.broadcast = (int)h.broadcast;
    g_grid = (unsigned)((g_args.pairs + cph::kWaves - 1) / cph::kWaves);       // the host's own grid

    hostk::group_init();
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, out, n_out);
    need(std::fclose(o) == 0, "close");
    if (!h.in_place) std::free(out);
    std::free(members); std::free(first); std::free(rec);
    return 0;
}
