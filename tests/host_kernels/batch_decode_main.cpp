// batch_decode_forward_kernel and batch_decode_trace_kernel (csrc/batch_decode.hpp) run as host code over grids given in a case file
// (tests/test_batch_decode_kernel_text_host.py writes it and states the format): every buffer is a heap block of exactly the size the
// host code would hand the kernel, a launch is a loop over its blocks, a block 256 threads.  "batch_decode_host.hpp" is the kernels'
// text on top of batch_smooth.hpp's, with the shim in place of batch_smc.hpp.
#include "batch_decode_host.hpp"

#include <vector>

namespace {
constexpr int64_t kMagic = 0x4b4445434f443031;      // "10DOCEDK"
struct Header { int64_t magic, B, k, T_max, lp_stride, lp_doubles, rows, full, lag, n_rows, path_entries, grid_x, grid_y, forward, trace; };

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

cph::BatchDecodeArgs g_args;
unsigned g_grid_x = 0, g_grid_y = 0;
bool g_forward = false;

void* thread_main(void* arg)
{
    threadIdx.x = (unsigned)(uintptr_t)arg;
    gridDim.x = g_grid_x; gridDim.y = g_grid_y; gridDim.z = 1;
    for (unsigned bx = 0; bx < g_grid_x; ++bx) {
        for (unsigned by = 0; by < g_grid_y; ++by) {
            pthread_barrier_wait(&hostk::g_group.all);
            blockIdx.x = bx; blockIdx.y = by; blockIdx.z = 0;
            if (g_forward) cph::batch_decode_forward_kernel(g_args);
            else cph::batch_decode_trace_kernel(g_args);
            pthread_barrier_wait(&hostk::g_group.all);         // the workgroup is done
        }
    }
    return nullptr;
}

void launch(bool forward, unsigned gx, unsigned gy)
{
    g_forward = forward; g_grid_x = gx; g_grid_y = gy;
    std::vector<pthread_t> th(cph::kThreads);
    for (int i = 0; i < cph::kThreads; ++i) need(pthread_create(&th[i], nullptr, thread_main, (void*)(uintptr_t)i) == 0, "pthread_create");
    for (pthread_t& t : th) pthread_join(t, nullptr);
}
}  // namespace

int main(int argc, char** argv)
{
    need(argc == 3, "usage: batch_decode_host CASE OUT");
    std::FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the case");
    Header h{};
    get(f, &h, 1);
    need(h.magic == kMagic, "not a case file");
    need(h.B >= 1 && h.k >= 2 && h.k <= 8 && h.T_max >= 1 && h.rows >= 0 && h.grid_x >= 1 && h.grid_y >= 1 && h.n_rows >= 0 && h.lag >= 0 && h.path_entries >= 0, "header out of range");
    const size_t B = (size_t)h.B;
    cph::BatchSmoothProblem* desc = exact_block<cph::BatchSmoothProblem>(B);
    double* lp = exact_block<double>((size_t)h.lp_doubles);
    double lp0 = 0.0;
    double* mass = exact_block<double>((size_t)h.rows * 8);
    double* tab = exact_block<double>(B * (size_t)h.T_max * cph::kBatchTab);
    double* v = exact_block<double>(B * 8);
    uint32_t* words = exact_block<uint32_t>((size_t)h.rows);
    double* score = exact_block<double>(B);                                         // (zeroed, as the caller hands it over)
    int8_t* path = exact_block<int8_t>((size_t)h.path_entries);
    get(f, desc, B);
    get(f, lp, (size_t)h.lp_doubles);
    get(f, &lp0, 1);
    get(f, mass, (size_t)h.rows * 8);
    get(f, tab, B * (size_t)h.T_max * cph::kBatchTab);
    get(f, v, B * 8);
    get(f, words, (size_t)h.rows);
    std::fclose(f);
    for (size_t i = 0; i < (size_t)h.path_entries; ++i) path[i] = h.full ? -7 : -1;  // full: an entry nobody wrote shows; fixed lag: the caller's fill

    g_args.desc = desc; g_args.mass = mass; g_args.tab = tab; g_args.lp = lp; g_args.lp0 = lp0; g_args.v = v; g_args.words = words;
    g_args.score = score; g_args.path = path;
    g_args.B = (int)B; g_args.T_max = (int)h.T_max; g_args.k = (int)h.k; g_args.lp_stride = (int)h.lp_stride;
    g_args.full = (int)h.full; g_args.lag = (int)h.lag; g_args.n_rows = (int)h.n_rows;

    hostk::group_init();
    if (h.forward) launch(true, (unsigned)h.grid_x, 1);
    if (h.trace) launch(false, (unsigned)B, (unsigned)h.grid_y);

    std::FILE* o = std::fopen(argv[2], "wb");
    need(o != nullptr, "cannot open the output");
    put(o, words, (size_t)h.rows);
    put(o, v, B * 8);
    put(o, score, B);
    put(o, path, (size_t)h.path_entries);
    need(std::fclose(o) == 0, "close");
    std::free(desc); std::free(lp); std::free(mass); std::free(tab); std::free(v); std::free(words); std::free(score); std::free(path);
    return 0;
}
