// batch_mass_row (csrc/batch_smc.hpp) as a host program: tests/test_batch_masses_host.py cuts the function's text out of the header into
// batch_mass_row_host.hpp and builds this file against it and tests/host_kernels/batch_smooth_shim.hpp (fix_weight is the oracle's,
// u64_to_double a cast) with -fsanitize=address,undefined.  usage: batch_mass_row_host <case> <out>
//
// The case file: a header of 3 int64 {magic, rows, k}, then the counts (uint32 [rows][8]) and the log-weights (double [rows][k]).  The
// output: the rows of the m table, double [rows][8].  Every row's log-weights are handed over in a heap block of exactly k doubles: a
// read of a state >= k shows.
#include "batch_smooth_shim.hpp"

#include <cstddef>
#include <vector>

#include "batch_mass_row_host.hpp"

namespace {
constexpr int64_t kMagic = 0x4b4d415353524f57;

bool read_all(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <case> <out>\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int64_t head[3];
    if (!read_all(f, head, sizeof head) || head[0] != kMagic || head[1] < 0 || head[2] < 2 || head[2] > 8) { std::fprintf(stderr, "bad header\n"); return 2; }
    const size_t rows = (size_t)head[1];
    const int k = (int)head[2];
    std::vector<uint32_t> cnt(rows * 8);
    std::vector<double> ll(rows * (size_t)k), out(rows * 8, -1.0);
    if (!read_all(f, cnt.data(), cnt.size() * sizeof(uint32_t)) || !read_all(f, ll.data(), ll.size() * sizeof(double))) { std::fprintf(stderr, "short case file\n"); return 2; }
    std::fclose(f);
    for (size_t r = 0; r < rows; ++r) {
        uint32_t c[8];
        for (int s = 0; s < 8; ++s) c[s] = cnt[r * 8 + s];
        const std::vector<double> row(ll.begin() + (std::ptrdiff_t)(r * k), ll.begin() + (std::ptrdiff_t)((r + 1) * k));
        cph::batch_mass_row(c, row.data(), k, out.data() + r * 8);
    }
    std::FILE* g = std::fopen(argv[2], "wb");
    if (!g || std::fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::fclose(g);
    return 0;
}
