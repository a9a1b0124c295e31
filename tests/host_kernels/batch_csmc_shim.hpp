// What csrc/batch_csmc.hpp takes from the headers behind batch_smc.hpp beyond tests/host_kernels/batch_smooth_shim.hpp, as host code:
// the four words of a lane's particles (the device's draw_words4 on the oracle's Philox block), the oracle's uniform_smallint and the
// high half of a 64 x 64 bit product.  tests/test_batch_csmc_kernel_text_host.py compiles the kernel's own text against this file.
#pragma once
#include "batch_smooth_shim.hpp"

extern "C" uint64_t orc_smallint_from_bits(uint32_t w, uint64_t a, uint64_t b);

inline uint64_t __umul64hi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }

namespace cph {
inline uint64_t smallint_from_word(uint32_t w, uint64_t a, uint64_t b) { return orc_smallint_from_bits(w, a, b); }

// 32-bit words of particles pid0 .. pid0 + 3: word i & 3 of block i >> 2
inline void draw_words4(uint64_t seed, uint64_t pid0, uint64_t draw, uint32_t (&w)[4])
{
    for (uint64_t q = 0; q < 4; ++q) {
        uint32_t r[4];
        orc_draw_block(seed, (pid0 + q) >> 2, draw, r);
        w[q] = r[(pid0 + q) & 3];
    }
}
}  // namespace cph
