// What csrc/batch_retable.hpp takes from batch_smc.hpp, as host code: tests/test_batch_retable_kernel_text_host.py compiles the
// kernels' own text against this file (its `#include "batch_smc.hpp"` line names this header instead).  The workgroup, its barrier and
// the launch variables are batch_smooth_shim.hpp's; the descriptor is restated with its size.
#pragma once
#include "batch_smooth_shim.hpp"

namespace cph {
struct BatchProblem { int32_t T, n; int64_t store; };
static_assert(sizeof(BatchProblem) == 16, "one problem's descriptor");
}  // namespace cph
