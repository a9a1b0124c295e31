"""The host pieces of the conditional runs (include/cpprob_hip.h: cpprob_hip_batch_run_conditional*): the symbols are declared,
listed and bound; what the library and the Python wrappers refuse without a device; the particle-Gibbs driver is exported and says
what it is; the C++ option as plain C++14; and the command line's refusal, which ends before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cpprob_amd
import cpprob_amd.capi as cp

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cpprob_amd", "bin", "cpprob_main")
NEW = {"cpprob_hip_batch_run_conditional": 4, "cpprob_hip_batch_run_conditional_device": 4}


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n_args, s
    assert re.search(r"int cpprob_hip_batch_run_conditional\(cpprob_hip_ctx\* ctx, const uint64_t\* h_seeds, const int32_t\* h_ref, size_t n_entries\);", header)
    assert re.search(r"int cpprob_hip_batch_run_conditional_device\(cpprob_hip_ctx\* ctx, const uint64_t\* h_seeds, const int8_t\* d_ref, size_t n_entries\);", header)
    assert "multinomial whatever cfg.resampler says" in header
    assert L.cpprob_hip_abi_version() == 3 and re.search(r"#define CPPROB_HIP_ABI_VERSION 3\b", header)
    for name in ("batch_run_conditional", "batch_run_conditional_device"):
        assert callable(getattr(cp.Engine, name)), name
    # the batch configuration keeps its fields and the flags their one bit
    assert [f for f, _ in cp.BatchConfig._fields_] == ["algorithm", "model", "resampler", "keep_history", "flags", "ess_threshold", "n_particles", "n_problems"]
    assert len(re.findall(r"#define CPPROB_HIP_BATCH_\w+\s+\d", header)) == 1


def test_refusals_without_a_device():
    L = cp.load_library()
    seeds = np.arange(3, dtype=np.uint64)
    ref = np.zeros(6, np.int32)
    sp = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.cpprob_hip_batch_run_conditional(None, sp, ref.ctypes.data, ref.size) == EINVAL
    assert b"ctx is NULL" in L.cpprob_hip_last_error(None)
    assert L.cpprob_hip_batch_run_conditional_device(None, sp, ref.ctypes.data, ref.size) == EINVAL
    assert L.cpprob_hip_batch_run_conditional(None, None, None, 0) == EINVAL


def _engine(T, B=None):
    """An Engine without a context: the wrappers' checks run before the library is called."""
    eng = cp.Engine.__new__(cp.Engine)
    if B is None:
        eng.batch_B, eng.batch_T, eng.batch_n = len(T), max(T), 4
        eng.batch_shapes = (np.array(T, np.uint32), np.full(len(T), 4, np.uint32))
    else:
        eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_shapes = B, T, 4, None
    return eng


class _Tensor:
    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


def test_wrappers_check_their_arguments():
    eng = _engine([3, 1, 2])
    good = [np.zeros(3, np.int32), np.zeros(1, np.int32), np.zeros(2, np.int32)]
    for seeds, ref in ((np.arange(2), good),                                    # a seed short
                       (np.arange(3), good[:2]),                                # a path short
                       (np.arange(3), [good[0], good[1], np.zeros(3, np.int32)]),     # a path too long
                       (np.arange(3), np.zeros(5, np.int32)),                   # a packed array of the wrong total
                       (np.arange(3), np.zeros(7, np.int32))):
        with pytest.raises(ValueError):
            eng.batch_run_conditional(seeds, ref)
    for seeds, n in ((np.arange(2), 6), (np.arange(3), 5), (np.arange(3), 7)):
        with pytest.raises(ValueError):
            eng.batch_run_conditional_device(seeds, _Tensor(n))
    with pytest.raises(ValueError):
        eng.batch_run_conditional_device(np.arange(3), None)
    uni = _engine(4, B=2)                                                       # a uniform batch: B paths of T states
    with pytest.raises(ValueError):
        uni.batch_run_conditional(np.arange(2), np.zeros(7, np.int32))
    with pytest.raises(ValueError):
        uni.batch_run_conditional(np.arange(2), [np.zeros(4, np.int32), np.zeros(3, np.int32)])


def test_particle_gibbs_is_exported_and_says_what_it_is():
    fn = cpprob_amd.hmm_table_particle_gibbs
    assert fn is cpprob_amd.pgibbs.hmm_table_particle_gibbs and callable(fn)
    doc = " ".join(fn.__doc__.split())
    assert "conditional" in doc and "particle Gibbs with backward sampling" in doc
    assert "at every n_particles >= 1" in doc and "32-bit quantisation" in doc
    import inspect
    names = list(inspect.signature(fn).parameters)
    assert names == ["engine", "observes", "means0", "trans0", "n_particles", "seeds", "sweeps", "rng", "prior"]
    # hmm_table_gibbs keeps its caveat
    assert "This is NOT a particle-Gibbs kernel with a retained path (conditional SMC)" in " ".join(cpprob_amd.hmm_table_gibbs.__doc__.split())


def test_kernel_is_built_into_the_library_and_results_wait_for_a_run():
    hip = open(os.path.join(ROOT, "cpprob_amd", "csrc", "cpprob_hip.hip")).read()
    assert "hipLaunchKernelGGL(batch_csmc_kernel, dim3((unsigned)B), dim3(kThreads), 0, c->stream, a);" in hip
    assert hip.count("a conditional run keeps masses, not books") == 2          # cpprob_hip_batch_results and _results_device


_OPTIONS_TU = r"""
#include <cstdint>
#include <string>
#include <vector>
#include "cpprob/cpprob.hpp"

int main()
{
    cpprob::gpu::options().keep_history = false;
    cpprob::gpu::options().keep_masses = true;
    cpprob::gpu::options().trajectory_stats = 1;
    cpprob::gpu::options().conditional_paths = {{0, 1}, {1, 1}};
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        const std::vector<cpprob::gpu::Result> q = cpprob::gpu::hmm_table_batch(tables, {{0.5, 0.25}}, {512}, seeds);
        return q.size() == 2 && q[0].trajectory_stats.size() == 1 && q[0].log_evidence == 0.0 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_conditional_paths_option_compiles_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    src = tmp_path / "csmc.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "csmc.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]


def test_cli_and_cpp_refusals_end_before_a_device(tmp_path):
    """cpprob_main --conditional_paths without --keep_masses: hmm_table_batch throws, worded like its neighbours; a path of the wrong
    length or with a state past k is refused too; so is a file with fewer lines than problems."""
    (tmp_path / "tables.txt").write_text("[-1 1] [0.9 0.1 0.2 0.8] [0.5 0.25 -0.5]\n[-1 1] [0.9 0.1 0.2 0.8] [0.5 0.25]\n")
    (tmp_path / "paths.txt").write_text("0 1 1\n1 0\n")
    (tmp_path / "short.txt").write_text("0 1 1\n1\n")
    (tmp_path / "state.txt").write_text("0 1 2\n1 0\n")
    (tmp_path / "lines.txt").write_text("0 1 1\n")
    base = [MAIN, "--smc", "--model_folder", str(tmp_path), "--batch_tables_file", "tables.txt", "-n", "8"]

    def run(*more):
        return subprocess.run(base + list(more), capture_output=True, text=True, timeout=60)
    p = run("--filtering_only", "--conditional_paths", "paths.txt")
    assert p.returncode != 0 and "conditional_paths" in p.stderr and "keep_masses" in p.stderr
    p = run("--conditional_paths", "paths.txt")
    assert p.returncode != 0 and "conditional_paths" in p.stderr and "keep_history = false" in p.stderr
    p = run("--filtering_only", "--keep_masses", "--conditional_paths", "short.txt")
    assert p.returncode != 0 and "one state per observe" in p.stderr
    p = run("--filtering_only", "--keep_masses", "--conditional_paths", "state.txt")
    assert p.returncode != 0 and "states 0 .. k - 1" in p.stderr
    p = run("--filtering_only", "--keep_masses", "--conditional_paths", "lines.txt")
    assert p.returncode != 0 and "1 lines for 2 problems" in p.stderr
    p = run("--filtering_only", "--keep_masses", "--conditional_paths", "paths.txt", "--stream_chunk", "1")
    assert p.returncode != 0 and "--conditional_paths" in p.stderr
