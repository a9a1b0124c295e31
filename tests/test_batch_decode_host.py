"""The host pieces of the decode calls (include/cpprob_hip.h: cpprob_hip_batch_decode*, cpprob_hip_batch_decode_lag*, _decode_logp):
the symbols are declared, listed and bound; what the library refuses without a device; the path's layout; the Python wrappers' own
argument checks; and the kernel header's standing promises that a text can show."""
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
NEW = {"cpprob_hip_batch_decode": 5, "cpprob_hip_batch_decode_device": 5, "cpprob_hip_batch_decode_lag": 8, "cpprob_hip_batch_decode_lag_device": 8,
       "cpprob_hip_batch_decode_logp": 4, "cpprob_hip_batch_pass_grid": 5}


def test_decode_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n_args, s
    assert L.cpprob_hip_abi_version() == 3
    for name in ("batch_decode", "batch_decode_device", "batch_decode_lag", "batch_decode_lag_device", "batch_decode_logp", "batch_pass_grid"):
        assert callable(getattr(cp.Engine, name)), name
    assert cpprob_amd.decode.hmm_table_decode is cpprob_amd.hmm_table_decode


def test_decode_refusals_without_a_device():
    L = cp.load_library()
    path = np.full(8, -5, np.int32)
    score = np.full(3, -5.0)
    lp = np.full(64, -5.0)
    lp0 = C.c_double(-5.0)
    assert L.cpprob_hip_batch_decode(None, path.ctypes.data, path.size, score.ctypes.data, score.size) == EINVAL
    assert b"ctx" in L.cpprob_hip_last_error(None)
    assert L.cpprob_hip_batch_decode_device(None, None, 0, None, 0) == EINVAL
    assert L.cpprob_hip_batch_decode_lag(None, 1, None, 4, path.ctypes.data, path.size, score.ctypes.data, score.size) == EINVAL
    assert L.cpprob_hip_batch_decode_lag_device(None, 1, None, 4, None, 0, None, 0) == EINVAL
    assert L.cpprob_hip_batch_decode_logp(None, 0, lp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(lp0)) == EINVAL
    assert b"ctx" in L.cpprob_hip_last_error(None)
    assert np.all(path == -5) and np.all(score == -5.0) and np.all(lp == -5.0) and lp0.value == -5.0
    grid = [C.c_uint32(7) for _ in range(4)]
    assert L.cpprob_hip_batch_pass_grid(None, *[C.byref(g) for g in grid]) == EINVAL and [g.value for g in grid] == [7] * 4


def test_path_layout_is_the_smoothers_with_one_trajectory():
    """A path is packed by the lengths reached: cpprob_hip_batch_smooth_layout with n_traj = 1, a problem of length 0 owning nothing."""
    T = np.array([0, 2, 7, 0, 23], np.uint32)
    first = cp.batch_smooth_layout(T, 1)
    assert [int(x) for x in first] == [0, 0, 2, 9, 9, 32]
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    assert "exactly cpprob_hip_batch_smooth_layout with n_traj = 1" in header


def _shell():
    """An Engine without a context: the wrappers' checks run before the library is called."""
    eng = cp.Engine.__new__(cp.Engine)
    eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K = 4, 23, 8, 8
    eng.batch_shapes = (np.array([0, 2, 7, 23], np.uint32), np.array([1, 300, 777, 1025], np.uint32))
    return eng


def test_wrappers_check_their_arguments():
    eng = _shell()
    for lag in (-1, (1 << 24) + 1):
        with pytest.raises(ValueError):
            eng.batch_decode_lag(lag)
        with pytest.raises(ValueError):
            eng.batch_decode_lag_device(lag)
    with pytest.raises(ValueError):
        eng.batch_decode_lag(1, [0, 0])                              # one first step per problem
    with pytest.raises(ValueError):
        eng.batch_decode_lag(1, [0, 0, -1, 0])
    with pytest.raises(ValueError):
        eng._batch_decode_lag_shapes(1, [0, 0, 1 << 32, 0])
    assert eng._batch_decode_lag_shapes(1 << 24, None) == (None, 23)
    h_from, rows = eng._batch_decode_lag_shapes(3, [0, 1, 7, 20])
    assert h_from.dtype == np.uint32 and h_from.tolist() == [0, 1, 7, 20] and rows == 3
    eng.batch_shapes = None                                          # a uniform batch: T of the begin
    assert eng._batch_decode_lag_shapes(0, None) == (None, 23)
    with pytest.raises(ValueError):
        cpprob_amd.hmm_table_decode(eng, [np.zeros(3)], np.zeros((2, 2)), np.zeros((2, 2, 2)), 8, [1, 2])      # one sequence per table
    with pytest.raises(ValueError):
        cpprob_amd.hmm_table_decode(eng, np.zeros(3), np.zeros((2, 2)), np.zeros((2, 3, 2)), 8, [1, 2])
    with pytest.raises(ValueError):
        cpprob_amd.hmm_table_decode(eng, np.zeros(3), np.zeros((2, 2)), np.zeros((2, 2, 2)), 8, [1, 2], lag=-1)


def test_kernel_header_keeps_its_promises():
    """csrc/batch_decode.hpp: on top of batch_smooth.hpp, the floating-point functions with fp contract off, no logarithm but the
    host's, two kernels and no LDS, and the existing headers untouched by it."""
    csrc = os.path.join(ROOT, "cpprob_amd", "csrc")
    text = open(os.path.join(csrc, "batch_decode.hpp")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert code.count('#include "batch_smooth.hpp"') == 1 and code.count("#include") == 1
    assert code.count("__global__") == 2 and "batch_decode_forward_kernel" in code and "batch_decode_trace_kernel" in code
    for word in ("__shared__", "__syncthreads", "atomic", "extern"):
        assert word not in code, word
    assert re.search(r"[^_\w]fma\s*\(", code) is None and "dmul_rn" not in code, "additions and comparisons only"
    forward = code.split("void batch_decode_forward_kernel")[1].split("void batch_decode_trace_kernel")[0]
    assert forward[forward.index("{") + 1:].lstrip().startswith("#pragma clang fp contract(off)")
    for other in ("batch_smooth.hpp", "batch_suffstats.hpp", "batch_forecast.hpp"):
        assert "decode" not in open(os.path.join(csrc, other)).read().lower()
    assert '#include "batch_decode.hpp"' in open(os.path.join(csrc, "cpprob_hip.hip")).read()


_OPTIONS_TU = r"""
#include <cstdint>
#include <string>
#include <tuple>
#include <vector>
#include <boost/random/normal_distribution.hpp>
#include "cpprob/cpprob.hpp"

void model(const double& y) { cpprob::observe(boost::random::normal_distribution<>{0, 1}, y); }

int main()
{
    cpprob::gpu::options().map_decode = true;
    std::vector<std::tuple<double>> obs{std::make_tuple(0.5), std::make_tuple(-0.5)};
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        const std::vector<cpprob::gpu::Result> r = cpprob::gpu::inference_batch(cpprob::StateType::smc, model, obs, 1024, seeds);
        const std::vector<cpprob::gpu::Result> q = cpprob::gpu::hmm_table_batch(tables, {{0.5, 0.25}}, {512}, seeds);
        const cpprob::gpu::HmmTableFit fit = cpprob::gpu::hmm_table_fit(tables, {{0.5, 0.25}}, {512}, seeds, 2);
        cpprob::gpu::options().decode_lag = 1;
        cpprob::gpu::HmmTableStream stream(tables, {4}, {512}, seeds);
        const std::vector<cpprob::gpu::Result> s = stream.advance({{0.25, 0.125}, {1.0}});
        return r.size() == 2 && q[0].map_decoded && q[0].map_path.size() == 2 && fit.results[0].map_score < 0 && s[1].map_path.size() == 1 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_decode_options_compile_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """Options::map_decode / ::decode_lag and the entry points that read them are plain C++14 host code (the pattern of
    tests/test_batch_forecast_host.py)."""
    src = tmp_path / "decode.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "decode.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]


def test_cli_refusals():
    """cpprob_main --decode outside the batch modes, --decode_lag without --decode and --decode on a filtering-only batch without
    its masses end with a message before anything touches a device."""
    main = os.path.join(ROOT, "cpprob_amd", "bin", "cpprob_main")
    p = subprocess.run([main, "--smc", "--model", "hmm16", "--observes", "1", "--decode"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--decode serves the batch modes" in p.stderr
    p = subprocess.run([main, "--smc", "--model", "hmm16", "--batch_observes_file", "none.txt", "--decode_lag", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--decode_lag delays a decode" in p.stderr
    p = subprocess.run([main, "--smc", "--model", "hmm16", "--batch_observes_file", "none.txt", "--decode", "--filtering_only"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--keep_masses" in p.stderr
