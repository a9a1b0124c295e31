"""CPU tests of the batch's posterior traces (include/cpprob_hip.h: cpprob_hip_batch_paths*): the packed layout is a pure host
function, and the C++ entry points that write a batch's posterior files are plain C++14."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cpprob_amd.capi as cp

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpprob_hip_batch_paths_layout", "cpprob_hip_batch_paths", "cpprob_hip_batch_paths_device")

# n = 1, a partial tile, exactly one tile, one past a tile, several tiles and the maximum; T = 1 and T > 1
SHAPES_T = [1, 2, 1, 5, 16, 7, 3, 4]
SHAPES_N = [1, 1, 777, 2, 1024, 1025, 4099, 8192]


def test_paths_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(cp.load_library(), s)
    assert cp.load_library().cpprob_hip_abi_version() == 3


def _formula(T, n, cap):
    """first_b = sum_{b' < b} T_b' m_b', wfirst_b = sum_{b' < b} m_b' over the problems that have a length; m = n, or min(n, cap)."""
    first, wfirst = [0], [0]
    for Tb, nb in zip(T, n):
        m = nb if cap == 0 else min(nb, cap)
        first.append(first[-1] + Tb * m)
        wfirst.append(wfirst[-1] + (m if Tb else 0))
    return first, wfirst


@pytest.mark.parametrize("zero_at", [None, 0, 4, 7])
@pytest.mark.parametrize("cap", [0, 1, 1000, 1024, 9000])
def test_layout_is_the_formula(cap, zero_at):
    T = list(SHAPES_T)
    if zero_at is not None:
        T[zero_at] = 0
    first, wfirst = cp.batch_paths_layout(T, SHAPES_N, cap)
    f, w = _formula(T, SHAPES_N, cap)
    assert first.dtype == np.uint64 and first.tolist() == f
    assert wfirst.dtype == np.uint64 and wfirst.tolist() == w
    if zero_at is not None:
        assert first[zero_at] == first[zero_at + 1] and wfirst[zero_at] == wfirst[zero_at + 1]


def test_layout_of_a_uniform_batch_and_null_outputs():
    B, T, n = 5, 6, 1500
    first, wfirst = cp.batch_paths_layout([T] * B, n, 0)
    assert first.tolist() == [b * T * n for b in range(B + 1)] and wfirst.tolist() == [b * n for b in range(B + 1)]
    L = cp.load_library()
    h_T, h_n = np.array(SHAPES_T, np.uint32), np.array(SHAPES_N, np.uint32)
    u32 = C.POINTER(C.c_uint32)
    only = np.zeros(len(SHAPES_T) + 1, np.uint64)
    assert L.cpprob_hip_batch_paths_layout(h_T.ctypes.data_as(u32), h_n.ctypes.data_as(u32), len(SHAPES_T), 0, only.ctypes.data_as(C.POINTER(C.c_uint64)), None) == 0
    assert only.tolist() == _formula(SHAPES_T, SHAPES_N, 0)[0]
    assert L.cpprob_hip_batch_paths_layout(h_T.ctypes.data_as(u32), h_n.ctypes.data_as(u32), len(SHAPES_T), 7, None, only.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    assert only.tolist() == _formula(SHAPES_T, SHAPES_N, 7)[1]


def test_layout_refusals_are_einval():
    L = cp.load_library()
    u32, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    h_T, h_n = np.array([3, 4], np.uint32), np.array([10, 20], np.uint32)
    out = np.zeros(3, np.uint64)

    def call(T, n, B):
        return L.cpprob_hip_batch_paths_layout(None if T is None else T.ctypes.data_as(u32), None if n is None else n.ctypes.data_as(u32), B, 0,
                                               out.ctypes.data_as(u64), out.ctypes.data_as(u64))
    assert call(h_T, h_n, 2) == 0
    assert call(None, h_n, 2) == EINVAL
    assert call(h_T, None, 2) == EINVAL
    assert call(h_T, h_n, 0) == EINVAL
    assert call(h_T, np.array([10, 0], np.uint32), 2) == EINVAL
    assert call(h_T, np.array([cp.BATCH_MAX_PARTICLES + 1, 5], np.uint32), 2) == EINVAL
    assert call(h_T, np.array([cp.BATCH_MAX_PARTICLES, 5], np.uint32), 2) == 0
    with pytest.raises(cp.CpprobHipError) as e:
        cp.batch_paths_layout([1, 2], [5, 0])
    assert e.value.code == EINVAL


_DUMP_TU = r"""
#include <cstdint>
#include <string>
#include <tuple>
#include <vector>
#include <boost/random/normal_distribution.hpp>
#include "cpprob/cpprob.hpp"

void model(const double& y) { cpprob::observe(boost::random::normal_distribution<>{0, 1}, y); }

int main()
{
    cpprob::gpu::options().batch_dump_file = "post_smc";
    cpprob::gpu::options().dump_max_particles = 100;
    std::vector<std::tuple<double>> obs{std::make_tuple(0.5), std::make_tuple(-0.5)};
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        const std::vector<cpprob::gpu::Result> r = cpprob::gpu::inference_batch(cpprob::StateType::smc, model, obs, 1024, seeds);
        const std::vector<cpprob::gpu::Result> q = cpprob::gpu::hmm_table_batch(tables, {{0.5, 0.25}}, {512}, seeds);
        cpprob::gpu::HmmTableStream stream(tables, {4}, {512}, seeds);
        stream.advance({{0.5}, {}}, false);
        stream.dump(std::string("post_stream"));
        return r.size() == 2 && q.size() == 2 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_batch_dumps_compile_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """Options::batch_dump_file, inference_batch, hmm_table_batch and HmmTableStream::dump are plain C++14 host code: a translation
    unit using them compiles with -Wall -Wextra -pedantic and says nothing (the pattern of tests/test_batch_host.py)."""
    src = tmp_path / "dump.cpp"
    src.write_text(_DUMP_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "dump.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]
