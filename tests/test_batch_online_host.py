"""CPU tests of the batch advanced in pieces (include/cpprob_hip.h: cpprob_hip_batch_online_workspace_bytes, _begin_online, _advance,
_lengths): the workspace function is a pure host function, so the validation of such a batch and the workspace it needs are checked
without a GPU; cpprob::gpu::HmmTableStream is plain C++14.  The cases mirror tests/test_batch_problems_host.py, with capacities in
the lengths' place."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd.capi as cp

EINVAL, EUNSUPPORTED = -1, -4


def _round(x):
    return (x + 255) // 256 * 256


def _regions(cap, n, spp, keep):
    """The workspace the header documents: the twelve regions of a batch of problems of lengths `cap`, then the first steps, the
    snapshots and (filtering) the carried generations; each rounded up to 256 bytes."""
    cap, n = np.asarray(cap, np.int64), np.asarray(n, np.int64)
    B, Tm, S, N = len(cap), int(cap.max()), int((cap * n).sum()), int(n.sum())
    described = [64 * B * Tm, 8 * B, 512 * B, 256 * B, 8 * B * Tm * spp, 8 * B * Tm, 4 * B * Tm, 4 * B, 16 * B, 4 * B, S if keep else 0, 4 * S if keep else 0]
    return described + [4 * B, 32 * B, 0 if keep else N]


def _formula(cap, n, spp, keep):
    return sum(_round(r) for r in _regions(cap, n, spp, keep))


SHAPES = [
    ([16], [1024]),
    ([1], [1]),
    ([16] * 7, [4096] * 7),
    ([1, 2, 5, 16, 40, 128], [1, 2, 777, 1025, 4099, 8192]),
    ([128, 1, 1, 1], [8192, 1, 8192, 1]),
    ([5, 40, 5], [8192, 8192, 8192]),
    ([3] * 1024, [512, 4096] * 512),
]


@pytest.mark.parametrize("model,rs,keep", list(itertools.product([cp.MODEL_HMM3, cp.MODEL_HMM_TABLE], [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED], [True, False])))
def test_workspace_bytes_is_the_documented_formula(model, rs, keep):
    spp = 3 if model == cp.MODEL_HMM3 else 8
    for cap, n in SHAPES:
        got = cp.batch_online_workspace_bytes(model, cap, n, resampler=rs, keep_history=keep, ess_threshold=2.0)
        assert got == _formula(cap, n, spp, keep), (cap, n)
        assert cp.batch_online_workspace_bytes(model, cap, n, max_particles=8192, resampler=rs, keep_history=keep) == got
        # what it holds beyond the described batch of the same lengths: first steps, snapshots, the carried generation
        B, N = len(cap), int(np.sum(n))
        described = cp.batch_problems_workspace_bytes(model, cap, n, resampler=rs, keep_history=keep)
        assert got - described == _round(4 * B) + _round(32 * B) + (0 if keep else _round(N))


def _code(**kw):
    """tests/test_batch_problems_host.py::_code through the new function: four problems of capacity 16 and 1024 particles."""
    args = dict(model=cp.MODEL_HMM3, n_particles=1024, n_problems=4, T=16)
    args.update(kw)
    B = args.pop("n_problems")
    cap = [args.pop("T")] * B
    n = args.pop("n_particles")
    with pytest.raises(cp.CpprobHipError) as e:
        cp.batch_online_workspace_bytes(args.pop("model"), cap, [n] * B, max_particles=n, **args)
    return e.value.code


def test_workspace_bytes_rejects_bad_arguments():
    assert _code(n_problems=0) == EINVAL
    assert _code(n_particles=0) == EINVAL
    assert _code(n_particles=cp.BATCH_MAX_PARTICLES + 1) == EINVAL
    assert _code(T=0) == EINVAL
    assert _code(flags=1) == EINVAL
    assert _code(resampler=7) == EINVAL
    assert _code(model=42) == EINVAL
    assert cp.batch_online_workspace_bytes(cp.MODEL_HMM3, [1], [cp.BATCH_MAX_PARTICLES]) > 0


def test_workspace_bytes_rejects_what_runs_on_the_single_population_path():
    assert _code(resampler=cp.RESAMPLE_MULTINOMIAL) == EUNSUPPORTED
    assert _code(ess_threshold=1.0) == EUNSUPPORTED
    assert _code(ess_threshold=0.5) == EUNSUPPORTED
    assert _code(algorithm=cp.ALG_SIS) == EUNSUPPORTED
    for m in (cp.MODEL_GAUSSIAN_UNKNOWN_MEAN, cp.MODEL_GAUSSIAN_README, cp.MODEL_LINEAR_GAUSSIAN_1D, cp.MODEL_GAUSSIAN_2D_UNKNOWN_MEAN):
        assert _code(model=m) == EUNSUPPORTED
    msg = cp.load_library().cpprob_hip_last_error(None).decode()
    assert "single-population path" in msg


def test_workspace_bytes_rejects_bad_problem_shapes():
    def code(cap, n, **kw):
        with pytest.raises(cp.CpprobHipError) as e:
            cp.batch_online_workspace_bytes(cp.MODEL_HMM_TABLE, cap, n, **kw)
        return e.value.code, str(e.value)

    c, msg = code([16, 0, 16], [100, 100, 100])                      # h_Tcap[1] = 0
    assert c == EINVAL and "problem 1" in msg
    c, msg = code([16, 16, 16], [100, 100, 0])                       # h_n[2] = 0
    assert c == EINVAL and "problem 2" in msg
    c, msg = code([16, 16, 16], [100, 101, 100], max_particles=100)  # h_n[1] > cfg.n_particles
    assert c == EINVAL and "problem 1" in msg
    assert code([16, 16], [100, 8193])[0] == EINVAL                  # cfg.n_particles = 8193
    assert code([16, 16], [100, 100], max_particles=8193)[0] == EINVAL
    assert code([0, 0], [100, 100])[0] == EINVAL


def test_online_batch_symbols_are_declared_and_bound():
    L = cp.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cpprob_hip.h")).read()
    for s in ("cpprob_hip_batch_online_workspace_bytes", "cpprob_hip_batch_begin_online", "cpprob_hip_batch_advance", "cpprob_hip_batch_lengths"):
        assert s in cp.SYMBOLS
        assert hasattr(L, s)
        assert ("int %s(" % s) in header
    assert L.cpprob_hip_abi_version() == 3
    for name in ("batch_begin_online", "batch_advance", "batch_lengths"):
        assert callable(getattr(cp.Engine, name))


_STREAM_TU = r"""
#include <cstdint>
#include <vector>
#include "cpprob/cpprob.hpp"

int main()
{
    const std::vector<cpprob::gpu::HmmTable> tables{{{-1.0, 1.0}, {0.7, 0.3, 0.4, 0.6}}, {{-2.0, 2.0}, {0.5, 0.5, 0.1, 0.9}}};
    const std::vector<std::size_t> capacities{8}, n{1024, 2048};
    const std::vector<std::uint64_t> seeds{1, 2};
    try {
        cpprob::gpu::HmmTableStream stream(tables, capacities, n, seeds);
        stream.advance({{0.5, -0.5}, {}}, false);
        const std::vector<cpprob::gpu::Result> r = stream.advance({{0.25}, {1.5}});
        return r.size() == 2 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_hmm_table_stream_compiles_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """cpprob::gpu::HmmTableStream is plain C++14 host code: a translation unit using it compiles with -Wall -Wextra -pedantic and
    says nothing."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "stream.cpp"
    src.write_text(_STREAM_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "stream.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]
