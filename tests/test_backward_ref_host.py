"""CPU tests of the batch's backward smoother (include/cpprob_hip.h: cpprob_hip_batch_smooth*): the fixed-point reference of
tests/backward_ref.py on the oracle's particle stores -- it has to beat the lineage walk it replaces and its trajectories have to
follow its marginals -- then the pure host pieces of the C ABI: the packed layout and the symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd.capi as cp
from oracle import exact
from oracle import oracle as O

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpprob_hip_batch_smooth_layout", "cpprob_hip_batch_smooth", "cpprob_hip_batch_smooth_device", "cpprob_hip_batch_smooth_grid")
N_PROBLEMS, T, N = 64, 32, 256


@pytest.fixture(scope="module")
def problems():
    """The issue's 64 HMM3 problems: (observes, oracle run, (m, P), reference marginals), computed once."""
    out = []
    for b in range(N_PROBLEMS):
        obs = exact.simulate_hmm(T, 100 + b)
        r = O.smc(O.MODEL_HMM3, obs, N, 1000 + b, O.RESAMPLE_SYSTEMATIC, 2.0)
        m, P = R.hmm3_problem(r["hist"], obs)
        out.append((obs, r, (m, P), R.marginals(m, P)))
    return out


def test_reference_marginals_halve_the_lineage_walks_error(problems):
    """Mean absolute error of P(x_t = s | y) over steps 0..15 against the exact posterior, averaged over the problems: the backward
    smoother's is at most one half of the lineage walk's (measured in floating point: 0.0177 against 0.0622)."""
    err_b, err_l = [], []
    for obs, r, _, g in problems:
        truth = exact.hmm_forward_backward(obs)
        truth = truth[0] if isinstance(truth, tuple) else truth
        walk = O.smoothing(r["hist"], r["anc"], r["logw"])
        err_b.append(np.abs(g[:16] - truth[:16]).mean())
        err_l.append(np.abs(walk[:16] - truth[:16]).mean())
    eb, el = float(np.mean(err_b)), float(np.mean(err_l))
    print("backward smoother %.4f, lineage walk %.4f, ratio %.2f, better in %d of %d" % (eb, el, el / eb, int(np.sum(np.array(err_b) < np.array(err_l))), N_PROBLEMS))
    assert eb <= 0.5 * el


def test_reference_marginals_are_distributions(problems):
    for _, _, _, g in problems:
        assert np.all(g >= 0.0) and np.allclose(g.sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("b", [0, 1, 2, 3])
def test_reference_trajectories_follow_the_marginals(problems, b):
    """M = 16384 backward draws: the frequency of x_t = s is within 0.02 of g_t[s] (five standard deviations at this M)."""
    _, _, (m, P), g = problems[b]
    M = 16384
    traj = R.trajectories_fast(m, P, 1000 + b, M)
    freq = np.stack([(traj == s).mean(axis=1) for s in range(3)], axis=1)
    print("problem %d: largest |frequency - marginal| = %.4f" % (b, np.abs(freq - g).max()))
    assert np.abs(freq - g).max() <= 0.02


def test_vectorised_walk_is_the_plain_one(problems):
    _, _, (m, P), _ = problems[5]
    for di in (0, 3):
        assert np.array_equal(R.trajectories(m, P, 77, 33, di), R.trajectories_fast(m, P, 77, 33, di))
    assert not np.array_equal(R.trajectories_fast(m, P, 77, 33, 0), R.trajectories_fast(m, P, 77, 33, 3))


def test_columns_are_the_full_walks_columns(problems):
    """trajectories_fast(columns=...) draws only the blocks it needs and returns those columns of the full result: both ends of
    the range, both halves of a block, repeats and an order that is not sorted."""
    _, _, (m, P), _ = problems[7]
    M = 1025
    full = R.trajectories_fast(m, P, 91, M, 255)
    rng = np.random.default_rng(3)
    for cols in ([0], [M - 1], [1024, 0, 1, 1, 513, 2, 1023], rng.choice(M, 300, replace=False), np.arange(M), []):
        got = R.trajectories_fast(m, P, 91, M, 255, columns=cols)
        assert got.dtype == np.int32 and got.shape == (T, len(cols))
        assert np.array_equal(got, full[:, np.asarray(cols, np.int64)]), cols
    assert np.array_equal(R.trajectories_fast(m, P, 91, 1 << 20, 255, columns=[5, 1024]), full[:, [5, 1024]])     # (n_traj is a bound only)


def test_integer_masses_of_the_hmm3_table():
    P = R.transition_masses(exact.HMM_T)
    assert all(sum(row) == 1 << 32 for row in P)
    assert np.allclose(np.array(P, np.float64) / 2.0**32, exact.HMM_T / exact.HMM_T.sum(axis=1, keepdims=True), atol=2.0**-31)
    P0 = R.transition_masses([[0.5, 0.0, 0.5], [1.0, 1.0, 0.0], [0.0, 0.0, 2.0]])
    assert P0 == [[1 << 31, 0, 1 << 31], [1 << 31, 1 << 31, 0], [0, 0, 1 << 32]]


# ---- the C ABI's host pieces -------------------------------------------------------------------------------------------------
def test_smooth_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(cp.load_library(), s)
    assert cp.load_library().cpprob_hip_abi_version() == 3


@pytest.mark.parametrize("n_traj", [0, 1, 1000, 1 << 20])
def test_layout_is_its_definition(n_traj):
    Ts = [1, 2, 0, 7, 64, 0, 3]
    first = cp.batch_smooth_layout(Ts, n_traj)
    assert first.dtype == np.uint64 and first.shape == (len(Ts) + 1,)
    assert first.tolist() == [n_traj * sum(Ts[:b]) for b in range(len(Ts) + 1)]


def test_layout_refusals_are_einval():
    L = cp.load_library()
    u32, u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    h_T = np.array([3, 4], np.uint32)
    out = np.zeros(3, np.uint64)

    def call(T_, B, n_traj, o=out):
        return L.cpprob_hip_batch_smooth_layout(None if T_ is None else T_.ctypes.data_as(u32), B, n_traj, None if o is None else o.ctypes.data_as(u64))
    assert call(h_T, 2, 5) == 0 and out.tolist() == [0, 15, 35]
    assert call(None, 2, 5) == EINVAL
    assert call(h_T, 2, 5, None) == EINVAL
    assert call(h_T, 0, 5) == EINVAL
    assert call(h_T, 2, (1 << 20) + 1) == EINVAL
    assert call(np.array([3, (1 << 24) + 1], np.uint32), 2, 5) == EINVAL
    assert call(np.array([3, 1 << 24], np.uint32), 2, 5) == 0
    with pytest.raises(cp.CpprobHipError) as e:
        cp.batch_smooth_layout([1, 2], (1 << 20) + 1)
    assert e.value.code == EINVAL


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
    cpprob::gpu::options().backward_smoothing = true;
    cpprob::gpu::options().backward_trajectories = 8;
    cpprob::gpu::options().batch_dump_file = "post_smc";
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
def test_backward_options_compile_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """Options::backward_smoothing / ::backward_trajectories and the entry points that read them are plain C++14 host code (the
    pattern of tests/test_batch_paths_host.py)."""
    import subprocess
    src = tmp_path / "smooth.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "smooth.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]
