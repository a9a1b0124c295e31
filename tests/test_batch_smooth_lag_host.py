"""CPU tests of fixed-lag smoothing of a batch (include/cpprob_hip.h: cpprob_hip_batch_smooth_lag*): the reference of
tests/lag_ref.py on the oracle's particle stores -- its identities with the full smoother of tests/backward_ref.py, the prefix property
the online path rests on, its error beside the lineage walk's -- then the pure host pieces: the symbols, the refusals that need no
device, and the C++ option."""
import os
import re

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd.capi as cp
import lag_ref as G
from oracle import exact
from oracle import oracle as O

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpprob_hip_batch_smooth_lag", "cpprob_hip_batch_smooth_lag_device")
N_PROBLEMS, T, N = 64, 32, 256
LAGS = (0, 1, 3, 8, T - 2, T - 1, T + 5)


@pytest.fixture(scope="module")
def problems():
    """tests/test_backward_ref_host.py's 64 HMM3 problems: (observes, oracle run, (m, P), full marginals), computed once."""
    out = []
    for b in range(N_PROBLEMS):
        obs = exact.simulate_hmm(T, 100 + b)
        r = O.smc(O.MODEL_HMM3, obs, N, 1000 + b, O.RESAMPLE_SYSTEMATIC, 2.0)
        m, P = R.hmm3_problem(r["hist"], obs)
        out.append((obs, r, (m, P), R.marginals(m, P)))
    return out


def _posterior(obs):
    truth = exact.hmm_forward_backward(obs)
    return truth[0] if isinstance(truth, tuple) else truth


# ---- the reference's identities ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [0, 7, 19])
def test_reference_identities(problems, b):
    _, _, (m, P), full = problems[b]
    filt = np.array([[float(x) / float(sum(row)) for x in row] for row in m])
    assert np.array_equal(G.fixed_lag_marginals(m, P, 0), filt), "lag 0 is not the normalised masses"
    for lag in (T - 1, T, T + 5):
        assert np.array_equal(G.fixed_lag_marginals(m, P, lag), full), lag
    for lag in LAGS:
        g = G.fixed_lag_marginals(m, P, lag)
        lo = max(T - 1 - lag, 0)
        assert g.shape == full.shape
        assert np.array_equal(g[lo:], full[lo:]), "lag %d: the rows whose end is T - 1 are not the full smoother's" % lag
        assert np.all(g >= 0.0) and np.abs(g.sum(axis=1) - 1.0).max() <= 1e-12, lag
        assert G.window(lag, T) == T - lo and [G.end_step(t, lag, T) for t in (0, T - 1)] == [min(lag, T - 1), T - 1]


@pytest.mark.parametrize("b", [1, 33])
@pytest.mark.parametrize("lag", [0, 1, 3, 8])
def test_prefix_property(problems, b, lag):
    """Row t is row t of the full smoother of the first t + lag + 1 steps: a final row never reads a later step."""
    _, _, (m, P), _ = problems[b]
    g = G.fixed_lag_marginals(m, P, lag)
    for t in range(T):
        assert np.array_equal(g[t], R.marginals(m[:t + lag + 1], P)[t]), (lag, t)
    # ... so a longer stream leaves the final rows alone
    for L in (lag + 1, 11, T - 1):
        final = max(L - lag, 0)
        assert np.array_equal(G.fixed_lag_marginals(m[:L], P, lag)[:final], g[:final]), (lag, L)


def test_window_trajectories_are_the_full_walks_last_rows(problems):
    _, _, (m, P), _ = problems[5]
    full = R.trajectories_fast(m, P, 77, 33, 3)
    for lag in (0, 3, T - 1, T + 2):
        W = G.window(lag, T)
        x = G.window_trajectories(m, P, 77, 33, lag, 3)
        assert x.shape == (W, 33) and np.array_equal(x, full[T - W:])


def test_lag8_rows_beat_the_lineage_walk(problems):
    """Mean absolute error over steps 0..15, averaged over the problems: the lag-8 rows against the exact posterior given the
    matching prefix y_0 .. y_{t+8}, beside the lineage walk's against the exact posterior given every observe -- each estimator
    against the quantity it estimates.  Measured: fixed lag 0.0177, lineage walk 0.0622 (ratio 3.52, better in 64 of 64 problems)."""
    err_g, err_l = [], []
    for obs, r, (m, P), _ in problems:
        g = G.fixed_lag_marginals(m, P, 8)
        truth = _posterior(obs)
        walk = O.smoothing(r["hist"], r["anc"], r["logw"])
        prefix = np.array([_posterior(obs[:t + 9])[t] for t in range(16)])
        err_g.append(np.abs(g[:16] - prefix).mean())
        err_l.append(np.abs(walk[:16] - truth[:16]).mean())
    eg, el = float(np.mean(err_g)), float(np.mean(err_l))
    print("fixed lag 8: %.4f, lineage walk %.4f, ratio %.2f, better in %d of %d" % (eg, el, el / eg, int(np.sum(np.array(err_g) < np.array(err_l))), N_PROBLEMS))
    assert eg < el


# ---- the C ABI's host pieces -------------------------------------------------------------------------------------------------
def test_lag_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == 10, s
    assert L.cpprob_hip_abi_version() == 3
    assert callable(cp.Engine.batch_smooth_lag) and callable(cp.Engine.batch_smooth_lag_device)
    import cpprob_amd
    assert cpprob_amd.Engine is cp.Engine


def test_lag_refusals_without_a_device():
    L = cp.load_library()
    marg = np.full(6, -5.0)
    traj = np.full(6, -5, np.int32)
    assert L.cpprob_hip_batch_smooth_lag(None, 2, None, 2, 3, 0, marg.ctypes.data, marg.size, traj.ctypes.data, traj.size) == EINVAL
    assert L.cpprob_hip_batch_smooth_lag_device(None, 2, None, 2, 3, 0, None, 0, None, 0) == EINVAL
    assert np.all(marg == -5.0) and np.all(traj == -5)
    # the wrapper's own shapes: one first step a problem; the windows' layout is cpprob_hip_batch_smooth_layout's of min(lag + 1, L_b)
    eng = cp.Engine.__new__(cp.Engine)
    eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K = 4, 23, 8, 8
    eng.batch_shapes = (np.array([1, 2, 7, 23], np.uint32), np.array([1, 300, 777, 1025], np.uint32))
    with pytest.raises(ValueError):
        eng._batch_lag_shapes(3, [0, 0])
    h_T, h_from, W, n_rows = eng._batch_lag_shapes(3, [1, 0, 7, 20])
    assert W.tolist() == [1, 2, 4, 4] and n_rows == 3 and h_from.dtype == np.uint32 and h_T.tolist() == [1, 2, 7, 23]
    _, none, W64, rows64 = eng._batch_lag_shapes(64, None)
    assert none is None and W64.tolist() == [1, 2, 7, 23] and rows64 == 23
    assert cp.batch_smooth_layout(W, 33).tolist() == [0, 33, 99, 231, 363]


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
    cpprob::gpu::options().smoothing_lag = 2;
    std::vector<std::tuple<double>> obs{std::make_tuple(0.5), std::make_tuple(-0.5)};
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        const std::vector<cpprob::gpu::Result> r = cpprob::gpu::inference_batch(cpprob::StateType::smc, model, obs, 1024, seeds);
        const std::vector<cpprob::gpu::Result> q = cpprob::gpu::hmm_table_batch(tables, {{0.5, 0.25}}, {512}, seeds);
        cpprob::gpu::HmmTableStream stream(tables, {4}, {512}, seeds);
        stream.advance({{0.5}, {}}, false);
        const std::vector<cpprob::gpu::Result> s = stream.advance({{0.25, 0.125}, {1.0}});
        return r.size() == 2 && q.size() == 2 && s.size() == 2 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_smoothing_lag_option_compiles_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """Options::smoothing_lag and the entry points that read it, the stream's kept rows included, are plain C++14 host code (the
    pattern of tests/test_backward_ref_host.py)."""
    import subprocess
    src = tmp_path / "lag.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "lag.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]
