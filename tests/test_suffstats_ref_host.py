"""CPU tests of the batch's expected sufficient statistics and of particle EM on them (include/cpprob_hip.h:
cpprob_hip_batch_smooth_stats*; cpprob_amd/em.py): the plain-Python reference of tests/suffstats_ref.py on the oracle's particle
stores -- its pair statistics have to beat the lineages' and satisfy the smoother's identities, and EM on them has to track exact
Baum-Welch -- then the M-step and the pure host pieces of the C ABI and the C++ interface."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd.capi as cp
import suffstats_ref as S
from cpprob_amd.em import m_step
from oracle import exact
from oracle import oracle as O

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cpprob_hip_batch_smooth_stats", "cpprob_hip_batch_smooth_stats_device")
N_PROBLEMS, T, N = 64, 32, 256


@pytest.fixture(scope="module")
def problems():
    """64 HMM3 problems (the ones of tests/test_backward_ref_host.py): (observes, oracle run, (m, P), reference statistics), once."""
    out = []
    for b in range(N_PROBLEMS):
        obs = exact.simulate_hmm(T, 100 + b)
        r = O.smc(O.MODEL_HMM3, obs, N, 1000 + b, O.RESAMPLE_SYSTEMATIC, 2.0)
        m, P = R.hmm3_problem(r["hist"], obs)
        out.append((obs, r, (m, P), S.stats(m, P, obs)))
    return out


def test_reference_pair_statistics_halve_the_lineages_error(problems):
    """Mean absolute error of the expected transition counts against exact forward-backward, averaged over the problems: the
    smoother's terms are at most one half of the weighted lineage pair counts' (measured: 0.0591 against 0.2091)."""
    err_s, err_l = [], []
    for obs, r, _, st in problems:
        truth = S.exact_stats(obs, exact.HMM_MEAN, exact.HMM_T)[0]
        walk = S.lineage_pair_counts(r["hist"], r["anc"], r["logw"], 3)
        err_s.append(np.abs(st["xi"][:3, :3] - truth).mean())
        err_l.append(np.abs(walk - truth).mean())
    es, el = float(np.mean(err_s)), float(np.mean(err_l))
    print("smoother's terms %.4f, lineage pair counts %.4f, ratio %.2f, better in %d of %d" % (es, el, el / es, int(np.sum(np.array(err_s) < np.array(err_l))), N_PROBLEMS))
    assert es <= 0.5 * el


def test_reference_identities(problems):
    """occ is the marginals' column sums; the terms leaving a state and the last marginal make up its visits; every step but the
    last contributes one transition; the padding is zero."""
    for obs, _, (m, P), st in problems:
        g = R.marginals(m, P)
        xi, occ = st["xi"], st["occ"]
        assert np.abs(occ[:3] - g.sum(axis=0)).max() <= 1e-12 * T
        assert np.abs(xi.sum(axis=1)[:3] + S.last_marginal(m) - occ[:3]).max() <= 1e-12 * T
        assert abs(xi.sum() - (T - 1)) <= 1e-10
        assert abs(occ.sum() - T) <= 1e-10
        assert np.abs(st["occ_y"][:3] - g.T @ obs).max() <= 1e-12 * T * max(1.0, np.abs(obs).max())
        assert np.abs(st["occ_yy"][:3] - g.T @ (obs * obs)).max() <= 1e-12 * T * max(1.0, np.abs(obs).max()) ** 2
        assert np.all(xi[3:] == 0.0) and np.all(xi[:, 3:] == 0.0) and all(np.all(st[f][3:] == 0.0) for f in ("occ", "occ_y", "occ_yy"))
        assert S.record(st).shape == (S.RECORD,) and S.record(st)[8 * 1 + 2] == xi[1, 2] and S.record(st)[72] == st["occ_y"][0]


def test_reference_short_problems(problems):
    _, _, (m, P), _ = problems[3]
    one = S.stats(m[:1], P, [0.5])
    assert np.all(one["xi"] == 0.0) and np.array_equal(one["occ"][:3], S.last_marginal(m[:1])) and np.array_equal(one["occ_y"], one["occ"] * 0.5)
    none = S.stats([], P, [])
    assert np.all(S.record(none) == 0.0)
    blind = S.stats(m, P)
    assert np.all(blind["occ_y"] == 0.0) and np.all(blind["occ_yy"] == 0.0) and np.array_equal(blind["xi"], problems[3][3]["xi"])


# ---- the M-step ----------------------------------------------------------------------------------------------------------------
def _stats(B):
    return {"xi": np.zeros((B, 8, 8)), "occ": np.zeros((B, 8)), "occ_y": np.zeros((B, 8)), "occ_yy": np.zeros((B, 8))}


def test_m_step_on_hand_made_statistics():
    st = _stats(2)
    st["xi"][0, :2, :2] = [[3.0, 1.0], [2.0, 6.0]]
    st["occ"][0, :2], st["occ_y"][0, :2] = [4.0, 8.0], [-6.0, 12.0]
    st["xi"][1, :2, :2] = [[1.0, 0.0], [0.0, 5.0]]
    st["occ"][1, :2], st["occ_y"][1, :2] = [2.0, 5.0], [1.0, -10.0]
    means0, trans0 = np.zeros((2, 2)), np.full((2, 2, 2), 0.5)
    means, trans = m_step(st, means0, trans0)
    assert np.array_equal(trans, [[[0.75, 0.25], [0.25, 0.75]], [[1.0, 0.0], [0.0, 1.0]]])
    assert np.array_equal(means, [[-1.5, 1.5], [0.5, -2.0]])
    assert np.all(means0 == 0.0) and np.all(trans0 == 0.5), "the M-step changed its arguments"


def test_m_step_keeps_what_has_no_mass():
    st = _stats(1)
    st["xi"][0, 0, :3] = [1.0, 1.0, 2.0]                      # rows 1 and 2 have no mass
    st["occ"][0, :3], st["occ_y"][0, :3] = [2.0, 0.0, 4.0], [3.0, 7.0, -2.0]
    means0 = np.array([[9.0, 8.0, 7.0]])
    trans0 = np.array([[[0.2, 0.3, 0.5], [0.6, 0.3, 0.1], [0.1, 0.1, 0.8]]])
    means, trans = m_step(st, means0, trans0)
    assert np.array_equal(trans[0], [[0.25, 0.25, 0.5], [0.6, 0.3, 0.1], [0.1, 0.1, 0.8]])
    assert np.array_equal(means[0], [1.5, 8.0, -0.5])


def test_m_step_reads_k_states_only():
    """k = 3 of 8: what the statistics hold for states >= k (nothing, from the device; here poison) is not read."""
    st = _stats(1)
    for f in st:
        st[f][...] = 1e300
    st["xi"][0, :3, :3] = [[2.0, 1.0, 1.0], [0.0, 1.0, 3.0], [5.0, 5.0, 0.0]]
    st["occ"][0, :3], st["occ_y"][0, :3] = [1.0, 2.0, 4.0], [1.0, 1.0, 1.0]
    means, trans = m_step(st, np.zeros((1, 3)), np.full((1, 3, 3), 1.0 / 3.0))
    assert means.shape == (1, 3) and trans.shape == (1, 3, 3)
    assert np.array_equal(trans[0], [[0.5, 0.25, 0.25], [0.0, 0.25, 0.75], [0.5, 0.5, 0.0]])
    assert np.array_equal(means[0], [1.0, 0.5, 0.25])
    with pytest.raises(ValueError):
        m_step(st, np.zeros((1, 3)), np.zeros((1, 2, 2)))


# ---- particle EM against exact EM -----------------------------------------------------------------------------------------------
def em_case():
    """The case the CPU and GPU tests share: k = 2, T = 64, true means -1.5 / +1.5 and self-transition 0.9; the start is means
    -0.5 / +0.5 and uniform transitions."""
    rng = np.random.default_rng(4242)
    true_means = np.array([-1.5, 1.5])
    s, obs = int(rng.integers(0, 2)), np.zeros(64)
    for t in range(64):
        if t > 0 and rng.random() >= 0.9:
            s = 1 - s
        obs[t] = true_means[s] + rng.standard_normal()
    return obs, np.array([-0.5, 0.5]), np.full((2, 2), 0.5)


def test_particle_em_tracks_exact_em():
    """10 iterations, n = 256, seeds 4242 + iteration, the oracle's runs and the reference's statistics: after every iteration the
    means are within 0.05 and the transition rows within 0.02 of Baum-Welch run alongside from the same start (four times what such
    a case showed when the bounds were set: 0.012 and 0.003)."""
    obs, means, trans = em_case()
    em_means, em_trans = S.exact_em(obs, means, trans, 10)
    means, trans = means[None], trans[None]
    worst_m = worst_t = 0.0
    for it in range(10):
        O.set_hmm(means[0], trans[0])
        r = O.smc(O.MODEL_HMM_TABLE, obs, 256, 4242 + it, O.RESAMPLE_SYSTEMATIC, 2.0)
        m, P = R.table_problem(r["hist"], obs, means[0], trans[0])
        st = S.stats(m, P, obs)
        means, trans = m_step({f: v[None] for f, v in st.items()}, means, trans)
        dm, dt = float(np.abs(means[0] - em_means[it + 1]).max()), float(np.abs(trans[0] - em_trans[it + 1]).max())
        print("iteration %d: means %s (exact %s, off by %.4f), transition rows off by %.4f" % (it, means[0], em_means[it + 1], dm, dt))
        worst_m, worst_t = max(worst_m, dm), max(worst_t, dt)
        assert dm <= 0.05 and dt <= 0.02, "iteration %d: means off by %.4f, transition rows by %.4f" % (it, dm, dt)
    print("largest differences: means %.4f, transition rows %.4f" % (worst_m, worst_t))
    assert np.abs(em_means[-1] - [-1.5, 1.5]).max() < 0.6          # (the exact fit itself found the two levels)


# ---- the C ABI's and the C++ interface's host pieces ---------------------------------------------------------------------------------
def test_stats_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(cp.load_library(), s)
    assert cp.load_library().cpprob_hip_abi_version() == 3
    assert cp.STATS_PER_PROBLEM == S.RECORD
    import cpprob_amd
    assert cpprob_amd.m_step is m_step and callable(cpprob_amd.hmm_table_em)


def test_refusals_without_a_device():
    L = cp.load_library()
    rec = np.full(88, -5.0)
    obs = np.zeros(4)
    for fn in (L.cpprob_hip_batch_smooth_stats, L.cpprob_hip_batch_smooth_stats_device):
        assert fn(None, obs.ctypes.data, obs.size, rec.ctypes.data, rec.size) == EINVAL
        assert fn(None, None, 0, rec.ctypes.data, rec.size) == EINVAL
    assert np.all(rec == -5.0)
    assert b"ctx is NULL" in L.cpprob_hip_last_error(None)


def test_split_stats_names_the_record():
    rec = np.arange(2 * 88, dtype=np.float64).reshape(2, 88)
    st = cp.split_stats(rec)
    assert st["xi"].shape == (2, 8, 8) and st["xi"][1, 2, 5] == 88 + 8 * 2 + 5
    assert st["occ"][0].tolist() == list(range(64, 72)) and st["occ_y"][0, 0] == 72 and st["occ_yy"][1, 7] == 88 + 87


_FIT_TU = r"""
#include <cstdint>
#include <string>
#include <vector>
#include "cpprob/cpprob.hpp"

int main()
{
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        const cpprob::gpu::HmmTableFit fit = cpprob::gpu::hmm_table_fit(tables, {{0.5, 0.25}}, {512}, seeds, 3);
        const std::vector<cpprob::gpu::Result> q = cpprob::gpu::hmm_table_batch(tables, {{0.5, 0.25}}, {512}, seeds);
        return fit.tables.size() == 2 && fit.results.size() == 2 && q.size() == 2 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_table_fit_compiles_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """hmm_table_fit and the pieces it shares with hmm_table_batch are plain C++14 host code (the pattern of
    tests/test_backward_ref_host.py)."""
    src = tmp_path / "fit.cpp"
    src.write_text(_FIT_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "fit.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]
