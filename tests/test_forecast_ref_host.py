"""CPU tests of the forecast's restatement (tests/forecast_ref.py) against things it does not define: the exact forward filter of
oracle/exact.py pushed through the real transition matrix, the frequencies of its own simulated futures, and the host pieces of
cpprob_amd.forecast against direct computations.

The exact filter: oracle/exact.py's hmm_forward_backward serves its own 3-state table; the 8-state table goes through the same
recursion written for k states (suffstats_ref.exact_stats' forward pass, on exact.normal_logpdf), and `_filter` is checked against
hmm_forward_backward on the 3-state table before it is used."""
import numpy as np
import pytest

import backward_ref as R
import forecast_ref as F
from cpprob_amd import forecast as CF
from oracle import exact
from oracle import oracle as O

T, N = 6, 4096


def _filter(obs, means, trans):
    """(filtering [T, k], predictive [T + 1, k], log-evidence) in floating point: uniform initial state, emission N(means[s], 1)."""
    obs, means = np.asarray(obs, np.float64), np.asarray(means, np.float64)
    A = np.asarray(trans, np.float64)
    A = A / A.sum(axis=1, keepdims=True)
    k = len(means)
    lik = np.exp(exact.normal_logpdf(obs[:, None], means[None, :], 1.0))
    alpha, pred, c = np.zeros((len(obs), k)), np.zeros((len(obs) + 1, k)), np.zeros(len(obs))
    pred[0] = 1.0 / k
    for t in range(len(obs)):
        a = pred[t] * lik[t]
        c[t] = a.sum()
        alpha[t] = a / c[t]
        pred[t + 1] = alpha[t] @ A
    return alpha, pred, float(np.log(c).sum()), A


def _table8():
    rng = np.random.default_rng(8)
    trans = rng.uniform(0.05, 1.0, (8, 8))
    trans[2, 5] = 0.0
    return np.linspace(-3.5, 3.5, 8), trans


@pytest.fixture(scope="module", params=["hmm3", "table8"])
def problem(request):
    """(k, means, trans, observes, m, P, thresholds, seed) of one oracle run of T = 6 steps."""
    if request.param == "hmm3":
        means, trans, seed = exact.HMM_MEAN, exact.HMM_T, 1003
        obs = exact.simulate_hmm(T, 103)
        r = O.smc(O.MODEL_HMM3, obs, N, seed, O.RESAMPLE_SYSTEMATIC, 2.0)
    else:
        (means, trans), seed = _table8(), 1008
        obs = np.random.default_rng(18).uniform(-3.0, 3.0, T)
        O.set_hmm(means, trans)
        r = O.smc(O.MODEL_HMM_TABLE, obs, N, seed, O.RESAMPLE_SYSTEMATIC, 2.0)
    m = R.filtering_masses(r["hist"], R.log_likelihoods(obs, means))
    return len(means), means, trans, obs, m, R.transition_masses(trans), R.thresholds(trans), seed


def test_the_k_state_filter_is_exacts_on_its_own_table():
    obs = exact.simulate_hmm(T, 103)
    _, alpha, logz = exact.hmm_forward_backward(obs)
    a, _, lz, _ = _filter(obs, exact.HMM_MEAN, exact.HMM_T)
    assert np.allclose(a, alpha, rtol=0, atol=1e-14) and abs(lz - logz) < 1e-12


def test_forecast_stays_within_the_filters_error(problem):
    """||f_h - exact_h||_1 <= ||f_0 - exact filter||_1 + h k 2^-32 + 1e-12: a stochastic matrix contracts L1, and each integer
    transition row differs from the real one by less than k 2^-32 in L1."""
    k, means, trans, obs, m, P, _, _ = problem
    alpha, _, _, A = _filter(obs, means, trans)
    assert np.abs(np.array(F.probabilities(P)) - A).sum(axis=1).max() < k * 2.0 ** -32
    f0 = np.array(F.start(m[-1]))
    e0 = np.abs(f0 - alpha[-1]).sum()
    H = 12
    f = F.marginals(m, P, H)
    ex = alpha[-1]
    for h in range(1, H + 1):
        ex = ex @ A
        err = np.abs(f[h - 1] - ex).sum()
        print("h = %d: L1 error %.3e (the filter's own %.3e)" % (h, err, e0))
        assert err <= e0 + h * k * 2.0 ** -32 + 1e-12
        assert abs(f[h - 1].sum() - 1.0) < 1e-12 and np.all(f[h - 1] >= 0.0)


def test_simulated_futures_follow_the_marginals(problem):
    """4096 trajectories, fixed seeds: every cell of the state frequencies at h = 1, 3 and 10 lies within 0.05 of f_h (Hoeffding:
    2 exp(-2 * 4096 * 0.05^2) < 3e-9 a cell); row 0 follows f_0."""
    k, _, _, _, m, P, thr, seed = problem
    M, H = 4096, 10
    f = F.marginals(m, P, H)
    traj = F.trajectories(m, thr, seed, H, M, draw_index=2)
    assert traj.shape == (H + 1, M) and traj.min() >= 0 and traj.max() < k
    for h in (1, 3, 10):
        freq = np.bincount(traj[h], minlength=k) / float(M)
        print("h = %d: largest |frequency - marginal| = %.4f" % (h, np.abs(freq - f[h - 1]).max()))
        assert np.all(np.abs(freq - f[h - 1]) <= 0.05)
    assert np.all(np.abs(np.bincount(traj[0], minlength=k) / float(M) - np.array(F.start(m[-1]))) <= 0.05)
    assert not np.array_equal(traj, F.trajectories(m, thr, seed, H, M, draw_index=3))
    assert np.array_equal(traj[:, :33], F.trajectories(m, thr, seed, H, 33, draw_index=2))       # (n_traj is a bound only)
    cols = [4095, 0, 1, 1023, 1024, 7, 6, 4094, 7]                 # (both halves of a block, one half alone, any order, one twice)
    assert np.array_equal(traj[:, cols], F.trajectories(m, thr, seed, H, M, draw_index=2, columns=cols))


def test_a_zero_transition_entry_is_never_taken():
    means, trans = _table8()
    P, thr = R.transition_masses(trans), R.thresholds(trans)
    assert P[2][5] == 0 and all(sum(row) == 1 << 32 for row in P)
    m = [[1000 + 37 * s for s in range(8)]]
    traj = F.trajectories(m, thr, 77, 40, 1025)
    assert np.sum(traj[:-1] == 2) > 1000
    assert not np.any((traj[:-1] == 2) & (traj[1:] == 5))
    assert np.any((traj[:-1] == 2) & (traj[1:] == 4)) and np.any((traj[:-1] == 1) & (traj[1:] == 5))
    f = F.marginals([[0, 0, 5, 0, 0, 0, 0, 0]], P, 1)
    assert f[0, 5] == 0.0 and np.array_equal(f[0], np.array(F.probabilities(P)[2]))


def test_predictive_rows_meet_the_forecast(problem):
    k, _, _, _, m, P, _, _ = problem
    r = F.predictive(m, P)
    assert r.shape == (T + 1, k)
    assert np.all(r[0] == 1.0 / k)
    assert np.array_equal(r[T], F.marginals(m, P, 1)[0])
    for L in (1, 3):                                           # (row t reads row t - 1 alone: the same at every length)
        assert np.array_equal(F.predictive(m[:L], P), r[:L + 1])
    out = F.predictive_rows(m, P, 2, 7, 8)
    assert np.array_equal(out[:5, :k], r[2:]) and np.all(out[5:] == 0.0) and np.all(out[:, k:] == 0.0)
    assert np.all(F.predictive_rows(m, P, T + 1, 3, 8) == 0.0)
    assert np.all(F.marginals([], P, 3) == 0.0) and np.all(F.trajectories([], None, 1, 3, 5) == 0)
    assert np.array_equal(F.predictive([], P), np.full((1, k), 1.0 / k))


def test_predictive_log_likelihood_sums_to_the_evidence(problem):
    _, means, trans, obs, _, _, _, _ = problem
    _, pred, logz, _ = _filter(obs, means, trans)
    ll = CF.predictive_log_likelihood(pred, means, obs)
    assert ll.shape == (T,) and abs(ll.sum() - logz) < 1e-10
    wide = np.zeros((T + 1, 8))
    wide[:, :len(means)] = pred
    assert np.array_equal(CF.predictive_log_likelihood(wide, means, obs), ll)
    # far out in the tails the densities underflow and log-sum-exp does not
    far = CF.predictive_log_likelihood(pred[:1], means, [60.0])
    assert np.isfinite(far[0]) and far[0] < -1000.0
    with pytest.raises(ValueError):
        CF.predictive_log_likelihood(pred[:2], means, obs)
    with pytest.raises(ValueError):
        CF.predictive_log_likelihood(pred[:, :2], means, obs)


def test_observation_forecast_is_the_mixtures_moments():
    rng = np.random.default_rng(4)
    means = np.array([-2.0, 0.5, 1.0, 4.0, 7.0])
    f = rng.dirichlet(np.ones(5), (3, 4))
    wide = np.zeros((3, 4, 8))
    wide[..., :5] = f
    mean, var = CF.observation_forecast(wide, means)
    assert mean.shape == (3, 4) and var.shape == (3, 4)
    # the mixture directly: E y = sum f mu, Var y = sum f (1 + (mu - E y)^2)
    for i in range(3):
        for j in range(4):
            ey = sum(f[i, j, s] * means[s] for s in range(5))
            vy = sum(f[i, j, s] * (1.0 + (means[s] - ey) ** 2) for s in range(5))
            assert abs(mean[i, j] - ey) < 1e-12 and abs(var[i, j] - vy) < 1e-10
    # and by numerical integration of the density of one row
    y = np.linspace(-12.0, 18.0, 60001)
    dens = sum(f[0, 0, s] * np.exp(exact.normal_logpdf(y, means[s], 1.0)) for s in range(5))
    dy = y[1] - y[0]
    ey = float(np.sum(y * dens) * dy)
    assert abs(ey - mean[0, 0]) < 1e-6 and abs(float(np.sum((y - ey) ** 2 * dens) * dy) - var[0, 0]) < 1e-6
    m1, v1 = CF.observation_forecast([1.0, 0.0, 0.0], [3.0, 0.0, -3.0])
    assert m1 == 3.0 and v1 == 1.0
    with pytest.raises(ValueError):
        CF.observation_forecast(wide, np.zeros(9))
