"""cpprob_amd.gibbs.sample_tables with emission scales, on the host: the conjugate draw of every state's variance against the
inverse-gamma posterior's mean, and a call without sigmas against the generator it consumed before the scales existed."""
import math

import numpy as np

from cpprob_amd import gibbs


def _stats(B, k, seed):
    rng = np.random.default_rng(seed)
    st = {"xi": np.zeros((B, 8, 8)), "occ": np.zeros((B, 8)), "occ_y": np.zeros((B, 8)), "occ_yy": np.zeros((B, 8))}
    st["xi"][:, :k, :k] = rng.integers(0, 20, (k, k))
    occ = rng.integers(30, 60, k).astype(float)
    mean, sd = rng.uniform(-2.0, 2.0, k), rng.uniform(0.5, 2.0, k)
    st["occ"][:, :k], st["occ_y"][:, :k], st["occ_yy"][:, :k] = occ, occ * mean, occ * (sd * sd + mean * mean)
    return st


def test_variance_draw_has_the_posterior_mean():
    """20000 draws from identical statistics.  Given the mean mu_i drawn, the variance is inverse-gamma(shape, rate_i) with mean
    rate_i / (shape - 1): the mean over the draws of variance_i - rate_i / (shape - 1) lies within 5 of its standard errors of 0."""
    N, k, a0, b0 = 20000, 3, 2.0, 1.0
    st = _stats(N, k, 1)
    sigmas = np.full((N, k), 1.3)
    means, trans, new = gibbs.sample_tables(st, k, np.random.default_rng(2), sigmas=sigmas, a0=a0, b0=b0)
    assert means.shape == new.shape == (N, k) and trans.shape == (N, k, k) and np.all(new > 0.0)
    occ, occ_y, occ_yy = st["occ"][:, :k], st["occ_y"][:, :k], st["occ_yy"][:, :k]
    shape = a0 + occ / 2
    rate = b0 + (occ_yy - 2 * means * occ_y + means * means * occ) / 2
    d = new * new - rate / (shape - 1)
    se = d.std(axis=0, ddof=1) / math.sqrt(N)
    print("mean variance", (new * new).mean(axis=0), "posterior mean", (rate / (shape - 1)).mean(axis=0), "standard error", se)
    assert np.all(np.abs(d.mean(axis=0)) <= 5.0 * se)
    # the mean's posterior uses the current sigma
    prec = 1 / 10.0**2 + occ / 1.3**2
    zs = (means - (occ_y / 1.3**2) / prec) * np.sqrt(prec)
    assert np.all(np.abs(zs.mean(axis=0)) <= 5.0 / math.sqrt(N)) and np.all(np.abs(zs.std(axis=0) - 1.0) < 0.05)


def test_a_call_without_sigmas_consumes_the_generator_as_before():
    B, k = 7, 4
    st = _stats(B, k, 3)
    rng, old = np.random.default_rng(9), np.random.default_rng(9)
    means, trans = gibbs.sample_tables(st, k, rng)
    G = old.standard_gamma(1.0 + st["xi"][:, :k, :k])
    z = old.standard_normal((B, k))
    prec = 1 / 10.0**2 + st["occ"][:, :k]
    assert np.array_equal(trans, G / G.sum(-1, keepdims=True)) and np.array_equal(means, (0.0 / 10.0**2 + st["occ_y"][:, :k]) / prec + z / np.sqrt(prec))
    assert rng.bit_generator.state == old.bit_generator.state
    # with sigmas: the same two draws first, then one standard_gamma call
    rng2 = np.random.default_rng(9)
    _, t2, _ = gibbs.sample_tables(st, k, rng2, sigmas=np.ones((B, k)))
    old.standard_gamma(2.0 + st["occ"][:, :k] / 2)
    assert np.array_equal(t2, trans) and rng2.bit_generator.state == old.bit_generator.state


def test_forecast_helpers_with_scales():
    """The forecast of the observe and the predictive likelihood under N(mu[s], sigma[s]) against the mixture's moments and density
    written out; with every sigma 1.0 they are the unit forms (to rounding: the sums are associated differently)."""
    from cpprob_amd import forecast
    from oracle import exact
    rng = np.random.default_rng(4)
    k = 3
    f = np.zeros((5, 8))
    f[:, :k] = rng.dirichlet(np.ones(k), 5)
    mu, sg = np.array([-1.0, 0.5, 2.0]), np.array([0.3, 1.0, 2.5])
    mean, var = forecast.observation_forecast(f, mu, sg)
    want_mean = (f[:, :k] * mu).sum(axis=1)
    want_var = (f[:, :k] * (sg * sg + (mu - want_mean[:, None]) ** 2)).sum(axis=1)
    assert np.allclose(mean, want_mean, rtol=0, atol=1e-14) and np.allclose(var, want_var, rtol=0, atol=1e-13)
    m1, v1 = forecast.observation_forecast(f, mu, np.ones(k))
    m0, v0 = forecast.observation_forecast(f, mu)
    assert np.array_equal(m1, m0) and np.allclose(v1, v0, rtol=0, atol=1e-14)
    y = rng.normal(0.0, 2.0, 5)
    got = forecast.predictive_log_likelihood(f, mu, y, sg)
    want = np.log((f[:, :k] * np.exp(exact.normal_logpdf(y[:, None], mu[None, :], sg[None, :]))).sum(axis=1))
    assert np.allclose(got, want, rtol=0, atol=1e-13)
    assert np.allclose(forecast.predictive_log_likelihood(f, mu, y, np.ones(k)), forecast.predictive_log_likelihood(f, mu, y), rtol=0, atol=1e-14)
