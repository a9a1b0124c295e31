"""The law of the generator tests/gibbs_ref.py restates (csrc/batch_gibbs.hpp): the device equals the restatement bit for bit
(tests/test_gpu_batch_draw_tables.py), so its law is the restatement's.  Sample moments against the exact ones, within 5 standard errors
computed from the exact second and fourth central moments -- no threshold is measured."""
import math

import pytest

import gibbs_ref as GR

N = 20000
SEED = 0x5EED0123


def _moments(xs):
    m = math.fsum(xs) / len(xs)
    return m, math.fsum((x - m) * (x - m) for x in xs) / (len(xs) - 1)


def _within(xs, mean, var, mu4):
    """Sample mean and variance within 5 standard errors: Var(mean) = var / N, Var(s^2) = (mu4 - var^2 (N - 3) / (N - 1)) / N."""
    n = len(xs)
    m, v = _moments(xs)
    se_m, se_v = math.sqrt(var / n), math.sqrt((mu4 - var * var * (n - 3) / (n - 1)) / n)
    assert abs(m - mean) <= 5 * se_m, "mean %.6g, exact %.6g, standard error %.3g" % (m, mean, se_m)
    assert abs(v - var) <= 5 * se_v, "variance %.6g, exact %.6g, standard error %.3g" % (v, var, se_v)


@pytest.mark.parametrize("shape", [1.0, 1.5, 7.0, 1000.5])
def test_gamma_moments(shape):
    """Gamma(a): mean a, variance a, fourth central moment 3 a^2 + 6 a.  A slot a variate, sweeps 0 and 1: the words of 20 000 draws."""
    log = []
    draws = [GR.gamma(shape, SEED, i % 80, i // 80, log=log) for i in range(N)]
    assert all(ok for _, ok in draws)
    _within([g for g, _ in draws], shape, shape, 3 * shape * shape + 6 * shape)
    if shape == 1.0:
        # the attempts the polar step refused: a binomial share of the closed-form rate 1 - pi / 4 over this run's attempts
        p, n = 1 - math.pi / 4, len(log)
        refused = sum(1 for polar, _ in log if not polar)
        assert abs(refused / n - p) <= 5 * math.sqrt(p * (1 - p) / n), "polar refusals %d of %d attempts" % (refused, n)
        assert all(polar for polar, accepted in log if accepted)


def test_normal_moments():
    draws = [GR.normal(SEED, GR.MEAN_SLOT + i % 8, i // 8) for i in range(N)]
    assert all(ok for _, ok in draws)
    _within([z for z, _ in draws], 0.0, 1.0, 3.0)
