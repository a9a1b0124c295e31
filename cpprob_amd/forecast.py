"""What to do with a batch's forecasts on the host (Engine.batch_forecast, Engine.batch_predictive): the forecast of the observe
itself and the one-step predictive likelihood of a stream, under the emission y | x = s ~ N(means[s], 1) of the HMM models -- or
N(means[s], sigmas[s]) where the batch carries per-state emission scales and the caller passes them, or Poisson(means[s]) with
emission="poisson" (the means are then the rates).  Pure numpy: the rows come from
the device, the emission is restated here."""
import math

import numpy as np

LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def _means(means, k_max):
    mu = np.asarray(means, np.float64).reshape(-1)
    if mu.size == 0 or mu.size > k_max:
        raise ValueError("%d means for rows of %d states" % (mu.size, k_max))
    return mu


def _sigmas(sigmas, mu):
    sg = np.asarray(sigmas, np.float64).reshape(-1)
    if sg.size != mu.size:
        raise ValueError("%d sigmas for %d means" % (sg.size, mu.size))
    return sg


def _family(emission, sigmas):
    if emission not in ("normal", "poisson"):
        raise ValueError('emission is "normal" or "poisson"')
    if emission == "poisson" and sigmas is not None:
        raise ValueError("a Poisson emission has no scales")
    return emission == "poisson"


def observation_forecast(marginals, means, sigmas=None, emission="normal"):
    """(mean, variance) of y_{L-1+h} for every row of `marginals` ([..., spp], a law over the states in its last axis; the states
    past len(means) carry no mass): mean = sum_s f[s] mu[s], variance = 1 + sum_s f[s] mu[s]^2 - mean^2.  sigmas [k] (a batch with
    emission scales): variance = sum_s f[s] (sigma[s]^2 + mu[s]^2) - mean^2.  emission="poisson" (means the rates lambda): mean =
    sum_s f[s] lambda[s], variance = sum_s f[s] lambda[s] + sum_s f[s] lambda[s]^2 - mean^2."""
    poisson = _family(emission, sigmas)
    f = np.asarray(marginals, np.float64)
    if f.ndim < 1:
        raise ValueError("marginals must have the states in their last axis")
    mu = _means(means, f.shape[-1])
    fk = f[..., :mu.size]
    mean = fk @ mu
    if poisson:
        return mean, fk @ mu + fk @ (mu * mu) - mean * mean
    if sigmas is None:
        return mean, 1.0 + fk @ (mu * mu) - mean * mean
    sg = _sigmas(sigmas, mu)
    return mean, fk @ (sg * sg + mu * mu) - mean * mean


def predictive_log_likelihood(rows, means, observes, sigmas=None, emission="normal"):
    """log p(y_t | y_0 .. y_{t-1}) = log sum_s r_t[s] N(y_t; mu[s], 1) for every observe, by log-sum-exp: rows [T', spp] with
    T' >= len(observes) (row t the predictive law of step t, Engine.batch_predictive's rows of one problem; the rows past the observes
    -- the forecast of the step to come -- are not read), observes [T].  Their sum is the log-evidence of the observes under the
    rows.  sigmas [k] (a batch with emission scales): the density is N(y_t; mu[s], sigma[s]).  emission="poisson" (means the rates,
    observes counts): the mass is Poisson(y_t; lambda[s]) = exp(y_t log lambda[s] - lambda[s] - lgamma(y_t + 1))."""
    poisson = _family(emission, sigmas)
    r = np.asarray(rows, np.float64)
    y = np.asarray(observes, np.float64).reshape(-1)
    if r.ndim != 2 or r.shape[0] < y.size:
        raise ValueError("rows must be [T', spp] with a row for every observe")
    mu = _means(means, r.shape[1])
    r = r[:y.size, :mu.size]
    with np.errstate(divide="ignore"):
        if poisson:
            lf = np.array([math.lgamma(v + 1.0) for v in y])
            a = np.log(r) + y[:, None] * np.log(mu)[None, :] - mu[None, :] - lf[:, None]
        elif sigmas is None:
            a = np.log(r) - 0.5 * (y[:, None] - mu[None, :]) ** 2 - LOG_SQRT_2PI
        else:
            sg = _sigmas(sigmas, mu)
            a = np.log(r) - 0.5 * ((y[:, None] - mu[None, :]) / sg[None, :]) ** 2 - LOG_SQRT_2PI - np.log(sg)[None, :]
    top = a.max(axis=1) if y.size else np.zeros(0)
    return top + np.log(np.exp(a - top[:, None]).sum(axis=1))
