"""csrc/batch_diag.hpp restated in plain Python: the diagonal rows and log_norms, the check, the weighted sums of the backward walk and
the M-step.  Every operation is one IEEE float64 operation; the one logarithm is scale_ref.table_log, the one root math.sqrt."""
import math

import numpy as np

import backward_ref as R2
import retable_ref as R
import scale_ref as S

MAX_DIM = 32
RECORD = 88 + 8 * 2 * MAX_DIM


def log_norms(sigmas):
    """[k]: ((0.0 + log_norm(sigma[s][0])) + log_norm(sigma[s][1])) + ..."""
    out = []
    for row in np.asarray(sigmas, np.float64):
        tot = 0.0
        for sg in row:
            tot = tot + S.log_norm(sg)
        out.append(tot)
    return np.array(out)


def rows(y, means, sigmas):
    """[T, 8]: entry s < k is (q + log_norm[s]) (-0.5), q the squared residuals added ascending over d from 0.0; -inf for s >= k and
    for a step with an infinite coordinate."""
    y, means, sigmas = np.asarray(y, np.float64), np.asarray(means, np.float64), np.asarray(sigmas, np.float64)
    (k, D), ln = means.shape, log_norms(sigmas)
    y = y.reshape(-1, D)
    out = np.full((len(y), 8), -np.inf)
    with np.errstate(all="ignore"):
        for s in range(k):
            q = np.zeros(len(y))
            for d in range(D):
                r = (y[:, d] - means[s, d]) / sigmas[s, d]
                q = q + r * r
            out[:, s] = np.where(np.isinf(y).any(axis=1), -np.inf, (q + ln[s]) * np.float64(-0.5))
    return out


def check(means, sigmas, trans):
    """The transition rows' two bits, bit 4 for a mean that is not finite, bit 8 for a sigma scale_ref.bad refuses."""
    means, sigmas = np.asarray(means, np.float64), np.asarray(sigmas, np.float64)
    bits = R.check(np.zeros(means.shape[0]), trans, means.shape[0])
    bits |= R.BAD_MEAN if not np.isfinite(means).all() else 0
    return bits | (S.BAD_SCALE if any(S.bad(sg) for sg in sigmas.reshape(-1)) else 0)


def sums(m, P, obs, D):
    """(sy, syy) [8, 32] of one problem from its masses m[t][0..8), its transition integers P[s][s'] and its observes [T, D]:
    g_t[s] y_t[d] and g_t[s] (y_t[d] y_t[d]) (backward_ref.marginals' g, the walk's own operations) added t = T-1 .. 0 from 0.0.  A last
    row of zeros (the exact run was dead) divides 0 by 0 on the device: every marginal of the walk is NaN."""
    T, k = len(m), len(P)
    y = np.asarray(obs, np.float64).reshape(T, D)
    mr = [[int(v) for v in row[:k]] for row in m]
    g = R2.marginals(mr, P) if sum(mr[-1]) else np.full((T, k), np.nan)
    sy, syy = np.zeros((8, MAX_DIM)), np.zeros((8, MAX_DIM))
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            gt = np.asarray(g[t], np.float64)[:, None]
            sy[:k, :D] = sy[:k, :D] + gt * y[t][None, :]
            syy[:k, :D] = syy[:k, :D] + gt * (y[t] * y[t])[None, :]
    return sy, syy


def m_step(rec, means, sigmas, trans, floor):
    """One problem's diagonal M-step on its record [600]: new (means [k, D], sigmas [k, D], trans [k, k])."""
    rec = np.asarray(rec, np.float64).reshape(RECORD)
    means, sigmas = np.array(means, np.float64), np.array(sigmas, np.float64)
    k, D = means.shape
    _, trans = R.m_step(rec[:88], np.zeros(k), trans, k)
    for s in range(k):
        occ = float(rec[64 + s])
        if occ > 0.0:
            for d in range(D):
                means[s, d] = float(rec[88 + 64 * s + d]) / occ
                sigmas[s, d] = S.sigma_step(occ, rec[88 + 64 * s + 32 + d], means[s, d], floor)
    return means, sigmas, trans
