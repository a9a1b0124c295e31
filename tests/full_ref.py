"""csrc/batch_full.hpp restated in plain Python: factor, rows, log_norms, the backward walk's weighted sums and the M-step.
Every operation is one IEEE float64 operation on Python floats; the one logarithm is scale_ref.table_log, the one root math.sqrt."""
import math

import numpy as np

import backward_ref as R2
import retable_ref as R
import scale_ref as S

MAX_DIM, TRI = 16, 136
RECORD = 88 + 8 * MAX_DIM + 8 * TRI
BAD_COV = 64


def factor(cov):
    """The lower-triangular L [D][D] of cov's lower triangle, column by column, or None where it does not factor."""
    D = len(cov)
    L = [[0.0] * D for _ in range(D)]
    for j in range(D):
        for i in range(j, D):
            a = float(cov[i][j])
            if not math.isfinite(a):
                return None
            for p in range(j):
                a = a - L[i][p] * L[j][p]
            if i == j:
                if not a > 0.0 or S.bad(math.sqrt(a)):
                    return None
                L[j][j] = math.sqrt(a)
            else:
                L[i][j] = a / L[j][j]
    return L


def log_norm(L):
    tot = 0.0
    for d in range(len(L)):
        tot = tot + float(S.log_norm(L[d][d]))
    return tot


def rows(y, means, covs):
    """[T, 8]: entry s < k is (q + log_norm[s]) (-0.5), q the substitution's squares added ascending; -inf for s >= k or an infinite y_d."""
    means = np.asarray(means, np.float64)
    k, D = means.shape
    y = np.asarray(y, np.float64).reshape(-1, D)
    out = np.full((len(y), 8), -np.inf)
    for s in range(k):
        L = factor(covs[s])
        ln = log_norm(L)
        for t in range(len(y)):
            if np.isinf(y[t]).any():
                continue
            z, q = [], 0.0
            for i in range(D):
                a = float(y[t, i]) - float(means[s, i])
                for p in range(i):
                    a = a - L[i][p] * z[p]
                a = a / L[i][i]
                z.append(a)
                q = q + a * a
            out[t, s] = (q + ln) * -0.5
    return out


def sums(m, P, obs, D):
    """The tail [RECORD - 88] of one problem's record from its masses m[t][0..8), its transition integers P[s][s'] and its observes
    [T, D]: sy[s][d] at 16 s + d and syy[s][i][j], j <= i, at 128 + 136 s + i (i + 1) / 2 + j, the products g_t[s] y_t[d] and
    g_t[s] (y_t[i] y_t[j]) (backward_ref.marginals' g) added t = T-1 .. 0 from 0.0.  A last row of zeros (the exact run was dead)
    divides 0 by 0 on the device: every marginal of the walk is NaN."""
    T, k = len(m), len(P)
    y = np.asarray(obs, np.float64).reshape(T, D).tolist()
    mr = [[int(v) for v in row[:k]] for row in m]
    g = np.asarray(R2.marginals(mr, P), np.float64).tolist() if sum(mr[-1]) else [[math.nan] * k] * T
    out = [0.0] * (RECORD - 88)
    for t in range(T - 1, -1, -1):
        for s in range(k):
            for i in range(D):
                out[16 * s + i] = out[16 * s + i] + g[t][s] * y[t][i]
                for j in range(i + 1):
                    at = 128 + TRI * s + i * (i + 1) // 2 + j
                    out[at] = out[at] + g[t][s] * (y[t][i] * y[t][j])
    return np.array(out)


def m_step(rec, means, covs, trans, floor):
    """One problem's full M-step on its record [1304]: new (means [k, D], covs [k, D, D], trans [k, k])."""
    rec = np.asarray(rec, np.float64).reshape(RECORD).tolist()
    means, covs = np.array(means, np.float64), np.array(covs, np.float64)
    k, D = means.shape
    _, trans = R.m_step(np.array(rec[:88]), np.zeros(k), trans, k)
    for s in range(k):
        occ = rec[64 + s]
        if not occ > 0.0:
            continue
        mu = [rec[88 + 16 * s + d] / occ for d in range(D)]
        c = [[0.0] * D for _ in range(D)]
        for i in range(D):
            for j in range(i + 1):
                c[i][j] = rec[216 + TRI * s + i * (i + 1) // 2 + j] / occ - mu[i] * mu[j]
            c[i][i] = c[i][i] if c[i][i] >= floor * floor else floor * floor
        if factor(c) is None:
            continue
        for i in range(D):
            means[s, i] = mu[i]
            for j in range(i + 1):
                covs[s, i, j] = covs[s, j, i] = c[i][j]
    return means, covs, trans
