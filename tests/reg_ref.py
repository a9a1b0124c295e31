"""csrc/batch_reg.hpp restated in plain Python on scale_ref (rows, log_norms), full_ref (the record) and retable_ref (the transition
row): every operation is one IEEE float64 operation on Python floats, the one root math.sqrt."""
import math

import numpy as np

import full_ref as FR
import retable_ref as R
import scale_ref as S

RECORD = FR.RECORD


def rows(z, coef, sigmas):
    """[T, 8] from the observes z [T, 1 + P] = (y, x): entry s < k is scale_ref's row at the mean pred = ((0.0 + coef_0 x_0) + ..);
    -inf for s >= k and where y or a covariate is infinite."""
    coef = np.asarray(coef, np.float64)
    k, P = coef.shape
    z = np.asarray(z, np.float64).reshape(-1, 1 + P)
    out = np.full((len(z), 8), -np.inf)
    for t in range(len(z)):
        if np.isinf(z[t]).any():
            continue
        pred = []
        for s in range(k):
            a = 0.0
            for i in range(P):
                a = a + float(coef[s, i]) * float(z[t, 1 + i])
            pred.append(a)
        out[t] = S.rows(z[t, :1], pred, sigmas, k)[0]
    return out


def solve(A, b):
    """beta of A beta = b through A = L D L^T, column by column (A's lower triangle read), or None where the state is kept."""
    P = len(b)
    W, L, d = [[0.0] * P for _ in range(P)], [[0.0] * P for _ in range(P)], [0.0] * P
    if not all(math.isfinite(v) for v in b) or not all(math.isfinite(A[i][j]) for i in range(P) for j in range(i + 1)):
        return None
    for j in range(P):
        for i in range(j, P):
            a = float(A[i][j])
            for p in range(j):
                a = a - W[i][p] * L[j][p]
            if i == j:
                if not a > 0.0 or not a < math.inf:
                    return None
                d[j] = a
            else:
                W[i][j], L[i][j] = a, a / d[j]
    beta = [float(v) for v in b]
    for i in range(P):
        for p in range(i):
            beta[i] = beta[i] - L[i][p] * beta[p]
    for i in range(P):
        beta[i] = beta[i] / d[i]
    for p in range(P - 1, 0, -1):
        for i in range(p):
            beta[i] = beta[i] - L[p][i] * beta[p]
    return beta if all(math.isfinite(v) for v in beta) else None


def m_step(rec, coef, sigmas, trans, floor):
    """One problem's regression M-step on its record [1304]: new (coef [k, P], sigmas [k], log_norms [k] -- NaN for a state that is
    kept --, trans [k, k])."""
    rec = np.asarray(rec, np.float64).reshape(RECORD).tolist()
    coef, sigmas = np.array(coef, np.float64), np.array(sigmas, np.float64)
    k, P = coef.shape
    _, trans = R.m_step(np.array(rec[:88]), np.zeros(k), trans, k)
    log_norms = np.full(k, np.nan)
    for s in range(k):
        occ = rec[64 + s]
        tri = rec[216 + FR.TRI * s:216 + FR.TRI * (s + 1)]
        c0, b = tri[0], [tri[(1 + i) * (2 + i) // 2] for i in range(P)]
        A = [[tri[(1 + i) * (2 + i) // 2 + 1 + j] for j in range(i + 1)] for i in range(P)]
        beta = solve(A, b) if occ > 0.0 and math.isfinite(occ) and math.isfinite(c0) else None
        if beta is None:
            continue
        v = c0 / occ
        for i in range(P):
            v = v - beta[i] * (b[i] / occ)
        coef[s] = beta
        sigmas[s] = math.sqrt(v) if v >= floor * floor else floor
        log_norms[s] = math.nan if S.bad(sigmas[s]) else S.log_norm(sigmas[s])
    return coef, sigmas, log_norms, trans
