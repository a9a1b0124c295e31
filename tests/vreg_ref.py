"""csrc/batch_vreg.hpp restated in plain Python on full_ref (factor, log_norm, the record), reg_ref (the solve) and retable_ref (the
transition row): every operation is one IEEE float64 operation on Python floats.  exact_em is the exact-run EM of the whole chain."""
import math

import numpy as np

import backward_ref as R2
import exact_ref as X
import full_ref as FR
import reg_ref as RR
import retable_ref as R
import suffstats_ref as SS

RECORD = FR.RECORD


def rows(z, coef, covs):
    """[T, 8] from the observes z [T, Q + P] = (y, x): entry s < k is full_ref's row at the mean pred_q = ((0.0 + coef_q0 x_0) + ..);
    -inf for s >= k and where a response or a covariate is infinite."""
    coef = np.asarray(coef, np.float64)
    k, Q, P = coef.shape
    z = np.asarray(z, np.float64).reshape(-1, Q + P)
    out = np.full((len(z), 8), -np.inf)
    for t in range(len(z)):
        if np.isinf(z[t]).any():
            continue
        pred = np.zeros((k, Q))
        for s in range(k):
            for q in range(Q):
                a = 0.0
                for i in range(P):
                    a = a + float(coef[s, q, i]) * float(z[t, Q + i])
                pred[s, q] = a
        out[t] = FR.rows(z[t, :Q], pred, covs)[0]
    return out


def m_step(rec, coef, covs, trans, floor):
    """One problem's M-step on its record [1304]: new (coef [k, Q, P], covs [k, Q, Q], trans [k, k])."""
    rec = np.asarray(rec, np.float64).reshape(RECORD).tolist()
    coef, covs = np.array(coef, np.float64), np.array(covs, np.float64)
    k, Q, P = coef.shape
    _, trans = R.m_step(np.array(rec[:88]), np.zeros(k), trans, k)
    for s in range(k):
        occ = rec[64 + s]
        tri = rec[216 + FR.TRI * s:216 + FR.TRI * (s + 1)]
        syy = [[tri[i * (i + 1) // 2 + j] for j in range(i + 1)] for i in range(Q + P)]
        if not (occ > 0.0 and math.isfinite(occ)) or not all(math.isfinite(v) for r in syy for v in r):
            continue
        A = [[syy[Q + i][Q + j] for j in range(i + 1)] for i in range(P)]
        beta = [RR.solve(A, [syy[Q + i][q] for i in range(P)]) for q in range(Q)]
        if any(b is None for b in beta):
            continue
        c = [[0.0] * Q for _ in range(Q)]
        for q in range(Q):
            for r in range(q + 1):
                v = syy[q][r] / occ
                for i in range(P):
                    v = v - beta[q][i] * (syy[Q + i][r] / occ)
                c[q][r] = v
            c[q][q] = c[q][q] if c[q][q] >= floor * floor else floor * floor
        if FR.factor(c) is None:
            continue
        coef[s] = beta
        for q in range(Q):
            for r in range(q + 1):
                covs[s, q, r] = covs[s, r, q] = c[q][r]
    return coef, covs, trans


def exact_em(obs, coef, covs, trans, iterations, floor):
    """The exact-run EM of one problem, every link a restatement: rows, exact_ref's run, the 88 doubles on coordinate 0, full_ref's
    sums, m_step.  Returns the tables' histories, the log-evidences and the smallest occupancy seen."""
    coef, covs, trans = np.array(coef, np.float64), np.array(covs, np.float64), np.array(trans, np.float64)
    k, Q, P = coef.shape
    hist, ev, low = [(coef, covs, trans)], [], math.inf
    for _ in range(iterations):
        Pm = R2.transition_masses(trans)
        m, logz, dead = X.run(rows(obs, coef, covs)[:, :k].tolist(), Pm)
        assert dead == -1
        mr = [[int(v) for v in row[:k]] for row in m]
        rec = np.concatenate([SS.record(SS.stats(mr, Pm, obs[:, 0])), FR.sums(m, Pm, obs, Q + P)])
        low = min(low, rec[64:64 + k].min())
        coef, covs, trans = m_step(rec, coef, covs, trans, floor)
        hist.append((coef, covs, trans))
        ev.append(logz)
    return [np.array(h) for h in zip(*hist)], np.array(ev), low
