"""csrc/batch_categorical.hpp restated in plain Python: the symbol a double is, the categorical rows, the check, the symbol counts of
the backward walk and the M-step.  Every operation is one IEEE float64 operation; the one logarithm is scale_ref.table_log."""
import math

import numpy as np

import backward_ref as R2
import retable_ref as R
import scale_ref as S

BAD_PROB = 32
MAX_SYMBOLS = 64
RECORD = 88 + 8 * MAX_SYMBOLS


def symbol(y, V):
    """The integer 0 .. V-1 that y is, or -1."""
    y = float(y)
    if not (y >= 0.0) or not (y < float(V)):
        return -1
    c = int(y)
    return c if float(c) == y else -1


def bad(p):
    p = float(p)
    return not (p > 0.0) or not (p < math.inf) or not (p >= S.MIN_NORMAL)


def log_matrix(E):
    """logE [k, V] = table_log of every entry."""
    E = np.asarray(E, np.float64)
    return np.array([[S.table_log(float(e)) for e in row] for row in E])


def rows(y, E):
    """[T, 8]: entry s < k is logE[s][symbol(y)]; -inf for s >= k and for a y that is no symbol."""
    (k, V), logE = np.shape(E), log_matrix(E)
    y = np.asarray(y, np.float64).reshape(-1)
    out = np.full((y.size, 8), -np.inf)
    for t, v in enumerate(y):
        c = symbol(v, V)
        if c >= 0:
            out[t, :k] = logE[:, c]
    return out


def check(E, trans):
    """The transition rows' two bits (retable_ref.check on means of 0) and bit 32."""
    E = np.asarray(E, np.float64)
    return R.check(np.zeros(E.shape[0]), trans, E.shape[0]) | (BAD_PROB if any(bad(e) for e in E.reshape(-1)) else 0)


def symbol_counts(m, P, obs, V):
    """cnt [8, 64] of one problem from its masses m[t][0..8), its transition integers P[s][s'] and its observes: g_t[s]
    (backward_ref.marginals, the walk's own operations) is added to cnt[s][symbol(y_t)], t = T-1 .. 0; an observe that is no symbol adds
    to no bin.  A last row of zeros (the exact run was dead) divides 0 by 0 on the device: every marginal of the walk is NaN."""
    T, k = len(m), len(P)
    rows = [[int(v) for v in row[:k]] for row in m]
    g = R2.marginals(rows, P) if sum(rows[-1]) else np.full((T, k), np.nan)
    cnt = np.zeros((8, MAX_SYMBOLS))
    for t in range(T - 1, -1, -1):
        c = symbol(obs[t], V)
        if c >= 0:
            cnt[:k, c] = cnt[:k, c] + g[t]
    return cnt


def m_step(rec, E, trans, floor):
    """One problem's categorical M-step on its record [600]: new (E [k, V], trans [k, k])."""
    rec = np.asarray(rec, np.float64).reshape(RECORD)
    E = np.array(E, np.float64)
    k, V = E.shape
    _, trans = R.m_step(rec[:88], np.zeros(k), trans, k)
    with np.errstate(all="ignore"):
        for s in range(k):
            cnt = rec[88 + 64 * s: 88 + 64 * s + V]
            tot = np.float64(0.0)
            for v in range(V):
                tot = tot + cnt[v]
            if tot > 0.0:
                for v in range(V):
                    p = cnt[v] / tot
                    E[s, v] = p if p >= floor else np.float64(floor)
    return E, trans
