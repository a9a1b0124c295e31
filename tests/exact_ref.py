"""The exact filter run of a batch (csrc/batch_exact.hpp) restated in plain Python integers and floats, one IEEE
double operation a statement: the reference of tests/test_exact_ref_host.py and tests/test_gpu_batch_exact.py.  The 32-bit weights are
the oracle's (oracle.fix_weights), the logarithm tests/scale_ref.py's table_log, the thresholds and rows tests/backward_ref.py's.  Beside
it the law it approximates: a scaled forward-backward in numpy float64 over any rows of log-likelihoods."""
import math

import numpy as np

import scale_ref as S
from oracle import oracle as O

SCALE = float(1 << 44)
LN2X32 = float.fromhex("0x1.62e42fefa39efp+4")


def run(ll, P):
    """One problem: ll[t][0..k) its rows, P[s][s'] its integer transition masses (backward_ref.transition_masses).  Returns (m [T][8]
    floats -- integers <= 2^44, states >= k zero --, log_z, dead)."""
    T, k = len(ll), len(P)
    m, log_z = [], 0.0
    prev = None
    for t in range(T):
        u = []
        for sn in range(k):
            if t == 0:
                u.append(1.0)
                continue
            acc = 0.0
            for s in range(k):
                a = prev[s] * float(P[s][sn])
                acc = acc + a
            u.append(acc)
        live = [float(ll[t][s]) for s in range(k) if u[s] > 0.0]
        M = max(live) if live else -math.inf
        if M == -math.inf:
            return m + [[0.0] * 8 for _ in range(T - t)], -math.inf, t
        q = O.fix_weights(np.array(ll[t][:k], np.float64), M)
        w = [u[s] * float(int(q[s])) for s in range(k)]
        W, U = 0.0, 0.0
        for s in range(k):
            W = W + w[s]
            U = U + u[s]
        row = []
        for s in range(k):
            r = w[s] / W
            r = r * SCALE
            row.append(float(round(r)))                     # (round half to even: rint)
        prev = row
        m.append(row + [0.0] * (8 - k))
        d = S.table_log(W) - S.table_log(U)
        d = M + d
        d = d - LN2X32
        log_z = log_z + d
    return m, log_z, -1


def float_forward_backward(ll, A):
    """The scaled forward-backward in float64 for rows ll [T][k], transition probabilities A [k][k] and a uniform initial state, every
    step normalised after its row's maximum is taken off: (filtering marginals [T, k], log-likelihood, smoothed marginals [T, k])."""
    ll = np.asarray(ll, np.float64)
    A = np.asarray(A, np.float64)
    T, k = ll.shape
    lik = np.exp(ll - ll.max(axis=1, keepdims=True))
    alpha, log_z = np.zeros((T, k)), 0.0
    pred = np.full(k, 1.0 / k)
    for t in range(T):
        a = pred * lik[t]
        log_z += float(np.log(a.sum()) + ll[t].max())
        alpha[t] = a / a.sum()
        pred = alpha[t] @ A
    beta = np.ones((T, k))
    for t in range(T - 2, -1, -1):
        b = A @ (lik[t + 1] * beta[t + 1])
        beta[t] = b / b.sum()
    gamma = alpha * beta
    return alpha, log_z, gamma / gamma.sum(axis=1, keepdims=True)
