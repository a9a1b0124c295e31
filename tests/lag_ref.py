"""Fixed-lag smoothing of a batch (include/cpprob_hip.h: cpprob_hip_batch_smooth_lag; csrc/batch_smooth.hpp) restated in plain Python
floats on tests/backward_ref.py's integers: the reference of tests/test_batch_smooth_lag_host.py and tests/test_gpu_batch_smooth_lag.py.
G_t is the backward recursion started from the filtering masses of the end step e(t) = min(t + lag, T - 1); the windowed trajectories
are the last min(lag + 1, T) rows of the full backward simulation (the draws keep the absolute step)."""
import numpy as np

import backward_ref as R


def end_step(t, lag, T):
    return min(t + int(lag), T - 1)


def window(lag, T):
    """W = min(lag + 1, T): the steps whose end is T - 1."""
    return min(int(lag) + 1, T)


def _step(m_u, P, g):
    """g_u from g_{u+1}: the statements of backward_ref.marginals' loop body."""
    k = len(m_u)
    rows = [R._weights(m_u, P, sn) for sn in range(k)]
    out = [0.0] * k
    for s in range(k):
        acc = 0.0
        for sn in range(k):
            if g[sn] == 0.0:
                continue
            w, D = rows[sn]
            acc = acc + (w[s] / D) * g[sn]
        out[s] = acc
    return out


def _start(m_e):
    tot = sum(m_e)
    return [float(x) / float(tot) for x in m_e]


def fixed_lag_marginals(m, P, lag):
    """G[t][s], t = 0 .. T-1, by the definition: a final row (t + lag <= T - 1) is its own walk of lag steps from its end step; the
    rows whose end is T - 1 are the steps of the one walk from T - 1 (the same operations on the same doubles, taken once)."""
    T = len(m)
    if T == 0:
        return np.zeros((0, len(P)))
    G = [None] * T
    g = _start(m[T - 1])
    G[T - 1] = g
    for t in range(T - 2, max(T - 2 - int(lag), -1), -1):
        g = _step(m[t], P, g)
        G[t] = g
    for t in range(0, T - 1 - int(lag)):
        g = _start(m[end_step(t, lag, T)])
        for u in range(t + int(lag) - 1, t - 1, -1):
            g = _step(m[u], P, g)
        G[t] = g
    return np.array(G)


def window_trajectories(m, P, seed, n_traj, lag, draw_index=0):
    """[W][n_traj] int32: rows T - W .. T - 1 of the full backward simulation."""
    T = len(m)
    return R.trajectories_fast(m, P, seed, n_traj, draw_index)[T - window(lag, T):]
