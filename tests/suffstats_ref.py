"""The expected sufficient statistics of a batch (csrc/batch_suffstats.hpp, include/cpprob_hip.h: cpprob_hip_batch_smooth_stats)
restated in plain Python on tests/backward_ref.py's integers and floats -- every product and sum one IEEE double operation, in the
kernel's order -- and the exact quantities they estimate: a floating-point forward-backward for a general table with a uniform initial
state, and the Baum-Welch step built on it.  The reference of tests/test_suffstats_ref_host.py, the kernel-text test and
tests/test_gpu_batch_suffstats.py."""
import numpy as np

import backward_ref as R
from oracle import exact
from oracle import oracle as O

RECORD = 88


def stats(m, P, obs=None):
    """The statistics of one problem from its masses m[t][s] (T rows, possibly none), its transition integers P[s][s'] and its
    observes: a dict of xi [8, 8] (xi[s][s'], expected transitions s -> s'), occ, occ_y, occ_yy [8]; states >= k stay zero."""
    T, k = len(m), len(P)
    xi = [[0.0] * 8 for _ in range(8)]
    occ, occ_y, occ_yy = [0.0] * 8, [0.0] * 8, [0.0] * 8
    g = None
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            tot = sum(m[t])
            g = [float(m[t][s]) / float(tot) for s in range(k)]
        else:
            rows = [R._weights(m[t], P, sn) for sn in range(k)]
            term = [[0.0] * k for _ in range(k)]                  # term[sn][s]
            for sn in range(k):
                if g[sn] == 0.0:
                    continue
                w, D = rows[sn]
                for s in range(k):
                    term[sn][s] = (w[s] / D) * g[sn]
            for s in range(k):
                for sn in range(k):
                    xi[s][sn] = xi[s][sn] + term[sn][s]
            g_new = []
            for s in range(k):
                acc = 0.0
                for sn in range(k):
                    acc = acc + term[sn][s]
                g_new.append(acc)
            g = g_new
        y = 0.0 if obs is None else float(obs[t])
        for s in range(k):
            occ[s] = occ[s] + g[s]
            occ_y[s] = occ_y[s] + g[s] * y
            occ_yy[s] = occ_yy[s] + g[s] * (y * y)
    return {"xi": np.array(xi), "occ": np.array(occ), "occ_y": np.array(occ_y), "occ_yy": np.array(occ_yy)}


def record(st):
    """The 88 doubles of a problem: xi at 8 s + s', then occ, occ_y, occ_yy."""
    return np.concatenate([st["xi"].reshape(-1), st["occ"], st["occ_y"], st["occ_yy"]])


def last_marginal(m):
    """g_{T-1}, the recursion's start."""
    tot = sum(m[-1])
    return np.array([float(v) / float(tot) for v in m[-1]])


def exact_stats(obs, means, trans):
    """Forward-backward in floating point for emission N(means[s], 1), transition weights trans (rows normalised here) and a uniform
    initial state: (xi [k, k], occ [k], occ_y [k], occ_yy [k], log-likelihood)."""
    obs = np.asarray(obs, np.float64)
    means = np.asarray(means, np.float64)
    A = np.asarray(trans, np.float64)
    A = A / A.sum(axis=1, keepdims=True)
    T, k = len(obs), len(means)
    lik = np.exp(exact.normal_logpdf(obs[:, None], means[None, :], 1.0))
    alpha, c = np.zeros((T, k)), np.zeros(T)
    a = np.full(k, 1.0 / k) * lik[0]
    c[0] = a.sum()
    alpha[0] = a / c[0]
    for t in range(1, T):
        a = (alpha[t - 1] @ A) * lik[t]
        c[t] = a.sum()
        alpha[t] = a / c[t]
    beta = np.ones((T, k))
    for t in range(T - 2, -1, -1):
        beta[t] = (A @ (lik[t + 1] * beta[t + 1])) / c[t + 1]
    gamma = alpha * beta
    gamma /= gamma.sum(axis=1, keepdims=True)
    xi = np.zeros((k, k))
    for t in range(T - 1):
        x = alpha[t][:, None] * A * (lik[t + 1] * beta[t + 1])[None, :] / c[t + 1]
        xi += x / x.sum()
    return xi, gamma.sum(axis=0), gamma.T @ obs, gamma.T @ (obs * obs), float(np.log(c).sum())


def exact_em(obs, means0, trans0, iterations):
    """Baum-Welch on the means and the transition rows (sigma fixed at 1, uniform initial state): the tables after every iteration,
    (means [iterations + 1, k], trans [iterations + 1, k, k])."""
    means, trans = np.array(means0, np.float64), np.array(trans0, np.float64)
    trans = trans / trans.sum(axis=1, keepdims=True)
    ms, ts = [means.copy()], [trans.copy()]
    for _ in range(iterations):
        xi, occ, occ_y, _, _ = exact_stats(obs, means, trans)
        trans = xi / xi.sum(axis=1, keepdims=True)
        means = occ_y / occ
        ms.append(means.copy())
        ts.append(trans.copy())
    return np.array(ms), np.array(ts)


def lineage_pair_counts(hist, anc, logw, k):
    """The expected transition counts the surviving lineages give: the final particles' normalised weights on the pairs
    (x_t, x_{t+1}) of their ancestral paths, summed over t.  [k, k]."""
    path = O.lineage(np.ascontiguousarray(anc))
    col = np.take_along_axis(hist, path, axis=1)
    w = np.exp(logw - np.max(logw))
    w = w / w.sum()
    out = np.zeros((k, k))
    for t in range(hist.shape[0] - 1):
        np.add.at(out, (col[t], col[t + 1]), w)
    return out
