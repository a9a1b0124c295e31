"""Decoding a batch (csrc/batch_decode.hpp) restated in plain Python floats on top of backward_ref.py: the
reference of tests/test_decode_ref_host.py, tests/test_batch_decode_kernel_text_host.py and tests/test_gpu_batch_decode*.py.  Every
sum below is one IEEE double addition and every comparison a comparison of doubles; the log table lp (and lp0) is PASSED IN -- the
library's own (cpprob_hip_batch_decode_logp) where a device run is restated, log_table() below elsewhere -- so that no result depends
on a second logarithm."""
import math

import numpy as np

import backward_ref as R  # noqa: F401  (the masses m and P every caller builds come from it)

NEG = -math.inf


def log_table(P, k=None):
    """(lp [k][k], lp0) of the integer masses P: lp[s][s'] = log(double(P[s][s']) * 2^-32), -inf where P = 0; lp0 = log(1.0 / double(k))."""
    k = len(P) if k is None else k
    lp = [[math.log(float(P[s][sn]) * 2.0 ** -32) if P[s][sn] else NEG for sn in range(k)] for s in range(k)]
    return lp, math.log(1.0 / float(k))


def _scan(vals):
    """(best, arg) of the strict scan in index order from (-inf, 0): ties go to the lowest index, all -inf keeps 0."""
    best, arg = NEG, 0
    for s, c in enumerate(vals):
        if c > best:
            best, arg = c, s
    return best, arg


def forward(m, ll, lp, lp0, v=None, start=0):
    """(words [L] uint32, v_{L-1} [k]) of masses m [L][k], table rows ll [L][>= k], the log table lp [k][k] and lp0.  start > 0: the
    walk resumes at step `start` from v = v_{start-1}; the words before it are returned as zeros."""
    L = len(m)
    k = len(lp)
    words = np.zeros(L, np.uint32)
    v = [NEG] * k if v is None else [float(x) for x in v[:k]]
    for t in range(start, L):
        new, w = [NEG] * k, 0
        for sn in range(k):
            if t == 0:
                best, arg = lp0, 0
            else:
                best, arg = _scan([v[s] + lp[s][sn] for s in range(k)])
            w |= arg << (3 * sn)
            new[sn] = best + float(ll[t][sn]) if m[t][sn] > 0 else NEG
        v = new
        words[t] = w | (_scan(v)[1] << 24)
    return words, v


def trace(words, e, lo=0):
    """The states at steps lo .. e of the traceback started at end_e: [e - lo + 1] int32."""
    out = np.zeros(e - lo + 1, np.int32)
    x = int(words[e]) >> 24
    for t in range(e, lo - 1, -1):
        out[t - lo] = x
        x = (int(words[t]) >> (3 * x)) & 7
    return out


def decode(m, ll, lp, lp0):
    """(path [L] int32, score) of the full decode; a problem of length 0: (empty, 0.0)."""
    L = len(m)
    if L == 0:
        return np.zeros(0, np.int32), 0.0
    words, v = forward(m, ll, lp, lp0)
    path = trace(words, L - 1)
    return path, v[int(path[L - 1])]


def decode_lag(words, lag, frm=0, n_rows=None):
    """Fixed-lag rows [n_rows] int32 of the words of L steps: row r is X_{frm + r}, the state at t = frm + r of the traceback started at
    end_{min(t + lag, L - 1)}; -1 past the length."""
    L = len(words)
    n_rows = max(L - frm, 0) if n_rows is None else n_rows
    out = np.full(n_rows, -1, np.int32)
    for t in range(frm, min(L, frm + n_rows)):
        e = min(t + lag, L - 1)
        out[t - frm] = trace(words, e, t)[0]
    return out


def decode_lag_fast(words, lag, frm=0, n_rows=None):
    """decode_lag(), the tracebacks of all rows walked side by side: the same shifts of the same words (a long problem's rows at a
    lag of hundreds are millions of steps of the plain walk)."""
    w = np.asarray(words, np.int64)
    L = len(w)
    n_rows = max(L - frm, 0) if n_rows is None else n_rows
    out = np.full(n_rows, -1, np.int32)
    t = np.arange(frm, min(L, frm + n_rows), dtype=np.int64)
    if t.size == 0:
        return out
    e = np.minimum(t + lag, L - 1)
    x = w[e] >> 24
    for d in range(int((e - t).max())):                            # step d of a walk: from e - d to e - d - 1, while that is >= t
        live = e - d > t
        at = np.where(live, e - d, 0)
        x = np.where(live, (w[at] >> (3 * x)) & 7, x)
    out[:t.size] = x
    return out
