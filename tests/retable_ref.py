"""csrc/batch_retable.hpp restated in plain Python / numpy: what a re-table writes from a table and the observes, and the M-step.
Every operation is one IEEE float64 operation (numpy elementwise, Python floats) or math.ceil; no logarithm is taken here -- log_norm,
log(2 pi) as the host evaluates it, is an argument."""
import math

import numpy as np

BAD_WEIGHT, NO_MASS, BAD_MEAN = 1, 2, 4
ROWS_PER_TRIP = 32                      # kRetableRows = kThreads / 8
GRID_MAX = 64                           # kRetableGridMax
GROUPS = 4096                           # kRetableGroups
RECORD = 88


def grid_y(T_max, B):
    """gridDim.y of the launch: the trips of the longest problem, capped by GRID_MAX and by GROUPS // B."""
    cap = max(1, min(GRID_MAX, GROUPS // max(1, int(B))))
    return max(1, min(cap, (int(T_max) + ROWS_PER_TRIP - 1) // ROWS_PER_TRIP))


def rows(y, means, k, log_norm):
    """[T, 8]: entry s < k is ((y - mean[s]) / 1.0)^2 + log_norm, times -0.5; -inf for s >= k and for an infinite y."""
    y = np.asarray(y, np.float64).reshape(-1)
    out = np.full((y.size, 8), -np.inf)
    for s in range(k):
        r = (y - np.float64(means[s])) / np.float64(1.0)
        r = r * r
        r = r + np.float64(log_norm)
        r = r * np.float64(-0.5)
        out[:, s] = np.where(np.isinf(y), -np.inf, r)
    return out


def thresholds(trans, k):
    """[64] uint64: word 8 s + j = ceil((acc / tot) 2^32) for s < k, j < k - 1; every other word ~0."""
    thr = np.full(64, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    tr = np.asarray(trans, np.float64).reshape(k, k)
    for s in range(k):
        tot = 0.0
        for j in range(k):
            tot = tot + float(tr[s, j])
        acc = 0.0
        for j in range(k - 1):
            acc = acc + float(tr[s, j])
            thr[8 * s + j] = np.uint64(math.ceil((acc / tot) * 4294967296.0))
    return thr


def check(means, trans, k):
    """The bit set of one problem's table."""
    tr = np.asarray(trans, np.float64).reshape(k, k)
    bits = 0
    for s in range(k):
        tot = 0.0
        for j in range(k):
            w = float(tr[s, j])
            if not (w >= 0.0) or not math.isfinite(w):
                bits |= BAD_WEIGHT
            tot = tot + w
        if not (tot > 0.0):
            bits |= NO_MASS
        if not math.isfinite(float(means[s])):
            bits |= BAD_MEAN
    return bits


def m_step(rec, means, trans, k):
    """One problem's M-step on its record [88]: new (means [k], trans [k, k])."""
    rec = np.asarray(rec, np.float64).reshape(RECORD)
    means = np.array(means, np.float64).reshape(k)
    trans = np.array(trans, np.float64).reshape(k, k)
    for s in range(k):
        row = 0.0
        for j in range(k):
            row = row + float(rec[8 * s + j])
        if row > 0.0:
            for j in range(k):
                trans[s, j] = float(rec[8 * s + j]) / row
        occ = float(rec[64 + s])
        if occ > 0.0:
            means[s] = float(rec[72 + s]) / occ
    return means, trans
