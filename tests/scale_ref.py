"""csrc/batch_scale.hpp restated in plain Python: the table logarithm, the scaled rows, the scaled check and the scaled M-step.  Every
operation is one IEEE float64 operation on Python floats (or numpy elementwise), a bit operation, or math.sqrt (correctly rounded); no
library logarithm is taken.  ScaledLearner is tests/learn_ref.py's Learner with the scaled rows, M-step and check: one problem of a scaled
learning stream (csrc/batch_learn.hpp)."""
import math
import struct

import numpy as np

import learn_ref as G
import retable_ref as R

BAD_SCALE = 8
TWO_PI = 2 * 3.14159265358979323846
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
LN2_HI = float.fromhex("0x1.62e42feep-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
MIN_NORMAL = float.fromhex("0x1p-1022")
# the doubles of 1 / (2 i + 1), i = 11 .. 1
COEF = [float.fromhex(h) for h in ("0x1.642c8590b2164p-5", "0x1.8618618618618p-5", "0x1.af286bca1af28p-5", "0x1.e1e1e1e1e1e1ep-5", "0x1.1111111111111p-4",
                                   "0x1.3b13b13b13b14p-4", "0x1.745d1745d1746p-4", "0x1.c71c71c71c71cp-4", "0x1.2492492492492p-3", "0x1.999999999999ap-3",
                                   "0x1.5555555555555p-2")]


def table_log(x):
    """log(x) for a normal positive finite x."""
    u = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    e = ((u >> 52) & 0x7FF) - 1023
    m = struct.unpack("<d", struct.pack("<Q", (u & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000))[0]
    if m >= SQRT2:
        m = m * 0.5
        e = e + 1
    f = (m - 1.0) / (m + 1.0)
    s = f * f
    p = COEF[0]
    for c in COEF[1:]:
        p = p * s
        p = p + c
    q = s * p
    q = 1.0 + q
    r = (f + f) * q
    ed = float(e)
    lo = ed * LN2_LO
    lo = lo + r
    hi = ed * LN2_HI
    return hi + lo


def norm_arg(sigma):
    a = TWO_PI * float(sigma)
    return a * float(sigma)


def bad(sigma):
    sigma = float(sigma)
    a = norm_arg(sigma)
    return not (sigma > 0.0) or not (sigma < math.inf) or not (a >= MIN_NORMAL) or not (a < math.inf)


def log_norm(sigma):
    return table_log(norm_arg(sigma))


def rows(y, means, sigmas, k):
    """[T, 8]: entry s < k is ((y - mean[s]) / sigma[s])^2 + log_norm[s], times -0.5; -inf for s >= k and for an infinite y."""
    y = np.asarray(y, np.float64).reshape(-1)
    out = np.full((y.size, 8), -np.inf)
    for s in range(k):
        with np.errstate(all="ignore"):                     # (an overflowing square is an infinite entry on the device too)
            r = (y - np.float64(means[s])) / np.float64(sigmas[s])
            r = r * r
            r = r + np.float64(log_norm(sigmas[s]))
            r = r * np.float64(-0.5)
        out[:, s] = np.where(np.isinf(y), -np.inf, r)
    return out


def check(means, sigmas, trans, k):
    bits = R.check(means, trans, k)
    for s in range(k):
        if bad(sigmas[s]):
            bits |= BAD_SCALE
    return bits


def sigma_step(occ, occ_yy, mean, floor):
    """The scale of a state with mass occ > 0 and new mean `mean`."""
    v = float(occ_yy) / float(occ)
    v = v - float(mean) * float(mean)
    if v >= float(floor) * float(floor):
        return math.sqrt(v)
    return float(floor)


def m_step(rec, means, sigmas, log_norms, trans, k, floor):
    """One problem's scaled M-step on its record [88]: new (means [k], sigmas [k], log_norms [k], trans [k, k]).  The log_norm of a
    sigma the check refuses is NaN."""
    rec = np.asarray(rec, np.float64).reshape(R.RECORD)
    means, trans = R.m_step(rec, means, trans, k)
    sigmas = np.array(sigmas, np.float64).reshape(k)
    log_norms = np.array(log_norms, np.float64).reshape(k)
    for s in range(k):
        occ = float(rec[64 + s])
        if occ > 0.0:
            sigmas[s] = sigma_step(occ, rec[80 + s], means[s], floor)
            log_norms[s] = math.nan if bad(sigmas[s]) else log_norm(sigmas[s])
    return means, sigmas, log_norms, trans


class ScaledLearner(G.Learner):
    """learn_ref.Learner with the scaled rows, M-step and check: floor None keeps the sigmas (a plain cpprob_hip_batch_learn_begin on a
    scaled batch).  State beside the Learner's: sigmas [k], log_norms [k]."""

    def __init__(self, means, trans, sigmas, k, gamma, t_min, floor):
        super().__init__(means, trans, k, gamma, t_min, None)
        self.sigmas = np.array(sigmas, np.float64).reshape(k)
        self.log_norms = np.array([log_norm(s) for s in self.sigmas])
        self.floor = floor

    def rows(self, y_new):
        return rows(y_new, self.means, self.sigmas, self.k)

    def advance(self, m_new, y_new):
        P = G.masses_of_words(self.thr, self.k)
        for row, y in zip(m_new, y_new):
            t = self.done
            self.tau, fb = G.push(self.tau, self.last, P, y, self.gamma[t], t == 0, self.F)
            self.fallbacks += fb
            self.last = [int(v) for v in row]
            self.done = t + 1
        self.record = G.read(self.tau, self.last, self.F)
        if len(m_new) == 0 or self.t_min is None or self.done < self.t_min:
            return
        rec = G.record_array(self.record)
        if self.floor is None:
            means, trans = R.m_step(rec, self.means, self.trans, self.k)
            sigmas, log_norms = self.sigmas, self.log_norms
        else:
            means, sigmas, log_norms, trans = m_step(rec, self.means, self.sigmas, self.log_norms, self.trans, self.k, self.floor)
        self.status = check(means, sigmas, trans, self.k)
        if self.status == 0:
            self.changed += 1
            self.means, self.trans, self.sigmas, self.log_norms = means, trans, sigmas, log_norms
            self.thr = R.thresholds(trans, self.k)
