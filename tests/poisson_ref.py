"""csrc/batch_poisson.hpp restated in plain Python: the log-factorials, the count a double is, the Poisson rows, the check and the
M-step.  Every operation is one IEEE float64 operation on Python floats (or numpy elementwise) or a table look-up; the one logarithm is
scale_ref.table_log, no library logarithm and no lgamma is taken."""
import math

import numpy as np

import retable_ref as R
import scale_ref as S

BAD_RATE = 16
MAX_COUNT = 4095


def log_fact_table():
    """lf[c] = log(c!), c = 0 .. MAX_COUNT: lf[0] = lf[1] = 0.0, then one addition a count, ascending."""
    lf = [0.0, 0.0]
    for i in range(2, MAX_COUNT + 1):
        lf.append(lf[i - 1] + S.table_log(float(i)))
    return lf


LF = log_fact_table()
LF_ARRAY = np.array(LF)


def count(y):
    """The integer 0 .. MAX_COUNT that y is, or -1."""
    y = float(y)
    if not (y >= 0.0) or not (y <= float(MAX_COUNT)):
        return -1
    c = int(y)
    return c if float(c) == y else -1


def entry(y, rate, log_rate):
    c = count(y)
    if c < 0:
        return -math.inf
    r = float(y) * float(log_rate)
    r = r - float(rate)
    r = r - LF[c]
    return r


def bad(rate):
    rate = float(rate)
    return not (rate > 0.0) or not (rate < math.inf) or not (rate >= S.MIN_NORMAL)


def rows(y, rates, k):
    """[T, 8]: entry s < k is y log_rate[s] - rate[s] - lf[y]; -inf for s >= k and for a y that is no count."""
    y = np.asarray(y, np.float64).reshape(-1)
    out = np.full((y.size, 8), -np.inf)
    for s in range(k):
        lr = S.table_log(rates[s])
        out[:, s] = [entry(v, rates[s], lr) for v in y]
    return out


def check(rates, trans, k):
    bits = R.check(np.zeros(k), trans, k)                  # (the transition rows' two bits: a rate is no mean)
    for s in range(k):
        if bad(rates[s]):
            bits |= BAD_RATE
    return bits


def m_step(rec, rates, log_rates, trans, k, floor):
    """One problem's Poisson M-step on its record [88]: new (rates [k], log_rates [k], trans [k, k]).  The logarithm of a rate the
    check refuses is NaN."""
    rec = np.asarray(rec, np.float64).reshape(R.RECORD)
    rates, trans = R.m_step(rec, rates, trans, k)
    log_rates = np.array(log_rates, np.float64).reshape(k)
    for s in range(k):
        if float(rec[64 + s]) > 0.0:
            r = float(rates[s]) if float(rates[s]) >= float(floor) else float(floor)
            rates[s] = r
            log_rates[s] = math.nan if bad(r) else S.table_log(r)
    return rates, log_rates, trans
