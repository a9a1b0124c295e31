"""Online EM of an online batch (csrc/batch_learn.hpp, include/cpprob_hip.h: cpprob_hip_batch_advance_learn) restated in plain Python
on tests/backward_ref.py's integers.  Nothing here is new but the discounted push: the weights are tests/onlinestats_ref.py's, the
read-out is its read-out, and the M-step, the check, the threshold words and the rows are tests/retable_ref.py's.  Over a number type
F as onlinestats_ref.Running: F=float, every product, sum and quotient one IEEE double operation in the kernel's order; F=Fraction,
exact arithmetic (with gamma[t] = 1 / (t + 1) and no M-step, L times the record is onlinestats_ref's record)."""
import numpy as np

import retable_ref as R

RECORD = 88
TWO32 = 1 << 32
ONES = 0xFFFFFFFFFFFFFFFF


def masses_of_words(thr, k):
    """P[s][s'] of a problem's 64 threshold words (smooth_trans_mass): integers."""
    thr = [int(v) for v in np.asarray(thr).reshape(64)]
    P = []
    for s in range(k):
        c = [0] + thr[8 * s:8 * s + k - 1] + [TWO32]
        P.append([c[j + 1] - c[j] for j in range(k)])
    return P


def push(tau, row, P, y, g, first, F=float):
    """One discounted step: tau [8][88] of type F, row = m_{t-1} (k integers; unused where first), P the transition integers, y the
    observe, g = gamma[t].  Returns (the new tau, the rows s' < k whose D was 0)."""
    k = len(P)
    y, g = F(float(y)) if not isinstance(y, F) else y, F(g)
    om = F(1) - g
    new = [[F(0)] * RECORD for _ in range(8)]
    fallbacks = 0
    if not first:
        Dm = F(0)
        for s in range(k):
            Dm = Dm + F(row[s])
        for sn in range(k):
            a = [F(row[s]) * F(P[s][sn]) for s in range(k)]
            D = F(0)
            for s in range(k):
                D = D + a[s]
            if D == 0:
                fallbacks += 1
                w = [F(row[s]) / Dm for s in range(k)]
            else:
                w = [a[s] / D for s in range(k)]
            for j in range(RECORD):
                acc = F(0)
                for s in range(k):
                    v = om * tau[s][j]
                    if j == 8 * s + sn:
                        v = v + g
                    acc = acc + w[s] * v
                new[sn][j] = acc
    for sn in range(k):
        new[sn][64 + sn] = new[sn][64 + sn] + g
        new[sn][72 + sn] = new[sn][72 + sn] + g * y
        new[sn][80 + sn] = new[sn][80 + sn] + g * (y * y)
    return new, fallbacks


def read(tau, last, F=float):
    """The record at the length reached: last = m_{L-1} (k integers), or None at length 0."""
    if last is None:
        return [F(0)] * RECORD
    k = len(last)
    tot = sum(int(v) for v in last)
    gm = [F(last[s]) / F(tot) for s in range(k)]
    out = []
    for j in range(RECORD):
        acc = F(0)
        for sn in range(k):
            acc = acc + gm[sn] * tau[sn][j]
        out.append(acc)
    return out


class Learner:
    """One problem of a learning stream.  gamma: the step sizes, indexed by the absolute step; t_min: the burn-in (None: no M-step
    ever).  State: means [k], trans [k, k], thr [64] uint64, tau [8][88], record [88], status, done; `changed` counts the M-steps
    that replaced the table, `fallbacks` the rows whose D was 0."""

    def __init__(self, means, trans, k, gamma, t_min, log_norm, F=float):
        self.k, self.F, self.gamma, self.t_min, self.log_norm = k, F, gamma, t_min, log_norm
        self.means = np.array(means, np.float64).reshape(k)
        self.trans = np.array(trans, np.float64).reshape(k, k)
        self.thr = R.thresholds(self.trans, k)
        self.tau = [[F(0)] * RECORD for _ in range(8)]
        self.record = [F(0)] * RECORD
        self.last, self.done, self.status, self.changed, self.fallbacks = None, 0, 0, 0, 0

    def rows(self, y_new):
        """[dT, 8]: the rows of the new steps under the table in force."""
        return R.rows(y_new, self.means, self.k, self.log_norm)

    def advance(self, m_new, y_new):
        """The m-table rows (k integers each) and the observes of the steps [done, done + len(m_new)): the push under the words in
        force, the record, and -- where a step was taken and the length has reached t_min -- the M-step, its check and the words."""
        P = masses_of_words(self.thr, self.k)
        for row, y in zip(m_new, y_new):
            t = self.done
            self.tau, fb = push(self.tau, self.last, P, y, self.gamma[t], t == 0, self.F)
            self.fallbacks += fb
            self.last = [int(v) for v in row]
            self.done = t + 1
        self.record = read(self.tau, self.last, self.F)
        if len(m_new) == 0 or self.t_min is None or self.done < self.t_min:
            return
        means, trans = R.m_step(record_array(self.record), self.means, self.trans, self.k)
        self.status = R.check(means, trans, self.k)
        if self.status == 0:
            self.changed += 0 if (np.array_equal(means, self.means) and np.array_equal(trans, self.trans)) else 1
            self.means, self.trans = means, trans
            self.thr = R.thresholds(trans, self.k)


def record_array(rec):
    return np.array([float(v) for v in rec])


def tau_array(tau):
    return np.array([[float(v) for v in row] for row in tau]).reshape(-1)
