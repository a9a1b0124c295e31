"""The running sufficient statistics of an online batch (csrc/batch_onlinestats.hpp, include/cpprob_hip.h:
cpprob_hip_batch_online_stats) restated in plain Python on tests/backward_ref.py's integers: the forward-only recursion on tau, its
read-out, and -- for the exact identity -- the backward walk of tests/suffstats_ref.py over a number type F.  F=float: every product,
sum and quotient one IEEE double operation in the kernel's order (Python floats never contract); F=Fraction: exact arithmetic.  The
reference of tests/test_onlinestats_ref_host.py, the kernel-text test and tests/test_gpu_batch_onlinestats.py."""
from fractions import Fraction

import numpy as np

RECORD = 88


class Running:
    """One problem's state: tau[8][88] and the steps consumed.  `fallbacks` counts the rows s' < k whose D was 0 (the defensive rule)
    and `zero_g` the read-outs' states s' < k with g = 0, so that a test can assert that those paths ran."""

    def __init__(self, F=float):
        self.F = F
        self.tau = [[F(0)] * RECORD for _ in range(8)]
        self.done = 0
        self.fallbacks = 0
        self.zero_g = 0

    def consume(self, m, P, obs=None):
        """Steps [done, len(m)) of the m table m[t][s] (integers, k a row) with transition integers P[s][s'] and observes obs[t]
        (indexed by the absolute step; None: every y is 0.0)."""
        F, k = self.F, len(P)
        for t in range(self.done, len(m)):
            y = F(0) if obs is None else F(float(obs[t]))
            new = [[F(0)] * RECORD for _ in range(8)]
            if t >= 1:
                row = m[t - 1]
                Dm = F(0)
                for s in range(k):
                    Dm = Dm + F(row[s])
                for sn in range(k):
                    a = [F(row[s]) * F(P[s][sn]) for s in range(k)]
                    D = F(0)
                    for s in range(k):
                        D = D + a[s]
                    if D == 0:
                        self.fallbacks += 1
                        w = [F(row[s]) / Dm for s in range(k)]
                    else:
                        w = [a[s] / D for s in range(k)]
                    for j in range(RECORD):
                        acc = F(0)
                        for s in range(k):
                            v = self.tau[s][j]
                            if j == 8 * s + sn:
                                v = v + F(1)
                            acc = acc + w[s] * v
                        new[sn][j] = acc
            for sn in range(k):
                new[sn][64 + sn] = new[sn][64 + sn] + F(1)
                new[sn][72 + sn] = new[sn][72 + sn] + y
                new[sn][80 + sn] = new[sn][80 + sn] + y * y
            self.tau = new
        self.done = max(self.done, len(m))

    def read(self, m):
        """The record at the length len(m) = done: 88 numbers of type F."""
        F = self.F
        assert len(m) == self.done
        if not m:
            return [F(0)] * RECORD
        k = len(m[-1])
        tot = sum(int(v) for v in m[-1])
        g = [F(m[-1][s]) / F(tot) for s in range(k)]
        self.zero_g += sum(1 for v in g if v == 0)
        out = []
        for j in range(RECORD):
            acc = F(0)
            for sn in range(k):
                acc = acc + g[sn] * self.tau[sn][j]
            out.append(acc)
        return out


def record(m, P, obs=None, cuts=(), F=float):
    """The record of one problem consumed in the pieces that end at `cuts` (lengths, ascending) and at len(m)."""
    run = Running(F)
    for L in list(cuts) + [len(m)]:
        run.consume(m[:L], P, obs)
    return run.read(m)


def as_array(rec):
    return np.array([float(v) for v in rec])


def int_masses(mass_rows, k):
    """Rows of the m table as the device holds them (float64 [T, 8], integers below 2^45) as backward_ref's lists of k integers."""
    return [[int(v) for v in row[:k]] for row in np.asarray(mass_rows)]


def backward_record(m, P, obs=None, F=Fraction):
    """tests/suffstats_ref.py's stats() -- the backward walk of csrc/batch_suffstats.hpp -- over the number type F, as a record of 88.
    F=float gives stats()' own bits (tests/test_onlinestats_ref_host.py asserts it)."""
    T, k = len(m), len(P)
    xi = [[F(0)] * 8 for _ in range(8)]
    occ, occ_y, occ_yy = [F(0)] * 8, [F(0)] * 8, [F(0)] * 8
    g = None
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            tot = sum(int(v) for v in m[t])
            g = [F(m[t][s]) / F(tot) for s in range(k)]
        else:
            term = [[F(0)] * k for _ in range(k)]                 # term[sn][s]
            for sn in range(k):
                w = [F(m[t][s]) * F(P[s][sn]) for s in range(k)]
                D = F(0)
                for s in range(k):
                    D = D + w[s]
                if D == 0:
                    w = [F(m[t][s]) for s in range(k)]
                    for s in range(k):
                        D = D + w[s]
                if g[sn] == 0:
                    continue
                for s in range(k):
                    term[sn][s] = (w[s] / D) * g[sn]
            g = []
            for s in range(k):
                acc = F(0)
                for sn in range(k):
                    xi[s][sn] = xi[s][sn] + term[sn][s]
                    acc = acc + term[sn][s]
                g.append(acc)
        y = F(0) if obs is None else F(float(obs[t]))
        for s in range(k):
            occ[s] = occ[s] + g[s]
            occ_y[s] = occ_y[s] + g[s] * y
            occ_yy[s] = occ_yy[s] + g[s] * (y * y)
    return [v for row in xi for v in row] + occ + occ_y + occ_yy
