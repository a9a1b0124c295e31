"""csrc/batch_gibbs.hpp restated in plain Python: the polar normal, the Marsaglia-Tsang gamma and the conjugate draw of one problem's
table.  Every operation is one IEEE float64 operation on Python floats (which never contract), math.sqrt (correctly rounded) or
scale_ref.table_log; the words are the oracle's Philox blocks (oracle.draw_block, orc_u01_53).  The reference of
tests/test_gibbs_ref_host.py and tests/test_gpu_batch_draw_tables.py."""
import math

import numpy as np

import retable_ref as R
import scale_ref as S
from oracle import oracle as O

DRAW_BASE = 1 << 44
NO_DRAW = 32
MEAN_SLOT, VAR_SLOT = 64, 72


def _base(sweep):
    return DRAW_BASE + (int(sweep) << 24)


def _u01(lo, hi):
    return float(O.lib().orc_u01_53(int(lo), int(hi)))


def normal_attempt(r):
    """One polar attempt on a block's four words: z, or None where it is refused."""
    v1 = 2.0 * _u01(r[0], r[1])
    v1 = v1 - 1.0
    v2 = 2.0 * _u01(r[2], r[3])
    v2 = v2 - 1.0
    s = v1 * v1
    t = v2 * v2
    s = s + t
    if s >= 1.0 or s == 0.0:
        return None
    q = -2.0 * S.table_log(s)
    q = q / s
    return v1 * math.sqrt(q)


def gamma_attempt(d, c, z, u):
    """One Marsaglia-Tsang attempt on an accepted z and a uniform u: the variate, or None."""
    v = c * z
    v = 1.0 + v
    if not (v > 0.0):
        return None
    v3 = v * v
    v3 = v3 * v
    if u == 0.0 or v3 < S.MIN_NORMAL:
        return None
    r = 0.5 * z
    r = r * z
    r = r + d
    r = r - d * v3
    r = r + d * S.table_log(v3)
    if not (S.table_log(u) < r):
        return None
    return d * v3


def normal(seed, slot, sweep, max_attempts=64, log=None):
    """The standard normal of a slot: (z, drawn).  log, a list, takes True / False per polar attempt (accepted or refused)."""
    for a in range(max_attempts):
        z = normal_attempt(O.draw_block(int(seed), int(slot), _base(sweep) + 2 * a))
        if log is not None:
            log.append(z is not None)
        if z is not None:
            return z, True
    return 0.0, False


def gamma(shape, seed, slot, sweep, max_attempts=64, log=None):
    """Gamma(shape, 1), shape >= 1: (g, drawn).  log takes (polar accepted, attempt accepted) per attempt."""
    d = float(shape) - 1.0 / 3.0
    c = 9.0 * d
    c = math.sqrt(c)
    c = 1.0 / c
    for a in range(max_attempts):
        z = normal_attempt(O.draw_block(int(seed), int(slot), _base(sweep) + 2 * a))
        g = None
        if z is not None:
            ru = O.draw_block(int(seed), int(slot), _base(sweep) + 2 * a + 1)
            g = gamma_attempt(d, c, z, _u01(ru[0], ru[1]))
        if log is not None:
            log.append((z is not None, g is not None))
        if g is not None:
            return g, True
    return 0.0, False


def draw_table(rec, seed, sweep, means, trans, k, sigmas=None, alpha=1.0, mu0=0.0, tau0=10.0, a0=2.0, b0=1.0, max_attempts=64):
    """One problem's draw from its record [88]: (means [k], trans [k, k], sigmas [k] or None, status) -- the arrays handed in, as
    copies, where status is not 0."""
    rec = [float(x) for x in np.asarray(rec, np.float64).reshape(R.RECORD)]
    old = (np.array(means, np.float64).reshape(k), np.array(trans, np.float64).reshape(k, k), None if sigmas is None else np.array(sigmas, np.float64).reshape(k))
    missing = False
    new_t = np.zeros((k, k))
    for s in range(k):
        G = []
        for j in range(k):
            g, drawn = gamma(alpha + rec[8 * s + j], seed, 8 * s + j, sweep, max_attempts)
            missing = missing or not drawn
            G.append(g)
        total = 0.0
        for j in range(k):
            total = total + G[j]
        for j in range(k):
            new_t[s, j] = G[j] / total if total != 0.0 or G[j] != 0.0 else math.nan
    new_m, new_s, bits = np.zeros(k), None if sigmas is None else np.zeros(k), 0
    t2 = float(tau0) * float(tau0)
    for c in range(k):
        occ, occ_y, occ_yy = rec[64 + c], rec[72 + c], rec[80 + c]
        z, drawn = normal(seed, MEAN_SLOT + c, sweep, max_attempts)
        missing = missing or not drawn
        var = 1.0 if sigmas is None else float(old[2][c]) * float(old[2][c])
        prec = occ if sigmas is None else occ / var
        prec = 1.0 / t2 + prec
        m = occ_y if sigmas is None else occ_y / var
        m = float(mu0) / t2 + m
        m = m / prec
        m = m + z / math.sqrt(prec)
        new_m[c] = m
        if sigmas is not None:
            g, drawn = gamma(float(a0) + occ / 2.0, seed, VAR_SLOT + c, sweep, max_attempts)
            missing = missing or not drawn
            r = 2.0 * m
            r = r * occ_y
            r = occ_yy - r
            q = m * m
            q = q * occ
            r = r + q
            r = r / 2.0
            r = float(b0) + r
            r = r / g if g != 0.0 else math.inf
            new_s[c] = math.sqrt(r) if r >= 0.0 else math.nan
            if S.bad(new_s[c]):
                bits |= S.BAD_SCALE
    status = NO_DRAW if missing else bits | R.check(new_m, new_t, k)
    if status:
        return old + (status,)
    return new_m, new_t, new_s, 0


def draw_tables(stats, seeds, sweep, means, trans, sigmas=None, **kw):
    """draw_table over the problems: stats [B, 88], seeds [B]; returns (means [B, k], trans [B, k, k], sigmas [B, k] or None, status
    int32 [B])."""
    B, k = np.asarray(means).shape
    out = [draw_table(stats[b], seeds[b], sweep, means[b], trans[b], k, None if sigmas is None else sigmas[b], **kw) for b in range(B)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), None if sigmas is None else np.array([o[2] for o in out]),
            np.array([o[3] for o in out], np.int32))
