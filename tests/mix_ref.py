"""csrc/batch_mix.hpp restated in plain Python: the table exponential, the log-weights, the mixture rows, the check, the responsibility
sums of the backward walk and the M-step.  Every operation is one IEEE float64 operation on Python floats; the diagonal entries are
diag_ref's, the logarithm scale_ref.table_log, no library exponential is taken."""
import math
import struct

import numpy as np

import backward_ref as R2
import diag_ref as DG
import retable_ref as R
import scale_ref as S

MAX_DIM, MAX_COMP, BLOCK = 16, 8, 33
RECORD = 88 + 64 * BLOCK
BAD_MIX_WEIGHT = 128
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
# the doubles of 1 / i!, i = 13 .. 1
COEF = [float.fromhex(h) for h in ("0x1.6124613a86d09p-33", "0x1.1eed8eff8d898p-29", "0x1.ae64567f544e4p-26", "0x1.27e4fb7789f5cp-22", "0x1.71de3a556c734p-19",
                                   "0x1.a01a01a01a01ap-16", "0x1.a01a01a01a01ap-13", "0x1.6c16c16c16c17p-10", "0x1.1111111111111p-7", "0x1.5555555555555p-5",
                                   "0x1.5555555555555p-3", "0x1p-1", "0x1p+0")]


def table_exp(x):
    """exp(x) for x in [-1000, 0]; exactly 0.0 where the result would be subnormal."""
    x = float(x)
    t = x * INV_LN2
    t = t - 0.5
    n = int(t)                                              # (towards zero)
    nd = float(n)
    r = x - nd * S.LN2_HI
    r = r - nd * S.LN2_LO
    p = COEF[0]
    for c in COEF[1:]:
        p = p * r
        p = p + c
    p = p * r
    p = 1.0 + p
    u = struct.unpack("<Q", struct.pack("<d", p))[0]
    e = ((u >> 52) & 0x7FF) + n
    if e < 1:
        return 0.0
    return struct.unpack("<d", struct.pack("<Q", (u & 0x000FFFFFFFFFFFFF) | (e << 52)))[0]


def totals(weights):
    """[k]: ((0.0 + w_0) + w_1) + ..."""
    out = []
    for row in np.asarray(weights, np.float64):
        tot = 0.0
        for w in row:
            tot = tot + float(w)
        out.append(tot)
    return out


def log_weights(weights):
    """[k, M]: table_log(w_c / tot), -inf for a weight of zero."""
    weights = np.asarray(weights, np.float64)
    return np.array([[S.table_log(float(w) / tot) if w > 0.0 else -math.inf for w in row] for row, tot in zip(weights, totals(weights))])


def join(lc):
    """(ll, e, S) of a state from its components' lc."""
    m = lc[0]
    for v in lc[1:]:
        if v > m:
            m = v
    if m == -math.inf:
        return -math.inf, [0.0] * len(lc), 0.0
    e = [0.0 if v == -math.inf else table_exp(v - m if v - m > -1000.0 else -1000.0) for v in lc]      # (fmax: a NaN takes -1000.0)
    tot = 0.0
    for v in e:
        tot = tot + v
    return m + S.table_log(tot), e, tot


def components(y, weights, means, sigmas):
    """lc [T, k, M]: lw[s][c] + diag_ref's entry of component c of state s."""
    means = np.asarray(means, np.float64)
    (k, M, D), lw = means.shape, log_weights(weights)
    y = np.asarray(y, np.float64).reshape(-1, D)
    with np.errstate(all="ignore"):
        return np.stack([lw[s][None, :] + DG.rows(y, means[s], np.asarray(sigmas, np.float64)[s])[:, :M] for s in range(k)], axis=1)


def rows(y, weights, means, sigmas):
    """[T, 8]: entry s < k is m + table_log(S); -inf for s >= k and where every component is -inf (an infinite y_d)."""
    lc = components(y, weights, means, sigmas)
    out = np.full((lc.shape[0], 8), -np.inf)
    for t in range(lc.shape[0]):
        for s in range(lc.shape[1]):
            out[t, s] = join(lc[t, s].tolist())[0]
    return out


def check(weights, means, sigmas, trans):
    """The transition rows' two bits, bit 4 for a mean that is not finite, bit 8 for a sigma scale_ref.bad refuses, bit 128 for a
    weight not finite or < 0, a total not > 0 and finite, or a positive share that is not a normal number."""
    weights, means = np.asarray(weights, np.float64), np.asarray(means, np.float64)
    bits = R.check(np.zeros(means.shape[0]), trans, means.shape[0])
    bits |= R.BAD_MEAN if not np.isfinite(means).all() else 0
    bits |= S.BAD_SCALE if any(S.bad(sg) for sg in np.asarray(sigmas, np.float64).reshape(-1)) else 0
    with np.errstate(all="ignore"):
        for row, tot in zip(weights, totals(weights)):
            bad = not (tot > 0.0 and tot < math.inf) or any(not (w >= 0.0 and w < math.inf) or (w > 0.0 and not w / tot >= S.MIN_NORMAL) for w in row)
            bits |= BAD_MIX_WEIGHT if bad else 0
    return bits


def sums(m, P, obs, weights, means, sigmas):
    """The tail [RECORD - 88] of one problem's record from its masses m[t][0..8), its transition integers P[s][s'], its observes [T, D]
    and the tables in force: the block of (s, c) at 33 (8 s + c) holds occ_c, sy[d] at 1 + d and syy[d] at 17 + d; v = g_t[s] (e_c / S)
    (backward_ref.marginals' g), v y_t[d] and v (y_t[d] y_t[d]) added t = T-1 .. 0 from 0.0.  A step with an infinite coordinate adds
    nothing, a state whose row is -inf has v = 0.  A last row of zeros (the exact run was dead) divides 0 by 0 on the device: every
    marginal of the walk is NaN."""
    T, (k, M, D) = len(m), np.asarray(means).shape
    y = np.asarray(obs, np.float64).reshape(T, D)
    lc = components(y, weights, means, sigmas)
    mr = [[int(v) for v in row[:k]] for row in m]
    g = np.asarray(R2.marginals(mr, P), np.float64).tolist() if sum(mr[-1]) else [[math.nan] * k] * T
    out = [0.0] * (RECORD - 88)
    for t in range(T - 1, -1, -1):
        yt = y[t].tolist()
        if any(math.isinf(v) for v in yt):
            continue
        for s in range(k):
            ll, e, tot = join(lc[t, s].tolist())
            for c in range(M):
                v = g[t][s] * (e[c] / tot) if ll != -math.inf else 0.0
                at = BLOCK * (8 * s + c)
                out[at] = out[at] + v
                for d in range(D):
                    out[at + 1 + d] = out[at + 1 + d] + v * yt[d]
                    out[at + 17 + d] = out[at + 17 + d] + v * (yt[d] * yt[d])
    return np.array(out)


def m_step(rec, weights, means, sigmas, trans, floor):
    """One problem's mixture M-step on its record [2200]: new (weights [k, M], means [k, M, D], sigmas [k, M, D], trans [k, k])."""
    rec = np.asarray(rec, np.float64).reshape(RECORD).tolist()
    weights, means, sigmas = np.array(weights, np.float64), np.array(means, np.float64), np.array(sigmas, np.float64)
    k, M, D = means.shape
    _, trans = R.m_step(np.array(rec[:88]), np.zeros(k), trans, k)
    for s in range(k):
        occ = 0.0
        for c in range(M):
            occ = occ + rec[88 + BLOCK * (8 * s + c)]
        if not occ > 0.0:
            continue
        for c in range(M):
            blk = rec[88 + BLOCK * (8 * s + c):][:BLOCK]
            if blk[0] > 0.0:
                weights[s, c] = blk[0] / occ
                for d in range(D):
                    means[s, c, d] = blk[1 + d] / blk[0]
                    sigmas[s, c, d] = S.sigma_step(blk[0], blk[17 + d], means[s, c, d], floor)
            else:
                weights[s, c] = 0.0
    return weights, means, sigmas, trans
