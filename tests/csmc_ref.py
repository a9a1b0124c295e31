"""The conditional SMC run of a batch (csrc/batch_csmc.hpp) restated in plain Python integers: the reference of
tests/test_csmc_ref_host.py, tests/test_batch_csmc_kernel_text_host.py and tests/test_gpu_batch_csmc.py.  The Philox blocks are the
oracle's (oracle.draw_block), the initial state its uniform_smallint (orc_smallint_from_bits), the integer weights its fix_weight
(oracle.fix_weights); the thresholds and the log-likelihood rows come from tests/backward_ref.py (thresholds, log_likelihoods).

Per problem (k states, n particles, reference path r_0 .. r_{T-1}):
  slot 0        x = r_t & 7, a value >= k taken as k - 1
  slot i >= 1   w = word i & 3 of draw_block(seed, i >> 2, t)
    t = 0       x = smallint_from_bits(w, 0, k - 1)
    t >= 1      C_s the inclusive sums of row t - 1's masses, S = C_{k-1}; W = (hi << 32) | lo, lo and hi words 2 (i & 1) and
                2 (i & 1) + 1 of draw_block(seed, i >> 1, 2^43 + t); V = (W S) >> 64; a = #{s < k-1 : V >= C_s};
                x = #{j < k-1 : w >= thr[a][j]}
  row t         m[s] = cnt_t[s] * fix_weight(ll_t[s], M_t), M_t the largest ll_t[s] over the states present (slot 0 counts)."""
import numpy as np

from oracle import oracle as O

DRAW_BASE = 1 << 43


def states(ll, thr, seed, n, ref):
    """The generations themselves, [T][n] int32 (slot 0 the retained particle), and their masses [T][k]."""
    T, k = len(ll), len(ll[0])
    seed, n = int(seed), int(n)
    L = O.lib()
    xs = np.zeros((T, n), np.int32)
    out = []
    C = None
    for t in range(T):
        cnt = [0] * k
        r = int(ref[t]) & 7
        xs[t, 0] = min(r, k - 1)
        cnt[xs[t, 0]] += 1
        wg, wb, ag, ab = -1, None, -1, None                 # (the block last drawn for the words / the ancestors)
        for i in range(1, n):
            if i >> 2 != wg:
                wg, wb = i >> 2, [int(v) for v in O.draw_block(seed, i >> 2, t)]
            w = wb[i & 3]
            if t == 0:
                x = int(L.orc_smallint_from_bits(w, 0, k - 1))
            else:
                if i >> 1 != ag:
                    ag, ab = i >> 1, [int(v) for v in O.draw_block(seed, i >> 1, DRAW_BASE + t)]
                W = (ab[2 * (i & 1) + 1] << 32) | ab[2 * (i & 1)]
                V = (W * C[k - 1]) >> 64
                a = sum(1 for s in range(k - 1) if V >= C[s])
                x = sum(1 for j in range(k - 1) if w >= int(thr[a][j]))
            xs[t, i] = x
            cnt[x] += 1
        M = max(float(ll[t][s]) for s in range(k) if cnt[s] > 0)
        q = O.fix_weights(np.array(ll[t], np.float64), M)
        m = [cnt[s] * int(q[s]) for s in range(k)]
        out.append(m)
        C, run = [], 0
        for s in range(k):
            run += m[s]
            C.append(run)
    return xs, out


def masses(ll, thr, seed, n, ref):
    """[T][k] integers: the rows of the m table a conditional run of the problem leaves."""
    return states(ll, thr, seed, n, ref)[1]
