"""The forecasts of a batch (csrc/batch_forecast.hpp) restated in plain Python integers and floats, on top of
tests/backward_ref.py (thresholds, transition_masses, filtering_masses, the oracle's Philox blocks and 53-bit uniform): the reference
of tests/test_forecast_ref_host.py, tests/test_batch_forecast_kernel_text_host.py and the GPU tests.  Every product and sum below is
one IEEE double operation (Python floats never contract)."""
import numpy as np

import backward_ref as R
from oracle import oracle as O

DRAW_BASE = 1 << 42
TWO32 = 1 << 32


def probabilities(P):
    """p[s][s'] = double(P[s][s']) * 2^-32: exact, a scaling by a power of two."""
    return [[float(v) * 2.0 ** -32 for v in row] for row in P]


def start(m_row):
    """smooth_marginal_start: the normalised filtering masses of one row of the m table."""
    tot = sum(int(v) for v in m_row)
    return [float(v) / float(tot) for v in m_row]


def push(f, p):
    """push(f)[s'] = sum over s = 0..k-1, in that order, of f[s] * p[s][s'], from 0.0, the terms with f[s] == 0 left out."""
    k = len(f)
    out = []
    for sn in range(k):
        acc = 0.0
        for s in range(k):
            if f[s] == 0.0:
                continue
            acc = acc + f[s] * p[s][sn]
        out.append(acc)
    return out


def marginals(m, P, H):
    """f_1 .. f_H as [H, k]; zeros for a problem of length 0."""
    k = len(P)
    out = np.zeros((H, k))
    if len(m) == 0:
        return out
    p = probabilities(P)
    f = start(m[-1])
    for h in range(H):
        f = push(f, p)
        out[h] = f
    return out


def predictive(m, P):
    """r_0 .. r_L as [L + 1, k]."""
    k = len(P)
    p = probabilities(P)
    rows = [[1.0 / float(k)] * k]
    for t in range(1, len(m) + 1):
        rows.append(push(start(m[t - 1]), p))
    return np.array(rows)


def predictive_rows(m, P, frm, n_rows, spp):
    """The call's output rows of one problem: [n_rows, spp], row r = r_{frm + r} for frm + r <= L, zero elsewhere and for states >= k."""
    k = len(P)
    full = predictive(m, P)
    out = np.zeros((n_rows, spp))
    for r in range(n_rows):
        if frm + r <= len(m):
            out[r, :k] = full[frm + r]
    return out


def trajectories(m, P_thr, seed, H, n_traj, draw_index=0, columns=None):
    """[H + 1, n_traj] int32.  P_thr: the threshold rows c[s][0 .. k-2] (R.thresholds).  Row 0 by the backward simulation's start
    rule on m_{L-1}; row h by the forward draw's statement on word 2 (j & 1) of the block of ordinal 2^42 + (draw_index << 24) + h.
    A problem of length 0: zeros.  columns: the trajectories wanted (indices below n_traj, any order); the result then holds those
    columns of the full [H + 1, n_traj] only, and only their blocks are drawn (as backward_ref.trajectories_fast's argument)."""
    cols = np.arange(n_traj, dtype=np.int64) if columns is None else np.asarray(columns, np.int64).reshape(-1)
    assert cols.size == 0 or (0 <= int(cols.min()) and int(cols.max()) < n_traj)
    out = np.zeros((H + 1, cols.size), np.int32)
    if len(m) == 0 or cols.size == 0:
        return out
    k = len(m[-1])
    L = O.lib()
    w = [float(v) for v in m[-1]]
    c, run = [], 0.0
    for s in range(k):
        run = run + w[s]
        c.append(run)
    last = max([s for s in range(k) if w[s] > 0.0] or [0])
    base = DRAW_BASE + (int(draw_index) << 24)
    blk = np.zeros(4, np.uint32)
    thr = [[int(v) for v in row] for row in P_thr]
    served = {}                                                    # block g serves trajectories 2 g and 2 g + 1: the places of each
    for i, j in enumerate(cols.tolist()):
        served.setdefault(j >> 1, []).append((i, j & 1))
    for g, places in served.items():
        L.orc_draw_block(int(seed), int(g), base, blk)
        x = {}
        for half in set(h for _, h in places):
            u = float(L.orc_u01_53(int(blk[2 * half]), int(blk[2 * half + 1])))
            target = u * c[k - 1]
            hit = [s for s in range(k) if c[s] > target]
            x[half] = hit[0] if hit else last
        for i, half in places:
            out[0, i] = x[half]
        for h in range(1, H + 1):
            L.orc_draw_block(int(seed), int(g), base + h, blk)
            for half in x:
                word = int(blk[2 * half])
                x[half] = sum(1 for i in range(k - 1) if word >= thr[x[half]][i])
            for i, half in places:
                out[h, i] = x[half]
    return out
