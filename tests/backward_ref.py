"""The backward smoother of a batch (csrc/batch_smooth.hpp) restated in plain Python integers and floats: the
reference of tests/test_backward_ref_host.py and tests/test_gpu_batch_smooth.py.  Every product and sum below is one IEEE double
operation (Python floats never contract), the integer weights are the oracle's (oracle.fix_weights), the uniforms the oracle's Philox
blocks (oracle.draw_block, orc_u01_53) and the thresholds the host's own statements (ceil((acc / tot) 2^32) on sequential sums)."""
import numpy as np

from oracle import exact
from oracle import oracle as O

DRAW_BASE = 1 << 41
TWO32 = 1 << 32


def thresholds(trans):
    """c[s][0 .. k-2] = ceil((acc / tot) 2^32) over the sequential sums of row s, as hmmk_thresholds / host_model_params compute them."""
    trans = np.asarray(trans, np.float64)
    k = trans.shape[0]
    thr = []
    for s in range(k):
        tot = 0.0
        for j in range(k):
            tot += float(trans[s, j])
        acc, row = 0.0, []
        for j in range(k - 1):
            acc += float(trans[s, j])
            row.append(int(np.ceil((acc / tot) * 4294967296.0)))
        thr.append(row)
    return thr


def transition_masses(trans):
    """P[s][s'] = c[s][s'] - c[s][s'-1], c[s][-1] = 0, c[s][k-1] = 2^32: integers."""
    k = len(trans)
    P = []
    for row in thresholds(trans):
        c = [0] + row + [TWO32]
        P.append([c[j + 1] - c[j] for j in range(k)])
    return P


def log_likelihoods(obs, means):
    """ll[t][s] = log N(y_t; means[s], 1), the host's per-step table rows (the oracle's normal_logpdf is the host's own statement)."""
    L = O.lib()
    return [[float(L.orc_normal_logpdf(float(y), float(m), 1.0)) for m in means] for y in obs]


def filtering_masses(values, ll):
    """m[t][s] = cnt_t[s] * fix_weight(ll_t[s], M_t), M_t the largest ll_t[s] over the states present: integers."""
    k = len(ll[0])
    out = []
    for t in range(len(values)):
        cnt = np.bincount(np.asarray(values[t], np.int64), minlength=k)
        M = max(ll[t][s] for s in range(k) if cnt[s] > 0)
        q = O.fix_weights(np.array(ll[t], np.float64), M)
        out.append([int(cnt[s]) * int(q[s]) for s in range(k)])
    return out


def _weights(m_t, P, nxt):
    """Row `nxt` of a_t, or the filtering masses where that row sums to zero (the defensive rule)."""
    k = len(m_t)
    w = [float(m_t[s]) * float(P[s][nxt]) for s in range(k)]
    D = 0.0
    for s in range(k):
        D = D + w[s]
    if D == 0.0:
        w = [float(m_t[s]) for s in range(k)]
        D = 0.0
        for s in range(k):
            D = D + w[s]
    return w, D


def marginals(m, P):
    """g[t][s], t = T-1 .. 0."""
    T, k = len(m), len(m[0])
    g = [[0.0] * k for _ in range(T)]
    tot = sum(m[T - 1])
    g[T - 1] = [float(m[T - 1][s]) / float(tot) for s in range(k)]
    for t in range(T - 2, -1, -1):
        rows = [_weights(m[t], P, sn) for sn in range(k)]
        for s in range(k):
            acc = 0.0
            for sn in range(k):
                if g[t + 1][sn] == 0.0:
                    continue
                w, D = rows[sn]
                acc = acc + (w[s] / D) * g[t + 1][sn]
            g[t][s] = acc
    return np.array(g)


def uniform(seed, j, draw_index, t):
    r = O.draw_block(int(seed), j >> 1, DRAW_BASE + (int(draw_index) << 24) + t)
    return float(O.lib().orc_u01_53(int(r[2 * (j & 1)]), int(r[2 * (j & 1) + 1])))


def trajectories(m, P, seed, n_traj, draw_index=0):
    """[T][n_traj] int32."""
    T, k = len(m), len(m[0])
    out = np.zeros((T, n_traj), np.int32)
    # (the k rows of a step are shared by the trajectories: computed once a step)
    rows = [None] * T
    for t in range(T):
        if t == T - 1:
            rows[t] = [[float(x) for x in m[t]]] * k
        else:
            rows[t] = [_weights(m[t], P, sn)[0] for sn in range(k)]
    cums = [[np.cumsum(np.array(w)) for w in rows[t]] for t in range(T)]      # (numpy's cumsum adds sequentially, in doubles)
    last = [[max([s for s in range(k) if w[s] > 0.0] or [0]) for w in rows[t]] for t in range(T)]
    for j in range(n_traj):
        x = 0
        for t in range(T - 1, -1, -1):
            c = cums[t][x]
            target = uniform(seed, j, draw_index, t) * float(c[k - 1])
            hit = [s for s in range(k) if c[s] > target]
            x = hit[0] if hit else last[t][x]
            out[t, j] = x
    return out


def trajectories_fast(m, P, seed, n_traj, draw_index=0, columns=None):
    """trajectories(), with the uniforms drawn a block (two trajectories) at a time and the walk vectorised over the trajectories:
    the same doubles compared with the same doubles.  columns: the trajectories wanted (indices below n_traj, any order); the
    result then holds those columns of the full [T][n_traj] only, and only their blocks are drawn."""
    T, k = len(m), len(m[0])
    cols = np.arange(n_traj, dtype=np.int64) if columns is None else np.asarray(columns, np.int64).reshape(-1)
    assert cols.size == 0 or (0 <= int(cols.min()) and int(cols.max()) < n_traj)
    out = np.zeros((T, cols.size), np.int32)
    L = O.lib()
    x = np.zeros(cols.size, np.int64)
    blk = np.zeros(4, np.uint32)
    blocks, where = np.unique(cols >> 1, return_inverse=True)      # block g serves trajectories 2 g and 2 g + 1
    half = cols & 1
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            rows = [[float(v) for v in m[t]]] * k
        else:
            rows = [_weights(m[t], P, sn)[0] for sn in range(k)]
        cums = np.array([np.cumsum(np.array(w)) for w in rows])
        last = np.array([max([s for s in range(k) if w[s] > 0.0] or [0]) for w in rows])
        ub = np.zeros((blocks.size, 2))
        for i, g in enumerate(blocks):
            L.orc_draw_block(int(seed), int(g), DRAW_BASE + (int(draw_index) << 24) + t, blk)
            ub[i, 0] = L.orc_u01_53(int(blk[0]), int(blk[1]))
            ub[i, 1] = L.orc_u01_53(int(blk[2]), int(blk[3]))
        u = ub[where, half]
        c = cums[x]                                         # [columns][k]
        target = u * c[:, k - 1]
        above = c > target[:, None]
        first = np.argmax(above, axis=1)
        x = np.where(above.any(axis=1), first, last[x])
        out[t] = x
    return out


def hmm3_problem(values, obs):
    """(m, P) of an HMM3 problem from its store rows and observes."""
    return filtering_masses(values, log_likelihoods(obs, exact.HMM_MEAN)), transition_masses(exact.HMM_T)


def table_problem(values, obs, means, trans):
    """(m, P) of an HMM_TABLE problem."""
    return filtering_masses(values, log_likelihoods(obs, means)), transition_masses(trans)
