"""EM for HMMs whose observe of a step is a Gaussian vector with a full covariance: MODEL_HMM_TABLE problems with full-covariance
emissions (csrc/batch_full.hpp).  A table is the means [k, D] and covariances [k, D, D] (k <= 8 states, D <= 16 coordinates) and the
transition rows [k, k]; the initial state is uniform and not fitted.  The E-step is Engine.batch_full_stats -- the backward smoother's
record and, beside it, the visits of every state weighted by every coordinate and by every product of two, two kernels on the device --,
the M-step below is 1304 doubles a problem on the host, or the device's own."""
import numpy as np

from .capi import FULL_STATS_PER_PROBLEM, RESAMPLE_SYSTEMATIC

_TWO_PI = np.float64(2 * 3.14159265358979323846)
_MIN_NORMAL = np.float64(2.0 ** -1022)


def _check_floor(var_floor):
    floor = np.float64(var_floor)
    if not (floor > 0.0) or not np.isfinite(floor):
        raise ValueError("var_floor must be finite and > 0")
    return floor


def _tables(means, covs, trans):
    means, covs, trans = np.array(means, np.float64), np.array(covs, np.float64), np.array(trans, np.float64)
    if means.ndim != 3 or covs.shape != means.shape + means.shape[2:] or trans.shape != (means.shape[0], means.shape[1], means.shape[1]):
        raise ValueError("means [B, k, D], covs [B, k, D, D] and trans [B, k, k]")
    return means, covs, trans


def factor(c):
    """full_factor on N matrices at once: c [N, D, D], the lower triangles read.  Returns (L [N, D, D], ok [N]); every entry takes the
    device's operations in the device's order, one numpy operation each."""
    c = np.asarray(c, np.float64)
    N, D = c.shape[0], c.shape[1]
    L, ok = np.zeros((N, D, D)), np.ones(N, bool)
    with np.errstate(all="ignore"):
        for j in range(D):
            for i in range(j, D):
                a = c[:, i, j].copy()
                ok &= np.isfinite(a)
                for p in range(j):
                    a = a - L[:, i, p] * L[:, j, p]
                if i == j:
                    r = np.sqrt(a)
                    arg = (_TWO_PI * r) * r
                    ok &= (a > 0.0) & (r > 0.0) & (r < np.inf) & (arg >= _MIN_NORMAL) & (arg < np.inf)
                    L[:, j, j] = r
                else:
                    L[:, i, j] = a / L[:, j, j]
    return L, ok


def m_step_full(stats, means, covs, trans, var_floor=1e-6):
    """The tables that maximise the expected complete-data log-likelihood under `stats` (a dict as Engine.batch_full_stats returns: xi
    [B, 8, 8], occ [B, 8], sy [B, 8, 16], syy [B, 8, 16, 16]): trans[b, s, :] = xi[b, s, :k] / its sum; for a state with occ > 0,
    mean = sy / occ and c[i][j] = syy[i][j] / occ - mean_i mean_j, a diagonal entry not below var_floor^2 (a NaN takes it too).  A
    candidate that does not factor (csrc/batch_full.hpp: full_factor) leaves the state's mean and covariance as they were, as a state
    without mass; a transition row without mass stays too.  Pure numpy; returns new (means [B, k, D], covs [B, k, D, D], trans
    [B, k, k]).  The statements of csrc/batch_full.hpp, which cpprob_hip_batch_mstep_full_device runs bit for bit."""
    floor = _check_floor(var_floor)
    means, covs, trans = _tables(means, covs, trans)
    B, k, D = means.shape
    xi = np.asarray(stats["xi"], np.float64)[:, :k, :k]
    occ = np.asarray(stats["occ"], np.float64)[:, :k]
    sy = np.asarray(stats["sy"], np.float64)[:, :k, :D]
    syy = np.asarray(stats["syy"], np.float64)[:, :k, :D, :D]
    row = np.zeros((B, k))
    for j in range(k):                                      # (sequential: the device's order of additions)
        row = row + xi[:, :, j]
    with np.errstate(all="ignore"):
        fit = row > 0.0
        trans[fit] = xi[fit] / row[fit][:, None]
        seen = occ > 0.0
        mass = occ[seen]
        mu = sy[seen] / mass[:, None]
        c = syy[seen] / mass[:, None, None]
        c = c - mu[:, :, None] * mu[:, None, :]
        d = np.arange(D)
        ff = floor * floor
        c[:, d, d] = np.where(c[:, d, d] >= ff, c[:, d, d], ff)
        _, ok = factor(c)
        low = np.tril(c)
        sym = low + np.transpose(np.tril(c, -1), (0, 2, 1))
        new_mu, new_c = means[seen], covs[seen]
        new_mu[ok], new_c[ok] = mu[ok], sym[ok]
        means[seen], covs[seen] = new_mu, new_c
    return means, covs, trans


def hmm_full_em(engine, observes, means0, covs0, trans0, n_particles, seeds, iterations, exact=False, resident=False, var_floor=1e-6,
                resampler=RESAMPLE_SYSTEMATIC):
    """Batched EM for HMMs with full-covariance Gaussian vector emissions.  observes: a list of B arrays [T_b, D], or one array [T, D]
    every problem shares; means0 [B, k, D], covs0 [B, k, D, D], trans0 [B, k, k] the initial tables; seeds [B].  One
    batch_begin_problems_full (filtering-only, keeping the smoother's masses); iteration i runs the batch with seeds + i -- exact=True:
    Engine.batch_run_exact, and the fit is Baum-Welch up to that run's quantisations; n_particles and seeds are then not used --, takes
    batch_full_stats and the M-step, and re-tables the batch where it stands.  Returns (means [iterations + 1, B, k, D], covs
    [iterations + 1, B, k, D, D], trans [iterations + 1, B, k, k], log_evidence [iterations, B]): the tables before every iteration and
    after the last, and every run's log-evidence of the tables it ran with.  resident=True: the loop is enqueued on the engine's stream
    -- batch_full_stats_device, batch_mstep_full_device and batch_retable_full_device on tensors that stay on the device; an M-step's
    output always factors, so no re-table needs a look -- and read once after it; the same arrays bit for bit."""
    floor = float(_check_floor(var_floor))
    means, covs, trans = _tables(means0, covs0, trans0)
    B, D = means.shape[0], means.shape[2]
    if isinstance(observes, np.ndarray) and observes.ndim == 2:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1, D) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    iterations = int(iterations)
    m_hist, c_hist, t_hist, ev = [means.copy()], [covs.copy()], [trans.copy()], np.zeros((iterations, B))
    if iterations == 0:
        return np.array(m_hist), np.array(c_hist), np.array(t_hist), ev
    engine.batch_begin_problems_full(seqs, n_particles, means, covs, trans, resampler=resampler, keep_history=False, keep_masses=True)
    if resident:
        return _em_resident(engine, seqs, means, covs, trans, sd, iterations, bool(exact), floor)
    for it in range(iterations):
        if exact:
            engine.batch_run_exact()
        else:
            engine.batch_run(sd + np.uint64(it))
        stats = engine.batch_full_stats(seqs)
        ev[it] = engine.batch_exact_evidence()[0] if exact else [s["log_evidence"] for s in engine.batch_results()[0]]
        means, covs, trans = m_step_full(stats, means, covs, trans, floor)
        m_hist.append(means.copy())
        c_hist.append(covs.copy())
        t_hist.append(trans.copy())
        if it + 1 < iterations:
            engine.batch_retable_full(means, covs, trans, seqs if it == 0 else None)
    return np.array(m_hist), np.array(c_hist), np.array(t_hist), ev


def _em_resident(engine, seqs, means, covs, trans, sd, iterations, exact, floor):
    """hmm_full_em's loop on the begun batch with the tables, the observes, the records and the evidences in device tensors; the host
    enqueues and looks at nothing until the loop is over."""
    import torch
    B, k, D = means.shape
    dev = torch.device("cuda", engine.device)
    obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(seqs).reshape(-1))).to(dev)
    m_all = torch.zeros((iterations + 1, B, k, D), dtype=torch.float64, device=dev)
    c_all = torch.zeros((iterations + 1, B, k, D, D), dtype=torch.float64, device=dev)
    t_all = torch.zeros((iterations + 1, B, k, k), dtype=torch.float64, device=dev)
    m_all[0].copy_(torch.from_numpy(means))
    c_all[0].copy_(torch.from_numpy(covs))
    t_all[0].copy_(torch.from_numpy(trans))
    stats = torch.zeros((B, FULL_STATS_PER_PROBLEM), dtype=torch.float64, device=dev)
    ev = torch.zeros((iterations, B, 4), dtype=torch.float64, device=dev)
    ev_exact = torch.zeros((iterations, B), dtype=torch.float64, device=dev) if exact else None
    dead = torch.zeros(B, dtype=torch.int32, device=dev) if exact else None
    torch.cuda.current_stream(dev).synchronize()            # (the engine's stream is not ordered behind torch's: the tensors are complete first)
    stream = torch.cuda.ExternalStream(engine.stream_ptr, device=dev)
    for it in range(iterations):
        if exact:
            engine.batch_run_exact()
        else:
            engine.batch_run(sd + np.uint64(it))
        engine.batch_full_stats_device(stats, obs)
        if exact:
            engine.batch_exact_evidence_device(ev_exact[it], dead)
        else:
            engine.batch_summaries_device(ev[it])
        with torch.cuda.stream(stream):                     # (the next tables start as these: a copy on the engine's stream)
            m_all[it + 1].copy_(m_all[it])
            c_all[it + 1].copy_(c_all[it])
            t_all[it + 1].copy_(t_all[it])
        engine.batch_mstep_full_device(stats, m_all[it + 1], c_all[it + 1], t_all[it + 1], floor)
        if it + 1 < iterations:
            engine.batch_retable_full_device(m_all[it + 1], c_all[it + 1], t_all[it + 1], obs)
    engine.sync()
    ev_host = np.ascontiguousarray((ev_exact if exact else ev[:, :, 0]).cpu().numpy())
    return m_all.cpu().numpy(), c_all.cpu().numpy(), t_all.cpu().numpy(), ev_host
