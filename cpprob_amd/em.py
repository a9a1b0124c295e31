"""Particle EM for the tables of MODEL_HMM_TABLE problems: the E-step is Engine.batch_smooth_stats (the backward smoother's expected
sufficient statistics, one record a problem, computed on the device), the M-step below is 88 doubles a problem on the host.  The
model fixes the emission's sigma at 1, so a table is its means and its transition rows; the initial state is uniform and not fitted."""
import numpy as np

from .capi import MODEL_HMM_TABLE, RESAMPLE_SYSTEMATIC, STATS_PER_PROBLEM


def m_step(stats, means, trans):
    """The tables that maximise the expected complete-data log-likelihood under `stats` (a dict as Engine.batch_smooth_stats returns:
    xi [B, 8, 8], occ, occ_y [B, 8]): trans[b, s, :] = xi[b, s, :k] / its sum, means[b, s] = occ_y[b, s] / occ[b, s], k =
    means.shape[1].  A transition row or a state with no mass keeps its previous value; states >= k of the statistics are not read.
    Pure numpy; returns new (means [B, k], trans [B, k, k])."""
    means = np.array(means, np.float64)
    trans = np.array(trans, np.float64)
    if means.ndim != 2 or trans.shape != (means.shape[0], means.shape[1], means.shape[1]):
        raise ValueError("means [B, k], trans [B, k, k]")
    k = means.shape[1]
    xi = np.asarray(stats["xi"], np.float64)[:, :k, :k]
    occ = np.asarray(stats["occ"], np.float64)[:, :k]
    occ_y = np.asarray(stats["occ_y"], np.float64)[:, :k]
    if xi.shape[0] != means.shape[0]:
        raise ValueError("one record of statistics per table")
    row = np.zeros(xi.shape[:2])
    for j in range(k):                                      # (in the order s' = 0..k-1, as the C++ M-step adds them)
        row = row + xi[:, :, j]
    fit = row > 0.0
    trans[fit] = xi[fit] / row[fit][:, None]
    seen = occ > 0.0
    means[seen] = occ_y[seen] / occ[seen]
    return means, trans


def hmm_table_em(engine, observes, means0, trans0, n_particles, seeds, iterations, resampler=RESAMPLE_SYSTEMATIC, keep_history=True, resident=False):
    """Batched particle EM.  observes: a list of B 1-D sequences, or one sequence every problem shares (restarts: one sequence under
    B initial tables); means0 [B, k], trans0 [B, k, k] the initial tables; seeds [B].  Iteration i begins a batch with the current
    tables (batch_begin_problems), runs it with seeds + i, takes the statistics and the M-step.  Returns (means [iterations + 1, B, k],
    trans [iterations + 1, B, k, k], log_evidence [iterations, B]): the tables before every iteration and after the last, and the
    log-evidence estimate of every iteration's run (of the tables it began with).  keep_history=False: the batches are filtering-only
    and keep the smoother's masses (keep_masses) -- the same arrays bit for bit, without a particle store.
    resident=True: one batch_begin_problems, then the whole loop is enqueued on the engine's stream -- per iteration batch_run,
    batch_smooth_stats_device, batch_summaries_device, batch_mstep_device and batch_retable_device on tensors that stay on the device
    -- and the tables of every iteration and the evidences are read once after it.  The same arrays bit for bit."""
    means = np.array(means0, np.float64)
    trans = np.array(trans0, np.float64)
    B = means.shape[0]
    if isinstance(observes, np.ndarray) and observes.ndim == 1:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    if resident and int(iterations) > 0:
        return _em_resident(engine, seqs, means, trans, n_particles, sd, int(iterations), resampler, bool(keep_history))
    m_hist, t_hist, ev = [means.copy()], [trans.copy()], np.zeros((int(iterations), B))
    for it in range(int(iterations)):
        engine.batch_begin_problems(MODEL_HMM_TABLE, seqs, n_particles, tables=(means, trans), resampler=resampler, keep_history=bool(keep_history),
                                    keep_masses=not keep_history)
        engine.batch_run(sd + np.uint64(it))
        stats = engine.batch_smooth_stats(seqs)
        ev[it] = [s["log_evidence"] for s in engine.batch_results()[0]]
        means, trans = m_step(stats, means, trans)
        m_hist.append(means.copy())
        t_hist.append(trans.copy())
    return np.array(m_hist), np.array(t_hist), ev


def _em_resident(engine, seqs, means, trans, n_particles, sd, iterations, resampler, keep_history):
    """hmm_table_em's loop with the tables, the observes, the records and the evidences in device tensors; the host enqueues and
    looks at nothing until the loop is over."""
    import torch
    B, k = means.shape
    dev = torch.device("cuda", engine.device)
    engine.batch_begin_problems(MODEL_HMM_TABLE, seqs, n_particles, tables=(means, trans), resampler=resampler, keep_history=keep_history, keep_masses=not keep_history)
    obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(seqs))).to(dev)
    m_all = torch.zeros((iterations + 1, B, k), dtype=torch.float64, device=dev)
    t_all = torch.zeros((iterations + 1, B, k, k), dtype=torch.float64, device=dev)
    m_all[0].copy_(torch.from_numpy(means))
    t_all[0].copy_(torch.from_numpy(trans))
    stats = torch.zeros((B, STATS_PER_PROBLEM), dtype=torch.float64, device=dev)
    ev = torch.zeros((iterations, B, 4), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()            # (the engine's stream is not ordered behind torch's: the tensors are complete first)
    stream = torch.cuda.ExternalStream(engine.stream_ptr, device=dev)
    for it in range(iterations):
        engine.batch_run(sd + np.uint64(it))
        engine.batch_smooth_stats_device(stats, obs)
        engine.batch_summaries_device(ev[it])
        with torch.cuda.stream(stream):                     # (the next tables start as these: a copy on the engine's stream)
            m_all[it + 1].copy_(m_all[it])
            t_all[it + 1].copy_(t_all[it])
        engine.batch_mstep_device(stats, m_all[it + 1], t_all[it + 1])
        if it + 1 < iterations:
            engine.batch_retable_device(m_all[it + 1], t_all[it + 1], obs)
    engine.sync()
    return m_all.cpu().numpy(), t_all.cpu().numpy(), np.ascontiguousarray(ev[:, :, 0].cpu().numpy())
