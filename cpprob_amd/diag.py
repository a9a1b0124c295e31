"""EM for HMMs whose observe of a step is a vector with independent Gaussian coordinates: MODEL_HMM_TABLE problems with diagonal-Gaussian
emissions (csrc/batch_diag.hpp).  A table is the means [k, D] and sigmas [k, D] (k <= 8 states, D <= 32 coordinates) and the transition
rows [k, k]; the initial state is uniform and not fitted.  The E-step is Engine.batch_diag_stats -- the backward smoother's record and,
beside it, the visits of every state weighted by every coordinate and its square, one kernel on the device --, the M-step below is 600
doubles a problem on the host, or the device's own."""
import numpy as np

from .capi import DIAG_STATS_PER_PROBLEM, RESAMPLE_SYSTEMATIC


def _check_floor(sigma_floor):
    floor = np.float64(sigma_floor)
    if not (floor > 0.0) or not np.isfinite(floor):
        raise ValueError("sigma_floor must be finite and > 0")
    return floor


def _tables(means, sigmas, trans):
    means, sigmas, trans = np.array(means, np.float64), np.array(sigmas, np.float64), np.array(trans, np.float64)
    if means.ndim != 3 or sigmas.shape != means.shape or trans.shape != (means.shape[0], means.shape[1], means.shape[1]):
        raise ValueError("means and sigmas [B, k, D] and trans [B, k, k]")
    return means, sigmas, trans


def m_step_diag(stats, means, sigmas, trans, sigma_floor=1e-3):
    """The tables that maximise the expected complete-data log-likelihood under `stats` (a dict as Engine.batch_diag_stats returns: xi
    [B, 8, 8], occ [B, 8], sy and syy [B, 8, 32]): trans[b, s, :] = xi[b, s, :k] / its sum; for a state with occ > 0,
    means[b, s, d] = sy / occ and v = syy / occ - mean mean, sigmas[b, s, d] = sqrt(v) where v >= sigma_floor^2, else sigma_floor (a NaN
    too).  A transition row or a state with no mass keeps its previous value.  Pure numpy; returns new (means [B, k, D], sigmas
    [B, k, D], trans [B, k, k]).  The statements of csrc/batch_diag.hpp, which cpprob_hip_batch_mstep_diag_device runs bit for bit."""
    floor = _check_floor(sigma_floor)
    means, sigmas, trans = _tables(means, sigmas, trans)
    B, k, D = means.shape
    xi = np.asarray(stats["xi"], np.float64)[:, :k, :k]
    occ = np.asarray(stats["occ"], np.float64)[:, :k]
    sy = np.asarray(stats["sy"], np.float64)[:, :k, :D]
    syy = np.asarray(stats["syy"], np.float64)[:, :k, :D]
    row = np.zeros((B, k))
    for j in range(k):                                      # (sequential: the device's order of additions)
        row = row + xi[:, :, j]
    with np.errstate(all="ignore"):
        fit = row > 0.0
        trans[fit] = xi[fit] / row[fit][:, None]
        seen = occ > 0.0
        mass = occ[seen][:, None]
        mu = sy[seen] / mass
        v = syy[seen] / mass
        v = v - mu * mu
        means[seen] = mu
        sigmas[seen] = np.where(v >= floor * floor, np.sqrt(v), floor)
    return means, sigmas, trans


def hmm_diag_em(engine, observes, means0, sigmas0, trans0, n_particles, seeds, iterations, exact=False, resident=False, sigma_floor=1e-3,
                resampler=RESAMPLE_SYSTEMATIC):
    """Batched EM for HMMs with diagonal-Gaussian vector emissions.  observes: a list of B arrays [T_b, D], or one array [T, D] every
    problem shares; means0 and sigmas0 [B, k, D], trans0 [B, k, k] the initial tables; seeds [B].  One batch_begin_problems_diag
    (filtering-only, keeping the smoother's masses); iteration i runs the batch with seeds + i -- exact=True: Engine.batch_run_exact,
    and the fit is Baum-Welch up to that run's quantisations; n_particles and seeds are then not used --, takes batch_diag_stats and
    the M-step, and re-tables the batch where it stands.  Returns (means [iterations + 1, B, k, D], sigmas [iterations + 1, B, k, D],
    trans [iterations + 1, B, k, k], log_evidence [iterations, B]): the tables before every iteration and after the last, and every
    run's log-evidence of the tables it ran with.  resident=True: the loop is enqueued on the engine's stream -- batch_diag_stats_device,
    batch_mstep_diag_device and batch_retable_diag_device on tensors that stay on the device -- and read once after it; the same arrays
    bit for bit."""
    floor = float(_check_floor(sigma_floor))
    means, sigmas, trans = _tables(means0, sigmas0, trans0)
    B, D = means.shape[0], means.shape[2]
    if isinstance(observes, np.ndarray) and observes.ndim == 2:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1, D) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    iterations = int(iterations)
    m_hist, s_hist, t_hist, ev = [means.copy()], [sigmas.copy()], [trans.copy()], np.zeros((iterations, B))
    if iterations == 0:
        return np.array(m_hist), np.array(s_hist), np.array(t_hist), ev
    engine.batch_begin_problems_diag(seqs, n_particles, means, sigmas, trans, resampler=resampler, keep_history=False, keep_masses=True)
    if resident:
        return _em_resident(engine, seqs, means, sigmas, trans, sd, iterations, bool(exact), floor)
    for it in range(iterations):
        if exact:
            engine.batch_run_exact()
        else:
            engine.batch_run(sd + np.uint64(it))
        stats = engine.batch_diag_stats(seqs)
        ev[it] = engine.batch_exact_evidence()[0] if exact else [s["log_evidence"] for s in engine.batch_results()[0]]
        means, sigmas, trans = m_step_diag(stats, means, sigmas, trans, floor)
        m_hist.append(means.copy())
        s_hist.append(sigmas.copy())
        t_hist.append(trans.copy())
        if it + 1 < iterations:
            engine.batch_retable_diag(means, sigmas, trans, seqs if it == 0 else None)
    return np.array(m_hist), np.array(s_hist), np.array(t_hist), ev


def _em_resident(engine, seqs, means, sigmas, trans, sd, iterations, exact, floor):
    """hmm_diag_em's loop on the begun batch with the tables, the observes, the records and the evidences in device tensors; the host
    enqueues and looks at nothing until the loop is over."""
    import torch
    B, k, D = means.shape
    dev = torch.device("cuda", engine.device)
    obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(seqs).reshape(-1))).to(dev)
    m_all = torch.zeros((iterations + 1, B, k, D), dtype=torch.float64, device=dev)
    s_all = torch.zeros((iterations + 1, B, k, D), dtype=torch.float64, device=dev)
    t_all = torch.zeros((iterations + 1, B, k, k), dtype=torch.float64, device=dev)
    m_all[0].copy_(torch.from_numpy(means))
    s_all[0].copy_(torch.from_numpy(sigmas))
    t_all[0].copy_(torch.from_numpy(trans))
    stats = torch.zeros((B, DIAG_STATS_PER_PROBLEM), dtype=torch.float64, device=dev)
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
        engine.batch_diag_stats_device(stats, obs)
        if exact:
            engine.batch_exact_evidence_device(ev_exact[it], dead)
        else:
            engine.batch_summaries_device(ev[it])
        with torch.cuda.stream(stream):                     # (the next tables start as these: a copy on the engine's stream)
            m_all[it + 1].copy_(m_all[it])
            s_all[it + 1].copy_(s_all[it])
            t_all[it + 1].copy_(t_all[it])
        engine.batch_mstep_diag_device(stats, m_all[it + 1], s_all[it + 1], t_all[it + 1], floor)
        if it + 1 < iterations:
            engine.batch_retable_diag_device(m_all[it + 1], s_all[it + 1], t_all[it + 1], obs)
    engine.sync()
    ev_host = np.ascontiguousarray((ev_exact if exact else ev[:, :, 0]).cpu().numpy())
    return m_all.cpu().numpy(), s_all.cpu().numpy(), t_all.cpu().numpy(), ev_host
