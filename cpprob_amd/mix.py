"""EM for HMMs whose states emit Gaussian mixtures: MODEL_HMM_TABLE problems with Gaussian-mixture vector emissions
(csrc/batch_mix.hpp).  A table is the weights [k, M], the means and sigmas [k, M, D] (k <= 8 states, M <= 8 components with independent
coordinates, D <= 16 coordinates) and the transition rows [k, k]; the initial state is uniform and not fitted.  The E-step is
Engine.batch_mix_stats -- the backward smoother's record and, beside it, the visits of every component of every state weighted by every
coordinate and its square, two kernels on the device --, the M-step below is 2200 doubles a problem on the host, or the device's own."""
import numpy as np

from .capi import MIX_STATS_PER_PROBLEM, RESAMPLE_SYSTEMATIC
from .diag import _check_floor


def _tables(weights, means, sigmas, trans):
    weights, means, sigmas, trans = np.array(weights, np.float64), np.array(means, np.float64), np.array(sigmas, np.float64), np.array(trans, np.float64)
    if means.ndim != 4 or sigmas.shape != means.shape or weights.shape != means.shape[:3] or trans.shape != (means.shape[0], means.shape[1], means.shape[1]):
        raise ValueError("weights [B, k, M], means and sigmas [B, k, M, D] and trans [B, k, k]")
    return weights, means, sigmas, trans


def m_step_mix(stats, weights, means, sigmas, trans, sigma_floor=1e-6):
    """The tables that maximise the expected complete-data log-likelihood under `stats` (a dict as Engine.batch_mix_stats returns: xi
    [B, 8, 8], occ_c [B, 8, 8], sy and syy [B, 8, 8, 16]): trans[b, s, :] = xi[b, s, :k] / its sum; for a state with
    occ = ((0 + occ_0) + occ_1) + ... > 0, weights[b, s, c] = occ_c / occ; a component with occ_c > 0 takes mean = sy / occ_c and
    v = syy / occ_c - mean mean, sigma = sqrt(v) where v >= sigma_floor^2, else sigma_floor (a NaN too); one with occ_c == 0 keeps
    mean and sigma and takes the weight 0.  A transition row or a state with no mass keeps its previous value.  Pure numpy; returns new
    (weights [B, k, M], means, sigmas [B, k, M, D], trans [B, k, k]).  The statements of csrc/batch_mix.hpp, which
    cpprob_hip_batch_mstep_mix_device runs bit for bit."""
    floor = _check_floor(sigma_floor)
    weights, means, sigmas, trans = _tables(weights, means, sigmas, trans)
    B, k, M, D = means.shape
    xi = np.asarray(stats["xi"], np.float64)[:, :k, :k]
    occ_c = np.asarray(stats["occ_c"], np.float64)[:, :k, :M]
    sy = np.asarray(stats["sy"], np.float64)[:, :k, :M, :D]
    syy = np.asarray(stats["syy"], np.float64)[:, :k, :M, :D]
    row, occ = np.zeros((B, k)), np.zeros((B, k))
    for j in range(k):                                      # (sequential: the device's order of additions)
        row = row + xi[:, :, j]
    for c in range(M):
        occ = occ + occ_c[:, :, c]
    with np.errstate(all="ignore"):
        fit = row > 0.0
        trans[fit] = xi[fit] / row[fit][:, None]
        seen = occ > 0.0
        weights[seen] = np.where(occ_c[seen] > 0.0, occ_c[seen] / occ[seen][:, None], 0.0)
        live = seen[:, :, None] & (occ_c > 0.0)
        mass = occ_c[live][:, None]
        mu = sy[live] / mass
        v = syy[live] / mass
        v = v - mu * mu
        means[live] = mu
        sigmas[live] = np.where(v >= floor * floor, np.sqrt(v), floor)
    return weights, means, sigmas, trans


def hmm_mix_em(engine, observes, weights0, means0, sigmas0, trans0, n_particles, seeds, iterations, exact=False, resident=False, sigma_floor=1e-6,
               resampler=RESAMPLE_SYSTEMATIC):
    """Batched EM for HMMs with Gaussian-mixture vector emissions.  observes: a list of B arrays [T_b, D], or one array [T, D] every
    problem shares; weights0 [B, k, M], means0 and sigmas0 [B, k, M, D], trans0 [B, k, k] the initial tables; seeds [B].  One
    batch_begin_problems_mix (filtering-only, keeping the smoother's masses); iteration i runs the batch with seeds + i -- exact=True:
    Engine.batch_run_exact, and the fit is Baum-Welch up to that run's quantisations; n_particles and seeds are then not used --, takes
    batch_mix_stats and the M-step, and re-tables the batch where it stands.  Returns (weights [iterations + 1, B, k, M], means and
    sigmas [iterations + 1, B, k, M, D], trans [iterations + 1, B, k, k], log_evidence [iterations, B]): the tables before every
    iteration and after the last, and every run's log-evidence of the tables it ran with.  resident=True: the loop is enqueued on the
    engine's stream -- batch_mix_stats_device, batch_mstep_mix_device and batch_retable_mix_device on tensors that stay on the device --
    and read once after it; the same arrays bit for bit."""
    floor = float(_check_floor(sigma_floor))
    tables = _tables(weights0, means0, sigmas0, trans0)
    B, D = tables[1].shape[0], tables[1].shape[3]
    if isinstance(observes, np.ndarray) and observes.ndim == 2:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1, D) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    iterations = int(iterations)
    hist, ev = [[t.copy()] for t in tables], np.zeros((iterations, B))
    if iterations == 0:
        return tuple(np.array(h) for h in hist) + (ev,)
    engine.batch_begin_problems_mix(seqs, n_particles, *tables, resampler=resampler, keep_history=False, keep_masses=True)
    if resident:
        return _em_resident(engine, seqs, tables, sd, iterations, bool(exact), floor)
    for it in range(iterations):
        if exact:
            engine.batch_run_exact()
        else:
            engine.batch_run(sd + np.uint64(it))
        stats = engine.batch_mix_stats(seqs)
        ev[it] = engine.batch_exact_evidence()[0] if exact else [s["log_evidence"] for s in engine.batch_results()[0]]
        tables = m_step_mix(stats, *tables, floor)
        for h, t in zip(hist, tables):
            h.append(t.copy())
        if it + 1 < iterations:
            engine.batch_retable_mix(*tables, seqs if it == 0 else None)
    return tuple(np.array(h) for h in hist) + (ev,)


def _em_resident(engine, seqs, tables, sd, iterations, exact, floor):
    """hmm_mix_em's loop on the begun batch with the tables, the observes, the records and the evidences in device tensors; the host
    enqueues and looks at nothing until the loop is over."""
    import torch
    B = tables[0].shape[0]
    dev = torch.device("cuda", engine.device)
    obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(seqs).reshape(-1))).to(dev)
    hist = [torch.zeros((iterations + 1,) + t.shape, dtype=torch.float64, device=dev) for t in tables]
    for h, t in zip(hist, tables):
        h[0].copy_(torch.from_numpy(t))
    stats = torch.zeros((B, MIX_STATS_PER_PROBLEM), dtype=torch.float64, device=dev)
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
        engine.batch_mix_stats_device(stats, obs)
        if exact:
            engine.batch_exact_evidence_device(ev_exact[it], dead)
        else:
            engine.batch_summaries_device(ev[it])
        with torch.cuda.stream(stream):                     # (the next tables start as these: a copy on the engine's stream)
            for h in hist:
                h[it + 1].copy_(h[it])
        nxt = [h[it + 1] for h in hist]
        engine.batch_mstep_mix_device(stats, *nxt, floor)
        if it + 1 < iterations:
            engine.batch_retable_mix_device(*nxt, obs)
    engine.sync()
    ev_host = np.ascontiguousarray((ev_exact if exact else ev[:, :, 0]).cpu().numpy())
    return tuple(h.cpu().numpy() for h in hist) + (ev_host,)
