"""EM for Markov-switching vector regressions (MS-VAR): MODEL_HMM_TABLE problems whose state s emits y_t ~ N(coef[s] x_t, covs[s]), y_t in
R^Q, on P covariates x_t known at the step (csrc/batch_vreg.hpp).  A table is the coefficients [k, Q, P] and covariances [k, Q, Q]
(k <= 8 states, Q + P <= 16) and the transition rows [k, k]; the initial state is uniform and not fitted; an intercept is a covariate
column of ones.  Hamilton's Markov-switching VAR is the case x_t = (1, y_{t-1}, .., y_{t-p}): var_design builds its observes.  The E-step
is Engine.batch_vreg_stats -- the full family's record over z_t = (y_t, x_t) --, the M-step below solves every state's normal equations
for all Q responses through one factorisation on the host, or the device does."""
import numpy as np

from .capi import FULL_MAX_DIM, FULL_STATS_PER_PROBLEM, RESAMPLE_SYSTEMATIC
from .full import _check_floor, factor
from .reg import solve


def _tables(coef, covs, trans):
    coef, covs, trans = np.array(coef, np.float64), np.array(covs, np.float64), np.array(trans, np.float64)
    if coef.ndim != 4 or covs.shape != coef.shape[:3] + coef.shape[2:3] or trans.shape != (coef.shape[0], coef.shape[1], coef.shape[1]):
        raise ValueError("coef [B, k, Q, P], covs [B, k, Q, Q] and trans [B, k, k]")
    if coef.shape[2] < 1 or coef.shape[3] < 1 or coef.shape[2] + coef.shape[3] > FULL_MAX_DIM:
        raise ValueError("Q and P must be at least 1 each and Q + P at most 16")
    return coef, covs, trans


def var_design(Y, p, intercept=True):
    """The observes [T - p, Q + P] of a VAR(p) HMM over the series Y [T, Q]: row t holds (Y_{t+p}, 1.0 if intercept, Y_{t+p-1}, ..,
    Y_t), so P = intercept + Q p."""
    Y, p = np.ascontiguousarray(Y, np.float64), int(p)
    if Y.ndim != 2 or Y.shape[1] < 1:
        raise ValueError("Y [T, Q], Q >= 1")
    Q = Y.shape[1]
    P = bool(intercept) + Q * p
    if p < 0 or P < 1 or Q + P > FULL_MAX_DIM or len(Y) < p:
        raise ValueError("P = intercept + Q p must be at least 1 and Q + P at most 16, and Y hold at least p rows")
    n = len(Y) - p
    cols = [Y[p:]] + ([np.ones((n, 1))] if intercept else []) + [Y[p - 1 - i:p - 1 - i + n] for i in range(p)]
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def m_step_vreg(stats, coef, covs, trans, var_floor=1e-6):
    """The tables that maximise the expected complete-data log-likelihood under `stats` (a dict as Engine.batch_vreg_stats returns: xi
    [B, 8, 8], occ [B, 8], syy [B, 8, 16, 16] over z = (y, x)): trans[b, s, :] = xi[b, s, :k] / its sum; for a state with occ > 0,
    row q of coef solves (sum g x x^T) beta_q = sum g x y_q and c[q][r] = sum g y_q y_r / occ - sum over i of beta_qi (sum g x_i y_r /
    occ), a diagonal entry not below var_floor^2 (a NaN takes it too).  A state whose system does not solve or whose candidate does not
    factor (csrc/batch_vreg.hpp: a pivot not > 0, anything not finite, full_factor's refusals) keeps coefficients and covariance, as a
    state without mass; a transition row without mass stays too.  Pure numpy; returns new (coef [B, k, Q, P], covs [B, k, Q, Q], trans
    [B, k, k]).  The statements of csrc/batch_vreg.hpp, which cpprob_hip_batch_mstep_vreg_device runs bit for bit."""
    floor = _check_floor(var_floor)
    coef, covs, trans = _tables(coef, covs, trans)
    B, k, Q, P = coef.shape
    xi = np.asarray(stats["xi"], np.float64)[:, :k, :k]
    occ = np.asarray(stats["occ"], np.float64)[:, :k]
    syy = np.asarray(stats["syy"], np.float64)[:, :k, :Q + P, :Q + P]
    row = np.zeros((B, k))
    for j in range(k):                                      # (sequential: the device's order of additions)
        row = row + xi[:, :, j]
    with np.errstate(all="ignore"):
        fit = row > 0.0
        trans[fit] = xi[fit] / row[fit][:, None]
        seen = (occ > 0.0) & (occ < np.inf)
        mass, z = occ[seen], syy[seen]
        ok = np.isfinite(z).all(axis=(1, 2))
        beta = np.zeros((len(mass), Q, P))
        for q in range(Q):                                  # (one factorisation on the device; the same entries of L here, Q times)
            beta[:, q], solved = solve(z[:, Q:, Q:], z[:, Q:, q])
            ok &= solved
        c = z[:, :Q, :Q] / mass[:, None, None]
        for i in range(P):
            c = c - beta[:, :, None, i] * (z[:, None, Q + i, :Q] / mass[:, None, None])
        d, ff = np.arange(Q), floor * floor
        c[:, d, d] = np.where(c[:, d, d] >= ff, c[:, d, d], ff)
        ok &= factor(c)[1]
        sym = np.tril(c) + np.transpose(np.tril(c, -1), (0, 2, 1))
        new_b, new_c = coef[seen], covs[seen]
        new_b[ok], new_c[ok] = beta[ok], sym[ok]
        coef[seen], covs[seen] = new_b, new_c
    return coef, covs, trans


def hmm_vreg_em(engine, observes, coef0, covs0, trans0, n_particles, seeds, iterations, exact=False, resident=False, var_floor=1e-6,
                resampler=RESAMPLE_SYSTEMATIC):
    """Batched EM for Markov-switching vector regressions.  observes: a list of B arrays [T_b, Q + P] (the responses first, then the
    covariates), or one such array every problem shares; coef0 [B, k, Q, P], covs0 [B, k, Q, Q], trans0 [B, k, k] the initial tables;
    seeds [B].  One batch_begin_problems_vreg (filtering-only, keeping the smoother's masses); iteration i runs the batch with seeds + i
    -- exact=True: Engine.batch_run_exact, and the fit is Baum-Welch up to that run's quantisations; n_particles and seeds are then not
    used --, takes batch_vreg_stats and the M-step, and re-tables the batch where it stands.  Returns (coef [iterations + 1, B, k, Q, P],
    covs [iterations + 1, B, k, Q, Q], trans [iterations + 1, B, k, k], log_evidence [iterations, B]): the tables before every
    iteration and after the last, and every run's log-evidence of the tables it ran with.  resident=True: the loop is enqueued on the
    engine's stream -- batch_vreg_stats_device, batch_mstep_vreg_device and batch_retable_vreg_device on tensors that stay on the
    device; an M-step's output always factors, so no re-table needs a look -- and read once after it; the same arrays bit for bit."""
    floor = float(_check_floor(var_floor))
    coef, covs, trans = _tables(coef0, covs0, trans0)
    B, D = coef.shape[0], coef.shape[2] + coef.shape[3]
    if isinstance(observes, np.ndarray) and observes.ndim == 2:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1, D) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    iterations = int(iterations)
    b_hist, c_hist, t_hist, ev = [coef.copy()], [covs.copy()], [trans.copy()], np.zeros((iterations, B))
    if iterations == 0:
        return np.array(b_hist), np.array(c_hist), np.array(t_hist), ev
    engine.batch_begin_problems_vreg(seqs, n_particles, coef, covs, trans, resampler=resampler, keep_history=False, keep_masses=True)
    if resident:
        return _em_resident(engine, seqs, coef, covs, trans, sd, iterations, bool(exact), floor)
    for it in range(iterations):
        if exact:
            engine.batch_run_exact()
        else:
            engine.batch_run(sd + np.uint64(it))
        stats = engine.batch_vreg_stats(seqs)
        ev[it] = engine.batch_exact_evidence()[0] if exact else [s["log_evidence"] for s in engine.batch_results()[0]]
        coef, covs, trans = m_step_vreg(stats, coef, covs, trans, floor)
        b_hist.append(coef.copy())
        c_hist.append(covs.copy())
        t_hist.append(trans.copy())
        if it + 1 < iterations:
            engine.batch_retable_vreg(coef, covs, trans, seqs if it == 0 else None)
    return np.array(b_hist), np.array(c_hist), np.array(t_hist), ev


def _em_resident(engine, seqs, coef, covs, trans, sd, iterations, exact, floor):
    """hmm_vreg_em's loop on the begun batch with the tables, the observes, the records and the evidences in device tensors; the host
    enqueues and looks at nothing until the loop is over."""
    import torch
    B, k, Q, P = coef.shape
    dev = torch.device("cuda", engine.device)
    obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(seqs).reshape(-1))).to(dev)
    b_all = torch.zeros((iterations + 1, B, k, Q, P), dtype=torch.float64, device=dev)
    c_all = torch.zeros((iterations + 1, B, k, Q, Q), dtype=torch.float64, device=dev)
    t_all = torch.zeros((iterations + 1, B, k, k), dtype=torch.float64, device=dev)
    b_all[0].copy_(torch.from_numpy(coef))
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
        engine.batch_vreg_stats_device(stats, obs)
        if exact:
            engine.batch_exact_evidence_device(ev_exact[it], dead)
        else:
            engine.batch_summaries_device(ev[it])
        with torch.cuda.stream(stream):                     # (the next tables start as these: a copy on the engine's stream)
            b_all[it + 1].copy_(b_all[it])
            c_all[it + 1].copy_(c_all[it])
            t_all[it + 1].copy_(t_all[it])
        engine.batch_mstep_vreg_device(stats, b_all[it + 1], c_all[it + 1], t_all[it + 1], floor)
        if it + 1 < iterations:
            engine.batch_retable_vreg_device(b_all[it + 1], c_all[it + 1], t_all[it + 1], obs)
    engine.sync()
    ev_host = np.ascontiguousarray((ev_exact if exact else ev[:, :, 0]).cpu().numpy())
    return b_all.cpu().numpy(), c_all.cpu().numpy(), t_all.cpu().numpy(), ev_host
