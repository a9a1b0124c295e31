"""EM for Markov-switching regressions: MODEL_HMM_TABLE problems whose state s emits y_t ~ N(coef[s] . x_t, sigma[s]) on covariates x_t
known at the step (csrc/batch_reg.hpp).  A table is the coefficients [k, P] (k <= 8 states, P <= 15 covariates), the sigmas [k] and
the transition rows [k, k]; the initial state is uniform and not fitted; an intercept is a covariate column of ones.  The
autoregressive HMM is the case x_t = (1, y_{t-1}, .., y_{t-p}): ar_design builds its observes.  The E-step is Engine.batch_reg_stats
-- the full family's record over z_t = (y_t, x_t) --, the M-step below solves every state's normal equations on the host, or the
device does."""
import numpy as np

from .capi import FULL_STATS_PER_PROBLEM, REG_MAX_COV, RESAMPLE_SYSTEMATIC


def _check_floor(sigma_floor):
    floor = np.float64(sigma_floor)
    if not (floor > 0.0) or not np.isfinite(floor):
        raise ValueError("sigma_floor must be finite and > 0")
    return floor


def _tables(coef, sigmas, trans):
    coef, sigmas, trans = np.array(coef, np.float64), np.array(sigmas, np.float64), np.array(trans, np.float64)
    if coef.ndim != 3 or sigmas.shape != coef.shape[:2] or trans.shape != (coef.shape[0], coef.shape[1], coef.shape[1]):
        raise ValueError("coef [B, k, P], sigmas [B, k] and trans [B, k, k]")
    if not 1 <= coef.shape[2] <= REG_MAX_COV:
        raise ValueError("P, the covariates of a step, must lie in 1 .. 15")
    return coef, sigmas, trans


def ar_design(y, p, intercept=True):
    """The observes [T - p, 1 + P] of an AR(p) HMM over the series y [T]: row t holds (y_{t+p}, 1.0 if intercept, y_{t+p-1}, ..,
    y_t), so P = p + 1 with the intercept and p without."""
    y, p = np.ascontiguousarray(y, np.float64).reshape(-1), int(p)
    if p < 0 or p + bool(intercept) < 1 or p + bool(intercept) > REG_MAX_COV or len(y) < p:
        raise ValueError("p + intercept must lie in 1 .. 15, and y hold at least p values")
    n = len(y) - p
    cols = [y[p:]] + ([np.ones(n)] if intercept else []) + [y[p - 1 - i:p - 1 - i + n] for i in range(p)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def solve(A, b):
    """reg_mstep's solve on N systems at once: A [N, P, P] (the lower triangles read), b [N, P].  Returns (beta [N, P], ok [N]); every
    entry takes the device's operations in the device's order, one numpy operation each."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    N, P = b.shape
    W, L, d, ok = np.zeros((N, P, P)), np.zeros((N, P, P)), np.ones((N, P)), np.isfinite(b).all(axis=1)
    with np.errstate(all="ignore"):
        for j in range(P):
            for i in range(j, P):
                a = A[:, i, j].copy()
                ok &= np.isfinite(a)
                for p in range(j):
                    a = a - W[:, i, p] * L[:, j, p]
                if i == j:
                    ok &= (a > 0.0) & (a < np.inf)
                    d[:, j] = a
                else:
                    W[:, i, j] = a
                    L[:, i, j] = a / d[:, j]
        beta = b.copy()
        for i in range(P):
            for p in range(i):
                beta[:, i] = beta[:, i] - L[:, i, p] * beta[:, p]
        for i in range(P):
            beta[:, i] = beta[:, i] / d[:, i]
        for p in range(P - 1, 0, -1):
            for i in range(p):
                beta[:, i] = beta[:, i] - L[:, p, i] * beta[:, p]
    return beta, ok & np.isfinite(beta).all(axis=1)


def m_step_reg(stats, coef, sigmas, trans, sigma_floor=1e-3):
    """The tables that maximise the expected complete-data log-likelihood under `stats` (a dict as Engine.batch_reg_stats returns: xi
    [B, 8, 8], occ [B, 8], syy [B, 8, 16, 16] over z = (y, x)): trans[b, s, :] = xi[b, s, :k] / its sum; for a state with occ > 0,
    coef solves (sum g x x^T) beta = sum g x y and sigma = sqrt(sum g y y / occ - sum over i of beta_i (sum g x_i y / occ)), not below
    sigma_floor (a NaN takes it too).  A state whose system does not solve (csrc/batch_reg.hpp: a pivot not > 0, anything not finite)
    keeps coefficients and sigma, as a state without mass; a transition row without mass stays too.  Pure numpy; returns new (coef
    [B, k, P], sigmas [B, k], trans [B, k, k]).  The statements of csrc/batch_reg.hpp, which cpprob_hip_batch_mstep_reg_device runs
    bit for bit."""
    floor = _check_floor(sigma_floor)
    coef, sigmas, trans = _tables(coef, sigmas, trans)
    B, k, P = coef.shape
    xi = np.asarray(stats["xi"], np.float64)[:, :k, :k]
    occ = np.asarray(stats["occ"], np.float64)[:, :k]
    syy = np.asarray(stats["syy"], np.float64)[:, :k, :1 + P, :1 + P]
    row = np.zeros((B, k))
    for j in range(k):                                      # (sequential: the device's order of additions)
        row = row + xi[:, :, j]
    with np.errstate(all="ignore"):
        fit = row > 0.0
        trans[fit] = xi[fit] / row[fit][:, None]
        seen = (occ > 0.0) & (occ < np.inf)
        mass, c0, b = occ[seen], syy[seen][:, 0, 0], syy[seen][:, 1:, 0]
        beta, ok = solve(syy[seen][:, 1:, 1:], b)
        ok &= np.isfinite(c0)
        v = c0 / mass
        for i in range(P):
            v = v - beta[:, i] * (b[:, i] / mass)
        sg = np.where(v >= floor * floor, np.sqrt(v), floor)
        new_c, new_s = coef[seen], sigmas[seen]
        new_c[ok], new_s[ok] = beta[ok], sg[ok]
        coef[seen], sigmas[seen] = new_c, new_s
    return coef, sigmas, trans


def hmm_reg_em(engine, observes, coef0, sigmas0, trans0, n_particles, seeds, iterations, exact=False, resident=False, sigma_floor=1e-3,
               resampler=RESAMPLE_SYSTEMATIC):
    """Batched EM for Markov-switching regressions.  observes: a list of B arrays [T_b, 1 + P] (column 0 the response, then the
    covariates), or one such array every problem shares; coef0 [B, k, P], sigmas0 [B, k], trans0 [B, k, k] the initial tables; seeds
    [B].  One batch_begin_problems_reg (filtering-only, keeping the smoother's masses); iteration i runs the batch with seeds + i --
    exact=True: Engine.batch_run_exact, and the fit is Baum-Welch up to that run's quantisations; n_particles and seeds are then not
    used --, takes batch_reg_stats and the M-step, and re-tables the batch where it stands.  Returns (coef [iterations + 1, B, k, P],
    sigmas [iterations + 1, B, k], trans [iterations + 1, B, k, k], log_evidence [iterations, B]): the tables before every iteration
    and after the last, and every run's log-evidence of the tables it ran with.  resident=True: the loop is enqueued on the engine's
    stream -- batch_reg_stats_device, batch_mstep_reg_device and batch_retable_reg_device on tensors that stay on the device -- and
    read once after it; the same arrays bit for bit."""
    floor = float(_check_floor(sigma_floor))
    coef, sigmas, trans = _tables(coef0, sigmas0, trans0)
    B, P = coef.shape[0], coef.shape[2]
    if isinstance(observes, np.ndarray) and observes.ndim == 2:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1, 1 + P) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    iterations = int(iterations)
    c_hist, s_hist, t_hist, ev = [coef.copy()], [sigmas.copy()], [trans.copy()], np.zeros((iterations, B))
    if iterations == 0:
        return np.array(c_hist), np.array(s_hist), np.array(t_hist), ev
    engine.batch_begin_problems_reg(seqs, n_particles, coef, sigmas, trans, resampler=resampler, keep_history=False, keep_masses=True)
    if resident:
        return _em_resident(engine, seqs, coef, sigmas, trans, sd, iterations, bool(exact), floor)
    for it in range(iterations):
        if exact:
            engine.batch_run_exact()
        else:
            engine.batch_run(sd + np.uint64(it))
        stats = engine.batch_reg_stats(seqs)
        ev[it] = engine.batch_exact_evidence()[0] if exact else [s["log_evidence"] for s in engine.batch_results()[0]]
        coef, sigmas, trans = m_step_reg(stats, coef, sigmas, trans, floor)
        c_hist.append(coef.copy())
        s_hist.append(sigmas.copy())
        t_hist.append(trans.copy())
        if it + 1 < iterations:
            engine.batch_retable_reg(coef, sigmas, trans, seqs if it == 0 else None)
    return np.array(c_hist), np.array(s_hist), np.array(t_hist), ev


def _em_resident(engine, seqs, coef, sigmas, trans, sd, iterations, exact, floor):
    """hmm_reg_em's loop on the begun batch with the tables, the observes, the records and the evidences in device tensors; the host
    enqueues and looks at nothing until the loop is over."""
    import torch
    B, k, P = coef.shape
    dev = torch.device("cuda", engine.device)
    obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(seqs).reshape(-1))).to(dev)
    c_all = torch.zeros((iterations + 1, B, k, P), dtype=torch.float64, device=dev)
    s_all = torch.zeros((iterations + 1, B, k), dtype=torch.float64, device=dev)
    t_all = torch.zeros((iterations + 1, B, k, k), dtype=torch.float64, device=dev)
    c_all[0].copy_(torch.from_numpy(coef))
    s_all[0].copy_(torch.from_numpy(sigmas))
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
        engine.batch_reg_stats_device(stats, obs)
        if exact:
            engine.batch_exact_evidence_device(ev_exact[it], dead)
        else:
            engine.batch_summaries_device(ev[it])
        with torch.cuda.stream(stream):                     # (the next tables start as these: a copy on the engine's stream)
            c_all[it + 1].copy_(c_all[it])
            s_all[it + 1].copy_(s_all[it])
            t_all[it + 1].copy_(t_all[it])
        engine.batch_mstep_reg_device(stats, c_all[it + 1], s_all[it + 1], t_all[it + 1], floor)
        if it + 1 < iterations:
            engine.batch_retable_reg_device(c_all[it + 1], s_all[it + 1], t_all[it + 1], obs)
    engine.sync()
    ev_host = np.ascontiguousarray((ev_exact if exact else ev[:, :, 0]).cpu().numpy())
    return c_all.cpu().numpy(), s_all.cpu().numpy(), t_all.cpu().numpy(), ev_host
