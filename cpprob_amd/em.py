"""Particle EM for the tables of MODEL_HMM_TABLE problems: the E-step is Engine.batch_smooth_stats (the backward smoother's expected
sufficient statistics, one record a problem, computed on the device), the M-step below is 88 doubles a problem on the host.  A
table is its means and its transition rows and, where the caller passes them, its per-state emission scales (without them the
emission's sigma is 1 and stays so); with emission="poisson" the means are the rates of Poisson emissions (csrc/batch_poisson.hpp);
the initial state is uniform and not fitted.  Problems may be tied (groups): the problems of a
group share one table, fitted to their pooled records (pool_stats; on the device cpprob_hip_batch_pool_stats)."""
import numpy as np

from .capi import MODEL_HMM_TABLE, RESAMPLE_SYSTEMATIC, STATS_PER_PROBLEM


def m_step(stats, means, trans, sigmas=None, sigma_floor=1e-3, emission="normal", rate_floor=1e-6):
    """The tables that maximise the expected complete-data log-likelihood under `stats` (a dict as Engine.batch_smooth_stats returns:
    xi [B, 8, 8], occ, occ_y [B, 8]): trans[b, s, :] = xi[b, s, :k] / its sum, means[b, s] = occ_y[b, s] / occ[b, s], k =
    means.shape[1].  A transition row or a state with no mass keeps its previous value; states >= k of the statistics are not read.
    Pure numpy; returns new (means [B, k], trans [B, k, k]).
    sigmas [B, k]: the emission scales are fitted too, and returned as a third array -- a state with mass takes v = occ_yy / occ -
    mean' mean' (mean' its new mean) and sigma' = sqrt(v) where v >= sigma_floor^2, else sigma_floor (a NaN v too); a state without
    mass keeps its sigma.  The statements of csrc/batch_scale.hpp, which cpprob_hip_batch_mstep_scaled_device runs bit for bit.
    emission="poisson": means are the rates of Poisson emissions; a state with mass takes occ_y / occ where that is >= rate_floor,
    else rate_floor (a NaN too), a state without mass keeps its rate.  The statements of csrc/batch_poisson.hpp, which
    cpprob_hip_batch_mstep_poisson_device runs bit for bit."""
    if emission not in ("normal", "poisson"):
        raise ValueError('emission is "normal" or "poisson"')
    if emission == "poisson" and sigmas is not None:
        raise ValueError("a Poisson emission has no scales: a table is unit, scaled or Poisson")
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
    if emission == "poisson":
        floor = np.float64(rate_floor)
        if not (floor > 0.0) or not np.isfinite(floor):
            raise ValueError("rate_floor must be finite and > 0")
        with np.errstate(all="ignore"):
            means[seen] = np.where(means[seen] >= floor, means[seen], floor)
        return means, trans
    if sigmas is None:
        return means, trans
    sigmas = np.array(sigmas, np.float64)
    if sigmas.shape != means.shape:
        raise ValueError("sigmas [B, k]")
    floor = np.float64(sigma_floor)
    if not (floor > 0.0) or not np.isfinite(floor):
        raise ValueError("sigma_floor must be finite and > 0")
    occ_yy = np.asarray(stats["occ_yy"], np.float64)[:, :k]
    with np.errstate(all="ignore"):
        v = occ_yy[seen] / occ[seen]
        v = v - means[seen] * means[seen]
        root = np.sqrt(np.where(v >= floor * floor, v, 1.0))
    sigmas[seen] = np.where(v >= floor * floor, root, floor)
    return means, trans, sigmas


def tie_groups(groups, n_problems):
    """groups as an int32 array [n_problems] with the number of groups G: the ids are integers in 0 .. G-1, G the largest + 1, and every
    id occurs (what cpprob_hip_batch_tie takes); ValueError otherwise."""
    g = np.asarray(groups)
    if g.ndim != 1 or g.shape[0] != int(n_problems) or g.shape[0] == 0 or g.dtype.kind not in "iu":
        raise ValueError("groups: one integer group id per problem, [%d]" % int(n_problems))
    if int(g.min()) < 0:
        raise ValueError("groups: a group id is negative")
    G = int(g.max()) + 1
    if G > g.shape[0] or np.unique(g).size != G:
        raise ValueError("groups: every id in 0 .. %d must occur" % (G - 1))
    return np.ascontiguousarray(g, np.int32), G


def pool_stats(stats, groups, broadcast=True):
    """The pooled sufficient statistics of tied problems, the statement cpprob_hip_batch_pool_stats is held to.  stats: the dict of
    Engine.batch_smooth_stats (arrays [B, ...]) or Engine.batch_traj_stats ([B, n_traj, ...]), or a raw array of records [B, 88] or
    [B, R, 88]; groups: int [B], problem b's group (tie_groups).  For a group with the members b_0 < b_1 < ..., every entry is
    (((0.0 + rec[b_0]) + rec[b_1]) + ...): one addition a member, in ascending problem order, from 0.0.  broadcast=True: the shapes
    stay and every member holds its group's sum; broadcast=False: the leading axis is the group, [G, ...].  Pure numpy with an
    explicit loop over the members; returns new arrays."""
    if isinstance(stats, dict):
        return {name: pool_stats(v, groups, broadcast) for name, v in stats.items()}
    rec = np.asarray(stats, np.float64)
    if rec.ndim < 1:
        raise ValueError("records [B, ...]")
    g, G = tie_groups(groups, rec.shape[0])
    pooled = np.zeros((G,) + rec.shape[1:])
    for b in range(rec.shape[0]):                           # (ascending problem order: a group's members in theirs)
        pooled[g[b]] = pooled[g[b]] + rec[b]
    return pooled[g] if broadcast else pooled


def check_tied_start(groups, means, trans, sigmas=None):
    """A tied fit starts from one table a group: the members' means, transition rows and (where given) sigmas must be equal bit for
    bit.  Returns (groups int32 [B], G, the first member of every group [G]); ValueError naming the group otherwise."""
    g, G = tie_groups(groups, np.asarray(means).shape[0])
    lead = np.full(G, -1, np.int64)
    for b in range(g.shape[0] - 1, -1, -1):
        lead[g[b]] = b
    for name, arr in (("means", means), ("transition rows", trans), ("sigmas", sigmas)):
        if arr is None:
            continue
        a = np.ascontiguousarray(arr, np.float64).reshape(g.shape[0], -1).view(np.uint64)
        bad = np.nonzero((a != a[lead[g]]).any(axis=1))[0]
        if bad.size:
            raise ValueError("group %d: the initial %s of problem %d differ from those of problem %d; a group's members start from one table"
                             % (int(g[bad[0]]), name, int(bad[0]), int(lead[g[bad[0]]])))
    return g, G, lead


def hmm_table_em(engine, observes, means0, trans0, n_particles, seeds, iterations, resampler=RESAMPLE_SYSTEMATIC, keep_history=True, resident=False,
                 sigmas0=None, sigma_floor=1e-3, groups=None, emission="normal", rate_floor=1e-6):
    """Batched particle EM.  observes: a list of B 1-D sequences, or one sequence every problem shares (restarts: one sequence under
    B initial tables); means0 [B, k], trans0 [B, k, k] the initial tables; seeds [B].  Iteration i begins a batch with the current
    tables (batch_begin_problems), runs it with seeds + i, takes the statistics and the M-step.  Returns (means [iterations + 1, B, k],
    trans [iterations + 1, B, k, k], log_evidence [iterations, B]): the tables before every iteration and after the last, and the
    log-evidence estimate of every iteration's run (of the tables it began with).  keep_history=False: the batches are filtering-only
    and keep the smoother's masses (keep_masses) -- the same arrays bit for bit, without a particle store.
    resident=True: one batch_begin_problems, then the whole loop is enqueued on the engine's stream -- per iteration batch_run,
    batch_smooth_stats_device, batch_summaries_device, batch_mstep_device and batch_retable_device on tensors that stay on the device
    -- and the tables of every iteration and the evidences are read once after it.  The same arrays bit for bit.
    sigmas0 [B, k]: the problems carry per-state emission scales, fitted with the rest (m_step with sigmas, none below sigma_floor); a
    fourth array, sigmas [iterations + 1, B, k], is returned behind the three.  Both routes, the same arrays bit for bit.
    groups int [B]: tied tables -- the problems of a group share one table, fitted to all of their sequences.  The members' initial
    tables must be equal bit for bit (ValueError naming the group).  The records of every iteration are pooled over each group in
    ascending problem order (pool_stats on the host route; resident: one Engine.batch_tie after the begin and one
    batch_pool_stats_device, in place, in front of the unchanged M-step), so the members hold bit-identical tables throughout.  The
    returned shapes stay: members repeat their group's table, log_evidence stays per problem (a group's log-likelihood is its
    members' sum).  Both routes, the same arrays bit for bit.
    emission="poisson": the observes are counts 0 .. 4095 and means0 [B, k] the initial rates of Poisson emissions, none fitted below
    rate_floor; the means returned are the rates.  Host loop and resident=True, untied and tied, the same arrays bit for bit."""
    if emission not in ("normal", "poisson"):
        raise ValueError('emission is "normal" or "poisson"')
    if emission == "poisson" and sigmas0 is not None:
        raise ValueError("a Poisson emission has no scales: a table is unit, scaled or Poisson")
    means = np.array(means0, np.float64)
    trans = np.array(trans0, np.float64)
    B = means.shape[0]
    if isinstance(observes, np.ndarray) and observes.ndim == 1:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    sigmas = None if sigmas0 is None else np.array(sigmas0, np.float64)
    if sigmas is not None and sigmas.shape != means.shape:
        raise ValueError("sigmas0 [B, k]")
    if groups is not None:
        groups = check_tied_start(groups, means, trans, sigmas)[0]
    if resident and int(iterations) > 0:
        return _em_resident(engine, seqs, means, trans, n_particles, sd, int(iterations), resampler, bool(keep_history), sigmas, float(sigma_floor), groups,
                            emission, float(rate_floor))
    m_hist, t_hist, ev = [means.copy()], [trans.copy()], np.zeros((int(iterations), B))
    s_hist = None if sigmas is None else [sigmas.copy()]
    for it in range(int(iterations)):
        tables = (means, trans) if sigmas is None else (means, trans, sigmas)
        engine.batch_begin_problems(MODEL_HMM_TABLE, seqs, n_particles, tables=tables, resampler=resampler, keep_history=bool(keep_history),
                                    keep_masses=not keep_history, emission=emission)
        engine.batch_run(sd + np.uint64(it))
        stats = engine.batch_smooth_stats(seqs)
        ev[it] = [s["log_evidence"] for s in engine.batch_results()[0]]
        if groups is not None:
            stats = pool_stats(stats, groups)
        if sigmas is None:
            means, trans = m_step(stats, means, trans, emission=emission, rate_floor=rate_floor)
        else:
            means, trans, sigmas = m_step(stats, means, trans, sigmas, sigma_floor)
            s_hist.append(sigmas.copy())
        m_hist.append(means.copy())
        t_hist.append(trans.copy())
    if sigmas is None:
        return np.array(m_hist), np.array(t_hist), ev
    return np.array(m_hist), np.array(t_hist), ev, np.array(s_hist)


def _em_resident(engine, seqs, means, trans, n_particles, sd, iterations, resampler, keep_history, sigmas=None, sigma_floor=1e-3, groups=None,
                 emission="normal", rate_floor=1e-6):
    """hmm_table_em's loop with the tables, the observes, the records and the evidences in device tensors; the host enqueues and
    looks at nothing until the loop is over."""
    import torch
    B, k = means.shape
    dev = torch.device("cuda", engine.device)
    tables = (means, trans) if sigmas is None else (means, trans, sigmas)
    engine.batch_begin_problems(MODEL_HMM_TABLE, seqs, n_particles, tables=tables, resampler=resampler, keep_history=keep_history, keep_masses=not keep_history,
                                emission=emission)
    if groups is not None:
        engine.batch_tie(groups)                            # (once: the re-tables keep it)
    obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(seqs))).to(dev)
    m_all = torch.zeros((iterations + 1, B, k), dtype=torch.float64, device=dev)
    t_all = torch.zeros((iterations + 1, B, k, k), dtype=torch.float64, device=dev)
    m_all[0].copy_(torch.from_numpy(means))
    t_all[0].copy_(torch.from_numpy(trans))
    s_all = None
    if sigmas is not None:
        s_all = torch.zeros((iterations + 1, B, k), dtype=torch.float64, device=dev)
        s_all[0].copy_(torch.from_numpy(sigmas))
    stats = torch.zeros((B, STATS_PER_PROBLEM), dtype=torch.float64, device=dev)
    ev = torch.zeros((iterations, B, 4), dtype=torch.float64, device=dev)
    torch.cuda.current_stream(dev).synchronize()            # (the engine's stream is not ordered behind torch's: the tensors are complete first)
    stream = torch.cuda.ExternalStream(engine.stream_ptr, device=dev)
    for it in range(iterations):
        engine.batch_run(sd + np.uint64(it))
        engine.batch_smooth_stats_device(stats, obs)
        if groups is not None:
            engine.batch_pool_stats_device(stats, stats)     # (in place: every member's record becomes its group's)
        engine.batch_summaries_device(ev[it])
        with torch.cuda.stream(stream):                     # (the next tables start as these: a copy on the engine's stream)
            m_all[it + 1].copy_(m_all[it])
            t_all[it + 1].copy_(t_all[it])
            if s_all is not None:
                s_all[it + 1].copy_(s_all[it])
        if s_all is None:
            engine.batch_mstep_device(stats, m_all[it + 1], t_all[it + 1], emission=emission, rate_floor=rate_floor)
        else:
            engine.batch_mstep_device(stats, m_all[it + 1], t_all[it + 1], sigmas=s_all[it + 1], sigma_floor=sigma_floor)
        if it + 1 < iterations:
            engine.batch_retable_device(m_all[it + 1], t_all[it + 1], obs, sigmas=None if s_all is None else s_all[it + 1], emission=emission)
    engine.sync()
    if s_all is None:
        return m_all.cpu().numpy(), t_all.cpu().numpy(), np.ascontiguousarray(ev[:, :, 0].cpu().numpy())
    return m_all.cpu().numpy(), t_all.cpu().numpy(), np.ascontiguousarray(ev[:, :, 0].cpu().numpy()), s_all.cpu().numpy()
