"""A batched Gibbs sampler for the tables of MODEL_HMM_TABLE problems, the Bayesian counterpart of cpprob_amd.em: one chain a problem.
A sweep draws one state trajectory a chain on the device and reads only its complete-data sufficient statistics
(Engine.batch_traj_stats, 88 doubles a chain); the tables are then drawn on the host from their conjugate posteriors.  A table is
its means and its transition rows and, where the caller passes them, its per-state emission scales (without them the emission's
sigma is 1 and stays so); the initial state is uniform and not sampled.  The emission is Gaussian: for emission="poisson" every
sampler here raises NotImplementedError (poisson_refusal) -- the rates have no conjugate draw here yet."""
import numpy as np

from .capi import MODEL_HMM_TABLE, RESAMPLE_SYSTEMATIC


def poisson_refusal(emission):
    """The samplers' answer to an emission family: nothing for "normal", a clear error for "poisson"."""
    if emission == "poisson":
        raise NotImplementedError('the Gibbs samplers draw the tables of Gaussian emissions: emission="poisson" has no conjugate (gamma) draw of '
                                  "the rates yet -- fit Poisson tables with cpprob_amd.em.hmm_table_em")
    if emission != "normal":
        raise ValueError('emission is "normal" or "poisson"')


def sample_tables(stats, k, rng, alpha=1.0, mu0=0.0, tau0=10.0, sigmas=None, a0=2.0, b0=1.0, emission="normal"):
    """One draw of the tables given one trajectory's statistics a problem (`stats`: the dict Engine.batch_traj_stats returns with the
    trajectory axis indexed away -- xi [B, 8, 8], occ, occ_y [B, 8]).  Priors: every transition row Dirichlet(alpha, .., alpha), every
    mean N(mu0, tau0^2); sigma is 1 as the model fixes it, so both posteriors are conjugate:
      G = rng.standard_gamma(alpha + xi[:, :k, :k]) (one call), trans = G / G.sum(-1, keepdims=True)
      z = rng.standard_normal((B, k)) (one call, after G), prec = 1 / tau0^2 + occ[:, :k],
      means = (mu0 / tau0^2 + occ_y[:, :k]) / prec + z / sqrt(prec)
    Pure numpy; returns (means [B, k], trans [B, k, k]).
    sigmas [B, k] (the current emission scales): the mean's posterior uses them -- prec = 1 / tau0^2 + occ / sigma^2, means =
    (mu0 / tau0^2 + occ_y / sigma^2) / prec + z / sqrt(prec) -- and every state's variance is drawn from its conjugate posterior under
    an inverse-gamma(a0, b0) prior at the mean just drawn: shape = a0 + occ / 2, rate = b0 + (occ_yy - 2 mu occ_y + mu^2 occ) / 2,
    variance = rate / rng.standard_gamma(shape) (one call, after the draws above: a call without sigmas consumes the generator as it
    did).  Returns (means, trans, sigmas [B, k])."""
    poisson_refusal(emission)
    k = int(k)
    xi, occ, occ_y = (np.asarray(stats[f], np.float64) for f in ("xi", "occ", "occ_y"))
    if xi.ndim != 3 or occ.ndim != 2 or occ_y.ndim != 2 or not xi.shape[0] == occ.shape[0] == occ_y.shape[0]:
        raise ValueError("one record of statistics per problem: xi [B, 8, 8], occ and occ_y [B, 8]")
    xi, occ, occ_y = xi[:, :k, :k], occ[:, :k], occ_y[:, :k]
    G = rng.standard_gamma(alpha + xi)
    trans = G / G.sum(-1, keepdims=True)
    z = rng.standard_normal((xi.shape[0], k))
    if sigmas is None:
        prec = 1 / tau0**2 + occ
        means = (mu0 / tau0**2 + occ_y) / prec + z / np.sqrt(prec)
        return means, trans
    var = np.asarray(sigmas, np.float64) ** 2
    if var.shape != occ.shape:
        raise ValueError("sigmas [B, k]")
    occ_yy = np.asarray(stats["occ_yy"], np.float64)[:, :k]
    prec = 1 / tau0**2 + occ / var
    means = (mu0 / tau0**2 + occ_y / var) / prec + z / np.sqrt(prec)
    rate = b0 + (occ_yy - 2 * means * occ_y + means * means * occ) / 2
    return means, trans, np.sqrt(rate / rng.standard_gamma(a0 + occ / 2))


def draw_tables(one, k, rng, sigmas, tie, prior):
    """A sweep's draw of the tables from the chains' records `one` (trajectory axis indexed away).  tie: None, or
    em.check_tied_start's (groups, G, first members) -- the records are then pooled over each group (em.pool_stats, compact), one
    sample_tables call on the G records draws one table a group, so the generator is consumed at shape [G, ...], and the draw is
    expanded to the members.  Returns sample_tables' tuple at shape [B, ...]."""
    if tie is None:
        return sample_tables(one, k, rng, **prior) if sigmas is None else sample_tables(one, k, rng, sigmas=sigmas, **prior)
    from .em import pool_stats
    groups, _, lead = tie
    pooled = pool_stats(one, groups, broadcast=False)
    drawn = sample_tables(pooled, k, rng, **prior) if sigmas is None else sample_tables(pooled, k, rng, sigmas=sigmas[lead], **prior)
    return tuple(a[groups] for a in drawn)


def hmm_table_gibbs(engine, observes, means0, trans0, n_particles, seeds, sweeps, rng, resampler=RESAMPLE_SYSTEMATIC, keep_history=True, retable=False, sigmas0=None,
                    groups=None, **prior):
    """Batched Gibbs sampling of the tables, one chain a problem.  observes: a list of B 1-D sequences, or one sequence every chain
    shares; means0 [B, k], trans0 [B, k, k] the chains' initial tables; seeds [B]; rng a numpy Generator; prior: sample_tables' alpha,
    mu0, tau0.  Sweep i begins a batch with the current tables (batch_begin_problems), runs it with seeds + i, takes the statistics of
    one backward-simulated trajectory a chain (batch_traj_stats(1, draw_index=i % 2^16, observes)) and draws the next tables with
    sample_tables.  Returns (means [sweeps + 1, B, k], trans [sweeps + 1, B, k, k], log_evidence [sweeps, B]): the tables before every
    sweep and after the last, and the log-evidence estimate of every sweep's run (of the tables it began with).  keep_history=False:
    the batches are filtering-only and keep the smoother's masses (keep_masses) -- the same chain bit for bit, without a particle store.
    retable=True: sweep 0 begins the batch; every later sweep gives it its new tables where it stands (batch_retable: the tables drawn
    on the host, the observes uploaded once) in place of a fresh begin -- the same chain bit for bit.

    The trajectory comes from the particle approximation of forward filtering / backward sampling: it is drawn from the n_particles
    filtering approximations of the run, not from the exact smoothing law.  The chain's invariant law is therefore the posterior only
    up to the particle filter's error in n_particles (it vanishes as n_particles grows).  This is NOT a particle-Gibbs kernel with a
    retained path (conditional SMC): nothing here corrects that error at finite n_particles.

    sigmas0 [B, k]: the chains carry per-state emission scales, sampled with the rest (sample_tables with sigmas; prior: its a0, b0);
    a fourth array, sigmas [sweeps + 1, B, k], is returned behind the three.

    groups int [B]: tied tables -- the chains of a group share one table, drawn from the posterior given all of their trajectories
    (draw_tables: the sweep's records pooled over each group, G tables drawn, expanded to the members).  The members' initial tables
    must be equal bit for bit (ValueError naming the group); every member keeps its own trajectory; the returned shapes stay, with
    and without retable=True."""
    poisson_refusal(prior.pop("emission", "normal"))
    means = np.array(means0, np.float64)
    trans = np.array(trans0, np.float64)
    B, k = means.shape
    if isinstance(observes, np.ndarray) and observes.ndim == 1:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    sigmas = None if sigmas0 is None else np.array(sigmas0, np.float64)
    tie = None
    if groups is not None:
        from .em import check_tied_start
        tie = check_tied_start(groups, means, trans, sigmas)
    m_hist, t_hist, ev = [means.copy()], [trans.copy()], np.zeros((int(sweeps), B))
    s_hist = None if sigmas is None else [sigmas.copy()]
    for i in range(int(sweeps)):
        tables = (means, trans) if sigmas is None else (means, trans, sigmas)
        if retable and i > 0:
            engine.batch_retable(tables, seqs if i == 1 else None)
        else:
            engine.batch_begin_problems(MODEL_HMM_TABLE, seqs, n_particles, tables=tables, resampler=resampler, keep_history=bool(keep_history),
                                        keep_masses=not keep_history)
        engine.batch_run(sd + np.uint64(i))
        stats = engine.batch_traj_stats(1, draw_index=i % (1 << 16), observes=seqs)
        ev[i] = [s["log_evidence"] for s in engine.batch_results()[0]]
        one = {name: v[:, 0] for name, v in stats.items()}
        if sigmas is None:
            means, trans = draw_tables(one, k, rng, None, tie, prior)
        else:
            means, trans, sigmas = draw_tables(one, k, rng, sigmas, tie, prior)
            s_hist.append(sigmas.copy())
        m_hist.append(means.copy())
        t_hist.append(trans.copy())
    if sigmas is None:
        return np.array(m_hist), np.array(t_hist), ev
    return np.array(m_hist), np.array(t_hist), ev, np.array(s_hist)
