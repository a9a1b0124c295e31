"""Particle Gibbs with backward sampling for the tables of MODEL_HMM_TABLE problems, one chain a problem: cpprob_amd.gibbs' sweep with
the particle filter replaced by a conditional one.  From the second sweep on the run is a conditional SMC run
(Engine.batch_run_conditional_device) whose retained particle follows the trajectory the previous sweep drew; the trajectory stays on
the device, in one of two buffers, and only its complete-data sufficient statistics (88 doubles a chain) reach the host."""
import numpy as np

from .capi import MODEL_HMM_TABLE, batch_smooth_layout
from .gibbs import draw_tables


def hmm_table_particle_gibbs(engine, observes, means0, trans0, n_particles, seeds, sweeps, rng, **prior):
    """Batched particle Gibbs sampling of the tables, one chain a problem.  observes: a list of B 1-D sequences, or one sequence every
    chain shares; means0 [B, k], trans0 [B, k, k] the chains' initial tables; seeds [B]; rng a numpy Generator; prior: sample_tables'
    alpha, mu0, tau0.  Sweep i begins a filtering-only batch that keeps its masses with the current tables
    (batch_begin_problems(keep_history=False, keep_masses=True)) and runs it -- sweep 0 with batch_run(seeds), sweep i >= 1 with
    batch_run_conditional_device(seeds + i, the previous sweep's trajectory) --, draws one backward-simulated trajectory a chain into the
    other of two device buffers (batch_smooth_device(traj_i8=..., n_traj=1, draw_index=i % 2^16)), takes that trajectory's statistics
    (batch_traj_stats(1, draw_index=i % 2^16, observes): the same trajectory) and draws the next tables with sample_tables.  No
    trajectory crosses to the host.  Returns (means [sweeps + 1, B, k], trans [sweeps + 1, B, k, k]): the tables before every sweep
    and after the last.  retable=True (a keyword beside the prior's, default False): sweep 0 begins the batch; every later sweep gives it its new tables where it stands
    (batch_retable: the tables drawn on the host, the observes uploaded once) in place of a fresh begin -- the same chain bit for bit.
    sigmas0 [B, k] (a keyword likewise, default None): the chains carry per-state emission scales, sampled with the rest
    (sample_tables with sigmas; prior: its a0, b0), and a third array, sigmas [sweeps + 1, B, k], is returned behind the two.
    groups int [B] (a keyword likewise, default None): tied tables -- the chains of a group share one table, drawn given all of
    their trajectories (gibbs.draw_tables); the members' initial tables must be equal bit for bit (ValueError naming the group), and
    every member keeps its own trajectory and its own retained path.

    This is particle Gibbs with backward sampling: a conditional SMC run with multinomial resampling, its retained particle the
    previous trajectory, followed by backward simulation.  That kernel leaves the smoothing law of the states given the tables
    invariant whatever the number of particles, so the posterior of tables and states is the chain's invariant law at every
    n_particles >= 1, up to the 32-bit quantisation of weights and thresholds; n_particles moves how fast the chain mixes, not where
    it settles.  (hmm_table_gibbs draws its trajectory from an unconditional filter and is exact only as n_particles grows.)"""
    import torch
    from .gibbs import poisson_refusal
    poisson_refusal(prior.pop("emission", "normal"))
    retable = bool(prior.pop("retable", False))
    sigmas0 = prior.pop("sigmas0", None)
    groups = prior.pop("groups", None)
    sigmas = None if sigmas0 is None else np.array(sigmas0, np.float64)
    s_hist = None if sigmas is None else [sigmas.copy()]
    means = np.array(means0, np.float64)
    trans = np.array(trans0, np.float64)
    B, k = means.shape
    if isinstance(observes, np.ndarray) and observes.ndim == 1:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    tie = None
    if groups is not None:
        from .em import check_tied_start
        tie = check_tied_start(groups, means, trans, sigmas)
    total = int(batch_smooth_layout([len(o) for o in seqs], 1)[-1])
    traj = [torch.empty(total, dtype=torch.int8, device="cuda:%d" % engine.device) for _ in range(2)]
    m_hist, t_hist = [means.copy()], [trans.copy()]
    for i in range(int(sweeps)):
        tables = (means, trans) if sigmas is None else (means, trans, sigmas)
        if retable and i > 0:
            engine.batch_retable(tables, seqs if i == 1 else None)
        else:
            engine.batch_begin_problems(MODEL_HMM_TABLE, seqs, n_particles, tables=tables, keep_history=False, keep_masses=True)
        if i == 0:
            engine.batch_run(sd)
        else:
            engine.batch_run_conditional_device(sd + np.uint64(i), traj[(i - 1) & 1])
        engine.batch_smooth_device(traj_i8=traj[i & 1], n_traj=1, draw_index=i % (1 << 16))
        stats = engine.batch_traj_stats(1, draw_index=i % (1 << 16), observes=seqs)
        one = {name: v[:, 0] for name, v in stats.items()}
        if sigmas is None:
            means, trans = draw_tables(one, k, rng, None, tie, prior)
        else:
            means, trans, sigmas = draw_tables(one, k, rng, sigmas, tie, prior)
            s_hist.append(sigmas.copy())
        m_hist.append(means.copy())
        t_hist.append(trans.copy())
    if sigmas is None:
        return np.array(m_hist), np.array(t_hist)
    return np.array(m_hist), np.array(t_hist), np.array(s_hist)
