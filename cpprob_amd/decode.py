"""Labelling sequences with their most probable state paths (Engine.batch_decode): the step that follows a fit of the tables
(cpprob_amd.em.hmm_table_em).  One call begins a batch of MODEL_HMM_TABLE problems under the given tables, runs it and decodes it.
The per-step argmax of the smoothed marginals is another estimator, and may name a sequence the transition table forbids."""
import numpy as np

from .capi import MODEL_HMM_TABLE, RESAMPLE_SYSTEMATIC


def hmm_table_decode(engine, observes, means, trans, n_particles, seeds, resampler=RESAMPLE_SYSTEMATIC, keep_history=True, lag=None, sigmas=None, emission="normal"):
    """observes: a list of B 1-D sequences, or one sequence every problem shares (one sequence under B tables); means [B, k],
    trans [B, k, k] the tables (hmm_table_em's last ones, say); seeds [B].  Returns (paths, scores, log_evidence): paths a list of
    int32 [T_b] arrays, the most probable state sequence over the states the particles occupy; scores float64 [B], the log joint
    density of path and observes; log_evidence [B], the run's estimate.  lag: an int -- the paths are the fixed-lag rows instead
    (Engine.batch_decode_lag: the state at t of the best path of steps 0 .. t + lag), what a stream would have labelled with that
    delay.  keep_history=False: the batch is filtering-only and keeps the smoother's masses (keep_masses) -- the same arrays bit
    for bit, without a particle store.  sigmas [B, k]: the tables' per-state emission scales (hmm_table_em's fourth array).
    emission="poisson": means are the rates of Poisson emissions and the observes counts."""
    if emission == "poisson" and sigmas is not None:
        raise ValueError("a Poisson emission has no scales: a table is unit, scaled or Poisson")
    means = np.array(means, np.float64)
    trans = np.array(trans, np.float64)
    if means.ndim != 2 or trans.shape != (means.shape[0], means.shape[1], means.shape[1]):
        raise ValueError("means [B, k], trans [B, k, k]")
    B = means.shape[0]
    if isinstance(observes, np.ndarray) and observes.ndim == 1:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    if lag is not None and int(lag) < 0:
        raise ValueError("lag must be at least 0")
    sd = np.ascontiguousarray(seeds, np.uint64)
    tables = (means, trans) if sigmas is None else (means, trans, np.array(sigmas, np.float64))
    engine.batch_begin_problems(MODEL_HMM_TABLE, seqs, n_particles, tables=tables, resampler=resampler, keep_history=bool(keep_history),
                                keep_masses=not keep_history, emission=emission)
    engine.batch_run(sd)
    if lag is None:
        paths, scores = engine.batch_decode()
    else:
        states, scores = engine.batch_decode_lag(int(lag))
        paths = [states[b, :len(seqs[b])].copy() for b in range(B)]
    ev = np.array([s["log_evidence"] for s in engine.batch_results()[0]])
    return paths, scores, ev
