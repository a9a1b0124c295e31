"""Online EM for the tables of MODEL_HMM_TABLE streams (Cappe 2011, Alg. 1, in its stochastic-approximation form): an online batch
learns its tables on the device while its observes arrive.  Every step discounts the running statistics by 1 - gamma[t] and adds the
new ones with weight gamma[t]; after every advance the M-step on the running record gives the tables the next observes are filtered
under (Engine.batch_advance_learn; include/cpprob_hip.h: cpprob_hip_batch_advance_learn).  The emission's sigma is 1 unless the
caller passes per-state scales, which are then learned with the rest.  With `groups` the streams of a group learn one table
(tied online EM; include/cpprob_hip.h: cpprob_hip_batch_learn_tie)."""
import math

import numpy as np

from .capi import MODEL_HMM_TABLE, RESAMPLE_SYSTEMATIC


def step_sizes(n, step_exponent=0.6):
    """gamma[t] = pow(t + 1, -step_exponent), t = 0 .. n - 1, evaluated on the host with the C library's pow (as the C++ stream
    evaluates them): the device reads these doubles."""
    return np.array([math.pow(t + 1.0, -float(step_exponent)) for t in range(int(n))], np.float64)


def hmm_table_online_em(engine, observes, tables0, n_particles, seeds, chunk, step_exponent=0.6, t_min=20, keep_history=False, resampler=RESAMPLE_SYSTEMATIC,
                        sigma_floor=1e-3, groups=None):
    """observes: a list of B 1-D sequences (the streams; their lengths are the capacities), or one sequence every problem shares;
    tables0 = (means [B, k], transition [B, k, k]), the tables the streams start under; seeds [B].  The streams are fed `chunk`
    observes at a time; t_min: the length a stream must have reached before its first M-step (the chunk is the update period
    afterwards).  keep_history=False: a filtering-only batch that keeps its masses.
    Returns (means [A + 1, B, k], trans [A + 1, B, k, k], status [A, B], summaries): the tables before the first advance and after
    each of the A advances, the status words after each (0, or the bits of a dropped M-step), and the summaries of the finished
    streams -- log_evidence is the prequential likelihood under the tables in force at each step.
    tables0 = (means, transition, sigmas [B, k]): the streams carry per-state emission scales and learn them too, none below
    sigma_floor; a fifth element, sigmas [A + 1, B, k], is returned behind the four.
    groups (int [B], ids 0 .. G-1, every one used): tied online EM -- the streams of a group learn one table from their pooled records,
    every stream weighing equally whatever its length; t_min then counts the observes the group has seen, and tables0 must be equal
    within a group (ValueError).  The shapes returned are unchanged: the members of a group hold equal rows."""
    if len(tables0) not in (2, 3):
        raise ValueError("tables0 = (means, transition) or (means, transition, sigmas)")
    means = np.array(tables0[0], np.float64)
    trans = np.array(tables0[1], np.float64)
    sigmas = np.array(tables0[2], np.float64) if len(tables0) == 3 else None
    B = means.shape[0]
    if isinstance(observes, np.ndarray) and observes.ndim == 1:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    if groups is not None:
        groups = np.ascontiguousarray(groups, np.int32).reshape(-1)
        if groups.size != B:
            raise ValueError("groups holds one id per table")
        lead = {}
        for b, g in enumerate(groups.tolist()):
            a = lead.setdefault(g, b)
            for name, x in (("means", means), ("transition rows", trans), ("sigmas", sigmas)):
                if x is not None and not np.array_equal(x[a].view(np.uint64), x[b].view(np.uint64)):
                    raise ValueError("group %d: the initial %s of problem %d differ from those of problem %d; a group's members start from one table" % (g, name, b, a))
    caps = np.array([max(1, len(o)) for o in seqs], np.uint32)
    tables = (means, trans) if sigmas is None else (means, trans, sigmas)
    engine.batch_begin_online(MODEL_HMM_TABLE, caps, n_particles, np.ascontiguousarray(seeds, np.uint64), tables=tables, resampler=resampler,
                              keep_history=bool(keep_history), keep_masses=not keep_history)
    if groups is not None:
        engine.batch_tie(groups)
    engine.batch_learn_begin(step_sizes(int(caps.max()), step_exponent), t_min, sigma_floor=None if sigmas is None else sigma_floor, tied=groups is not None)
    m_hist, t_hist, st_hist = [means.copy()], [trans.copy()], []
    s_hist = None if sigmas is None else [sigmas.copy()]
    top = max(len(o) for o in seqs)
    for at in range(0, top, chunk):
        engine.batch_advance_learn([o[at:at + chunk] for o in seqs])
        if sigmas is None:
            m, t, st = engine.batch_learn_tables(means.shape[1])
        else:
            m, t, sg, st = engine.batch_learn_tables(means.shape[1], scales=True)
            s_hist.append(sg)
        m_hist.append(m)
        t_hist.append(t)
        st_hist.append(st)
    out = (np.array(m_hist), np.array(t_hist), np.array(st_hist, np.int32).reshape(len(st_hist), B), engine.batch_results(with_stats=False)[0])
    return out if sigmas is None else out + (np.array(s_hist),)
