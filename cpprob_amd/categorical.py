"""EM for discrete HMMs: MODEL_HMM_TABLE problems whose states emit symbols of a finite alphabet (csrc/batch_categorical.hpp).  A table
is an emission matrix [k, V] (k <= 8 states, V <= 64 symbols) and the transition rows [k, k]; the initial state is uniform and not
fitted.  The E-step is Engine.batch_symbol_stats -- the backward smoother's record and, beside it, the expected visits of every state
at every symbol, one kernel on the device --, the M-step below is 600 doubles a problem on the host, or the device's own."""
import numpy as np

from .capi import RESAMPLE_SYSTEMATIC, SYMBOL_STATS_PER_PROBLEM

MIN_NORMAL = float.fromhex("0x1p-1022")


def _check_floor(prob_floor):
    floor = np.float64(prob_floor)
    if not (floor > 0.0) or not np.isfinite(floor) or not (floor >= MIN_NORMAL):
        raise ValueError("prob_floor must be > 0, finite and a normal number")
    return floor


def m_step_categorical(stats, emission, trans, prob_floor=1e-6):
    """The tables that maximise the expected complete-data log-likelihood under `stats` (a dict as Engine.batch_symbol_stats returns:
    xi [B, 8, 8], cnt [B, 8, 64]): trans[b, s, :] = xi[b, s, :k] / its sum; tot = cnt[b, s, 0] + ... + cnt[b, s, V-1], added
    ascending from 0.0, and emission[b, s, v] = cnt[b, s, v] / tot where that is >= prob_floor, else prob_floor (a NaN too).  A
    transition row or a state with no mass keeps its previous value.  A fitted row of the matrix may sum to as much as
    1 + 64 prob_floor: it is not renormalised.  Pure numpy; returns new (emission [B, k, V], trans [B, k, k]).  The statements of
    csrc/batch_categorical.hpp, which cpprob_hip_batch_mstep_categorical_device runs bit for bit."""
    floor = _check_floor(prob_floor)
    emission = np.array(emission, np.float64)
    trans = np.array(trans, np.float64)
    if emission.ndim != 3 or trans.shape != (emission.shape[0], emission.shape[1], emission.shape[1]):
        raise ValueError("emission [B, k, V] and trans [B, k, k]")
    B, k, V = emission.shape
    xi = np.asarray(stats["xi"], np.float64)[:, :k, :k]
    cnt = np.asarray(stats["cnt"], np.float64)[:, :k, :V]
    row = np.zeros((B, k))
    for j in range(k):                                      # (sequential: the device's order of additions)
        row = row + xi[:, :, j]
    tot = np.zeros((B, k))
    for v in range(V):
        tot = tot + cnt[:, :, v]
    with np.errstate(all="ignore"):
        fit = row > 0.0
        trans[fit] = xi[fit] / row[fit][:, None]
        seen = tot > 0.0
        p = cnt[seen] / tot[seen][:, None]
        emission[seen] = np.where(p >= floor, p, floor)
    return emission, trans


def hmm_categorical_em(engine, observes, emission0, trans0, n_particles, seeds, iterations, exact=False, resident=False, prob_floor=1e-6,
                       resampler=RESAMPLE_SYSTEMATIC):
    """Batched EM for discrete HMMs.  observes: a list of B 1-D sequences of symbol indices 0 .. V-1, or one sequence every problem
    shares; emission0 [B, k, V], trans0 [B, k, k] the initial tables; seeds [B].  One batch_begin_problems_categorical (filtering-only,
    keeping the smoother's masses); iteration i runs the batch with seeds + i -- exact=True: Engine.batch_run_exact, and the fit is
    Baum-Welch up to that run's quantisations; n_particles and seeds are then not used --, takes batch_symbol_stats and the M-step,
    and re-tables the batch where it stands.  Returns (emission [iterations + 1, B, k, V], trans [iterations + 1, B, k, k],
    log_evidence [iterations, B]): the tables before every iteration and after the last, and every run's log-evidence of the tables
    it ran with.  resident=True: the loop is enqueued on the engine's stream -- batch_symbol_stats_device,
    batch_mstep_categorical_device and batch_retable_categorical_device on tensors that stay on the device -- and read once after it;
    the same arrays bit for bit."""
    floor = float(_check_floor(prob_floor))
    emission = np.array(emission0, np.float64)
    trans = np.array(trans0, np.float64)
    if emission.ndim != 3 or trans.shape != (emission.shape[0], emission.shape[1], emission.shape[1]):
        raise ValueError("emission0 [B, k, V] and trans0 [B, k, k]")
    B = emission.shape[0]
    if isinstance(observes, np.ndarray) and observes.ndim == 1:
        observes = [observes] * B
    seqs = [np.ascontiguousarray(o, np.float64).reshape(-1) for o in observes]
    if len(seqs) != B:
        raise ValueError("one sequence per table (or one for all)")
    sd = np.ascontiguousarray(seeds, np.uint64)
    iterations = int(iterations)
    e_hist, t_hist, ev = [emission.copy()], [trans.copy()], np.zeros((iterations, B))
    if iterations == 0:
        return np.array(e_hist), np.array(t_hist), ev
    engine.batch_begin_problems_categorical(seqs, n_particles, emission, trans, resampler=resampler, keep_history=False, keep_masses=True)
    if resident:
        return _em_resident(engine, seqs, emission, trans, sd, iterations, bool(exact), floor)
    for it in range(iterations):
        if exact:
            engine.batch_run_exact()
        else:
            engine.batch_run(sd + np.uint64(it))
        stats = engine.batch_symbol_stats(seqs)
        ev[it] = engine.batch_exact_evidence()[0] if exact else [s["log_evidence"] for s in engine.batch_results()[0]]
        emission, trans = m_step_categorical(stats, emission, trans, floor)
        e_hist.append(emission.copy())
        t_hist.append(trans.copy())
        if it + 1 < iterations:
            engine.batch_retable_categorical(emission, trans, seqs if it == 0 else None)
    return np.array(e_hist), np.array(t_hist), ev


def _em_resident(engine, seqs, emission, trans, sd, iterations, exact, floor):
    """hmm_categorical_em's loop on the begun batch with the tables, the observes, the records and the evidences in device tensors;
    the host enqueues and looks at nothing until the loop is over."""
    import torch
    B, k, V = emission.shape
    dev = torch.device("cuda", engine.device)
    obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(seqs))).to(dev)
    e_all = torch.zeros((iterations + 1, B, k, V), dtype=torch.float64, device=dev)
    t_all = torch.zeros((iterations + 1, B, k, k), dtype=torch.float64, device=dev)
    e_all[0].copy_(torch.from_numpy(emission))
    t_all[0].copy_(torch.from_numpy(trans))
    stats = torch.zeros((B, SYMBOL_STATS_PER_PROBLEM), dtype=torch.float64, device=dev)
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
        engine.batch_symbol_stats_device(stats, obs)
        if exact:
            engine.batch_exact_evidence_device(ev_exact[it], dead)
        else:
            engine.batch_summaries_device(ev[it])
        with torch.cuda.stream(stream):                     # (the next tables start as these: a copy on the engine's stream)
            e_all[it + 1].copy_(e_all[it])
            t_all[it + 1].copy_(t_all[it])
        engine.batch_mstep_categorical_device(stats, e_all[it + 1], t_all[it + 1], floor)
        if it + 1 < iterations:
            engine.batch_retable_categorical_device(e_all[it + 1], t_all[it + 1], obs)
    engine.sync()
    ev_host = np.ascontiguousarray((ev_exact if exact else ev[:, :, 0]).cpu().numpy())
    return e_all.cpu().numpy(), t_all.cpu().numpy(), ev_host
