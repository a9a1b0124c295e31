#!/usr/bin/env python3
"""A batch advanced in pieces (cpprob_hip_batch_begin_online / _advance) against the one-shot batch and against the old way of
extending one (profiles/r12_notes.md).  B = 1024 problems of n = 1024 particles and T = 64 observes, both models, keep_history 1 and 0.
Device-synchronised wall time; every form is warmed up, then timed `--reps` times in alternation, and the median and the spread
(max - min) over the repeats are reported.  Per cell:
  one_shot_ms          batch_run of the begun whole batch (begin not counted)
  online_P_ms          the whole sequence fed P observes at a time, P in --pieces: begin_online + T / P advances + one synchronisation
                       (the read-out with the last advance only); online_P_per_advance_ms = the advances' share / (T / P)
  online_P_sync_ms     the same with a synchronisation after every advance (a caller that reads each result before the next observes)
  rebegin_16_ms        the old way, for pieces of 16: per piece a begin_problems with the longer sequences and a run from step 0
usage: python tools/bench_batch_online.py [--models hmm3 table] [--pieces 1 4 16 64] [--reps 5] [--B 1024] [--n 1024] [--T 64]
One JSON line per cell."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(forms, reps):
    """forms: {name: callable returning seconds or None (then: its wall time)}.  {name: (median ms, spread ms)}."""
    def once(f):
        t0 = time.perf_counter()
        got = f()
        return (time.perf_counter() - t0 if got is None else got) * 1e3
    for f in forms.values():
        f()
    got = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            got[k].append(once(f))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", choices=["hmm3", "table"], default=["hmm3", "table"])
    ap.add_argument("--pieces", nargs="+", type=int, default=[1, 4, 16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--T", type=int, default=64)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    from oracle import exact
    B, n, T = args.B, args.n, args.T
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-2.0, 2.0, (1, 3)), axis=1)
    trans = rng.uniform(0.05, 1.0, (1, 3, 3))
    obs = np.stack([exact.simulate_hmm(T, 1000 + b) for b in range(B)])
    seqs = list(obs)
    seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
    e = cp.Engine(0)
    ref = cp.Engine(0)
    for x in (e, ref):
        x.set_hmm(means[0], trans[0])
    for name in args.models:
        model = cp.MODEL_HMM3 if name == "hmm3" else cp.MODEL_HMM_TABLE
        for keep in (True, False):
            ref.batch_begin_problems(model, seqs, n, keep_history=keep)

            def one_shot():
                ref.batch_run(seeds)
                ref.sync()

            def online(P, sync_each):
                def run():
                    e.batch_begin_online(model, [T] * B, n, seeds, keep_history=keep)
                    t0 = time.perf_counter()
                    for at in range(0, T, P):
                        e.batch_advance([o[at:at + P] for o in seqs], readout=at + P >= T)
                        if sync_each:
                            e.sync()
                    e.sync()
                    return time.perf_counter() - t0
                return run

            def rebegin(P):
                def run():
                    t0 = time.perf_counter()
                    for at in range(0, T, P):
                        e.batch_begin_problems(model, [o[:at + P] for o in seqs], n, keep_history=keep)
                        e.batch_run(seeds)
                    e.sync()
                    return time.perf_counter() - t0
                return run

            forms = {"one_shot": one_shot}
            for P in args.pieces:
                forms["online_%d" % P] = online(P, False)
                forms["online_%d_sync" % P] = online(P, True)
            if 16 in args.pieces:
                forms["rebegin_16"] = rebegin(16)
            r = alternate(forms, args.reps)
            # the last form run was an online one or the re-begun one: check the pieces against the whole once more, exactly
            online(args.pieces[0], False)()
            same = all(np.array_equal(x, y) for x, y in zip(e.batch_results()[1:], ref.batch_results()[1:])) and e.batch_results()[0] == ref.batch_results()[0]
            row = dict(model=name, B=B, n=n, T=T, keep_history=int(keep), results_equal=bool(same))
            for k, (med, spread) in r.items():
                row[k + "_ms"], row[k + "_spread_ms"] = med, spread
            for P in args.pieces:
                row["online_%d_per_advance_ms" % P] = r["online_%d" % P][0] / ((T + P - 1) // P)
                row["online_%d_sync_per_advance_ms" % P] = r["online_%d_sync" % P][0] / ((T + P - 1) // P)
            print(json.dumps(row), flush=True)
    e.close()
    ref.close()


if __name__ == "__main__":
    main()
