#!/usr/bin/env python3
"""Batched SMC against one problem at a time (profiles/r08_notes.md).  The same problems -- hmm observes from oracle.exact.simulate_hmm,
seeds 1000 + b -- are timed three ways:
  (a) one batched run: cpprob_hip_batch_run, one launch for all B problems;
  (b) B sequential Engine.begin + run calls on one context (each problem has its own observes, so each needs its begin);
  (c) three contexts in flight, problems dealt round-robin: a context's next begin waits only for its own previous run.
Device-synchronised wall time; every form is warmed up, then (a) and (b) / (c) are timed in alternation `--reps` times and the
median is reported.  (b) and (c) cost ~0.1 ms a problem, so they time the first `--sample` problems and scale to B (the per-problem
cost does not depend on B); the JSON says so.  (a)'s statistics are compared with (b)'s for the problems (b) ran.
usage: python tools/bench_batch.py [--T 16 128] [--B 256 1024 4096] [--n 1024 4096 8192] [--reps 3] [--sample 128]
One JSON line per cell."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--B", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096, 8192])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=128)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    from oracle import exact

    eng = [cp.Engine(0) for _ in range(3)]
    for T in args.T:
        obs_all = np.stack([exact.simulate_hmm(T, 1000 + b) for b in range(max(args.B))])
        for B in args.B:
            obs = obs_all[:B]
            seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
            S = min(B, args.sample)
            for n in args.n:
                e0 = eng[0]

                def run_a():
                    t0 = time.perf_counter()
                    e0.batch_run(seeds)
                    e0.sync()
                    return time.perf_counter() - t0

                def run_b():
                    t0 = time.perf_counter()
                    for b in range(S):
                        e0.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs[b], n, seed=int(seeds[b]))
                        e0.run(0)
                    e0.sync()
                    return (time.perf_counter() - t0) * B / S

                def run_c():
                    t0 = time.perf_counter()
                    for b in range(S):
                        e = eng[b % 3]
                        e.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs[b], n, seed=int(seeds[b]))   # (begin waits for this context's own stream)
                        e.run(0)
                    for e in eng:
                        e.sync()
                    return (time.perf_counter() - t0) * B / S

                e0.batch_begin(cp.MODEL_HMM3, obs, n)
                run_a()
                run_b()
                run_c()
                ta, tb, tc = [], [], []
                for _ in range(args.reps):
                    ta.append(run_a()); tb.append(run_b()); tc.append(run_c())
                # (a) against (b): the same problems, the same seeds
                _, stats_a, _, _ = e0.batch_results()
                worst = 0.0
                for b in range(min(S, 16)):
                    e0.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs[b], n, seed=int(seeds[b]))
                    e0.run(0)
                    worst = max(worst, float(np.abs(e0.results()[1] - stats_a[b]).max()))
                a, bb, c = float(np.median(ta)), float(np.median(tb)), float(np.median(tc))
                ps = float(B) * n * T
                print(json.dumps(dict(T=T, B=B, n=n, a_ms=a * 1e3, b_ms=bb * 1e3, c_ms=c * 1e3, a_spread_ms=(max(ta) - min(ta)) * 1e3,
                                      a_particle_steps_per_s=ps / a, b_particle_steps_per_s=ps / bb, c_particle_steps_per_s=ps / c,
                                      speedup_vs_b=bb / a, speedup_vs_c=c / a, bc_sampled_problems=S, stats_max_abs_diff=worst,
                                      stats_match=worst < 1e-11)), flush=True)
    for e in eng:
        e.close()


if __name__ == "__main__":
    main()
