#!/usr/bin/env python3
"""The conditional SMC run of a batch (cpprob_hip_batch_run_conditional_device; csrc/batch_csmc.hpp) beside the unconditional run it
replaces in a particle-Gibbs sweep (cpprob_hip_batch_run on the same filtering-only batch that keeps its masses).  The batch is the
Gibbs sampler's: a table a problem (cpprob_hip_batch_begin_problems), every problem of T steps and n particles; the reference paths
are the trajectories cpprob_hip_batch_smooth_device left of an unconditional run.  Device-synchronised wall time of `--calls` calls
back to back; both forms are warmed up, then timed `--reps` times in alternation, and the median and the spread (max - min) of the time
a call are reported.
usage: python tools/bench_batch_csmc.py [--shapes 1024x256x1024] [--k 3] [--reps 9] [--calls 10]
One JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_batch_smooth import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1024x256x1024"], help="BxNxT")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    rng = np.random.default_rng(1)
    k = args.k
    e = cp.Engine(0)
    for shape in args.shapes:
        B, n, T = (int(x) for x in shape.split("x"))
        means = np.sort(rng.uniform(-2.0, 2.0, (B, k)), axis=1)
        trans = rng.uniform(0.05, 1.0, (B, k, k))
        obs = [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b in range(B)]
        seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
        e.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans), keep_history=False, keep_masses=True)
        ref = torch.empty(B * T, dtype=torch.int8, device="cuda:0")
        e.batch_run(seeds)
        e.batch_smooth_device(traj_i8=ref, n_traj=1)
        e.sync()

        def run():
            for _ in range(args.calls):
                e.batch_run(seeds)
            e.sync()

        def conditional():
            for _ in range(args.calls):
                e.batch_run_conditional_device(seeds, ref)
            e.sync()

        r = alternate({"batch_run": run, "batch_run_conditional": conditional}, args.reps)
        row = dict(B=B, n=n, T=T, k=k, calls=args.calls)
        for name, (med, spread) in r.items():
            row[name + "_ms"], row[name + "_spread_ms"] = med / args.calls, spread / args.calls
        row["conditional_over_run"] = r["batch_run_conditional"][0] / r["batch_run"][0]
        print(json.dumps(row), flush=True)
    e.close()


if __name__ == "__main__":
    main()
