#!/usr/bin/env python3
"""Backward smoothing of a batch (cpprob_hip_batch_smooth_device; csrc/batch_smooth.hpp) against the run it follows and against the
lineage read-out of the same size, batch_paths_device at M = n (profiles/r14_notes.md).  Shape: B = 1024, n = 1024, T = 64, the
workload of tools/bench_batch_paths.py, both models.  Device-synchronised wall time; every form is warmed up, then timed `--reps`
times in alternation, and the median and the spread (max - min) over the repeats are reported.  Per cell:
  run_ms              batch_run of the begun batch (begin not counted), synchronised
  paths_device_ms     batch_paths_device into tensors made beforehand (all n lineages), synchronised
  smooth_marg_ms      batch_smooth_device, the marginals only (counting pass + one wavefront a problem)
  smooth_ms           batch_smooth_device, the marginals and M = n trajectories a problem
  smooth_100_ms       the same with M = 100
  run_then_smooth_ms  run and smoothing (M = n) enqueued back to back, one synchronisation
usage: python tools/bench_batch_smooth.py [--models hmm3 table] [--shapes 1024x1024x64] [--reps 5]
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
    """forms: {name: callable}.  {name: (median ms, spread ms)} of their wall times."""
    def once(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3
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
    ap.add_argument("--shapes", nargs="+", default=["1024x1024x64"], help="BxNxT")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    from oracle import exact
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-2.0, 2.0, 3))
    trans = rng.uniform(0.05, 1.0, (3, 3))
    e = cp.Engine(0)
    e.set_hmm(means, trans)
    for shape in args.shapes:
        B, n, T = (int(x) for x in shape.split("x"))
        obs = np.stack([exact.simulate_hmm(T, 1000 + b) for b in range(B)])
        seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
        for name in args.models:
            model = cp.MODEL_HMM3 if name == "hmm3" else cp.MODEL_HMM_TABLE
            e.batch_begin(model, obs, n)
            K = 3 if name == "hmm3" else 8
            first, wfirst = cp.capi.batch_paths_layout([T] * B, n)
            d_paths = torch.zeros(int(first[-1]), dtype=torch.int8, device="cuda:0")
            d_logw = torch.zeros(int(wfirst[-1]), dtype=torch.float64, device="cuda:0")
            d_traj = torch.zeros(B * T * n, dtype=torch.int8, device="cuda:0")
            d_marg = torch.zeros(B * T * K, dtype=torch.float64, device="cuda:0")
            torch.cuda.current_stream().synchronize()

            def run():
                e.batch_run(seeds)
                e.sync()

            def paths_device():
                e.batch_paths_device(d_paths, d_logw)
                e.sync()

            def smooth_marg():
                e.batch_smooth_device(d_marg, None)
                e.sync()

            def smooth():
                e.batch_smooth_device(d_marg, d_traj, n_traj=n)
                e.sync()

            def smooth_100():
                e.batch_smooth_device(d_marg, d_traj[:B * T * 100], n_traj=100)
                e.sync()

            def run_then_smooth():
                e.batch_run(seeds)
                e.batch_smooth_device(d_marg, d_traj, n_traj=n)
                e.sync()

            run()
            r = alternate({"run": run, "paths_device": paths_device, "smooth_marg": smooth_marg, "smooth": smooth, "smooth_100": smooth_100,
                           "run_then_smooth": run_then_smooth}, args.reps)
            # the marginals are distributions over the model's states, and the trajectories' frequencies follow them
            smooth()
            marg = d_marg.cpu().numpy().reshape(B, T, K)
            traj = d_traj.cpu().numpy().reshape(B, T, n)
            freq = np.stack([(traj == s).mean(axis=2) for s in range(K)], axis=2)
            row = dict(model=name, B=B, n=n, T=T, marginal_sum_error=float(np.abs(marg.sum(axis=2) - 1.0).max()),
                       frequency_minus_marginal=float(np.abs(freq - marg).max()))
            for k, (med, spread) in r.items():
                row[k + "_ms"], row[k + "_spread_ms"] = med, spread
            row["smooth_over_run"] = r["smooth"][0] / r["run"][0]
            row["smooth_over_paths"] = r["smooth"][0] / r["paths_device"][0]
            print(json.dumps(row), flush=True)
    e.close()


if __name__ == "__main__":
    main()
