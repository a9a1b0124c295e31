#!/usr/bin/env python3
"""The expected sufficient statistics of a batch (cpprob_hip_batch_smooth_stats_device; csrc/batch_suffstats.hpp) beside the marginals
of the walk they share (cpprob_hip_batch_smooth_device, marginals only).  Shape: B = 1024, n = 1024, T = 64, the workload of
tools/bench_batch_smooth.py, both models.  Both calls share one counting pass, and both are timed without it the same way: the batch
is an online batch advanced to its full length, whose m table is kept -- the first smoothing call counts the rows, every timed call
finds them counted and launches its walk alone.  Device-synchronised wall time; every form is warmed up, then timed `--reps` times in
alternation, and the median and the spread (max - min) over the repeats are reported.  Per cell:
  smooth_marg_ms      batch_smooth_device, the marginals only: one wavefront a problem, T spp stores a problem
  stats_device_ms     batch_smooth_stats_device with the observes: one wavefront a problem, four additions a step more, 88 stores a problem
  stats_blind_ms      the same without observes
usage: python tools/bench_batch_stats.py [--models hmm3 table] [--shapes 1024x1024x64] [--reps 9]
One JSON line per cell."""
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
    ap.add_argument("--models", nargs="+", choices=["hmm3", "table"], default=["hmm3", "table"])
    ap.add_argument("--shapes", nargs="+", default=["1024x1024x64"], help="BxNxT")
    ap.add_argument("--reps", type=int, default=9)
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
            K = 3 if name == "hmm3" else 8
            e.batch_begin_online(model, [T] * B, n, seeds)
            e.batch_advance(list(obs))
            d_marg = torch.zeros(B * T * K, dtype=torch.float64, device="cuda:0")
            d_stats = torch.zeros(B * 88, dtype=torch.float64, device="cuda:0")
            d_obs = torch.from_numpy(obs.reshape(-1)).to("cuda:0")
            torch.cuda.current_stream().synchronize()
            e.batch_smooth_device(d_marg, None)                 # counts the rows, once
            e.sync()
            assert e.batch_smooth_grid()[0] > 0

            def smooth_marg():
                e.batch_smooth_device(d_marg, None)
                e.sync()

            def stats_device():
                e.batch_smooth_stats_device(d_stats, d_obs)
                e.sync()

            def stats_blind():
                e.batch_smooth_stats_device(d_stats)
                e.sync()

            r = alternate({"smooth_marg": smooth_marg, "stats_device": stats_device, "stats_blind": stats_blind}, args.reps)
            assert e.batch_smooth_grid()[0] == 0, "a timed call counted rows"
            stats_device()
            st = cp.capi.split_stats(d_stats.cpu().numpy())
            marg = d_marg.cpu().numpy().reshape(B, T, K)
            row = dict(model=name, B=B, n=n, T=T, occ_minus_marginal_sums=float(np.abs(st["occ"][:, :K] - marg.sum(axis=1)).max()),
                       transitions_minus_steps=float(np.abs(st["xi"].sum(axis=(1, 2)) - (T - 1)).max()))
            for k, (med, spread) in r.items():
                row[k + "_ms"], row[k + "_spread_ms"] = med, spread
            row["stats_over_marg"] = r["stats_device"][0] / r["smooth_marg"][0]
            print(json.dumps(row), flush=True)
    e.close()


if __name__ == "__main__":
    main()
