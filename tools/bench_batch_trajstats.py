#!/usr/bin/env python3
"""The trajectory sufficient statistics of a batch (cpprob_hip_batch_traj_stats_device; csrc/batch_trajstats.hpp) beside the plain
trajectory walk they mirror (cpprob_hip_batch_smooth_device, trajectories only, the same n_traj) and beside the host route the call
replaces (Engine.batch_smooth to the host, then numpy counting).  Both device calls share one counting pass and are timed without it:
the batch is an online batch advanced to its full length, whose m table is kept -- the first smoothing call counts the rows, every
timed call finds them counted and launches its walk alone.  Device-synchronised wall time; every form is warmed up, then timed
`--reps` times in alternation, and the median and the spread (max - min) over the repeats are reported.  Per cell:
  smooth_traj_ms     batch_smooth_device, the trajectories only: T n_traj bytes a problem written
  traj_stats_ms      batch_traj_stats_device with the observes: 88 n_traj doubles a problem written
  host_route_ms      batch_smooth to host arrays, then the records counted with numpy (--host_reps times; 0: skipped)
usage: python tools/bench_batch_trajstats.py [--models hmm3 table] [--shapes 256x256x256x1024 1024x256x1024x1] [--reps 9]
One JSON line per cell; the device records are checked against the host route's at the timed size."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_batch_smooth import alternate  # noqa: E402


def count_records(traj, obs):
    """[n_traj, 88] of one problem's trajectories [T, n_traj] and observes [T], vectorised over the trajectories (the counts are exact;
    the weighted sums are numpy's, in another order than the device's)."""
    T, M = traj.shape
    col = np.arange(M)
    rec = np.zeros((M, 88))
    pair = (traj[:-1] * 8 + traj[1:]) + 64 * col
    rec[:, :64] = np.bincount(pair.ravel(), minlength=64 * M).reshape(M, 64)
    at = (traj + 8 * col).ravel()
    rec[:, 64:72] = np.bincount(at, minlength=8 * M).reshape(M, 8)
    y = np.repeat(obs, M)
    rec[:, 72:80] = np.bincount(at, weights=y, minlength=8 * M).reshape(M, 8)
    rec[:, 80:88] = np.bincount(at, weights=y * y, minlength=8 * M).reshape(M, 8)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", choices=["hmm3", "table"], default=["hmm3", "table"])
    ap.add_argument("--shapes", nargs="+", default=["256x256x256x1024", "1024x256x1024x1"], help="BxNxTxn_traj")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host_reps", type=int, default=3)
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
        B, n, T, M = (int(x) for x in shape.split("x"))
        obs = np.stack([exact.simulate_hmm(T, 1000 + b) for b in range(B)])
        seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
        for name in args.models:
            model = cp.MODEL_HMM3 if name == "hmm3" else cp.MODEL_HMM_TABLE
            e.batch_begin_online(model, [T] * B, n, seeds)
            e.batch_advance(list(obs))
            d_traj = torch.zeros(B * T * M, dtype=torch.int8, device="cuda:0")
            d_stats = torch.zeros(B * M * 88, dtype=torch.float64, device="cuda:0")
            d_obs = torch.from_numpy(obs.reshape(-1)).to("cuda:0")
            torch.cuda.current_stream().synchronize()
            e.batch_smooth_device(None, d_traj, M)                  # counts the rows, once
            e.sync()
            assert e.batch_smooth_grid()[0] > 0

            def smooth_traj():
                e.batch_smooth_device(None, d_traj, M)
                e.sync()

            def traj_stats():
                e.batch_traj_stats_device(d_stats, M, 0, d_obs)
                e.sync()

            r = alternate({"smooth_traj": smooth_traj, "traj_stats": traj_stats}, args.reps)
            assert e.batch_smooth_grid()[0] == 0, "a timed call counted rows"
            traj_stats()
            tiles = e.batch_traj_stats_grid()
            got = d_stats.cpu().numpy().reshape(B, M, 88)
            row = dict(model=name, B=B, n=n, T=T, n_traj=M, tiles=tiles)
            for k, (med, spread) in r.items():
                row[k + "_ms"], row[k + "_spread_ms"] = med, spread
            row["stats_over_traj"] = r["traj_stats"][0] / r["smooth_traj"][0]
            host = []
            for _ in range(args.host_reps):
                t0 = time.perf_counter()
                _, traj = e.batch_smooth(M, 0)
                want = np.stack([count_records(traj[b], obs[b]) for b in range(B)])
                host.append((time.perf_counter() - t0) * 1e3)
            if host:
                row["host_route_ms"], row["host_route_spread_ms"] = float(np.median(host)), float(max(host) - min(host))
                row["host_over_stats"] = row["host_route_ms"] / r["traj_stats"][0]
                row["counts_equal"] = bool(np.array_equal(got[:, :, :72], want[:, :, :72]))
                row["weighted_sums_max_diff"] = float(np.abs(got[:, :, 72:] - want[:, :, 72:]).max())
            print(json.dumps(row), flush=True)
    e.close()


if __name__ == "__main__":
    main()
