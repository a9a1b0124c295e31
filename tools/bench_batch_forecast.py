#!/usr/bin/env python3
"""What a forecast costs a streaming user beside the advance it follows (profiles/r19_notes.md; no threshold hangs on these times).
Shape: CPPROB_HIP_MODEL_HMM_TABLE, k = 8, B = 4096 problems of n = 1024 particles, capacity 64, history kept, one observe an advance.
A repetition begins the stream, advances it 63 times, forecasts once (so the table of masses is current, as after the advance before)
and synchronises; then it times, host clock around enqueue and synchronise, each on its own:
  advance     the 64th one-observe advance (cpprob_hip_batch_advance, no read-out)
  marginals   cpprob_hip_batch_forecast_device, H = 16, n_traj = 0: counts the one new row, then 16 pushes a problem
  futures     the same call with n_traj = 1024 (the row is counted by then: the forecast launch alone)
  predictive  cpprob_hip_batch_predictive_device for the one new row (from = 64)
It reports the median and the spread (max - min) of `--reps` repetitions, the first (code objects, allocations) left out.
usage: python tools/bench_batch_forecast.py [--reps 7]
One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, CAP, K, H, M = 4096, 1024, 64, 8, 16, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, K)), axis=1) + 0.5 * np.arange(K)
    trans = rng.uniform(0.05, 1.0, (B, K, K))
    obs = means[np.arange(B)[:, None], rng.integers(0, K, (B, CAP))] + rng.standard_normal((B, CAP))
    seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
    e = cp.Engine(0)
    d_marg = torch.zeros((B, H, 8), dtype=torch.float64, device="cuda:0")
    d_traj = torch.zeros((B, H + 1, M), dtype=torch.int8, device="cuda:0")
    d_rows = torch.zeros((B, 1, 8), dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    frm = np.full(B, CAP, np.uint32)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        e.sync()
        return (time.perf_counter() - t0) * 1e3

    times = {"advance": [], "marginals": [], "futures": [], "predictive": []}
    for _ in range(args.reps + 1):
        e.batch_begin_online(cp.MODEL_HMM_TABLE, [CAP] * B, N, seeds, tables=(means, trans))
        for at in range(CAP - 1):
            e.batch_advance(list(obs[:, at:at + 1]), readout=False)
        e.batch_forecast_device(H, d_marg)
        e.sync()
        last = list(obs[:, CAP - 1:CAP])
        times["advance"].append(timed(lambda: e.batch_advance(last, readout=False)))
        times["marginals"].append(timed(lambda: e.batch_forecast_device(H, d_marg)))
        times["futures"].append(timed(lambda: e.batch_forecast_device(H, d_marg, d_traj, n_traj=M)))
        times["predictive"].append(timed(lambda: e.batch_predictive_device(d_rows, frm)))
    marg, traj, rows = d_marg.cpu().numpy(), d_traj.cpu().numpy(), d_rows.cpu().numpy()
    e.close()
    out = dict(B=B, n=N, k=K, capacity=CAP, horizon=H, n_traj=M, reps=args.reps,
               marginal_sum_error=float(np.abs(marg.sum(axis=2) - 1.0).max()), states_in_range=bool(traj.min() >= 0 and traj.max() < K),
               predictive_is_first_row=bool(np.array_equal(rows[:, 0], marg[:, 0])))
    for name, t in times.items():
        out[name + "_ms"] = float(np.median(t[1:]))
        out[name + "_spread_ms"] = float(max(t[1:]) - min(t[1:]))
        out[name + "_first_ms"] = t[0]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
