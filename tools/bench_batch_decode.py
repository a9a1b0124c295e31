#!/usr/bin/env python3
"""What a decode costs a streaming user beside the advance it follows (profiles/r20_notes.md; no threshold hangs on these times).
Shape: CPPROB_HIP_MODEL_HMM_TABLE, k = 8, B = 4096 problems of n = 1024 particles, capacity 64, history kept, one observe an advance.
A repetition begins the stream, advances it 63 times, decodes once (so the step words and the table of masses are current, as after the
advance before) and synchronises; then it times, host clock around enqueue and synchronise, each on its own:
  advance     the 64th one-observe advance (cpprob_hip_batch_advance, no read-out)
  lag         cpprob_hip_batch_decode_lag_device, lag = 8, the 9 rows the new observe can still change (from = 64 - 1 - 8; the first
              of them became final): counts the new row, walks the one new step forward, traces 8 words back
  full        cpprob_hip_batch_decode_device: no step is new by then; the traceback of all 64 words a problem
  cold        the same full decode on a batch begun and run at once (cpprob_hip_batch_begin_problems, 64 observes): counts 64 rows,
              walks 64 steps forward, traces them back -- what a run batch pays every call
It reports the median and the spread (max - min) of `--reps` repetitions, the first (code objects, allocations) left out.
usage: python tools/bench_batch_decode.py [--reps 7]
One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, CAP, K, LAG = 4096, 1024, 64, 8, 8


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
    d_path = torch.zeros((B * CAP,), dtype=torch.int8, device="cuda:0")
    d_cold = torch.zeros((B * CAP,), dtype=torch.int8, device="cuda:0")
    d_row = torch.zeros((B, LAG + 1), dtype=torch.int8, device="cuda:0")
    d_score = torch.zeros((B,), dtype=torch.float64, device="cuda:0")
    d_score_cold = torch.zeros((B,), dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    frm = np.full(B, CAP - 1 - LAG, np.uint32)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        e.sync()
        return (time.perf_counter() - t0) * 1e3

    times = {"advance": [], "lag": [], "full": [], "cold": []}
    for _ in range(args.reps + 1):
        e.batch_begin_online(cp.MODEL_HMM_TABLE, [CAP] * B, N, seeds, tables=(means, trans))
        for at in range(CAP - 1):
            e.batch_advance(list(obs[:, at:at + 1]), readout=False)
        e.batch_decode_device(d_path, d_score)
        e.sync()
        last = list(obs[:, CAP - 1:CAP])
        times["advance"].append(timed(lambda: e.batch_advance(last, readout=False)))
        times["lag"].append(timed(lambda: e.batch_decode_lag_device(LAG, d_row, d_score, frm)))
        times["full"].append(timed(lambda: e.batch_decode_device(d_path, d_score)))
    row, path, score = d_row.cpu().numpy(), d_path.cpu().numpy().reshape(B, CAP), d_score.cpu().numpy()
    for _ in range(args.reps + 1):
        e.batch_begin_problems(cp.MODEL_HMM_TABLE, list(obs), N, tables=(means, trans))
        e.batch_run(seeds)
        e.sync()
        times["cold"].append(timed(lambda: e.batch_decode_device(d_cold, d_score_cold)))
    cold, cold_score = d_cold.cpu().numpy().reshape(B, CAP), d_score_cold.cpu().numpy()
    e.close()
    out = dict(B=B, n=N, k=K, capacity=CAP, lag=LAG, reps=args.reps, states_in_range=bool(path.min() >= 0 and path.max() < K),
               scores_finite=bool(np.all(np.isfinite(score))), run_batch_is_the_streams=bool(np.array_equal(cold, path) and np.array_equal(cold_score, score)),
               lag_rows_are_the_paths_tail=bool(np.array_equal(row, path[:, CAP - 1 - LAG:])))
    for name, t in times.items():
        out[name + "_ms"] = float(np.median(t[1:]))
        out[name + "_spread_ms"] = float(max(t[1:]) - min(t[1:]))
        out[name + "_first_ms"] = t[0]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
