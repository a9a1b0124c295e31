#!/usr/bin/env python3
"""The smoothing work a streaming user enqueues after one advance of an online batch (profiles/r15_notes.md): fixed-lag smoothing
(cpprob_hip_batch_smooth_lag_device) beside the full backward smoother (cpprob_hip_batch_smooth_device), at two lengths of the same
stream.  Shape: CPPROB_HIP_MODEL_HMM_TABLE, k = 8, B = 1024 problems of n = 1024 particles, capacity 512, advances of 8 observes,
lag = 16, marginals only.  A cell is (call, length): the stream is begun, advanced 8 observes at a time to length - 8, smoothed once
(so the table of masses is current, as after the advance before), advanced by the last 8 observes and synchronised; then the call is
timed, host clock around enqueue and synchronise.  That is one repetition; a cell reports the median and the spread (max - min) of
`--reps` of them, the first (which loads the code objects and makes the allocations) left out.
  lag   batch_smooth_lag_device, from = length - 8 - lag: the rows the advance changed, 24 of them
  full  batch_smooth_device: every row (a library without the fixed-lag call runs these cells only)
Every cell runs in a process of its own under `timeout`; the first cell that fails ends the run with its exit status.
usage: python tools/bench_batch_smooth_lag.py [--cells lag@64 lag@512 full@64 full@512] [--reps 7] [--limit 240]
One JSON line per cell."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, CAP, K, STEP, LAG = 1024, 1024, 512, 8, 8, 16


def cell(call, length, reps):
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    if call == "lag" and not hasattr(cp.Engine, "batch_smooth_lag_device"):
        raise SystemExit("this library has no fixed-lag call: run the full cells")
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, K)), axis=1) + 0.5 * np.arange(K)
    trans = rng.uniform(0.05, 1.0, (B, K, K))
    obs = means[np.arange(B)[:, None], rng.integers(0, K, (B, CAP))] + rng.standard_normal((B, CAP))
    seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
    e = cp.Engine(0)
    frm = np.full(B, max(0, length - STEP - LAG), np.uint32)
    prev = np.full(B, max(0, length - 2 * STEP - LAG), np.uint32)      # ... of the advance before
    rows = length - int(frm[0])
    d_marg = torch.zeros((B, rows if call == "lag" else CAP, 8), dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()

    def smooth(before):
        if call == "lag":
            e.batch_smooth_lag_device(LAG, prev if before else frm, d_marg)
        else:
            e.batch_smooth_device(d_marg, None)

    times = []
    for _ in range(reps + 1):
        e.batch_begin_online(cp.MODEL_HMM_TABLE, [CAP] * B, N, seeds, tables=(means, trans))
        for at in range(0, length - STEP, STEP):
            e.batch_advance(list(obs[:, at:at + STEP]), readout=False)
        if length > STEP:
            smooth(True)
        e.batch_advance(list(obs[:, length - STEP:length]), readout=False)
        e.sync()
        t0 = time.perf_counter()
        smooth(False)
        e.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    got = d_marg.cpu().numpy()
    last = got[:, rows - 1] if call == "lag" else got[:, length - 1]
    e.close()
    t = times[1:]
    print(json.dumps(dict(call=call, length=length, B=B, n=N, k=K, capacity=CAP, advance=STEP, lag=LAG, reps=reps, ms=float(np.median(t)), spread_ms=float(max(t) - min(t)),
                          first_ms=times[0], marginal_sum_error=float(np.abs(last.sum(axis=1) - 1.0).max()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=["lag@64", "lag@512", "full@64", "full@512"], help="call@length")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds a cell may take")
    ap.add_argument("--cell", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cell:
        call, length = args.cell.split("@")
        if call not in ("lag", "full") or not STEP <= int(length) <= CAP or int(length) % STEP:
            raise SystemExit("a cell is lag@L or full@L, L a multiple of %d up to %d" % (STEP, CAP))
        return cell(call, int(length), args.reps)
    for c in args.cells:
        rc = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--cell", c, "--reps", str(args.reps)]).returncode
        if rc:
            print("cell %s ended with status %d: stopping" % (c, rc), file=sys.stderr)
            sys.exit(rc)


if __name__ == "__main__":
    main()
