#!/usr/bin/env python3
"""The running statistics of an online batch (cpprob_hip_batch_online_stats_device; csrc/batch_onlinestats.hpp) beside the backward
walk that returns the same 88 numbers (cpprob_hip_batch_smooth_stats_device; csrc/batch_suffstats.hpp) on one stream: B = 1024
problems of the k = 8 table HMM, n = 256 particles, a filtering-only batch that keeps its masses -- the run writes the m table, so
neither call has a counting pass and each is timed as its one launch.  The stream is advanced to every base length in turn; there
  backward_ms         batch_smooth_stats_device with all the observes so far, at the base length (it does not consume: repeated)
  readout_ms          batch_online_stats_device with no new steps: the read-out alone
  forward_ms[chunk]   batch_online_stats_device after an advance of `chunk` steps (the advance itself is not timed), `--reps` times, the
                      length growing by chunk each time
Device-synchronised wall time; every form is warmed up once before the first base; median and spread (max - min) over the repeats.
The last line fits backward_ms = a + b L over the bases and says at which length each chunk's forward call costs the same.
usage: python tools/bench_batch_onlinestats.py [--shape 1024x256] [--bases 64 256 1024 4096] [--chunks 1 16] [--reps 9]
One JSON line a base, then the fit."""
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
    ap.add_argument("--shape", default="1024x256", help="BxN")
    ap.add_argument("--bases", nargs="+", type=int, default=[64, 256, 1024, 4096])
    ap.add_argument("--chunks", nargs="+", type=int, default=[1, 16])
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    B, n = (int(x) for x in args.shape.split("x"))
    k = 8
    bases = sorted(args.bases)
    spent = args.reps * sum(args.chunks)                        # steps the timed advances of one base take
    assert all(b1 - b0 > spent for b0, b1 in zip(bases, bases[1:])) and bases[0] > sum(args.chunks), "the bases lie too close for --reps and --chunks"
    cap = bases[-1] + spent
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    obs = np.take_along_axis(means, rng.integers(0, k, (B, cap)), axis=1) + rng.standard_normal((B, cap))
    e = cp.Engine(0)
    e.batch_begin_online(cp.MODEL_HMM_TABLE, [cap] * B, n, np.arange(1000, 1000 + B, dtype=np.uint64), tables=(means, trans), keep_history=False, keep_masses=True)
    d_stats = torch.zeros(B * 88, dtype=torch.float64, device="cuda:0")
    d_back = torch.zeros(B * 88, dtype=torch.float64, device="cuda:0")
    state = {"L": 0}

    def feed(steps):
        """Advances every problem by `steps`; returns their observes on the device, packed as the running call takes them."""
        L = state["L"]
        piece = np.ascontiguousarray(obs[:, L:L + steps])
        d = torch.from_numpy(piece.reshape(-1)).to("cuda:0")
        torch.cuda.current_stream().synchronize()
        e.batch_advance(list(piece), readout=True)
        e.sync()
        state["L"] = L + steps
        return d

    def timed(f):
        t0 = time.perf_counter()
        f()
        e.sync()
        return (time.perf_counter() - t0) * 1e3

    def med(v):
        return float(np.median(v)), float(max(v) - min(v))

    # warm-up: every form once
    for c in args.chunks:
        d = feed(c)
        e.batch_online_stats_device(d_stats, d)
    e.batch_online_stats_device(d_stats)
    d_all = torch.from_numpy(np.ascontiguousarray(obs[:, :state["L"]]).reshape(-1)).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    e.batch_smooth_stats_device(d_back, d_all)
    e.sync()
    rows = []
    for base in bases:
        d = feed(base - state["L"])
        catch_up = timed(lambda: e.batch_online_stats_device(d_stats, d))
        d_all = torch.from_numpy(np.ascontiguousarray(obs[:, :base]).reshape(-1)).to("cuda:0")
        torch.cuda.current_stream().synchronize()
        back, ro = [], []
        for _ in range(args.reps):
            back.append(timed(lambda: e.batch_smooth_stats_device(d_back, d_all)))
            ro.append(timed(lambda: e.batch_online_stats_device(d_stats)))
        # the two routes' records at the base length, relative to max(1, |backward|), in units of L 2^-52
        f, b = d_stats.cpu().numpy(), d_back.cpu().numpy()
        r = float(np.max(np.abs(f - b) / np.maximum(1.0, np.abs(b)))) / (base * 2.0 ** -52)
        row = dict(B=B, n=n, k=k, L=base, backward_ms=med(back)[0], backward_spread_ms=med(back)[1], readout_ms=med(ro)[0], readout_spread_ms=med(ro)[1],
                   catch_up_steps=int(d.numel() // B), catch_up_ms=catch_up, forward_minus_backward_over_L_ulp=r)
        for c in args.chunks:
            t = []
            for _ in range(args.reps):
                dc = feed(c)
                t.append(timed(lambda: e.batch_online_stats_device(d_stats, dc)))
            row["forward_ms_chunk%d" % c], row["forward_spread_ms_chunk%d" % c] = med(t)
        row["L_after"] = state["L"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if len(rows) >= 2:
        Ls = np.array([r["L"] for r in rows], np.float64)
        slope, icpt = np.polyfit(Ls, np.array([r["backward_ms"] for r in rows]), 1)
        fit = dict(backward_ms_per_step=float(slope), backward_ms_at_0=float(icpt))
        for c in args.chunks:
            fwd = float(np.median([r["forward_ms_chunk%d" % c] for r in rows]))
            fit["forward_ms_chunk%d" % c] = fwd
            fit["crossing_length_chunk%d" % c] = float((fwd - icpt) / slope) if slope > 0 else None
        print(json.dumps(fit), flush=True)
    e.close()


if __name__ == "__main__":
    main()
