#!/usr/bin/env python3
"""What diagonal-Gaussian vector emissions cost beside the scaled family (cpprob_hip_batch_begin_problems_diag, _retable_diag_device,
_diag_stats_device, _mstep_diag_device; csrc/batch_diag.hpp).  Shape: B = 1024 problems of k = 8 states, T = 1024, D coordinates a
step; per-problem tables; exact runs.  Device-synchronised wall time: every form is warmed up twice, then timed `--reps` times in
alternation, and the median and the spread (max - min) over the repeats are reported, for a scaled batch (name_scaled_ms) and, for every
D of --D, a diagonal one (name_dD_ms):
  stats            batch_smooth_stats_device (88 doubles a problem) / batch_diag_stats_device (600), then sync()
  retable_device   batch_retable_device(sigmas=) / batch_retable_diag_device, then sync()
  em_resident      one resident exact iteration: batch_run_exact, the statistics, the evidences, the M-step, the re-table, and the run
                   that follows it (which `stats` needs), then sync()
  run_exact        batch_run_exact, then sync(): what to take off em_resident for one run
  begin            the begin itself (the host evaluates the first rows), `--begin_reps` times
usage: python tools/bench_batch_diag.py [--T 1024] [--D 1 8 32] [--reps 9]
One JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    from bench_batch_scale import alternate
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1024)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--D", nargs="+", type=int, default=[1, 8, 32])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--begin_reps", type=int, default=3)
    args = ap.parse_args()
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    B, k, T = args.B, args.k, args.T
    rng = np.random.default_rng(1)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    kw = dict(keep_history=False, keep_masses=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    ev, dead = torch.zeros(B, dtype=torch.float64, device="cuda:0"), torch.zeros(B, dtype=torch.int32, device="cuda:0")

    def synced(eng, *calls):
        def f():
            for call in calls:
                call()
            eng.sync()
        return f
    forms, retables, begins, engines = {}, {}, {}, []
    for D in [0] + list(args.D):                            # (0: the scaled batch, one double a step)
        name, d = ("scaled", 1) if D == 0 else ("d%d" % D, D)
        means, sigmas = np.sort(rng.normal(0.0, 3.0, (B, k, d)), axis=1), rng.uniform(0.5, 2.0, (B, k, d))
        obs = [means[b][rng.integers(0, k, T)] + rng.normal(0.0, 1.0, (T, d)) for b in range(B)]
        e = cp.Engine(0)
        engines.append(e)
        if D == 0:
            obs, means, sigmas = [o[:, 0] for o in obs], means[:, :, 0], sigmas[:, :, 0]
            begin = lambda e=e, o=obs, m=means, s=sigmas: e.batch_begin_problems(cp.MODEL_HMM_TABLE, o, 8, tables=(m, trans, s), **kw)      # noqa: E731
        else:
            begin = lambda e=e, o=obs, m=means, s=sigmas: e.batch_begin_problems_diag(o, 8, m, s, trans, **kw)      # noqa: E731
        begin()
        t = [dev(means), dev(sigmas), dev(trans), dev(np.concatenate(obs).reshape(-1))]
        st = torch.zeros((B, 88 if D == 0 else 600), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        e.batch_run_exact()
        if D == 0:
            stats = lambda e=e, st=st, t=t: e.batch_smooth_stats_device(st, t[3])      # noqa: E731
            ret = lambda e=e, t=t: e.batch_retable_device(t[0], t[2], t[3], sigmas=t[1])      # noqa: E731
            mstep = lambda e=e, st=st, t=t: e.batch_mstep_device(st, t[0], t[2], sigmas=t[1])      # noqa: E731
        else:
            stats = lambda e=e, st=st, t=t: e.batch_diag_stats_device(st, t[3])      # noqa: E731
            ret = lambda e=e, t=t: e.batch_retable_diag_device(t[0], t[1], t[2], t[3])      # noqa: E731
            mstep = lambda e=e, st=st, t=t: e.batch_mstep_diag_device(st, t[0], t[1], t[2])      # noqa: E731
        # (em_resident first in a round: it leaves a finished run, which `stats` needs after a `retable_device`)
        forms["em_resident_" + name] = synced(e, e.batch_run_exact, stats, lambda e=e: e.batch_exact_evidence_device(ev, dead), mstep, ret, e.batch_run_exact)
        forms["stats_" + name] = synced(e, stats)
        forms["run_exact_" + name] = synced(e, e.batch_run_exact)
        retables["retable_device_" + name] = synced(e, ret)
        begins["begin_" + name] = synced(e, begin)
    row = dict(B=B, k=k, T=T, D=list(args.D), reps=args.reps, begin_reps=args.begin_reps)
    r = alternate(forms, args.reps)
    r.update(alternate(retables, args.reps))
    r.update(alternate(begins, args.begin_reps))
    for name, (med, spread) in r.items():
        row[name + "_ms"], row[name + "_spread_ms"] = round(med, 4), round(spread, 4)
    print(json.dumps(row), flush=True)
    for e in engines:
        e.close()


if __name__ == "__main__":
    main()
