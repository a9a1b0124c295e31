#!/usr/bin/env python3
"""What Gaussian-mixture vector emissions cost beside the diagonal family (cpprob_hip_batch_begin_problems_mix, _retable_mix_device,
_mix_stats_device, _mstep_mix_device; csrc/batch_mix.hpp).  Shape: B = 1024 problems of k = 8 states, T = 1024, D coordinates a step,
M components a state; per-problem tables; exact runs.  Device-synchronised wall time: every form is warmed up twice, then timed `--reps`
times in alternation, and the median and the spread (max - min) over the repeats are reported, for every D of --D for a diagonal batch
(name_dD_diag_ms) and for every M of --M a mixture one (name_dD_mM_ms):
  stats            batch_diag_stats_device (600 doubles a problem) / batch_mix_stats_device (2200: the walk, then the moments), then sync()
  retable_device   batch_retable_diag_device / batch_retable_mix_device, then sync()
  em_resident      one resident exact iteration: batch_run_exact, the statistics, the evidences, the M-step, the re-table, and the run
                   that follows it (which `stats` needs), then sync()
  run_exact        batch_run_exact, then sync(): what to take off em_resident for one run
usage: python tools/bench_batch_mix.py [--T 1024] [--D 1 8 16] [--M 1 4 8] [--reps 7]
One JSON line a D."""
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
    ap.add_argument("--D", nargs="+", type=int, default=[1, 8, 16])
    ap.add_argument("--M", nargs="+", type=int, default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=7)
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
    for D in args.D:
        forms, retables, engines = {}, {}, []
        centres = np.sort(rng.normal(0.0, 3.0, (B, k, D)), axis=1)
        obs = [centres[b][rng.integers(0, k, T)] + rng.normal(0.0, 1.0, (T, D)) for b in range(B)]
        d_obs = dev(np.concatenate(obs).reshape(-1))
        for M in [0] + list(args.M):                        # (0: the diagonal batch)
            name = "d%d_%s" % (D, "diag" if M == 0 else "m%d" % M)
            e = cp.Engine(0)
            engines.append(e)
            if M == 0:
                sigmas = rng.uniform(0.5, 2.0, (B, k, D))
                e.batch_begin_problems_diag(obs, 8, centres, sigmas, trans, **kw)
                t = [dev(centres), dev(sigmas), dev(trans), d_obs]
                st = torch.zeros((B, 600), dtype=torch.float64, device="cuda:0")
                stats = lambda e=e, st=st, t=t: e.batch_diag_stats_device(st, t[3])      # noqa: E731
                ret = lambda e=e, t=t: e.batch_retable_diag_device(t[0], t[1], t[2], t[3])      # noqa: E731
                mstep = lambda e=e, st=st, t=t: e.batch_mstep_diag_device(st, t[0], t[1], t[2])      # noqa: E731
            else:
                weights, sigmas = rng.uniform(0.2, 1.0, (B, k, M)), rng.uniform(0.5, 2.0, (B, k, M, D))
                means = centres[:, :, None, :] + rng.normal(0.0, 1.0, (B, k, M, D))
                e.batch_begin_problems_mix(obs, 8, weights, means, sigmas, trans, **kw)
                t = [dev(weights), dev(means), dev(sigmas), dev(trans), d_obs]
                st = torch.zeros((B, cp.capi.MIX_STATS_PER_PROBLEM), dtype=torch.float64, device="cuda:0")
                stats = lambda e=e, st=st, t=t: e.batch_mix_stats_device(st, t[4])      # noqa: E731
                ret = lambda e=e, t=t: e.batch_retable_mix_device(*t)      # noqa: E731
                mstep = lambda e=e, st=st, t=t: e.batch_mstep_mix_device(st, t[0], t[1], t[2], t[3])      # noqa: E731
            torch.cuda.synchronize()
            e.batch_run_exact()
            # (em_resident first in a round: it leaves a finished run, which `stats` needs after a `retable_device`)
            forms["em_resident_" + name] = synced(e, e.batch_run_exact, stats, lambda e=e: e.batch_exact_evidence_device(ev, dead), mstep, ret, e.batch_run_exact)
            forms["stats_" + name] = synced(e, stats)
            forms["run_exact_" + name] = synced(e, e.batch_run_exact)
            retables["retable_device_" + name] = synced(e, ret)
        row = dict(B=B, k=k, T=T, D=D, M=list(args.M), reps=args.reps)
        r = alternate(forms, args.reps)
        r.update(alternate(retables, args.reps))
        for name, (med, spread) in r.items():
            row[name + "_ms"], row[name + "_spread_ms"] = round(med, 4), round(spread, 4)
        print(json.dumps(row), flush=True)
        for e in engines:
            e.close()


if __name__ == "__main__":
    main()
