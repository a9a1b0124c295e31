#!/usr/bin/env python3
"""What categorical emissions cost beside their Poisson siblings (cpprob_hip_batch_symbol_stats_device, _retable_categorical_device,
_mstep_categorical_device; csrc/batch_categorical.hpp).  Shape: B = 1024 problems of k = 8 states, V = 64 symbols, T = 1024; per-problem
tables; exact runs.  Device-synchronised wall time: every form is warmed up twice, then timed `--reps` times in alternation, and the
median and the spread (max - min) over the repeats are reported, for the Poisson batch (name_poisson_ms) and the categorical batch
(name_categorical_ms):
  stats            batch_smooth_stats_device (88 doubles a problem) / batch_symbol_stats_device (600), then sync()
  retable_device   batch_retable_device(emission="poisson") / batch_retable_categorical_device, then sync()
  em_resident      one resident exact iteration: batch_run_exact, the statistics, the evidences, the M-step, the re-table, and the run
                   that follows it (which `stats` needs), then sync()
  run_exact        batch_run_exact, then sync(): what to take off em_resident for one run
usage: python tools/bench_batch_categorical.py [--T 1024] [--reps 9]
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
    ap.add_argument("--V", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    B, k, V, T = args.B, args.k, args.V, args.T
    rng = np.random.default_rng(1)
    rates = np.sort(np.exp(rng.uniform(-1.0, 3.0, (B, k))), axis=1)
    E = np.maximum(rng.dirichlet(np.ones(V), (B, k)), 1e-4)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    kw = dict(keep_history=False, keep_masses=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    pe, ce = cp.Engine(0), cp.Engine(0)
    p_obs = [rng.poisson(rates[b][rng.integers(0, k, T)]).astype(np.float64) for b in range(B)]
    c_obs = [rng.integers(0, V, T).astype(np.float64) for b in range(B)]
    pe.batch_begin_problems(cp.MODEL_HMM_TABLE, p_obs, 8, tables=(rates, trans), emission="poisson", **kw)
    ce.batch_begin_problems_categorical(c_obs, 8, E, trans, **kw)
    dp, dc = [dev(rates), dev(trans), dev(np.concatenate(p_obs))], [dev(E), dev(trans), dev(np.concatenate(c_obs))]
    sp, sc = torch.zeros((B, 88), dtype=torch.float64, device="cuda:0"), torch.zeros((B, 600), dtype=torch.float64, device="cuda:0")
    ev, dead = torch.zeros(B, dtype=torch.float64, device="cuda:0"), torch.zeros(B, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pe.batch_run_exact()
    ce.batch_run_exact()

    def synced(eng, *calls):
        def f():
            for call in calls:
                call()
            eng.sync()
        return f
    p_stats, c_stats = (lambda: pe.batch_smooth_stats_device(sp, dp[2])), (lambda: ce.batch_symbol_stats_device(sc, dc[2]))
    p_ret, c_ret = (lambda: pe.batch_retable_device(dp[0], dp[1], dp[2], emission="poisson")), (lambda: ce.batch_retable_categorical_device(*dc))
    p_m, c_m = (lambda: pe.batch_mstep_device(sp, dp[0], dp[1], emission="poisson")), (lambda: ce.batch_mstep_categorical_device(sc, dc[0], dc[1]))
    # (em_resident first in a round: it leaves a finished run, which `stats` needs after a `retable_device`)
    forms = {"em_resident_poisson": synced(pe, pe.batch_run_exact, p_stats, lambda: pe.batch_exact_evidence_device(ev, dead), p_m, p_ret, pe.batch_run_exact),
             "em_resident_categorical": synced(ce, ce.batch_run_exact, c_stats, lambda: ce.batch_exact_evidence_device(ev, dead), c_m, c_ret, ce.batch_run_exact),
             "stats_poisson": synced(pe, p_stats), "stats_categorical": synced(ce, c_stats),
             "run_exact_poisson": synced(pe, pe.batch_run_exact), "run_exact_categorical": synced(ce, ce.batch_run_exact)}
    row = dict(B=B, k=k, V=V, T=T, reps=args.reps)
    r = alternate(forms, args.reps)
    r.update(alternate({"retable_device_poisson": synced(pe, p_ret), "retable_device_categorical": synced(ce, c_ret)}, args.reps))
    for name, (med, spread) in r.items():
        row[name + "_ms"], row[name + "_spread_ms"] = round(med, 4), round(spread, 4)
    print(json.dumps(row), flush=True)
    pe.close()
    ce.close()


if __name__ == "__main__":
    main()
