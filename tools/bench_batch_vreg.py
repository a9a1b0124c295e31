#!/usr/bin/env python3
"""What Markov-switching vector regressions cost beside the full family (cpprob_hip_batch_begin_problems_vreg, _retable_vreg_device,
_vreg_stats_device, _mstep_vreg_device; csrc/batch_vreg.hpp).  Shape: B = 1024 problems of k = 8 states, T = 1024, Q responses and P
covariates a step; per-problem tables; exact runs.  Device-synchronised wall time: every form is warmed up twice, then timed `--reps`
times in alternation, and the median and the spread (max - min) over the repeats are reported, for every (Q, P) of --QP a
vector-regression batch (name_vreg_qQpP_ms) and a full batch on the same Q + P doubles a step (name_full_qQpP_ms):
  stats            batch_vreg_stats_device / batch_full_stats_device (1304 doubles a problem), then sync()
  retable_device   the family's device re-table, then sync()
  mstep            the statistics, then the family's device M-step, then sync(): take `stats` off
  em_resident      one resident exact iteration: batch_run_exact, the statistics, the evidences, the M-step, the re-table, and the run
                   that follows it (which `stats` needs), then sync()
usage: python tools/bench_batch_vreg.py [--T 1024] [--QP 2,3 8,8 15,1] [--reps 9]
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
    ap.add_argument("--QP", nargs="+", default=["2,3", "8,8", "15,1"])
    ap.add_argument("--reps", type=int, default=9)
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
    forms, retables, engines = {}, {}, []

    def add(name, e, stats, mstep, ret):
        torch.cuda.synchronize()
        e.batch_run_exact()
        # (em_resident first in a round: it leaves a finished run, which `stats` needs after a `retable_device`)
        forms["em_resident_" + name] = synced(e, e.batch_run_exact, stats, lambda: e.batch_exact_evidence_device(ev, dead), mstep, ret, e.batch_run_exact)
        forms["stats_" + name] = synced(e, stats)
        forms["mstep_" + name] = synced(e, stats, mstep)
        retables["retable_device_" + name] = synced(e, ret)
    for Q, P in [tuple(int(v) for v in qp.split(",")) for qp in args.QP]:
        D = Q + P
        coef = rng.normal(0.0, 0.5, (B, k, Q, P))
        W = rng.normal(0.0, 0.3, (B, k, Q, Q))
        covs = W @ W.transpose(0, 1, 3, 2) + np.eye(Q)
        x = rng.normal(0.0, 1.0, (B, T, P))
        x[:, :, 0] = 1.0
        obs = []
        for b in range(B):
            s = rng.integers(0, k, T)
            obs.append(np.column_stack([np.einsum("tqi,ti->tq", coef[b][s], x[b]) + rng.normal(0.0, 1.0, (T, Q)), x[b]]))
        flat = dev(np.concatenate(obs).reshape(-1))
        e = cp.Engine(0)
        engines.append(e)
        e.batch_begin_problems_vreg(obs, 8, coef, covs, trans, **kw)
        t, st = [dev(coef), dev(covs), dev(trans), flat], torch.zeros((B, 1304), dtype=torch.float64, device="cuda:0")
        add("vreg_q%dp%d" % (Q, P), e, lambda e=e, st=st, t=t: e.batch_vreg_stats_device(st, t[3]), lambda e=e, st=st, t=t: e.batch_mstep_vreg_device(st, t[0], t[1], t[2]),
            lambda e=e, t=t: e.batch_retable_vreg_device(*t))
        f = cp.Engine(0)
        engines.append(f)
        means, Wf = rng.normal(0.0, 1.0, (B, k, D)), rng.normal(0.0, 0.3, (B, k, D, D))
        f.batch_begin_problems_full(obs, 8, means, Wf @ Wf.transpose(0, 1, 3, 2) + np.eye(D), trans, **kw)
        u, su = [dev(means), dev(Wf @ Wf.transpose(0, 1, 3, 2) + np.eye(D)), dev(trans), flat], torch.zeros((B, 1304), dtype=torch.float64, device="cuda:0")
        add("full_q%dp%d" % (Q, P), f, lambda f=f, su=su, u=u: f.batch_full_stats_device(su, u[3]), lambda f=f, su=su, u=u: f.batch_mstep_full_device(su, u[0], u[1], u[2]),
            lambda f=f, u=u: f.batch_retable_full_device(*u))
    row = dict(B=B, k=k, T=T, QP=list(args.QP), reps=args.reps)
    r = alternate(forms, args.reps)
    r.update(alternate(retables, args.reps))
    for name, (med, spread) in r.items():
        row[name + "_ms"], row[name + "_spread_ms"] = round(med, 4), round(spread, 4)
    print(json.dumps(row), flush=True)
    for e in engines:
        e.close()


if __name__ == "__main__":
    main()
