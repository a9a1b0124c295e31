#!/usr/bin/env python3
"""What re-tabling a begun batch saves over beginning a fresh one (cpprob_hip_batch_retable*; csrc/batch_retable.hpp).  Shapes:
B = 1024 problems of k = 8 states, n = 256 particles, T in {16, 256, 1024}; per-problem tables.  Device-synchronised wall time: every
form is warmed up, then timed `--reps` times in alternation, and the median and the spread (max - min) over the repeats are reported.
Per shape:
  begin_ms          (a) batch_begin_problems with the tables: the route re-tabling replaces (it ends with a synchronisation of its own)
  retable_host_ms   (b) batch_retable with host tables, the observes already on the device, then sync()
  retable_device_ms (c) batch_retable_device on device tensors, then sync()
  run_ms            batch_run, then sync() (what no form here may slow down)
  em_host_ms        (d) one EM iteration of cpprob_amd.hmm_table_em: begin, run, batch_smooth_stats, batch_results, the host M-step
  em_resident_ms    ... of the resident loop: run, batch_smooth_stats_device, batch_summaries_device, batch_mstep_device,
                    batch_retable_device, then sync()
  gibbs_begin_ms    (e) one sweep of cpprob_amd.hmm_table_gibbs: begin, run, batch_traj_stats, batch_results, sample_tables
  gibbs_retable_ms  ... with batch_retable in the begin's place
--package-root DIR measures the cpprob_amd package of another checkout of this project (built there), e.g. the parent commit's: the
forms its Engine does not know are left out, so begin_ms and run_ms of two checkouts can be set side by side.
--once FORM runs the named form a few times and exits: a process of its own for a profiler's kernel trace.
usage: python tools/bench_batch_retable.py [--T 16 256 1024] [--reps 9] [--package-root DIR] [--once retable_device]
One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alternate(forms, reps):
    """forms: {name: callable}.  {name: (median ms, spread ms)} of their wall times."""
    def once(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3
    for f in forms.values():
        f()
        f()
    got = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            got[k].append(once(f))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", nargs="+", type=int, default=[16, 256, 1024])
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--once", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repeats")
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    from cpprob_amd import em, gibbs
    has = hasattr(cp.Engine, "batch_retable")
    B, n, k = args.B, args.n, args.k
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    trans /= trans.sum(-1, keepdims=True)
    seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
    eng = cp.Engine(0)
    kept = cp.Engine(0)                                         # the batch that is begun once and re-tabled (a begin forgets the staged observes)
    for T in args.T:
        seqs = [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b in range(B)]
        flat = np.ascontiguousarray(np.concatenate(seqs))
        kw = dict(keep_history=False, keep_masses=True)
        draw = np.random.default_rng(2)

        def begin():
            eng.batch_begin_problems(cp.MODEL_HMM_TABLE, seqs, n, tables=(means, trans), **kw)
            eng.sync()

        def run():
            eng.batch_run(seeds)
            eng.sync()

        def em_host():
            begin()
            eng.batch_run(seeds)
            stats = eng.batch_smooth_stats(seqs)
            eng.batch_results()
            em.m_step(stats, means, trans)

        def gibbs_begin():
            begin()
            eng.batch_run(seeds)
            stats = eng.batch_traj_stats(1, 0, seqs)
            eng.batch_results()
            gibbs.sample_tables({f: v[:, 0] for f, v in stats.items()}, k, draw)
        forms = {"begin": begin, "run": run, "em_host": em_host, "gibbs_begin": gibbs_begin}
        if has:
            d_obs = torch.from_numpy(flat).to("cuda:0")
            d_means, d_trans = torch.from_numpy(means).to("cuda:0"), torch.from_numpy(trans).to("cuda:0")
            d_stats = torch.zeros((B, 88), dtype=torch.float64, device="cuda:0")
            d_ev = torch.zeros((B, 4), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()

            def retable_host():
                kept.batch_retable((means, trans), None)
                kept.sync()

            def retable_device():
                kept.batch_retable_device(d_means, d_trans, d_obs)
                kept.sync()

            def em_resident():
                kept.batch_run(seeds)
                kept.batch_smooth_stats_device(d_stats, d_obs)
                kept.batch_summaries_device(d_ev)
                kept.batch_mstep_device(d_stats, d_means, d_trans)
                kept.batch_retable_device(d_means, d_trans, d_obs)
                kept.sync()

            def gibbs_retable():
                kept.batch_retable((means, trans), None)
                kept.batch_run(seeds)
                stats = kept.batch_traj_stats(1, 0, seqs)
                kept.batch_results()
                gibbs.sample_tables({f: v[:, 0] for f, v in stats.items()}, k, draw)
            forms.update(retable_host=retable_host, retable_device=retable_device, gibbs_retable=gibbs_retable, em_resident=em_resident)
        begin()
        if has:
            kept.batch_begin_problems(cp.MODEL_HMM_TABLE, seqs, n, tables=(means, trans), **kw)
            kept.batch_retable((means, trans), seqs)            # (stages the observes once)
            kept.batch_run(seeds)
            kept.sync()
        if args.once:
            for _ in range(5):
                forms[args.once]()
            continue
        r = alternate(forms, args.reps)
        row = dict(B=B, n=n, k=k, T=T, reps=args.reps, package=os.path.abspath(args.package_root), retable=has)
        for name, (med, spread) in r.items():
            row[name + "_ms"], row[name + "_spread_ms"] = round(med, 4), round(spread, 4)
        if has:
            row["retable_grid_y"] = kept.batch_retable_grid()
            row["retable_bytes"] = 72 * B * T
        print(json.dumps(row), flush=True)
    eng.close()
    kept.close()


if __name__ == "__main__":
    main()
