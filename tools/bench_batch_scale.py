#!/usr/bin/env python3
"""What per-state emission scales cost beside their unit-scale siblings (cpprob_hip_batch_retable_scaled_device,
_mstep_scaled_device; csrc/batch_scale.hpp).  Shapes: B = 1024 problems of k = 8 states, n = 256 particles, T in {16, 256, 1024};
per-problem tables.  Device-synchronised wall time: every form is warmed up twice, then timed `--reps` times in alternation, and the
median and the spread (max - min) over the repeats are reported.  Per shape:
  run_ms                 batch_run on the unit batch, then sync()
  retable_device_ms      batch_retable_device on the unit batch, then sync()
  em_resident_ms         one resident EM iteration on the unit batch: run, batch_smooth_stats_device, batch_summaries_device,
                         batch_mstep_device, batch_retable_device, then sync()
  advance1_ms, advance16_ms          a plain batch_advance of 1 / 16 observes a problem on a unit online batch, then sync()
  learn1_ms, learn16_ms              a batch_advance_learn of 1 / 16 observes a problem on an armed unit online batch, then sync()
  run_scaled_ms, retable_scaled_device_ms, em_resident_scaled_ms, advance1_scaled_ms, advance16_scaled_ms, learn1_scaled_ms, learn16_scaled_ms
                         the same on a batch begun with sigmas (left out where the package does not know them)
--package-root DIR measures the cpprob_amd package of another checkout of this project (built there), e.g. the parent commit's.
--unit-only leaves the scaled forms out: the process then runs what a checkout without them runs, and the two compare like with like.
usage: python tools/bench_batch_scale.py [--T 16 256 1024] [--reps 9] [--package-root DIR] [--unit-only]
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
    ap.add_argument("--unit-only", action="store_true")
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repeats")
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    has = "cpprob_hip_batch_retable_scaled_device" in cp.capi.SYMBOLS and not args.unit_only
    B, n, k = args.B, args.n, args.k
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    trans /= trans.sum(-1, keepdims=True)
    sigmas = rng.uniform(0.5, 2.0, (B, k))
    seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
    unit, scaled, online = cp.Engine(0), cp.Engine(0), cp.Engine(0)
    kw = dict(keep_history=False, keep_masses=True)
    for T in args.T:
        seqs = [means[b][rng.integers(0, k, T)] + sigmas[b][rng.integers(0, k, T)] * rng.standard_normal(T) for b in range(B)]
        d_obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(seqs))).to("cuda:0")
        d_means, d_trans, d_sigmas = (torch.from_numpy(a).to("cuda:0") for a in (means, trans, sigmas))
        d_stats = torch.zeros((B, 88), dtype=torch.float64, device="cuda:0")
        d_ev = torch.zeros((B, 4), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        unit.batch_begin_problems(cp.MODEL_HMM_TABLE, seqs, n, tables=(means, trans), **kw)
        if has:
            scaled.batch_begin_problems(cp.MODEL_HMM_TABLE, seqs, n, tables=(means, trans, sigmas), **kw)

        def forms_of(eng, sg):
            def run():
                eng.batch_run(seeds)
                eng.sync()

            def retable():
                if sg is None:
                    eng.batch_retable_device(d_means, d_trans, d_obs)
                else:
                    eng.batch_retable_device(d_means, d_trans, d_obs, sigmas=sg)
                eng.sync()

            def em_resident():
                eng.batch_run(seeds)
                eng.batch_smooth_stats_device(d_stats, d_obs)
                eng.batch_summaries_device(d_ev)
                if sg is None:
                    eng.batch_mstep_device(d_stats, d_means, d_trans)
                    eng.batch_retable_device(d_means, d_trans, d_obs)
                else:
                    eng.batch_mstep_device(d_stats, d_means, d_trans, sigmas=sg)
                    eng.batch_retable_device(d_means, d_trans, d_obs, sigmas=sg)
                eng.sync()
            return run, retable, em_resident

        def advance_of(tables, chunk):
            # (an online batch of capacity 256 a problem: begun again when it is full)
            state = {"at": 256}
            new = [np.resize(s, chunk) for s in seqs]

            def advance():
                if state["at"] + chunk > 256:
                    online.batch_begin_online(cp.MODEL_HMM_TABLE, [256] * B, n, seeds, tables=tables, **kw)
                    online.batch_advance([s[:1] for s in seqs])
                    online.sync()
                    state["at"] = 1
                t0 = time.perf_counter()
                online.batch_advance(new)
                online.sync()
                state["at"] += chunk
                return (time.perf_counter() - t0) * 1e3
            return advance

        def learn_of(tables, chunk):
            # (a learning advance of an armed online batch; a scaled one fits its sigmas)
            state = {"at": 256}
            new = [np.resize(s, chunk) for s in seqs]
            gamma = (np.arange(256) + 1.0) ** -0.6

            def advance():
                if state["at"] + chunk > 256:
                    online.batch_begin_online(cp.MODEL_HMM_TABLE, [256] * B, n, seeds, tables=tables, **kw)
                    if len(tables) == 3:
                        online.batch_learn_begin(gamma, 1, sigma_floor=1e-3)
                    else:
                        online.batch_learn_begin(gamma, 1)
                    online.batch_advance_learn([s[:1] for s in seqs])
                    online.sync()
                    state["at"] = 1
                t0 = time.perf_counter()
                online.batch_advance_learn(new)
                online.sync()
                state["at"] += chunk
                return (time.perf_counter() - t0) * 1e3
            return advance
        forms = dict(zip(("run", "retable_device", "em_resident"), forms_of(unit, None)))
        if has:
            forms.update(zip(("run_scaled", "retable_scaled_device", "em_resident_scaled"), forms_of(scaled, d_sigmas)))
        r = alternate(forms, args.reps)
        row = dict(B=B, n=n, k=k, T=T, reps=args.reps, package=os.path.abspath(args.package_root), scales=has)
        for name, (med, spread) in r.items():
            row[name + "_ms"], row[name + "_spread_ms"] = round(med, 4), round(spread, 4)
        if T == args.T[0]:
            # the advances do not depend on T: measured once (the host's packing of the observes is outside the timed part)
            for name, tables in (("", (means, trans)), ("_scaled", (means, trans, sigmas))):
                if name and not has:
                    continue
                for chunk in (1, 16):
                    for what, make in (("advance", advance_of), ("learn", learn_of)):
                        adv = make(tables, chunk)
                        adv()
                        adv()
                        v = [adv() for _ in range(args.reps)]
                        row["%s%d%s_ms" % (what, chunk, name)], row["%s%d%s_spread_ms" % (what, chunk, name)] = round(float(np.median(v)), 4), round(max(v) - min(v), 4)
        print(json.dumps(row), flush=True)
    for e in (unit, scaled, online):
        e.close()


if __name__ == "__main__":
    main()
