#!/usr/bin/env python3
"""What Poisson emissions cost beside their scaled siblings (cpprob_hip_batch_begin_problems_poisson, _retable_poisson*,
_mstep_poisson_device; csrc/batch_poisson.hpp).  Shapes: B = 1024 problems of k = 8 states, n = 256 particles, T in {16, 256, 1024};
per-problem tables.  Device-synchronised wall time: every form is warmed up twice, then timed `--reps` times in alternation, and the
median and the spread (max - min) over the repeats are reported.  Per shape, for the scaled batch (name_scaled_ms) and the Poisson batch
(name_poisson_ms):
  begin            batch_begin_problems (the host writes the rows and uploads them), then sync()
  retable          batch_retable with the observes staged by an earlier call, then sync()
  retable_device   batch_retable_device, then sync()
  run              batch_run, then sync()
  em_host          one iteration of the host loop: batch_begin_problems, batch_run, batch_smooth_stats, the evidences, em.m_step
  em_resident      one resident iteration: run, batch_smooth_stats_device, batch_summaries_device, batch_mstep_device,
                   batch_retable_device, then sync()
usage: python tools/bench_batch_poisson.py [--T 16 256 1024] [--reps 9]
One JSON line per shape."""
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
    ap.add_argument("--T", nargs="+", type=int, default=[16, 256, 1024])
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repeats")
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    from cpprob_amd import em
    B, n, k = args.B, args.n, args.k
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, k)), axis=1) + 0.5 * np.arange(k)
    sigmas = rng.uniform(0.5, 2.0, (B, k))
    rates = np.sort(np.exp(rng.uniform(-1.0, 3.0, (B, k))), axis=1)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    trans /= trans.sum(-1, keepdims=True)
    seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
    kw = dict(keep_history=False, keep_masses=True)
    engines = {"scaled": cp.Engine(0), "poisson": cp.Engine(0)}
    for T in args.T:
        seqs = {"scaled": [means[b][rng.integers(0, k, T)] + sigmas[b][rng.integers(0, k, T)] * rng.standard_normal(T) for b in range(B)],
                "poisson": [rng.poisson(rates[b][rng.integers(0, k, T)]).astype(np.float64) for b in range(B)]}
        forms = {}
        for fam, eng in engines.items():
            obs = seqs[fam]
            tables = (means, trans, sigmas) if fam == "scaled" else (rates, trans)
            emission = "normal" if fam == "scaled" else "poisson"
            d_obs = torch.from_numpy(np.ascontiguousarray(np.concatenate(obs))).to("cuda:0")
            d_tab = [torch.from_numpy(a.copy()).to("cuda:0") for a in tables]
            d_stats = torch.zeros((B, 88), dtype=torch.float64, device="cuda:0")
            d_ev = torch.zeros((B, 4), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()

            def make(eng=eng, obs=obs, tables=tables, emission=emission, d_obs=d_obs, d_tab=d_tab, d_stats=d_stats, d_ev=d_ev, fam=fam):
                extra = dict(sigmas=d_tab[2]) if fam == "scaled" else dict(emission="poisson")

                def begin():
                    eng.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=tables, emission=emission, **kw)
                    eng.sync()

                def retable():
                    eng.batch_retable(tables, None, emission=emission)
                    eng.sync()

                def retable_device():
                    eng.batch_retable_device(d_tab[0], d_tab[1], d_obs, **extra)
                    eng.sync()

                def run():
                    eng.batch_run(seeds)
                    eng.sync()

                def em_host():
                    eng.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=tables, emission=emission, **kw)
                    eng.batch_run(seeds)
                    st = eng.batch_smooth_stats(obs)
                    eng.batch_results()
                    if fam == "scaled":
                        em.m_step(st, tables[0], tables[1], tables[2], 1e-3)
                    else:
                        em.m_step(st, tables[0], tables[1], emission="poisson")
                    eng.batch_retable(tables, obs, emission=emission)      # (stages the observes again for `retable`)
                    eng.sync()

                def em_resident():
                    eng.batch_run(seeds)
                    eng.batch_smooth_stats_device(d_stats, d_obs)
                    eng.batch_summaries_device(d_ev)
                    if fam == "scaled":
                        eng.batch_mstep_device(d_stats, d_tab[0], d_tab[1], sigmas=d_tab[2])
                    else:
                        eng.batch_mstep_device(d_stats, d_tab[0], d_tab[1], emission="poisson")
                    eng.batch_retable_device(d_tab[0], d_tab[1], d_obs, **extra)
                    eng.sync()
                return dict(begin=begin, retable=retable, retable_device=retable_device, run=run, em_host=em_host, em_resident=em_resident)
            made = make()
            made["begin"]()
            eng.batch_retable(tables, obs, emission=emission)              # (stages the observes)
            eng.sync()
            # em_host first in a round: it ends with the observes staged, which `retable` needs after `begin`
            for name in ("em_host", "retable", "retable_device", "run", "em_resident", "begin"):
                forms["%s_%s" % (name, fam)] = made[name]
        ordered = {}
        for name in ("em_host", "retable", "retable_device", "run", "em_resident"):
            for fam in engines:
                ordered["%s_%s" % (name, fam)] = forms["%s_%s" % (name, fam)]
        r = alternate(ordered, args.reps)
        r.update(alternate({"begin_%s" % fam: forms["begin_%s" % fam] for fam in engines}, args.reps))
        row = dict(B=B, n=n, k=k, T=T, reps=args.reps)
        for name, (med, spread) in r.items():
            row[name + "_ms"], row[name + "_spread_ms"] = round(med, 4), round(spread, 4)
        print(json.dumps(row), flush=True)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
