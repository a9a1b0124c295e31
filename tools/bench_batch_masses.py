#!/usr/bin/env python3
"""What the kept masses cost and save (CPPROB_HIP_BATCH_KEEP_MASSES; csrc/batch_smc.hpp).  Shape: B = 1024, n = 1024, T = 64, the
workload of tools/bench_batch_stats.py, both models.  Device-synchronised wall time; every form is warmed up, then timed `--reps`
times in alternation, and the median and the spread (max - min) over the repeats are reported.  Per cell:
  run_filter_ms     batch_run of a filtering-only batch (keep_history = 0), no bit
  run_masses_ms     ... with the bit: the cost of the rows (64 bytes and eight fix_weights a problem and step)
  run_keep_ms       batch_run of the same batch with keep_history = 1
  em_keep_ms        one EM iteration as cpprob_amd.hmm_table_em does it -- batch_begin_problems, batch_run, batch_smooth_stats (host
                    variant) -- with keep_history = 1 (model table only)
  em_masses_ms      ... as a filtering-only batch with masses
  ws_*_bytes        the three batches' workspaces
--package-root DIR measures the cpprob_amd package of another checkout of this project (built there), e.g. the parent commit's: the
forms its Engine does not know are left out, so run_filter_ms of two checkouts can be set side by side, process by process.
usage: python tools/bench_batch_masses.py [--models hmm3 table] [--shapes 1024x1024x64] [--reps 9] [--package-root DIR]
One JSON line per cell."""
import argparse
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_batch_smooth import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", choices=["hmm3", "table"], default=["hmm3", "table"])
    ap.add_argument("--shapes", nargs="+", default=["1024x1024x64"], help="BxNxT")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--package-root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch  # noqa: F401  (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    from oracle import exact
    has_masses = "keep_masses" in inspect.signature(cp.Engine.batch_begin).parameters
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-2.0, 2.0, 3))
    trans = rng.uniform(0.05, 1.0, (3, 3))
    kinds = {"filter": dict(keep_history=False), "keep": dict(keep_history=True)}
    if has_masses:
        kinds["masses"] = dict(keep_history=False, keep_masses=True)
    engines = {k: cp.Engine(0) for k in kinds}                  # a context a kind: begun once, run many times
    for e in engines.values():
        e.set_hmm(means, trans)
    for shape in args.shapes:
        B, n, T = (int(x) for x in shape.split("x"))
        obs = np.stack([exact.simulate_hmm(T, 1000 + b) for b in range(B)])
        seqs = list(obs)
        seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
        tables = (np.repeat(means[None], B, 0), np.repeat(trans[None], B, 0))
        for name in args.models:
            model = cp.MODEL_HMM3 if name == "hmm3" else cp.MODEL_HMM_TABLE
            row = dict(model=name, B=B, n=n, T=T, package=os.path.abspath(args.package_root), masses=has_masses)
            forms = {}
            for kind, kw in kinds.items():
                e = engines[kind]
                e.batch_begin(model, obs, n, **kw)
                row["ws_%s_bytes" % kind] = cp.capi.batch_workspace_bytes(model, n, B, T, **kw)

                def run(e=e):
                    e.batch_run(seeds)
                    e.sync()
                forms["run_" + kind] = run
            r = alternate(forms, args.reps)
            if has_masses:
                a, b = engines["filter"].batch_results(), engines["masses"].batch_results()
                assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), "the bit changed the filtering results"
                want, got = engines["keep"].batch_smooth_stats(obs), engines["masses"].batch_smooth_stats(obs)
                assert all(np.array_equal(want[f], got[f]) for f in want), "the statistics differ between the two kinds of batch"
                assert engines["masses"].batch_smooth_grid()[0] == 0 and engines["keep"].batch_smooth_grid()[0] > 0
            if name == "table":
                em = {}
                for kind in ("keep", "masses") if has_masses else ("keep",):
                    def iteration(e=engines[kind], kw=kinds[kind]):
                        e.batch_begin_problems(model, seqs, n, tables=tables, **kw)
                        e.batch_run(seeds)
                        return e.batch_smooth_stats(seqs)
                    em["em_" + kind] = iteration
                r.update(alternate(em, args.reps))
            for k, (med, spread) in r.items():
                row[k + "_ms"], row[k + "_spread_ms"] = med, spread
            if has_masses:
                row["masses_over_filter"] = r["run_masses"][0] / r["run_filter"][0]
                if "em_masses" in r:
                    row["em_masses_over_keep"] = r["em_masses"][0] / r["em_keep"][0]
            print(json.dumps(row), flush=True)
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
