#!/usr/bin/env python3
"""Batches of problems that differ (cpprob_hip_batch_begin_problems) against the uniform batch and against one table at a time
(profiles/r09_notes.md).  Device-synchronised wall time; every form is warmed up, the forms of a cell are timed in alternation
`--reps` times (each timing the median of `--inner` runs) and the median and the spread (max - min) over the repeats are reported.
Cells (--cells):
  uniform   --model (HMM_TABLE or HMM3), B = 1024, n = 4096, T = 16, keep_history 1 and 0: the same batch begun by batch_begin and by
            batch_begin_problems (shared table); both run the one kernel, so the two forms show what the descriptors cost.  Also the
            host time of batch_begin alone (begin_ms)
  order     a skewed batch (1024 problems, T_b log-uniform in 4 .. 128, n_b in {512, 4096}) in the dispatch order of the loaded library
  buys      B = 1024 tables x one sequence, T = 16, n = 1024 and 4096: one heterogeneous batch (begin + run + results) against, per table,
            set_hmm + batch_begin of one problem + batch_run + batch_results, timed on `--sample` tables and scaled to B
--libs A B ...: the cells run in child processes that load these builds of the library in alternation (CPPROB_HIP_LIB) -- how
profiles/r09_notes.md compared the shipped kernel with builds that read the thresholds from global memory or keep the caller's dispatch
order, and profiles/r10_notes.md the one kernel with the parent commit's two.
usage: python tools/bench_batch_problems.py [--cells uniform order buys] [--model table|hmm3] [--reps 3] [--inner 5] [--sample 128] [--libs A B ...]
One JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tables(B, k=3, seed=1):
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-2.0, 2.0, (B, k)), axis=1)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    return means, trans


def timed(fn, inner):
    out = []
    for _ in range(inner):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def alternate(forms, reps, inner):
    """forms: {name: callable}.  Returns {name: (median ms, spread ms)} over `reps` alternated timings."""
    for f in forms.values():
        f()
    got = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            got[k].append(timed(f, inner) * 1e3)
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in got.items()}


def cell_uniform(cp, args, emit, keeps=(True, False)):
    from oracle import exact
    B, n, T = 1024, 4096, 16
    means, trans = tables(1, 3, 7)
    obs = np.stack([exact.simulate_hmm(T, 1000 + b) for b in range(B)])
    seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
    model = cp.MODEL_HMM3 if args.model == "hmm3" else cp.MODEL_HMM_TABLE
    eu, eh = cp.Engine(0), cp.Engine(0)
    for e in (eu, eh):
        e.set_hmm(means[0], trans[0])
    for keep in keeps:
        begin_ms = timed(lambda: eu.batch_begin(model, obs, n, keep_history=keep), args.inner) * 1e3
        eh.batch_begin_problems(model, list(obs), n, keep_history=keep)

        def run(e):
            e.batch_run(seeds)
            e.sync()
        r = alternate({"uniform": lambda: run(eu), "problems": lambda: run(eh)}, args.reps, args.inner)
        same = all(np.array_equal(x, y) for x, y in zip(eu.batch_results()[1:], eh.batch_results()[1:]))
        emit(dict(cell="uniform", model=args.model, B=B, n=n, T=T, keep_history=int(keep), begin_ms=begin_ms, uniform_ms=r["uniform"][0], uniform_spread_ms=r["uniform"][1],
                  problems_ms=r["problems"][0], problems_spread_ms=r["problems"][1], results_equal=bool(same)))
    eu.close()
    eh.close()


def cell_order(cp, args, emit):
    """The skewed batch in the dispatch order the loaded library gives it (compare two builds with --libs)."""
    B = 1024
    rng = np.random.default_rng(3)
    Ts = np.exp(rng.uniform(np.log(4.0), np.log(128.0), B)).astype(int)
    ns = rng.choice([512, 4096], B)
    means, trans = tables(B, 3, 5)
    obs = [means[b][rng.integers(0, 3, Ts[b])] + rng.standard_normal(Ts[b]) for b in range(B)]
    seeds = np.arange(B, dtype=np.uint64)
    e = cp.Engine(0)
    for keep in (True, False):
        e.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans), keep_history=keep)

        def run():
            e.batch_run(seeds)
            e.sync()
        r = alternate({"skewed": run}, args.reps, args.inner)
        lz = float(sum(x["log_evidence"] for x in e.batch_results()[0]))
        emit(dict(cell="order", B=B, keep_history=int(keep), particle_steps=int((Ts * ns).sum()), skewed_ms=r["skewed"][0], skewed_spread_ms=r["skewed"][1],
                  log_evidence_sum=lz))
    e.close()


def cell_buys(cp, args, emit):
    from oracle import exact
    B, T = 1024, 16
    means, trans = tables(B, 3, 11)
    obs = exact.simulate_hmm(T, 99)
    seeds = np.arange(B, dtype=np.uint64)
    S = min(B, args.sample)
    e = cp.Engine(0)
    for n in (1024, 4096):
        parts = {}

        def batch():
            t0 = time.perf_counter()
            e.batch_begin_problems(cp.MODEL_HMM_TABLE, [obs] * B, n, tables=(means, trans), keep_history=False)
            t1 = time.perf_counter()
            e.batch_run(seeds)
            e.sync()
            t2 = time.perf_counter()
            out = e.batch_results()
            parts["begin_ms"], parts["run_ms"], parts["results_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3
            return out

        def one_by_one():
            lz = []
            for b in range(S):
                e.set_hmm(means[b], trans[b])
                e.batch_begin(cp.MODEL_HMM_TABLE, obs[None, :], n, keep_history=False)
                e.batch_run(seeds[b:b + 1])
                lz.append(e.batch_results()[0][0]["log_evidence"])
            return lz
        r = alternate({"batch": batch, "one_by_one": one_by_one}, args.reps, 1)
        lz_b = [s["log_evidence"] for s in batch()[0]][:S]
        worst = float(np.abs(np.array(lz_b) - np.array(one_by_one())).max())
        scale = B / S
        emit(dict(cell="buys", B=B, n=n, T=T, batch_ms=r["batch"][0], batch_spread_ms=r["batch"][1], one_by_one_ms=r["one_by_one"][0] * scale,
                  one_by_one_spread_ms=r["one_by_one"][1] * scale, sampled_tables=S, ratio=r["one_by_one"][0] * scale / r["batch"][0],
                  log_evidence_max_abs_diff=worst, **parts))
    e.close()


def across_libs(args, emit):
    """The cells in child processes that load the builds of `--libs` in alternation, `--reps` times; per build and cell row the median
    and the spread over the repeats of every *_ms figure."""
    got = {lib: [] for lib in args.libs}
    for _ in range(args.reps):
        for lib in args.libs:
            env = dict(os.environ, CPPROB_HIP_LIB=lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--cells"] + args.cells + ["--model", args.model, "--reps", "1", "--inner", str(args.inner), "--sample", str(args.sample)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode:
                raise RuntimeError("child with %s failed (%d): %s" % (lib, p.returncode, p.stderr[-2000:]))
            got[lib].append([json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")])
    for lib, runs in got.items():
        for i, row in enumerate(runs[0]):
            out = {k: v for k, v in row.items() if not k.endswith("_ms")}
            for k in row:
                if k.endswith("_ms") and not k.endswith("_spread_ms"):
                    v = [r[i][k] for r in runs]
                    out[k] = float(np.median(v))
                    out[k[:-3] + "_spread_ms"] = max(v) - min(v)
            out["lib"] = os.path.basename(lib)
            emit(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", nargs="+", default=["uniform", "order", "buys"])
    ap.add_argument("--model", choices=["table", "hmm3"], default="table", help="the uniform cell's model")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sample", type=int, default=128)
    ap.add_argument("--libs", nargs="+", default=None)
    args = ap.parse_args()

    def emit(d):
        print(json.dumps(d), flush=True)
    if args.libs:
        across_libs(args, emit)
        return
    rest = args.cells
    if rest:
        import torch  # noqa: F401  (first: shares libamdhip64 with the library)
        import cpprob_amd as cp
        for c in rest:
            {"uniform": cell_uniform, "order": cell_order, "buys": cell_buys}[c](cp, args, emit)


if __name__ == "__main__":
    main()
