#!/usr/bin/env python3
"""The posterior traces of a batch (cpprob_hip_batch_paths_device; csrc/batch_paths.hpp) against the run they follow and against the
old route to the same arrays (profiles/r13_notes.md).  Shapes: B = 1024, n = 1024, T = 64 and B = 8, n = 8192, T = 128, both models.
Device-synchronised wall time; every form is warmed up, then timed `--reps` times in alternation, and the median and the spread
(max - min) over the repeats are reported.  Per cell:
  run_ms               batch_run of the begun batch (begin not counted), synchronised
  paths_device_ms      batch_paths_device into tensors made beforehand (all particles), synchronised
  paths_device_100_ms  the same for the first 100 traces of every problem (max_particles = 100)
  run_then_paths_ms    both enqueued back to back, one synchronisation
  paths_host_ms        batch_paths: the same launch, then the copy to the host and the widening to int32
  store_walk_ms        the old route: B batch_store calls (a synchronisation each) and oracle.lineage + take_along_axis on the host
usage: python tools/bench_batch_paths.py [--models hmm3 table] [--shapes 1024x1024x64 8x8192x128] [--reps 5]
One JSON line per cell."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternate(forms, reps):
    """forms: {name: callable}.  {name: (median ms, spread ms)} of their wall times."""
    def once(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3
    for f in forms.values():
        f()
    got = {k: [] for k in forms}
    for _ in range(reps):
        for k, f in forms.items():
            got[k].append(once(f))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", choices=["hmm3", "table"], default=["hmm3", "table"])
    ap.add_argument("--shapes", nargs="+", default=["1024x1024x64", "8x8192x128"], help="BxNxT")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch  # (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    from oracle import exact
    from oracle import oracle as O
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-2.0, 2.0, 3))
    trans = rng.uniform(0.05, 1.0, (3, 3))
    e = cp.Engine(0)
    e.set_hmm(means, trans)
    for shape in args.shapes:
        B, n, T = (int(x) for x in shape.split("x"))
        obs = np.stack([exact.simulate_hmm(T, 1000 + b) for b in range(B)])
        seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
        for name in args.models:
            model = cp.MODEL_HMM3 if name == "hmm3" else cp.MODEL_HMM_TABLE
            e.batch_begin(model, obs, n)
            first, wfirst = cp.capi.batch_paths_layout([T] * B, n)
            first_c, wfirst_c = cp.capi.batch_paths_layout([T] * B, n, 100)
            d_paths = torch.zeros(int(first[-1]), dtype=torch.int8, device="cuda:0")
            d_logw = torch.zeros(int(wfirst[-1]), dtype=torch.float64, device="cuda:0")
            torch.cuda.current_stream().synchronize()

            def run():
                e.batch_run(seeds)
                e.sync()

            def paths_device():
                e.batch_paths_device(d_paths, d_logw)
                e.sync()

            def paths_device_100():
                e.batch_paths_device(d_paths[:int(first_c[-1])], d_logw[:int(wfirst_c[-1])], max_particles=100)
                e.sync()

            def run_then_paths():
                e.batch_run(seeds)
                e.batch_paths_device(d_paths, d_logw)
                e.sync()

            def paths_host():
                return e.batch_paths()

            def store_walk():
                out = []
                for b in range(B):
                    vals, anc, logw = e.batch_store(b)
                    out.append((np.take_along_axis(vals, O.lineage(anc), axis=1), logw))
                return out

            run()
            r = alternate({"run": run, "paths_device": paths_device, "paths_device_100": paths_device_100, "run_then_paths": run_then_paths,
                           "paths_host": paths_host, "store_walk": store_walk}, args.reps)
            # the two routes give the same arrays, exactly
            new_p, new_w = paths_host()
            same = all(np.array_equal(p, q) and np.array_equal(w, v) for (p, w), q, v in zip(store_walk(), new_p, new_w))
            paths_device()
            same = same and np.array_equal(d_paths.cpu().numpy().astype(np.int32), np.concatenate([p.reshape(-1) for p in new_p]))
            row = dict(model=name, B=B, n=n, T=T, routes_equal=bool(same), entries=int(first[-1]))
            for k, (med, spread) in r.items():
                row[k + "_ms"], row[k + "_spread_ms"] = med, spread
            row["paths_over_run"] = r["paths_device"][0] / r["run"][0]
            print(json.dumps(row), flush=True)
    e.close()


if __name__ == "__main__":
    main()
