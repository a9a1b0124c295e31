#!/usr/bin/env python3
"""A/B of the folded trace-word read-out (step_counts.hpp: step_fold_tail) against the two-launch form
(FLAG_SEPARATE_TRACE_READOUT), hmm<16> SMC, systematic resampling every step: both forms alternated in one process, best of
`--passes` passes of `--runs` back-to-back runs each (wall clock over the enqueued runs, as bench.py times them).
usage: python tools/ab_fold_readout.py [--sizes 100000,1000000,...] [--runs 50] [--passes 3] [--filter-only-at 1000000]
Prints one JSON line per (size, keep_history)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401
import cpprob_amd as cp  # noqa: E402

SEP = cp.capi.FLAG_SEPARATE_TRACE_READOUT


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="100000,1000000,4000000,10000000")
    p.add_argument("--runs", type=int, default=50)
    p.add_argument("--passes", type=int, default=3)
    p.add_argument("--filter-only-at", default="1000000", help="sizes also timed with keep_history=False (comma list, empty: none)")
    a = p.parse_args()
    obs = np.load(os.path.join(ROOT, "tests", "golden", "observations.npz"))["hmm16"]
    engs = {name: cp.Engine(0) for name in ("folded", "separate")}
    cases = [(int(n), True) for n in a.sizes.split(",") if n] + [(int(n), False) for n in a.filter_only_at.split(",") if n]
    for n, keep in cases:
        for name, eng in engs.items():
            eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=12345, resampler=cp.RESAMPLE_SYSTEMATIC, ess_threshold=2.0,
                      keep_history=keep, flags=0 if name == "folded" else SEP)
            for i in range(5):
                eng.run(i)
            eng.sync()
        times = {name: [] for name in engs}
        for ps in range(a.passes):
            for name, eng in (engs.items() if ps % 2 == 0 else reversed(list(engs.items()))):
                eng.sync()
                t0 = time.perf_counter()
                for i in range(a.runs):
                    eng.run(1000 + ps * a.runs + i)
                eng.sync()
                times[name].append((time.perf_counter() - t0) / a.runs * 1e3)
        res = {"n": n, "keep_history": keep, "runs": a.runs, "passes": a.passes}
        for name, ts in times.items():
            res[name + "_ms_best"] = round(min(ts), 5)
            res[name + "_ms_spread"] = round(max(ts) - min(ts), 5)
            res[name + "_ms_all"] = [round(x, 5) for x in ts]
        res["gain_us"] = round((res["separate_ms_best"] - res["folded_ms_best"]) * 1e3, 2)
        res["gain_pct"] = round(100.0 * (1.0 - res["folded_ms_best"] / res["separate_ms_best"]), 2)
        print(json.dumps(res), flush=True)
    for eng in engs.values():
        eng.close()


if __name__ == "__main__":
    main()
