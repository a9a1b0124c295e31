#!/usr/bin/env python3
"""A/B of the run lanes (include/cpprob_hip.h: cpprob_hip_infer_lanes) against one-at-a-time runs (FLAG_SERIAL_RUNS): both forms in one
process and on ONE context, begun again with the other form pass by pass (a second context would hold a stream of its own: with the
lanes' three that is every hardware queue a process opens, and the lanes then measure ~0.104 ms instead of ~0.076 at 10^6,
profiles/r11_notes.md), best of `passes` passes of `runs` back-to-back runs each (wall clock from the first enqueue to the sync
behind the last run, as bench.py times them).  Per case also: the host's enqueue time per run (the calls' own duration, before
the sync) and the one-at-a-time pattern run -> results() -> run, which must cost the same in both forms (it never leaves lane 0).
usage: python tools/ab_run_lanes.py [--cases hmm16:100000,hmm16:1000000,...] [--runs 50] [--passes 3] [--runs-at-1e6 200] [--passes-at-1e6 5]
Prints one JSON line per case.  The library's lane depth is a build constant: run this under CPPROB_HIP_LIB=<another build> to
compare depths (the serial form of the same process is the common yardstick)."""
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

SERIAL = cp.capi.FLAG_SERIAL_RUNS
DEFAULT = "hmm16:100000,hmm16:1000000,hmm16:4000000,hmm16:10000000,hmm128_ess:1250000,lgssm100:1250000"


def spec(name, z):
    if name == "hmm16":
        return cp.MODEL_HMM3, z["hmm16"], 2.0
    if name == "hmm128_ess":
        return cp.MODEL_HMM3, z["hmm128"], 0.5
    if name == "lgssm100":
        return cp.MODEL_LINEAR_GAUSSIAN_1D, z["lgssm100"], 0.5
    raise SystemExit("unknown workload %s" % name)


def timed(eng, runs, first):
    eng.sync()
    t0 = time.perf_counter()
    for i in range(runs):
        eng.run(first + i)
    t1 = time.perf_counter()
    eng.sync()
    t2 = time.perf_counter()
    return (t2 - t0) / runs * 1e3, (t1 - t0) / runs * 1e3


def timed_one_at_a_time(eng, runs, first):
    eng.sync()
    t0 = time.perf_counter()
    for i in range(runs):
        eng.run(first + i)
        eng.results()
    return (time.perf_counter() - t0) / runs * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cases", default=DEFAULT)
    p.add_argument("--runs", type=int, default=50)
    p.add_argument("--passes", type=int, default=3)
    p.add_argument("--runs-at-1e6", type=int, default=200)
    p.add_argument("--passes-at-1e6", type=int, default=5)
    a = p.parse_args()
    z = np.load(os.path.join(ROOT, "tests", "golden", "observations.npz"))
    eng = cp.Engine(0)
    forms = ("lanes", "serial")
    for case in a.cases.split(","):
        name, n = case.split(":")
        n = int(n)
        model, obs, ess = spec(name, z)
        runs, passes = (a.runs_at_1e6, a.passes_at_1e6) if (name == "hmm16" and n == 1_000_000) else (a.runs, a.passes)
        def begin(form):
            eng.begin(cp.ALG_SMC, model, obs, n, seed=12345, resampler=cp.RESAMPLE_SYSTEMATIC, ess_threshold=ess, flags=0 if form == "lanes" else SERIAL)
            for i in range(8):                       # (warm: every lane begun again and run)
                eng.run(i)
            eng.sync()
        times = {f: [] for f in forms}
        enq = {f: [] for f in forms}
        single = {f: [] for f in forms}
        last = {}
        info = None
        for ps in range(passes):
            for form in (forms if ps % 2 == 0 else forms[::-1]):
                begin(form)
                t, e = timed(eng, runs, 1000 + ps * runs)
                times[form].append(t)
                enq[form].append(e)
                if form == "lanes":
                    info = eng.lanes()
                last[form] = eng.stats()
                single[form].append(timed_one_at_a_time(eng, min(runs, 50), 5000 + ps * runs))
        same = bool(np.array_equal(last["lanes"], last["serial"]))
        res = {"workload": name, "n": n, "T": int(len(obs)), "tiles": (n + 1023) // 1024, "runs": runs, "passes": passes, "depth": info["depth"],
               "serial_reason": info["serial_reason"], "lane_bytes": info["lane_bytes"], "last_results_equal": same}
        for f in forms:
            res[f + "_ms_best"] = round(min(times[f]), 5)
            res[f + "_ms_spread"] = round(max(times[f]) - min(times[f]), 5)
            res[f + "_ms_all"] = [round(x, 5) for x in times[f]]
            res[f + "_enqueue_ms_per_run"] = round(min(enq[f]), 5)
            res[f + "_one_at_a_time_ms_best"] = round(min(single[f]), 5)
            res[f + "_one_at_a_time_ms_spread"] = round(max(single[f]) - min(single[f]), 5)
        res["gain_us"] = round((res["serial_ms_best"] - res["lanes_ms_best"]) * 1e3, 2)
        res["gain_pct"] = round(100.0 * (1.0 - res["lanes_ms_best"] / res["serial_ms_best"]), 2)
        res["gain_over_3x_spread"] = bool(res["serial_ms_best"] - res["lanes_ms_best"] > 3 * max(res["lanes_ms_spread"], res["serial_ms_spread"]))
        print(json.dumps(res), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
