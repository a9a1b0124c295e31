#!/usr/bin/env python3
"""What a learning advance of an online batch costs (cpprob_hip_batch_advance_learn; csrc/batch_learn.hpp) next to a plain advance and
next to the host-stepped route it replaces.  Shape: B = 1024 streams of k = 8 states, n = 256 particles, chunk in {1, 16} observes an
advance; per-problem tables; a filtering-only batch that keeps its masses.  Device-synchronised wall time: every form has a stream of
its own with room for `--reps` + 1 advances, the forms are timed in alternation, the first repetition is left out, and the median and
the spread (max - min) of the others are reported.  Per chunk:
  learn_ms          batch_advance_learn (rows on the device, the run, the learn step), then sync()
  plain_ms          batch_advance of the same chunk, then sync() (what the feature may not slow down)
  host_stepped_ms   batch_advance, batch_online_stats, cpprob_amd.m_step on the host, batch_online_tables, then sync()
The advances hand over flat arrays prepared before the clock starts (the ctypes calls themselves), so that a chunk of one observe is
not measured as numpy's concatenation of 1024 pieces; the host-stepped route's statistics call goes through the Engine as a user's would.
--package-root DIR measures the cpprob_amd package of another checkout of this project (built there), e.g. the parent commit's: the
forms its Engine does not know are left out, so plain_ms of two checkouts can be set side by side.
--forms plain measures the named forms alone: the plain advance of two checkouts is compared with nothing else in the process.
usage: python tools/bench_batch_learn.py [--chunk 1 16] [--reps 21] [--package-root DIR] [--forms plain learn host_stepped]
One JSON line per chunk."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", nargs="+", type=int, default=[1, 16])
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--forms", nargs="+", default=["plain", "learn", "host_stepped"])
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repeats")
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch  # noqa: F401  (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    has = hasattr(cp.Engine, "batch_advance_learn")
    B, n, k = args.B, args.n, args.k
    rng = np.random.default_rng(1)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    trans /= trans.sum(-1, keepdims=True)
    seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
    p32 = C.POINTER(C.c_uint32)
    for chunk in args.chunk:
        steps = args.reps + 1
        cap = chunk * steps
        obs = means[np.arange(B)[:, None], rng.integers(0, k, (B, cap))] + rng.standard_normal((B, cap))
        flats = [np.ascontiguousarray(obs[:, i * chunk:(i + 1) * chunk]).reshape(-1) for i in range(steps)]
        pieces = [[obs[b, i * chunk:(i + 1) * chunk] for b in range(B)] for i in range(steps)]
        h_dT = np.full(B, chunk, np.uint32)
        engines = {}

        def stream(name, arm):
            e = engines[name] = cp.Engine(0)
            e.batch_begin_online(cp.MODEL_HMM_TABLE, [cap] * B, n, seeds, tables=(means, trans), keep_history=False, keep_masses=True)
            if arm:
                e.batch_learn_begin(cp.online_em.step_sizes(cap, 0.6), 1)
            return e

        def plain(i, e):
            e._chk(e.L.cpprob_hip_batch_advance(e.h, h_dT.ctypes.data_as(p32), flats[i].ctypes.data, 1))
            e.sync()

        def learn(i, e):
            e._chk(e.L.cpprob_hip_batch_advance_learn(e.h, h_dT.ctypes.data_as(p32), flats[i].ctypes.data))
            e.sync()

        state = {"tables": (means, trans)}

        def host_stepped(i, e):
            e._chk(e.L.cpprob_hip_batch_advance(e.h, h_dT.ctypes.data_as(p32), flats[i].ctypes.data, 1))
            stats = e.batch_online_stats(pieces[i])
            state["tables"] = cp.m_step(stats, *state["tables"])
            e.batch_online_tables(state["tables"])
            e.sync()
        forms = {}
        if "plain" in args.forms:
            forms["plain"] = (plain, stream("plain", False))
        if has and "learn" in args.forms:
            forms["learn"] = (learn, stream("learn", True))
        if has and "host_stepped" in args.forms:
            forms["host_stepped"] = (host_stepped, stream("host_stepped", False))
        got = {name: [] for name in forms}
        for i in range(steps):
            for name, (f, e) in forms.items():
                t0 = time.perf_counter()
                f(i, e)
                got[name].append((time.perf_counter() - t0) * 1e3)
        row = dict(B=B, n=n, k=k, chunk=chunk, reps=args.reps, package=os.path.abspath(args.package_root), learn=has)
        for name, v in got.items():
            v = v[1:]                                               # (the first repetition: allocations and the first launches)
            row[name + "_ms"], row[name + "_spread_ms"] = round(float(np.median(v)), 4), round(float(max(v) - min(v)), 4)
        print(json.dumps(row), flush=True)
        for e in engines.values():
            e.close()


if __name__ == "__main__":
    main()
