#!/usr/bin/env python3
"""What a tied learning advance of an online batch costs (cpprob_hip_batch_learn_tie; csrc/batch_learn_tied.hpp) next to the untied
learning advance, the plain advance and the host-stepped route it replaces.  Shape: B = 1024 streams of k = 8 states, n = 256
particles, chunk in {1, 16} observes an advance, G groups of B / G streams each (the tables equal within a group); a filtering-only
batch that keeps its masses.  Device-synchronised wall time, measured as tools/bench_batch_learn.py measures: every form has a stream of
its own with room for `--reps` + 1 advances, the forms are timed in alternation, the first repetition is left out, and the median and
the spread (max - min) of the others are reported.  Per chunk:
  tied_G<g>_ms      batch_advance_learn on a tied learner of g groups (rows, the run, learn, pool, the group M-step), then sync()
  learn_ms          the untied batch_advance_learn, then sync()
  plain_ms          batch_advance of the same chunk, then sync()
  host_tied_ms      batch_advance, batch_online_stats, cpprob_amd.em.pool_stats and cpprob_amd.m_step on the host,
                    batch_online_tables, then sync() -- G = --host-groups
The advances hand over flat arrays prepared before the clock starts.
usage: python tools/bench_batch_learn_tied.py [--chunk 1 16] [--reps 21] [--groups 1024 128 1] [--host-groups 128]
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
    ap.add_argument("--groups", nargs="+", type=int, default=[1024, 128, 1])
    ap.add_argument("--host-groups", type=int, default=128)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repeats")
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: shares libamdhip64 with the library)
    import cpprob_amd as cp
    B, n, k = args.B, args.n, args.k
    if any(B % g for g in args.groups + [args.host_groups]):
        ap.error("every group count divides B")
    rng = np.random.default_rng(1)
    seeds = np.arange(1000, 1000 + B, dtype=np.uint64)
    p32 = C.POINTER(C.c_uint32)

    def tables(G):
        means = np.sort(rng.uniform(-3.0, 3.0, (G, k)), axis=1) + 0.5 * np.arange(k)
        trans = rng.uniform(0.05, 1.0, (G, k, k))
        trans /= trans.sum(-1, keepdims=True)
        ids = np.arange(B, dtype=np.int32) % G                         # (the memberships interleaved)
        return ids, (np.ascontiguousarray(means[ids]), np.ascontiguousarray(trans[ids]))
    for chunk in args.chunk:
        steps = args.reps + 1
        cap = chunk * steps
        base = tables(B)[1]
        obs = base[0][np.arange(B)[:, None], rng.integers(0, k, (B, cap))] + rng.standard_normal((B, cap))
        flats = [np.ascontiguousarray(obs[:, i * chunk:(i + 1) * chunk]).reshape(-1) for i in range(steps)]
        pieces = [[obs[b, i * chunk:(i + 1) * chunk] for b in range(B)] for i in range(steps)]
        h_dT = np.full(B, chunk, np.uint32)
        gamma = cp.online_em.step_sizes(cap, 0.6)
        engines = []

        def stream(tabs, ids=None, arm=False):
            e = cp.Engine(0)
            engines.append(e)
            e.batch_begin_online(cp.MODEL_HMM_TABLE, [cap] * B, n, seeds, tables=tabs, keep_history=False, keep_masses=True)
            if ids is not None:
                e.batch_tie(ids)
            if arm:
                e.batch_learn_begin(gamma, 1, tied=ids is not None)
            return e

        def plain(i, e, st):
            e._chk(e.L.cpprob_hip_batch_advance(e.h, h_dT.ctypes.data_as(p32), flats[i].ctypes.data, 1))
            e.sync()

        def learn(i, e, st):
            e._chk(e.L.cpprob_hip_batch_advance_learn(e.h, h_dT.ctypes.data_as(p32), flats[i].ctypes.data))
            e.sync()

        def host_tied(i, e, st):
            e._chk(e.L.cpprob_hip_batch_advance(e.h, h_dT.ctypes.data_as(p32), flats[i].ctypes.data, 1))
            stats = cp.em.pool_stats(e.batch_online_stats(pieces[i]), st["ids"])
            st["tables"] = cp.m_step(stats, *st["tables"])
            e.batch_online_tables(st["tables"])
            e.sync()
        forms = {"plain": (plain, stream(base), {}), "learn": (learn, stream(base, arm=True), {})}
        for G in args.groups:
            ids, tabs = tables(G)
            forms["tied_G%d" % G] = (learn, stream(tabs, ids, arm=True), {})
        ids, tabs = tables(args.host_groups)
        forms["host_tied"] = (host_tied, stream(tabs, ids), {"tables": tabs, "ids": ids})
        got = {name: [] for name in forms}
        for i in range(steps):
            for name, (f, e, st) in forms.items():
                t0 = time.perf_counter()
                f(i, e, st)
                got[name].append((time.perf_counter() - t0) * 1e3)
        row = dict(B=B, n=n, k=k, chunk=chunk, reps=args.reps, host_groups=args.host_groups)
        for name, v in got.items():
            v = v[1:]                                               # (the first repetition: allocations and the first launches)
            row[name + "_ms"], row[name + "_spread_ms"] = round(float(np.median(v)), 4), round(float(max(v) - min(v)), 4)
        print(json.dumps(row), flush=True)
        for e in engines:
            e.close()


if __name__ == "__main__":
    main()
