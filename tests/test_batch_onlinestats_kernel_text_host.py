"""batch_online_stats_kernel (csrc/batch_onlinestats.hpp) as host code: the translation unit is formed here from the text of
csrc/batch_smooth.hpp (as tests/test_batch_suffstats_kernel_text_host.py forms it) and csrc/batch_onlinestats.hpp (its include line
naming that text), built against tests/host_kernels/batch_smooth_shim.hpp as a stand-alone program with g++ -O1
-fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_onlinestats_main.cpp) and run
over grids from one workgroup to one per kWaves problems.  Every buffer has exactly the size the host code hands the kernel, the rows of
the m table no problem has reached AT THAT CALL are NaN, tau of a problem that has consumed nothing is NaN on the way in, and the
records and tau must equal tests/onlinestats_ref.py's bit for bit (host division is IEEE) on every grid, call after call: each call
resumes from the tau the call before it stored.  Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 9 int64 {magic, B, k, thr_stride, gridDim.x, rows of the m table, threshold words, observes, 1: the
observes are passed}, then the descriptors, the thresholds, the m table, the observes and tau [B][8][88].  The output: the records
[B][88], then tau."""
import os
import re
import subprocess

import numpy as np
import pytest

import onlinestats_ref as N
import test_batch_suffstats_kernel_text_host as K
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b4f4e4c494e3031
TAU = 8 * N.RECORD


def _texts():
    """(csrc/batch_smooth.hpp, csrc/batch_onlinestats.hpp) with their textual changes; each must find its line exactly once."""
    smooth = K._texts()[0]
    text = open(os.path.join(CSRC, "batch_onlinestats.hpp")).read()
    inc = '#include "batch_smooth.hpp"'
    assert text.count(inc) == 1 and text.count("#include") == 1
    code = re.sub(r"//[^\n]*", "", text)
    for word in ("__shared__", "__syncthreads", "atomic"):
        assert word not in code, "the running statistics kernel uses no LDS, no barrier and no atomics: " + word
    return smooth, text.replace(inc, '#include "batch_smooth_host.hpp"')


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_onlinestats_host"))
    smooth, text = _texts()
    open(os.path.join(d, "batch_smooth_host.hpp"), "w").write(smooth)
    open(os.path.join(d, "batch_onlinestats_host.hpp"), "w").write(text)
    so = O.build()
    exe = os.path.join(d, "batch_onlinestats_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_onlinestats_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(bt, grid_x, done, lens, tau, with_obs=True):
        """One call on a grid of grid_x workgroups: problem b has consumed done[b] steps and has reached lens[b]; tau [B, 704] as
        the call before left it.  Returns (records [B, 88], tau [B, 704])."""
        desc = np.zeros(bt.B, K.DESC)
        obs, at = [], 0
        mass = bt.mass.copy()
        for b, (d0, L) in enumerate(zip(done, lens)):
            desc[b] = (L, 1, 0, bt.rows[b], at, 0, L, d0, 0)
            obs.append(bt.obs[b][d0:L])
            at += L - d0
            mass[bt.rows[b] + L:bt.rows[b + 1]] = np.nan
        obs = np.concatenate(obs)
        head = np.array([MAGIC, bt.B, bt.k, bt.thr_stride, grid_x, mass.shape[0], bt.thr.size, obs.size, 1 if with_obs else 0], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            for arr, dt in ((desc, K.DESC), (bt.thr, np.uint64), (mass, np.float64), (obs, np.float64), (tau, np.float64)):
                f.write(np.ascontiguousarray(arr, dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = np.frombuffer(open(fout, "rb").read(), np.float64)
        assert raw.size == bt.B * (N.RECORD + TAU)
        return raw[:bt.B * N.RECORD].reshape(bt.B, N.RECORD), raw[bt.B * N.RECORD:].reshape(bt.B, TAU)
    return run


def walk(prog, bt, grid_x, schedule, with_obs=True):
    """The calls of `schedule` (the lengths reached at each) on the program and on the reference, compared after every call."""
    runs = [N.Running() for _ in range(bt.B)]
    tau = np.full((bt.B, TAU), np.nan)                          # (a problem that has consumed nothing: never read)
    done = [0] * bt.B
    for lens in schedule:
        got, tau_out = prog(bt, grid_x, done, lens, tau, with_obs)
        for b, L in enumerate(lens):
            runs[b].consume(bt.m[b][:L], bt.P[b], bt.obs[b] if with_obs else None)
            want = N.as_array(runs[b].read(bt.m[b][:L]))
            assert np.array_equal(got[b], want), "grid %d, lengths %s, problem %d: largest difference %.3g" % (grid_x, lens, b, np.nanmax(np.abs(got[b] - want)))
            if L > 0:
                assert np.array_equal(tau_out[b], np.array(runs[b].tau).reshape(-1)), "grid %d, lengths %s, problem %d: tau" % (grid_x, lens, b)
            else:
                assert np.all(np.isnan(tau_out[b])), "a problem of length 0 stores no tau"
        tau, done = tau_out.copy(), list(lens)
    return runs


TS = [0, 1, 2, 7, 64, 7, 64]                    # seven problems: the last workgroup of four holds three


@pytest.fixture(scope="module", params=["hmm3", "table2", "table5", "table8"])
def batch(request):
    ns = [5, 3, 1, 70, 300, 40, 9]
    if request.param == "hmm3":
        return K.Batch(TS, ns, 3, True, 5, rare=5)
    k = int(request.param[5:])
    return K.Batch(TS, ns, k, False, 7 + k, rare=5)


def test_every_grid_gives_the_references_bits_call_after_call(prog, batch):
    """gridDim.x in {1, 2}: a wavefront walks two problems or one.  Three calls: the first consumes a few steps, the second resumes
    from the stored tau (some problems with no new steps: the read-out alone), the third is a repeat with nothing new."""
    first = [0, 1, 1, 3, 5, 0, 64]
    for gx in (1, 2):
        runs = walk(prog, batch, gx, [first, TS, TS])
        assert np.all(np.array(runs[0].tau) == 0.0)
    rare = np.array(batch.m[5])[:, batch.k - 1]
    assert np.sum(rare == 0) >= 4 and np.any(rare > 0), "the last state of problem 5 should be absent from most generations"


def test_one_call_equals_many(prog, batch):
    whole = walk(prog, batch, 2, [TS])
    steps = walk(prog, batch, 1, [[min(T, L) for T in TS] for L in (1, 2, 3, 4, 5, 6, 7)] + [TS])
    for a, b in zip(whole, steps):
        assert np.array_equal(np.array(a.tau), np.array(b.tau))


def test_no_observes_leaves_the_weighted_sums_zero(prog, batch):
    runs = walk(prog, batch, 2, [TS], with_obs=False)
    for b, run in enumerate(runs):
        rec = N.as_array(run.read(batch.m[b]))
        assert np.all(rec[72:] == 0.0)


def test_table_addressed_by_capacity(prog):
    """An online batch: rows by capacity, lengths reached below them, a problem still at length 0 between two that are not."""
    bt = K.Batch([23, 9, 5], [70, 1, 300], 5, False, 11, caps=[25, 12, 8])
    for gx in (1, 3):
        walk(prog, bt, gx, [[5, 0, 1], [6, 9, 1], [6, 9, 1], [23, 9, 5]])
