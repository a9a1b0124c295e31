"""batch_smooth_stats_kernel (csrc/batch_suffstats.hpp) as host code: the translation unit is formed here from the text of
csrc/batch_smooth.hpp and csrc/batch_suffstats.hpp (the former as tests/test_batch_smooth_kernel_text_host.py forms it, the latter's
include line naming that text), built against tests/host_kernels/batch_smooth_shim.hpp as a stand-alone program with g++ -O1
-fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_suffstats_main.cpp) and run
over grids from one workgroup to one a problem.  Every buffer has exactly the size the host code hands the kernel, rows of the m table
no problem has reached are NaN, and the records must equal tests/suffstats_ref.py's bit for bit (host division is IEEE) on every grid.
Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 9 int64 {magic, B, k, thr_stride, gridDim.x, rows of the m table, threshold words, observes, 1: the
observes are passed}, then the descriptors, the thresholds, the m table and the observes.  The output: the records [B][88]."""
import os
import re
import subprocess

import numpy as np
import pytest

import backward_ref as R
import suffstats_ref as S
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b53544154533031
DESC = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8"), ("rows", "<i8"), ("trows", "<i8"), ("cfrom", "<i4"), ("cto", "<i4"), ("lo", "<i4"), ("mfrom", "<i4")])
K_WAVES = 4


def _texts():
    """(csrc/batch_smooth.hpp, csrc/batch_suffstats.hpp) with their textual changes; each must find its line exactly once."""
    smooth = open(os.path.join(CSRC, "batch_smooth.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert smooth.count(inc) == 1
    smooth = smooth.replace(inc, '#include "batch_smooth_shim.hpp"')
    lds = re.findall(r"^[ \t]*extern __shared__[^\n;]*\bs_mass\[\];", smooth, re.M)
    assert len(lds) == 1 and smooth.count("extern __shared__") == 1, lds
    smooth = smooth.replace(lds[0], "    double* s_mass = hostk::dynamic_lds();")
    stats = open(os.path.join(CSRC, "batch_suffstats.hpp")).read()
    inc = '#include "batch_smooth.hpp"'
    assert stats.count(inc) == 1 and stats.count("#include") == 1
    code = re.sub(r"//[^\n]*", "", stats)
    for word in ("__shared__", "__syncthreads", "atomic"):
        assert word not in code, "the statistics kernel uses no LDS, no barrier and no atomics: " + word
    return smooth, stats.replace(inc, '#include "batch_smooth_host.hpp"')


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_suffstats_host"))
    smooth, stats = _texts()
    open(os.path.join(d, "batch_smooth_host.hpp"), "w").write(smooth)
    open(os.path.join(d, "batch_suffstats_host.hpp"), "w").write(stats)
    so = O.build()
    exe = os.path.join(d, "batch_suffstats_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_suffstats_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(bt, grid_x, lens=None, with_obs=True):
        """The records [B, 88] of batch `bt` at the lengths reached `lens` on a grid of grid_x workgroups."""
        desc, obs = bt.desc(lens)
        head = np.array([MAGIC, bt.B, bt.k, bt.thr_stride, grid_x, bt.mass.shape[0], bt.thr.size, obs.size, 1 if with_obs else 0], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            for arr, dt in ((desc, DESC), (bt.thr, np.uint64), (bt.mass, np.float64), (obs, np.float64)):
                f.write(np.ascontiguousarray(arr, dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        assert len(raw) == 8 * bt.B * S.RECORD
        return np.frombuffer(raw, np.float64).reshape(bt.B, S.RECORD)
    return run


class Batch:
    """Problems of lengths Ts (capacities caps: an online batch's m table, addressed by capacity) with random states and table rows.
    `rare`: the problem whose last state is absent from four generations in five.  Model HMM_TABLE: a table a problem, the second
    one's with a zero transition entry.  The m table holds NaN wherever no problem has a row."""

    def __init__(self, Ts, ns, k, hmm3, seed, caps=None, rare=None):
        rng = np.random.default_rng(seed)
        self.Ts, self.k, self.hmm3, self.B = list(Ts), k, hmm3, len(Ts)
        self.caps = list(caps) if caps else list(Ts)
        self.rows = np.concatenate([[0], np.cumsum(self.caps)]).astype(np.int64)
        trans = rng.uniform(0.05, 1.0, (1 if hmm3 else self.B, k, k))
        if not hmm3 and self.B > 1:
            trans[1, 0, k - 1] = 0.0
        self.thr = np.full((trans.shape[0], 8, 8), np.iinfo(np.uint64).max, np.uint64)     # (words behind a row's k - 1 entries: all ones)
        for i, tr in enumerate(trans):
            for s, row in enumerate(R.thresholds(tr)):
                self.thr[i, s, :k - 1] = row
        self.thr_stride = 0 if hmm3 else 64
        self.mass = np.full((int(self.rows[-1]), 8), np.nan)
        self.m, self.P, self.obs = [], [], []
        for b, (T, n) in enumerate(zip(self.Ts, ns)):
            v = rng.integers(0, k, (T, n))
            if b == rare:
                keep = np.arange(T) % 5 == 4
                v[~keep] = np.minimum(v[~keep], k - 2)
            ll = -rng.uniform(0.0, 30.0, (T, k))
            m = R.filtering_masses(v, ll.tolist()) if T else []
            self.m.append(m)
            self.P.append(R.transition_masses(trans[0 if hmm3 else b]))
            self.obs.append(rng.uniform(-4.0, 4.0, T))
            self.mass[self.rows[b]:self.rows[b] + T] = 0.0
            if T:
                self.mass[self.rows[b]:self.rows[b] + T, :k] = np.array(m, np.float64)

    def desc(self, lens=None):
        """batch_smooth_enqueue's descriptors of a full call at the lengths reached, and the observes packed by those lengths."""
        lens = self.Ts if lens is None else lens
        d = np.zeros(self.B, DESC)
        at = 0
        for b, L in enumerate(lens):
            d[b] = (L, 1, 0, self.rows[b], at, 0, L, 0, 0)
            at += L
        obs = [self.obs[b][:L] for b, L in enumerate(lens)]
        return d, np.concatenate(obs) if obs else np.zeros(0)

    def want(self, lens=None, with_obs=True):
        lens = self.Ts if lens is None else lens
        return np.stack([S.record(S.stats(self.m[b][:L], self.P[b], self.obs[b][:L] if with_obs else None)) for b, L in enumerate(lens)])


TS = [0, 1, 2, 7, 64, 7, 64]                    # seven problems: the last workgroup of four holds three


@pytest.fixture(scope="module", params=["hmm3", "table2", "table5", "table8"])
def batch(request):
    ns = [5, 3, 1, 70, 300, 40, 9]
    if request.param == "hmm3":
        return Batch(TS, ns, 3, True, 5, rare=5)
    k = int(request.param[5:])
    return Batch(TS, ns, k, False, 7 + k, rare=5)


def test_every_grid_gives_the_references_records(prog, batch):
    """gridDim.x in {1, 2, 7}: a wavefront walks two problems, one or none; the records are the reference's bits on each."""
    want = batch.want()
    assert np.all(want[0] == 0.0) and np.all(want[1, :64] == 0.0) and np.any(want[4, :64] > 0.0)
    rare = np.array(batch.m[5])[:, batch.k - 1]
    assert np.sum(rare == 0) >= 4 and np.any(rare > 0), "the last state of problem 5 should be absent from most generations"
    for gx in (1, 2, 7):
        got = prog(batch, gx)
        assert np.array_equal(got, want), "grid %d: records differ from the reference (largest difference %.3g)" % (gx, np.nanmax(np.abs(got - want)))
    for b in range(batch.B):
        st = S.stats(batch.m[b], batch.P[b], batch.obs[b])
        assert np.all(st["xi"][batch.k:] == 0.0) and np.all(st["xi"][:, batch.k:] == 0.0) and np.all(st["occ"][batch.k:] == 0.0)


def test_no_observes_leaves_the_weighted_sums_zero(prog, batch):
    got = prog(batch, 2, with_obs=False)
    assert np.array_equal(got, batch.want(with_obs=False))
    assert np.all(got[:, 72:] == 0.0) and np.array_equal(got[:, :72], batch.want()[:, :72])


def test_table_addressed_by_capacity(prog):
    """An online batch: rows by capacity, lengths reached below them, a problem still at length 0 between two that are not."""
    bt = Batch([23, 9, 5], [70, 1, 300], 5, False, 11, caps=[25, 12, 8])
    for lens in ([5, 0, 1], [6, 9, 1], [23, 9, 5]):
        want = bt.want(lens)
        for gx in (1, 3):
            assert np.array_equal(prog(bt, gx, lens=lens), want), "lengths %s, grid %d" % (lens, gx)
