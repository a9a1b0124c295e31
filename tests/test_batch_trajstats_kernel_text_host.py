"""batch_traj_stats_kernel (csrc/batch_trajstats.hpp) as host code: the translation unit is formed here from the text of
csrc/batch_smooth.hpp and csrc/batch_trajstats.hpp (the former as tests/test_batch_smooth_kernel_text_host.py forms it, the latter's
include line naming that text and its dynamic LDS array a heap block of the launch's size), built against
tests/host_kernels/batch_smooth_shim.hpp as a stand-alone program with g++ -O1 -fsanitize=address,undefined
-fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_trajstats_main.cpp).  Every buffer has exactly the size the
host code hands the kernel, rows of the m table no problem has reached are NaN, and the records must equal tests/trajstats_ref.py's
applied to tests/backward_ref.py's trajectories, bit for bit.  Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 12 int64 {magic, B, k, thr_stride, n_traj, bytes of dynamic LDS, gridDim.y, rows of the m table, threshold
words, observes, 1: the observes are passed, 1: batch_traj_stats_kernel<3>} and one uint64 (draw_base), then the descriptors, the
thresholds, the seeds, the m table and the observes.  The output: the records [B][n_traj][88]."""
import os
import re
import subprocess

import numpy as np
import pytest

import backward_ref as R
import trajstats_ref as TS
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b54524a53543031
DESC = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8"), ("rows", "<i8"), ("trows", "<i8"), ("cfrom", "<i4"), ("cto", "<i4"), ("lo", "<i4"), ("mfrom", "<i4")])
DRAW_BASE, LDS_MAX, TILE = 1 << 41, 32768, 256


def _texts():
    """(csrc/batch_smooth.hpp, csrc/batch_trajstats.hpp) with their textual changes; each must find its line exactly once."""
    smooth = open(os.path.join(CSRC, "batch_smooth.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert smooth.count(inc) == 1
    smooth = smooth.replace(inc, '#include "batch_smooth_shim.hpp"')
    lds = re.findall(r"^[ \t]*extern __shared__[^\n;]*\bs_mass\[\];", smooth, re.M)
    assert len(lds) == 1 and smooth.count("extern __shared__") == 1, lds
    smooth = smooth.replace(lds[0], "    double* s_mass = hostk::dynamic_lds();")
    traj = open(os.path.join(CSRC, "batch_trajstats.hpp")).read()
    inc = '#include "batch_smooth.hpp"'
    assert traj.count(inc) == 1 and traj.count("#include") == 1
    lds = re.findall(r"^[ \t]*extern __shared__[^\n;]*\bs_tmass\[\];", traj, re.M)
    assert len(lds) == 1 and traj.count("extern __shared__") == 1, lds
    traj = traj.replace(lds[0], "    double* s_tmass = hostk::dynamic_lds();")
    return smooth, traj.replace(inc, '#include "batch_smooth_host.hpp"')


def test_kernel_header_keeps_its_promises():
    """No atomics, one barrier (the staging barrier), fp contract off, 256 trajectories a workgroup, and the two headers the
    kernel-text tests read are as they were: neither names this one."""
    text = open(os.path.join(CSRC, "batch_trajstats.hpp")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "atomic" not in code.lower() and code.count("__syncthreads") == 1
    assert code.count("#pragma clang fp contract(off)") == 1 and re.search(r"[^_\w]fma\s*\(", code) is None
    assert re.search(r"constexpr int kTrajStatsTile = kThreads;", code) and re.search(r"constexpr int kTrajStats = 88;", code)
    staging, walk = code.split("__syncthreads", 1)
    assert "for (int t = T - 1; t >= 0; --t)" in walk and "for (int t" not in staging
    for other in ("batch_smooth.hpp", "batch_suffstats.hpp"):
        assert "traj_stats" not in open(os.path.join(CSRC, other)).read().lower()
    assert '#include "batch_trajstats.hpp"' in open(os.path.join(CSRC, "cpprob_hip.hip")).read()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_trajstats_host"))
    smooth, traj = _texts()
    open(os.path.join(d, "batch_smooth_host.hpp"), "w").write(smooth)
    open(os.path.join(d, "batch_trajstats_host.hpp"), "w").write(traj)
    so = O.build()
    exe = os.path.join(d, "batch_trajstats_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_trajstats_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(bt, n_traj, lens=None, with_obs=True, draw_index=0, lds_bytes=None, idle_tiles=0):
        """The records [B, n_traj, 88] of batch `bt` at the lengths reached `lens`; the dynamic LDS is the host code's
        min(64 * the longest problem, 32768) bytes unless given; idle_tiles: workgroups past the last trajectory."""
        lens = bt.Ts if lens is None else lens
        desc, obs = bt.desc(lens)
        lds = min(64 * max(lens), LDS_MAX) if lds_bytes is None else lds_bytes
        gy = -(-n_traj // TILE) + idle_tiles
        head = np.array([MAGIC, bt.B, bt.k, bt.thr_stride, n_traj, lds, gy, bt.mass.shape[0], bt.thr.size, obs.size, 1 if with_obs else 0, 1 if bt.hmm3 else 0], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            f.write(np.array([DRAW_BASE + (draw_index << 24)], "<u8").tobytes())
            for arr, dt in ((desc, DESC), (bt.thr, np.uint64), (bt.seeds, np.uint64), (bt.mass, np.float64), (obs, np.float64)):
                f.write(np.ascontiguousarray(arr, dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        assert len(raw) == 8 * bt.B * n_traj * TS.RECORD
        return np.frombuffer(raw, np.float64).reshape(bt.B, n_traj, TS.RECORD)
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
        self.seeds = np.array([1000 + 77 * b for b in range(self.B)], np.uint64)
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
        self._traj = {}

    def desc(self, lens):
        """batch_smooth_enqueue's descriptors of a full call at the lengths reached, and the observes packed by those lengths."""
        d = np.zeros(self.B, DESC)
        at = 0
        for b, L in enumerate(lens):
            d[b] = (L, 1, 0, self.rows[b], at, 0, L, 0, 0)
            at += L
        obs = [self.obs[b][:L] for b, L in enumerate(lens)]
        return d, np.concatenate(obs) if obs else np.zeros(0)

    def paths(self, n_traj, lens=None, draw_index=0):
        """backward_ref's trajectories [L_b][n_traj] of every problem, computed once a (shape, draw_index)."""
        lens = self.Ts if lens is None else lens
        key = (n_traj, tuple(lens), draw_index)
        if key not in self._traj:
            self._traj[key] = [R.trajectories_fast(self.m[b][:L], self.P[b], int(self.seeds[b]), n_traj, draw_index) if L else np.zeros((0, n_traj), np.int32)
                               for b, L in enumerate(lens)]
        return self._traj[key]

    def want(self, n_traj, lens=None, with_obs=True, draw_index=0):
        lens = self.Ts if lens is None else lens
        return np.stack([TS.records(x, self.obs[b][:L] if with_obs else None) for b, (x, L) in enumerate(zip(self.paths(n_traj, lens, draw_index), lens))])


TS_LENS = [0, 1, 2, 7, 64, 7, 64]


@pytest.fixture(scope="module", params=["hmm3", "table2", "table5", "table8"])
def batch(request):
    ns = [5, 3, 1, 70, 300, 40, 9]
    if request.param == "hmm3":
        return Batch(TS_LENS, ns, 3, True, 5, rare=5)
    k = int(request.param[5:])
    return Batch(TS_LENS, ns, k, False, 7 + k, rare=5)


def test_records_are_the_references(prog, batch):
    """n_traj in {1, 2, 3, one tile, one tile + 1, two tiles + 5 under a grid with an idle tile}: odd word pairs, a partial tile, a
    tile past the trajectories; the trajectories do not depend on n_traj."""
    rare = np.array(batch.m[5])[:, batch.k - 1]
    assert np.sum(rare == 0) >= 4 and np.any(rare > 0), "the last state of problem 5 should be absent from most generations"
    big = batch.want(2 * TILE + 5)
    assert np.all(big[0] == 0.0) and np.all(big[1, :, :64] == 0.0) and np.all(big[1, :, 64:72].sum(axis=1) == 1.0)
    assert np.all(big[4, :, :64].sum(axis=1) == 63.0) and np.all(big[4, :, 64:72].sum(axis=1) == 64.0)
    assert np.all(big[:, :, :64].reshape(batch.B, -1, 8, 8)[:, :, batch.k:] == 0.0) and np.all(big[:, :, 64 + batch.k:72] == 0.0)
    for n_traj, idle in ((1, 0), (2, 0), (3, 0), (TILE, 0), (TILE + 1, 0), (2 * TILE + 5, 1)):
        got = prog(batch, n_traj, idle_tiles=idle)
        assert np.array_equal(got, big[:, :n_traj]), "n_traj %d: records differ from the reference (largest difference %.3g)" % (n_traj, np.nanmax(np.abs(got - big[:, :n_traj])))
        if n_traj <= 3:
            assert np.array_equal(got, batch.want(n_traj))      # (the reference asked for n_traj trajectories draws the same ones)


def test_rows_read_from_memory_give_the_same_records(prog, batch):
    """Dynamic LDS of 7 rows: the problems of 64 steps read their masses from memory, the others stage them."""
    want = batch.want(2 * TILE + 5)[:, :TILE + 1]
    assert np.array_equal(prog(batch, TILE + 1, lds_bytes=64 * 7), want)
    assert np.array_equal(prog(batch, 3, lds_bytes=0), want[:, :3])


def test_no_observes_and_another_draw_index(prog, batch):
    got = prog(batch, 3, with_obs=False)
    assert np.array_equal(got, batch.want(3, with_obs=False))
    assert np.all(got[:, :, 72:] == 0.0) and np.array_equal(got[:, :, :72], batch.want(2 * TILE + 5)[:, :3, :72])
    other = prog(batch, 3, draw_index=5)
    assert np.array_equal(other, batch.want(3, draw_index=5)) and not np.array_equal(other, batch.want(2 * TILE + 5)[:, :3])


def test_table_addressed_by_capacity(prog):
    """An online batch: rows by capacity, lengths reached below them, a problem still at length 0 between two that are not."""
    bt = Batch([23, 9, 5], [70, 1, 300], 5, False, 11, caps=[25, 12, 8])
    for lens in ([5, 0, 1], [23, 9, 5]):
        for n_traj in (2, TILE + 1):
            for with_obs in (True, False):
                got = prog(bt, n_traj, lens=lens, with_obs=with_obs)
                assert np.array_equal(got, bt.want(n_traj, lens, with_obs)), "lengths %s, n_traj %d" % (lens, n_traj)
        if lens[1] == 0:
            assert np.all(prog(bt, 2, lens=lens)[1] == 0.0)
