"""batch_forecast_kernel and batch_predictive_kernel (csrc/batch_forecast.hpp) as host code: the translation unit is formed here from
the text of csrc/batch_smooth.hpp and csrc/batch_forecast.hpp (the former as tests/test_batch_smooth_kernel_text_host.py forms it, the
latter's include line naming that text), built against tests/host_kernels/batch_smooth_shim.hpp as a stand-alone program with g++ -O1
-fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_forecast_main.cpp) and run
over grids from one workgroup a problem to one a tile or step.  Every buffer has exactly the size the host code hands the kernel, rows
of the m table no problem has reached are NaN, and the rows must equal tests/forecast_ref.py's bit for bit (host division is IEEE).
Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 14 int64 {magic, B, k, spp, thr_stride, 1: HMM3, 1: the predictive kernel, gridDim.y, rows of the m table,
threshold words, H, n_traj, rows a problem of the doubles' output, draw_index}, then the descriptors, the thresholds, the m table and
the seeds.  The output: the doubles [B][rows][spp], then (the forecast kernel) the trajectories [B][H + 1][n_traj] int8."""
import os
import re
import subprocess

import numpy as np
import pytest

import backward_ref as R
import forecast_ref as F
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b46434153543031
DESC = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8"), ("rows", "<i8"), ("trows", "<i8"), ("cfrom", "<i4"), ("cto", "<i4"), ("lo", "<i4"), ("mfrom", "<i4")])
K_WAVES, K_TILE = 4, 1024


def _texts():
    """(csrc/batch_smooth.hpp, csrc/batch_forecast.hpp) with their textual changes; each must find its line exactly once."""
    smooth = open(os.path.join(CSRC, "batch_smooth.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert smooth.count(inc) == 1
    smooth = smooth.replace(inc, '#include "batch_smooth_shim.hpp"')
    lds = re.findall(r"^[ \t]*extern __shared__[^\n;]*\bs_mass\[\];", smooth, re.M)
    assert len(lds) == 1 and smooth.count("extern __shared__") == 1, lds
    smooth = smooth.replace(lds[0], "    double* s_mass = hostk::dynamic_lds();")
    fc = open(os.path.join(CSRC, "batch_forecast.hpp")).read()
    inc = '#include "batch_smooth.hpp"'
    assert fc.count(inc) == 1 and fc.count("#include") == 1
    code = re.sub(r"//[^\n]*", "", fc)
    assert "extern" not in code and "atomic" not in code, "the forecast kernels use no dynamic LDS and no atomics"
    assert code.count("__syncthreads") == 1 and code.count("__shared__") == 1, "one static LDS block, one barrier after its staging"
    return smooth, fc.replace(inc, '#include "batch_smooth_host.hpp"')


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_forecast_host"))
    smooth, fc = _texts()
    open(os.path.join(d, "batch_smooth_host.hpp"), "w").write(smooth)
    open(os.path.join(d, "batch_forecast_host.hpp"), "w").write(fc)
    so = O.build()
    exe = os.path.join(d, "batch_forecast_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_forecast_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(bt, lens, predictive, grid_y, H=0, n_traj=0, rows=0, frm=None, draw_index=0):
        """(doubles [B, rows, spp], trajectories [B, H + 1, n_traj]) of batch `bt` at the lengths reached `lens`."""
        desc = bt.desc(lens, frm)
        head = np.array([MAGIC, bt.B, bt.k, bt.spp, bt.thr_stride, int(bt.hmm3), int(predictive), grid_y, bt.mass.shape[0], bt.thr.size, H, n_traj, rows, draw_index], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            for arr, dt in ((desc, DESC), (bt.thr, np.uint64), (bt.mass, np.float64), (bt.seeds, np.uint64)):
                f.write(np.ascontiguousarray(arr, dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        n_d = bt.B * rows * bt.spp
        n_t = 0 if predictive else bt.B * (H + 1) * n_traj
        assert len(raw) == 8 * n_d + n_t
        return (np.frombuffer(raw[:8 * n_d], np.float64).reshape(bt.B, rows, bt.spp),
                np.frombuffer(raw[8 * n_d:], np.int8).reshape(bt.B, H + 1, n_traj) if not predictive else None)
    return run


class Batch:
    """Problems of lengths Ts (capacities caps: an online batch's m table, addressed by capacity) with random states and table rows.
    Model HMM_TABLE: a table a problem, the second one's with a zero transition entry.  The m table holds NaN wherever no problem has
    a row."""

    def __init__(self, Ts, ns, k, hmm3, seed, caps=None):
        rng = np.random.default_rng(seed)
        self.Ts, self.k, self.hmm3, self.B = list(Ts), k, hmm3, len(Ts)
        self.spp = 3 if hmm3 else 8
        self.caps = list(caps) if caps else list(Ts)
        self.rows = np.concatenate([[0], np.cumsum(self.caps)]).astype(np.int64)
        trans = rng.uniform(0.05, 1.0, (1 if hmm3 else self.B, k, k))
        if not hmm3 and self.B > 1:
            trans[1, 0, k - 1] = 0.0
        self.thr = np.full((trans.shape[0], 8, 8), np.iinfo(np.uint64).max, np.uint64)     # (words behind a row's k - 1 entries: all ones)
        self.c = []
        for i, tr in enumerate(trans):
            self.c.append(R.thresholds(tr))
            for s, row in enumerate(self.c[-1]):
                self.thr[i, s, :k - 1] = row
        self.thr_stride = 0 if hmm3 else 64
        self.seeds = rng.integers(1, 1 << 62, self.B).astype(np.uint64)
        self.mass = np.full((max(int(self.rows[-1]), 1), 8), np.nan)
        self.m, self.P = [], []
        for b, (T, n) in enumerate(zip(self.Ts, ns)):
            v = rng.integers(0, k, (T, n))
            ll = -rng.uniform(0.0, 30.0, (T, k))
            m = R.filtering_masses(v, ll.tolist()) if T else []
            self.m.append(m)
            self.P.append(R.transition_masses(trans[0 if hmm3 else b]))
            self.mass[self.rows[b]:self.rows[b] + T] = 0.0
            if T:
                self.mass[self.rows[b]:self.rows[b] + T, :k] = np.array(m, np.float64)

    def thresholds(self, b):
        return self.c[0 if self.hmm3 else b]

    def desc(self, lens, frm=None):
        """batch_smooth_enqueue's descriptors at the lengths reached; mfrom the first predictive row wanted."""
        d = np.zeros(self.B, DESC)
        at = 0
        for b, L in enumerate(lens):
            d[b] = (L, 1, 0, self.rows[b], at, L, L, 0, 0 if frm is None else frm[b])
            at += L
        return d

    def check_forecast(self, prog, lens, H, n_traj, draw_index=0):
        tiles = (n_traj + K_TILE - 1) // K_TILE
        marg, traj = prog(self, lens, False, 1 + tiles, H=H, n_traj=n_traj, rows=H, draw_index=draw_index)
        for b, L in enumerate(lens):
            want = np.zeros((H, self.spp))
            want[:, :self.k] = F.marginals(self.m[b][:L], self.P[b], H)
            assert np.array_equal(marg[b], want), "problem %d, length %d: marginals differ (largest %.3g)" % (b, L, np.nanmax(np.abs(marg[b] - want)))
            wt = F.trajectories(self.m[b][:L], self.thresholds(b), int(self.seeds[b]), H, n_traj, draw_index)
            assert np.array_equal(traj[b], wt), "problem %d, length %d: trajectories differ" % (b, L)
        return marg, traj

    def check_predictive(self, prog, lens, grid_y, frm=None):
        fr = [0] * self.B if frm is None else frm
        rows = max(max(L + 1 - f for L, f in zip(lens, fr)), 0)
        got, _ = prog(self, lens, True, grid_y, rows=rows, frm=frm)
        for b, L in enumerate(lens):
            want = F.predictive_rows(self.m[b][:L], self.P[b], fr[b], rows, self.spp)
            assert np.array_equal(got[b], want), "problem %d, length %d, grid %d: predictive rows differ" % (b, L, grid_y)
        return got


TS = [0, 1, 2, 7, 64]


@pytest.fixture(scope="module", params=["hmm3", "table2", "table5", "table8"])
def batch(request):
    ns = [5, 3, 1, 70, 300]
    if request.param == "hmm3":
        return Batch(TS, ns, 3, True, 5)
    k = int(request.param[5:])
    return Batch(TS, ns, k, False, 7 + k)


@pytest.mark.parametrize("H,n_traj", [(1, 1), (3, 257), (40, 1025)])
def test_forecast_is_the_references(prog, batch, H, n_traj):
    """n_traj 1 (an odd pair), 257 (a lane owns two chains), 1025 (two tiles); the length-0 problem's rows are zeros."""
    marg, traj = batch.check_forecast(prog, TS, H, n_traj, draw_index=H)
    assert np.all(marg[0] == 0.0) and np.all(traj[0] == 0)
    assert np.all(marg[:, :, batch.k:] == 0.0) and np.allclose(marg[1:, :, :batch.k].sum(axis=2), 1.0, atol=1e-12)
    assert traj.min() >= 0 and traj.max() < batch.k


def test_draw_index_selects_the_draws(prog, batch):
    _, a = batch.check_forecast(prog, TS, 3, 33, draw_index=0)
    _, b = batch.check_forecast(prog, TS, 3, 33, draw_index=5)
    assert not np.array_equal(a, b)


def test_zero_entry_is_never_taken(prog):
    """Table 1 has P[0][k-1] = 0: no simulated future of problem 1 steps from state 0 to state k - 1."""
    bt = Batch([9, 9, 9], [50, 50, 50], 5, False, 21)
    assert bt.P[1][0][4] == 0
    _, traj = bt.check_forecast(prog, [9, 9, 9], 40, 1025)
    t = traj[1]
    assert np.any(t[:-1] == 0) and not np.any((t[:-1] == 0) & (t[1:] == 4))
    assert np.any((traj[0][:-1] == 0) & (traj[0][1:] == 4))


def test_predictive_rows_on_every_grid(prog, batch):
    """gridDim.y in {1, 2, 17}: a wavefront takes 65 steps' rows in 17 trips, 9 trips or one; row L is the forecast's first row."""
    for gy in (1, 2, 17):
        got = batch.check_predictive(prog, TS, gy)
    marg, _ = prog(batch, TS, False, 1, H=1, n_traj=0, rows=1)
    for b, L in enumerate(TS):
        assert np.all(got[b, 0, :batch.k] == 1.0 / batch.k)
        if L:
            assert np.array_equal(got[b, L], marg[b, 0])
    frm = [1, 0, 3, 5, 60]                                     # (problem 0: past its one row; problem 2: from = L + 1)
    for gy in (1, 3):
        got = batch.check_predictive(prog, TS, gy, frm=frm)
        assert np.all(got[0] == 0.0) and np.all(got[2] == 0.0)


def test_table_addressed_by_capacity(prog):
    """An online batch: rows by capacity, lengths reached below them, a problem still at length 0 between two that are not."""
    bt = Batch([23, 9, 5], [70, 1, 300], 5, False, 11, caps=[25, 12, 8])
    for lens in ([5, 0, 1], [6, 9, 1], [23, 9, 5]):
        bt.check_forecast(prog, lens, 3, 257)
        for gy in (1, 2):
            bt.check_predictive(prog, lens, gy)


def test_predictive_rows_from_mid_table_in_several_trips(prog):
    """A `from` list that starts inside the table on grids that hold fewer items than the problems owe: 131 rows from step 70 on one
    and two grid rows (33 and 17 trips of a workgroup's four wavefronts), beside problems asked from 0, from L (one row) and from
    L + 1 (none)."""
    bt = Batch([200, 64, 65, 9], [70, 3, 300, 1], 5, False, 17)
    frm = [70, 0, 65, 10]
    one = bt.check_predictive(prog, bt.Ts, 64, frm=frm)               # (one trip: the grid holds 256 items a problem)
    for gy in (1, 2, 5):
        got = bt.check_predictive(prog, bt.Ts, gy, frm=frm)
        assert np.array_equal(got, one), "gridDim.y = %d differs from the grid of one trip" % gy
    full = bt.check_predictive(prog, bt.Ts, 3)
    assert np.array_equal(one[0], full[0, 70:]) and np.array_equal(one[2, 0], full[2, 65]) and np.all(one[2, 1:] == 0.0) and np.all(one[3] == 0.0)
