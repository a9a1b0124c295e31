"""The kernels of csrc/batch_smooth.hpp as host code: the translation unit is formed here from the file's own text (its
`#include "batch_smc.hpp"` line names tests/host_kernels/batch_smooth_shim.hpp instead, its dynamic LDS array becomes a heap block of
the launch's size), built as a stand-alone program with g++ -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined
-ffp-contract=off and run over grids this file chooses (tests/host_kernels/batch_smooth_main.cpp: a workgroup is 256 threads, a launch a
loop over its blocks).  The loops that make the kernels independent of the grid -- the counting pass's rounds with their LDS slots by
round parity, the lag kernel's trips -- then run once, twice and many times on the same input: every grid gives the same bytes, and
those bytes equal tests/backward_ref.py and tests/lag_ref.py exactly (host division is IEEE: the marginals are array_equal too).  The
counting launches run under an adversarial schedule: the threads that reduce the wavefronts' partial counts leave every barrier late,
so a slot that is written again before it was read shows.  Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 18 int64 {magic, B, T_max, k, spp, thr_stride, n_traj, lds_bytes, marg_rows, lag, count grid (0: no
launch), lag grid (0: no launch), flags (1: the lag launch writes marginals, 2: the smoothing launch does, 4: it writes trajectories,
8: batch_smooth_kernel<3>, 16: the smoothing launch happens), store entries, rows of the m table, threshold words, trajectory entries,
the schedule's delay in microseconds} and one uint64 (draw_base), then the descriptors, the store, the table, the thresholds, the seeds
and the m table as the launches find it.  The output: the m table, the marginals, the trajectories."""
import os
import re
import subprocess

import numpy as np
import pytest

import backward_ref as R
import lag_ref as G
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
MAGIC = 0x4b534d4f4f544831
LAG_MARG, SMOOTH_MARG, SMOOTH_TRAJ, HMM3, SMOOTH = 1, 2, 4, 8, 16
DESC = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8"), ("rows", "<i8"), ("trows", "<i8"), ("cfrom", "<i4"), ("cto", "<i4"), ("lo", "<i4"), ("mfrom", "<i4")])
DRAW_BASE, LDS_MAX, K_WAVES, TILE = 1 << 41, 32768, 4, 1024
SKEW_US = 300


def _kernel_text():
    """csrc/batch_smooth.hpp with the two textual changes; each must find its line exactly once."""
    src = open(os.path.join(ROOT, "cpprob_amd", "csrc", "batch_smooth.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert src.count(inc) == 1
    src = src.replace(inc, '#include "batch_smooth_shim.hpp"')
    lds = re.findall(r"^[ \t]*extern __shared__[^\n;]*\bs_mass\[\];", src, re.M)
    assert len(lds) == 1 and src.count("extern __shared__") == 1, lds
    return src.replace(lds[0], "    double* s_mass = hostk::dynamic_lds();")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_smooth_host"))
    open(os.path.join(d, "batch_smooth_host.hpp"), "w").write(_kernel_text())
    so = O.build()
    exe = os.path.join(d, "batch_smooth_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_smooth_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(case):
        """case: the header's fields by name plus the arrays; returns (m table [rows, 8], marginals [B, marg_rows, spp], trajectories)."""
        B, spp = len(case["desc"]), case["spp"]
        head = np.array([MAGIC, B, case["T_max"], case["k"], spp, case["thr_stride"], case.get("n_traj", 0), case.get("lds_bytes", 0), case.get("marg_rows", 0),
                         case.get("lag", 0), case.get("count_gy", 0), case.get("lag_gy", 0), case.get("flags", 0), case["values"].size, case["mass"].shape[0],
                         case["thr"].size, case.get("traj_entries", 0), case.get("skew_us", SKEW_US)], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            f.write(np.array([case.get("draw_base", DRAW_BASE)], "<u8").tobytes())
            for name, dt in (("desc", DESC), ("values", np.int8), ("tab", np.float64), ("thr", np.uint64), ("seeds", np.uint64), ("mass", np.float64)):
                f.write(np.ascontiguousarray(case[name], dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        n_mass, n_marg, n_traj = case["mass"].size, B * case.get("marg_rows", 0) * spp, case.get("traj_entries", 0)
        assert len(raw) == 8 * (n_mass + n_marg) + n_traj
        mass = np.frombuffer(raw, np.float64, n_mass).reshape(-1, 8)
        marg = np.frombuffer(raw, np.float64, n_marg, 8 * n_mass).reshape(B, case.get("marg_rows", 0), spp)
        return mass, marg, np.frombuffer(raw, np.int8, n_traj, 8 * (n_mass + n_marg))
    return run


def test_shim_restates_the_headers_constants():
    wave = open(os.path.join(ROOT, "cpprob_amd", "include", "cpprob", "detail", "wave.hpp")).read()
    smc = open(os.path.join(ROOT, "cpprob_amd", "csrc", "batch_smc.hpp")).read()
    shim = open(os.path.join(HERE, "batch_smooth_shim.hpp")).read()
    assert re.search(r"constexpr int kWave = 64;", wave) and re.search(r"constexpr int kThreads = 256;", wave) and re.search(r"#define CPPROB_PPT 4\b", wave)
    assert re.search(r"constexpr int kTile = kThreads \* kPPT;", wave) and re.search(r"constexpr int kBatchTab = 8;", smc)
    assert "kGroupThreads = 256, kGroupWave = 64" in shim and "constexpr int kPPT = 4;" in shim and "constexpr int kBatchTab = 8;" in shim
    assert "constexpr int kTile = kThreads * kPPT;" in shim
    assert DESC.itemsize == 48 and TILE == 256 * 4


# ---- synthetic batches -------------------------------------------------------------------------------------------------------------
class Batch:
    """Problems of lengths Ts (capacities caps: an online batch's addressing, rows and store by capacity) with random states -- a
    generation without its last state every third step --, random table rows and, model HMM_TABLE, a table a problem whose second one
    has a zero transition entry.  m, P: the references' integers."""

    def __init__(self, Ts, ns, k, hmm3, seed, caps=None):
        rng = np.random.default_rng(seed)
        self.Ts, self.ns, self.k, self.hmm3 = list(Ts), list(ns), k, hmm3
        self.caps = list(caps) if caps else list(Ts)
        self.B, self.T_max, self.spp = len(Ts), max(self.caps), 3 if hmm3 else 8
        self.seeds = np.array([1000 + 77 * b for b in range(self.B)], np.uint64)
        self.store = np.concatenate([[0], np.cumsum([c * n for c, n in zip(self.caps, self.ns)])]).astype(np.int64)
        self.rows = np.concatenate([[0], np.cumsum(self.caps)]).astype(np.int64)
        self.values = np.full(int(self.store[-1]), 0, np.int8)
        self.tab = np.full((self.B, self.T_max, 8), np.nan)                       # (a row or state the kernels must not read: NaN)
        trans = rng.uniform(0.05, 1.0, (1 if hmm3 else self.B, k, k))
        if not hmm3 and self.B > 1:
            trans[1, 0, k - 1] = 0.0
        self.thr = np.full((trans.shape[0], 8, 8), np.iinfo(np.uint64).max, np.uint64)     # (words behind a row's k - 1 entries: all ones)
        for i, tr in enumerate(trans):
            for s, row in enumerate(R.thresholds(tr)):
                self.thr[i, s, :k - 1] = row
        self.thr_stride = 0 if hmm3 else 64
        self.m, self.P, self.vals = [], [], []
        for b, (T, n) in enumerate(zip(self.Ts, self.ns)):
            v = rng.integers(0, k, (T, n))
            v[2::3][v[2::3] == k - 1] = 0
            ll = -rng.uniform(0.0, 30.0, (T, k))
            self.values[self.store[b]:self.store[b] + T * n] = v.reshape(-1)
            self.tab[b, :T, :k] = ll
            self.vals.append(v)
            self.m.append(R.filtering_masses(v, ll.tolist()))
            self.P.append(R.transition_masses(trans[0 if hmm3 else b]))

    def desc(self, lens=None, cfrom=None, lag=None, frm=None):
        """batch_smooth_enqueue's descriptor arithmetic: lengths reached `lens`, the counting ranges [cfrom_b, L_b), the window of a
        fixed-lag call and its first rows."""
        lens = self.Ts if lens is None else lens
        d = np.zeros(self.B, DESC)
        at_traj = 0
        for b, L in enumerate(lens):
            W = L if lag is None else min(lag + 1, L)
            d[b] = (L, self.ns[b], self.store[b], self.rows[b], at_traj, 0 if cfrom is None else cfrom[b], L, L - W, 0 if frm is None else frm[b])
            at_traj += W
        return d, at_traj

    def case(self, **kw):
        c = dict(T_max=self.T_max, k=self.k, spp=self.spp, thr_stride=self.thr_stride, values=self.values, tab=self.tab, thr=self.thr, seeds=self.seeds,
                 flags=HMM3 if self.hmm3 else 0)
        c["flags"] |= kw.pop("flags", 0)
        c.update(kw)
        return c

    def table(self, lens=None, fill=-1.0):
        """The m table one pass over rows [0, lens_b) leaves in a table filled with `fill`."""
        lens = self.Ts if lens is None else lens
        out = np.full((int(self.rows[-1]), 8), fill)
        for b, L in enumerate(lens):
            out[self.rows[b]:self.rows[b] + L] = 0.0
            out[self.rows[b]:self.rows[b] + L, :self.k] = np.array(self.m[b][:L], np.float64).reshape(L, self.k)
        return out


@pytest.fixture(scope="module", params=["table5", "hmm3"])
def batch(request):
    if request.param == "hmm3":
        return Batch([23, 9, 1], [70, 1, 300], 3, True, 5)
    return Batch([23, 9, 1], [70, 1, 300], 5, False, 7)


def _ref_lag(bt, lag, frm, n_rows):
    out = np.zeros((bt.B, n_rows, bt.spp))
    for b, T in enumerate(bt.Ts):
        g = G.fixed_lag_marginals(bt.m[b], bt.P[b], lag)[frm[b]:]
        out[b, :g.shape[0], :bt.k] = g
    return out


def _lag_items(bt, lag, frm):
    return max([max(1, T - f - lag) for T, f in zip(bt.Ts, frm) if f < T] + [0])


# ---- 1. the counting pass: every grid, the same table ------------------------------------------------------------------------------
def test_counting_grids_give_the_references_table(prog, batch):
    """gridDim.y in {1, 2, 3, 8, 23} over ranges of 23, 9 and 1 rows: workgroups of 0 .. 23 rounds."""
    d, _ = batch.desc()
    want = batch.table()
    for gy in (1, 2, 3, 8, 23):
        mass, _, _ = prog(batch.case(desc=d, mass=np.full_like(want, -1.0), count_gy=gy))
        assert np.array_equal(mass, want), "counting grid %d: the m table differs from the reference's masses" % gy


def test_ranges_counted_in_pieces(prog):
    """An online batch: the table is addressed by capacity and counted range by range [counted_b, L_b) as the rows arrive, each piece on
    another grid; rows past a length stay what they were."""
    bt = Batch([23, 9, 1], [70, 1, 300], 5, False, 11, caps=[25, 12, 4])
    mass = np.full((int(bt.rows[-1]), 8), -1.0)
    counted = [0, 0, 0]
    for lens, gy in (([5, 0, 1], 2), ([6, 9, 1], 8), ([6, 9, 1], 0), ([23, 9, 1], 3)):
        d, _ = bt.desc(lens=lens, cfrom=counted)
        mass, _, _ = prog(bt.case(desc=d, mass=mass, count_gy=gy))
        counted = lens
        assert np.array_equal(mass, bt.table(lens)), "lengths %s: the table is not one pass's" % lens
    d, _ = bt.desc()
    once, _, _ = prog(bt.case(desc=d, mass=np.full_like(mass, -1.0), count_gy=23))
    assert np.array_equal(once, mass)


# ---- 2. the lag kernel: every grid, the same rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lag,frm", [(0, None), (3, None), (64, None), (3, [5, 9, 0]), (0, [20, 0, 1])])
def test_lag_grids_give_the_references_rows(prog, batch, lag, frm):
    """gridDim.y in {1, 2, 6}: at lag 0 and 3 the longest problem's items need 6, 3 and 1 trips."""
    f = frm or [0] * batch.B
    n_rows = max(T - x for T, x in zip(batch.Ts, f))
    d, _ = batch.desc(lag=lag, frm=f)
    want = _ref_lag(batch, lag, f, n_rows)
    items = _lag_items(batch, lag, f)
    for gy in (1, 2, 6):
        _, marg, _ = prog(batch.case(desc=d, mass=batch.table(), lag=lag, lag_gy=gy, marg_rows=n_rows, flags=LAG_MARG))
        assert np.array_equal(marg, want), "lag %d, from %s, lag grid %d (%d items, %d a trip): rows differ from the reference" % (lag, frm, gy, items, gy * K_WAVES)
    if lag == 3 and frm is None:
        assert items == 20 and -(-items // K_WAVES) == 5          # (the grid of one workgroup takes five trips)


def test_whole_calls_on_every_counting_grid(prog, batch):
    """The launches of one call in order -- count, lag, trajectories -- and of the full call, on counting grids of many rounds: the
    results do not depend on the grid, the window is the full call's last rows, and both are the references'."""
    M, di, lag = 33, 3, 3
    base = DRAW_BASE + (di << 24)
    d_full, n_full = batch.desc()
    d_lag, n_win = batch.desc(lag=lag)
    ref_x = [R.trajectories_fast(batch.m[b], batch.P[b], int(batch.seeds[b]), M, di) for b in range(batch.B)]
    ref_g = np.zeros((batch.B, batch.T_max, batch.spp))
    for b, T in enumerate(batch.Ts):
        ref_g[b, :T, :batch.k] = R.marginals(batch.m[b], batch.P[b])
    want_lag = _ref_lag(batch, lag, [0] * batch.B, batch.T_max)
    for gy, lgy in ((1, 1), (2, 6), (8, 2)):
        empty = np.full((int(batch.rows[-1]), 8), -1.0)
        _, marg, traj = prog(batch.case(desc=d_full, mass=empty, count_gy=gy, marg_rows=batch.T_max, n_traj=M, traj_entries=n_full * M, draw_base=base,
                                        lds_bytes=min(64 * max(batch.Ts), LDS_MAX), flags=SMOOTH | SMOOTH_MARG | SMOOTH_TRAJ))
        assert np.array_equal(marg, ref_g), "counting grid %d: the full marginals differ from the reference" % gy
        assert np.array_equal(traj, np.concatenate([x.reshape(-1) for x in ref_x])), "counting grid %d: the trajectories differ from the reference" % gy
        _, marg, traj = prog(batch.case(desc=d_lag, mass=empty, count_gy=gy, lag=lag, lag_gy=lgy, marg_rows=batch.T_max, n_traj=M, traj_entries=n_win * M, draw_base=base,
                                        lds_bytes=min(64 * min(lag + 1, max(batch.Ts)), LDS_MAX), flags=LAG_MARG | SMOOTH | SMOOTH_TRAJ))
        assert np.array_equal(marg, want_lag), "grids %d, %d: the fixed-lag rows differ from the reference" % (gy, lgy)
        assert np.array_equal(traj, np.concatenate([x[T - min(lag + 1, T):].reshape(-1) for x, T in zip(ref_x, batch.Ts)])), "grids %d, %d: the windows differ" % (gy, lgy)
        for b, T in enumerate(batch.Ts):
            W = min(lag + 1, T)
            assert np.array_equal(marg[b, T - W:T], ref_g[b, T - W:T])      # (the rows whose end is the last step: the full smoother's)


# ---- 3. the staging boundary -------------------------------------------------------------------------------------------------------
def test_windows_of_512_and_513_rows(prog):
    """T = 513 beside T = 5, 32768 bytes of dynamic LDS: the window of 512 rows is staged from lo = 1 and fills the block to its last
    byte, the window of 513 rows reads its masses from memory; both are the reference's rows."""
    bt = Batch([513, 5], [3, 70], 3, True, 13)
    M = 33
    d, _ = bt.desc()
    mass, _, _ = prog(bt.case(desc=d, mass=np.full((int(bt.rows[-1]), 8), -1.0), count_gy=8, skew_us=20))
    assert np.array_equal(mass, bt.table())
    ref_x = [R.trajectories_fast(bt.m[b], bt.P[b], int(bt.seeds[b]), M) for b in range(bt.B)]
    for lag in (511, 512):
        d, n_win = bt.desc(lag=lag)
        assert d["lo"].tolist() == [512 - lag, 0] and min(64 * (lag + 1), LDS_MAX) == LDS_MAX
        _, _, traj = prog(bt.case(desc=d, mass=mass, lag=lag, n_traj=M, traj_entries=n_win * M, lds_bytes=LDS_MAX, flags=SMOOTH | SMOOTH_TRAJ))
        assert np.array_equal(traj, np.concatenate([x[T - min(lag + 1, T):].reshape(-1) for x, T in zip(ref_x, bt.Ts)])), "a window of %d rows differs from the reference" % (lag + 1)
