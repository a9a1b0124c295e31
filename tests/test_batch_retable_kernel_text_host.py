"""batch_retable_kernel and batch_mstep_kernel (csrc/batch_retable.hpp) as host code: the header's own text, its include line naming
tests/host_kernels/batch_retable_shim.hpp, built as a stand-alone program with g++ -O1 -fsanitize=address,undefined
-fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_retable_main.cpp) and run over grids from one workgroup a
problem to the capped grid.  Every buffer has exactly the size the host code hands the kernel, the table region is NaN on the way in --
an untouched padded row or a refused problem shows --, and the rows, threshold words, status words and M-step tables must equal
tests/retable_ref.py's bit for bit.  Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 7 int64 {magic, B, k, T_max, gridDim.y, observes, the grid the reference states for (T_max, B)}, then the descriptors [B] {T int32, n int32, store int64},
the first observes [B] int64, the means [B][k], the transition rows [B][k][k], the observes, log_norm, the table region
[B][T_max][8], the threshold words [B][64] and the M-step's records [B][88].  The output: the table region, the threshold words, the
status words [B] int32, then the M-step's means and transition rows."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import retable_ref as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b52455441423031
DESC = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8")])
LOG_NORM = math.log(2 * 3.14159265358979323846 * 1.0 * 1.0)      # (the value is an input: both sides are handed the same double)
TS = [1, R.ROWS_PER_TRIP - 1, R.ROWS_PER_TRIP, R.ROWS_PER_TRIP + 1, 70, 70]
OLD_THR = np.uint64(0x1234)


def _text():
    text = open(os.path.join(CSRC, "batch_retable.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert text.count(inc) == 1 and text.count("#include") == 1
    return text, text.replace(inc, '#include "batch_retable_shim.hpp"')


def test_text():
    """fp contract off in every function, no logarithm, no atomics, one barrier, LDS for the staged table alone, eight lanes a row,
    the grid's cap a named constant; the library includes the header and launches both kernels."""
    text, _ = _text()
    code = re.sub(r"//[^\n]*", "", text)
    bodies = re.findall(r"\n(?:__host__ __device__ inline|__global__)[^\n]*\)\n\{\n(.*?)\n\}\n", code, re.S)
    assert len(bodies) == 8
    for body in bodies:
        if "double" in body or "retable_threshold(" in body:
            assert body.lstrip().startswith("#pragma clang fp contract(off)"), body[:80]
    assert re.search(r"[^_\w]log\s*\(", code) is None and re.search(r"[^_\w]fma\s*\(", code) is None and "atomic" not in code
    assert code.count("__syncthreads") == 1 and code.count("__shared__") == 1 and "__shared__ double s_tab[8 + 64];" in code
    assert "constexpr int kRetableRows = kThreads / 8;" in code and re.search(r"constexpr int kRetableGridMax = %d;" % R.GRID_MAX, code) and re.search(r"constexpr int kRetableGroups = %d;" % R.GROUPS, code)
    assert R.ROWS_PER_TRIP == 256 // 8
    hip = open(os.path.join(CSRC, "cpprob_hip.hip")).read()
    assert '#include "batch_retable.hpp"' in hip and "hipLaunchKernelGGL(batch_retable_kernel" in hip and "hipLaunchKernelGGL(batch_mstep_kernel" in hip
    assert "a.log_norm = std::log(2 * kPi * 1.0 * 1.0);" in hip


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_retable_host"))
    open(os.path.join(d, "batch_retable_host.hpp"), "w").write(_text()[1])
    so = O.build()
    exe = os.path.join(d, "batch_retable_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, "-I", os.path.join(ROOT, "cpprob_amd", "include"), os.path.join(HERE, "batch_retable_main.cpp"), "-o", exe, so,
           "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(case, grid_y):
        B, k, T_max = case.B, case.k, case.T_max
        desc = np.zeros(B, DESC)
        desc["T"], desc["n"] = case.T, 7
        first = np.concatenate([[0], np.cumsum(case.T)[:-1]]).astype("<i8")
        head = np.array([MAGIC, B, k, T_max, grid_y, case.obs.size, R.grid_y(T_max, B)], "<i8")
        tab0 = np.full((B, T_max, 8), np.nan)
        thr0 = np.full((B, 64), OLD_THR, np.uint64)
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            for arr, dt in ((desc, DESC), (first, "<i8"), (case.means, np.float64), (case.trans, np.float64), (case.obs, np.float64),
                            (np.array([LOG_NORM]), np.float64), (tab0, np.float64), (thr0, np.uint64), (case.stats, np.float64)):
                f.write(np.ascontiguousarray(arr, dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        n_tab = B * T_max * 8
        at = [0]

        def take(n, dt):
            a = np.frombuffer(raw, dt, n, at[0])
            at[0] += a.nbytes
            return a
        out = (take(n_tab, np.float64).reshape(B, T_max, 8), take(B * 64, np.uint64).reshape(B, 64), take(B, np.int32),
               take(B * k, np.float64).reshape(B, k), take(B * k * k, np.float64).reshape(B, k, k))
        assert at[0] == len(raw)
        return out
    return run


class Case:
    def __init__(self, k, seed, bad=()):
        """B = 6 problems of the lengths TS; problem 1 has a transition row with zero entries (equal consecutive thresholds);
        bad: (problem, bit) pairs, each problem failing that one check."""
        rng = np.random.default_rng(seed)
        self.k, self.B, self.T, self.T_max = k, len(TS), np.array(TS, np.int64), max(TS)
        self.means = rng.normal(0.0, 3.0, (self.B, k))
        self.trans = rng.gamma(0.7, 1.0, (self.B, k, k))            # (unnormalised rows: the totals matter)
        self.trans[1, 0, :] = 0.0
        self.trans[1, 0, k - 1] = 2.5                               # words 0 .. k-2 of the row all 0
        self.trans[1, 1, 0] = 0.0
        if k > 2:
            self.trans[1, 1, 1] = 0.0                               # two equal words in front
            self.trans[1, 1, 2] = 1.0
        self.obs = rng.normal(0.0, 4.0, int(self.T.sum()))
        self.obs[3] = np.inf                                        # (an infinite observe: -inf in every state)
        for b, bit in bad:
            if bit == R.BAD_WEIGHT:
                self.trans[b, k - 1, 0] = -0.25 if b % 2 else np.nan
            elif bit == R.NO_MASS:
                self.trans[b, 0, :] = 0.0
            else:
                self.means[b, k - 1] = np.inf
        self.bad = dict(bad)
        # the M-step's records: random masses, a massless row (problem 0, state 1) and a massless state (problem 2, state 0)
        self.stats = np.zeros((self.B, R.RECORD))
        self.stats[:, :64] = rng.gamma(1.0, 2.0, (self.B, 64))
        self.stats[:, 64:72] = rng.gamma(2.0, 3.0, (self.B, 8))
        self.stats[:, 72:88] = rng.normal(0.0, 5.0, (self.B, 16))
        self.stats[0, 8:8 + k] = 0.0
        self.stats[2, 64] = 0.0

    def want(self):
        tab = np.full((self.B, self.T_max, 8), np.nan)
        thr = np.full((self.B, 64), OLD_THR, np.uint64)
        status = np.zeros(self.B, np.int32)
        at = 0
        for b in range(self.B):
            T = int(self.T[b])
            status[b] = R.check(self.means[b], self.trans[b], self.k)
            if status[b] == 0:
                tab[b, :T] = R.rows(self.obs[at:at + T], self.means[b], self.k, LOG_NORM)
                thr[b] = R.thresholds(self.trans[b], self.k)
            at += T
        ms = [R.m_step(self.stats[b], self.means[b], self.trans[b], self.k) for b in range(self.B)]
        return tab, thr, status, np.array([m for m, _ in ms]), np.array([t for _, t in ms])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("k", [2, 5, 8])
def test_every_grid_gives_the_references_bits(prog, k):
    """gridDim.y = 1: the workgroup of a 70-step problem makes 3 trips; 2: trips 0 and 2 against trip 1; the host's own grid (3: one
    trip each).  Problems 3, 4, 5 fail one check each and keep NaN rows and the old words; the others' padded rows stay NaN."""
    case = Case(k, 100 + k, bad=((3, R.BAD_WEIGHT), (4, R.NO_MASS), (5, R.BAD_MEAN)))
    tab_w, thr_w, st_w, m_w, t_w = case.want()
    assert list(st_w) == [0, 0, 0, R.BAD_WEIGHT, R.NO_MASS, R.BAD_MEAN]
    assert thr_w[1, 0] == 0 and thr_w[1, 8] == 0 and (k == 2 or thr_w[1, 9] == 0)          # equal consecutive thresholds occur
    assert (70 + R.ROWS_PER_TRIP - 1) // R.ROWS_PER_TRIP >= 3 and R.grid_y(70, 6) == 3 and R.grid_y(1024, 1024) == 4 and R.grid_y(16, 1024) == 1 and R.grid_y(10 ** 6, 6) == R.GRID_MAX
    for gy in (1, 2, R.grid_y(case.T_max, case.B)):
        tab, thr, st, m, t = prog(case, gy)
        assert np.array_equal(st, st_w), gy
        assert _same(tab, tab_w), "grid %d: rows" % gy
        assert np.array_equal(thr, thr_w), "grid %d: thresholds" % gy
        assert _same(m, m_w) and _same(t, t_w), "grid %d: M-step" % gy
    assert np.all(np.isnan(tab_w[0, 1:])) and np.all(np.isneginf(tab_w[0, 0, k:]))
    # the M-step: a massless row and a massless state keep their values, the others moved
    assert _same(t_w[0, 1], case.trans[0, 1]) and not np.array_equal(t_w[0, 0], case.trans[0, 0])
    assert m_w[2, 0] == case.means[2, 0] and m_w[2, 1] != case.means[2, 1]


@pytest.mark.parametrize("k", [2, 8])
def test_a_long_problem_on_the_capped_grid(prog, k):
    """All six tables valid; the 70-step problems on a grid of 1 (3 trips) and on more workgroups than trips (idle ones write nothing)."""
    case = Case(k, 7 + k)
    tab_w, thr_w, st_w, m_w, t_w = case.want()
    assert not st_w.any()
    for gy in (1, 5):
        tab, thr, st, m, t = prog(case, gy)
        assert not st.any() and _same(tab, tab_w) and np.array_equal(thr, thr_w) and _same(m, m_w) and _same(t, t_w), gy
    b3 = np.searchsorted(np.cumsum(case.T), 3, side="right")
    assert np.all(np.isneginf(tab_w[b3, 3 - int(case.T[:b3].sum())]))                      # the infinite observe's row


def test_reference_thresholds_are_the_hosts(prog):
    """retable_ref.thresholds against the oracle-free closed form on a table whose cumulative sums are exact."""
    thr = R.thresholds(np.array([[0.5, 0.25, 0.25], [0.0, 1.0, 0.0], [1.0, 1.0, 2.0]]), 3)
    assert list(thr[0:2]) == [1 << 31, 3 << 30] and list(thr[8:10]) == [0, 1 << 32] and list(thr[16:18]) == [1 << 30, 1 << 31]
    assert np.all(thr[[2, 10, 18] + list(range(24, 64))] == np.uint64(0xFFFFFFFFFFFFFFFF))
