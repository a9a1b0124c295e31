"""batch_learn_rows_kernel and batch_learn_kernel (csrc/batch_learn.hpp) as host code: the translation unit is formed here from the
text of csrc/batch_smooth.hpp, csrc/batch_onlinestats.hpp, csrc/batch_retable.hpp (as their own kernel-text tests form them),
csrc/batch_scale.hpp and csrc/batch_learn.hpp (their include lines naming those texts), built against
tests/host_kernels/batch_smooth_shim.hpp and batch_retable_shim.hpp as a stand-alone program with g++ -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined
-ffp-contract=off (tests/host_kernels/batch_learn_main.cpp).  Every buffer has exactly the size the host code hands the kernels, the rows
of the m table no problem has reached AT THAT CALL are NaN, the table region starts as NaN, tau of a problem that has consumed nothing
is NaN on the way in, and records, tau, tables, threshold words, status words and rows must equal tests/learn_ref.py's (host division
is IEEE) on every grid, call after call.  Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 10 int64 {magic, B, k, t_min, gridDim.x of the learn launch, rows of the m table, observes, step sizes,
T_max, gridDim.y of the rows launch}, then the smoothing descriptors [B], the batch descriptors [B] {T int32, n int32, store int64},
the lengths before [B] int32 (-1: idle), the first new observes [B] int64, the threshold words [B][64], the m table, the new observes,
gamma, tau [B][8][88], the means [B][k], the transition rows [B][k][k], the status words [B] int32, the table region [B][T_max][8] and
log_norm.  The output: the records [B][88], tau, the means, the transition rows, the words, the status words, the table region."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import learn_ref as G
import test_batch_onlinestats_kernel_text_host as KO
import test_batch_retable_kernel_text_host as KR
import test_batch_suffstats_kernel_text_host as K
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b4c4541524e3031
TAU = 8 * G.RECORD
LOG_NORM = math.log(2 * 3.14159265358979323846 * 1.0 * 1.0)
PROB = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8")])
POISON = 64                                     # a status word nobody has written


def _texts():
    smooth, online = KO._texts()
    retable = KR._text()[1]
    scale = open(os.path.join(CSRC, "batch_scale.hpp")).read()
    inc = '#include "batch_retable.hpp"'
    assert scale.count(inc) == 1 and scale.count("#include") == 1
    scale = scale.replace(inc, '#include "batch_retable_host.hpp"')
    text = open(os.path.join(CSRC, "batch_learn.hpp")).read()
    incs = ('#include "batch_onlinestats.hpp"', '#include "batch_scale.hpp"')
    assert all(text.count(i) == 1 for i in incs) and text.count("#include") == 2
    text = text.replace(incs[0], '#include "batch_onlinestats_host.hpp"').replace(incs[1], '#include "batch_scale_host.hpp"')
    return {"batch_smooth_host.hpp": smooth, "batch_onlinestats_host.hpp": online, "batch_retable_host.hpp": retable, "batch_scale_host.hpp": scale,
            "batch_learn_host.hpp": text}


def test_text():
    """fp contract off in every function (the two bodies, learn_row_bits and the four kernels over them), no power, no logarithm, no
    LDS, no barrier, no atomics; the library launches both kernels and leaves batch_smc_kernel's launch to batch_launch."""
    text = open(os.path.join(CSRC, "batch_learn.hpp")).read()
    code = re.sub(r"//[^\n]*", "", text)
    for word in ("__shared__", "__syncthreads", "atomic", "pow(", "exp("):
        assert word not in code, word
    assert re.search(r"[^_\w]log\s*\(", code) is None and re.search(r"[^_\w]fma\s*\(", code) is None
    bodies = re.findall(r"\n(?:__device__ __forceinline__|__global__)[^\n]*\)\n\{\n(.*?)\n\}\n", code, re.S)
    assert len(bodies) == 7
    for body in bodies:
        assert body.lstrip().startswith("#pragma clang fp contract(off)"), body[:80]
    hip = open(os.path.join(CSRC, "cpprob_hip.hip")).read()
    assert '#include "batch_learn.hpp"' in hip and "hipLaunchKernelGGL(batch_learn_kernel" in hip and "hipLaunchKernelGGL(batch_learn_rows_kernel" in hip
    assert "ra.log_norm = std::log(2 * kPi * 1.0 * 1.0);" in hip


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_learn_host"))
    for name, text in _texts().items():
        open(os.path.join(d, name), "w").write(text)
    so = O.build()
    exe = os.path.join(d, "batch_learn_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_learn_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(st, grid_x, rows_gy, lens):
        """One learning advance to the lengths `lens` on the state st (a State): returns the outputs and moves nothing."""
        B, k, T_max = st.B, st.k, st.T_max
        desc, prob = np.zeros(B, K.DESC), np.zeros(B, PROB)
        first, ofirst = np.zeros(B, "<i4"), np.zeros(B, "<i8")
        obs, at = [], 0
        mass = st.bt.mass.copy()
        for b, (d0, L) in enumerate(zip(st.done, lens)):
            desc[b] = (L, 1, 0, st.bt.rows[b], at, 0, L, d0, 0)
            prob[b] = (L, 1, 0)
            first[b] = d0 if L > d0 else -1
            ofirst[b] = at
            obs.append(st.bt.obs[b][d0:L])
            at += L - d0
            mass[st.bt.rows[b] + L:st.bt.rows[b + 1]] = np.nan
        obs = np.concatenate(obs)
        head = np.array([MAGIC, B, k, st.t_min, grid_x, mass.shape[0], obs.size, st.gamma.size, T_max, rows_gy], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            for arr, dt in ((desc, K.DESC), (prob, PROB), (first, "<i4"), (ofirst, "<i8"), (st.thr, np.uint64), (mass, np.float64), (obs, np.float64),
                            (st.gamma, np.float64), (st.tau, np.float64), (st.means, np.float64), (st.trans, np.float64), (st.status, "<i4"),
                            (st.tab, np.float64), (np.array([LOG_NORM]), np.float64)):
                f.write(np.ascontiguousarray(arr, dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        at = [0]

        def take(n, dt):
            a = np.frombuffer(raw, dt, n, at[0])
            at[0] += a.nbytes
            return a.copy()
        out = dict(rec=take(B * G.RECORD, np.float64).reshape(B, G.RECORD), tau=take(B * TAU, np.float64).reshape(B, TAU),
                   means=take(B * k, np.float64).reshape(B, k), trans=take(B * k * k, np.float64).reshape(B, k, k),
                   thr=take(B * 64, np.uint64).reshape(B, 64), status=take(B, np.int32), tab=take(B * T_max * 8, np.float64).reshape(B, T_max, 8))
        assert at[0] == len(raw)
        return out
    return run


TS = [0, 1, 2, 7, 64, 7, 64]                    # seven problems: the last workgroup of four holds three
NS = [5, 3, 1, 70, 300, 40, 9]
SCHEDULE = [[0, 1, 1, 3, 5, 0, 64], [0, 1, 1, 5, 30, 7, 64], TS]
T_MIN = 3


class State:
    """The device state of a learning stream between two advances, and the reference's learners beside it."""

    def __init__(self, k, seed):
        self.bt = K.Batch(TS, NS, k, False, seed, rare=5)
        rng = np.random.default_rng(seed + 1000)
        self.B, self.k, self.T_max, self.t_min = len(TS), k, max(TS), T_MIN
        self.gamma = (np.arange(self.T_max) + 1.0) ** -0.6
        self.means = rng.normal(0.0, 3.0, (self.B, k))
        self.trans = rng.uniform(0.05, 1.0, (self.B, k, k))
        self.trans[5, :k - 1, 0] = 0.0          # problem 5: state 0 is reached from its rare last state alone, D[0] = 0 where that is absent
        self.learners = [G.Learner(self.means[b], self.trans[b], k, self.gamma, T_MIN, LOG_NORM) for b in range(self.B)]
        for lr in self.learners:
            lr.status = POISON
        self.thr = np.stack([lr.thr for lr in self.learners])
        self.tau = np.full((self.B, TAU), np.nan)               # (a problem that has consumed nothing: never read)
        self.status = np.full(self.B, POISON, np.int32)
        self.tab = np.full((self.B, self.T_max, 8), np.nan)
        self.done = [0] * self.B

    def want(self, lens):
        """Moves the learners to `lens`; returns what the program must leave."""
        tab = self.tab.copy()
        for b, (d0, L) in enumerate(zip(self.done, lens)):
            lr = self.learners[b]
            tab[b, d0:L] = lr.rows(self.bt.obs[b][d0:L])        # (under the table in force before the advance)
            lr.advance(self.bt.m[b][d0:L], self.bt.obs[b][d0:L])
        L = self.learners
        return dict(rec=np.stack([G.record_array(lr.record) for lr in L]), tau=[G.tau_array(lr.tau) for lr in L], means=np.stack([lr.means for lr in L]),
                    trans=np.stack([lr.trans for lr in L]), thr=np.stack([lr.thr for lr in L]), status=np.array([lr.status for lr in L], np.int32), tab=tab)

    def move(self, out, lens):
        self.tau, self.means, self.trans, self.thr, self.status, self.tab, self.done = out["tau"], out["means"], out["trans"], out["thr"], out["status"], out["tab"], list(lens)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def compare(out, want, lens, note):
    assert np.array_equal(out["status"], want["status"]), "%s: status %s, want %s" % (note, out["status"], want["status"])
    assert np.array_equal(out["rec"], want["rec"], equal_nan=True), "%s: records" % note
    for b, L in enumerate(lens):
        if L > 0:
            assert np.array_equal(out["tau"][b], want["tau"][b], equal_nan=True), "%s, problem %d: tau" % (note, b)
        else:
            assert np.all(np.isnan(out["tau"][b])), "a problem of length 0 stores no tau"
    assert _same(out["means"], want["means"]) and _same(out["trans"], want["trans"]), "%s: tables" % note
    assert np.array_equal(out["thr"], want["thr"]), "%s: threshold words" % note
    assert _same(out["tab"], want["tab"]), "%s: rows" % note


@pytest.mark.parametrize("k", [2, 5, 8])
def test_every_grid_gives_the_references_bits_call_after_call(prog, k):
    """gridDim.x in {1, 2}: a wavefront walks two problems or one; the rows launch with one workgroup a problem (a 64-step piece: two
    trips) and with three.  Three calls: a few steps; a resume in which problem 5 crosses the burn-in and some problems have nothing
    new; a last one with nothing new for problems 0, 1, 5 and 6, where the M-step must not fire (their status words stay)."""
    for gx, gy in ((1, 1), (2, 3)):
        st = State(k, 7 + k)
        fired = np.zeros(st.B, int)
        for call, lens in enumerate(SCHEDULE):
            before = [lr.changed for lr in st.learners]
            thr0 = st.thr.copy()
            out = prog(st, gx, gy, lens)
            want = st.want(lens)
            compare(out, want, lens, "k %d, grid %d x %d, call %d" % (k, gx, gy, call))
            for b in range(st.B):
                fired[b] += st.learners[b].changed - before[b]
                if lens[b] == st.done[b] or lens[b] < T_MIN:
                    assert st.learners[b].changed == before[b] and np.array_equal(out["thr"][b], thr0[b])
            # rows outside [done, L) are as they were: NaN where no advance has written
            for b, L in enumerate(lens):
                assert np.all(np.isnan(out["tab"][b, L:])) and not np.any(np.isnan(out["tab"][b, :L]))
            st.move(out, lens)
            if call == 0:
                assert list(out["status"]) == [POISON, POISON, POISON, 0, 0, POISON, 0]
            if call == 1:
                assert out["status"][5] == 0 and fired[5] == 1, "problem 5 crosses the burn-in in the second call"
            if call == 2:
                assert list(out["status"]) == [POISON, POISON, POISON, 0, 0, 0, 0] and fired[6] == 1 and fired[3] == 3 and fired[4] == 3
        lr5 = st.learners[5]
        rare = np.array(st.bt.m[5])[:, k - 1]
        assert np.sum(rare == 0) >= 4 and np.any(rare > 0) and rare[-1] == 0, "the last state of problem 5 should be absent from most generations"
        assert lr5.fallbacks >= 1, "a row with D = 0 should have taken the defensive rule"


@pytest.mark.parametrize("k", [2, 8])
def test_a_bad_m_step_keeps_the_old_table_and_the_old_words(prog, k):
    """A NaN in an occ_y column of problem 3's tau: its mean is not finite, the problem keeps its table and its words, status bit 4."""
    st = State(k, 40 + k)
    out = prog(st, 2, 1, SCHEDULE[0])
    compare(out, st.want(SCHEDULE[0]), SCHEDULE[0], "first call")
    st.move(out, SCHEDULE[0])
    st.tau = st.tau.copy()
    st.tau[3, 72] = np.nan
    st.learners[3].tau[0][72] = float("nan")
    old = (st.means[3].copy(), st.trans[3].copy(), st.thr[3].copy())
    out = prog(st, 2, 1, SCHEDULE[1])
    want = st.want(SCHEDULE[1])
    compare(out, want, SCHEDULE[1], "second call")
    assert out["status"][3] == 4 and out["status"][4] == 0
    assert _same(out["means"][3], old[0]) and _same(out["trans"][3], old[1]) and np.array_equal(out["thr"][3], old[2])
    assert np.isnan(out["rec"][3, 72]) and not _same(out["means"][4], st.means[4])


def test_the_rows_kernel_writes_the_new_rows_only(prog):
    """The rows launch alone decides the table region: rows [done, L) of the pieces, nothing before them, nothing behind them."""
    st = State(5, 3)
    out = prog(st, 1, 2, SCHEDULE[0])
    st.want(SCHEDULE[0])
    st.move(out, SCHEDULE[0])
    st.tab = np.full_like(st.tab, np.nan)                       # (forget the first call's rows: the second must not rewrite them)
    out = prog(st, 1, 2, SCHEDULE[1])
    for b, (d0, L) in enumerate(zip(SCHEDULE[0], SCHEDULE[1])):
        assert np.all(np.isnan(out["tab"][b, :d0])) and np.all(np.isnan(out["tab"][b, L:]))
        assert not np.any(np.isnan(out["tab"][b, d0:L, :5])) and np.all(np.isneginf(out["tab"][b, d0:L, 5:]))
