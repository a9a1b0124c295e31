"""batch_learn_rows_scaled_kernel and batch_learn_scaled_kernel (csrc/batch_learn.hpp: the kScaled instantiations of its two bodies) as
host code: the translation unit of tests/test_batch_learn_kernel_text_host.py, built as a stand-alone program with g++ -O1
-fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_learn_scaled_main.cpp).  Records, tau, tables, sigmas, log_norms, threshold words, status
words and rows must equal tests/scale_ref.py's ScaledLearner on every grid, call after call: the learner's step (c) -- the scale of a
state with mass, its logarithm only where the scale passes, bit 8 gathered on the rows' lanes -- and the rows from the resident
scales.  Nothing is loaded into python and nothing runs on a GPU.

The case file: batch_learn_main.cpp's with an eleventh header word (the learner fits the scales) and, in log_norm's place, the sigmas
[B][8], the log_norms [B][8] and the floor.  The output: that program's, then the sigmas and the log_norms."""
import os
import re
import subprocess

import numpy as np
import pytest

import learn_ref as G
import scale_ref as S
import test_batch_learn_kernel_text_host as KL
import test_batch_suffstats_kernel_text_host as K
from oracle import oracle as O

ROOT, HERE, CSRC = KL.ROOT, KL.HERE, KL.CSRC
MAGIC = 0x4b4c524e53433031
TAU, PROB, POISON, SCHEDULE, T_MIN = KL.TAU, KL.PROB, KL.POISON, KL.SCHEDULE, KL.T_MIN
FLOOR = 1e-3


_texts = KL._texts


def test_text():
    """fp contract off in every function, no power, no library logarithm, no LDS, no barrier, no atomics; the unit and the scaled
    learner are one text -- one loop over the problems and one walk over the steps in the file, and each of the four kernels is the
    pragma and a single call of its body --; the library launches both kernels."""
    text = open(os.path.join(CSRC, "batch_learn.hpp")).read()
    code = re.sub(r"//[^\n]*", "", text)
    for word in ("__shared__", "__syncthreads", "atomic", "pow(", "exp("):
        assert word not in code, word
    assert re.search(r"[^_\w]log\s*\(", code) is None and re.search(r"[^_\w]fma\s*\(", code) is None
    assert code.count("for (int b = online_uniform(") == 1 and code.count("for (int t = done; t < T; ++t)") == 1
    kernels = re.findall(r"\n__global__[^\n]* void (\w+)\([^\n]*\)\n\{\n(.*?)\n\}\n", code, re.S)
    assert [name for name, _ in kernels] == ["batch_learn_rows_kernel", "batch_learn_rows_scaled_kernel", "batch_learn_kernel", "batch_learn_scaled_kernel"]
    for (name, body), call in zip(kernels, ("batch_learn_rows_body<false>", "batch_learn_rows_body<true>", "batch_learn_body<false>", "batch_learn_body<true>")):
        assert re.fullmatch(r"#pragma clang fp contract\(off\)\n\s*" + re.escape(call) + r"\(\w+\);", body.strip()), (name, body)
    hip = open(os.path.join(CSRC, "cpprob_hip.hip")).read()
    assert '#include "batch_learn.hpp"' in hip and "hipLaunchKernelGGL(batch_learn_scaled_kernel" in hip and "hipLaunchKernelGGL(batch_learn_rows_scaled_kernel" in hip


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_learn_scaled_host"))
    for name, text in _texts().items():
        open(os.path.join(d, name), "w").write(text)
    so = O.build()
    exe = os.path.join(d, "batch_learn_scaled_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_learn_scaled_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(st, grid_x, rows_gy, lens):
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
        head = np.array([MAGIC, B, k, st.t_min, grid_x, mass.shape[0], obs.size, st.gamma.size, T_max, rows_gy, 0 if st.floor is None else 1], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            for arr, dt in ((desc, K.DESC), (prob, PROB), (first, "<i4"), (ofirst, "<i8"), (st.thr, np.uint64), (mass, np.float64), (obs, np.float64),
                            (st.gamma, np.float64), (st.tau, np.float64), (st.means, np.float64), (st.trans, np.float64), (st.status, "<i4"),
                            (st.tab, np.float64), (st.sigmas, np.float64), (st.log_norms, np.float64), (np.array([st.floor or 0.0]), np.float64)):
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
                   thr=take(B * 64, np.uint64).reshape(B, 64), status=take(B, np.int32), tab=take(B * T_max * 8, np.float64).reshape(B, T_max, 8),
                   sigmas=take(B * 8, np.float64).reshape(B, 8), log_norms=take(B * 8, np.float64).reshape(B, 8))
        assert at[0] == len(raw)
        return out
    return run


class State(KL.State):
    """test_batch_learn_kernel_text_host.State with the scales [B][8] (the entries of the states >= k poisoned) and ScaledLearners."""

    def __init__(self, k, seed, floor=FLOOR):
        super().__init__(k, seed)
        rng = np.random.default_rng(seed + 2000)
        self.floor = floor
        sg = rng.uniform(0.4, 2.5, (self.B, k))
        self.learners = [S.ScaledLearner(self.means[b], self.trans[b], sg[b], k, self.gamma, T_MIN, floor) for b in range(self.B)]
        for lr in self.learners:
            lr.status = POISON
        self.sigmas, self.log_norms = np.full((self.B, 8), -3.0), np.full((self.B, 8), -4.0)
        self.sigmas[:, :k] = sg
        self.log_norms[:, :k] = np.stack([lr.log_norms for lr in self.learners])

    def want(self, lens):
        w = super().want(lens)
        w["sigmas"], w["log_norms"] = np.full((self.B, 8), -3.0), np.full((self.B, 8), -4.0)
        w["sigmas"][:, :self.k] = np.stack([lr.sigmas for lr in self.learners])
        w["log_norms"][:, :self.k] = np.stack([lr.log_norms for lr in self.learners])
        return w

    def move(self, out, lens):
        super().move(out, lens)
        self.sigmas, self.log_norms = out["sigmas"], out["log_norms"]


def compare(out, want, lens, note):
    KL.compare(out, want, lens, note)
    assert KL._same(out["sigmas"], want["sigmas"]), "%s: sigmas" % note
    assert KL._same(out["log_norms"], want["log_norms"]), "%s: log_norms" % note


@pytest.mark.parametrize("k", [2, 5, 8])
def test_every_grid_gives_the_references_bits_call_after_call(prog, k):
    """gridDim.x in {1, 2} and rows launches of 1 and 3 workgroups a problem, three calls (a few steps; a resume in which problem 5
    crosses the burn-in; a last one with nothing new for some problems), the learner fitting the scales."""
    for gx, gy in ((1, 1), (2, 3)):
        st = State(k, 7 + k)
        start = st.sigmas.copy()
        for call, lens in enumerate(SCHEDULE):
            out = prog(st, gx, gy, lens)
            compare(out, st.want(lens), lens, "k %d, grid %d x %d, call %d" % (k, gx, gy, call))
            for b, L in enumerate(lens):
                assert np.all(np.isnan(out["tab"][b, L:])) and not np.any(np.isnan(out["tab"][b, :L]))
            st.move(out, lens)
        assert list(out["status"]) == [POISON, POISON, POISON, 0, 0, 0, 0]
        assert not KL._same(out["sigmas"][3], start[3]) and KL._same(out["sigmas"][:3], start[:3]), "a problem no M-step visits keeps its scales"


def test_a_plain_arming_reads_the_scales_and_never_writes_them(prog):
    st = State(5, 21, floor=None)
    start = (st.sigmas.copy(), st.log_norms.copy())
    for call, lens in enumerate(SCHEDULE):
        out = prog(st, 2, 1, lens)
        compare(out, st.want(lens), lens, "call %d" % call)
        st.move(out, lens)
    assert KL._same(out["sigmas"], start[0]) and KL._same(out["log_norms"], start[1]) and not KL._same(out["means"][3], st.learners[3].means * 0.0)
    assert all(lr.changed >= 1 for lr in st.learners[3:])


@pytest.mark.parametrize("case", ["subnormal", "overflow", "nan mean"])
def test_a_bad_scaled_m_step_keeps_table_scales_and_words(prog, case):
    """Problem 3's second M-step is refused -- a floor of 1e-160 under a variance of 0 (2 pi sigma^2 subnormal: bit 8), an occ_yy column
    of infinity (the scale overflows: bit 8), a NaN occ_y (the mean: bit 4; the variance is NaN and takes the floor) -- and the problem
    keeps its table, its sigmas, its log_norms and its words, while problem 4 moves on."""
    k = 3
    st = State(k, 40, floor=1e-160 if case == "subnormal" else FLOOR)
    out = prog(st, 2, 1, SCHEDULE[0])
    compare(out, st.want(SCHEDULE[0]), SCHEDULE[0], "first call")
    st.move(out, SCHEDULE[0])
    st.tau = st.tau.copy()
    for s in range(k):
        if case == "subnormal":                                  # (every observe of the problem and every y-column of its tau: 0)
            st.tau[3, s * G.RECORD + 72:s * G.RECORD + 88] = 0.0
            for j in range(72, 88):
                st.learners[3].tau[s][j] = 0.0
        elif case == "overflow":
            st.tau[3, s * G.RECORD + 80 + s] = np.inf
            st.learners[3].tau[s][80 + s] = float("inf")
        else:
            st.tau[3, s * G.RECORD + 72 + s] = np.nan
            st.learners[3].tau[s][72 + s] = float("nan")
    if case == "subnormal":
        st.bt.obs[3] = np.zeros_like(st.bt.obs[3])
    old = (st.means[3].copy(), st.trans[3].copy(), st.thr[3].copy(), st.sigmas[3].copy(), st.log_norms[3].copy())
    out = prog(st, 2, 1, SCHEDULE[1])
    compare(out, st.want(SCHEDULE[1]), SCHEDULE[1], "second call")
    assert out["status"][3] == (4 if case == "nan mean" else S.BAD_SCALE) and out["status"][4] == 0
    assert KL._same(out["means"][3], old[0]) and KL._same(out["trans"][3], old[1]) and np.array_equal(out["thr"][3], old[2])
    assert KL._same(out["sigmas"][3], old[3]) and KL._same(out["log_norms"][3], old[4]) and not KL._same(out["sigmas"][4], st.sigmas[4])
