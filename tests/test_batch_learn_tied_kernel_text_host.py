"""batch_learn_tied_kernel and batch_learn_tied_scaled_kernel (csrc/batch_learn_tied.hpp) as host code: the translation unit of
tests/test_batch_learn_kernel_text_host.py with csrc/batch_pool.hpp's and the new header's text on top (their include lines naming
those texts), built against tests/host_kernels/batch_smooth_shim.hpp and batch_retable_shim.hpp as a stand-alone program with g++ -O1
-fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_learn_tied_main.cpp).  The
program runs the three launches of a tied learning advance behind its run -- the learn kernel with t_min = INT32_MAX, the pooling
kernel (compact, R = 1), the tied kernel -- on the grids the library launches.  Every buffer has exactly the size the host code hands
the kernels; the status words, the tables of every member but a group's first (the one the M-step starts from) and, on a scaled batch,
their sigmas and log_norms are poisoned on the way in, and tau of a problem that has consumed nothing is NaN.  Records, pooled records,
tau, tables, scales, threshold words and status words must equal tests/learn_tied_ref.py's TiedLearner bit for bit, call after call.
Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 11 int64 {magic, B, k, t_min, G, rows of the m table, observes, step sizes, scaled, fit, gridDim.x of the
learn launch}, then the smoothing descriptors [B], the members sorted by (group, problem) [B] int32, the groups' first positions
[G + 1] int32, the threshold words [B][64], the m table, the new observes, gamma, tau [B][8][88], the means [B][k], the transition rows
[B][k][k], the status words [B] int32, scaled: the sigmas [B][8] and the log_norms [B][8], and the floor.  The output: the records
[B][88], the pooled records [G][88], tau, the means, the transition rows, the words, the status words, scaled: sigmas and log_norms."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import learn_ref as G
import learn_tied_ref as T
import pool_ref as P
import test_batch_learn_kernel_text_host as KL
import test_batch_pool_kernel_text_host as KP
import test_batch_suffstats_kernel_text_host as K
from oracle import oracle as O

ROOT, HERE, CSRC = KL.ROOT, KL.HERE, KL.CSRC
MAGIC = 0x4b4c544945443031
TAU, POISON, LOG_NORM = KL.TAU, KL.POISON, KL.LOG_NORM
FLOOR = 1e-3
K_WAVES = 4

# Twelve problems in six groups, the memberships interleaved; two workgroups of the tied launch, the last one holding two groups.
#   group 0 = {0}          a singleton; nothing new in the third call, where others fire: its status stays 0
#   group 1 = {1, 4}       problem 4 has length 0 for good
#   group 2 = {2, 6, 9}    all three advance in the first call, problem 6 alone in the second, problem 2 alone in the third
#   group 3 = {3, 7}       3 observes after the first call (no M-step), nothing new in the second (status poisoned, words old), 9 after the
#                          third: it crosses the burn-in by its members' sum while neither has reached it alone
#   group 4 = {5, 8, 10}   5 observes, then 8: crosses the burn-in in the second call by the sum, no member beyond 3
#   group 5 = {11}         a singleton in the last workgroup; nothing new in the second call
GROUPS = [0, 1, 2, 3, 1, 4, 2, 3, 4, 2, 4, 5]
SCHEDULE = [[2, 3, 4, 1, 0, 2, 4, 2, 2, 3, 1, 6],
            [7, 8, 4, 1, 0, 3, 6, 2, 2, 3, 3, 6],
            [7, 12, 9, 5, 0, 3, 6, 4, 4, 3, 5, 10]]
TS = SCHEDULE[-1]
NS = [5, 3, 9, 1, 4, 7, 3, 40, 9, 6, 2, 8]
T_MIN = 6
FIRES = [[0, 0, 1, 0, 0, 1], [1, 1, 1, 0, 1, 0], [0, 1, 1, 1, 1, 1]]      # [call][group], as the firing rule has it on SCHEDULE


def _texts():
    texts = dict(KL._texts())
    texts["batch_pool_host.hpp"] = KP._text()[1]
    text = open(os.path.join(CSRC, "batch_learn_tied.hpp")).read()
    incs = ('#include "batch_learn.hpp"', '#include "batch_pool.hpp"')
    assert all(text.count(i) == 1 for i in incs) and text.count("#include") == 2
    texts["batch_learn_tied_host.hpp"] = text.replace(incs[0], '#include "batch_learn_host.hpp"').replace(incs[1], '#include "batch_pool_host.hpp"')
    return texts


def test_text():
    """fp contract off in every function (the body and the two kernels over it, each the pragma and one call of the body), no power,
    no exponential, no logarithm, no fused multiply-add, no LDS, no barrier, no atomics, no striding; the member list is read through
    the tie's arrays; the library includes the header and launches both kernels."""
    text = open(os.path.join(CSRC, "batch_learn_tied.hpp")).read()
    code = re.sub(r"//[^\n]*", "", text)
    for word in ("__shared__", "__syncthreads", "atomic", "pow(", "exp(", "gridDim"):
        assert word not in code, word
    assert re.search(r"[^_\w]log\s*\(", code) is None and re.search(r"[^_\w]fma\s*\(", code) is None
    bodies = re.findall(r"\n(?:__device__ __forceinline__|__global__)[^\n]*\)\n\{\n(.*?)\n\}\n", code, re.S)
    assert len(bodies) == 3
    for body in bodies:
        assert body.lstrip().startswith("#pragma clang fp contract(off)"), body[:80]
    kernels = re.findall(r"\n__global__[^\n]* void (\w+)\([^\n]*\)\n\{\n(.*?)\n\}\n", code, re.S)
    assert [name for name, _ in kernels] == ["batch_learn_tied_kernel", "batch_learn_tied_scaled_kernel"]
    for (name, body), call in zip(kernels, ("batch_learn_tied_body<false>", "batch_learn_tied_body<true>")):
        assert re.fullmatch(r"#pragma clang fp contract\(off\)\n\s*" + re.escape(call) + r"\(\w+\);", body.strip()), (name, body)
    assert "a.members[" in code and "a.first[g + 1]" in code
    hip = open(os.path.join(CSRC, "cpprob_hip.hip")).read()
    assert '#include "batch_learn_tied.hpp"' in hip and "hipLaunchKernelGGL(batch_learn_tied_kernel" in hip and "hipLaunchKernelGGL(batch_learn_tied_scaled_kernel" in hip


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_learn_tied_host"))
    for name, text in _texts().items():
        open(os.path.join(d, name), "w").write(text)
    so = O.build()
    exe = os.path.join(d, "batch_learn_tied_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_learn_tied_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(st, lens, learn_gx=2):
        """One tied learning advance to the lengths `lens` on the state st (a State): returns the outputs and moves nothing."""
        B, k = st.B, st.k
        desc = np.zeros(B, K.DESC)
        obs, at = [], 0
        mass = st.bt.mass.copy()
        for b, (d0, L) in enumerate(zip(st.done, lens)):
            desc[b] = (L, 1, 0, st.bt.rows[b], at, 0, L, d0, 0)
            obs.append(st.bt.obs[b][d0:L])
            at += L - d0
            mass[st.bt.rows[b] + L:st.bt.rows[b + 1]] = np.nan
        obs = np.concatenate(obs)
        mem = P.members(GROUPS)
        first = np.concatenate([[0], np.cumsum([len(m) for m in mem])])
        head = np.array([MAGIC, B, k, st.t_min, len(mem), mass.shape[0], obs.size, st.gamma.size, int(st.scaled), 0 if st.floor is None else 1, learn_gx], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        arrays = [(desc, K.DESC), (np.concatenate(mem), "<i4"), (first, "<i4"), (st.thr, np.uint64), (mass, np.float64), (obs, np.float64), (st.gamma, np.float64),
                  (st.tau, np.float64), (st.means, np.float64), (st.trans, np.float64), (st.status, "<i4")]
        if st.scaled:
            arrays += [(st.sigmas, np.float64), (st.log_norms, np.float64)]
        arrays.append((np.array([st.floor or 0.0]), np.float64))
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            for arr, dt in arrays:
                f.write(np.ascontiguousarray(arr, dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        at = [0]

        def take(n, dt):
            a = np.frombuffer(raw, dt, n, at[0])
            at[0] += a.nbytes
            return a.copy()
        out = dict(rec=take(B * G.RECORD, np.float64).reshape(B, G.RECORD), pooled=take(len(mem) * G.RECORD, np.float64).reshape(len(mem), G.RECORD),
                   tau=take(B * TAU, np.float64).reshape(B, TAU), means=take(B * k, np.float64).reshape(B, k), trans=take(B * k * k, np.float64).reshape(B, k, k),
                   thr=take(B * 64, np.uint64).reshape(B, 64), status=take(B, np.int32))
        if st.scaled:
            out["sigmas"], out["log_norms"] = take(B * 8, np.float64).reshape(B, 8), take(B * 8, np.float64).reshape(B, 8)
        assert at[0] == len(raw)
        return out
    return run


class State:
    """The device state of a tied learning stream between two advances, and the reference beside it.  scaled: the batch has emission
    scales; floor None on a scaled batch: a plain arming, which keeps them."""

    def __init__(self, k, seed, scaled=False, floor=None):
        self.bt = K.Batch(TS, NS, k, False, seed)
        rng = np.random.default_rng(seed + 1000)
        self.B, self.k, self.t_min, self.scaled, self.floor = len(TS), k, T_MIN, scaled, floor
        self.mem = P.members(GROUPS)
        self.gamma = (np.arange(max(TS)) + 1.0) ** -0.6
        nG = len(self.mem)
        gm, gt, gs = rng.normal(0.0, 3.0, (nG, k)), rng.uniform(0.05, 1.0, (nG, k, k)), rng.uniform(0.4, 2.5, (nG, k))
        gt[2, 0, k - 1] = 0.0                   # group 2's table has a zero transition entry
        grp = np.array(GROUPS)
        self.ref = T.TiedLearner(gm[grp], gt[grp], k, GROUPS, self.gamma, T_MIN, LOG_NORM, sigmas=gs[grp] if scaled else None, floor=floor)
        for lr in self.ref.learners:
            lr.status = POISON
        self.thr = np.stack([lr.thr for lr in self.ref.learners])
        self.tau = np.full((self.B, TAU), np.nan)               # (a problem that has consumed nothing: never read)
        self.status = np.full(self.B, POISON, np.int32)
        # the tables: real where the M-step starts from them -- a group's first member --, poisoned in every other member
        lead = np.array([b == self.mem[g][0] for b, g in enumerate(GROUPS)])
        self.means, self.trans = np.where(lead[:, None], gm[grp], np.nan), np.where(lead[:, None, None], gt[grp], np.nan)
        self.sigmas, self.log_norms = np.full((self.B, 8), -3.0), np.full((self.B, 8), -4.0)
        if scaled:
            for b in np.flatnonzero(lead):
                self.sigmas[b, :k], self.log_norms[b, :k] = self.ref.learners[b].sigmas, self.ref.learners[b].log_norms
        self.done = [0] * self.B

    def want(self, lens):
        """Moves the reference to `lens`; returns what the program must leave and the groups that fired."""
        fired0, L = list(self.ref.fired), self.ref.learners
        self.ref.advance([self.bt.m[b][d0:n] for b, (d0, n) in enumerate(zip(self.done, lens))], [self.bt.obs[b][d0:n] for b, (d0, n) in enumerate(zip(self.done, lens))])
        fires = [self.ref.fired[g] - fired0[g] for g in range(len(self.mem))]
        w = dict(rec=self.ref.records(), pooled=self.ref.pooled, tau=[G.tau_array(lr.tau) for lr in L], means=self.means.copy(), trans=self.trans.copy(),
                 thr=self.thr.copy(), status=self.status.copy(), sigmas=self.sigmas.copy(), log_norms=self.log_norms.copy())
        for g, mem in enumerate(self.mem):
            for b in mem:
                if not fires[g]:
                    continue                                    # (tables, scales, words and status words as they were: poisoned or old)
                w["status"][b] = L[b].status
                if L[b].status == 0:
                    w["means"][b], w["trans"][b], w["thr"][b] = L[b].means, L[b].trans, L[b].thr
                    if self.scaled and self.floor is not None:
                        w["sigmas"][b, :self.k], w["log_norms"][b, :self.k] = L[b].sigmas, L[b].log_norms
        return w, fires

    def move(self, out, lens):
        self.tau, self.means, self.trans, self.thr, self.status, self.done = out["tau"], out["means"], out["trans"], out["thr"], out["status"], list(lens)
        if self.scaled:
            self.sigmas, self.log_norms = out["sigmas"], out["log_norms"]


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def compare(st, out, want, lens, note):
    assert np.array_equal(out["status"], want["status"]), "%s: status %s, want %s" % (note, out["status"], want["status"])
    assert _same(out["rec"], want["rec"]), "%s: records" % note
    assert _same(out["pooled"], want["pooled"]), "%s: pooled records" % note
    for b, L in enumerate(lens):
        if L > 0:
            assert _same(out["tau"][b], want["tau"][b]), "%s, problem %d: tau" % (note, b)
        else:
            assert np.all(np.isnan(out["tau"][b])), "a problem of length 0 stores no tau"
    assert _same(out["means"], want["means"]) and _same(out["trans"], want["trans"]), "%s: tables" % note
    assert np.array_equal(out["thr"], want["thr"]), "%s: threshold words" % note
    if st.scaled:
        assert _same(out["sigmas"], want["sigmas"]) and _same(out["log_norms"], want["log_norms"]), "%s: scales" % note


def _stream(prog, st, note):
    """The three calls of SCHEDULE with the events that make the case mean something."""
    k, mem = st.k, st.mem
    for call, lens in enumerate(SCHEDULE):
        before = (st.means.copy(), st.trans.copy(), st.thr.copy(), st.status.copy())
        out = prog(st, lens, learn_gx=1 + call % 2)
        want, fires = st.want(lens)
        compare(st, out, want, lens, "%s, call %d" % (note, call))
        assert fires == FIRES[call], "call %d: %s" % (call, fires)
        for g, m in enumerate(mem):
            if fires[g]:
                assert all(out["status"][b] == 0 for b in m) and all(_same(out["means"][b], out["means"][m[0]]) and _same(out["trans"][b], out["trans"][m[0]]) for b in m)
                assert not np.isnan(out["means"][m]).any() and not np.isnan(out["trans"][m]).any(), "the broadcast overwrites every member's poison"
            else:
                assert all(_same(out["means"][b], before[0][b]) and _same(out["trans"][b], before[1][b]) and np.array_equal(out["thr"][b], before[2][b]) for b in m)
                assert np.array_equal(out["status"][m], before[3][m])
        assert np.all(out["rec"][4] == 0.0), "a member of length 0 contributes 88 zeros"
        st.move(out, lens)
        if call == 0:
            assert list(out["status"][[3, 7]]) == [POISON, POISON] and np.isnan(out["means"][7]).all(), "group 3 has seen 3 observes"
        if call == 1:
            assert list(out["status"][[3, 7]]) == [POISON, POISON], "group 3 does not advance in the second call"
            assert list(out["status"][[5, 8, 10]]) == [0, 0, 0] and max(lens[b] for b in (5, 8, 10)) < T_MIN <= sum(lens[b] for b in (5, 8, 10))
        if call == 2:
            assert list(out["status"][[3, 7]]) == [0, 0] and max(lens[3], lens[7]) < T_MIN <= lens[3] + lens[7]
            assert not out["status"].any() and st.ref.changed[2] == 3 and st.ref.changed[0] == 1
    return out


@pytest.mark.parametrize("k", [2, 5, 8])
def test_three_calls_give_the_references_bits(prog, k):
    st = State(k, 7 + k)
    _stream(prog, st, "unit, k %d" % k)
    assert not st.scaled


@pytest.mark.parametrize("k", [2, 5, 8])
@pytest.mark.parametrize("fit", [True, False], ids=["fitted", "kept"])
def test_three_scaled_calls_give_the_references_bits(prog, k, fit):
    st = State(k, 17 + k, scaled=True, floor=FLOOR if fit else None)
    start = (st.sigmas.copy(), st.log_norms.copy())
    out = _stream(prog, st, "scaled (%s), k %d" % ("fitted" if fit else "kept", k))
    if fit:
        lead = [0, 1, 2, 3, 5, 11]
        assert np.all(np.any(out["sigmas"][lead, :k] != start[0][lead, :k], axis=1)) and np.all(out["sigmas"][:, k:] == -3.0)
        assert not np.any(out["sigmas"][:, :k] == -3.0), "every member has received its group's scales"
    else:
        assert _same(out["sigmas"], start[0]) and _same(out["log_norms"], start[1]), "a plain arming never writes the scales"


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "scaled"])
def test_a_refused_pooled_m_step_leaves_every_member_its_table_and_the_bits(prog, scaled):
    """A NaN in an occ_y column of problem 6's tau: the pooled record of group 2 = {2, 6, 9} carries it, the group's mean is not finite,
    every member keeps its table, its scales and its words and receives bit 4; the other groups move on."""
    k = 3
    st = State(k, 40, scaled=scaled, floor=FLOOR if scaled else None)
    out = prog(st, SCHEDULE[0])
    want, _ = st.want(SCHEDULE[0])
    compare(st, out, want, SCHEDULE[0], "first call")
    st.move(out, SCHEDULE[0])
    st.tau = st.tau.copy()
    st.tau[6, 72] = np.nan
    st.ref.learners[6].tau[0][72] = float("nan")
    old = (st.means.copy(), st.trans.copy(), st.thr.copy(), st.sigmas.copy(), st.log_norms.copy())
    out = prog(st, SCHEDULE[1])
    want, fires = st.want(SCHEDULE[1])
    compare(st, out, want, SCHEDULE[1], "second call")
    assert fires == FIRES[1] and list(out["status"][[2, 6, 9]]) == [4, 4, 4] and list(out["status"][[0, 1, 4, 5, 8, 10]]) == [0] * 6
    assert np.isnan(out["pooled"][2, 72]) and not np.isnan(out["pooled"][[0, 1, 3, 4, 5]]).any()
    for b in (2, 6, 9):
        assert _same(out["means"][b], old[0][b]) and _same(out["trans"][b], old[1][b]) and np.array_equal(out["thr"][b], old[2][b])
        if scaled:
            assert _same(out["sigmas"][b], old[3][b]) and _same(out["log_norms"][b], old[4][b])
    assert not _same(out["means"][5], old[0][5])
