"""batch_csmc_kernel (csrc/batch_csmc.hpp) as host code: the translation unit is formed here from the kernel header's own text -- its
include line names batch_csmc_pre.hpp, which is tests/host_kernels/batch_csmc_shim.hpp plus the texts of BatchProblem, batch_mass and
batch_mass_row cut out of csrc/batch_smc.hpp --, built as a stand-alone program with g++ -O1 -fsanitize=address,undefined
-fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_csmc_main.cpp).  Every buffer has exactly the size the
host code hands the kernel, rows of the m table no problem owns are NaN and must stay NaN, and the rows must equal tests/csmc_ref.py's,
bit for bit.  Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 10 int64 {magic, B, k, thr_stride, T_max, n (the batch's largest), 1: a described batch, microseconds by
which threads 0 .. 7 leave every barrier late, threshold words, entries of the reference paths}; a described batch's descriptors
{T, n, store} [B], order int32 [B] and first entries int64 [B]; the thresholds, the seeds, the per-step table [B][T_max][8] and the
reference paths (int8).  The output: the m table [B][T_max][8]."""
import os
import re
import subprocess

import numpy as np
import pytest

import backward_ref as R
import csmc_ref as CS
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b43534d43303031
PROB = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8")])


def _code(text):
    return re.sub(r"//[^\n]*", "", text)


def _texts():
    """(batch_csmc_pre.hpp, batch_csmc_host.hpp): every cut and every replaced line must be found exactly once."""
    smc = open(os.path.join(CSRC, "batch_smc.hpp")).read()
    defs = re.findall(r"^__host__ __device__ inline [^\n]*\bbatch_mass(?:_row)?\([^\n]*\)\n\{\n.*?^\}\n", smc, re.M | re.S)
    assert len(defs) == 2 and "batch_mass(" in defs[0] and "batch_mass_row(" in defs[1], defs
    prob = re.findall(r"^struct BatchProblem \{[^\n]*\};\nstatic_assert\(sizeof\(BatchProblem\) == 16[^\n]*\n", smc, re.M)
    assert len(prob) == 1, prob
    pre = '#pragma once\n#include "batch_csmc_shim.hpp"\nnamespace cph {\n' + prob[0] + "".join(defs) + "}  // namespace cph\n"
    kern = open(os.path.join(CSRC, "batch_csmc.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert kern.count(inc) == 1 and kern.count("#include") == 1
    return pre, kern.replace(inc, '#include "batch_csmc_pre.hpp"')


def test_kernel_header_keeps_its_promises():
    """One barrier, inside the step loop; no atomics; no dynamic LDS; the draw base; no other kernel header names the kernel, and the
    library includes it."""
    code = _code(open(os.path.join(CSRC, "batch_csmc.hpp")).read())
    assert code.count("__syncthreads") == 1 and "atomic" not in code.lower() and "extern __shared__" not in code
    head, loop = code.split("for (int t = 0; t < T; ++t) {", 1)
    assert "__syncthreads" in loop and "__syncthreads" not in head
    assert re.search(r"constexpr uint64_t kConditionalDrawBase = 1ull << 43;", code)
    assert re.search(r"[^_\w]fma\s*\(", code) is None and "double" in code       # (batch_mass_row's doubles; no arithmetic of its own)
    assert "batch_mass_row(cnt, ll, k, m)" in code
    for other in sorted(os.listdir(CSRC)):
        if other.endswith((".hpp", ".h")) and other != "batch_csmc.hpp":
            text = open(os.path.join(CSRC, other)).read()
            assert "batch_csmc" not in text and "kConditionalDrawBase" not in text, other
    hip = open(os.path.join(CSRC, "cpprob_hip.hip")).read()
    assert '#include "batch_csmc.hpp"' in hip and "hipLaunchKernelGGL(batch_csmc_kernel" in hip
    # 2^43 is this pass's alone
    for other in ("batch_smooth.hpp", "batch_forecast.hpp"):
        assert "1ull << 43" not in open(os.path.join(CSRC, other)).read()
    assert "1ull << 43" not in open(os.path.join(ROOT, "cpprob_amd", "include", "cpprob", "detail", "rng.hpp")).read()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_csmc_host"))
    pre, kern = _texts()
    open(os.path.join(d, "batch_csmc_pre.hpp"), "w").write(pre)
    open(os.path.join(d, "batch_csmc_host.hpp"), "w").write(kern)
    so = O.build()
    exe = os.path.join(d, "batch_csmc_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_csmc_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(bt, skew_us=0):
        """The m table [B, T_max, 8] the kernel leaves for batch `bt`."""
        head = np.array([MAGIC, bt.B, bt.k, bt.thr_stride, bt.T_max, bt.n_max, 1 if bt.described else 0, skew_us, bt.thr.size, bt.ref.size], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            if bt.described:
                f.write(bt.prob.tobytes())
                f.write(np.ascontiguousarray(bt.order, "<i4").tobytes())
                f.write(np.ascontiguousarray(bt.first, "<i8").tobytes())
            for arr, dt in ((bt.thr, np.uint64), (bt.seeds, np.uint64), (bt.tab, np.float64), (bt.ref, np.int8)):
                f.write(np.ascontiguousarray(arr, dt).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        assert len(raw) == 8 * 8 * bt.B * bt.T_max
        return np.frombuffer(raw, np.float64).reshape(bt.B, bt.T_max, 8)
    return run


class Batch:
    """Problems of lengths Ts and particle counts ns over k states; described: a table a problem (the second one's with a zero
    transition entry), descriptors, the host code's dispatch order (the longest chains first, ties by index) and first entries;
    else one shared table, every problem of T_max steps and n_max particles."""

    def __init__(self, Ts, ns, k, described, seed, zero_entry=False):
        rng = np.random.default_rng(seed)
        seeds = np.array([(7 << 40) + 1000 + 77 * b for b in range(len(Ts))], np.uint64)
        trans = rng.uniform(0.05, 1.0, (len(Ts) if described else 1, k, k))
        if zero_entry:
            trans[-1, 0, k - 1] = 0.0
            trans[-1, 1 % k, 0] = 0.0
        ll, paths = [], []
        for T in Ts:
            ll.append((-rng.uniform(0.0, 12.0, (T, k))).tolist())
            paths.append(rng.integers(0, k, T).astype(np.int8))
        self._fill(Ts, ns, k, described, seeds, [R.thresholds(tr) for tr in trans], ll, paths)

    @classmethod
    def given(cls, Ts, ns, k, described, seeds, rows, ll, paths):
        """A batch over tables, log-likelihoods and reference bytes the caller states: rows[i] = backward_ref.thresholds of table i (one
        a problem, or one for all), ll[b] = [T_b][k] floats, paths[b] = T_b reference bytes (any int8 values)."""
        bt = cls.__new__(cls)
        bt._fill(Ts, ns, k, described, np.array(seeds, np.uint64), [list(r) for r in rows], [[list(map(float, r)) for r in x] for x in ll],
                 [np.asarray(p).astype(np.int8) for p in paths])
        return bt

    def _fill(self, Ts, ns, k, described, seeds, rows, ll, paths):
        self.Ts, self.ns, self.k, self.B, self.described = list(Ts), list(ns), k, len(Ts), described
        self.T_max, self.n_max = max(Ts), max(ns)
        assert described or (len(set(Ts)) == 1 and len(set(ns)) == 1)
        assert len(rows) == (self.B if described else 1) and len(ll) == len(paths) == len(seeds) == self.B
        self.seeds = seeds
        self.rows = rows
        self.thr = np.full((len(rows), 8, 8), np.iinfo(np.uint64).max, np.uint64)           # (words behind a row's k - 1 entries: all ones)
        for i, rows_i in enumerate(self.rows):
            for s, row in enumerate(rows_i):
                self.thr[i, s, :k - 1] = row
        self.thr_stride = 64 if described else 0
        self.tab = np.zeros((self.B, self.T_max, 8))
        self.ll, self.paths = ll, paths
        for b, T in enumerate(self.Ts):
            assert len(ll[b]) == len(paths[b]) == T
            self.tab[b, :T, :k] = np.array(ll[b])
        self.ref = np.concatenate(self.paths)
        self.first = np.concatenate([[0], np.cumsum(self.Ts)])[:-1].astype(np.int64)
        self.prob = np.zeros(self.B, PROB)
        self.prob["T"], self.prob["n"] = self.Ts, self.ns
        cost = [T * (-(-n // 1024)) for T, n in zip(self.Ts, self.ns)]
        self.order = sorted(range(self.B), key=lambda b: -cost[b])                          # (sorted is stable: ties by index)

    def want(self):
        out = np.full((self.B, self.T_max, 8), np.nan)
        for b, (T, n) in enumerate(zip(self.Ts, self.ns)):
            out[b, :T] = 0.0
            out[b, :T, :self.k] = np.array(CS.masses(self.ll[b], self.rows[b if self.described else 0], int(self.seeds[b]), n, self.paths[b]), np.float64)
        return out


def _same(got, want):
    return np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("k", [2, 5, 8])
def test_rows_are_the_references_on_a_ragged_described_batch(prog, k):
    """n in {1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 2049}: a partial run of 4, a partial pass, more than one pass; T in {1, 2, 7};
    a table with zero transition entries; an order that is not the identity; the rows past a problem's length stay NaN."""
    ns = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 2049]
    Ts = [2, 7, 1, 2, 7, 1, 2, 7, 2, 7, 1]
    bt = Batch(Ts, ns, k, True, 40 + k, zero_entry=True)
    assert bt.order != list(range(bt.B))
    want = bt.want()
    assert np.isnan(want).any()
    got = prog(bt)
    assert _same(got, want), "rows differ from the reference in problems %s" % sorted({int(b) for b in np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:, 0]})
    assert np.all(np.nansum(want[:, :, :k] > 0, axis=2)[~np.isnan(want[:, :, 0])] >= 1)


def test_the_count_field_limit_on_a_uniform_batch(prog):
    """n = 8192, the most a problem holds: eight passes, and a generation crowded into one state fills its 16-bit count field to
    8192 (a table whose every row sends nearly all mass to state 0)."""
    bt = Batch([3, 3], [8192, 8192], 5, False, 9)
    crowd = np.full((5, 5), 1e-7)
    crowd[:, 0] = 1.0
    bt.rows = [R.thresholds(crowd)]
    for s, row in enumerate(bt.rows[0]):
        bt.thr[0, s, :4] = row
    want = bt.want()
    xs = CS.states(bt.ll[0], bt.rows[0], int(bt.seeds[0]), 8192, bt.paths[0])[0]
    assert np.sum(xs[1:] == 0, axis=1).max() >= 8100, "state 0 should hold nearly every particle of a later generation"
    assert _same(prog(bt), want)


def test_a_uniform_batch_and_the_skewed_barrier_schedule(prog):
    """One shared table, every problem T = 7 and n = 1025; then the same with threads 0 .. 7 leaving every barrier late: a
    wavefront's totals of step t must survive until every thread has read them."""
    bt = Batch([7, 7, 7], [1025, 1025, 1025], 5, False, 21)
    want = bt.want()
    assert not np.isnan(want).any()
    assert _same(prog(bt), want)
    assert _same(prog(bt, skew_us=300), want)
    rag = Batch([7, 2, 5], [300, 5, 1025], 3, True, 23)
    assert _same(prog(rag, skew_us=300), rag.want())


def test_a_reference_entry_past_k_is_taken_as_the_last_state(prog):
    bt = Batch([4, 4], [6, 6], 3, False, 31)
    bad = Batch([4, 4], [6, 6], 3, False, 31)
    bt.paths = [np.array([2, 2, 0, 1], np.int8), np.array([1, 2, 2, 2], np.int8)]
    bad.paths = [np.array([3, 7, 0, 1], np.int8), np.array([1, 5, 6, 2], np.int8)]
    bt.ref, bad.ref = np.concatenate(bt.paths), np.concatenate(bad.paths)
    assert _same(prog(bad), bt.want()) and _same(prog(bt), bt.want())
