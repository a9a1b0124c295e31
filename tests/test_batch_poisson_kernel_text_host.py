"""batch_retable_poisson_kernel and batch_mstep_poisson_kernel (csrc/batch_poisson.hpp) as host code: the header's own text next to
batch_scale.hpp's and batch_retable.hpp's (the latter's include line naming tests/host_kernels/batch_retable_shim.hpp), built as a
stand-alone program with g++ -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off
(tests/host_kernels/batch_poisson_main.cpp) and run over grids from one workgroup a problem to the capped grid.  Every buffer has exactly
the size the host code hands the kernel, the table region is NaN on the way in -- an untouched padded row or a refused problem shows --,
and the rows, threshold words, status words, rates, log-rates, the M-step's tables and the log-factorials must equal
tests/poisson_ref.py's bit for bit.  Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 6 int64 {magic, B, k, T_max, gridDim.y, observes}, then the descriptors [B] {T int32, n int32, store int64},
the first observes [B] int64, the rates [B][k], the transition rows [B][k][k], the observes, the table region [B][T_max][8], the
threshold words [B][64], the rates and log-rates in force [B][8] each, the M-step's records [B][88] and its floor.  The output: the table
region, the threshold words, the status words [B] int32, the rates and log-rates in force, the M-step's rates, transition rows and
log-rates, then the log-factorials [4096]."""
import os
import re
import subprocess

import numpy as np
import pytest

import poisson_ref as P
import retable_ref as R
from test_poisson_ref_host import INVALID, fused_pairs, mstep_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b504f4953533031
DESC = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8")])
TS = [1, R.ROWS_PER_TRIP - 1, R.ROWS_PER_TRIP, R.ROWS_PER_TRIP + 1, 70, 70]
assert TS == [1, 31, 32, 33, 70, 70]
OLD_THR = np.uint64(0x1234)


def test_text():
    """fp contract off in every function, no library logarithm or lgamma, no fused multiply-add, no atomics, one barrier, LDS for the
    staged table alone, the one include; the library includes the header and launches both kernels."""
    text = open(os.path.join(CSRC, "batch_poisson.hpp")).read()
    assert text.count("#include") == 1 and '#include "batch_scale.hpp"' in text
    code = re.sub(r"//[^\n]*", "", text)
    bodies = re.findall(r"\n(?:__host__ __device__ inline|__global__)[^\n]*\)\n\{\n(.*?)\n\}\n", code, re.S)
    assert len(bodies) == 8                                    # (the six poisson_* functions and the two kernels)
    for body in bodies:
        assert body.lstrip().startswith("#pragma clang fp contract(off)"), body[:80]
    assert re.search(r"[^_\w]log\s*\(", code) is None and re.search(r"[^_\w]fma\s*\(", code) is None and "atomic" not in code and "lgamma" not in code
    assert code.count("__syncthreads") == 1 and code.count("__shared__") == 1
    # the row: three separate operations
    entry = code.split("poisson_entry(double y")[1].split("\n}\n")[0]
    assert "double r = y * log_rate;" in entry and "r = r - rate;" in entry and "r = r - lf[c];" in entry
    hip = open(os.path.join(CSRC, "cpprob_hip.hip")).read()
    assert '#include "batch_poisson.hpp"' in hip and "hipLaunchKernelGGL(batch_retable_poisson_kernel" in hip and "hipLaunchKernelGGL(batch_mstep_poisson_kernel" in hip


class Case:
    def __init__(self, k, seed, bad=()):
        rng = np.random.default_rng(seed)
        self.k, self.B, self.T, self.T_max = k, len(TS), np.array(TS), max(TS)
        self.rates = np.sort(np.exp(rng.uniform(-3.0, 4.0, (self.B, k))), axis=1)
        self.trans = rng.uniform(0.05, 1.0, (self.B, k, k))
        pairs = fused_pairs()
        self.rates[4, :] = [r for _, r in pairs[:k]]          # the pairs at which a fused row differs
        for b, what in bad:
            self.rates[b, {"zero": 0, "nan": 1, "subnormal": k - 1, "inf": 0}[what]] = {"zero": 0.0, "nan": np.nan, "subnormal": 1e-310, "inf": np.inf}[what]
        self.obs = rng.poisson(6.0, int(self.T.sum())).astype(np.float64)
        lo = int(np.sum(TS[:4]))
        self.obs[lo:lo + k] = [y for y, _ in pairs[:k]]
        self.obs[lo + k:lo + 2 * k] = [pairs[s][0] for s in range(k)][::-1]
        lo = int(np.sum(TS[:5]))
        self.obs[lo:lo + len(INVALID)] = INVALID               # a problem whose observes are no counts
        self.obs[lo + 10:lo + 14] = [0.0, 4095.0, 4094.0, 2048.0]
        self.stats = rng.uniform(0.1, 2.0, (self.B, R.RECORD))
        self.stats[1, 64] = 0.0                             # a state without mass
        self.stats[2, 72] = 0.0                             # a rate below the floor
        self.stats[3, 72] = np.nan
        self.floor = 1e-6


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_poisson_host"))
    retable = open(os.path.join(CSRC, "batch_retable.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert retable.count(inc) == 1
    open(os.path.join(d, "batch_retable.hpp"), "w").write(retable.replace(inc, '#include "batch_retable_shim.hpp"'))
    for name in ("batch_scale.hpp", "batch_poisson.hpp"):
        open(os.path.join(d, name), "w").write(open(os.path.join(CSRC, name)).read())
    exe = os.path.join(d, "batch_poisson_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_poisson_main.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(case, grid_y):
        B, k, T_max = case.B, case.k, case.T_max
        desc = np.zeros(B, DESC)
        desc["T"], desc["n"] = case.T, 7
        first = np.concatenate([[0], np.cumsum(case.T)[:-1]]).astype("<i8")
        head = np.array([MAGIC, B, k, T_max, grid_y, case.obs.size], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            for a in (head, desc, first, case.rates, case.trans, case.obs, np.full((B, T_max, 8), np.nan), np.full((B, 64), OLD_THR, np.uint64),
                      np.full((B, 8), -3.0), np.full((B, 8), -4.0), case.stats, np.array([case.floor])):
                f.write(np.ascontiguousarray(a).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        raw = open(fout, "rb").read()
        out, at = {}, 0
        for name, dt, shape in (("tab", "<f8", (B, T_max, 8)), ("thr", "<u8", (B, 64)), ("status", "<i4", (B,)), ("rate", "<f8", (B, 8)), ("log_rate", "<f8", (B, 8)),
                                ("m_rates", "<f8", (B, k)), ("m_trans", "<f8", (B, k, k)), ("m_log_rates", "<f8", (B, k)), ("lfact", "<f8", (P.MAX_COUNT + 1,))):
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            out[name] = np.frombuffer(raw[at:at + n], dt).reshape(shape)
            at += n
        assert at == len(raw)
        return out
    return run


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(case, out):
    k = case.k
    assert np.array_equal(_bits(out["lfact"]), _bits(P.LF_ARRAY))
    for b in range(case.B):
        bits = P.check(case.rates[b], case.trans[b], k)
        assert out["status"][b] == bits, b
        T = TS[b]
        lo = int(np.sum(TS[:b]))
        if bits:
            assert np.all(np.isnan(out["tab"][b])) and np.all(out["thr"][b] == OLD_THR)
            assert np.all(out["rate"][b] == -3.0) and np.all(out["log_rate"][b] == -4.0)
            continue
        assert np.array_equal(_bits(out["tab"][b, :T]), _bits(P.rows(case.obs[lo:lo + T], case.rates[b], k))), b
        assert np.all(np.isnan(out["tab"][b, T:]))
        assert np.array_equal(out["thr"][b], R.thresholds(case.trans[b], k))
        assert np.array_equal(out["rate"][b, :k], case.rates[b]) and np.all(out["rate"][b, k:] == -3.0)
        assert np.array_equal(_bits(out["log_rate"][b, :k]), _bits([P.S.table_log(r) for r in case.rates[b]])) and np.all(out["log_rate"][b, k:] == -4.0)
    for b in range(case.B):
        rt, lr, tr = P.m_step(case.stats[b], case.rates[b], np.full(k, -7.0), case.trans[b], k, case.floor)
        assert np.array_equal(_bits(out["m_rates"][b]), _bits(rt)) and np.array_equal(_bits(out["m_trans"][b]), _bits(tr)), b
        assert np.array_equal(_bits(out["m_log_rates"][b]), _bits(lr)), b


@pytest.mark.parametrize("k", [2, 5, 8])
@pytest.mark.parametrize("grid_y", [1, 2, 3])
def test_kernels_against_the_reference(prog, k, grid_y):
    case = Case(k, 200 + k, bad=((1, "subnormal"),) if grid_y == 1 else ((2, "zero"), (3, "nan")) if grid_y == 2 else ((0, "inf"),))
    out = prog(case, grid_y)
    _check(case, out)
    assert np.sum(out["status"] == P.BAD_RATE) >= 1
    assert out["m_rates"][2, 0] == case.floor and out["m_rates"][3, 0] == case.floor and out["m_rates"][1, 0] == case.rates[1, 0] and out["m_log_rates"][1, 0] == -7.0
    # the problem whose observes are no counts: rows of -inf, and the counts at the table's ends beside them
    assert np.all(np.isneginf(out["tab"][5, :len(INVALID)])) and np.all(np.isfinite(out["tab"][5, 10:14, :k]))


def test_mstep_edge_cases(prog):
    """The constructed records of tests/test_poisson_ref_host.py through the kernel's text."""
    for name, rec, rates, trans, floor in mstep_cases():
        case = Case(2, 7)
        case.rates[:], case.trans[:], case.stats[:], case.floor = rates, trans, rec, floor
        out = prog(case, 1)
        rt, lr, tr = P.m_step(rec, rates, np.full(2, -7.0), trans, 2, floor)
        for b in range(case.B):
            assert np.array_equal(_bits(out["m_rates"][b]), _bits(rt)) and np.array_equal(_bits(out["m_trans"][b]), _bits(tr)), name
            assert np.array_equal(_bits(out["m_log_rates"][b]), _bits(lr)), name
