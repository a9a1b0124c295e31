"""batch_retable_scaled_kernel and batch_mstep_scaled_kernel (csrc/batch_scale.hpp) as host code: the header's own text next to
batch_retable.hpp's (its include line naming tests/host_kernels/batch_retable_shim.hpp), built as a stand-alone program with g++ -O1
-fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_scale_main.cpp) and run over
grids from one workgroup a problem to the capped grid.  Every buffer has exactly the size the host code hands the kernel, the table
region is NaN on the way in -- an untouched padded row or a refused problem shows --, and the rows, threshold words, status words,
sigmas, log_norms, the M-step's tables and the logarithms must equal tests/scale_ref.py's bit for bit.  Nothing is loaded into python
and nothing runs on a GPU.

The case file: a header of 7 int64 {magic, B, k, T_max, gridDim.y, observes, logarithm arguments}, then the descriptors [B] {T int32,
n int32, store int64}, the first observes [B] int64, the means [B][k], the sigmas [B][k], the transition rows [B][k][k], the observes,
the table region [B][T_max][8], the threshold words [B][64], the sigmas and log_norms in force [B][8] each, the M-step's records
[B][88], its floor and the logarithm's arguments.  The output: the table region, the threshold words, the status words [B] int32, the
sigmas and log_norms in force, the M-step's means, transition rows, sigmas and log_norms, then the logarithms."""
import os
import re
import subprocess

import numpy as np
import pytest

import retable_ref as R
import scale_ref as S
from oracle import oracle as O
from test_scale_ref_host import ARGS, mstep_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b5343414c453031
DESC = np.dtype([("T", "<i4"), ("n", "<i4"), ("store", "<i8")])
TS = [1, R.ROWS_PER_TRIP - 1, R.ROWS_PER_TRIP, R.ROWS_PER_TRIP + 1, 70, 70]
OLD_THR = np.uint64(0x1234)


def test_text():
    """fp contract off in every function, no library logarithm, no fused multiply-add, no atomics, one barrier, LDS for the staged table
    alone; the coefficients are the doubles of 1 / (2 i + 1) as hex-float literals; the library includes the header and launches both
    kernels."""
    text = open(os.path.join(CSRC, "batch_scale.hpp")).read()
    assert text.count("#include") == 1 and '#include "batch_retable.hpp"' in text
    code = re.sub(r"//[^\n]*", "", text)
    bodies = re.findall(r"\n(?:__host__ __device__ inline|__global__)[^\n]*\)\n\{\n(.*?)\n\}\n", code, re.S)
    assert len(bodies) >= 10                                   # (table_log, the seven scale_* functions, the two kernels; helpers may join them)
    for body in bodies:
        assert body.lstrip().startswith("#pragma clang fp contract(off)"), body[:80]
    assert re.search(r"[^_\w]log\s*\(", code) is None and re.search(r"[^_\w]fma\s*\(", code) is None and "atomic" not in code
    assert code.count("__syncthreads") == 1 and code.count("__shared__") == 1
    lits = [float.fromhex(h) for h in re.findall(r"0x1\.[0-9a-f]+p-\d+", code.split("table_log(double x)")[1].split("double q")[0])]
    assert lits == [1.0 / (2 * i + 1) for i in range(11, 0, -1)] == S.COEF
    hip = open(os.path.join(CSRC, "cpprob_hip.hip")).read()
    assert '#include "batch_scale.hpp"' in hip and "hipLaunchKernelGGL(batch_retable_scaled_kernel" in hip and "hipLaunchKernelGGL(batch_mstep_scaled_kernel" in hip


class Case:
    def __init__(self, k, seed, bad=()):
        rng = np.random.default_rng(seed)
        self.k, self.B, self.T, self.T_max = k, len(TS), np.array(TS), max(TS)
        self.means = np.sort(rng.uniform(-3.0, 3.0, (self.B, k)), axis=1)
        self.sigmas = rng.uniform(0.05, 3.0, (self.B, k))
        self.trans = rng.uniform(0.05, 1.0, (self.B, k, k))
        for b, what in bad:
            if what == "sigma":
                self.sigmas[b, k - 1] = 1e-170
            elif what == "zero":
                self.sigmas[b, 0] = 0.0
            elif what == "nan":
                self.sigmas[b, 1] = np.nan
            else:
                self.means[b, 0] = np.inf
        self.obs = rng.normal(0.0, 3.0, int(self.T.sum()))
        self.obs[3] = np.inf
        self.stats = rng.uniform(0.1, 2.0, (self.B, R.RECORD))
        self.stats[:, 80:] += 8.0                           # (occ_yy / occ well above the mean's square)
        self.stats[1, 64] = 0.0                             # a state without mass
        self.stats[2, 80] = 0.0                             # a variance below the floor
        self.floor = 1e-3


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_scale_host"))
    retable = open(os.path.join(CSRC, "batch_retable.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert retable.count(inc) == 1
    open(os.path.join(d, "batch_retable.hpp"), "w").write(retable.replace(inc, '#include "batch_retable_shim.hpp"'))
    open(os.path.join(d, "batch_scale.hpp"), "w").write(open(os.path.join(CSRC, "batch_scale.hpp")).read())
    so = O.build()
    exe = os.path.join(d, "batch_scale_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, "-I", os.path.join(ROOT, "cpprob_amd", "include"), os.path.join(HERE, "batch_scale_main.cpp"), "-o", exe, so,
           "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(case, grid_y, args=()):
        B, k, T_max = case.B, case.k, case.T_max
        desc = np.zeros(B, DESC)
        desc["T"], desc["n"] = case.T, 7
        first = np.concatenate([[0], np.cumsum(case.T)[:-1]]).astype("<i8")
        args = np.asarray(args, np.float64)
        head = np.array([MAGIC, B, k, T_max, grid_y, case.obs.size, args.size], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            for a in (head, desc, first, case.means, case.sigmas, case.trans, case.obs, np.full((B, T_max, 8), np.nan), np.full((B, 64), OLD_THR, np.uint64),
                      np.full((B, 8), -3.0), np.full((B, 8), -4.0), case.stats, np.array([case.floor]), args):
                f.write(np.ascontiguousarray(a).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-4000:]
        raw = open(fout, "rb").read()
        out, at = {}, 0
        for name, dt, shape in (("tab", "<f8", (B, T_max, 8)), ("thr", "<u8", (B, 64)), ("status", "<i4", (B,)), ("sigma", "<f8", (B, 8)), ("log_norm", "<f8", (B, 8)),
                                ("m_means", "<f8", (B, k)), ("m_trans", "<f8", (B, k, k)), ("m_sigmas", "<f8", (B, k)), ("m_log_norms", "<f8", (B, k)), ("logs", "<f8", (args.size,))):
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
    for b in range(case.B):
        bits = S.check(case.means[b], case.sigmas[b], case.trans[b], k)
        assert out["status"][b] == bits, b
        T = TS[b]
        lo = int(np.sum(TS[:b]))
        if bits:
            assert np.all(np.isnan(out["tab"][b])) and np.all(out["thr"][b] == OLD_THR)
            assert np.all(out["sigma"][b] == -3.0) and np.all(out["log_norm"][b] == -4.0)
            continue
        assert np.array_equal(_bits(out["tab"][b, :T]), _bits(S.rows(case.obs[lo:lo + T], case.means[b], case.sigmas[b], k))), b
        assert np.all(np.isnan(out["tab"][b, T:]))
        assert np.array_equal(out["thr"][b], R.thresholds(case.trans[b], k))
        assert np.array_equal(out["sigma"][b, :k], case.sigmas[b]) and np.all(out["sigma"][b, k:] == -3.0)
        assert np.array_equal(_bits(out["log_norm"][b, :k]), _bits([S.log_norm(s) for s in case.sigmas[b]])) and np.all(out["log_norm"][b, k:] == -4.0)
    for b in range(case.B):
        if not np.all(np.isfinite(case.sigmas[b])):
            continue                                          # (sigmas the M-step keeps are compared as bits below only where they are numbers)
        m, sg, ln, tr = S.m_step(case.stats[b], case.means[b], case.sigmas[b], np.full(k, -7.0), case.trans[b], k, case.floor)
        assert np.array_equal(_bits(out["m_means"][b]), _bits(m)) and np.array_equal(_bits(out["m_trans"][b]), _bits(tr)), b
        assert np.array_equal(_bits(out["m_sigmas"][b]), _bits(sg)) and np.array_equal(_bits(out["m_log_norms"][b]), _bits(ln)), b


@pytest.mark.parametrize("k", [2, 5, 8])
@pytest.mark.parametrize("grid_y", [1, 2, 3])
def test_kernels_against_the_reference(prog, k, grid_y):
    case = Case(k, 100 + k, bad=((1, "sigma"), (3, "mean")) if grid_y == 2 else ((2, "zero"), (4, "nan")) if grid_y == 3 else ())
    out = prog(case, grid_y, ARGS[::40] if grid_y == 1 else ())
    _check(case, out)
    assert case.stats[2, 80] == 0.0 and out["m_sigmas"][2, 0] == case.floor and out["m_sigmas"][1, 0] == case.sigmas[1, 0]
    if grid_y == 1:
        assert np.array_equal(_bits(out["logs"]), _bits([S.table_log(x) for x in ARGS[::40]]))


def test_mstep_edge_cases(prog):
    """The constructed records of tests/test_scale_ref_host.py through the kernel's text."""
    for name, rec, means, sigmas, trans, floor in mstep_cases():
        case = Case(2, 7)
        case.means[:], case.sigmas[:], case.trans[:], case.stats[:], case.floor = means, sigmas, trans, rec, floor
        out = prog(case, 1)
        m, sg, ln, tr = S.m_step(rec, means, sigmas, np.full(2, -7.0), trans, 2, floor)
        for b in range(case.B):
            assert np.array_equal(_bits(out["m_means"][b]), _bits(m)) and np.array_equal(_bits(out["m_trans"][b]), _bits(tr)), name
            assert np.array_equal(_bits(out["m_sigmas"][b]), _bits(sg)) and np.array_equal(_bits(out["m_log_norms"][b]), _bits(ln)), name
