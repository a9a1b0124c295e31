"""CPU tests of the masses a filtering-only batch keeps (include/cpprob_hip.h: CPPROB_HIP_BATCH_KEEP_MASSES).

1. batch_check through the three workspace-size exports (pure host functions): the bit is admitted with keep_history = 0, refused with
   keep_history = 1, every other bit stays refused, and the bit adds exactly one region of batch_round(B * T_max * 64) bytes.
2. batch_mass_row (csrc/batch_smc.hpp), the one statement of a row of the m table the batch kernel writes: its text is cut out of the
   header, built against tests/host_kernels/batch_smooth_shim.hpp as a stand-alone program (tests/host_kernels/batch_mass_row_main.cpp)
   with g++ -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off and run directly.  Its rows must equal
   tests/backward_ref.py's filtering_masses -- what batch_smooth_count_kernel derives from a particle store -- exactly.  Nothing is
   loaded into python and nothing runs on a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd.capi as cp
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
EINVAL = -1
MAGIC = 0x4b4d415353524f57
GAP_LIMIT = 6.0                                # kFixGapLimit


def _round(x):
    return (x + 255) // 256 * 256


# ---- 1. the opt-in -----------------------------------------------------------------------------------------------------------------
def _uniform(**kw):
    return cp.batch_workspace_bytes(kw.pop("model", cp.MODEL_HMM_TABLE), 300, 5, 17, **kw)


def _described(**kw):
    return cp.batch_problems_workspace_bytes(kw.pop("model", cp.MODEL_HMM_TABLE), [1, 2, 7, 16], [1, 5, 300, 1500], **kw)


def _online(**kw):
    return cp.batch_online_workspace_bytes(kw.pop("model", cp.MODEL_HMM_TABLE), [4, 40, 9], [8192, 3, 100], **kw)


KINDS = [(_uniform, 5, 17), (_described, 4, 16), (_online, 3, 40)]          # (the export, B, T_max)


def _code(fn, **kw):
    with pytest.raises(cp.CpprobHipError) as e:
        fn(**kw)
    return e.value.code, str(e.value)


@pytest.mark.parametrize("fn,B,T_max", KINDS)
def test_the_bit_is_admitted_for_filtering_only_batches_alone(fn, B, T_max):
    assert cp.BATCH_KEEP_MASSES == 2
    assert fn(keep_history=False, flags=2) > 0
    assert fn(keep_history=False, keep_masses=True) == fn(keep_history=False, flags=2)
    code, msg = _code(fn, keep_history=True, flags=2)
    assert code == EINVAL and "filtering-only" in msg
    assert _code(fn, keep_history=True, keep_masses=True)[0] == EINVAL
    for keep in (False, True):
        for flags in (1, 3, 4, 6, 1 << 31):
            assert _code(fn, keep_history=keep, flags=flags)[0] == EINVAL, (keep, flags)


@pytest.mark.parametrize("fn,B,T_max", KINDS)
@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
@pytest.mark.parametrize("rs", [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED])
def test_the_bit_adds_one_region_of_64_bytes_a_problem_and_step(fn, B, T_max, model, rs):
    plain = fn(model=model, resampler=rs, keep_history=False)
    assert fn(model=model, resampler=rs, keep_history=False, keep_masses=True) == plain + _round(B * T_max * 64)
    assert fn(model=model, resampler=rs, keep_history=False, flags=0) == plain


def test_region_sizes_that_are_no_multiple_of_256():
    for B, T in ((1, 1), (3, 1), (1, 5), (7, 9)):
        plain = cp.batch_workspace_bytes(cp.MODEL_HMM3, 64, B, T, keep_history=False)
        assert cp.batch_workspace_bytes(cp.MODEL_HMM3, 64, B, T, keep_history=False, keep_masses=True) == plain + _round(B * T * 64)


# ---- 2. batch_mass_row as a host program -------------------------------------------------------------------------------------------
def _function_text():
    """The definitions of batch_mass and batch_mass_row in csrc/batch_smc.hpp, each found exactly once, inside namespace cph."""
    src = open(os.path.join(ROOT, "cpprob_amd", "csrc", "batch_smc.hpp")).read()
    defs = re.findall(r"^__host__ __device__ inline [^\n]*\bbatch_mass(?:_row)?\([^\n]*\)\n\{\n.*?^\}\n", src, re.M | re.S)
    assert len(defs) == 2 and "batch_mass(" in defs[0] and "batch_mass_row(" in defs[1], defs
    return "#pragma once\nnamespace cph {\n" + "".join(defs) + "}  // namespace cph\n"


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_mass_row_host"))
    open(os.path.join(d, "batch_mass_row_host.hpp"), "w").write(_function_text())
    so = O.build()
    exe = os.path.join(d, "batch_mass_row_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, os.path.join(HERE, "batch_mass_row_main.cpp"), "-o", exe, so, "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(cnt, ll):
        """cnt [rows, 8] counts, ll [rows, k] log-weights -> the rows [rows, 8]."""
        cnt, ll = np.ascontiguousarray(cnt, np.uint32), np.ascontiguousarray(ll, np.float64)
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([MAGIC, cnt.shape[0], ll.shape[1]], "<i8").tobytes())
            f.write(cnt.tobytes())
            f.write(ll.tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        raw = open(fout, "rb").read()
        assert len(raw) == 8 * 8 * cnt.shape[0]
        return np.frombuffer(raw, np.float64).reshape(-1, 8)
    return run


def _reference(cnt, ll):
    """filtering_masses of a store whose generation t holds cnt[t][s] particles in state s; states >= k zero."""
    k = ll.shape[1]
    values = [np.repeat(np.arange(k), c[:k]) for c in cnt]
    out = np.zeros((len(cnt), 8))
    out[:, :k] = np.array(R.filtering_masses(values, ll.tolist()), np.float64)
    return out


def _cases(k, seed):
    """Random rows and the constructed ones, as (counts [rows, 8], log-weights [rows, k], the rows' kinds)."""
    rng = np.random.default_rng(seed)
    cnt, ll, kind = [], [], []

    def add(c, l, what):
        row = np.zeros(8, np.int64)
        row[:k] = c
        assert row.sum() >= 1
        cnt.append(row), ll.append(np.asarray(l, np.float64)), kind.append(what)

    for _ in range(40):                                                     # populations of 1 .. 8192, every state possibly empty
        n = int(rng.choice([1, 2, 3, 64, 257, 1027, 8192]))
        add(rng.multinomial(n, rng.dirichlet(np.full(k, 0.4))), -rng.uniform(0.0, 5.0, k), "near")
    for _ in range(20):                                                     # differences far past kFixGapLimit: weights that quantise to 0
        add(rng.multinomial(300, np.full(k, 1.0 / k)), -rng.uniform(0.0, 60.0, k), "far")
    for s in range(k):                                                      # only state s occupied, and not the likeliest one
        l = -rng.uniform(1.0, 5.0, k)
        l[(s + 1) % k] = -0.25
        add(np.eye(k, dtype=np.int64)[s] * (1 + 37 * s), l, "single")
    for s in range(k):                                                      # the largest ll belongs to the empty state s: inside the gap limit, and past it
        for gap in (0.5, 5.9, 6.1, 40.0):
            l = -rng.uniform(gap, gap + 3.0, k)
            l[s] = 0.0
            c = rng.integers(1, 500, k)
            c[s] = 0
            add(c, l, "empty-top")
    add(np.full(k, 8192 // k), np.zeros(k), "ties")                         # every weight 2^32 - 1
    add(np.full(k, 1), np.full(k, -745.0), "tiny")                          # log-weights at the edge of the doubles' exp
    return np.array(cnt), np.array(ll), kind


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_rows_equal_the_references_filtering_masses(prog, k):
    cnt, ll, kind = _cases(k, 100 + k)
    got = prog(cnt, ll)
    want = _reference(cnt, ll)
    assert np.array_equal(got, want), [(i, kind[i]) for i in np.nonzero((got != want).any(axis=1))[0]]
    assert np.all(got[:, k:] == 0.0)
    # the constructed rows are what they claim to be
    occupied = cnt[:, :k] > 0
    M = np.where(occupied, ll, -np.inf).max(axis=1)
    kinds = np.array(kind)
    assert np.all(occupied[kinds == "single"].sum(axis=1) == 1)
    top = kinds == "empty-top"
    assert np.all(ll[top].max(axis=1) > M[top])                             # the step's bound sits above the exact maximum
    assert np.any(ll[top].max(axis=1) - M[top] < GAP_LIMIT) and np.any(ll[top].max(axis=1) - M[top] > GAP_LIMIT)
    far = kinds == "far"
    assert np.any((got[far][:, :k] == 0.0) & occupied[far]), "no occupied state's weight quantised to 0"
    # against the bound instead of M the rows differ: q[s] of the step is the wrong number
    bound_rows = np.array([[int(c) * int(q) for c, q in zip(cnt[i, :k], O.fix_weights(ll[i], float(ll[i].max())))] for i in np.nonzero(top)[0]], np.float64)
    assert np.any(bound_rows != got[top][:, :k])
    # the heaviest occupied state carries the full 32 bits
    assert np.all(got[np.arange(len(cnt)), np.where(occupied, ll, -np.inf).argmax(axis=1)] >= (2.0 ** 32 - 1))
