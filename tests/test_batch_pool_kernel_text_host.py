"""batch_pool_stats_kernel (csrc/batch_pool.hpp) as host code: the header's own text, its include line naming
tests/host_kernels/batch_retable_shim.hpp, built as a stand-alone program with g++ -O1 -fsanitize=address,undefined
-fno-sanitize-recover=undefined -ffp-contract=off (tests/host_kernels/batch_pool_main.cpp) and run on the grid the host code launches.
Every buffer has exactly the size the host code hands the kernel and the output is NaN on the way in, so an entry nobody wrote, or one
an idle wavefront of the last workgroup wrote, shows.  The compact, the broadcast and the in-place forms must equal tests/pool_ref.py's
bit for bit.  Nothing is loaded into python and nothing runs on a GPU.

The case file: a header of 6 int64 {magic, B, G, R, broadcast, in place}, the members sorted by (group, problem) [B] int32, the groups'
first positions [G + 1] int32, the records [B][R][88].  The output: the pooled records, [G][R][88] or [B][R][88]."""
import os
import re
import subprocess

import numpy as np
import pytest

import pool_ref as P
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_kernels")
CSRC = os.path.join(ROOT, "cpprob_amd", "csrc")
MAGIC = 0x4b504f4f4c303031


def _text():
    text = open(os.path.join(CSRC, "batch_pool.hpp")).read()
    inc = '#include "batch_smc.hpp"'
    assert text.count(inc) == 1 and text.count("#include") == 1
    return text, text.replace(inc, '#include "batch_retable_shim.hpp"')


def test_text():
    """One include, fp contract off in every body that touches a double, no atomics, no barrier, no LDS, the look-ahead a named
    constant; the library includes the header and launches the kernel."""
    text, _ = _text()
    code = re.sub(r"//[^\n]*", "", text)
    bodies = re.findall(r"\n(?:__device__ __forceinline__|__host__ __device__ inline|__global__)[^\n]*\)\n\{\n(.*?)\n\}\n", code, re.S)
    assert len(bodies) == 2
    with_double = [b for b in bodies if "double" in b]
    assert len(with_double) == 1
    for body in with_double:
        assert body.lstrip().startswith("#pragma clang fp contract(off)"), body[:80]
    assert "atomic" not in code and "__syncthreads" not in code and "__shared__" not in code and "__shfl" not in code
    assert re.search(r"[^_\w]fma\s*\(", code) is None
    assert re.search(r"^constexpr int kPoolAhead = \d+;", code, re.M) and 1 <= P.pool_ahead() <= 7        # (B = 40 holds the case's six groups)
    assert "constexpr int kPoolStats = 88;" in code
    hip = open(os.path.join(CSRC, "cpprob_hip.hip")).read()
    assert '#include "batch_pool.hpp"' in hip and "hipLaunchKernelGGL(batch_pool_stats_kernel" in hip
    # the other fitting headers keep their functions: the kernel lives in a header of its own
    assert "pool" not in open(os.path.join(CSRC, "batch_retable.hpp")).read() and "pool" not in open(os.path.join(CSRC, "batch_scale.hpp")).read()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("batch_pool_host"))
    open(os.path.join(d, "batch_pool_host.hpp"), "w").write(_text()[1])
    so = O.build()
    exe = os.path.join(d, "batch_pool_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-pthread",
           "-I", d, "-I", HERE, "-I", os.path.join(ROOT, "cpprob_amd", "include"), os.path.join(HERE, "batch_pool_main.cpp"), "-o", exe, so,
           "-Wl,-rpath," + os.path.dirname(so)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]

    def run(groups, rec, broadcast, in_place=False):
        B, R = rec.shape[0], rec.shape[1]
        mem = P.members(groups)
        G = len(mem)
        first = np.concatenate([[0], np.cumsum([len(m) for m in mem])]).astype("<i4")
        head = np.array([MAGIC, B, G, R, int(broadcast), int(in_place)], "<i8")
        fin, fout = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            f.write(np.concatenate(mem).astype("<i4").tobytes())
            f.write(first.tobytes())
            f.write(np.ascontiguousarray(rec, np.float64).tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "" and p.stdout == "", "exit %d\n%s" % (p.returncode, p.stderr[-4000:])      # (the sanitizers are silent)
        return np.fromfile(fout, np.float64).reshape((B if broadcast else G), R, P.RECORD)
    return run


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("R", [1, 3])
def test_every_form_gives_the_references_bits(prog, R):
    """Groups of 1, A - 1, A, A + 1, 2 A + 3 members and the rest (A = kPoolAhead), interleaved; G R = 6 or 18 pairs on 2 or 5
    workgroups of four wavefronts: the last one has idle wavefronts."""
    groups, rec = P.case(R, 50 + R)
    G = int(groups.max()) + 1
    assert (G * R) % 4 != 0
    compact_w, full_w = P.pool(rec, groups, broadcast=False), P.pool(rec, groups)
    assert not np.isnan(full_w).any() and not _same(compact_w, P.pool(rec, groups, broadcast=False, descending=True))
    assert _same(prog(groups, rec, False), compact_w), "compact"
    assert _same(prog(groups, rec, True), full_w), "broadcast"
    assert _same(prog(groups, rec, True, in_place=True), full_w), "in place"


def test_one_group_of_all_and_groups_of_one(prog):
    _, rec = P.case(2, 77)
    all_one = np.zeros(40, np.int32)
    assert _same(prog(all_one, rec, True, in_place=True), P.pool(rec, all_one)) and _same(prog(all_one, rec, False), P.pool(rec, all_one, broadcast=False))
    each = np.arange(40, dtype=np.int32)[::-1].copy()
    assert _same(prog(each, rec, False), rec[::-1]) and _same(prog(each, rec, True), rec)
