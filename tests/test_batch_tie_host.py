"""The host pieces of tied tables (include/cpprob_hip.h: cpprob_hip_batch_tie, _tie_get, _pool_stats, _pool_stats_device): the symbols
are declared, listed and bound; what the library refuses without a context; the entry points' text -- the device form waits for
nothing, a begin forgets the tie, a re-table keeps it, no workspace region is added --; the drivers refuse unequal starts before they
touch the engine; cpprob_main refuses the flags without a fit; cpprob::gpu::Options::tie_groups compiles as pedantic C++14."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cpprob_amd
import cpprob_amd.capi as cp

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cpprob_hip_batch_tie": 3, "cpprob_hip_batch_tie_get": 3, "cpprob_hip_batch_pool_stats": 7, "cpprob_hip_batch_pool_stats_device": 7}


def _hip():
    return open(os.path.join(ROOT, "cpprob_amd", "csrc", "cpprob_hip.hip")).read()


def _fn(hip, head):
    return re.search(r"^%s\(.*?^\}" % head, hip, re.M | re.S).group(0)


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS and hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n_args, s
    assert "int cpprob_hip_batch_tie(cpprob_hip_ctx* ctx, const int32_t* h_group, size_t n);" in header
    assert "int cpprob_hip_batch_tie_get(cpprob_hip_ctx* ctx, int32_t* h_group, int32_t* n_groups);" in header
    assert re.search(r"int cpprob_hip_batch_pool_stats_device\(cpprob_hip_ctx\* ctx, const double\* d_records, size_t n_doubles, uint32_t per_problem, int broadcast,\s+double\* d_out, size_t n_out\);", header)
    assert re.search(r"int cpprob_hip_batch_pool_stats\(cpprob_hip_ctx\* ctx, const double\* h_records, size_t n_doubles, uint32_t per_problem, int broadcast,\s+double\* h_out, size_t n_out\);", header)
    assert L.cpprob_hip_abi_version() == 3 and "#define CPPROB_HIP_ABI_VERSION 3" in header
    for name in ("batch_tie", "batch_tie_get", "batch_pool_stats", "batch_pool_stats_device"):
        assert callable(getattr(cp.Engine, name)), name
    assert cpprob_amd.pool_stats is cpprob_amd.em.pool_stats


def test_refusals_without_a_context():
    L = cp.load_library()
    x = np.full(88, 5.0)
    g = np.zeros(1, np.int32)
    n = C.c_int32(7)
    assert L.cpprob_hip_batch_tie(None, g.ctypes.data_as(C.POINTER(C.c_int32)), 1) == EINVAL
    assert b"ctx is NULL" in L.cpprob_hip_last_error(None)
    assert L.cpprob_hip_batch_tie_get(None, g.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)) == EINVAL and n.value == 7
    assert L.cpprob_hip_batch_pool_stats(None, x.ctypes.data, 88, 1, 1, x.ctypes.data, 88) == EINVAL
    assert L.cpprob_hip_batch_pool_stats_device(None, x.ctypes.data, 88, 1, 1, x.ctypes.data, 88) == EINVAL
    assert np.all(x == 5.0)


def test_the_entry_points_text():
    hip = _hip()
    # the device form is enqueued: it waits for nothing, and nothing is enqueued before the check has passed
    dev = _fn(hip, "int cpprob_hip_batch_pool_stats_device")
    assert "hipStreamSynchronize" not in dev and "hipDeviceSynchronize" not in dev and "hipMalloc" not in dev and ".grow(" not in dev
    assert dev.index("batch_pool_check(") < dev.index("batch_pool_enqueue(")
    enq = _fn(hip, "static int batch_pool_enqueue")
    assert "hipStreamSynchronize" not in enq and "hipMalloc" not in enq and ".grow(" not in enq and "hipLaunchKernelGGL(batch_pool_stats_kernel" in enq and "c->stream" in enq
    host = _fn(hip, "int cpprob_hip_batch_pool_stats")
    assert host.index("batch_pool_check(") < host.index("batch_stage(") < host.index("hipMemcpyAsync") < host.index("batch_pool_enqueue(") < host.index("batch_fetch(")
    check = _fn(hip, "static int batch_pool_check")
    for code, words in (("CPPROB_HIP_ESTATE", "no batch is begun"), ("CPPROB_HIP_ESTATE", "the begun batch has no tie"), ("CPPROB_HIP_EINVAL", "per_problem must be >= 1"),
                        ("CPPROB_HIP_EINVAL", "the records are too small"), ("CPPROB_HIP_EINVAL", "the output is too small"), ("CPPROB_HIP_EINVAL", "is beyond one launch's grid"),
                        ("CPPROB_HIP_EINVAL", "the output overlaps the records"), ("CPPROB_HIP_EINVAL", "the compact form does not pool in place")):
        assert re.search(r"fail\(c, %s, \"[^\n]*%s" % (code, re.escape(words)), check), words
    assert "hipMemcpy" not in check and "hipLaunch" not in check
    # the tie: validated before anything changes; any begin forgets it; a re-table does not name it
    tie = _fn(hip, "int cpprob_hip_batch_tie")
    assert tie.rindex("return fail(") < tie.index("hipStreamSynchronize") < tie.index("bs->tied = false;") < tie.index("bs->d_tie.grow(c->stream, ") < tie.index("hipMemcpyAsync") \
        < tie.index("bs->tied = true;")
    assert tie.count(".grow(") == 1 and "hipMalloc" not in tie
    for code, words in (("CPPROB_HIP_ESTATE", "no batch is begun"), ("CPPROB_HIP_EINVAL", "the begun batch has"), ("CPPROB_HIP_EINVAL", "negative group id"), ("CPPROB_HIP_EINVAL", "is unused")):
        assert re.search(r"fail\(c, %s, \"[^\n]*%s" % (code, re.escape(words)), tie), words
    get = _fn(hip, "int cpprob_hip_batch_tie_get")
    assert "hip" not in get.replace("cpprob_hip", "").replace("CPPROB_HIP", "")          # host only
    begin = _fn(hip, "int batch_begin")
    assert "bs->tied = false; bs->tie_groups = 0; bs->tie_map.clear();" in begin
    assert begin.index("bs->tied = false;") < begin.index(".grow(") and begin.index("bs->tied = false;") < begin.index(".reserve(") and "hipMalloc" not in begin
    for name in ("static int batch_retable_enqueue", "int cpprob_hip_batch_retable", "int cpprob_hip_batch_retable_device", "int cpprob_hip_batch_retable_scaled",
                 "int cpprob_hip_batch_retable_scaled_device", "static int batch_retable_check", "static int batch_retable_device", "static int batch_retable_host",
                 "static int batch_retable_observes"):
        assert re.search(r"\btied\b|tie_", _fn(hip, name)) is None, name
    # arrays of the context's own: no workspace region is added
    layout = re.search(r"^struct BatchLayout \{[^\n]*\};", hip, re.M).group(0)
    assert layout == "struct BatchLayout { size_t tab, seeds, thr, ctrl, stats, ess, res, nreq, prob, order, values, anc, first, snap, carry, mass, total; };"
    # ... one the state owns: declared an owning buffer in BatchState, freed when batch_free deletes the state
    state = re.search(r"^struct BatchState \{.*?^\};", hip, re.M | re.S).group(0)
    assert re.search(r"^    DeviceBuffer d_tie;$", state, re.M) and "int32_t* d_tie" not in state
    free = _fn(hip, "void batch_free")
    assert "delete c->batch;" in free and "dfree(" not in free and "hipFree" not in free


def test_drivers_take_groups_and_default_to_the_untied_loops():
    assert inspect.signature(cpprob_amd.em.hmm_table_em).parameters["groups"].default is None
    assert inspect.signature(cpprob_amd.gibbs.hmm_table_gibbs).parameters["groups"].default is None
    assert 'prior.pop("groups", None)' in inspect.getsource(cpprob_amd.pgibbs.hmm_table_particle_gibbs)
    res = inspect.getsource(cpprob_amd.em._em_resident)
    assert res.count("engine.batch_tie(") == 1 and res.index("engine.batch_tie(") < res.index("for it in range(iterations)")
    assert res.index("batch_smooth_stats_device(stats, obs)") < res.index("batch_pool_stats_device(stats, stats)") < res.index("engine.batch_mstep_device(")


class _Untouched:
    """An engine that must not be reached."""

    def __getattr__(self, name):
        raise AssertionError("the engine was touched: " + name)


@pytest.mark.parametrize("field", ["means", "trans", "sigmas"])
def test_drivers_refuse_unequal_starts_before_touching_the_engine(field):
    means = np.tile(np.array([-0.5, 0.5]), (4, 1))
    trans = np.tile(np.array([[0.5, 0.5], [0.5, 0.5]]), (4, 1, 1))
    sigmas = np.ones((4, 2))
    groups = np.array([0, 1, 0, 1])
    {"means": means, "trans": trans, "sigmas": sigmas}[field][3].flat[1] = np.nextafter(0.5 if field != "sigmas" else 1.0, 2.0)      # (one ulp: bit for bit)
    obs = [np.zeros(3)] * 4
    seeds = np.arange(4, dtype=np.uint64)
    s0 = sigmas if field == "sigmas" else None
    eng = _Untouched()
    with pytest.raises(ValueError, match="group 1"):
        cpprob_amd.hmm_table_em(eng, obs, means, trans, 8, seeds, 2, sigmas0=s0, groups=groups)
    with pytest.raises(ValueError, match="group 1"):
        cpprob_amd.hmm_table_em(eng, obs, means, trans, 8, seeds, 2, sigmas0=s0, groups=groups, resident=True)
    with pytest.raises(ValueError, match="group 1"):
        cpprob_amd.hmm_table_gibbs(eng, obs, means, trans, 8, seeds, 2, np.random.default_rng(0), sigmas0=s0, groups=groups)
    with pytest.raises(ValueError, match="group 1"):
        cpprob_amd.hmm_table_particle_gibbs(eng, obs, means, trans, 8, seeds, 2, np.random.default_rng(0), sigmas0=s0, groups=groups)
    # what is no partition is refused too
    with pytest.raises(ValueError):
        cpprob_amd.hmm_table_em(eng, obs, means, trans, 8, seeds, 2, groups=[0, 2, 0, 2])


def test_the_equal_start_check_takes_equal_tables():
    means = np.tile(np.array([-0.5, 0.5]), (4, 1))
    means[1] = means[3] = [-1.0, 2.0]
    trans = np.full((4, 2, 2), 0.5)
    g, G, lead = cpprob_amd.em.check_tied_start([0, 1, 0, 1], means, trans)
    assert g.dtype == np.int32 and list(g) == [0, 1, 0, 1] and G == 2 and list(lead) == [0, 1]


_OPTIONS_TU = r"""
#include <cstdint>
#include <vector>
#include "cpprob/cpprob.hpp"

int main()
{
    if (!cpprob::gpu::options().tie_groups.empty()) return 3;   // off by default
    cpprob::gpu::options().tie_groups = std::vector<std::int32_t>{0, 0};
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        const cpprob::gpu::HmmTableFit fit = cpprob::gpu::hmm_table_fit(tables, {{0.5, 0.25}}, {512}, seeds, 2);
        return fit.tables.size() == 2 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_tie_groups_option_compiles_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    src = tmp_path / "tie.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "tie.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]
    fit = re.search(r"^inline HmmTableFit hmm_table_fit\(.*?^\}", open(os.path.join(ROOT, "cpprob_amd", "include", "cpprob", "detail", "host_engine.hpp")).read(), re.M | re.S).group(0)
    assert "options().tie_groups" in fit and "cpprob_hip_batch_tie(" in fit and "1, 1, pooled.data(), pooled.size())" in fit
    assert fit.index("cpprob_hip_batch_smooth_stats(") < fit.index("cpprob_hip_batch_pool_stats(") < fit.index("double row = 0.0;")


@pytest.mark.parametrize("flag", [["--tie_tables"], ["--tie_groups", "[0]"]])
def test_cli_flags_need_the_iterations(tmp_path, flag):
    main = os.path.join(ROOT, "cpprob_amd", "bin", "cpprob_main")
    (tmp_path / "tables.txt").write_text("[-1 1] [0.9 0.1 0.2 0.8] [0.5 0.25 -0.5]\n")
    p = subprocess.run([main, "--smc", "--model_folder", str(tmp_path), "--batch_tables_file", "tables.txt", "-n", "8"] + flag, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--tie_tables" in p.stderr and "--tie_groups" in p.stderr and "--em_iterations" in p.stderr
