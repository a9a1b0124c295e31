"""The host pieces of re-tabling (include/cpprob_hip.h: cpprob_hip_batch_retable* and their companions): the symbols are declared,
listed and bound; what the library refuses without a context and what the wrappers refuse before they call it; the refusals a begun
batch earns are worded in the library (they are exercised on a device in tests/test_gpu_batch_retable.py); the host state a re-table
resets; the workspace sizes, which the feature leaves where they were; and the drivers' keywords."""
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
NEW = {"cpprob_hip_batch_retable": 5, "cpprob_hip_batch_retable_device": 5, "cpprob_hip_batch_retable_status": 2, "cpprob_hip_batch_retable_grid": 2,
       "cpprob_hip_batch_mstep_device": 5, "cpprob_hip_batch_copy_step_tables": 5, "cpprob_hip_batch_summaries_device": 2}


def _hip():
    return open(os.path.join(ROOT, "cpprob_amd", "csrc", "cpprob_hip.hip")).read()


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n_args, s
    assert re.search(r"int cpprob_hip_batch_retable_device\(cpprob_hip_ctx\* ctx, const double\* d_means, const double\* d_transition, const double\* d_observes, size_t n_observes\);", header)
    assert re.search(r"int cpprob_hip_batch_retable\(cpprob_hip_ctx\* ctx, const double\* h_means, const double\* h_transition, const double\* h_observes, size_t n_observes\);", header)
    assert re.search(r"int cpprob_hip_batch_copy_step_tables\(cpprob_hip_ctx\* ctx, uint64_t problem, double\* h_rows, size_t n_doubles, uint64_t\* h_thr\);", header)
    assert "h_observes may be NULL" in header and "waits for the stream once" in header
    assert L.cpprob_hip_abi_version() == 3
    for name in ("batch_retable", "batch_retable_device", "batch_retable_status", "batch_mstep_device", "batch_step_tables", "batch_summaries_device", "batch_retable_grid"):
        assert callable(getattr(cp.Engine, name)), name


def test_refusals_without_a_context():
    L = cp.load_library()
    x = np.zeros(8)
    w = np.zeros(64, np.uint64)
    st = np.zeros(2, np.int32)
    g = C.c_uint32(7)
    assert L.cpprob_hip_batch_retable(None, x.ctypes.data, x.ctypes.data, x.ctypes.data, 2) == EINVAL
    assert b"ctx is NULL" in L.cpprob_hip_last_error(None)
    assert L.cpprob_hip_batch_retable_device(None, x.ctypes.data, x.ctypes.data, x.ctypes.data, 2) == EINVAL
    assert L.cpprob_hip_batch_retable_status(None, st.ctypes.data_as(C.POINTER(C.c_int32))) == EINVAL
    assert L.cpprob_hip_batch_retable_grid(None, C.byref(g)) == EINVAL and g.value == 7
    assert L.cpprob_hip_batch_mstep_device(None, x.ctypes.data, 88, x.ctypes.data, x.ctypes.data) == EINVAL
    assert L.cpprob_hip_batch_copy_step_tables(None, 0, x.ctypes.data, 8, w.ctypes.data) == EINVAL
    assert L.cpprob_hip_batch_summaries_device(None, x.ctypes.data) == EINVAL


def _engine(T):
    """An Engine without a context: the wrappers' checks run before the library is called."""
    eng = cp.Engine.__new__(cp.Engine)
    eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K = len(T), max(T), 4, 8
    eng.batch_shapes = (np.array(T, np.uint32), np.full(len(T), 4, np.uint32))
    return eng


def test_wrappers_check_their_arguments():
    eng = _engine([3, 1, 2])
    good = (np.zeros((3, 2)), np.zeros((3, 2, 2)))
    for tables in ((np.zeros((2, 2)), np.zeros((2, 2, 2))),            # a table short
                   (np.zeros((3, 2)), np.zeros((3, 2, 3))),            # rows of another k
                   (np.zeros(6), np.zeros((3, 2, 2)))):                # means without their axis
        with pytest.raises(ValueError):
            eng.batch_retable(tables)
    assert good[0].shape == (3, 2)
    with pytest.raises(ValueError):
        eng.batch_summaries_device(None)


def test_the_library_words_every_refusal_and_resets_the_state_of_a_begin():
    hip = _hip()
    check = re.search(r"^static int batch_retable_check\(.*?^\}", hip, re.M | re.S).group(0)
    for code, words in (("CPPROB_HIP_ESTATE", "no batch is begun"),
                        ("CPPROB_HIP_EUNSUPPORTED", "an online batch is not re-tabled"),
                        ("CPPROB_HIP_EUNSUPPORTED", "the table of CPPROB_HIP_MODEL_HMM3 is the model's"),
                        ("CPPROB_HIP_EUNSUPPORTED", "a batch begun by cpprob_hip_batch_begin shares one table"),
                        ("CPPROB_HIP_EINVAL", "the problems' lengths sum to")):
        assert re.search(r"fail\(c, %s, \"[^\n]*%s" % (code, re.escape(words)), check), words
    # the unit and the scaled entry points are one shared body each: the device forms', the host forms'
    for name, call in (("cpprob_hip_batch_retable_device", "batch_retable_device(c, d_means, d_transition, nullptr, d_observes, n_observes, false)"),
                       ("cpprob_hip_batch_retable_scaled_device", "batch_retable_device(c, d_means, d_transition, d_sigmas, d_observes, n_observes, true)"),
                       ("cpprob_hip_batch_retable", "batch_retable_host(c, h_means, h_transition, nullptr, h_observes, n_observes, false)"),
                       ("cpprob_hip_batch_retable_scaled", "batch_retable_host(c, h_means, h_transition, h_sigmas, h_observes, n_observes, true)")):
        entry = re.search(r"^int %s\([^;{}]*\)\n\{\n(.*?)^\}" % name, hip, re.M | re.S).group(1)
        assert [line.strip() for line in entry.splitlines()] == ["LANES_OWN(c);", "return %s;" % call], name
    # nothing is enqueued before the check has passed, in either form; the host form validates with the begin's own statements
    observes = re.search(r"^static int batch_retable_observes\(.*?^\}", hip, re.M | re.S).group(0)
    for name in ("batch_retable_device", "batch_retable_host"):
        body = re.search(r"^static int %s\(.*?^\}" % name, hip, re.M | re.S).group(0)
        assert body.index("batch_retable_check(") < body.index("batch_retable_enqueue(")
        # no wait of its own; one growth -- the observes' buffer -- in the host form, none in the device form (a growth waits for the
        # stream: csrc/batch_buffers.hpp, tests/test_batch_buffers_host.py)
        assert "hipStreamSynchronize" not in body and "hipStreamSynchronize" not in observes and "hipMalloc" not in body + observes
        grows = body.count(".grow(") + (observes.count(".grow(") if name == "batch_retable_host" else 0)
        assert grows == (1 if name == "batch_retable_host" else 0)
        assert ("batch_retable_observes(" in body) == (name == "batch_retable_host")
    host = re.search(r"^static int batch_retable_host\(.*?^\}", hip, re.M | re.S).group(0)
    assert "hipMemcpyAsync" in observes and host.count("batch_retable_observes(") == 1 and "bs->d_robs.grow(c->stream, " in observes
    assert host.index("batch_check_tables(") < host.index("batch_check_scales(") < host.index("batch_retable_observes(") < host.index("hipMemcpyAsync")
    assert "batch_stage(" in host and "bs->thr_stale = false;" in host
    enq = re.search(r"^static int batch_retable_enqueue\(.*?^\}", hip, re.M | re.S).group(0)
    for line in ("bs->ran = false; bs->conditional = false;", "bs->lp_ready = false; bs->lp_sent = false;", "bs->tab_stale = true; bs->thr_stale = true;"):
        assert line in enq, line
    assert "cfirst_ready = false" not in enq and "hipStreamSynchronize" not in enq and "hipMalloc" not in enq
    assert enq.count(".grow(") == 1 and "bs->d_rstatus.grow(c->stream, " in enq                              # (the status words' growth alone)
    # the two host paths that read the mirrors fetch from the device when they are stale; nothing else names the mirrors
    store = re.search(r"^int cpprob_hip_batch_copy_store\(.*?^\}", hip, re.M | re.S).group(0)
    assert "bs->tab_stale ? fetched" in store
    table = re.search(r"^static int batch_decode_table\(.*?^\}", hip, re.M | re.S).group(0)
    assert "if (bs->thr_stale)" in table and "bs->lay.thr" in table
    # a begin forgets all of it
    begin = re.search(r"^int batch_begin\(.*?^\}", hip, re.M | re.S).group(0)
    assert "bs->retabled = false; bs->robs_ready = false; bs->tab_stale = false; bs->thr_stale = false; bs->retable_gy = 0;" in begin


def test_workspace_sizes_are_where_they_were():
    """No workspace region is added: the three size functions return what they returned before re-tabling existed."""
    want = {(True, False): (142592, 432128, 189696), (False, False): (14848, 64768, 29184), (False, True): (20480, 91648, 36864)}
    for (kh, km), (uni, prob, online) in want.items():
        assert cp.batch_workspace_bytes(cp.MODEL_HMM_TABLE, 300, 5, 17, keep_history=kh, keep_masses=km) == uni
        assert cp.batch_problems_workspace_bytes(cp.MODEL_HMM_TABLE, [1, 31, 32, 33, 70, 70], [1, 64, 1500, 64, 5, 300], keep_history=kh, keep_masses=km) == prob
        assert cp.batch_online_workspace_bytes(cp.MODEL_HMM_TABLE, [4, 40, 9], [8192, 3, 100], keep_history=kh, keep_masses=km) == online
    layout = re.search(r"^struct BatchLayout \{[^\n]*\};", _hip(), re.M).group(0)
    assert layout == "struct BatchLayout { size_t tab, seeds, thr, ctrl, stats, ess, res, nreq, prob, order, values, anc, first, snap, carry, mass, total; };"


def test_drivers_take_their_keywords_and_default_to_the_old_loops():
    em = inspect.signature(cpprob_amd.em.hmm_table_em).parameters
    assert em["resident"].default is False
    gb = inspect.signature(cpprob_amd.gibbs.hmm_table_gibbs).parameters
    assert gb["retable"].default is False
    src = inspect.getsource(cpprob_amd.pgibbs.hmm_table_particle_gibbs)
    assert 'prior.pop("retable", False)' in src
    for fn in (cpprob_amd.gibbs.hmm_table_gibbs, cpprob_amd.pgibbs.hmm_table_particle_gibbs):
        assert "retable=True" in fn.__doc__ and "bit for bit" in fn.__doc__
    assert "resident=True" in cpprob_amd.em.hmm_table_em.__doc__


_OPTIONS_TU = r"""
#include <cstdint>
#include <vector>
#include "cpprob/cpprob.hpp"

int main()
{
    if (cpprob::gpu::options().fit_on_device) return 3;         // off by default
    cpprob::gpu::options().fit_on_device = true;
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        const cpprob::gpu::HmmTableFit fit = cpprob::gpu::hmm_table_fit(tables, {{0.5, 0.25}}, {512}, seeds, 2);
        return fit.tables.size() == 2 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_fit_on_device_option_compiles_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    src = tmp_path / "fit.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "fit.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]


def test_cli_flag_needs_the_iterations(tmp_path):
    main = os.path.join(ROOT, "cpprob_amd", "bin", "cpprob_main")
    (tmp_path / "tables.txt").write_text("[-1 1] [0.9 0.1 0.2 0.8] [0.5 0.25 -0.5]\n")
    p = subprocess.run([main, "--smc", "--model_folder", str(tmp_path), "--batch_tables_file", "tables.txt", "-n", "8", "--em_on_device"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--em_on_device" in p.stderr and "--em_iterations" in p.stderr
    fit = re.search(r"^inline HmmTableFit hmm_table_fit\(.*?^\}", open(os.path.join(ROOT, "cpprob_amd", "include", "cpprob", "detail", "host_engine.hpp")).read(), re.M | re.S).group(0)
    assert "options().fit_on_device" in fit and fit.count("kept && runs > 0, runs == 1") == 2
