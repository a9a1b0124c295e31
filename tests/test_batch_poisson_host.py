"""The host pieces of Poisson emissions (include/cpprob_hip.h: cpprob_hip_batch_begin_problems_poisson, _begin_online_poisson,
_retable_poisson, _retable_poisson_device, _mstep_poisson_device, _online_tables_poisson, _copy_rates): the symbols are declared, listed
and bound; what the library refuses without a context; the entry points go through the single routes of their unit and scaled siblings
and word every mix of families; what the Python layer refuses before it reaches the library; cpprob_main refuses the flag where it has
nothing to act on.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cpprob_amd.capi as cp

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cpprob_amd", "bin", "cpprob_main")
NEW = {"cpprob_hip_batch_begin_problems_poisson": 8, "cpprob_hip_batch_begin_online_poisson": 8, "cpprob_hip_batch_retable_poisson": 5,
       "cpprob_hip_batch_retable_poisson_device": 5, "cpprob_hip_batch_mstep_poisson_device": 7, "cpprob_hip_batch_online_tables_poisson": 3,
       "cpprob_hip_batch_copy_rates": 4}


def _hip():
    return open(os.path.join(ROOT, "cpprob_amd", "csrc", "cpprob_hip.hip")).read()


def _fn(hip, head):
    return re.search(r"^%s\(.*?^\}" % re.escape(head), hip, re.M | re.S).group(0)


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS and hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n_args, s
    assert "int cpprob_hip_batch_copy_rates(cpprob_hip_ctx* ctx, uint64_t problem, double* h_rates, double* h_log_rates);" in header
    assert re.search(r"int cpprob_hip_batch_mstep_poisson_device\(cpprob_hip_ctx\* ctx, const double\* d_stats, size_t n_doubles, double\* d_rates, double\* d_transition,\s+"
                     r"double\* d_log_rates, double rate_floor\);", header)
    assert callable(cp.Engine.batch_copy_rates)


def test_refusals_without_a_context():
    L = cp.load_library()
    x = np.full(88, 5.0)
    t = np.ones(1, np.uint32)
    u32 = C.POINTER(C.c_uint32)
    cfg = cp.BatchConfig(cp.ALG_SMC, cp.MODEL_HMM_TABLE, cp.RESAMPLE_SYSTEMATIC, 1, 0, 2.0, 8, 1)
    assert L.cpprob_hip_batch_begin_problems_poisson(None, C.byref(cfg), t.ctypes.data_as(u32), t.ctypes.data_as(u32), x.ctypes.data_as(C.POINTER(C.c_double)), 2,
                                                     x.ctypes.data, x.ctypes.data) == EINVAL
    assert L.cpprob_hip_batch_begin_online_poisson(None, C.byref(cfg), t.ctypes.data_as(u32), t.ctypes.data_as(u32), 2, x.ctypes.data, x.ctypes.data, None) == EINVAL
    assert L.cpprob_hip_batch_retable_poisson(None, x.ctypes.data, x.ctypes.data, x.ctypes.data, 1) == EINVAL
    assert b"ctx is NULL" in L.cpprob_hip_last_error(None)
    assert L.cpprob_hip_batch_retable_poisson_device(None, x.ctypes.data, x.ctypes.data, x.ctypes.data, 1) == EINVAL
    assert L.cpprob_hip_batch_mstep_poisson_device(None, x.ctypes.data, 88, x.ctypes.data, x.ctypes.data, None, 1e-6) == EINVAL
    assert L.cpprob_hip_batch_online_tables_poisson(None, x.ctypes.data, x.ctypes.data) == EINVAL
    assert L.cpprob_hip_batch_copy_rates(None, 0, x.ctypes.data, x.ctypes.data) == EINVAL
    assert np.all(x == 5.0)


def test_the_entry_points_are_the_single_routes():
    hip = _hip()
    for name, call in (("cpprob_hip_batch_begin_problems_poisson", "batch_begin_described(c, cfg, h_T, h_n, h_obs, k_in, h_rates, h_transition, nullptr, nullptr, kFamilyPoisson)"),
                       ("cpprob_hip_batch_begin_online_poisson", "batch_begin_described(c, cfg, h_Tcap, h_n, nullptr, k_in, h_rates, h_transition, nullptr, h_seeds, kFamilyPoisson)"),
                       ("cpprob_hip_batch_retable_poisson_device", "batch_retable_device(c, d_rates, d_transition, nullptr, d_observes, n_observes, false, true)"),
                       ("cpprob_hip_batch_retable_poisson", "batch_retable_host(c, h_rates, h_transition, nullptr, h_observes, n_observes, false, true)"),
                       ("cpprob_hip_batch_online_tables_poisson", 'batch_online_tables(c, h_rates, h_transition, nullptr, false, "cpprob_hip_batch_online_tables_poisson", true)')):
        entry = re.search(r"^int %s\([^;{}]*\)\n\{\n(.*?)^\}" % name, hip, re.M | re.S).group(1)
        assert [line.strip() for line in entry.splitlines()] == ["LANES_OWN(c);", "return %s;" % call], name
    assert "return batch_mstep_device(c, d_stats, n_doubles, d_rates, d_transition, kFamilyPoisson, nullptr, d_log_rates, rate_floor);" in _fn(hip, "int cpprob_hip_batch_mstep_poisson_device")
    # one copy of every route
    for head in ("static int batch_begin_described", "int batch_begin", "static int batch_retable_check", "static int batch_retable_enqueue", "static int batch_retable_device",
                 "static int batch_retable_host", "static int batch_mstep_device", "static int batch_online_tables", "static int batch_advance"):
        assert len(re.findall(r"^%s\(" % re.escape(head), hip, re.M)) == 1, head
    # every mix of families is worded, with CPPROB_HIP_ESTATE, before anything is read or enqueued
    check = _fn(hip, "static int batch_retable_check")
    for words in ("the batch has Poisson emissions: it is re-tabled by cpprob_hip_batch_retable_poisson", "the batch has no Poisson emissions: begin it with cpprob_hip_batch_begin_problems_poisson"):
        assert re.search(r"fail\(c, CPPROB_HIP_ESTATE, \"%s" % re.escape(words), check), words
    assert check.index("has Poisson emissions") < check.index("has emission scales") < check.index("lengths sum to")
    online = _fn(hip, "static int batch_online_tables")
    assert online.index("batch_learn_check(") < online.index("the batch has Poisson emissions: its tables are replaced by cpprob_hip_batch_online_tables_poisson") < online.index('"NULL argument"')
    mstep = _fn(hip, "static int batch_mstep_device")
    assert mstep.index("the batch has Poisson emissions: its M-step is") < mstep.index("the batch has no Poisson emissions: its M-step is") < mstep.index("hipSetDevice")
    assert re.search(r"fail\(c, CPPROB_HIP_EINVAL, \"rate_floor must be finite and > 0\"", mstep)
    for name in ("cpprob_hip_batch_learn_begin", "cpprob_hip_batch_learn_begin_scaled"):
        arm = _fn(hip, "int " + name)
        assert re.search(r"poisson\) return fail\(c, CPPROB_HIP_ESTATE, \"the batch has Poisson emissions: online EM serves", arm), name
        assert arm.index("has Poisson emissions") < (arm.index(".grow(") if ".grow(" in arm else len(arm))
    described = _fn(hip, "static int batch_begin_described")
    assert re.search(r"fail\(c, CPPROB_HIP_EUNSUPPORTED, \"Poisson emissions serve CPPROB_HIP_MODEL_HMM_TABLE with per-problem tables\"", described)
    assert described.index("batch_check_tables(") < described.index("return batch_begin(")
    tables = _fn(hip, "static int batch_check_tables")
    assert "poisson_bad(" in tables and "emission rates must be > 0, finite and normal numbers" in tables and '"problem " + std::to_string(b)' in tables
    # the host writes Poisson rows with poisson_entry itself, at the begin and in the plain advance; the log-factorials are uploaded once
    assert "poisson_entry(y, rate[s2], log_rate[s2], lf)" in hip
    assert "poisson_step_ll(" in _fn(hip, "int batch_begin") and "poisson_step_ll(" in _fn(hip, "static int batch_advance")
    assert hip.count("poisson_log_fact_table(") == 1 and hip.count("d_lfact.grow(") == 1 and "if (poisson && bs->lfact.empty())" in hip
    # no workspace region is added
    assert "lfact" not in _fn(hip, "BatchLayout batch_layout")


def test_python_refusals_before_the_library():
    import cpprob_amd.decode as decode
    import cpprob_amd.em as em
    rates, trans = np.ones((1, 2)), np.full((1, 2, 2), 0.5)
    for tables in (None, (rates, trans, np.ones((1, 2))), (rates, None)):
        with pytest.raises(ValueError, match="poisson"):
            cp._poisson("poisson", tables)
    with pytest.raises(ValueError):
        cp._poisson("gamma", (rates, trans))
    assert cp._poisson("poisson", (rates, trans)) is True and cp._poisson("normal", None) is False
    with pytest.raises(ValueError, match="Poisson"):
        em.hmm_table_em(None, [np.ones(3)], rates, trans, 8, [1], 1, emission="poisson", sigmas0=np.ones((1, 2)))
    with pytest.raises(ValueError, match="Poisson"):
        decode.hmm_table_decode(None, [np.ones(3)], rates, trans, 8, [1], emission="poisson", sigmas=np.ones((1, 2)))


def test_cli_refusals_end_before_a_device(tmp_path):
    (tmp_path / "t.txt").write_text("[1 8] [0.9 0.1 0.1 0.9] [0 3 9]\n")
    base = [MAIN, "--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", "16"]
    for extra, words in ((["--model", "hmm16", "--observes", "[1 2]", "--poisson_emissions"], ("--poisson_emissions", "--batch_tables_file")),
                         (["--batch_tables_file", "t.txt", "--poisson_emissions", "--emission_scales"], ("--poisson_emissions", "--emission_scales")),
                         (["--batch_tables_file", "t.txt", "--poisson_emissions", "--stream_chunk", "2", "--online_em"], ("--online_em", "Poisson"))):
        q = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert q.returncode != 0 and all(w in q.stderr for w in words), (extra, q.stderr)
