"""The host pieces of online EM (include/cpprob_hip.h: cpprob_hip_batch_learn_begin, _advance_learn*, _online_tables, _learn_tables*,
_learn_record): the symbols are declared, listed and bound; what the library refuses without a context and what the wrappers refuse
before they call it; the refusals a begun batch earns are worded in the library with their codes (they are exercised on a device in
tests/test_gpu_batch_learn.py), re-tabling an online batch included, which answers as before; the host state a learning advance
leaves stale; the workspace sizes, which the feature leaves where they were; the driver's step sizes."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cpprob_amd
import cpprob_amd.capi as cp

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cpprob_hip_batch_learn_begin": 4, "cpprob_hip_batch_advance_learn": 3, "cpprob_hip_batch_advance_learn_device": 4, "cpprob_hip_batch_online_tables": 3,
       "cpprob_hip_batch_learn_tables": 4, "cpprob_hip_batch_learn_tables_device": 3, "cpprob_hip_batch_learn_record": 3}


def _hip():
    return open(os.path.join(ROOT, "cpprob_amd", "csrc", "cpprob_hip.hip")).read()


def _body(hip, head):
    return re.search(r"^%s\([^;{}]*\)\n\{.*?^\}" % head, hip, re.M | re.S).group(0)      # (a definition, not a declaration)


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n_args, s
    assert "int cpprob_hip_batch_learn_begin(cpprob_hip_ctx* ctx, const double* h_gamma, size_t n_gamma, uint32_t t_min);" in header
    assert "int cpprob_hip_batch_advance_learn_device(cpprob_hip_ctx* ctx, const uint32_t* h_dT, const double* d_observes, size_t n_observes);" in header
    assert "CURRENT threshold words for every row" in header and "prequential" in header
    assert L.cpprob_hip_abi_version() == 3
    for name in ("batch_learn_begin", "batch_advance_learn", "batch_advance_learn_device", "batch_online_tables", "batch_learn_tables", "batch_learn_tables_device",
                 "batch_learn_record"):
        assert callable(getattr(cp.Engine, name)), name
    assert cpprob_amd.hmm_table_online_em is cpprob_amd.online_em.hmm_table_online_em


def test_refusals_without_a_context():
    L = cp.load_library()
    x = np.ones(8)
    dT = np.zeros(2, np.uint32)
    st = np.zeros(2, np.int32)
    p32 = C.POINTER(C.c_uint32)
    assert L.cpprob_hip_batch_learn_begin(None, x.ctypes.data, 8, 3) == EINVAL
    assert b"ctx is NULL" in L.cpprob_hip_last_error(None)
    assert L.cpprob_hip_batch_advance_learn(None, dT.ctypes.data_as(p32), x.ctypes.data) == EINVAL
    assert L.cpprob_hip_batch_advance_learn_device(None, dT.ctypes.data_as(p32), x.ctypes.data, 0) == EINVAL
    assert L.cpprob_hip_batch_online_tables(None, x.ctypes.data, x.ctypes.data) == EINVAL
    assert L.cpprob_hip_batch_learn_tables(None, x.ctypes.data, x.ctypes.data, st.ctypes.data_as(C.POINTER(C.c_int32))) == EINVAL
    assert L.cpprob_hip_batch_learn_tables_device(None, x.ctypes.data, x.ctypes.data) == EINVAL
    assert L.cpprob_hip_batch_learn_record(None, x.ctypes.data, 8) == EINVAL
    assert np.all(x == 1.0) and not st.any()


def _engine(T):
    """An Engine without a context: the wrappers' checks run before the library is called."""
    eng = cp.Engine.__new__(cp.Engine)
    eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K, eng.batch_k = len(T), max(T), 4, 8, 2
    eng.batch_shapes = (np.array(T, np.uint32), np.full(len(T), 4, np.uint32))
    return eng


def test_wrappers_check_their_arguments():
    eng = _engine([3, 1, 2])
    for tables in ((np.zeros((2, 2)), np.zeros((2, 2, 2))),            # a table short
                   (np.zeros((3, 2)), np.zeros((3, 2, 3))),            # rows of another k
                   (np.zeros(6), np.zeros((3, 2, 2)))):                # means without their axis
        with pytest.raises(ValueError):
            eng.batch_online_tables(tables)
    with pytest.raises(ValueError):
        eng.batch_advance_learn([np.zeros(1), np.zeros(0)])             # a sequence short
    with pytest.raises(ValueError):
        eng.batch_advance_learn_device([1, 0], None)                    # a count short
    with pytest.raises(ValueError):
        cpprob_amd.hmm_table_online_em(eng, [np.zeros(3)] * 3, (np.zeros((3, 2)), np.zeros((3, 2, 2))), 4, [1, 2, 3], 0)
    with pytest.raises(ValueError):
        cpprob_amd.hmm_table_online_em(eng, [np.zeros(3)] * 2, (np.zeros((3, 2)), np.zeros((3, 2, 2))), 4, [1, 2, 3], 4)


def test_the_library_words_every_refusal_with_its_code():
    hip = _hip()
    check = _body(hip, "static int batch_learn_check")
    for code, words in (("CPPROB_HIP_ESTATE", "serves a batch begun by cpprob_hip_batch_begin_online"),
                        ("CPPROB_HIP_EUNSUPPORTED", "the table of CPPROB_HIP_MODEL_HMM3 is the model's"),
                        ("CPPROB_HIP_EUNSUPPORTED", "the context's shared table")):
        assert re.search(r"fail\(c, %s, [^\n]*%s" % (code, re.escape(words)), check), words
    arm = _body(hip, "int cpprob_hip_batch_learn_begin")
    for code, words in (("CPPROB_HIP_ESTATE", "begin it with CPPROB_HIP_BATCH_KEEP_MASSES"),
                        ("CPPROB_HIP_ESTATE", "comes before the first advance"),
                        ("CPPROB_HIP_EINVAL", "lies below the largest capacity"),
                        ("CPPROB_HIP_EINVAL", "lies outside \\(0, 1\\]")):
        assert re.search(r"fail\(c, %s, [^\n]*%s" % (code, words), arm), words
    # nothing is allocated, freed or enqueued before every check has passed
    assert arm.index("lies outside") < arm.index("batch_learn_free(") < arm.index(".grow(") and "hipMalloc" not in arm
    adv = _body(hip, "static int batch_advance")
    for code, words in (("CPPROB_HIP_ESTATE", "the online batch is not armed"),
                        ("CPPROB_HIP_ESTATE", "it is advanced by cpprob_hip_batch_advance_learn"),
                        ("CPPROB_HIP_EINVAL", "the sum of h_dT")):
        assert re.search(r"fail\(c, %s, [^\n]*%s" % (code, re.escape(words)), adv), words
    assert '" exceed its capacity of "' in adv                                 # (cpprob_hip_batch_advance's check and message)
    assert adv.index("the sum of h_dT") < adv.index("hipSetDevice") < adv.index("bs->prob[b].T = (int32_t)(L + h_dT[b]);")
    # the three public advances are the one helper
    for name, call in (("cpprob_hip_batch_advance", "batch_advance(c, h_dT, h_obs, nullptr, 0, readout, false)"),
                       ("cpprob_hip_batch_advance_learn", "batch_advance(c, h_dT, h_obs, nullptr, 0, 1, true)"),
                       ("cpprob_hip_batch_advance_learn_device", "batch_advance(c, h_dT, nullptr, d_obs, n_observes, 1, true)")):
        assert call in _body(hip, "int " + name), name
    # the host route validates with the begin's own statements before it changes anything
    host = _body(hip, "static int batch_online_tables")
    assert host.index("batch_learn_check(") < host.index("batch_check_tables(") < host.index("bs->means.assign(") < host.index("hipMemcpyAsync")
    assert "bs->thr_stale = false; bs->lp_ready = false; bs->lp_sent = false;" in host and "if (bs->armed)" in host
    # ... and is the body of the unit and of the scaled entry point, which name themselves for the state's refusal
    for name, call in (("cpprob_hip_batch_online_tables", 'batch_online_tables(c, h_means, h_transition, nullptr, false, "cpprob_hip_batch_online_tables")'),
                       ("cpprob_hip_batch_online_tables_scaled", 'batch_online_tables(c, h_means, h_transition, h_sigmas, true, "cpprob_hip_batch_online_tables_scaled")')):
        entry = _body(hip, "int " + name)
        assert [line.strip() for line in entry.splitlines()[2:-1]] == ["LANES_OWN(c);", "return %s;" % call], name
    # the state is judged after batch_learn_check and before the arguments
    assert host.index("batch_learn_check(") < host.index('"the batch has emission scales: its tables are replaced by') < host.index('"the batch has no emission scales: begin it with') \
        < host.index('"NULL argument"') < host.index("batch_check_tables(")
    # re-tabling an online batch answers as before
    retable = _body(hip, "static int batch_retable_check")
    assert 'if (bs->online) return fail(c, CPPROB_HIP_EUNSUPPORTED, "an online batch is not re-tabled: its advances evaluate their rows from the host\'s means");' in retable


def test_a_learning_advance_leaves_the_mirrors_stale_and_a_begin_disarms():
    hip = _hip()
    adv = _body(hip, "static int batch_advance")
    assert "bs->tab_stale = true;" in adv and adv.index("hipLaunchKernelGGL(batch_learn_rows_kernel") < adv.index("batch_launch(c, bs, readout != 0)") < adv.index("batch_learn_enqueue(")
    enq = _body(hip, "static int batch_learn_enqueue")
    assert "bs->thr_stale = true; bs->lp_ready = false; bs->lp_sent = false;" in enq and "bs->decoded.assign(B, 0);" in enq
    assert "hipStreamSynchronize" not in enq and ".grow(" not in enq and "batch_pass_prologue(" in enq
    begin = _body(hip, "int batch_begin")
    assert "if (bs->armed) batch_learn_free(bs);" in begin
    # the learner's allocations are owning members of the state: disarming releases them, batch_free deletes the state
    state = re.search(r"^struct BatchState \{.*?^\};", hip, re.M | re.S).group(0)
    learner = re.search(r"struct Learner \{.*?\} learn;", state, re.S).group(0)
    assert "DeviceBuffer gamma, means, trans, tau, rec, obs, status, first;" in learner and "PinnedBuffer pin_first;" in learner
    disarm = _body(hip, "void batch_learn_free")
    assert "bs->learn.release();" in disarm and "bs->armed = false;" in disarm
    free = _body(hip, "void batch_free")
    assert "delete c->batch;" in free and "dfree(" not in free
    # batch_smc_kernel is launched where it was: by batch_launch alone
    assert hip.count("hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(kThreads), (size_t)batch_lds_bytes(a.n), c->stream, a);") == 1


def test_workspace_sizes_are_where_they_were():
    """No workspace region is added: the device tables, tau, the records and the status words are allocations of the context's own."""
    want = {(True, False): (142592, 432128, 189696), (False, False): (14848, 64768, 29184), (False, True): (20480, 91648, 36864)}
    for (kh, km), (uni, prob, online) in want.items():
        assert cp.batch_workspace_bytes(cp.MODEL_HMM_TABLE, 300, 5, 17, keep_history=kh, keep_masses=km) == uni
        assert cp.batch_problems_workspace_bytes(cp.MODEL_HMM_TABLE, [1, 31, 32, 33, 70, 70], [1, 64, 1500, 64, 5, 300], keep_history=kh, keep_masses=km) == prob
        assert cp.batch_online_workspace_bytes(cp.MODEL_HMM_TABLE, [4, 40, 9], [8192, 3, 100], keep_history=kh, keep_masses=km) == online
    layout = re.search(r"^struct BatchLayout \{[^\n]*\};", _hip(), re.M).group(0)
    assert layout == "struct BatchLayout { size_t tab, seeds, thr, ctrl, stats, ess, res, nreq, prob, order, values, anc, first, snap, carry, mass, total; };"


def test_the_driver_evaluates_the_step_sizes_on_the_host():
    g = cpprob_amd.online_em.step_sizes(5, 0.6)
    assert g.dtype == np.float64 and g[0] == 1.0 and list(g) == [math.pow(t + 1.0, -0.6) for t in range(5)] and np.all((g > 0) & (g <= 1))
    sig = inspect.signature(cpprob_amd.hmm_table_online_em).parameters
    assert sig["step_exponent"].default == 0.6 and sig["keep_history"].default is False and "chunk" in sig and "t_min" in sig


_OPTIONS_TU = r"""
#include <cstdint>
#include <vector>
#include "cpprob/cpprob.hpp"

int main()
{
    cpprob::gpu::Options& opt = cpprob::gpu::options();
    if (opt.learn_tables || opt.learn_step_exponent != 0.6 || opt.learn_burn_in != 20) return 3;     // off by default
    opt.learn_tables = true; opt.learn_step_exponent = 0.75; opt.learn_burn_in = 4;
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        cpprob::gpu::HmmTableStream stream(tables, {8}, {64}, seeds);
        stream.advance({{0.5, 0.25}, {1.5}});
        return stream.tables().size() == 2 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_learn_options_compile_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    src = tmp_path / "learn.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "learn.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]


def test_cli_flag_needs_the_stream(tmp_path):
    main = os.path.join(ROOT, "cpprob_amd", "bin", "cpprob_main")
    (tmp_path / "tables.txt").write_text("[-1 1] [0.9 0.1 0.2 0.8] [0.5 0.25 -0.5]\n")
    base = [main, "--smc", "--model_folder", str(tmp_path), "--batch_tables_file", "tables.txt", "-n", "8", "--online_em"]
    p = subprocess.run(base, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--online_em" in p.stderr and "--stream_chunk" in p.stderr
    p = subprocess.run(base + ["--stream_chunk", "2", "--filtering_only"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--online_em" in p.stderr and "--keep_masses" in p.stderr
