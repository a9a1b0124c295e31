"""The host pieces of tied online EM (include/cpprob_hip.h: cpprob_hip_batch_learn_tie, _learn_pooled_record): the symbols are declared,
listed and bound; what the library refuses without a context; the refusals a begun batch earns are worded in the library with their
codes (they are exercised on a device in tests/test_gpu_batch_learn_tied.py); the tied branch of a learning advance enqueues learn,
pool, tied in that order, allocates nothing and waits for nothing; the workspace sizes, which the feature leaves where they were; the
drivers' signatures; the C++ option; the command line's refusal."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cpprob_amd
import cpprob_amd.capi as cp
import test_batch_learn_host as H

EINVAL = -1
ROOT = H.ROOT
NEW = {"cpprob_hip_batch_learn_tie": 1, "cpprob_hip_batch_learn_pooled_record": 3}


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS and cp.SYMBOLS.count(s) == 1
        assert hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n_args, s
        assert getattr(L, s).restype is C.c_int
    assert "int cpprob_hip_batch_learn_tie(cpprob_hip_ctx* ctx);" in header
    assert "int cpprob_hip_batch_learn_pooled_record(cpprob_hip_ctx* ctx, double* h_out, size_t n_doubles);" in header
    assert L.cpprob_hip_batch_learn_tie.argtypes == [C.c_void_p] and L.cpprob_hip_batch_learn_pooled_record.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t]
    assert "weigh equally whatever their lengths" in header
    assert L.cpprob_hip_abi_version() == 3
    assert callable(cp.Engine.batch_learn_pooled_record)


def test_refusals_without_a_context():
    L = cp.load_library()
    x = np.ones(88)
    assert L.cpprob_hip_batch_learn_tie(None) == EINVAL
    assert b"ctx is NULL" in L.cpprob_hip_last_error(None)
    assert L.cpprob_hip_batch_learn_pooled_record(None, x.ctypes.data, 88) == EINVAL
    assert np.all(x == 1.0)


def test_the_library_words_every_refusal_with_its_code():
    hip = H._hip()
    tie = H._body(hip, "int cpprob_hip_batch_learn_tie")
    for code, words in (("CPPROB_HIP_ESTATE", "is not armed: call cpprob_hip_batch_learn_begin before cpprob_hip_batch_learn_tie"),
                        ("CPPROB_HIP_ESTATE", "has no tie: call cpprob_hip_batch_tie before cpprob_hip_batch_learn_tie"),
                        ("CPPROB_HIP_ESTATE", "cpprob_hip_batch_learn_tie comes before the first advance")):
        assert re.search(r"fail\(c, %s, [^\n]*%s" % (code, re.escape(words)), tie), words
    # the state first, then the tables on the host mirrors, then the one allocation; the flag last
    assert tie.index("batch_learn_check(") < tie.index("comes before the first advance") < tie.index("batch_tied_tables_check(") < tie.index(".grow(") < tie.index("bs->learn_tied = true;")
    assert "bs->means.data(), bs->trans.data()" in tie and "hipMalloc" not in tie
    same = H._body(hip, "static int batch_tied_tables_check")
    assert re.search(r"fail\(c, CPPROB_HIP_EINVAL, [^\n]*the table of problem [^\n]*differs from that of problem", same)
    assert "hipMemcpy" not in same and ".grow(" not in same and "std::memcmp" in same
    rec = H._body(hip, "int cpprob_hip_batch_learn_pooled_record")
    assert re.search(r"fail\(c, CPPROB_HIP_ESTATE, [^\n]*does not pool: call cpprob_hip_batch_learn_tie", rec)
    assert re.search(r"fail\(c, CPPROB_HIP_EINVAL, [^\n]*the output is too small", rec) and "hipStreamSynchronize" in rec
    # while the learner pools: no new tie, no tables that differ within a group -- and nothing else changes for any other batch
    retie = H._body(hip, "int cpprob_hip_batch_tie")
    assert re.search(r"if \(bs->learn_tied\) return fail\(c, CPPROB_HIP_ESTATE, [^\n]*pools over the tie in force", retie)
    assert retie.index("pools over the tie in force") < retie.index("hipStreamSynchronize")
    host = H._body(hip, "static int batch_online_tables")
    assert "if (bs->learn_tied) if (int rc = batch_tied_tables_check(" in host
    assert host.index("batch_check_tables(") < host.index("batch_tied_tables_check(") < host.index("bs->means.assign(")
    # arming again and any begin end the pooling: both disarm through batch_learn_free
    assert "bs->armed = false; bs->learn_tied = false;" in H._body(hip, "void batch_learn_free")
    assert "batch_learn_free(bs);" in H._body(hip, "int cpprob_hip_batch_learn_begin") and "if (bs->armed) batch_learn_free(bs);" in H._body(hip, "int batch_begin")
    assert hip.count("learn_tied = true") == 1


def test_the_tied_branch_enqueues_learn_pool_tied_and_nothing_else():
    hip = H._hip()
    enq = H._body(hip, "static int batch_learn_enqueue")
    assert "hipStreamSynchronize" not in enq and "hipDeviceSynchronize" not in enq and ".grow(" not in enq and "hipMalloc" not in enq
    assert "la.t_min = bs->learn_tied ? INT32_MAX : " in enq
    order = [enq.index(w) for w in ("hipLaunchKernelGGL(batch_learn_scaled_kernel", "hipLaunchKernelGGL(batch_learn_kernel", "if (bs->learn_tied) {",
                                    "batch_pool_enqueue(c, bs->learn.rec.as<double>(), 1, 0, bs->learn.pooled.as<double>())",
                                    "hipLaunchKernelGGL(batch_learn_tied_scaled_kernel", "hipLaunchKernelGGL(batch_learn_tied_kernel", "bs->thr_stale = true;")]
    assert order == sorted(order)
    assert "ta.t_min = (int64_t)bs->learn_t_min;" in enq and "(bs->tie_groups + kWaves - 1) / kWaves" in enq
    pool = H._body(hip, "static int batch_pool_enqueue")
    assert "hipStreamSynchronize" not in pool and ".grow(" not in pool
    # the learner owns the pooled records: a line of its own in the Learner, grown by cpprob_hip_batch_learn_tie, released with the rest
    state = re.search(r"^struct BatchState \{.*?^\};", hip, re.M | re.S).group(0)
    learner = re.search(r"struct Learner \{.*?\} learn;", state, re.S).group(0)
    assert "DeviceBuffer gamma, means, trans, tau, rec, obs, status, first;" in learner and re.search(r"^\s*DeviceBuffer pooled;", learner, re.M)
    assert "&pooled}) b->release();" in learner
    assert hip.count("learn.pooled.grow(") == 1 and "learn.pooled.grow(" in H._body(hip, "int cpprob_hip_batch_learn_tie")


def test_workspace_sizes_are_where_they_were():
    H.test_workspace_sizes_are_where_they_were()


def test_the_drivers_signatures():
    sig = inspect.signature(cpprob_amd.hmm_table_online_em).parameters
    assert sig["groups"].default is None and list(sig)[-1] == "groups" and sig["sigma_floor"].default == 1e-3 and sig["t_min"].default == 20
    sig = inspect.signature(cp.Engine.batch_learn_begin).parameters
    assert list(sig) == ["self", "gamma", "t_min", "sigma_floor", "tied"] and sig["tied"].default is False and sig["sigma_floor"].default is None
    assert list(inspect.signature(cp.Engine.batch_learn_pooled_record).parameters) == ["self"]
    # the driver checks tables0 within the groups before it touches the engine
    eng = H._engine([3, 3, 3])
    means, trans = np.zeros((3, 2)), np.full((3, 2, 2), 0.5)
    means[2, 1] = 1.0
    with pytest.raises(ValueError, match="problem 2 differ from those of problem 0"):
        cpprob_amd.hmm_table_online_em(eng, [np.zeros(3)] * 3, (means, trans), 4, [1, 2, 3], 2, groups=[0, 1, 0])
    with pytest.raises(ValueError, match="one id per table"):
        cpprob_amd.hmm_table_online_em(eng, [np.zeros(3)] * 3, (means, trans), 4, [1, 2, 3], 2, groups=[0, 1])


_OPTIONS_TU = r"""
#include <cstdint>
#include <vector>
#include "cpprob/cpprob.hpp"

int main()
{
    cpprob::gpu::Options& opt = cpprob::gpu::options();
    if (opt.learn_tied || !opt.tie_groups.empty()) return 3;                                        // off by default
    opt.learn_tables = true; opt.learn_tied = true; opt.tie_groups = {0, 0}; opt.learn_burn_in = 4;
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
def test_the_tied_option_compiles_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    src = tmp_path / "learn_tied.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "learn_tied.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]
    engine = open(os.path.join(ROOT, "cpprob_amd", "include", "cpprob", "detail", "host_engine.hpp")).read()
    assert engine.index('"cpprob_hip_batch_learn_begin")') < engine.index('"cpprob_hip_batch_learn_tie")') and engine.count("cpprob_hip_batch_learn_tie(ctx.get())") == 1


@pytest.mark.parametrize("flag", [["--tie_tables"], ["--tie_groups", "[0]"]])
def test_cli_tie_flags_need_a_fit_or_online_em(tmp_path, flag):
    main = os.path.join(ROOT, "cpprob_amd", "bin", "cpprob_main")
    (tmp_path / "tables.txt").write_text("[-1 1] [0.9 0.1 0.2 0.8] [0.5 0.25 -0.5]\n")
    base = [main, "--smc", "--model_folder", str(tmp_path), "--batch_tables_file", "tables.txt", "-n", "8"]
    p = subprocess.run(base + flag, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and all(w in p.stderr for w in ("--tie_tables", "--tie_groups", "--em_iterations", "--online_em"))
    p = subprocess.run(base + flag + ["--stream_chunk", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--em_iterations" in p.stderr and "--online_em" in p.stderr
    # with --online_em the tie is taken: what is refused next is the missing stream, by --online_em's own message
    p = subprocess.run(base + flag + ["--online_em"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--online_em" in p.stderr and "--stream_chunk" in p.stderr and "--em_iterations" not in p.stderr
