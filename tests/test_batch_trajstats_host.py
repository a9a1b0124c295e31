"""The host pieces of the trajectory statistics calls (include/cpprob_hip.h: cpprob_hip_batch_traj_stats*): the symbols are declared,
listed and bound; what the library and the Python wrappers refuse without a device; the records' names; the C++ options as plain
C++14; and the command line's refusals, which end before anything touches a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import cpprob_amd.capi as cp
import trajstats_ref as TS

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cpprob_amd", "bin", "cpprob_main")
NEW = {"cpprob_hip_batch_traj_stats": 7, "cpprob_hip_batch_traj_stats_device": 7, "cpprob_hip_batch_traj_stats_grid": 2}


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n_args, s
    assert L.cpprob_hip_abi_version() == 3
    for name in ("batch_traj_stats", "batch_traj_stats_device", "batch_traj_stats_grid"):
        assert callable(getattr(cp.Engine, name)), name
    assert cp.STATS_PER_PROBLEM == TS.RECORD and cp.TRAJ_STATS_TILE == 256
    # cpprob_hip_batch_pass_grid keeps its signature
    assert len(L.cpprob_hip_batch_pass_grid.argtypes) == 5
    assert re.search(r"int cpprob_hip_batch_pass_grid\(cpprob_hip_ctx\* ctx, uint32_t\* decode_forward_grid_x, uint32_t\* decode_trace_grid_y, uint32_t\* forecast_grid_y,", header)


def test_refusals_without_a_device():
    L = cp.load_library()
    rec = np.full(2 * 88, -5.0)
    obs = np.zeros(4)
    for fn in (L.cpprob_hip_batch_traj_stats, L.cpprob_hip_batch_traj_stats_device):
        assert fn(None, 2, 0, obs.ctypes.data, obs.size, rec.ctypes.data, rec.size) == EINVAL
        assert fn(None, 2, 0, None, 0, rec.ctypes.data, rec.size) == EINVAL
    assert b"ctx is NULL" in L.cpprob_hip_last_error(None)
    import ctypes as C
    gy = C.c_uint32(77)
    assert L.cpprob_hip_batch_traj_stats_grid(None, C.byref(gy)) == EINVAL and gy.value == 77
    assert np.all(rec == -5.0)


def test_wrappers_check_their_arguments():
    """An Engine without a context: the wrappers' checks run before anything is allocated or the library is called."""
    eng = cp.Engine.__new__(cp.Engine)
    eng.batch_B = 4
    for bad in (dict(n_traj=0), dict(n_traj=(1 << 20) + 1), dict(n_traj=-1), dict(n_traj=3, draw_index=1 << 16), dict(n_traj=3, draw_index=-1)):
        with pytest.raises(ValueError):
            eng.batch_traj_stats(**bad)
        with pytest.raises(ValueError):
            eng.batch_traj_stats_device(None, **bad)
    assert cp.Engine._traj_stats_args(1 << 20, (1 << 16) - 1) == (1 << 20, (1 << 16) - 1)


def test_records_keep_their_names():
    rec = np.arange(2 * 3 * 88, dtype=np.float64).reshape(2, 3, 88)
    st = cp.split_traj_stats(rec)
    assert st["xi"].shape == (2, 3, 8, 8) and st["occ"].shape == st["occ_y"].shape == st["occ_yy"].shape == (2, 3, 8)
    assert st["xi"][1, 2, 4, 5] == (3 + 2) * 88 + 8 * 4 + 5 and st["occ"][0, 1, 0] == 88 + 64 and st["occ_y"][0, 0, 0] == 72 and st["occ_yy"][1, 2, 7] == 6 * 88 - 1
    one = {f: v[:, 0] for f, v in st.items()}                          # (the trajectory axis indexed away: split_stats' dict)
    flat = cp.split_stats(rec[:, 0])
    assert all(np.array_equal(one[f], flat[f]) for f in flat)
    # split_stats on [B, 88] is what it was
    old = cp.split_stats(np.arange(2 * 88, dtype=np.float64).reshape(2, 88))
    assert old["xi"].shape == (2, 8, 8) and old["xi"][1, 2, 5] == 88 + 8 * 2 + 5 and old["occ"][0].tolist() == list(range(64, 72)) and old["occ_yy"][1, 7] == 88 + 87
    path = np.array([0, 2, 2, 1])
    assert np.array_equal(cp.split_stats(TS.record(TS.stats(path, [1.0, 2.0, 3.0, 4.0]))[None])["xi"][0], TS.stats(path)["xi"])


def test_kernel_is_built_into_the_library():
    hip = open(os.path.join(ROOT, "cpprob_amd", "csrc", "cpprob_hip.hip")).read()
    assert "batch_traj_stats_kernel<3>" in hip and "batch_traj_stats_kernel<8>" in hip
    # both calls reach them through the one batch_smooth_enqueue (as every other pass does)
    assert len(re.findall(r"^static int batch_smooth_enqueue\(", hip, re.M)) == 1 and hip.count("static int batch_smooth_enqueue(") == 1
    for name in ("cpprob_hip_batch_traj_stats", "cpprob_hip_batch_traj_stats_device"):
        body = re.search(r"^int %s\(.*?^\}" % name, hip, re.M | re.S)
        assert body and "batch_smooth_enqueue(" in body.group(0), name


_OPTIONS_TU = r"""
#include <cstdint>
#include <string>
#include <tuple>
#include <vector>
#include <boost/random/normal_distribution.hpp>
#include "cpprob/cpprob.hpp"

void model(const double& y) { cpprob::observe(boost::random::normal_distribution<>{0, 1}, y); }

int main()
{
    cpprob::gpu::options().trajectory_stats = 3;
    cpprob::gpu::options().trajectory_stats_draw_index = 2;
    std::vector<std::tuple<double>> obs{std::make_tuple(0.5), std::make_tuple(-0.5)};
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        const std::vector<cpprob::gpu::Result> r = cpprob::gpu::inference_batch(cpprob::StateType::smc, model, obs, 1024, seeds);
        const std::vector<cpprob::gpu::Result> q = cpprob::gpu::hmm_table_batch(tables, {{0.5, 0.25}}, {512}, seeds);
        cpprob::gpu::HmmTableStream stream(tables, {4}, {512}, seeds);
        const std::vector<cpprob::gpu::Result> s = stream.advance({{0.25, 0.125}, {1.0}});
        return r.size() == 2 && q[0].trajectory_stats.size() == 3 && s[1].trajectory_stats[0].size() == 88 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_trajectory_stats_options_compile_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """Options::trajectory_stats / ::trajectory_stats_draw_index and the entry points that read them are plain C++14 host code (the
    pattern of tests/test_batch_forecast_host.py)."""
    src = tmp_path / "trajstats.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "trajstats.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]


def test_cli_refusals_name_the_flag():
    """cpprob_main --trajectory_stats outside the batch modes, or on a filtering-only batch that keeps no masses, ends with a message
    that names the flag before anything touches a device."""
    p = subprocess.run([MAIN, "--smc", "--model", "hmm16", "--observes", "1", "--trajectory_stats", "3"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--trajectory_stats serves the batch modes" in p.stderr
    q = subprocess.run([MAIN, "--smc", "--batch_tables_file", "none.txt", "--filtering_only", "--trajectory_stats", "3"], capture_output=True, text=True, timeout=60)
    assert q.returncode != 0 and "--trajectory_stats" in q.stderr and "--keep_masses" in q.stderr
