"""The host pieces of the forecast calls (include/cpprob_hip.h: cpprob_hip_batch_forecast*, cpprob_hip_batch_predictive*): the symbols
are declared, listed and bound; what the library refuses without a device; the Python wrappers' own argument checks; and the kernel
header's standing promises that a text can show."""
import os
import re

import numpy as np
import pytest

import cpprob_amd
import cpprob_amd.capi as cp

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cpprob_hip_batch_forecast": 8, "cpprob_hip_batch_forecast_device": 8, "cpprob_hip_batch_predictive": 5, "cpprob_hip_batch_predictive_device": 5,
       "cpprob_hip_batch_pass_grid": 5}


def test_forecast_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in cp.SYMBOLS
        assert hasattr(L, s)
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == n_args, s
    assert L.cpprob_hip_abi_version() == 3
    for name in ("batch_forecast", "batch_forecast_device", "batch_predictive", "batch_predictive_device"):
        assert callable(getattr(cp.Engine, name)), name
    assert cpprob_amd.forecast.observation_forecast is cpprob_amd.observation_forecast
    assert cpprob_amd.forecast.predictive_log_likelihood is cpprob_amd.predictive_log_likelihood


def test_forecast_refusals_without_a_device():
    L = cp.load_library()
    marg = np.full(6, -5.0)
    traj = np.full(8, -5, np.int32)
    assert L.cpprob_hip_batch_forecast(None, 1, 2, 0, marg.ctypes.data, marg.size, traj.ctypes.data, traj.size) == EINVAL
    assert L.cpprob_hip_batch_forecast_device(None, 1, 2, 0, None, 0, None, 0) == EINVAL
    assert L.cpprob_hip_batch_predictive(None, None, 2, marg.ctypes.data, marg.size) == EINVAL
    assert L.cpprob_hip_batch_predictive_device(None, None, 2, None, 0) == EINVAL
    assert b"ctx" in L.cpprob_hip_last_error(None)
    assert np.all(marg == -5.0) and np.all(traj == -5)


def _shell():
    """An Engine without a context: the wrappers' checks run before the library is called."""
    eng = cp.Engine.__new__(cp.Engine)
    eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K = 4, 23, 8, 8
    eng.batch_shapes = (np.array([0, 2, 7, 23], np.uint32), np.array([1, 300, 777, 1025], np.uint32))
    return eng


def test_wrappers_check_their_arguments():
    eng = _shell()
    for bad in (dict(horizon=0), dict(horizon=1 << 24), dict(horizon=-1), dict(horizon=3, n_traj=(1 << 20) + 1), dict(horizon=3, n_traj=-1),
                dict(horizon=3, draw_index=1 << 16), dict(horizon=3, draw_index=-1)):
        with pytest.raises(ValueError):
            eng.batch_forecast(**bad)
        with pytest.raises(ValueError):
            eng.batch_forecast_device(**bad)
    assert cp.Engine._forecast_args((1 << 24) - 1, 1 << 20, (1 << 16) - 1) == ((1 << 24) - 1, 1 << 20, (1 << 16) - 1)
    with pytest.raises(ValueError):
        eng._batch_predictive_shapes([0, 0])
    with pytest.raises(ValueError):
        eng._batch_predictive_shapes([0, 0, -1, 0])
    with pytest.raises(ValueError):
        eng.batch_predictive_device(None)
    none, rows = eng._batch_predictive_shapes(None)
    assert none is None and rows == 24
    h_from, rows = eng._batch_predictive_shapes([1, 0, 7, 20])
    assert h_from.dtype == np.uint32 and h_from.tolist() == [1, 0, 7, 20] and rows == 4
    _, rows = eng._batch_predictive_shapes([1, 3, 8, 24])            # every problem past its last row
    assert rows == 0 and eng.batch_predictive([1, 3, 8, 24]).shape == (4, 0, 8)
    eng.batch_shapes = None                                          # a uniform batch: T and n of the begin
    assert eng._batch_predictive_shapes(None) == (None, 24)


def test_kernel_header_keeps_its_promises():
    """csrc/batch_forecast.hpp: on top of batch_smooth.hpp, every function with fp contract off, the draw ordinals clear of the
    others', and the existing headers untouched by it."""
    csrc = os.path.join(ROOT, "cpprob_amd", "csrc")
    text = open(os.path.join(csrc, "batch_forecast.hpp")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert code.count('#include "batch_smooth.hpp"') == 1 and code.count("#include") == 1
    assert re.search(r"kForecastDrawBase\s*=\s*1ull\s*<<\s*42", code)
    bodies = re.findall(r"\n\{\n(.*?)\n\}\n", code, re.S)
    assert len(bodies) == 4, len(bodies)
    for body in bodies:
        assert body.lstrip().startswith("#pragma clang fp contract(off)"), body[:80]
    assert re.search(r"[^_\w]fma\s*\(", code) is None
    for other in ("batch_smooth.hpp", "batch_suffstats.hpp"):
        assert "forecast" not in open(os.path.join(csrc, other)).read().lower()
    assert '#include "batch_forecast.hpp"' in open(os.path.join(csrc, "cpprob_hip.hip")).read()


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
    cpprob::gpu::options().forecast_horizon = 3;
    cpprob::gpu::options().forecast_trajectories = 5;
    std::vector<std::tuple<double>> obs{std::make_tuple(0.5), std::make_tuple(-0.5)};
    const std::vector<std::uint64_t> seeds{1, 2};
    const std::vector<cpprob::gpu::HmmTable> tables{cpprob::gpu::HmmTable{{-1.0, 1.0}, {0.9, 0.1, 0.2, 0.8}}};
    try {
        const std::vector<cpprob::gpu::Result> r = cpprob::gpu::inference_batch(cpprob::StateType::smc, model, obs, 1024, seeds);
        const std::vector<cpprob::gpu::Result> q = cpprob::gpu::hmm_table_batch(tables, {{0.5, 0.25}}, {512}, seeds);
        cpprob::gpu::HmmTableStream stream(tables, {4}, {512}, seeds);
        const std::vector<cpprob::gpu::Result> s = stream.advance({{0.25, 0.125}, {1.0}});
        return r.size() == 2 && q[0].forecast.size() == 3 && s[1].forecast_trajectories.size() == 5 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_forecast_options_compile_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """Options::forecast_horizon / ::forecast_trajectories and the entry points that read them are plain C++14 host code (the pattern
    of tests/test_batch_smooth_lag_host.py)."""
    import subprocess
    src = tmp_path / "forecast.cpp"
    src.write_text(_OPTIONS_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "forecast.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]


def test_cli_refuses_a_forecast_outside_the_batch_modes():
    """cpprob_main --forecast without a batch file ends with a message before anything touches a device."""
    import subprocess
    main = os.path.join(ROOT, "cpprob_amd", "bin", "cpprob_main")
    p = subprocess.run([main, "--smc", "--model", "hmm16", "--observes", "1", "--forecast", "3"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--forecast serves the batch modes" in p.stderr
