"""CPU tests of the batched-SMC entry points (include/cpprob_hip.h: cpprob_hip_batch_*): cpprob_hip_batch_workspace_bytes is a pure
host function, so the validation of a batch configuration and the workspace it needs are checked without a GPU."""
import itertools

import pytest

import cpprob_amd.capi as cp

EINVAL, EUNSUPPORTED = -1, -4


def _round(x):
    return (x + 255) // 256 * 256


def _formula(B, T, n, spp, keep):
    """The workspace the header documents: ten regions, each rounded up to 256 bytes."""
    regions = [64 * B * T, 8 * B, 512, 256 * B, 8 * B * T * spp, 8 * B * T, 4 * B * T, 4 * B, B * T * n if keep else 0, 4 * B * T * n if keep else 0]
    return sum(_round(r) for r in regions)


def _code(**kw):
    args = dict(model=cp.MODEL_HMM3, n_particles=1024, n_problems=4, T=16)
    args.update(kw)
    with pytest.raises(cp.CpprobHipError) as e:
        cp.batch_workspace_bytes(**args)
    return e.value.code


@pytest.mark.parametrize("model,rs,keep", list(itertools.product([cp.MODEL_HMM3, cp.MODEL_HMM_TABLE], [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED], [True, False])))
def test_workspace_bytes_is_the_documented_formula(model, rs, keep):
    spp = 3 if model == cp.MODEL_HMM3 else 8
    for B, T, n in [(1, 1, 1), (256, 16, 1024), (1024, 16, 4096), (4096, 128, 8192), (7, 5, 777), (3, 40, 4099)]:
        got = cp.batch_workspace_bytes(model, n, B, T, resampler=rs, keep_history=keep, ess_threshold=2.0)
        assert got == _formula(B, T, n, spp, keep), (B, T, n)


def test_workspace_bytes_rejects_bad_arguments():
    assert _code(n_problems=0) == EINVAL
    assert _code(n_particles=0) == EINVAL
    assert _code(n_particles=cp.BATCH_MAX_PARTICLES + 1) == EINVAL
    assert _code(T=0) == EINVAL
    assert _code(flags=1) == EINVAL
    assert _code(resampler=7) == EINVAL
    assert _code(model=42) == EINVAL
    assert cp.batch_workspace_bytes(cp.MODEL_HMM3, cp.BATCH_MAX_PARTICLES, 1, 1) > 0


def test_workspace_bytes_rejects_what_runs_on_the_single_population_path():
    assert _code(resampler=cp.RESAMPLE_MULTINOMIAL) == EUNSUPPORTED
    assert _code(ess_threshold=1.0) == EUNSUPPORTED
    assert _code(ess_threshold=0.5) == EUNSUPPORTED
    assert _code(algorithm=cp.ALG_SIS) == EUNSUPPORTED
    for m in (cp.MODEL_GAUSSIAN_UNKNOWN_MEAN, cp.MODEL_GAUSSIAN_README, cp.MODEL_LINEAR_GAUSSIAN_1D, cp.MODEL_GAUSSIAN_2D_UNKNOWN_MEAN):
        assert _code(model=m) == EUNSUPPORTED
    msg = cp.load_library().cpprob_hip_last_error(None).decode()
    assert "single-population path" in msg


def test_batch_symbols_are_declared_and_bound():
    for s in ("cpprob_hip_batch_workspace_bytes", "cpprob_hip_batch_begin", "cpprob_hip_batch_run", "cpprob_hip_batch_results",
              "cpprob_hip_batch_results_device", "cpprob_hip_batch_copy_store"):
        assert s in cp.SYMBOLS
        assert hasattr(cp.load_library(), s)


_BATCH_TU = r"""
#include <cstdint>
#include <tuple>
#include <vector>
#include <boost/random/normal_distribution.hpp>
#include "cpprob/cpprob.hpp"

void model(const double& y) { cpprob::observe(boost::random::normal_distribution<>{0, 1}, y); }

int main()
{
    std::vector<std::tuple<double>> obs{std::make_tuple(0.5), std::make_tuple(-0.5)};
    const std::vector<std::uint64_t> seeds{1, 2};
    try {
        const std::vector<cpprob::gpu::Result> r = cpprob::gpu::inference_batch(cpprob::StateType::smc, model, obs, 1024, seeds);
        return r.size() == 2 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_inference_batch_compiles_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """cpprob::gpu::inference_batch is plain C++14 host code: a translation unit calling it compiles with -Wall -Wextra -pedantic and
    says nothing."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "batch.cpp"
    src.write_text(_BATCH_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "batch.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]


def test_batch_near_tie_cases_are_sharp():
    """tests/golden/near_ties_batch.json (tests/near_ties_batch.py): every case still sits at its recorded gap from a tie, and some
    rounding change of its one decision (an ulp, a non-strict compare, a contracted or unfused product) changes an oracle ancestor."""
    import collections
    import near_ties as NT
    import near_ties_batch as NB
    cases = NB.load_cases()
    cover = collections.defaultdict(set)
    for c in cases:
        assert c["n"] <= cp.BATCH_MAX_PARTICLES and c["gen"] in (0, 1) and len(c["obs"]) == NB.T
        r = NT.check_case(c)
        assert r["gap"] == c["gap"] and r["sharp"] and r["sharp"] == c["sharp"], c
        assert c["k"] == NB.POSITIONS[c["position"]]
        cover[(c["row"], c["gen"])].add(c["gap"])
    for row in ("systematic", "stratified"):
        for gen in (0, 1):
            assert cover[(row, gen)] == {-1, 0, 1}, (row, gen)
    assert {c["position"] for c in cases} == set(NB.POSITIONS)
