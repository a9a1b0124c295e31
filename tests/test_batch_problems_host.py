"""CPU tests of the batch of problems with their own shapes (include/cpprob_hip.h: cpprob_hip_batch_problems_workspace_bytes,
cpprob_hip_batch_begin_problems): the workspace function is a pure host function, so the validation of such a batch and the
workspace it needs are checked without a GPU; cpprob::gpu::hmm_table_batch is plain C++14."""
import itertools

import numpy as np
import pytest

import cpprob_amd.capi as cp

EINVAL, EUNSUPPORTED = -1, -4


def _round(x):
    return (x + 255) // 256 * 256


def _regions(T, n, spp, keep):
    """The workspace the header documents: twelve regions, each rounded up to 256 bytes."""
    T, n = np.asarray(T, np.int64), np.asarray(n, np.int64)
    B, Tm, S = len(T), int(T.max()), int((T * n).sum())
    return [64 * B * Tm, 8 * B, 512 * B, 256 * B, 8 * B * Tm * spp, 8 * B * Tm, 4 * B * Tm, 4 * B, 16 * B, 4 * B, S if keep else 0, 4 * S if keep else 0]


def _formula(T, n, spp, keep):
    return sum(_round(r) for r in _regions(T, n, spp, keep))


def _uniform_regions(B, T, n, spp, keep):
    """tests/test_batch_host.py::_formula's regions: what cpprob_hip_batch_workspace_bytes documents."""
    return [64 * B * T, 8 * B, 512, 256 * B, 8 * B * T * spp, 8 * B * T, 4 * B * T, 4 * B, B * T * n if keep else 0, 4 * B * T * n if keep else 0]


SHAPES = [
    ([16], [1024]),                                              # B = 1
    ([1], [1]),                                                  # T = 1, n = 1
    ([16] * 7, [4096] * 7),                                      # all equal
    ([1, 2, 5, 16, 40, 128], [1, 2, 777, 1025, 4099, 8192]),     # ragged, n = 1 and n = 8192
    ([128, 1, 1, 1], [8192, 1, 8192, 1]),
    ([5, 40, 5], [8192, 8192, 8192]),
    ([3] * 1024, [512, 4096] * 512),
]


@pytest.mark.parametrize("model,rs,keep", list(itertools.product([cp.MODEL_HMM3, cp.MODEL_HMM_TABLE], [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED], [True, False])))
def test_workspace_bytes_is_the_documented_formula(model, rs, keep):
    spp = 3 if model == cp.MODEL_HMM3 else 8
    for T, n in SHAPES:
        got = cp.batch_problems_workspace_bytes(model, T, n, resampler=rs, keep_history=keep, ess_threshold=2.0)
        assert got == _formula(T, n, spp, keep), (T, n)
        # cfg.n_particles above the largest problem's count sizes LDS, not the workspace
        assert cp.batch_problems_workspace_bytes(model, T, n, max_particles=8192, resampler=rs, keep_history=keep) == got


@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
def test_equal_shapes_take_the_uniform_batchs_store(model):
    """All problems alike: the two store regions (states, ancestors) are the uniform formula's, and the whole workspace differs from
    cpprob_hip_batch_workspace_bytes by the documented extra regions alone (a table a problem, descriptors, order)."""
    spp = 3 if model == cp.MODEL_HMM3 else 8
    for B, T, n in [(1, 1, 1), (7, 5, 777), (256, 16, 1024), (1024, 16, 4096), (3, 40, 4099), (2, 128, 8192)]:
        het, uni = _regions([T] * B, [n] * B, spp, True), _uniform_regions(B, T, n, spp, True)
        assert het[10:] == uni[8:]
        got = cp.batch_problems_workspace_bytes(model, [T] * B, n)
        ref = cp.batch_workspace_bytes(model, n, B, T)
        assert got - ref == _round(512 * B) - _round(512) + _round(16 * B) + _round(4 * B)
        nokeep = cp.batch_problems_workspace_bytes(model, [T] * B, n, keep_history=False)
        assert got - nokeep == _round(B * T * n) + _round(4 * B * T * n)


def _code(**kw):
    """The arguments of tests/test_batch_host.py::_code, through the new function: four problems of 16 observes and 1024 particles."""
    args = dict(model=cp.MODEL_HMM3, n_particles=1024, n_problems=4, T=16)
    args.update(kw)
    B = args.pop("n_problems")
    T = [args.pop("T")] * B
    n = args.pop("n_particles")
    with pytest.raises(cp.CpprobHipError) as e:
        cp.batch_problems_workspace_bytes(args.pop("model"), T, [n] * B, max_particles=n, **args)
    return e.value.code


def test_workspace_bytes_rejects_bad_arguments():
    assert _code(n_problems=0) == EINVAL
    assert _code(n_particles=0) == EINVAL
    assert _code(n_particles=cp.BATCH_MAX_PARTICLES + 1) == EINVAL
    assert _code(T=0) == EINVAL
    assert _code(flags=1) == EINVAL
    assert _code(resampler=7) == EINVAL
    assert _code(model=42) == EINVAL
    assert cp.batch_problems_workspace_bytes(cp.MODEL_HMM3, [1], [cp.BATCH_MAX_PARTICLES]) > 0


def test_workspace_bytes_rejects_what_runs_on_the_single_population_path():
    assert _code(resampler=cp.RESAMPLE_MULTINOMIAL) == EUNSUPPORTED
    assert _code(ess_threshold=1.0) == EUNSUPPORTED
    assert _code(ess_threshold=0.5) == EUNSUPPORTED
    assert _code(algorithm=cp.ALG_SIS) == EUNSUPPORTED
    for m in (cp.MODEL_GAUSSIAN_UNKNOWN_MEAN, cp.MODEL_GAUSSIAN_README, cp.MODEL_LINEAR_GAUSSIAN_1D, cp.MODEL_GAUSSIAN_2D_UNKNOWN_MEAN):
        assert _code(model=m) == EUNSUPPORTED
    msg = cp.load_library().cpprob_hip_last_error(None).decode()
    assert "single-population path" in msg


def test_workspace_bytes_rejects_bad_problem_shapes():
    def code(T, n, **kw):
        with pytest.raises(cp.CpprobHipError) as e:
            cp.batch_problems_workspace_bytes(cp.MODEL_HMM_TABLE, T, n, **kw)
        return e.value.code, str(e.value)

    c, msg = code([16, 0, 16], [100, 100, 100])                      # h_T[1] = 0
    assert c == EINVAL and "problem 1" in msg
    c, msg = code([16, 16, 16], [100, 100, 0])                       # h_n[2] = 0
    assert c == EINVAL and "problem 2" in msg
    c, msg = code([16, 16, 16], [100, 101, 100], max_particles=100)  # h_n[1] > cfg.n_particles
    assert c == EINVAL and "problem 1" in msg
    c, msg = code([16, 16], [100, 8193])                             # cfg.n_particles = 8193
    assert c == EINVAL
    c, msg = code([16, 16], [100, 100], max_particles=8193)
    assert c == EINVAL
    assert code([0, 0], [100, 100])[0] == EINVAL


def test_batch_problems_symbols_are_declared_and_bound():
    L = cp.load_library()
    for s in ("cpprob_hip_batch_problems_workspace_bytes", "cpprob_hip_batch_begin_problems"):
        assert s in cp.SYMBOLS
        assert hasattr(L, s)
    assert L.cpprob_hip_abi_version() == 3


_SWEEP_TU = r"""
#include <cstdint>
#include <vector>
#include "cpprob/cpprob.hpp"

int main()
{
    const std::vector<cpprob::gpu::HmmTable> tables{{{-1.0, 1.0}, {0.7, 0.3, 0.4, 0.6}}, {{-2.0, 2.0}, {0.5, 0.5, 0.1, 0.9}}};
    const std::vector<std::vector<double>> observes{{0.5, -0.5, 0.25}};
    const std::vector<std::size_t> n{1024, 2048};
    const std::vector<std::uint64_t> seeds{1, 2};
    try {
        const std::vector<cpprob::gpu::Result> r = cpprob::gpu::hmm_table_batch(tables, observes, n, seeds);
        return r.size() == 2 ? 0 : 1;
    } catch (const std::exception&) { return 2; }
}
"""


@pytest.mark.parametrize("opt", ["-O0", "-O2"])
def test_hmm_table_batch_compiles_as_pedantic_cpp14_without_warnings(tmp_path, opt):
    """cpprob::gpu::hmm_table_batch is plain C++14 host code: a translation unit calling it compiles with -Wall -Wextra -pedantic and
    says nothing."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sweep.cpp"
    src.write_text(_SWEEP_TU)
    p = subprocess.run(["g++", opt, "-std=c++14", "-Wall", "-Wextra", "-pedantic", "-I", os.path.join(root, "include"), "-I", os.path.join(root, "cpprob_amd", "include"),
                        "-c", str(src), "-o", str(tmp_path / "sweep.o")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert p.stderr.strip() == "", p.stderr[-3000:]


def test_evidence_grid_precheck_with_the_oracle():
    """The CPU rehearsal of tests/test_gpu_batch_problems.py::test_evidence_grid_against_the_forward_recursion: the oracle in the
    GPU's place on the 64-table subgrid (every fourth spread, every second self-transition weight) with the GPU test's seeds and
    n = 2048; the mean evidence ratio lies within 4 standard errors of 1 (measured: mean 1.0054, standard error 0.0074)."""
    import test_gpu_batch_problems as G
    from oracle import oracle as O
    means, trans, obs = G.evidence_grid(32, 16)
    idx = [i * 16 + j for i in range(0, 32, 4) for j in range(0, 16, 2)]
    seeds = G._seeds(512, 31)
    log_z = []
    for b in idx:
        O.set_hmm(means[b], trans[b])
        log_z.append(O.smc(O.MODEL_HMM_TABLE, obs, 2048, int(seeds[b]), O.RESAMPLE_SYSTEMATIC, 2.0)["log_z"])
    mean, se = G.evidence_ratio_check(log_z, means[idx], trans[idx], obs)
    print("evidence ratio on the subgrid: mean %.6f, standard error %.6f" % (mean, se))
    assert abs(mean - 1.0) < 4 * se + 1e-12, (mean, se)
