"""Switching-regression emissions without a GPU: the entry points are declared, listed and bound; m_step_reg against tests/reg_ref.py on
made-up records and one hand-computed fit; ar_design; the wrappers refuse P outside 1 .. 15 and the library a missing context."""
import os

import numpy as np
import pytest

import cpprob_amd as cp
import reg_ref as RR

NAMES = ["cpprob_hip_batch_begin_problems_reg", "cpprob_hip_batch_retable_reg", "cpprob_hip_batch_retable_reg_device",
         "cpprob_hip_batch_reg_stats", "cpprob_hip_batch_reg_stats_device", "cpprob_hip_batch_mstep_reg_device", "cpprob_hip_batch_copy_reg"]
TRI = np.tril_indices(16)


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_listed_and_bound(name):
    header = open(os.path.join(os.path.dirname(cp.__file__), "..", "include", "cpprob_hip.h")).read()
    assert "int %s(cpprob_hip_ctx* ctx" % name in header and name in cp.capi.SYMBOLS
    assert getattr(cp.load_library(), name).restype is not None and hasattr(cp.Engine, name[len("cpprob_hip_"):])


def _stats(z, g):
    """The record's dict for one problem of two states from observes z [T, 1 + P] and marginals g [T, 2], summed t = T-1 .. 0."""
    st = {"xi": np.zeros((1, 8, 8)), "occ": np.zeros((1, 8)), "syy": np.zeros((1, 8, 16, 16))}
    D = z.shape[1]
    for t in range(len(z) - 1, -1, -1):
        for s in range(2):
            st["occ"][0, s] = st["occ"][0, s] + g[t, s]
            st["syy"][0, s, :D, :D] = st["syy"][0, s, :D, :D] + g[t, s] * np.outer(z[t], z[t])
    st["xi"][0, :2, :2] = [[1.0, 3.0], [0.0, 0.0]]
    return st


@pytest.mark.parametrize("case", ["plain", "no_mass", "duplicate", "below_floor"])
def test_m_step_is_the_restatement(case):
    """plain: both states fit.  no_mass: state 1 has no visits and stays.  duplicate: covariates 1 and 2 are one column, the second
    pivot is exactly 0.0 and both states stay, their transition rows fitted all the same.  below_floor: y = 2 x exactly, the residual
    variance is a rounding error and the sigma takes the floor."""
    rng = np.random.default_rng(5)
    x = rng.normal(0.0, 1.0, (9, 3))
    y = x @ [1.0, -2.0, 0.5] + rng.normal(0.0, 0.3, 9)
    g = rng.dirichlet([1.0, 1.0], 9)
    if case == "no_mass":
        g = np.stack([np.ones(9), np.zeros(9)], axis=1)
    if case == "duplicate":
        x[:, 2] = x[:, 1]
    if case == "below_floor":
        x, y = x[:, :1], 2.0 * x[:, 0]
    P = x.shape[1]
    st = _stats(np.column_stack([y, x]), g)
    C0, S0, A0 = np.full((1, 2, P), 9.0), np.array([[3.0, 4.0]]), np.array([[[0.5, 0.5], [0.9, 0.1]]])
    Cf, Sg, A = cp.m_step_reg(st, C0, S0, A0, 1e-2)
    rec = np.concatenate([st["xi"].reshape(-1), st["occ"][0], np.zeros(16 + 128), st["syy"][0][:, TRI[0], TRI[1]].reshape(-1)])
    want = RR.m_step(rec, C0[0], S0[0], A0[0], 1e-2)
    assert np.array_equal(Cf[0], want[0]) and np.array_equal(Sg[0], want[1]) and np.array_equal(A[0], want[3])
    assert np.array_equal(A[0], [[0.25, 0.75], [0.9, 0.1]])
    kept = {"plain": [False, False], "no_mass": [False, True], "duplicate": [True, True], "below_floor": [False, False]}[case]
    assert [bool(np.array_equal(Cf[0, s], C0[0, s]) and Sg[0, s] == S0[0, s]) for s in range(2)] == kept
    if case == "plain":
        w = g[:, 0]
        beta = np.linalg.solve((x * w[:, None]).T @ x, (x * w[:, None]).T @ y)
        assert np.allclose(Cf[0, 0], beta, rtol=1e-10) and abs(Sg[0, 0] ** 2 - (w * (y - x @ beta) ** 2).sum() / w.sum()) < 1e-12
    if case == "below_floor":
        assert np.allclose(Cf[0, :, 0], 2.0, rtol=1e-14) and np.array_equal(Sg[0], [1e-2, 1e-2])


def test_ar_design_and_refusals():
    y = np.arange(6.0)
    assert np.array_equal(cp.ar_design(y, 2), [[2, 1, 1, 0], [3, 1, 2, 1], [4, 1, 3, 2], [5, 1, 4, 3]])
    assert np.array_equal(cp.ar_design(y, 1, intercept=False), [[1, 0], [2, 1], [3, 2], [4, 3], [5, 4]])
    st = {"xi": np.zeros((1, 8, 8)), "occ": np.zeros((1, 8)), "syy": np.zeros((1, 8, 16, 16))}
    for P in (0, 16):
        with pytest.raises(ValueError, match="1 .. 15"):
            cp.m_step_reg(st, np.ones((1, 2, P)), np.ones((1, 2)), np.ones((1, 2, 2)))
        with pytest.raises(ValueError, match="1 .. 15"):
            cp.hmm_reg_em(None, [np.zeros((3, 1 + P))], np.ones((1, 2, P)), np.ones((1, 2)), np.ones((1, 2, 2)), 8, [0], 1)
    L, a = cp.load_library(), np.ones(8)
    assert L.cpprob_hip_batch_begin_problems_reg(None, None, None, None, None, 2, 1, a.ctypes.data, a.ctypes.data, a.ctypes.data) == -1
    assert L.cpprob_hip_batch_mstep_reg_device(None, a.ctypes.data, 8, a.ctypes.data, a.ctypes.data, a.ctypes.data, None, 1e-3) == -1
