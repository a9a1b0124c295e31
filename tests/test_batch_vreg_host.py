"""Markov-switching vector regressions without a GPU: the entry points are declared, listed and bound; m_step_vreg against
tests/vreg_ref.py and against its two anchors, m_step_reg at Q = 1 and m_step_full at P = 1 with a column of ones; var_design; the
wrappers' refusals."""
import os

import numpy as np
import pytest

import cpprob_amd as cp
import vreg_ref as VR

NAMES = ["cpprob_hip_batch_begin_problems_vreg", "cpprob_hip_batch_retable_vreg", "cpprob_hip_batch_retable_vreg_device",
         "cpprob_hip_batch_vreg_stats", "cpprob_hip_batch_vreg_stats_device", "cpprob_hip_batch_mstep_vreg_device", "cpprob_hip_batch_copy_vreg"]
TRI = np.tril_indices(16)


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_listed_and_bound(name):
    header = open(os.path.join(os.path.dirname(cp.__file__), "..", "include", "cpprob_hip.h")).read()
    assert "int %s(cpprob_hip_ctx* ctx" % name in header and name in cp.capi.SYMBOLS
    assert getattr(cp.load_library(), name).restype is not None and hasattr(cp.Engine, name[len("cpprob_hip_"):])


def _stats(z, g):
    """The record's dict for one problem of two states from observes z [T, D] and marginals g [T, 2], summed t = T-1 .. 0."""
    st = {"xi": np.zeros((1, 8, 8)), "occ": np.zeros((1, 8)), "sy": np.zeros((1, 8, 16)), "syy": np.zeros((1, 8, 16, 16))}
    D = z.shape[1]
    for t in range(len(z) - 1, -1, -1):
        for s in range(2):
            st["occ"][0, s] = st["occ"][0, s] + g[t, s]
            st["sy"][0, s, :D] = st["sy"][0, s, :D] + g[t, s] * z[t]
            st["syy"][0, s, :D, :D] = st["syy"][0, s, :D, :D] + g[t, s] * np.outer(z[t], z[t])
    st["xi"][0, :2, :2] = [[1.0, 3.0], [0.0, 0.0]]
    return st


def _data(Q, P, seed=5, T=40):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (T, P))
    y = x @ rng.normal(0.0, 1.0, (P, Q)) + rng.normal(0.0, 0.3, (T, Q))
    return y, x, rng.dirichlet([1.0, 1.0], T)


@pytest.mark.parametrize("case", ["plain", "no_mass", "duplicate", "nan"])
@pytest.mark.parametrize("Q,P", [(1, 3), (2, 3), (8, 8), (15, 1)])
def test_m_step_is_the_restatement(Q, P, case):
    """plain: both states fit.  no_mass: state 1 has no visits and stays.  duplicate (P > 1): covariates 0 and 1 are one column, the
    second pivot is exactly 0.0 and both states stay, their transition rows fitted all the same.  nan: one entry of state 0's record."""
    y, x, g = _data(Q, P)
    if case == "no_mass":
        g = np.stack([np.ones(len(g)), np.zeros(len(g))], axis=1)
    if case == "duplicate" and P > 1:
        x[:, 1] = x[:, 0]
    st = _stats(np.column_stack([y, x]), g)
    if case == "nan":
        st["syy"][0, 0, Q, 0] = st["syy"][0, 0, 0, Q] = np.nan
    C0, V0, A0 = np.full((1, 2, Q, P), 9.0), np.stack([[np.eye(Q) * 3.0, np.eye(Q) * 4.0]]), np.array([[[0.5, 0.5], [0.9, 0.1]]])
    got = cp.m_step_vreg(st, C0, V0, A0, 1e-2)
    rec = np.concatenate([st["xi"].reshape(-1), st["occ"][0], np.zeros(16 + 128), st["syy"][0][:, TRI[0], TRI[1]].reshape(-1)])
    want = VR.m_step(rec, C0[0], V0[0], A0[0], 1e-2)
    assert all(np.array_equal(a[0], w) for a, w in zip(got, want)) and np.array_equal(got[2][0], [[0.25, 0.75], [0.9, 0.1]])
    kept = {"plain": [False, False], "no_mass": [False, True], "duplicate": [P > 1, P > 1], "nan": [True, False]}[case]
    assert [bool(np.array_equal(got[0][0, s], C0[0, s]) and np.array_equal(got[1][0, s], V0[0, s])) for s in range(2)] == kept
    if case == "plain":
        w = g[:, 0]
        beta = np.linalg.solve((x * w[:, None]).T @ x, (x * w[:, None]).T @ y).T
        res = y - x @ beta.T
        assert np.allclose(got[0][0, 0], beta, rtol=1e-9, atol=1e-12) and np.allclose(got[1][0, 0], (res * w[:, None]).T @ res / w.sum(), rtol=1e-8, atol=1e-12)
        assert np.array_equal(got[1][0, 0], got[1][0, 0].T)


@pytest.mark.parametrize("P", [1, 4, 15])
def test_one_response_is_the_regression_family(P):
    y, x, g = _data(1, P, seed=6)
    st = _stats(np.column_stack([y, x]), g)
    C0, S0, A0 = np.full((1, 2, P), 9.0), np.array([[3.0, 4.0]]), np.array([[[0.5, 0.5], [0.9, 0.1]]])
    reg = cp.m_step_reg(st, C0, S0, A0, 1e-2)
    got = cp.m_step_vreg(st, C0[:, :, None, :], (S0 * S0)[:, :, None, None], A0, 1e-2)
    assert np.array_equal(got[0][:, :, 0], reg[0]) and np.array_equal(np.sqrt(got[1][:, :, 0, 0]), reg[1]) and np.array_equal(got[2], reg[2])
    assert not np.array_equal(reg[0], C0)


@pytest.mark.parametrize("Q", [1, 3, 15])
def test_one_covariate_of_ones_is_the_full_family(Q):
    y, _, g = _data(Q, 1, seed=7)
    st = _stats(np.column_stack([y, np.ones(len(y))]), g)
    assert np.array_equal(st["syy"][0, :, Q, :Q], st["sy"][0, :, :Q]) and np.array_equal(st["syy"][0, :, Q, Q], st["occ"][0])
    M0, V0, A0 = np.full((1, 2, Q), 9.0), np.stack([[np.eye(Q) * 3.0, np.eye(Q) * 4.0]]), np.array([[[0.5, 0.5], [0.9, 0.1]]])
    full = cp.m_step_full(st, M0, V0, A0, 1e-2)
    got = cp.m_step_vreg(st, M0[:, :, :, None], V0, A0, 1e-2)
    assert np.array_equal(got[0][:, :, :, 0], full[0]) and np.array_equal(got[1], full[1]) and np.array_equal(got[2], full[2])
    assert not np.array_equal(full[0], M0)


def test_var_design_and_refusals():
    Y = np.arange(10.0).reshape(5, 2)
    assert np.array_equal(cp.var_design(Y, 1), [[2, 3, 1, 0, 1], [4, 5, 1, 2, 3], [6, 7, 1, 4, 5], [8, 9, 1, 6, 7]])
    assert np.array_equal(cp.var_design(Y, 2, intercept=False), [[4, 5, 2, 3, 0, 1], [6, 7, 4, 5, 2, 3], [8, 9, 6, 7, 4, 5]])
    st = {"xi": np.zeros((1, 8, 8)), "occ": np.zeros((1, 8)), "syy": np.zeros((1, 8, 16, 16))}
    with pytest.raises(ValueError, match="at most 16"):
        cp.var_design(np.zeros((9, 4)), 3)                  # (Q + P = 4 + 13)
    with pytest.raises(ValueError, match="at least 1"):
        cp.var_design(Y, 0, intercept=False)
    for Q, P in ((8, 9), (16, 1), (0, 3), (3, 0)):
        with pytest.raises(ValueError, match="at most 16"):
            cp.m_step_vreg(st, np.ones((1, 2, Q, P)), np.ones((1, 2, Q, Q)), np.ones((1, 2, 2)))
        with pytest.raises(ValueError, match="at most 16"):
            cp.hmm_vreg_em(None, [np.zeros((3, Q + P))], np.ones((1, 2, Q, P)), np.ones((1, 2, Q, Q)), np.ones((1, 2, 2)), 8, [0], 1)
    with pytest.raises(ValueError, match=r"covs \[B, k, Q, Q\]"):
        cp.m_step_vreg(st, np.ones((1, 2, 2, 3)), np.ones((1, 2, 3, 3)), np.ones((1, 2, 2)))
    for floor in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="var_floor"):
            cp.m_step_vreg(st, np.ones((1, 2, 2, 3)), np.ones((1, 2, 2, 2)), np.ones((1, 2, 2)), floor)
    L, a = cp.load_library(), np.ones(8)
    assert L.cpprob_hip_batch_begin_problems_vreg(None, None, None, None, None, 2, 1, 1, a.ctypes.data, a.ctypes.data, a.ctypes.data) == -1
    assert L.cpprob_hip_batch_mstep_vreg_device(None, a.ctypes.data, 8, a.ctypes.data, a.ctypes.data, a.ctypes.data, 1e-3) == -1
