"""Full-covariance Gaussian vector emissions without a GPU: the entry points are declared, listed and bound; one hand-computed 2 x 2
case of the factor, a row and the M-step; a candidate that does not factor keeps its state."""
import math
import os

import numpy as np
import pytest

import cpprob_amd as cp
import full_ref as FR

NAMES = ["cpprob_hip_batch_begin_problems_full", "cpprob_hip_batch_retable_full", "cpprob_hip_batch_retable_full_device",
         "cpprob_hip_batch_full_stats", "cpprob_hip_batch_full_stats_device", "cpprob_hip_batch_mstep_full_device", "cpprob_hip_batch_copy_full"]


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_listed_and_bound(name):
    header = open(os.path.join(os.path.dirname(cp.__file__), "..", "include", "cpprob_hip.h")).read()
    assert "int %s(cpprob_hip_ctx* ctx" % name in header and name in cp.capi.SYMBOLS
    assert getattr(cp.load_library(), name).restype is not None and hasattr(cp.Engine, name[len("cpprob_hip_"):])


def _stats(occ, sy, syy):
    st = {"xi": np.zeros((1, 8, 8)), "occ": np.zeros((1, 8)), "sy": np.zeros((1, 8, 16)), "syy": np.zeros((1, 8, 16, 16))}
    st["xi"][0, 0, :2] = [1.0, 3.0]
    st["occ"][0, 0] = occ
    st["sy"][0, 0, :2] = sy
    st["syy"][0, 0, :2, :2] = syy
    return st


def test_a_hand_computed_factor_row_and_m_step():
    """cov = [[4, 2], [2, 10]] has L = [[2, 0], [1, 3]].  y - mean = (2, 7): z = (1, 2), q = 5.  State 0 has mass 4, sy = (8, 4) and
    syy = [[32, 16], [16, 44]]: mean (2, 1), c = [[8 - 4, 4 - 2], [., 11 - 1]] = cov again.  State 1 has no mass and stays."""
    cov = [[4.0, 2.0], [2.0, 10.0]]
    assert FR.factor(cov) == [[2.0, 0.0], [1.0, 3.0]] and np.array_equal(cp.full.factor(np.array([cov]))[0][0], [[2.0, 0.0], [1.0, 3.0]])
    ln = FR.log_norm(FR.factor(cov))
    assert abs(ln - math.log((2 * math.pi) ** 2 * 36.0)) < 1e-14
    row = FR.rows([[3.0, 6.0]], [[1.0, -1.0]], [cov])
    assert row[0, 0] == (5.0 + ln) * -0.5 and np.isneginf(row[0, 1:]).all()
    M0, C0 = np.array([[[9.0, 9.0], [7.0, -7.0]]]), np.array([[np.eye(2), 2 * np.eye(2)]])
    A0 = np.array([[[0.5, 0.5], [0.9, 0.1]]])
    M, C, A = cp.m_step_full(_stats(4.0, [8.0, 4.0], [[32.0, 16.0], [16.0, 44.0]]), M0, C0, A0)
    assert np.array_equal(M[0], [[2.0, 1.0], [7.0, -7.0]]) and np.array_equal(C[0], [cov, 2 * np.eye(2)])
    assert np.array_equal(A[0], [[0.25, 0.75], [0.9, 0.1]])


def test_a_candidate_that_does_not_factor_keeps_its_state():
    """Two identical observes at D = 2, weights 0.3 and 0.6.  (1, 2): every entry of the candidate is a rounding error below
    f = 1e-12, it is [[f, e], [e, f]] with |e| < f after the floor, and factors.  (1000, 2000): the rounding errors are -1.2e-10,
    -2.3e-10 and -4.7e-10, the diagonal takes f, and the second pivot f - e e / f is not positive: the state keeps mean and covariance,
    and its transition row is fitted all the same.  The restatement agrees."""
    M0, C0, A0 = np.array([[[9.0, 9.0], [7.0, -7.0]]]), np.array([[np.eye(2), 2 * np.eye(2)]]), np.array([[[0.5, 0.5], [0.9, 0.1]]])
    for scale, kept in ((1.0, False), (1000.0, True)):
        y = np.array([1.0, 2.0]) * scale
        g = [0.3, 0.6]
        sy = (0.0 + g[1] * y) + g[0] * y
        syy = (0.0 + g[1] * np.outer(y, y)) + g[0] * np.outer(y, y)
        st = _stats(g[1] + g[0], sy, syy)
        M, C, A = cp.m_step_full(st, M0, C0, A0)
        rec = np.concatenate([st["xi"].reshape(-1), st["occ"][0], np.zeros(16), st["sy"].reshape(-1), st["syy"][0][:, cp.capi._FULL_I, cp.capi._FULL_J].reshape(-1)])
        want = FR.m_step(rec, M0[0], C0[0], A0[0], 1e-6)
        assert all(np.array_equal(x[0], w) for x, w in zip((M, C, A), want))
        assert np.array_equal(A[0], [[0.25, 0.75], [0.9, 0.1]])
        assert (np.array_equal(M[0], M0[0]) and np.array_equal(C[0], C0[0])) == kept
