"""Diagonal-Gaussian vector emissions without a GPU: the entry points are declared, listed and bound, and cpprob_amd.m_step_diag on a
hand-made record."""
import os

import numpy as np
import pytest

import cpprob_amd as cp

NAMES = ["cpprob_hip_batch_begin_problems_diag", "cpprob_hip_batch_retable_diag", "cpprob_hip_batch_retable_diag_device",
         "cpprob_hip_batch_diag_stats", "cpprob_hip_batch_diag_stats_device", "cpprob_hip_batch_mstep_diag_device", "cpprob_hip_batch_copy_diag"]


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_listed_and_bound(name):
    header = open(os.path.join(os.path.dirname(cp.__file__), "..", "include", "cpprob_hip.h")).read()
    assert "int %s(cpprob_hip_ctx* ctx" % name in header and name in cp.capi.SYMBOLS
    assert getattr(cp.load_library(), name).restype is not None and hasattr(cp.Engine, name[len("cpprob_hip_"):])


def test_m_step_on_a_hand_made_record():
    """k = 2, D = 2.  State 0 has mass 4: coordinate 0 has mean 2 and variance 5 - 4 = 1, coordinate 1 has mean 0.5 and variance
    0.25 - 0.25 = 0, below the floor.  State 1 has no mass: its tables and its transition row stay."""
    M0 = np.array([[[9.0, 9.0], [7.0, -7.0]]])
    S0 = np.array([[[3.0, 3.0], [2.0, 0.5]]])
    A0 = np.array([[[0.5, 0.5], [0.9, 0.1]]])
    st = {"xi": np.zeros((1, 8, 8)), "occ": np.zeros((1, 8)), "sy": np.zeros((1, 8, 32)), "syy": np.zeros((1, 8, 32))}
    st["xi"][0, 0, :2] = [1.0, 3.0]
    st["occ"][0, 0] = 4.0
    st["sy"][0, 0, :2] = [8.0, 2.0]
    st["syy"][0, 0, :2] = [20.0, 1.0]
    M, S, A = cp.m_step_diag(st, M0, S0, A0, sigma_floor=1e-2)
    assert np.array_equal(M[0], [[2.0, 0.5], [7.0, -7.0]]) and np.array_equal(S[0], [[1.0, 1e-2], [2.0, 0.5]])
    assert np.array_equal(A[0], [[0.25, 0.75], [0.9, 0.1]])
    st["syy"][0, 0, 0] = np.nan                             # a NaN variance takes the floor
    assert cp.m_step_diag(st, M0, S0, A0, sigma_floor=1e-2)[1][0, 0, 0] == 1e-2
    for floor in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="sigma_floor"):
            cp.m_step_diag(st, M0, S0, A0, sigma_floor=floor)
