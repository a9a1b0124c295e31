"""Categorical emissions without a GPU: the entry points are declared, listed and bound, and cpprob_amd.m_step_categorical on a
hand-made record."""
import os

import numpy as np
import pytest

import cpprob_amd as cp

NAMES = ["cpprob_hip_batch_begin_problems_categorical", "cpprob_hip_batch_retable_categorical", "cpprob_hip_batch_retable_categorical_device",
         "cpprob_hip_batch_symbol_stats", "cpprob_hip_batch_symbol_stats_device", "cpprob_hip_batch_mstep_categorical_device", "cpprob_hip_batch_copy_emission"]


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_listed_and_bound(name):
    header = open(os.path.join(os.path.dirname(cp.__file__), "..", "include", "cpprob_hip.h")).read()
    assert "int %s(cpprob_hip_ctx* ctx" % name in header and name in cp.capi.SYMBOLS
    assert getattr(cp.load_library(), name).restype is not None and hasattr(cp.Engine, name[len("cpprob_hip_"):])


def test_m_step_on_a_hand_made_record():
    """k = 2, V = 3.  State 0 saw symbols 0 and 1 with masses 3 and 1 and never symbol 2: its row is (0.75, 0.25, floor).  State 1 has
    no mass: its row and its transition row stay."""
    E0 = np.array([[[0.2, 0.3, 0.5], [0.6, 0.3, 0.1]]])
    A0 = np.array([[[0.5, 0.5], [0.9, 0.1]]])
    st = {"xi": np.zeros((1, 8, 8)), "cnt": np.zeros((1, 8, 64))}
    st["xi"][0, 0, :2] = [1.0, 3.0]
    st["cnt"][0, 0, :2] = [3.0, 1.0]
    E, A = cp.m_step_categorical(st, E0, A0, prob_floor=1e-3)
    assert np.array_equal(E[0], [[0.75, 0.25, 1e-3], [0.6, 0.3, 0.1]]) and np.array_equal(A[0], [[0.25, 0.75], [0.9, 0.1]])
    st["cnt"][0, 0, 1] = np.inf                             # tot = inf: the quotients are 0 and NaN, and both take the floor
    assert np.array_equal(cp.m_step_categorical(st, E0, A0, prob_floor=1e-3)[0][0, 0], [1e-3] * 3)
    for floor in (0.0, -1.0, np.nan, np.inf, 1e-310):
        with pytest.raises(ValueError, match="prob_floor"):
            cp.m_step_categorical(st, E0, A0, prob_floor=floor)
