"""Gaussian-mixture vector emissions without a GPU: the entry points are declared, listed and bound; the library's table_exp and the
rows of its host begin's loops against tests/mix_ref.py, and one hand-computed two-component row; the wrappers refuse bad shapes."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import cpprob_amd as cp
import mix_ref as MR

NAMES = ["cpprob_hip_batch_begin_problems_mix", "cpprob_hip_batch_retable_mix", "cpprob_hip_batch_retable_mix_device",
         "cpprob_hip_batch_mix_stats", "cpprob_hip_batch_mix_stats_device", "cpprob_hip_batch_mstep_mix_device", "cpprob_hip_batch_copy_mix"]


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_is_declared_listed_and_bound(name):
    header = open(os.path.join(os.path.dirname(cp.__file__), "..", "include", "cpprob_hip.h")).read()
    assert "int %s(cpprob_hip_ctx* ctx" % name in header and name in cp.capi.SYMBOLS
    assert getattr(cp.load_library(), name).restype is not None and hasattr(cp.Engine, name[len("cpprob_hip_"):])


def test_exported_table_exp_is_the_restatement_and_within_an_ulp_of_the_library():
    L = cp.load_library()
    x = np.concatenate([[0.0, -1000.0, -708.3, -708.5, -745.2, -0.5 * math.log(2.0), -1e-300], -np.random.default_rng(0).uniform(0.0, 720.0, 2000)])
    got = np.array([L.cpprob_hip_table_exp(C.c_double(v)) for v in x])
    assert np.array_equal(got.view(np.uint64), np.array([MR.table_exp(v) for v in x]).view(np.uint64))
    assert got[0] == 1.0 and got[1] == 0.0 and got[3] == 0.0 and got[4] == 0.0 and got[2] > 0.0
    normal = x >= -708.39                                   # (below about -708.4 the result would be subnormal: exactly 0.0)
    assert (got[x < -708.4] == 0.0).all() and (np.abs(got[normal] - np.exp(x[normal])) <= np.spacing(np.exp(x[normal]))).all()


def _host_rows(y, W, Mu, Sg):
    y, W, Mu, Sg = [np.ascontiguousarray(a, np.float64) for a in (y, W, Mu, Sg)]
    k, M, D = Mu.shape
    out = np.zeros((len(y), 8))
    assert cp.load_library().cpprob_hip_mix_rows(y.ctypes.data, len(y), k, M, D, W.ctypes.data, Mu.ctypes.data, Sg.ctypes.data, out.ctypes.data) == 0
    return out


def test_a_hand_computed_two_component_row_and_the_host_begins_rows():
    """k = 1, M = 2, D = 1, weights (1, 3), means (0, 2), sigmas (1, 1), y = 1: both residuals are 1, lc_c = log(w_c / 4) - 0.5 (1 + ln),
    so m = lc_1, e = (exp(log(1/4) - log(3/4)), 1) and the row is lc_1 + log(1 + 1/3) = -0.5 (1 + log 2 pi)."""
    row = _host_rows([[1.0]], [[1.0, 3.0]], [[[0.0], [2.0]]], [[[1.0], [1.0]]])
    assert abs(row[0, 0] - -0.5 * (1.0 + math.log(2 * math.pi))) < 4e-16 and np.isneginf(row[0, 1:]).all()
    assert np.array_equal(row, MR.rows([[1.0]], [[1.0, 3.0]], [[[0.0], [2.0]]], [[[1.0], [1.0]]]))
    rng = np.random.default_rng(3)
    y, W, Mu, Sg = rng.normal(0, 2, (9, 5)), rng.uniform(0.1, 1, (3, 4)), rng.normal(0, 2, (3, 4, 5)), rng.uniform(0.5, 2, (3, 4, 5))
    W[1, 2], Mu[2, 0], y[4, 1] = 0.0, 400.0, np.inf         # a zero weight; a component 1000 nats below; an infinite observe
    got, lc = _host_rows(y, W, Mu, Sg), MR.components(y, W, Mu, Sg)
    assert np.array_equal(got, MR.rows(y, W, Mu, Sg)) and np.isneginf(got[4]).all() and np.isfinite(got[[0, 8], :3]).all()
    assert MR.join(lc[0, 1].tolist())[1][2] == 0.0 and lc[0, 2, 0] < lc[0, 2].max() - 1000 and MR.join(lc[0, 2].tolist())[1][0] == 0.0
    one = _host_rows(y, np.ones((3, 1)), Mu[:, :1], Sg[:, :1])        # M = 1: the diagonal family's rows
    import diag_ref as DG
    assert np.array_equal(one, DG.rows(y, Mu[:, 0], Sg[:, 0]))


def test_m_step_on_a_hand_made_record_and_bad_shapes():
    """State 0: components of mass 1 and 3 -- weights 1/4 and 3/4; component 1 has mean 2, variance 5 - 4 = 1.  A component without
    mass keeps its tables and takes the weight 0; a state without mass keeps everything."""
    W0, M0, S0, A0 = np.array([[[0.5, 0.5, 0.1], [0.2, 0.8, 0.0]]]), np.full((1, 2, 3, 1), 9.0), np.full((1, 2, 3, 1), 3.0), np.array([[[0.5, 0.5], [0.9, 0.1]]])
    st = {"xi": np.zeros((1, 8, 8)), "occ_c": np.zeros((1, 8, 8)), "sy": np.zeros((1, 8, 8, 16)), "syy": np.zeros((1, 8, 8, 16))}
    st["xi"][0, 0, :2], st["occ_c"][0, 0, :2], st["sy"][0, 0, :2, 0], st["syy"][0, 0, :2, 0] = [1.0, 3.0], [1.0, 3.0], [4.0, 6.0], [16.0, 15.0]
    W, M, S, A = cp.m_step_mix(st, W0, M0, S0, A0, sigma_floor=1e-2)
    assert np.array_equal(W[0], [[0.25, 0.75, 0.0], [0.2, 0.8, 0.0]]) and np.array_equal(M[0, :, :, 0], [[4.0, 2.0, 9.0], [9.0, 9.0, 9.0]])
    assert np.array_equal(S[0, :, :, 0], [[1e-2, 1.0, 3.0], [3.0, 3.0, 3.0]]) and np.array_equal(A[0], [[0.25, 0.75], [0.9, 0.1]])
    rec = np.concatenate([st["xi"].reshape(-1), np.zeros(24), np.concatenate([st["occ_c"][..., None], st["sy"], st["syy"]], axis=-1).reshape(-1)])
    assert all(np.array_equal(g[0], w) for g, w in zip((W, M, S, A), MR.m_step(rec, W0[0], M0[0], S0[0], A0[0], 1e-2)))
    with pytest.raises(ValueError, match="weights"):
        cp.m_step_mix(st, W0[:, :, :2], M0, S0, A0)
    with pytest.raises(ValueError, match="sigma_floor"):
        cp.m_step_mix(st, W0, M0, S0, A0, sigma_floor=0.0)
    with pytest.raises(ValueError, match="weights"):
        cp.Engine._batch_mix_tables(None, W0, M0[..., 0], S0, A0, 1)
    assert cp.load_library().cpprob_hip_mix_rows(M0.ctypes.data, 1, 2, 9, 1, W0.ctypes.data, M0.ctypes.data, S0.ctypes.data, M0.ctypes.data) == -1
