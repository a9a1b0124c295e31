"""The Poisson fitting kernels at many problems (csrc/batch_poisson.hpp), where the launches differ from those of a few problems:

  batch_mstep_poisson_kernel, one thread a (problem, state): 259 threads of k = 7 -- thread 256, the first of workgroup 1, is problem
  36's state 4, and the last workgroup holds 3 live threads -- and 264 threads of k = 8, against tests/poisson_ref.py and
  cpprob_amd.em.m_step; one more problem's worth of every array lies behind the launch's and must stay as it was;

  batch_retable_poisson_kernel at B = 1366 problems of fit_grid_cases.many_lengths (up to 70 steps): retable_grid_y's share of 4096
  workgroups caps gridDim.y at 2, so workgroup y = 0 walks tiles 0 and 2 and y = 1 tile 1 -- every problem's rows against
  tests/poisson_ref.py, and the threshold words and the rates in force of every length's first problem and the last.

Everything is array_equal on bits."""
import numpy as np
import pytest

import cpprob_amd as cp
import fit_grid_cases as F
import poisson_ref as P
import retable_ref as R
import scale_ref as S
from cpprob_amd import em
from test_gpu_batch_poisson import _observes, _tables
from test_gpu_batch_scale import MODES, _dev, _seeds

pytestmark = pytest.mark.gpu

B_MANY, N = 1366, 64
POISON = -123.456


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _behind(a):
    """`a` on the device with one more problem's worth of POISON behind it."""
    return _dev(np.concatenate([a, np.full((1,) + a.shape[1:], POISON)]))


@pytest.mark.parametrize("B,k", [(37, 7), (33, 8)])
def test_mstep_kernel_past_the_first_workgroup(engine, B, k):
    import torch
    assert B * k > 256 and (B * k) % 256 in (3, 8) and (256 // k, 256 % k) == ((36, 4) if k == 7 else (32, 0))
    obs = _observes([20 + b % 5 for b in range(B)], 200 + k)
    rates, trans = _tables(B, k, 201 + k)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=(rates, trans), emission="poisson")
    engine.batch_run(_seeds(23, B))
    st = engine.batch_smooth_stats(obs)
    recs = np.concatenate([st["xi"].reshape(B, 64), st["occ"], st["occ_y"], st["occ_yy"]], axis=1)
    recs[1, 8:16] = 0.0                                          # a row without mass (problem 1, state 1)
    recs[2, 64] = 0.0                                            # a state without mass (problem 2, state 0)
    recs[3, 72] = 0.0                                            # a state with mass and no counts: the floor
    recs[B - 1, 8 * (k - 1):8 * k] = 0.0                         # ... and in the last workgroup: the last problem's last row
    recs[B - 1, 64 + k - 2] = 0.0                                # ... and its state k - 2
    floor = 1e-6
    d = [_behind(a) for a in (recs, rates, trans, np.full(rates.shape, -7.0))]
    engine.batch_mstep_device(d[0], d[1], d[2], emission="poisson", rate_floor=floor, log_rates=d[3])
    engine.sync()
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in d]
    for x in got:
        assert np.array_equal(_bits(x[B]), _bits(np.full(x.shape[1:], POISON))), "the launch wrote behind problem B - 1"
    assert np.array_equal(_bits(got[0][:B]), _bits(recs))
    for b in range(B):
        wr, wl, wt = P.m_step(recs[b], rates[b], np.full(k, -7.0), trans[b], k, floor)
        assert np.array_equal(_bits(got[1][b]), _bits(wr)) and np.array_equal(_bits(got[2][b]), _bits(wt)) and np.array_equal(_bits(got[3][b]), _bits(wl)), b
    hm, ht = em.m_step(cp.capi.split_stats(recs), rates, trans, emission="poisson", rate_floor=floor)
    assert np.array_equal(_bits(hm), _bits(got[1][:B])) and np.array_equal(_bits(ht), _bits(got[2][:B]))
    assert (recs[3, 64] > 0.0 and hm[3, 0] == floor) and hm[2, 0] == rates[2, 0] and got[3][2, 0] == -7.0
    assert np.array_equal(ht[B - 1, k - 1], trans[B - 1, k - 1]) and hm[B - 1, k - 2] == rates[B - 1, k - 2]
    assert not np.array_equal(ht[B - 1], trans[B - 1]) and not np.array_equal(hm[B - 1], rates[B - 1])


@pytest.mark.parametrize("form", ["host", "device"])
def test_retable_of_many_problems_writes_the_reference_rows(engine, form):
    k = 8
    Ts = F.many_lengths(B_MANY)
    assert max(Ts) == 70 and R.grid_y(max(Ts), B_MANY) == 2 and R.grid_y(max(Ts), B_MANY - 1) == 3
    assert F.tiles_walked(max(Ts), B_MANY) == [[0, 2], [1]]
    obs = _observes(Ts, 401)
    A, Bt = _tables(B_MANY, k, 402), _tables(B_MANY, k, 403)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=A, emission="poisson", **MODES["masses"])
    if form == "host":
        engine.batch_retable(Bt, obs, emission="poisson")
    else:
        engine.batch_retable_device(_dev(Bt[0]), _dev(Bt[1]), _dev(np.concatenate(obs)), emission="poisson")
        engine.sync()
    assert engine.batch_retable_grid() == 2 and not engine.batch_retable_status().any()
    for b in range(B_MANY):
        rows = engine.batch_step_tables(b)[0]
        assert rows.shape == (Ts[b], 8) and np.array_equal(_bits(rows), _bits(P.rows(obs[b], Bt[0][b], k))), b
    for b in list(range(len(F.LENGTHS))) + [B_MANY - 1]:
        assert np.array_equal(engine.batch_step_tables(b)[1], R.thresholds(Bt[1][b], k))
        rt, lr = engine.batch_copy_rates(b)
        assert np.array_equal(rt, Bt[0][b]) and np.array_equal(_bits(lr), _bits([S.table_log(r) for r in Bt[0][b]]))
    # the batch runs under the new tables
    engine.batch_run(_seeds(900, B_MANY))
    assert np.all(np.isfinite([s["log_evidence"] for s in engine.batch_results()[0]]))
