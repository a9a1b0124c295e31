"""The fitting kernels at many problems (csrc/batch_retable.hpp, batch_scale.hpp, batch_learn.hpp, batch_learn_scaled.hpp), where
the launches differ from those of the suite's batches of a few problems:

  the M-step kernels, one thread a (problem, state): 259 threads of k = 7 -- thread 256, the first of workgroup 1, is problem 36's
  state 4, and the last workgroup holds 3 live threads -- and 264 threads of k = 8, against tests/retable_ref.py, tests/scale_ref.py
  and cpprob_amd.em.m_step; one more problem's worth of every array lies behind the launch's and must stay as it was;

  the re-table kernels at B = 1366 problems of up to 70 steps: retable_grid_y's share of 4096 workgroups caps gridDim.y at 2, so
  workgroup y = 0 walks tiles 0 and 2 and y = 1 tile 1 (tests/test_fit_grid_cases_host.py) -- against a second context that BEGINS
  with the tables, every problem's rows, words, scales, results and masses;

  the learn-rows kernels on 1366 frozen streams, whose second advance of up to 70 observes starts at the unaligned row 5 under the
  same grid of 2 -- against the plain online batch of a second context.

Everything is array_equal on bits.  No Python learner runs at this size."""
import numpy as np
import pytest

import cpprob_amd as cp
import fit_grid_cases as F
import retable_ref as R
import scale_ref as S
from cpprob_amd import em
from test_gpu_batch_learn import assert_same, snapshot
from test_gpu_batch_scale import MODES, _assert_same, _dev, _observes, _readout, _seeds, _tables

pytestmark = pytest.mark.gpu

B_MANY, N = 1366, 64
POISON = -123.456


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the batch the one under test is compared with."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. the M-step kernels past their first workgroup --------------------------------------------------------------------------------
def _behind(a):
    """`a` on the device with one more problem's worth of POISON behind it."""
    return _dev(np.concatenate([a, np.full((1,) + a.shape[1:], POISON)]))


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "scaled"])
@pytest.mark.parametrize("B,k", [(37, 7), (33, 8)])
def test_mstep_kernels_past_the_first_workgroup(engine, B, k, scaled):
    import torch
    assert B * k > 256 and (B * k) % 256 in (3, 8) and (256 // k, 256 % k) == ((36, 4) if k == 7 else (32, 0))
    obs = _observes([20 + b % 5 for b in range(B)], k, 200 + k)
    means, trans, sigmas = _tables(B, k, 201 + k)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=(means, trans, sigmas) if scaled else (means, trans))
    engine.batch_run(_seeds(23, B))
    st = engine.batch_smooth_stats(obs)
    recs = np.concatenate([st["xi"].reshape(B, 64), st["occ"], st["occ_y"], st["occ_yy"]], axis=1)
    recs[1, 8:16] = 0.0                                          # a row without mass (problem 1, state 1)
    recs[2, 64] = 0.0                                            # a state without mass (problem 2, state 0)
    recs[B - 1, 8 * (k - 1):8 * k] = 0.0                         # ... and in the last workgroup: the last problem's last row
    recs[B - 1, 64 + k - 2] = 0.0                                # ... and its state k - 2
    floor = 1e-3
    d = [_behind(a) for a in ((recs, means, trans, sigmas, np.full(sigmas.shape, -7.0)) if scaled else (recs, means, trans))]
    if scaled:
        engine.batch_mstep_device(d[0], d[1], d[2], sigmas=d[3], sigma_floor=floor, log_norms=d[4])
    else:
        engine.batch_mstep_device(d[0], d[1], d[2])
    engine.sync()
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in d]
    for x in got:
        assert np.array_equal(_bits(x[B]), _bits(np.full(x.shape[1:], POISON))), "the launch wrote behind problem B - 1"
    assert np.array_equal(_bits(got[0][:B]), _bits(recs))
    for b in range(B):
        if scaled:
            wm, ws, wl, wt = S.m_step(recs[b], means[b], sigmas[b], np.full(k, -7.0), trans[b], k, floor)
            assert np.array_equal(_bits(got[3][b]), _bits(ws)) and np.array_equal(_bits(got[4][b]), _bits(wl)), b
        else:
            wm, wt = R.m_step(recs[b], means[b], trans[b], k)
        assert np.array_equal(_bits(got[1][b]), _bits(wm)) and np.array_equal(_bits(got[2][b]), _bits(wt)), b
    if scaled:
        hm, ht, hs = em.m_step(cp.capi.split_stats(recs), means, trans, sigmas, floor)
        assert np.array_equal(_bits(hs), _bits(got[3][:B]))
    else:
        hm, ht = em.m_step(cp.capi.split_stats(recs), means, trans)
    assert np.array_equal(_bits(hm), _bits(got[1][:B])) and np.array_equal(_bits(ht), _bits(got[2][:B]))
    # the zeroed rows and states kept their values, the others of the last workgroup moved
    assert np.array_equal(ht[B - 1, k - 1], trans[B - 1, k - 1]) and hm[B - 1, k - 2] == means[B - 1, k - 2]
    assert not np.array_equal(ht[B - 1], trans[B - 1]) and not np.array_equal(hm[B - 1], means[B - 1])


# ---- 2. the re-table kernels where the share of workgroups makes them stride -------------------------------------------------------------
def _retable(eng, form, tables, obs):
    sigmas = tables[2] if len(tables) > 2 else None
    if form == "host":
        eng.batch_retable(tables, obs)
    else:
        eng.batch_retable_device(_dev(tables[0]), _dev(tables[1]), _dev(np.concatenate(obs)), sigmas=None if sigmas is None else _dev(sigmas))
        eng.sync()


def _many(scaled):
    k = 8 if scaled else 5
    Ts, obs, A, Bt = F.many_problems(B_MANY, k)
    assert max(Ts) == 70 and R.grid_y(max(Ts), B_MANY) == 2 and R.grid_y(max(Ts), B_MANY - 1) == 3
    return k, Ts, obs, (A if scaled else A[:2]), (Bt if scaled else Bt[:2])


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "scaled"])
def test_retable_of_many_problems_equals_a_fresh_begin(engine, ref_engine, scaled, form):
    k, Ts, obs, A, Bt = _many(scaled)
    S2 = _seeds(900, B_MANY)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=A, **MODES["masses"])
    engine.batch_run(_seeds(5, B_MANY))
    _retable(engine, form, Bt, obs)
    assert engine.batch_retable_grid() == 2 and not engine.batch_retable_status().any()
    engine.batch_run(S2)
    ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=Bt, **MODES["masses"])
    ref_engine.batch_run(S2)
    got, want = _readout(engine, "masses", obs, scales=scaled), _readout(ref_engine, "masses", obs, scales=scaled)
    _assert_same(got, want)
    # the rows against the restatements, for the problems of every length's first occurrence and the last problem
    for b in list(range(len(F.LENGTHS))) + [B_MANY - 1]:
        rows = got["tables"][b][0]
        ref = S.rows(obs[b], Bt[0][b], Bt[2][b], k) if scaled else R.rows(obs[b], Bt[0][b], k, S.log_norm(1.0))
        assert rows.shape == (Ts[b], 8) and np.array_equal(_bits(rows), _bits(ref)), b


def test_refused_tables_among_many_problems_keep_table_a(engine, ref_engine):
    """The last problem carries a sigma the check refuses, the one before it a NaN mean: the status words name them, both keep table A
    (rows, words, scales), every other problem runs with table B."""
    k, Ts, obs, A, Bt = _many(True)
    bad = tuple(a.copy() for a in Bt)
    bad[2][B_MANY - 1, 3] = 1e-170                               # (2 pi sigma^2 underflows)
    bad[0][B_MANY - 2, 0] = np.nan
    mixed = tuple(a.copy() for a in Bt)
    for a, old in zip(mixed, A):
        a[B_MANY - 2:] = old[B_MANY - 2:]
    S2 = _seeds(901, B_MANY)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=A, **MODES["masses"])
    _retable(engine, "device", bad, obs)
    assert engine.batch_retable_grid() == 2
    assert list(engine.batch_retable_status()) == [0] * (B_MANY - 2) + [R.BAD_MEAN, S.BAD_SCALE]
    engine.batch_run(S2)
    ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=mixed, **MODES["masses"])
    ref_engine.batch_run(S2)
    _assert_same(_readout(engine, "masses", obs), _readout(ref_engine, "masses", obs))


# ---- 3. the learn-rows kernels, frozen, where they stride from an unaligned first row ------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "scaled"])
def test_frozen_learning_streams_of_many_problems_are_the_plain_online_batch(engine, ref_engine, scaled):
    k = 8 if scaled else 5
    schedule = F.learn_schedule(B_MANY)
    caps = [F.LEARN_CAP] * B_MANY
    assert R.grid_y(max(schedule[1]), B_MANY) == 2 and schedule[0][0] % R.ROWS_PER_TRIP == 5
    obs = _observes(caps, k, 301)
    tables = _tables(B_MANY, k, 302)
    if not scaled:
        tables = tables[:2]
    seeds = _seeds(77, B_MANY)
    gamma = (np.arange(F.LEARN_CAP) + 1.0) ** -0.6
    for eng in (engine, ref_engine):
        eng.batch_begin_online(cp.MODEL_HMM_TABLE, caps, N, seeds, tables=tables, keep_history=False, keep_masses=True)
    engine.batch_learn_begin(gamma, F.LEARN_CAP + 1, sigma_floor=1e-3 if scaled else None)
    lens = [0] * B_MANY
    for a, dT in enumerate(schedule):
        piece = [obs[b][lens[b]:lens[b] + dT[b]] for b in range(B_MANY)]
        engine.batch_advance_learn(piece)
        ref_engine.batch_advance(piece)
        lens = [lens[b] + dT[b] for b in range(B_MANY)]
        got, want = snapshot(engine, False, True), snapshot(ref_engine, False, True)
        assert [r.shape[0] for r in got["rows"]] == lens
        assert_same(got, want, "advance %d" % a)
        held = engine.batch_learn_tables(k, scales=True) if scaled else engine.batch_learn_tables(k)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(held[:-1], tables)) and not held[-1].any(), "advance %d: the tables moved" % a
    b = B_MANY - 1
    ref = S.rows(obs[b][:75], tables[0][b], tables[2][b], k) if scaled else R.rows(obs[b][:75], tables[0][b], k, S.log_norm(1.0))
    assert lens[b] == 75 and np.array_equal(_bits(got["rows"][b]), _bits(ref))
