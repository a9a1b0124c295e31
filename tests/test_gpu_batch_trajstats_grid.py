"""batch_traj_stats_kernel<8> (csrc/batch_trajstats.hpp) on the device where the existing suite does not take it: k = 8 (states 5, 6
and 7 drawn, the last register of each bank counted into) and k = 2, problems on both sides of the staging boundary T = 512 / 513,
full and partial last tiles, 17 tiles a problem, the largest draw_index.  The reference is tests/trajstats_ref.py applied to
tests/backward_ref.py's trajectories of the masses the run kept -- never to Engine.batch_smooth's.  Counts are integers and sums
sequential IEEE additions: every comparison is array_equal."""
import time

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import csmc_grid_cases as G
import trajstats_ref as TS
from batch_grid_cases import kept_masses
from test_gpu_batch_trajstats import _device_form, _records

pytestmark = pytest.mark.gpu

TILE = cp.capi.TRAJ_STATS_TILE
BIG = 2 * TILE + 5
DRAWS = (0, 65535)
# The trajectories the reference walks, of the BIG a call draws: both ends of every tile, both words of a Philox block on either side
# of a tile's edge, and a fixed sample of the rest -- 64 columns, so that a test holds about 130 000 reference trajectory entries.
EDGES = [0, 1, 2, 3, TILE - 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 2, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 2 * TILE + 2, 2 * TILE + 3, 2 * TILE + 4]
COLUMNS = np.array(sorted(EDGES + [int(j) for j in np.random.default_rng(5).permutation(BIG) if int(j) not in EDGES][:64 - len(EDGES)]))


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - t0))


def _begin(engine, case, **kw):
    k, Ts, ns, means, trans, obs, seeds = case
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans), **kw)
    engine.batch_run(seeds)


def _reference(engine, case, n_traj, draw_index, columns=None):
    """[B, columns, 88] and whether a trajectory visits the last state: trajstats_ref on backward_ref's trajectories of the kept masses."""
    k, Ts, ns, means, trans, obs, seeds = case
    out, last = [], False
    for b in range(len(Ts)):
        traj = R.trajectories_fast(kept_masses(engine, b, k), R.transition_masses(trans[b]), int(seeds[b]), n_traj, draw_index, columns)
        last = last or bool(np.any(traj == k - 1))
        out.append(TS.records(traj, obs[b]))
    return np.stack(out), last


def _call(engine, n_traj, draw_index, obs):
    got = _records(engine.batch_traj_stats(n_traj, draw_index, obs))
    assert engine.batch_traj_stats_grid() == -(-n_traj // TILE), "n_traj %d: %d tiles" % (n_traj, engine.batch_traj_stats_grid())
    assert got.shape == (len(obs), n_traj, TS.RECORD)
    return got


@pytest.mark.parametrize("k", [2, 8])
def test_staging_boundary_and_full_and_partial_tiles(engine, k):
    """T in {1, 2, 7, 512, 513}: 512 steps are staged in LDS, 513 read from memory.  n_traj in {1, 2 TILE (the last tile full),
    2 TILE + 5} at draw_index 0 and 65535; a trajectory's record does not depend on n_traj; the twin batch with its history gives the
    same bits."""
    case = G.stats_case(k)
    obs = case[5]
    assert COLUMNS.size <= 64 and set(EDGES) <= set(COLUMNS.tolist()) and sum(case[1]) * COLUMNS.size * len(DRAWS) <= 150000
    _begin(engine, case, keep_history=False, keep_masses=True)
    got = {}
    for d in DRAWS:
        want, last = _reference(engine, case, BIG, d, COLUMNS)
        assert last, "the reference should visit state %d" % (k - 1)
        if k == 8:
            assert np.any(want[:, :, 63] > 0) and np.any(want[:, :, 79] != 0.0) and np.any(want[:, :, 87] != 0.0)
        for n_traj in (1, 2 * TILE, BIG):
            got[n_traj, d] = rec = _call(engine, n_traj, d, obs)
            cols = COLUMNS[COLUMNS < n_traj]
            for b, T in enumerate(case[1]):
                assert np.array_equal(rec[b, cols], want[b, :cols.size]), "k = %d, draw_index %d, n_traj %d, problem %d (T = %d): the records of trajectories %s differ from the reference's" % (
                    k, d, n_traj, b, T, cols[np.nonzero((rec[b, cols] != want[b, :cols.size]).any(axis=1))[0]].tolist()[:16])
        for n_traj in (1, 2 * TILE):
            assert np.array_equal(got[n_traj, d], got[BIG, d][:, :n_traj]), "k = %d, draw_index %d: a trajectory's record depends on n_traj (%d)" % (k, d, n_traj)
    assert not np.array_equal(got[BIG, 0], got[BIG, 65535]), "another draw_index gives other records"
    _begin(engine, case, keep_history=True)
    for (n_traj, d), rec in got.items():
        assert np.array_equal(_call(engine, n_traj, d, obs), rec), "k = %d, draw_index %d, n_traj %d: the batch with its history gives other records" % (k, d, n_traj)


@pytest.mark.parametrize("k", [2, 8])
def test_seventeen_tiles_of_short_problems(engine, k):
    """T in {1, 2, 7} at n_traj = 16 TILE + 3: gridDim.y = 17, the Philox counter j >> 1 passes 2048; every trajectory against the
    reference, and the device form between guard words equal to the host call."""
    case = G.stats_case(k, short=True)
    obs = case[5]
    n_traj, d = 16 * TILE + 3, 65535
    assert sum(case[1]) * n_traj <= 150000 and (n_traj - 1) >> 1 > 2048
    _begin(engine, case, keep_history=False, keep_masses=True)
    want, last = _reference(engine, case, n_traj, d)
    assert last
    got = _call(engine, n_traj, d, obs)
    assert engine.batch_traj_stats_grid() == 17
    for b, T in enumerate(case[1]):
        assert np.array_equal(got[b], want[b]), "k = %d, problem %d (T = %d): the records of trajectories %s differ from the reference's" % (
            k, b, T, np.nonzero((got[b] != want[b]).any(axis=1))[0].tolist()[:16])
    _device_form(engine, n_traj, d, obs, got)
