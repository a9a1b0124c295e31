"""batch_csmc_kernel (csrc/batch_csmc.hpp) and what reads its rows on the device at the cases of tests/csmc_grid_cases.py: walks of up
to 1500 steps, 300 workgroups in an order that is not the identity, rows with a single non-zero mass, seeds over the whole 64 bits and
reference bytes over the whole int8 range; the backward smoother and batch_traj_stats_kernel<8> on those rows with states 5, 6 and 7
drawn; and the particle-Gibbs sweep (cpprob_amd/pgibbs.py) against the three plain references chained on the CPU.  Everything compared
is integers or sequential uncontracted IEEE operations: every comparison is array_equal."""
import time

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import csmc_grid_cases as G
import csmc_ref as CS
import trajstats_ref as TS
from cpprob_amd.gibbs import sample_tables
from test_gpu_batch_csmc import EINVAL, _rc
from test_gpu_batch_trajstats import _records

pytestmark = pytest.mark.gpu

TILE = cp.capi.TRAJ_STATS_TILE


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - t0))


def _begin(engine, case):
    k, Ts, ns, means, trans, obs, seeds, paths = case
    if len(means) == 1:                                          # a uniform batch under the shared table
        engine.set_hmm(means[0], trans[0])
        engine.batch_begin(cp.MODEL_HMM_TABLE, np.array(obs), ns[0], keep_history=False, keep_masses=True)
    else:
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans), keep_history=False, keep_masses=True)


def _run(engine, case):
    _begin(engine, case)
    engine.batch_run_conditional(case[6], case[7])


def _assert_rows(engine, case, b, what):
    rows = G.want(case, b)[0]
    got = engine.batch_masses(b)
    assert got.shape == rows.shape and np.array_equal(got, rows), "%s problem %d (T = %d, n = %d): rows differ from the reference at steps %s" % (
        what, b, case[1][b], case[2][b], np.nonzero((got != rows).any(axis=1))[0].tolist()[:16])


def _assert_rows_and_a_trajectory(engine, case, what):
    traj = engine.batch_smooth(1)[1]
    for b in range(len(case[1])):
        _assert_rows(engine, case, b, what)
        _, m, P = G.want(case, b)
        assert np.array_equal(traj[b], R.trajectories(m, P, int(case[6][b]), 1)), "%s problem %d: the backward trajectory differs from the reference's on these masses" % (what, b)
    return traj


def test_long_walks_leave_the_reference_rows_and_the_smoother_serves_them(engine):
    """LONG: the rows of every problem, then TILE + 1 backward trajectories a problem at the largest draw_index -- T = 512 from LDS,
    T = 513 and T = 1500 from global memory, on rows the conditional run wrote."""
    case = G.long_case()
    _run(engine, case)
    for b in range(len(case[1])):
        _assert_rows(engine, case, b, "LONG")
    traj = engine.batch_smooth(TILE + 1, draw_index=G.LONG_DRAW)[1]
    for b, T in enumerate(case[1]):
        want = G.trajectories(case, b, TILE + 1, G.LONG_DRAW)
        assert traj[b].shape == want.shape == (T, TILE + 1)
        assert np.array_equal(traj[b], want), "LONG problem %d (T = %d): trajectories %s differ from the reference's" % (b, T, np.nonzero((traj[b] != want).any(axis=0))[0].tolist()[:16])


def test_long_walks_statistics_are_the_references_on_the_reference_trajectories(engine):
    """LONG: batch_traj_stats_kernel<8> at k = 8 against trajstats_ref on backward_ref's trajectories of the reference masses -- not
    on batch_smooth's.  State 7 is visited: cnt[63], sy[7] and syy[7] carry numbers."""
    case = G.long_case()
    obs = case[5]
    _run(engine, case)
    got = _records(engine.batch_traj_stats(TILE + 1, G.LONG_DRAW, obs))
    assert engine.batch_traj_stats_grid() == 2
    seven = [False] * 4
    for b, T in enumerate(case[1]):
        traj = G.trajectories(case, b, TILE + 1, G.LONG_DRAW)
        want = TS.records(traj, obs[b])
        seven = [seven[0] or bool(np.any(traj == 7)), seven[1] or bool(np.any(want[:, 63] > 0)), seven[2] or bool(np.any(want[:, 79] != 0.0)), seven[3] or bool(np.any(want[:, 87] != 0.0))]
        assert np.array_equal(got[b], want), "LONG problem %d (T = %d): the records of trajectories %s differ from the reference's" % (
            b, T, np.nonzero((got[b] != want).any(axis=1))[0].tolist()[:16])
    assert all(seven), "the reference should visit state 7 and leave xi[7][7], occ_y[7] and occ_yy[7] non-zero: %s" % seven


def test_many_ragged_problems_then_reversed_lengths_then_one_problem_more(engine):
    """MANY: 300 workgroups over lengths no two neighbours share; a second batch of the same B with the lengths reversed (first[] is
    derived again after a begin); then B = 301 (the buffer of first entries grows)."""
    case = G.many_case()
    _run(engine, case)
    for b in range(G.MANY_B):
        _assert_rows(engine, case, b, "MANY")
    back = G.many_case(reverse=True)
    assert back[1] == case[1][::-1] and back[1] != case[1]
    _run(engine, back)
    for b in range(G.MANY_B):
        _assert_rows(engine, back, b, "MANY, lengths reversed,")
    more = G.many_case(G.MANY_B + 1)
    _run(engine, more)
    for b in (0, 17, 150, G.MANY_B):
        _assert_rows(engine, more, b, "MANY, B = 301,")


def test_one_hot_rows_and_starved_states(engine):
    """ONE_HOT: rows with one non-zero mass under several occupied states and occupied states of mass 0 (the case asserts both); the
    n = 1 problem's rows are one-hot at its reference path and its backward trajectory is that path."""
    case = G.one_hot_case()
    _run(engine, case)
    traj = _assert_rows_and_a_trajectory(engine, case, "ONE_HOT")
    rows = engine.batch_masses(0)
    assert case[2][0] == 1 and np.all((rows > 0).sum(axis=1) == 1) and np.array_equal(np.nonzero(rows)[1], case[7][0])
    assert np.array_equal(traj[0][:, 0], case[7][0])


def test_seeds_over_the_whole_word(engine):
    """SEEDS: a uniform batch whose Philox keys are 0, 2^64 - 1, 2^63 and 2^32."""
    case = G.seeds_case()
    assert [int(s) for s in case[6]] == [0, (1 << 64) - 1, 1 << 63, 1 << 32]
    _run(engine, case)
    _assert_rows_and_a_trajectory(engine, case, "SEEDS")
    assert not np.array_equal(engine.batch_masses(0), engine.batch_masses(1))


@pytest.mark.parametrize("k", [5, 2])
def test_device_form_takes_any_byte(engine, k):
    """BYTES: the device form on reference bytes over -128 .. 127 takes the low three bits of each and a value >= k as k - 1, as the
    header documents; the host form refuses the same values and leaves the rows."""
    import torch
    case = G.bytes_case(k)
    flat = np.concatenate(case[7])
    assert flat.dtype == np.int8
    _begin(engine, case)
    buf = torch.from_numpy(flat).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_run_conditional_device(case[6], buf)
    engine.sync()
    for b in range(len(case[1])):
        _assert_rows(engine, case, b, "BYTES, k = %d," % k)
    before = [engine.batch_masses(b) for b in range(len(case[1]))]
    assert _rc(engine, case[6], flat.astype(np.int32)) == EINVAL
    assert b"reference state" in engine.L.cpprob_hip_last_error(engine.h)
    assert all(np.array_equal(engine.batch_masses(b), before[b]) for b in range(len(case[1])))


def test_sweeps_are_the_chained_references(engine):
    """hmm_table_particle_gibbs against csmc_ref -> backward_ref.trajectories -> trajstats_ref.records -> sample_tables chained on the
    CPU: k = 8, four chains of 40, 1, 23 and 65 steps, n = 6, four sweeps.  Sweep 0's masses are the device's (an unconditional
    batch_run, checked in tests/test_gpu_batch_masses.py); every later sweep runs wholly on the CPU, on the trajectory the reference
    chain itself drew -- so the driver's two device buffers must hand sweep i what sweep i - 1 wrote."""
    k, Ts, n, sweeps = 8, [40, 1, 23, 65], 6, 4
    B = len(Ts)
    rng = np.random.default_rng(53)
    truth = 2.5 * np.arange(k) - 8.0
    obs = [truth[rng.integers(0, k, T)] + rng.standard_normal(T) for T in Ts]
    means0 = np.tile(truth, (B, 1)) + rng.uniform(-0.5, 0.5, (B, k))
    trans0 = rng.uniform(0.2, 1.0, (B, k, k))
    seeds = np.array([(5 << 50) + 11 + 7919 * b for b in range(B)], np.uint64)
    got = cp.hmm_table_particle_gibbs(engine, obs, means0, trans0, n, seeds, sweeps, np.random.default_rng(59), tau0=5.0)

    chain = np.random.default_rng(59)
    means, trans = means0.copy(), trans0.copy()
    m_hist, t_hist, path = [means.copy()], [trans.copy()], None
    visited = set()
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans), keep_history=False, keep_masses=True)
    engine.batch_run(seeds)
    first = [[[int(v) for v in row[:k]] for row in engine.batch_masses(b)] for b in range(B)]       # sweep 0's masses: the device's
    for i in range(sweeps):
        rec = np.zeros((B, 1, TS.RECORD))
        new_path = []
        for b in range(B):
            seed = int(seeds[b]) + i
            m = first[b] if i == 0 else CS.masses(R.log_likelihoods(obs[b], means[b]), R.thresholds(trans[b]), seed, n, path[b])
            x = R.trajectories(m, R.transition_masses(trans[b]), seed, 1, draw_index=i)
            new_path.append(x[:, 0])
            visited.update(int(s) for s in x[:, 0])
            rec[b] = TS.records(x, obs[b])
        path = new_path
        st = cp.capi.split_traj_stats(rec)
        means, trans = sample_tables({f: v[:, 0] for f, v in st.items()}, k, chain, tau0=5.0)
        m_hist.append(means.copy())
        t_hist.append(trans.copy())
    assert {5, 6, 7} <= visited, "the chain's trajectories should visit the states past 4: %s" % sorted(visited)
    assert got[0].shape == (sweeps + 1, B, k) and got[1].shape == (sweeps + 1, B, k, k)
    for i in range(sweeps + 1):
        assert np.array_equal(got[0][i], m_hist[i]) and np.array_equal(got[1][i], t_hist[i]), "the tables after %d sweeps differ from the reference chain's" % i
