"""Forecasts of a batch at the shapes where the loops of csrc/batch_forecast.hpp run more than once: a second trip of
batch_predictive_kernel (16501 rows against 4096 * 4 a trip, from step 0 and from the middle of the table), up to five trajectory
tiles and the 1024 of n_traj = 2^20 in batch_forecast_kernel, a horizon of 3000, the top of the draw ordinals, a uniform batch of nine
problems and an online batch asked for its new rows after every advance.  The long ragged batch (tests/batch_grid_cases.py) also gives
batch_smooth_stats_kernel a walk of 16500 steps on three workgroups.  Every test reads the grids of its call
(cpprob_hip_batch_pass_grid) and asserts the trips or tiles it is named for; where the second context runs a twin of one trip, it
asserts that too.

References: tests/forecast_ref.py and tests/suffstats_ref.py on the masses of the rows the run left, as tests/test_gpu_batch_forecast.py
and tests/test_gpu_batch_suffstats.py.  Marginals, predictive rows and trajectories are pure functions of integers and uncontracted IEEE
operations: array_equal, no tolerance.  The statistics use tests/test_gpu_batch_suffstats.py::_assert_problem's bound, unchanged."""
import time

import numpy as np
import pytest

import backward_ref as R
import batch_grid_cases as G
import cpprob_amd as cp
import forecast_ref as F
import suffstats_ref as S
from oracle import exact
from test_gpu_batch_suffstats import FIELDS, _assert_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the twins of one trip, the uniform batch and the one-shot batches an online batch is compared with."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _reference(engine, case):
    """[(m, P, thresholds)] of the problems of the batch engine has just run."""
    return [(G.masses(engine, case, b)[0], R.transition_masses(case[4][b]), R.thresholds(case[4][b])) for b in range(len(case[1]))]


@pytest.fixture(scope="module")
def long_run(engine):
    """The long ragged batch run once with its history kept, and its masses formed once.  A test begins it again (the same seeds:
    the same run) where another batch may have taken the context since."""
    case = G.long_case()
    t0 = time.perf_counter()
    G.begin(engine, case)
    engine.sync()
    t1 = time.perf_counter()
    prob = _reference(engine, case)
    print("the long batch: run %.3f s, masses %.3f s" % (t1 - t0, time.perf_counter() - t1))
    return case, prob


def _check_predictive(what, rows, prob, frm=None):
    for b, (m, P, _) in enumerate(prob):
        f = 0 if frm is None else frm[b]
        want = F.predictive_rows(m, P, f, rows.shape[1], rows.shape[2])
        assert np.array_equal(rows[b], want), "%s, problem %d (L = %d, from %d): predictive rows differ, first at row %s" % (
            what, b, len(m), f, np.flatnonzero((rows[b] != want).any(axis=1))[:1])


def _check_forecast(what, marg, traj, prob, ref_marg, ref_traj):
    H, M = marg.shape[1], traj.shape[2]
    for b, (_, P, _) in enumerate(prob):
        k = len(P)
        assert np.array_equal(marg[b, :, :k], ref_marg[b][:H]) and np.all(marg[b, :, k:] == 0.0), "%s, problem %d: marginals differ" % (what, b)
        assert np.array_equal(traj[b], ref_traj[b][:H + 1, :M]), "%s, problem %d: trajectories differ, first in column %s" % (
            what, b, np.flatnonzero((traj[b] != ref_traj[b][:H + 1, :M]).any(axis=0))[:1])


# ---- 1. predictive rows: a second trip ---------------------------------------------------------------------------------------------
def test_predictive_rows_take_a_second_trip(engine, ref_engine, long_run):
    """Problem 0 owes 16501 rows against 16384 a trip: rows 16384 .. 16500 belong to the second trip.  From a list (0, L + 1: no
    row, L, and 100 on the long problem) it owes 16401: two trips again, starting mid-table.  Row L is the forecast's row h = 1."""
    case, prob = long_run
    G.begin(engine, case)
    Ts = case[1]
    t0 = time.perf_counter()
    rows = engine.batch_predictive()
    wall = time.perf_counter() - t0
    gy, trips, owed = G.predictive_grid(Ts)
    G.pass_grid(engine, "predictive rows, %d owed, %d trip(s)" % (owed, trips), forward=0, trace=0, forecast=0, predictive=gy)
    print("predictive rows: %.3f s wall" % wall)
    assert (gy, trips, owed) == (4096, 2, 16501)
    assert rows.shape == (len(Ts), 16501, 8)
    _check_predictive("long batch", rows, prob)
    assert np.any(rows[0, 16384:] != 0.0) and np.all(rows[0, :, :G.LONG_K].sum(axis=1) > 0.99)
    frm = [100, 2, 63, 0, 0, 128, 70, 0, 3, 300, 0]
    assert [b for b in range(len(Ts)) if frm[b] == Ts[b] + 1] == [1, 8] and [b for b in range(len(Ts)) if frm[b] == Ts[b]] == [2, 5, 9]
    part = engine.batch_predictive(frm)
    gy, trips, owed = G.predictive_grid(Ts, frm)
    G.pass_grid(engine, "predictive rows from a list, %d owed, %d trip(s)" % (owed, trips), predictive=gy)
    assert (gy, trips, owed) == (4096, 2, 16401) and part.shape == (len(Ts), 16401, 8)
    _check_predictive("long batch, from a list", part, prob, frm)
    for b, T in enumerate(Ts):
        n = max(T + 1 - frm[b], 0)
        assert np.array_equal(part[b, :n], rows[b, frm[b]:T + 1]) and np.all(part[b, n:] == 0.0), "problem %d: not the rows of the call from 0" % b
    marg, _ = engine.batch_forecast(1)
    G.pass_grid(engine, "forecast, H = 1, no trajectory", forecast=1, predictive=0)
    for b, T in enumerate(Ts):
        assert np.array_equal(marg[b, 0], rows[b, T]), "problem %d: row L is not the forecast's first row" % b
    # the twin: the problems of at most 600 steps, one trip
    short = G.sub_case(case, G.SHORT)
    G.begin(ref_engine, short)
    twin = ref_engine.batch_predictive()
    gy, trips, owed = G.predictive_grid(short[1])
    G.pass_grid(ref_engine, "the twin of at most 600 steps, %d owed, %d trip(s)" % (owed, trips), predictive=gy)
    assert (gy, trips) == (151, 1)
    assert np.array_equal(twin, rows[G.SHORT, :601]), "the twin of one trip differs"
    twin = ref_engine.batch_predictive([frm[b] for b in G.SHORT])
    assert G.predictive_grid(short[1], [frm[b] for b in G.SHORT])[1] == 1
    assert np.array_equal(twin, part[G.SHORT, :601]), "the twin of one trip differs (from a list)"


# ---- 2. trajectory tiles, the horizon, the draw ordinals ---------------------------------------------------------------------------
def test_forecast_over_many_tiles(engine, long_run):
    """n_traj = 1024, 2047 and 4097 at H = 2: one, two and five tiles (the last with one trajectory) a problem."""
    case, prob = long_run
    G.begin(engine, case)
    H, top = 2, 4097
    t0 = time.perf_counter()
    ref_marg = [F.marginals(m, P, H) for m, P, _ in prob]
    ref_traj = [F.trajectories(m, thr, int(case[6][b]), H, top) for b, (m, _, thr) in enumerate(prob)]
    t1 = time.perf_counter()
    for M, tiles in ((1024, 1), (2047, 2), (4097, 5)):
        marg, traj = engine.batch_forecast(H, M)
        G.pass_grid(engine, "forecast, n_traj = %d" % M, forward=0, trace=0, forecast=1 + tiles, predictive=0)
        assert marg.shape == (len(prob), H, 8) and traj.shape == (len(prob), H + 1, M) and traj.dtype == np.int32
        _check_forecast("n_traj = %d" % M, marg, traj, prob, ref_marg, ref_traj)
    print("many tiles: references %.3f s, three calls %.3f s wall" % (t1 - t0, time.perf_counter() - t1))
    assert not np.array_equal(ref_traj[0][:, :1024], ref_traj[0][:, 1024:2048]), "two tiles of the reference are the same"


def test_long_horizon(engine, long_run):
    """H = 3000 with three trajectories: the h loops are long, the marginals are pushed 3000 times and the draw ordinal carries h up
    to 3000.  The push reaches a fixed point in floating point; the test prints at which h a problem's rows stop changing, so that the
    reader knows over how many rows the equality of the marginals says something.  The trajectories' draws differ at every h."""
    case, prob = long_run
    G.begin(engine, case)
    H, M = 3000, 3
    t0 = time.perf_counter()
    ref_marg = [F.marginals(m, P, H) for m, P, _ in prob]
    ref_traj = [F.trajectories(m, thr, int(case[6][b]), H, M) for b, (m, _, thr) in enumerate(prob)]
    t1 = time.perf_counter()
    marg, traj = engine.batch_forecast(H, M)
    wall = time.perf_counter() - t1
    G.pass_grid(engine, "forecast, H = %d" % H, forecast=2)
    print("long horizon: references %.3f s, the call %.3f s wall" % (t1 - t0, wall))
    _check_forecast("H = %d" % H, marg, traj, prob, ref_marg, ref_traj)
    moving = []
    for b, f in enumerate(ref_marg):
        same = np.all(f[1:] == f[:-1], axis=1)                           # row h + 1 == row h
        changes = np.flatnonzero(~same)
        last = int(changes[-1]) + 2 if changes.size else 1               # the last h (1-based) whose row differs from the one before
        moving.append(last)
        print("problem %d: the marginals change up to h = %d of %d%s" % (b, last, H, "" if last > H - 100 else ": a fixed point from there on"))
        assert last >= 3, "problem %d: the marginals never move" % b
    print("long horizon: a problem still changes in the last 100 rows: %s" % any(x > H - 100 for x in moving))
    for b in range(len(prob)):
        assert len(set(map(tuple, traj[b, 1:].tolist()))) >= 2, "problem %d: every simulated row is the same" % b
    assert any(np.any(traj[b, H - 100:, :] != traj[b, H - 100, :]) for b in range(len(prob))), "no trajectory moves in the last 100 rows"


def test_draw_index_reaches_bits_32_to_39(engine, long_run):
    """draw_index << 24 sets bits 32 .. 39 of the ordinal from 256 on: 255, 256 and 65535 give three different, correct results."""
    case, prob = long_run
    G.begin(engine, case)
    H, M = 3, 257
    ref_marg = [F.marginals(m, P, H) for m, P, _ in prob]
    got = {}
    t0 = time.perf_counter()
    for di in (255, 256, 65535):
        marg, got[di] = engine.batch_forecast(H, M, di)
        G.pass_grid(engine, "forecast, draw_index %d" % di, forecast=2)
        ref_traj = [F.trajectories(m, thr, int(case[6][b]), H, M, di) for b, (m, _, thr) in enumerate(prob)]
        _check_forecast("draw_index %d" % di, marg, got[di], prob, ref_marg, ref_traj)
    print("draw ordinals: %.3f s wall" % (time.perf_counter() - t0))
    for x, y in ((255, 256), (255, 65535), (256, 65535)):
        assert not np.array_equal(got[x][0], got[y][0]), "draw_index %d and %d give the same trajectories" % (x, y)


def test_largest_n_traj(engine):
    """n_traj = 2^20: 1024 tiles, the block index j >> 1 up to 2^19 - 1; the first and last columns, the tile border and 300 picked
    columns against the reference."""
    T, n, M, H, di = 2, 3, 1 << 20, 2, 65535
    obs = np.array([exact.simulate_hmm(T, 6100)])
    seeds = G._seeds(1, 409)
    engine.batch_begin(cp.MODEL_HMM3, obs, n)
    engine.batch_run(seeds)
    t0 = time.perf_counter()
    marg, traj = engine.batch_forecast(H, M, di)
    wall = time.perf_counter() - t0
    G.pass_grid(engine, "forecast, n_traj = 2^20", forecast=1 + 1024)
    print("n_traj = 2^20: %.3f s wall" % wall)
    x = traj[0]
    assert x.shape == (H + 1, M) and x.dtype == np.int32
    assert int(x.min()) >= 0 and int(x.max()) < 3, "a trajectory entry outside [0, k)"
    vals, _, _ = engine.batch_store(0)
    m = R.filtering_masses(vals, R.log_likelihoods(obs[0], exact.HMM_MEAN))
    P, thr = R.transition_masses(exact.HMM_T), R.thresholds(exact.HMM_T)
    assert np.array_equal(marg[0], F.marginals(m, P, H))
    picked = np.sort(np.random.default_rng(13).choice(M, 300, replace=False))
    cols = np.concatenate([[0, 1, 1023, 1024, M - 2, M - 1], picked])
    assert np.array_equal(x[:, cols], F.trajectories(m, thr, int(seeds[0]), H, M, di, columns=cols)), "picked columns differ from the reference"
    assert all(len(set(x[h].tolist())) >= 2 for h in range(H + 1))


# ---- 3. a uniform batch ------------------------------------------------------------------------------------------------------------
def test_uniform_hmm3_batch_of_nine(ref_engine):
    """B = 9, T = 130, n = 70 under CPPROB_HIP_MODEL_HMM3: the thresholds behind the descriptors, thr_stride = 0 read by every
    problem; forecast and predictive rows of every problem."""
    case = G.hmm3_case()
    Ts = case[1]
    t0 = time.perf_counter()
    G.begin(ref_engine, case)
    prob = _reference(ref_engine, case)
    H, M = 3, 257
    marg, traj = ref_engine.batch_forecast(H, M, 7)
    G.pass_grid(ref_engine, "HMM3, forecast", forecast=2, predictive=0)
    assert marg.shape == (9, H, 3) and traj.shape == (9, H + 1, M)
    _check_forecast("HMM3", marg, traj, prob, [F.marginals(m, P, H) for m, P, _ in prob],
                    [F.trajectories(m, thr, int(case[6][b]), H, M, 7) for b, (m, _, thr) in enumerate(prob)])
    rows = ref_engine.batch_predictive()
    gy, trips, owed = G.predictive_grid(Ts)
    G.pass_grid(ref_engine, "HMM3, predictive rows, %d owed" % owed, forecast=0, predictive=gy)
    assert (gy, trips) == (33, 1) and rows.shape == (9, 131, 3)
    _check_predictive("HMM3", rows, prob)
    frm = [0, 131, 130, 64, 65, 1, 129, 100, 7]
    part = ref_engine.batch_predictive(frm)
    G.pass_grid(ref_engine, "HMM3, predictive rows from a list", predictive=G.predictive_grid(Ts, frm)[0])
    _check_predictive("HMM3, from a list", part, prob, frm)
    print("HMM3, B = 9: %.3f s wall" % (time.perf_counter() - t0))


# ---- 4. an online batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kept", [False, True], ids=["history", "keep_masses"])
def test_online_predictive_rows_assemble(engine, ref_engine, kept):
    """The 150-step stream of tests/batch_grid_cases.py: after each advance the predictive rows are asked from the previous length
    on (its row L, final when first available, comes once more).  Assembled, they are the one call's at the end and the one-shot batch's; the forecast at the end is the one-shot batch's."""
    means, trans, obs, seeds = G.online_case()
    B, k = len(G.ONLINE_CAPS), G.ONLINE_K
    mode = dict(keep_history=False, keep_masses=True) if kept else {}
    t0 = time.perf_counter()
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, G.ONLINE_CAPS, G.ONLINE_NS, seeds, tables=(means, trans), **mode)
    lens = [0] * B
    series = np.zeros((B, max(G.ONLINE_CAPS) + 1, 8))
    first = engine.batch_predictive()
    G.pass_grid(engine, "online, no observes yet", predictive=1)
    assert first.shape == (B, 1, 8) and np.all(first[:, 0, :k] == 1.0 / k) and np.all(first[:, 0, k:] == 0.0)
    series[:, 0] = first[:, 0]
    for now in G.online_lengths():
        engine.batch_advance([obs[b][lens[b]:now[b]] for b in range(B)])
        frm = list(lens)                                                 # (row L of the last length once more: it was final then)
        lens = now
        part = engine.batch_predictive(frm)
        gy, trips, owed = G.predictive_grid(lens, frm)
        G.pass_grid(engine, "online, lengths %s, %d owed" % (lens, owed), predictive=gy)
        assert trips == 1 and part.shape == (B, owed, 8)
        for b in range(B):
            n = lens[b] + 1 - frm[b]
            assert np.array_equal(part[b, 0], series[b, frm[b]]), "problem %d at length %d: row %d changed" % (b, lens[b], frm[b])
            series[b, frm[b]:lens[b] + 1] = part[b, :n]
            assert np.all(part[b, n:] == 0.0)
    assert lens == [150, 0, 150, 150, 128, 150]
    whole = engine.batch_predictive()
    G.pass_grid(engine, "online, the one call", predictive=G.predictive_grid(lens)[0])
    marg, traj = engine.batch_forecast(3, 257, 1)
    G.pass_grid(engine, "online, forecast", forecast=2)
    print("online (%s): six advances, %.3f s wall" % ("keep_masses" if kept else "history", time.perf_counter() - t0))
    assert whole.shape == (B, 151, 8)
    for b in range(B):
        assert np.array_equal(series[b, :lens[b] + 1], whole[b, :lens[b] + 1]), "problem %d: the assembled rows are not the one call's" % b
        assert np.all(whole[b, lens[b] + 1:] == 0.0)
    assert np.all(marg[G.ONLINE_UNFED] == 0.0) and np.all(traj[G.ONLINE_UNFED] == 0)
    # the one-shot batch of the lengths reached, and the reference on its rows
    fed = [b for b in range(B) if b != G.ONLINE_UNFED]
    case = (cp.MODEL_HMM_TABLE, [lens[b] for b in fed], [G.ONLINE_NS[b] for b in fed], means[fed], trans[fed], [obs[b][:lens[b]] for b in fed], seeds[fed])
    G.begin(ref_engine, case)
    one = ref_engine.batch_predictive()
    G.pass_grid(ref_engine, "one-shot batch, predictive rows", predictive=G.predictive_grid(case[1])[0])
    one_marg, one_traj = ref_engine.batch_forecast(3, 257, 1)
    prob = _reference(ref_engine, case)
    _check_predictive("one-shot batch", one, prob)
    for i, b in enumerate(fed):
        assert np.array_equal(whole[b], one[i]), "problem %d: differs from the one-shot batch" % b
        assert np.array_equal(marg[b], one_marg[i]) and np.array_equal(traj[b], one_traj[i]), "problem %d: the forecast differs from the one-shot batch" % b


# ---- 5. the statistics kernel's long walk ------------------------------------------------------------------------------------------
def test_statistics_of_the_long_ragged_batch(engine, long_run):
    """batch_smooth_stats_kernel on three workgroups, the last with three problems: a walk of 16500 steps, and T = 1 and T = 2 among
    the rest.  The bound is tests/test_gpu_batch_suffstats.py's."""
    case, prob = long_run
    G.begin(engine, case)
    obs = case[5]
    t0 = time.perf_counter()
    stats = engine.batch_smooth_stats(obs)
    t1 = time.perf_counter()
    print("statistics: counting gridDim.y %d, the call %.3f s wall" % (engine.batch_smooth_grid()[0], t1 - t0))
    assert engine.batch_smooth_grid()[0] > 0 and engine.batch_pass_grid() == (0, 0, 0, 0)
    worst = dict((f, 0.0) for f, _ in FIELDS)
    for b, (m, P, _) in enumerate(prob):
        ref = S.stats(m, P, obs[b])
        got = {f: v[b] for f, v in stats.items()}
        _assert_problem(b, got, ref, obs[b], G.LONG_K, "long batch, ")
        for f, _ in FIELDS:
            worst[f] = max(worst[f], float(np.abs(got[f] - ref[f]).max()))
    print("statistics: references %.3f s; largest differences over the batch: %s" % (time.perf_counter() - t1, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert np.all(stats["xi"][1] == 0.0), "T = 1 has no transition"
    assert abs(stats["occ"][0].sum() - 16500.0) <= 16500 * (1e-12 + 16500 * 2.0 ** -53)
