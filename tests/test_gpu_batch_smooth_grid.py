"""Batch smoothing on grids where a workgroup walks several rows (csrc/batch_smooth.hpp): the counting pass in more than one round
(batch_smooth_count_kernel reuses its per-parity LDS slots from the third round on), workgroups of zero, one and several rounds in
one launch, the ranges [counted_b, L_b) of an online batch, a second trip of batch_smooth_lag_kernel, the staging boundary of
batch_smooth_kernel at 512 rows, the top of the draw ordinals and the largest n_traj.  Every test reads the grids of its launches
(cpprob_hip_batch_smooth_grid) and asserts the rounds or trips it is named for; on the second context, where the batches are cut
into chunks of at most 128 problems, it asserts that the counting grid is the largest range: one round a workgroup.

References: tests/backward_ref.py and tests/lag_ref.py on the rows the run left, as tests/test_gpu_batch_smooth_lag.py.
Trajectories array_equal.  Marginals within 1e-12 absolute where a row lies at most 65 steps from its end step, and within
T k^2 2^-52 for the walks of a longer problem (the derivation at the top of tests/test_gpu_batch_smooth.py: 3.3e-11 at T = 16500,
k = 3).  Rows whose end is the last step are array_equal to batch_smooth's, and everything is array_equal to the one-round runs."""
import time

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import lag_ref as G
from oracle import exact
from test_gpu_batch_smooth_lag import _assert_rows, _masses, _seeds, _table_observes, _tables

pytestmark = pytest.mark.gpu

RESAMPLERS = [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED]
TOL = 1e-12
CHUNK = 128
K_WAVES = 4                                   # wavefronts a workgroup: items a row of the lag grid


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the same problems in chunks of at most 128, where every workgroup of the counting pass has one round."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _walk_tol(T, k):
    """A walk of more than 65 steps: T k^2 operations of 2^-52 relative on quantities <= 1."""
    return TOL if T <= 66 else T * k * k * 2.0 ** -52


def _rounds(gy, ranges):
    """The rounds of every workgroup (problem, y) of a counting launch of gridDim.y = gy over the ranges [cfrom_b, cto_b)."""
    out = set()
    for lo, hi in ranges:
        out.update(len(range(lo + y, hi, gy)) for y in range(gy))
    return sorted(out)


def _count_grid(eng, ranges, want_gy, want_rounds, what):
    """Asserts the counting launch of eng's last smoothing call: gridDim.y and the rounds that follow from it."""
    gy, _ = eng.batch_smooth_grid()
    top = max([hi - lo for lo, hi in ranges] + [0])
    assert gy == want_gy, "%s: counting grid %d, expected %d (largest range %d)" % (what, gy, want_gy, top)
    rounds = _rounds(gy, ranges) if gy else []
    print("%s: counting grid %d over ranges up to %d rows: rounds a workgroup %s" % (what, gy, top, rounds))
    assert rounds == want_rounds, "%s: rounds %s, expected %s" % (what, rounds, want_rounds)
    return gy


def _one_round(eng, top, what):
    gy, _ = eng.batch_smooth_grid()
    assert gy == top, "%s: the reference context's counting grid is %d, its largest range %d: not one round" % (what, gy, top)


def _lag_grid(eng, items_top, want_gy, want_trips, what):
    _, gy = eng.batch_smooth_grid()
    assert gy == want_gy, "%s: lag grid %d, expected %d" % (what, gy, want_gy)
    trips = -(-items_top // (gy * K_WAVES)) if gy else 0
    print("%s: lag grid %d, %d items the longest problem: %d trip(s)" % (what, gy, items_top, trips))
    assert trips == want_trips, "%s: %d trips, expected %d" % (what, trips, want_trips)


def _rows_err(what, b, marg_b, ref_g, frm, k, tol=TOL):
    """_assert_rows without its line of output; returns the difference."""
    rows = ref_g.shape[0] - frm
    err = float(np.abs(marg_b[:rows, :k] - ref_g[frm:]).max()) if rows > 0 else 0.0
    assert err <= tol, "%s problem %d: marginals differ from the reference by %.3g (bound %.3g)" % (what, b, err, tol)
    assert np.all(marg_b[max(rows, 0):] == 0.0) and np.all(marg_b[:, k:] == 0.0), "%s problem %d: padding is not zero" % (what, b)
    return err


def _same(what, got, want):
    """(marginals, trajectories) of two calls, bit for bit."""
    assert np.array_equal(got[0], want[0]), what + ": marginals differ"
    assert len(got[1]) == len(want[1]) and all(np.array_equal(x, y) for x, y in zip(got[1], want[1])), what + ": trajectories differ"


# ---- 1. uniform batch, three rounds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rs", RESAMPLERS)
def test_uniform_batch_in_three_rounds(engine, ref_engine, rs):
    """B = 1100: gridDim.y = 8 over T = 24 rows, a workgroup counts rows y, y + 8, y + 16 (round 2 writes round 0's LDS slots);
    n = 70 leaves two of the four wavefronts without particles."""
    B, T, n, M = 1100, 24, 70, 33
    picked = [0, 1, 547, 1098, 1099]
    obs = np.array([exact.simulate_hmm(T, 2000 + b) for b in range(B)])
    seeds = _seeds(B, 5 + rs)
    engine.batch_begin(cp.MODEL_HMM3, obs, n, resampler=rs)
    engine.batch_run(seeds)
    whole = [(0, T)] * B
    lag0 = engine.batch_smooth_lag(0)
    _count_grid(engine, whole, 8, [3], "uniform, lag 0")
    _lag_grid(engine, T, T // K_WAVES, 1, "uniform, lag 0")
    full = engine.batch_smooth(M)
    _count_grid(engine, whole, 8, [3], "uniform, full")
    lag3 = engine.batch_smooth_lag(3, None, M)
    _count_grid(engine, whole, 8, [3], "uniform, lag 3")
    assert lag0[0].shape == (B, T, 3) and full[0].shape == (B, T, 3) and lag3[0].shape == (B, T, 3)
    # lag 0 is the mass table normalised row by row: every (b, t)
    top = 0.0
    for b in range(B):
        m, P = _masses(engine, b, obs[b], exact.HMM_MEAN, exact.HMM_T)
        top = max(top, _rows_err("uniform, lag 0,", b, lag0[0][b], G.fixed_lag_marginals(m, P, 0), 0, 3))
        if b in picked:
            _assert_rows("uniform, full,", b, full[0][b], R.marginals(m, P), 0, 3)
            _assert_rows("uniform, lag 3,", b, lag3[0][b], G.fixed_lag_marginals(m, P, 3), 0, 3)
            ref_x = R.trajectories_fast(m, P, int(seeds[b]), M)
            assert np.array_equal(full[1][b], ref_x), "problem %d: trajectories differ from the reference" % b
            assert np.array_equal(lag3[1][b], ref_x[T - 4:]), "problem %d: window differs from the reference" % b
            assert np.array_equal(lag3[0][b, T - 4:], full[0][b, T - 4:]), "problem %d: tail rows differ from batch_smooth's" % b
    print("uniform, lag 0: %d x %d rows against the normalised masses, largest marginal difference %.3g" % (B, T, top))
    # the same problems and seeds, one round a workgroup
    for c in range(0, B, CHUNK):
        e = min(c + CHUNK, B)
        ref_engine.batch_begin(cp.MODEL_HMM3, obs[c:e], n, resampler=rs)
        ref_engine.batch_run(seeds[c:e])
        for name, got, call in (("lag 0", lag0, lambda: ref_engine.batch_smooth_lag(0)), ("full", full, lambda: ref_engine.batch_smooth(M)),
                                ("lag 3", lag3, lambda: ref_engine.batch_smooth_lag(3, None, M))):
            want = call()
            _one_round(ref_engine, T, "uniform, %s, problems %d .. %d" % (name, c, e))
            _same("uniform, %s, problems %d .. %d against one round a workgroup" % (name, c, e), (got[0][c:e], got[1][c:e]), want)


# ---- 2. described batch, ragged rounds ---------------------------------------------------------------------------------------------
LENGTHS, COUNTS = [1, 2, 7, 9, 17, 40], [1, 3, 64, 65, 300]


def test_described_batch_with_ragged_rounds(engine, ref_engine):
    """k = 5, B = 1030: gridDim.y = 8 over lengths 1 .. 40 -- workgroups of 0, 1, 2, 3 and 5 rounds in one launch."""
    B, k, M = 1030, 5, 33
    Ts = [LENGTHS[b % 6] for b in range(B)]
    ns = [COUNTS[b % 5] for b in range(B)]
    frm = [(7 * b) % (Ts[b] + 1) for b in range(B)]                  # 0, inside, and the length itself (no rows)
    means, trans = _tables(k, B, 53)
    obs = _table_observes(means, Ts, 53)
    seeds = _seeds(B, 23)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans))
    engine.batch_run(seeds)
    whole = [(0, T) for T in Ts]
    full = engine.batch_smooth(M)
    _count_grid(engine, whole, 8, [0, 1, 2, 3, 5], "described, full")
    lag0 = engine.batch_smooth_lag(0)
    _count_grid(engine, whole, 8, [0, 1, 2, 3, 5], "described, lag 0")
    lag3 = engine.batch_smooth_lag(3, None, M)
    _count_grid(engine, whole, 8, [0, 1, 2, 3, 5], "described, lag 3")
    _lag_grid(engine, 37, 10, 1, "described, lag 3")
    lag3f = engine.batch_smooth_lag(3, frm)
    # (marginals alone: the pass owes the rows from `from` on)
    _count_grid(engine, [(f, T) for f, T in zip(frm, Ts)], 8, _rounds(8, [(f, T) for f, T in zip(frm, Ts)]), "described, lag 3 from a list")
    assert full[0].shape == (B, 40, 8) and lag3f[0].shape == (B, max(T - f for T, f in zip(Ts, frm)), 8)
    traj_of = list(range(12)) + list(range(B - 6, B))                # three problems of every length
    top = {"full": 0.0, "lag 0": 0.0, "lag 3": 0.0, "lag 3 from": 0.0}
    for b in range(B):
        m, P = _masses(engine, b, obs[b], means[b], trans[b])
        g3 = G.fixed_lag_marginals(m, P, 3)
        top["full"] = max(top["full"], _rows_err("described, full,", b, full[0][b], R.marginals(m, P), 0, k))
        top["lag 0"] = max(top["lag 0"], _rows_err("described, lag 0,", b, lag0[0][b], G.fixed_lag_marginals(m, P, 0), 0, k))
        top["lag 3"] = max(top["lag 3"], _rows_err("described, lag 3,", b, lag3[0][b], g3, 0, k))
        top["lag 3 from"] = max(top["lag 3 from"], _rows_err("described, lag 3 from %d," % frm[b], b, lag3f[0][b], g3, frm[b], k))
        W = min(4, Ts[b])
        assert np.array_equal(lag3[0][b, Ts[b] - W:Ts[b]], full[0][b, Ts[b] - W:Ts[b]]), "problem %d: tail rows differ from batch_smooth's" % b
        assert np.array_equal(lag3[1][b], full[1][b][Ts[b] - W:]), "problem %d: window differs from batch_smooth's last rows" % b
        if b in traj_of:
            assert np.array_equal(full[1][b], R.trajectories_fast(m, P, int(seeds[b]), M)), "problem %d: trajectories differ from the reference" % b
    print("described: %d problems, largest marginal differences %s" % (B, ", ".join("%s %.3g" % kv for kv in top.items())))
    for c in range(0, B, CHUNK):
        e = min(c + CHUNK, B)
        ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs[c:e], ns[c:e], tables=(means[c:e], trans[c:e]))
        ref_engine.batch_run(seeds[c:e])
        what = "described, problems %d .. %d against one round a workgroup" % (c, e)
        for name, got, call, rng in (("full", full, lambda: ref_engine.batch_smooth(M), max(Ts[c:e])), ("lag 0", lag0, lambda: ref_engine.batch_smooth_lag(0), max(Ts[c:e])),
                                     ("lag 3", lag3, lambda: ref_engine.batch_smooth_lag(3, None, M), max(Ts[c:e])),
                                     ("lag 3 from", lag3f, lambda: ref_engine.batch_smooth_lag(3, frm[c:e]), max(T - f for T, f in zip(Ts[c:e], frm[c:e])))):
            want = call()
            _one_round(ref_engine, rng, "%s, %s" % (what, name))
            rows = want[0].shape[1]
            assert np.all(got[0][c:e, rows:] == 0.0)
            _same("%s, %s" % (what, name), (got[0][c:e, :rows], got[1][c:e]), want)


# ---- 3. online batch: the ranges [counted_b, L_b) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", [(cp.MODEL_HMM_TABLE, 8), (cp.MODEL_HMM3, 3)])
def test_online_watermark_ranges(engine, ref_engine, model, k):
    """Three advances of ragged sizes: the counting pass owes [counted_b, L_b), ranges that start and end anywhere, in launches of
    zero to five rounds a workgroup; the watermark moves under batch_smooth too."""
    B, cap, lag, M = 1030, 40, 3, 33
    ns = [COUNTS[b % 5] for b in range(B)]
    final = [[40, 33, 12, 0][b % 4] for b in range(B)]
    a1 = [min([0, 1, 9, 17, 30][b % 5], final[b]) for b in range(B)]
    a2 = [min([10, 0, 3, 1, 0, 7, 2][b % 7], final[b] - a1[b]) for b in range(B)]
    a3 = [final[b] - a1[b] - a2[b] for b in range(B)]
    spp = 3 if model == cp.MODEL_HMM3 else 8
    if model == cp.MODEL_HMM3:
        tables, obs = None, [exact.simulate_hmm(cap, 3000 + b) for b in range(B)]
        means, trans = [exact.HMM_MEAN] * B, [exact.HMM_T] * B
    else:
        means, trans = _tables(k, B, 67)
        tables, obs = (means, trans), _table_observes(means, [cap] * B, 67)
    seeds = _seeds(B, 131)
    engine.batch_begin_online(model, [cap] * B, ns, seeds, tables=tables)
    lens, series = [0] * B, np.zeros((B, cap, spp))
    for a, dT in enumerate((a1, a2, a3)):
        before = list(lens)
        engine.batch_advance([obs[b][lens[b]:lens[b] + dT[b]] for b in range(B)], readout=(a != 1))
        lens = [lens[b] + dT[b] for b in range(B)]
        owed = list(zip(before, lens))
        if a == 1:                                                       # the full call counts this advance's rows; the lag call after it owes none
            mid = engine.batch_smooth(M)
            _count_grid(engine, owed, 8, _rounds(8, owed), "online, advance 1, batch_smooth")
            assert 0 in _rounds(8, owed) and 2 in _rounds(8, owed)
            owed = [(L, L) for L in lens]
        frm = [max(0, L - lag) for L in before]
        marg, _ = engine.batch_smooth_lag(lag, frm)
        want_gy = 0 if a == 1 else 8
        _count_grid(engine, owed, want_gy, _rounds(8, owed) if want_gy else [], "online, advance %d, lag %d from L_before - %d" % (a, lag, lag))
        if a != 1:
            r = _rounds(8, owed)
            assert 0 in r and 1 in r and max(r) >= 4, r
        for b in range(B):
            series[b, frm[b]:lens[b]] = marg[b, :lens[b] - frm[b]]
            assert np.all(marg[b, lens[b] - frm[b]:] == 0.0)
    assert lens == final
    whole = engine.batch_smooth_lag(lag, None, M)
    _count_grid(engine, [(L, L) for L in lens], 0, [], "online, the one call")
    full = engine.batch_smooth(M)
    for b in range(B):
        assert np.array_equal(series[b, :lens[b]], whole[0][b, :lens[b]]), "problem %d: the assembled rows are not the one call's" % b
        assert np.all(whole[0][b, lens[b]:] == 0.0) and np.all(full[0][b, lens[b]:] == 0.0)
        assert whole[1][b].shape == (min(lag + 1, lens[b]), M) and full[1][b].shape == (lens[b], M)
        # the full call between the advances saw a prefix: its masses are the rows the later calls walked
        assert mid[1][b].shape == (a1[b] + a2[b], M)
    # one-shot batches of the same problems, one round a workgroup (a length-0 problem owns nothing)
    for c in range(0, B, CHUNK):
        idx = [b for b in range(c, min(c + CHUNK, B)) if lens[b] >= 1]
        tb = None if tables is None else (means[idx], trans[idx])
        ref_engine.batch_begin_problems(model, [obs[b][:lens[b]] for b in idx], [ns[b] for b in idx], tables=tb)
        ref_engine.batch_run(seeds[idx])
        ref_w = ref_engine.batch_smooth_lag(lag, None, M)
        _one_round(ref_engine, max(lens[b] for b in idx), "online, one-shot chunk at %d, lag" % c)
        ref_f = ref_engine.batch_smooth(M)
        _one_round(ref_engine, max(lens[b] for b in idx), "online, one-shot chunk at %d, full" % c)
        for i, b in enumerate(idx):
            what = "online, problem %d" % b
            assert np.array_equal(whole[0][b, :lens[b]], ref_w[0][i, :lens[b]]), what + ": differs from the one-shot batch"
            assert np.array_equal(whole[1][b], ref_w[1][i]), what + ": window differs from the one-shot batch"
            assert np.array_equal(full[0][b, :lens[b]], ref_f[0][i, :lens[b]]) and np.array_equal(full[1][b], ref_f[1][i]), what + ": batch_smooth differs from the one-shot batch"
    # the references: three problems of every length, and the batch's last ones
    for b in list(range(12)) + list(range(B - 4, B)):
        if lens[b] == 0:
            continue
        m, P = _masses(engine, b, obs[b][:lens[b]], means[b], trans[b])
        what = "online, %s," % ("HMM3" if model == cp.MODEL_HMM3 else "table")
        _assert_rows(what + " lag 3,", b, whole[0][b, :lens[b]], G.fixed_lag_marginals(m, P, lag), 0, k)
        _assert_rows(what + " full,", b, full[0][b, :lens[b]], R.marginals(m, P), 0, k)
        ref_x = R.trajectories_fast(m, P, int(seeds[b]), M)
        assert np.array_equal(full[1][b], ref_x) and np.array_equal(whole[1][b], ref_x[lens[b] - min(lag + 1, lens[b]):]), what


# ---- 4. a second trip of the lag kernel --------------------------------------------------------------------------------------------
def test_lag_kernel_takes_a_second_trip(engine):
    """16498 end steps against 4096 * 4 a trip: rows 0 .. 113 belong to the second trip.  The counting pass runs gridDim.y = 4096,
    five rounds; batch_smooth reads its masses from global memory up to t = 16499 at the top of the draw ordinals."""
    Ts, ns, lag, M, di = [16500, 3], [5, 70], 2, 33, 65535
    obs = [exact.simulate_hmm(T, 4000 + b) for b, T in enumerate(Ts)]
    seeds = _seeds(2, 211)
    t0 = time.perf_counter()
    engine.batch_begin_problems(cp.MODEL_HMM3, obs, ns)
    engine.batch_run(seeds)
    engine.sync()
    print("a run of %d steps, n = %d: %.3f s wall" % (Ts[0], ns[0], time.perf_counter() - t0))
    marg, traj = engine.batch_smooth_lag(lag, None, M, di)
    _count_grid(engine, [(0, T) for T in Ts], 4096, [0, 1, 4, 5], "second trip, lag 2")
    _lag_grid(engine, Ts[0] - lag, 4096, 2, "second trip, lag 2")
    full_m, full_x = engine.batch_smooth(3, di)
    _count_grid(engine, [(0, T) for T in Ts], 4096, [0, 1, 4, 5], "second trip, full")
    assert engine.batch_smooth_grid()[1] == 0
    assert marg.shape == (2, Ts[0], 3)
    for b, T in enumerate(Ts):
        m, P = _masses(engine, b, obs[b], exact.HMM_MEAN, exact.HMM_T)
        _assert_rows("second trip, lag 2,", b, marg[b], G.fixed_lag_marginals(m, P, lag), 0, 3)
        ref_g = R.marginals(m, P)
        tol = _walk_tol(T, 3)
        err = _rows_err("second trip, full,", b, full_m[b], ref_g, 0, 3, tol)
        print("second trip, full, problem %d: T = %d, largest marginal difference %.3g (bound %.3g)" % (b, T, err, tol))
        W = min(lag + 1, T)
        assert np.array_equal(marg[b, T - W:T], full_m[b, T - W:T]), "problem %d: tail rows differ from batch_smooth's" % b
        ref_x = R.trajectories_fast(m, P, int(seeds[b]), M, di)
        assert traj[b].shape == (W, M) and np.array_equal(traj[b], ref_x[T - W:]), "problem %d: window differs from the reference" % b
        assert full_x[b].shape == (T, 3) and np.array_equal(full_x[b], ref_x[:, :3]), "problem %d: trajectories differ from the reference" % b


# ---- 5. the staging boundary -------------------------------------------------------------------------------------------------------
def test_staging_boundary_at_512_rows(engine):
    """A tile stages (T - lo) * 64 <= 32768 bytes of masses.  batch_smooth: T = 512 and 511 staged beside T = 513 read from memory;
    lag 511: T = 513 staged with lo = 1 and exactly 32768 bytes; lag 512: T = 513 unstaged beside two staged problems."""
    Ts, ns, M = [512, 513, 511], [3, 3, 3], 33
    obs = [exact.simulate_hmm(T, 5000 + b) for b, T in enumerate(Ts)]
    seeds = _seeds(3, 307)
    engine.batch_begin_problems(cp.MODEL_HMM3, obs, ns)
    engine.batch_run(seeds)
    full = engine.batch_smooth(M)
    _count_grid(engine, [(0, T) for T in Ts], 513, [0, 1], "staging, full")
    got = {}
    for lag in (511, 512):
        got[lag] = engine.batch_smooth_lag(lag, None, M)
        _count_grid(engine, [(0, T) for T in Ts], 513, [0, 1], "staging, lag %d" % lag)
        _lag_grid(engine, max(1, 513 - lag), 1, 1, "staging, lag %d" % lag)
    for b, T in enumerate(Ts):
        m, P = _masses(engine, b, obs[b], exact.HMM_MEAN, exact.HMM_T)
        tol = _walk_tol(T, 3)
        ref_g, ref_x = R.marginals(m, P), R.trajectories_fast(m, P, int(seeds[b]), M)
        err = _rows_err("staging, full,", b, full[0][b], ref_g, 0, 3, tol)
        print("staging, full, problem %d: T = %d, largest marginal difference %.3g (bound %.3g)" % (b, T, err, tol))
        assert np.array_equal(full[1][b], ref_x), "problem %d: trajectories differ from the reference" % b
        for lag in (511, 512):
            W = min(lag + 1, T)
            marg, traj = got[lag]
            err = _rows_err("staging, lag %d," % lag, b, marg[b], G.fixed_lag_marginals(m, P, lag), 0, 3, tol)
            print("staging, lag %d, problem %d: window of %d rows from step %d, largest marginal difference %.3g" % (lag, b, W, T - W, err))
            assert np.array_equal(marg[b, T - W:T], full[0][b, T - W:T]), "lag %d, problem %d: tail rows differ from batch_smooth's" % (lag, b)
            assert traj[b].shape == (W, M) and np.array_equal(traj[b], ref_x[T - W:]), "lag %d, problem %d: window differs from the reference" % (lag, b)
            assert np.array_equal(traj[b], full[1][b][T - W:]), "lag %d, problem %d: window differs from batch_smooth's last rows" % (lag, b)
        assert np.array_equal(got[511][1][b][-min(512, T):], got[512][1][b][-min(512, T):]), "problem %d: the two windows differ on their shared rows" % b


# ---- 6. draw ordinals and the largest n_traj ---------------------------------------------------------------------------------------
def test_draw_index_reaches_bits_32_to_39(engine):
    """draw_index << 24 sets bits 32 .. 39 of the ordinal from 256 on: 255, 256 and 65535 give three different, correct results."""
    Ts, ns, M, k = [1, 2, 7, 23], [1, 300, 777, 1025], 33, 8
    B = len(Ts)
    means, trans = _tables(k, B, 71)
    obs = _table_observes(means, Ts, 71)
    seeds = _seeds(B, 59)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans))
    engine.batch_run(seeds)
    mp = [_masses(engine, b, obs[b], means[b], trans[b]) for b in range(B)]
    got = {}
    for di in (255, 256, 65535):
        marg, got[di] = engine.batch_smooth(M, di)
        _count_grid(engine, [(0, T) for T in Ts], 23, [0, 1], "draw_index %d" % di)
        for b, (m, P) in enumerate(mp):
            _assert_rows("draw_index %d," % di, b, marg[b], R.marginals(m, P), 0, k)
            assert np.array_equal(got[di][b], R.trajectories_fast(m, P, int(seeds[b]), M, di)), "draw_index %d, problem %d: trajectories differ from the reference" % (di, b)
    for x, y in ((255, 256), (255, 65535), (256, 65535)):
        assert not np.array_equal(got[x][3], got[y][3]), "draw_index %d and %d give the same trajectories" % (x, y)


def test_largest_n_traj(engine):
    """n_traj = 2^20: 1024 tiles a problem; the first and last 2048 columns and 2048 picked ones against the reference."""
    T, n, M = 2, 3, 1 << 20
    obs = np.array([exact.simulate_hmm(T, 6000)])
    seeds = _seeds(1, 401)
    engine.batch_begin(cp.MODEL_HMM3, obs, n)
    engine.batch_run(seeds)
    marg, traj = engine.batch_smooth(M, 65535)
    _count_grid(engine, [(0, T)], T, [1], "n_traj = 2^20")
    x = traj[0]
    assert x.shape == (T, M) and x.dtype == np.int32
    assert int(x.min()) >= 0 and int(x.max()) < 3, "a trajectory entry outside [0, k)"
    m, P = _masses(engine, 0, obs[0], exact.HMM_MEAN, exact.HMM_T)
    _assert_rows("n_traj = 2^20,", 0, marg[0], R.marginals(m, P), 0, 3)
    picked = np.sort(np.random.default_rng(11).choice(M, 2048, replace=False))
    for cols in (np.arange(2048), np.arange(M - 2048, M), picked):
        ref = R.trajectories_fast(m, P, int(seeds[0]), M, 65535, columns=cols)
        assert np.array_equal(x[:, cols], ref), "columns %d .. %d differ from the reference" % (cols[0], cols[-1])
