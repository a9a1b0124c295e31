"""Forecasts of an online batch (cpprob_hip_batch_forecast, cpprob_hip_batch_predictive on a batch begun with
cpprob_hip_batch_begin_online): 9 observes fed as 9 x 1, as 4 + 5 and at once, with the history kept and with the masses kept.  The
predictive rows do not depend on the cut, the forecast after every advance is the one-shot batch's of that length, and a forecast
between two smoothing calls moves the counting watermark as one of them would."""
import numpy as np
import pytest

import cpprob_amd as cp
from oracle import exact

pytestmark = pytest.mark.gpu

L_END, H, M = 9, 3, 33
CUTS = {"9x1": [1] * 9, "4+5": [4, 5], "at once": [9]}
CAPS, NS = [9, 9, 9], [100, 3, 1025]
FED = (0, 2)                                                       # problem 1 never sees an observe


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the one-shot batches an online batch is compared with (a begin on `engine` would replace it)."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _seeds(nb, base=11):
    return np.array([base + 7919 * b for b in range(nb)], np.uint64)


def _problem(model):
    """(tables or None, observes, k)."""
    if model == cp.MODEL_HMM3:
        return None, [exact.simulate_hmm(L_END, 60 + b) for b in range(3)], 3
    rng = np.random.default_rng(41)
    k = 8
    means = np.sort(rng.uniform(-3.0, 3.0, (3, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (3, k, k))
    trans[2, 0, k - 1] = 0.0
    return (means, trans), [means[b][rng.integers(0, k, L_END)] + rng.standard_normal(L_END) for b in range(3)], k


def _mode(kept):
    return dict(keep_history=False, keep_masses=True) if kept else {}


def _one_shot(ref_engine, model, tables, obs, L):
    """(forecast marginals, trajectories, predictive rows) of the fed problems run at once at length L, their history kept."""
    idx = list(FED)
    tb = None if tables is None else (tables[0][idx], tables[1][idx])
    ref_engine.batch_begin_problems(model, [obs[b][:L] for b in idx], [NS[b] for b in idx], tables=tb)
    ref_engine.batch_run(_seeds(3)[idx])
    marg, traj = ref_engine.batch_forecast(H, M, 1)
    return marg, traj, ref_engine.batch_predictive()


@pytest.mark.parametrize("kept", [False, True], ids=["history", "keep_masses"])
@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE], ids=["hmm3", "table8"])
def test_cuts_agree_and_meet_the_one_shot_batch(engine, ref_engine, model, kept):
    tables, obs, k = _problem(model)
    final = {}
    for name, cut in CUTS.items():
        engine.batch_begin_online(model, CAPS, NS, _seeds(3), tables=tables, **_mode(kept))
        marg, traj = engine.batch_forecast(H, M, 1)                   # no observes yet: rows of zeros, and the uniform initial law
        assert np.all(marg == 0.0) and np.all(traj == 0) and traj.shape == (3, H + 1, M)
        rows = engine.batch_predictive()
        assert rows.shape[:2] == (3, 1) and np.all(rows[:, 0, :k] == 1.0 / k) and np.all(rows[:, 0, k:] == 0.0)
        L, seen = 0, None
        for dT in cut:
            engine.batch_advance([obs[b][L:L + dT] if b in FED else np.zeros(0) for b in range(3)])
            L += dT
            marg, traj = engine.batch_forecast(H, M, 1)
            rows = engine.batch_predictive()
            assert rows.shape[1] == L + 1
            ref_marg, ref_traj, ref_rows = _one_shot(ref_engine, model, tables, obs, L)
            for i, b in enumerate(FED):
                assert np.array_equal(marg[b], ref_marg[i]), "%s, length %d, problem %d: marginals" % (name, L, b)
                assert np.array_equal(traj[b], ref_traj[i]), "%s, length %d, problem %d: trajectories" % (name, L, b)
                assert np.array_equal(rows[b], ref_rows[i]), "%s, length %d, problem %d: predictive rows" % (name, L, b)
                assert np.array_equal(marg[b, 0], rows[b, L])
            # the problem still at length 0: zero forecast rows, predictive row 0 = 1 / k and nothing after it
            assert np.all(marg[1] == 0.0) and np.all(traj[1] == 0)
            assert np.all(rows[1, 0, :k] == 1.0 / k) and np.all(rows[1, 1:] == 0.0)
            # a row is final when it is first available
            if seen is not None:
                assert np.array_equal(rows[:, :seen.shape[1]], seen), "%s, length %d: an earlier row changed" % (name, L)
            seen = rows
            tail = engine.batch_predictive([max(L - 1, 0), 0, L + 1])
            assert np.array_equal(tail[0, :2], rows[0, L - 1:L + 1]) and np.all(tail[2] == 0.0) and np.array_equal(tail[1, 0], rows[1, 0])
        assert L == L_END
        final[name] = rows
    assert np.array_equal(final["9x1"], final["4+5"]) and np.array_equal(final["4+5"], final["at once"])


def _smoothing_session(engine, model, tables, obs, kept, with_forecast):
    """Advance 4, smooth, advance 5, (forecast calls,) smooth again: what the later smoothing calls return."""
    engine.batch_begin_online(model, CAPS, NS, _seeds(3), tables=tables, **_mode(kept))
    engine.batch_advance([obs[b][:4] if b in FED else np.zeros(0) for b in range(3)])
    first = engine.batch_smooth_lag(2, n_traj=5)
    engine.batch_advance([obs[b][4:9] if b in FED else np.zeros(0) for b in range(3)])
    if with_forecast:
        engine.batch_forecast(H, M)
        engine.batch_predictive([5, 0, 9])
    lag = engine.batch_smooth_lag(2, n_traj=5)
    stats = engine.batch_smooth_stats([obs[b][:9] if b in FED else np.zeros(0) for b in range(3)])
    full = engine.batch_smooth(5)
    return first, lag, stats, full


@pytest.mark.parametrize("kept", [False, True], ids=["history", "keep_masses"])
def test_forecast_between_smoothing_calls_moves_the_watermark(engine, kept):
    tables, obs, _ = _problem(cp.MODEL_HMM_TABLE)
    a = _smoothing_session(engine, cp.MODEL_HMM_TABLE, tables, obs, kept, True)
    b = _smoothing_session(engine, cp.MODEL_HMM_TABLE, tables, obs, kept, False)
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[3], b[3])):
        assert np.array_equal(x[0], y[0]) and all(np.array_equal(p, q) for p, q in zip(x[1], y[1]))
    assert all(np.array_equal(a[2][key], b[2][key]) for key in b[2])
    assert np.any(a[2]["xi"][0] > 0.0) and np.all(a[2]["xi"][1] == 0.0)
