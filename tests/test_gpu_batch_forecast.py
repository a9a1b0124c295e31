"""Forecasts of a batch (include/cpprob_hip.h: cpprob_hip_batch_forecast, _forecast_device, cpprob_hip_batch_predictive,
_predictive_device; csrc/batch_forecast.hpp) against the plain-Python restatement of their arithmetic (tests/forecast_ref.py) on the
masses formed from the rows the run left (cpprob_hip_batch_copy_store), as tests/test_gpu_batch_smooth.py forms them.  Marginals,
predictive rows and trajectories are pure functions of integers and uncontracted IEEE operations: array_equal."""
import ctypes as C

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import forecast_ref as F
from oracle import exact

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
H_MAX, M_MAX = 40, 1025
HS, MS = (1, 3, 40), (0, 1, 257, 1025)


def _seeds(nb, base=77):
    return np.array([base + 7919 * b for b in range(nb)], np.uint64)


def _tables(k, nb, seed):
    """tests/test_gpu_batch_problems.py::_tables: table 1 has a zero transition entry."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (nb, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (nb, k, k))
    if nb > 1:
        trans[1, 0, k - 1] = 0.0
    return means, trans


def _table_observes(means, Ts, seed):
    rng = np.random.default_rng(seed)
    k = means.shape[1]
    return [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]


def _case(name):
    """(model, Ts, ns, means [B, k], trans [B, k, k], observes, seeds)."""
    if name == "hmm3":
        B, T = 3, 5
        return (cp.MODEL_HMM3, [T] * B, [100] * B, np.array([exact.HMM_MEAN] * B), np.array([exact.HMM_T] * B),
                [exact.simulate_hmm(T, 900 + b) for b in range(B)], _seeds(B, 3))
    k = int(name[5:])
    Ts, ns = [1, 4, 9], [1, 100, 1025]
    means, trans = _tables(k, 3, 31 + k)
    return cp.MODEL_HMM_TABLE, Ts, ns, means, trans, _table_observes(means, Ts, 31 + k), _seeds(3, 19 + k)


def _begin(engine, case, **kw):
    model, Ts, ns, means, trans, obs, seeds = case
    if model == cp.MODEL_HMM3:
        engine.batch_begin(model, np.array(obs), ns[0], **kw)
    else:
        engine.batch_begin_problems(model, obs, ns, tables=(means, trans), **kw)
    engine.batch_run(seeds)


def _masses(engine, case):
    """[(m, P, thresholds)] of the problems from the rows the run left."""
    _, Ts, _, means, trans, obs, _ = case
    out = []
    for b in range(len(Ts)):
        vals, _, logw = engine.batch_store(b)
        ll = R.log_likelihoods(obs[b], means[b])
        assert np.all(logw == np.array(ll[-1])[vals[-1]]), "problem %d: restated log-likelihoods differ from the run's table" % b
        out.append((R.filtering_masses(vals, ll), R.transition_masses(trans[b]), R.thresholds(trans[b])))
    return out


@pytest.fixture(scope="module", params=["hmm3", "table2", "table8"])
def ran(request, engine):
    """The batch run with its history kept, and the reference of every call computed once: marginals [B, 40, k], predictive rows
    (a list of [L_b + 1, k]) and trajectories [B, 41, 1025] at draw_index 0 (smaller calls are their leading rows and columns)."""
    case = _case(request.param)
    _begin(engine, case)
    prob = _masses(engine, case)
    seeds = case[6]
    ref = {"marg": [F.marginals(m, P, H_MAX) for m, P, _ in prob], "pred": [F.predictive(m, P) for m, P, _ in prob],
           "traj": [F.trajectories(m, thr, int(seeds[b]), H_MAX, M_MAX) for b, (m, _, thr) in enumerate(prob)], "prob": prob}
    return case, ref


def _k(case):
    return case[3].shape[1]


def test_marginals_and_trajectories_are_the_references(engine, ran):
    case, ref = ran
    _begin(engine, case)
    B, k = len(case[1]), _k(case)
    spp = 3 if case[0] == cp.MODEL_HMM3 else 8
    for H in HS:
        for M in MS:
            marg, traj = engine.batch_forecast(H, M)
            assert marg.shape == (B, H, spp) and traj.shape == (B, H + 1, M) and traj.dtype == np.int32
            for b in range(B):
                assert np.array_equal(marg[b, :, :k], ref["marg"][b][:H]), "H = %d, problem %d: marginals differ by %.3g" % (
                    H, b, np.abs(marg[b, :, :k] - ref["marg"][b][:H]).max())
                assert np.all(marg[b, :, k:] == 0.0)
                assert np.array_equal(traj[b], ref["traj"][b][:H + 1, :M]), "H = %d, M = %d, problem %d: trajectories differ" % (H, M, b)
    if case[0] == cp.MODEL_HMM_TABLE:                              # table 1: P[0][k-1] = 0 is never taken
        t = engine.batch_forecast(H_MAX, M_MAX)[1][1]
        assert np.any(t[:-1] == 0) and not np.any((t[:-1] == 0) & (t[1:] == k - 1))


def test_predictive_rows_are_the_references(engine, ran):
    case, ref = ran
    _begin(engine, case)
    Ts, k = case[1], _k(case)
    B = len(Ts)
    rows = engine.batch_predictive()
    assert rows.shape == (B, max(Ts) + 1, 3 if case[0] == cp.MODEL_HMM3 else 8)
    for b in range(B):
        assert np.array_equal(rows[b, :Ts[b] + 1, :k], ref["pred"][b]), "problem %d" % b
        assert np.all(rows[b, Ts[b] + 1:] == 0.0) and np.all(rows[b, :, k:] == 0.0)
        assert np.all(rows[b, 0, :k] == 1.0 / k)
    frm = [min(T + 1, f) for T, f in zip(Ts, (2, 0, 4))]            # (problem 0 of the tables: from = L + 1, no row)
    part = engine.batch_predictive(frm)
    assert part.shape[1] == max(T + 1 - f for T, f in zip(Ts, frm))
    for b in range(B):
        m, P, _ = ref["prob"][b]
        assert np.array_equal(part[b], F.predictive_rows(m, P, frm[b], part.shape[1], part.shape[2])), "from_steps, problem %d" % b
    # row h = 1 of the forecast is predictive row L; the smoother's last marginal row is the f_0 the restatement starts from
    marg, _ = engine.batch_forecast(1)
    smooth, _ = engine.batch_smooth(0)
    for b in range(B):
        assert np.array_equal(marg[b, 0], rows[b, Ts[b]])
        assert np.array_equal(smooth[b, Ts[b] - 1, :k], np.array(F.start(ref["prob"][b][0][-1])))
    ll = cp.predictive_log_likelihood(rows[B - 1], case[3][B - 1], case[5][B - 1])
    assert ll.shape == (Ts[B - 1],) and np.all(np.isfinite(ll))


def test_draw_index_device_forms_and_untouched_results(engine, ran):
    import torch
    case, ref = ran
    _begin(engine, case)
    B = len(case[1])
    H, M = 3, 257
    before = (engine.batch_results(), engine.batch_smooth(33), engine.batch_smooth_stats(case[5]))
    marg0, traj0 = engine.batch_forecast(H, M, 0)
    marg5, traj5 = engine.batch_forecast(H, M, 5)
    _, again = engine.batch_forecast(H, M, 5)
    assert np.array_equal(marg0, marg5) and not np.array_equal(traj0, traj5) and np.array_equal(traj5, again)
    for b, (m, _, thr) in enumerate(ref["prob"]):
        assert np.array_equal(traj5[b], F.trajectories(m, thr, int(case[6][b]), H, M, 5)), "draw_index 5, problem %d" % b
    rows = engine.batch_predictive()
    # the outputs alone
    only = np.full(traj5.size, -5, np.int32)
    assert engine.L.cpprob_hip_batch_forecast(engine.h, H, M, 5, None, 0, only.ctypes.data, only.size) == 0
    assert np.array_equal(only.reshape(traj5.shape), traj5)
    only_m = np.full(marg0.size, -5.0)
    assert engine.L.cpprob_hip_batch_forecast(engine.h, H, 0, 0, only_m.ctypes.data, only_m.size, None, 0) == 0
    assert np.array_equal(only_m.reshape(marg0.shape), marg0)
    # the device forms, behind guard bands
    pad = 256
    d_traj = torch.full((traj5.size + 2 * pad,), -9, dtype=torch.int8, device="cuda:0")
    d_marg = torch.full((marg0.size + 2 * pad,), 12345.5, dtype=torch.float64, device="cuda:0")
    d_rows = torch.full((rows.size + 2 * pad,), 12345.5, dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_forecast_device(H, d_marg[pad:pad + marg0.size], d_traj[pad:pad + traj5.size], n_traj=M, draw_index=5)
    engine.batch_predictive_device(d_rows[pad:pad + rows.size].view(rows.shape))
    engine.sync()
    gx, gm, gr = d_traj.cpu().numpy(), d_marg.cpu().numpy(), d_rows.cpu().numpy()
    assert np.all(gx[:pad] == -9) and np.all(gx[pad + traj5.size:] == -9)
    assert np.all(gm[:pad] == 12345.5) and np.all(gm[pad + marg0.size:] == 12345.5)
    assert np.all(gr[:pad] == 12345.5) and np.all(gr[pad + rows.size:] == 12345.5)
    assert np.array_equal(gx[pad:pad + traj5.size].astype(np.int32).reshape(traj5.shape), traj5)
    assert np.array_equal(gm[pad:pad + marg0.size].reshape(marg0.shape), marg0)
    assert np.array_equal(gr[pad:pad + rows.size].reshape(rows.shape), rows)
    # nothing the other entry points return has changed
    after = (engine.batch_results(), engine.batch_smooth(33), engine.batch_smooth_stats(case[5]))
    assert before[0][0] == after[0][0] and all(np.array_equal(x, y) for x, y in zip(before[0][1:], after[0][1:]))
    assert np.array_equal(before[1][0], after[1][0]) and all(np.array_equal(x, y) for x, y in zip(before[1][1], after[1][1]))
    assert all(np.array_equal(before[2][key], after[2][key]) for key in before[2])
    assert B == len(before[1][1])


def test_keep_masses_batch_returns_the_same_bits(engine, ran):
    case, ref = ran
    _begin(engine, case)
    want = (engine.batch_forecast(3, 257, 2), engine.batch_predictive(), engine.batch_predictive([1] * len(case[1])))
    _begin(engine, case, keep_history=False, keep_masses=True)
    got = (engine.batch_forecast(3, 257, 2), engine.batch_predictive(), engine.batch_predictive([1] * len(case[1])))
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[0][0][0, :, :_k(case)], ref["marg"][0][:3])


def test_forecast_refusals():
    import torch
    eng = cp.Engine(0)
    try:
        eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K, eng.batch_shapes = 1, 1, 1, 3, None
        for call in (lambda: eng.batch_forecast(2, 4), lambda: eng.batch_predictive()):
            with pytest.raises(cp.CpprobHipError) as e:          # no batch at all
                call()
            assert e.value.code == ESTATE
        obs = [exact.simulate_hmm(T, 70 + b) for b, T in enumerate([3, 2])]
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20])
        for call in (lambda: eng.batch_forecast(2, 4), lambda: eng.batch_predictive()):
            with pytest.raises(cp.CpprobHipError) as e:          # begun, not run
                call()
            assert e.value.code == ESTATE
        eng.batch_run(_seeds(2))
        H, M = 2, 4
        need_m, need_x, need_r = 2 * H * 3, 2 * (H + 1) * M, 2 * 4 * 3
        marg, traj, rows = np.full(need_m, -5.0), np.full(need_x, -5, np.int32), np.full(need_r, -5.0)
        fc = eng.L.cpprob_hip_batch_forecast
        bad = [(0, M, 0, need_m, need_x), (1 << 24, M, 0, need_m, need_x), (H, M, 1 << 16, need_m, need_x), (H, (1 << 20) + 1, 0, need_m, need_x),
               (H, M, 0, need_m - 1, need_x), (H, M, 0, need_m, need_x - 1)]
        for h, m, di, nm, nx in bad:
            assert fc(eng.h, h, m, di, marg.ctypes.data, nm, traj.ctypes.data, nx) == EINVAL, (h, m, di, nm, nx)
            assert np.all(marg == -5.0) and np.all(traj == -5), (h, m, di, nm, nx)
        pr = eng.L.cpprob_hip_batch_predictive
        u32 = C.POINTER(C.c_uint32)
        past = np.array([0, 4], np.uint32)                       # problem 1: from = L + 2
        assert pr(eng.h, past.ctypes.data_as(u32), 4, rows.ctypes.data, need_r) == EINVAL
        assert "problem 1" in eng.L.cpprob_hip_last_error(eng.h).decode()
        assert pr(eng.h, None, 3, rows.ctypes.data, need_r) == EINVAL                   # problem 0 owes 4 rows
        assert "problem 0" in eng.L.cpprob_hip_last_error(eng.h).decode()
        assert pr(eng.h, None, 4, rows.ctypes.data, need_r - 1) == EINVAL
        assert pr(eng.h, None, 4, None, 0) == EINVAL
        assert np.all(rows == -5.0)
        edge = np.array([4, 3], np.uint32)                       # from = L + 1: allowed, no row
        assert pr(eng.h, edge.ctypes.data_as(u32), 1, rows.ctypes.data, 6) == 0 and np.all(rows[:6] == 0.0) and np.all(rows[6:] == -5.0)
        assert fc(eng.h, H, M, 0, marg.ctypes.data, need_m, traj.ctypes.data, need_x) == 0
        assert np.all(marg >= 0.0) and np.all((traj >= 0) & (traj < 3))
        assert pr(eng.h, None, 4, rows.ctypes.data, need_r) == 0 and np.all(rows >= 0.0)
        d = torch.full((need_x,), -9, dtype=torch.int8, device="cuda:0")
        dr = torch.full((need_r,), -9.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.current_stream().synchronize()
        assert eng.L.cpprob_hip_batch_forecast_device(eng.h, H, M, 0, None, 0, C.c_void_p(d.data_ptr()), need_x - 1) == EINVAL
        assert eng.L.cpprob_hip_batch_predictive_device(eng.h, None, 4, C.c_void_p(dr.data_ptr()), need_r - 1) == EINVAL
        eng.sync()
        assert bool((d == -9).all()) and bool((dr == -9.0).all())
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20], keep_history=False)      # a plain filtering batch
        eng.batch_run(_seeds(2))
        for call in (lambda: eng.batch_forecast(2, 4), lambda: eng.batch_predictive()):
            with pytest.raises(cp.CpprobHipError) as e:
                call()
            assert e.value.code == ESTATE and "keep_history" in str(e.value)
    finally:
        eng.close()
