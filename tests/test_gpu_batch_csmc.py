"""Conditional SMC runs of a batch on the device (include/cpprob_hip.h: cpprob_hip_batch_run_conditional*, csrc/batch_csmc.hpp):
the rows of the m table equal tests/csmc_ref.py's bit for bit on uniform batches (a shared table) and described ones (a table a
problem), the backward smoother serves them as tests/backward_ref.py does, the device form fed cpprob_hip_batch_smooth_device's own
buffer equals the host form fed the same path, the refusals, and what the run leaves of an unconditional one before and after it."""
import ctypes as C

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import csmc_ref as CS

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -3, -4
NS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 2049, 8192]      # a partial run of 4, a partial pass, more than one pass, the count-field limit
TS = [2, 7, 1, 2, 7, 1, 2, 7, 2, 7, 1, 2]


def _tables(k, nb, seed):
    """Table 1 has a zero transition entry."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (nb, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (nb, k, k))
    if nb > 1:
        trans[1, 0, k - 1] = 0.0
    return means, trans


def _observes(means, Ts, seed):
    rng = np.random.default_rng(seed)
    k = means.shape[1]
    return [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]


def _paths(k, Ts, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, k, T).astype(np.int32) for T in Ts]


def _seeds(nb, base=77):
    return np.array([(3 << 36) + base + 7919 * b for b in range(nb)], np.uint64)


def _want(obs_b, means_b, trans_b, seed, n, path):
    """(rows [T, 8] float64, the integer masses, P) of one problem."""
    k = len(means_b)
    m = CS.masses(R.log_likelihoods(obs_b, means_b), R.thresholds(trans_b), int(seed), int(n), path)
    rows = np.zeros((len(obs_b), 8))
    rows[:, :k] = np.array(m, np.float64)
    return rows, m, R.transition_masses(trans_b)


def _assert_problem(engine, b, want, traj, seed, what):
    rows, m, P = want
    got = engine.batch_masses(b)
    assert got.shape == rows.shape and np.array_equal(got, rows), "%s problem %d: rows differ from the reference at steps %s" % (what, b, np.nonzero((got != rows).any(axis=1))[0].tolist())
    assert np.array_equal(traj, R.trajectories(m, P, int(seed), 1)), "%s problem %d: the backward trajectory differs from the reference's on these masses" % (what, b)


@pytest.mark.parametrize("k", [2, 5, 8])
def test_described_batches_leave_the_reference_rows(engine, k):
    """One ragged batch a k: every n of the grid, T in {1, 2, 7}, a table a problem (one with a zero entry), systematic and stratified
    batches alike (a conditional run resamples multinomially whatever the batch says)."""
    nb = len(NS)
    means, trans = _tables(k, nb, 60 + k)
    obs = _observes(means, TS, 70 + k)
    paths = _paths(k, TS, 80 + k)
    seeds = _seeds(nb, 5 + k)
    want = [_want(obs[b], means[b], trans[b], seeds[b], NS[b], paths[b]) for b in range(nb)]
    for rs in (cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED):
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, NS, tables=(means, trans), resampler=rs, keep_history=False, keep_masses=True)
        engine.batch_run_conditional(seeds, paths if rs == cp.RESAMPLE_SYSTEMATIC else np.concatenate(paths))
        _, traj = engine.batch_smooth(1)
        for b in range(nb):
            _assert_problem(engine, b, want[b], traj[b], seeds[b], "k = %d, resampler %d," % (k, rs))


@pytest.mark.parametrize("k", [2, 5, 8])
def test_uniform_batches_leave_the_reference_rows(engine, k):
    """A shared table (cpprob_hip_set_hmm), B = 2 problems of the same shape; every n of the grid at one of T = 1, 2, 7."""
    means, trans = _tables(k, 1, 90 + k)
    engine.set_hmm(means[0], trans[0])
    for n, T in zip(NS, TS):
        obs = _observes(np.repeat(means, 2, 0), [T, T], 100 + n)
        paths = _paths(k, [T, T], 110 + n)
        seeds = _seeds(2, n + k)
        engine.batch_begin(cp.MODEL_HMM_TABLE, np.array(obs), n, keep_history=False, keep_masses=True)
        engine.batch_run_conditional(seeds, paths)
        _, traj = engine.batch_smooth(1)
        for b in range(2):
            _assert_problem(engine, b, _want(obs[b], means[0], trans[0], seeds[b], n, paths[b]), traj[b], seeds[b], "k = %d, n = %d, T = %d," % (k, n, T))


def test_device_form_on_the_smoothers_own_buffer_equals_the_host_form(engine):
    """batch_smooth_device(traj_i8, n_traj = 1) after an unconditional run leaves the paths where the device form reads them; the host
    form fed the same paths leaves the same rows, and both equal the reference on those paths."""
    import torch
    k, Ts, ns = 3, [5, 1, 7, 3], [40, 300, 7, 1025]
    means, trans = _tables(k, 4, 17)
    obs = _observes(means, Ts, 18)
    seeds = _seeds(4, 19)
    begin = lambda: engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans), keep_history=False, keep_masses=True)  # noqa: E731
    begin()
    engine.batch_run(seeds)
    first = cp.capi.batch_smooth_layout(Ts, 1)
    buf = torch.empty(int(first[-1]), dtype=torch.int8, device="cuda:0")
    engine.batch_smooth_device(traj_i8=buf, n_traj=1, draw_index=3)
    engine.batch_run_conditional_device(seeds + np.uint64(1), buf)
    engine.sync()
    flat = buf.cpu().numpy().astype(np.int32)
    paths = [flat[int(first[b]):int(first[b + 1])] for b in range(4)]
    assert all(p.min() >= 0 and p.max() < k for p in paths)
    dev = [engine.batch_masses(b) for b in range(4)]
    dev_traj = engine.batch_smooth(2, draw_index=4)[1]
    begin()
    engine.batch_run_conditional(seeds + np.uint64(1), paths)
    for b in range(4):
        assert np.array_equal(engine.batch_masses(b), dev[b]), b
        assert np.array_equal(dev[b], _want(obs[b], means[b], trans[b], seeds[b] + np.uint64(1), ns[b], paths[b])[0]), b
    assert all(np.array_equal(x, y) for x, y in zip(engine.batch_smooth(2, draw_index=4)[1], dev_traj))


def _rc(engine, seeds, ref, n=None, device=False):
    fn = engine.L.cpprob_hip_batch_run_conditional_device if device else engine.L.cpprob_hip_batch_run_conditional
    return fn(engine.h, None if seeds is None else seeds.ctypes.data_as(C.POINTER(C.c_uint64)), None if ref is None else ref.ctypes.data, ref.size if n is None else n)


def test_refusals(engine):
    k, T, B = 3, 4, 2
    means, trans = _tables(k, 1, 31)
    engine.set_hmm(means[0], trans[0])
    obs = np.array(_observes(np.repeat(means, B, 0), [T] * B, 32))
    seeds = _seeds(B, 33)
    ref = np.zeros(B * T, np.int32)
    fresh = cp.Engine(0)
    try:
        assert _rc(fresh, seeds, ref) == ESTATE and _rc(fresh, seeds, ref, device=True) == ESTATE      # no batch begun
    finally:
        fresh.close()
    engine.batch_begin(cp.MODEL_HMM_TABLE, obs, 8)                                                  # keep_history = 1
    assert _rc(engine, seeds, ref) == ESTATE and _rc(engine, seeds, ref, device=True) == ESTATE
    engine.batch_begin(cp.MODEL_HMM_TABLE, obs, 8, keep_history=False)                              # no masses bit
    assert _rc(engine, seeds, ref) == ESTATE and _rc(engine, seeds, ref, device=True) == ESTATE
    engine.batch_begin(cp.MODEL_HMM3, obs, 8, keep_history=False, keep_masses=True)
    assert _rc(engine, seeds, ref) == EUNSUPPORTED and _rc(engine, seeds, ref, device=True) == EUNSUPPORTED
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, [T] * B, 8, seeds, keep_history=False, keep_masses=True)
    assert _rc(engine, seeds, ref) == EUNSUPPORTED and _rc(engine, seeds, ref, device=True) == EUNSUPPORTED
    # a batch that admits the call: the refusals enqueue nothing, so the rows of the run before them stand
    engine.batch_begin(cp.MODEL_HMM_TABLE, obs, 8, keep_history=False, keep_masses=True)
    engine.batch_run(seeds)
    before = [engine.batch_masses(b) for b in range(B)]
    res = engine.batch_results()
    bad = ref.copy()
    bad[5] = k
    neg = ref.copy()
    neg[0] = -1
    for rc in (_rc(engine, None, ref), _rc(engine, seeds, None, n=B * T), _rc(engine, seeds, ref, n=B * T - 1), _rc(engine, seeds, ref, n=B * T + 1),
               _rc(engine, seeds, bad), _rc(engine, seeds, neg), _rc(engine, None, ref, device=True), _rc(engine, seeds, ref, n=B * T - 1, device=True)):
        assert rc == EINVAL
    assert b"reference state 3" in engine.L.cpprob_hip_last_error(engine.h) or b"lengths sum" in engine.L.cpprob_hip_last_error(engine.h)
    assert all(np.array_equal(engine.batch_masses(b), before[b]) for b in range(B))
    again = engine.batch_results()
    assert again[0] == res[0] and all(np.array_equal(x, y) for x, y in zip(again[1:], res[1:]))
    with pytest.raises(ValueError):
        engine.batch_run_conditional(seeds, ref[:-1])


def test_results_wait_for_a_run_and_the_run_returns_what_it_returned(engine):
    """After a conditional run cpprob_hip_batch_results and _results_device return ESTATE -- it keeps masses, not books, and a run
    before it must not be read as its own --; the next batch_run reproduces its earlier results and rows bit for bit; the calls that
    read the m table all serve the conditional run."""
    import torch
    k, Ts, ns = 5, [6, 2, 9], [64, 1025, 5]
    means, trans = _tables(k, 3, 41)
    obs = _observes(means, Ts, 42)
    seeds = _seeds(3, 43)
    paths = _paths(k, Ts, 44)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans), keep_history=False, keep_masses=True)
    engine.batch_run(seeds)
    res = engine.batch_results()
    rows = [engine.batch_masses(b) for b in range(3)]
    engine.batch_run_conditional(seeds, paths)
    out = torch.zeros(3 * (4 + 9 * 8), dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    sums = (cp.capi.Summary * 3)()
    assert engine.L.cpprob_hip_batch_results(engine.h, sums, None, 0, None, None) == ESTATE
    assert b"conditional run" in engine.L.cpprob_hip_last_error(engine.h)
    assert engine.L.cpprob_hip_batch_results_device(engine.h, C.c_void_p(out.data_ptr()), out.numel()) == ESTATE
    with pytest.raises(cp.CpprobHipError):
        engine.batch_results()
    cond = [engine.batch_masses(b) for b in range(3)]
    assert not all(np.array_equal(x, y) for x, y in zip(cond, rows))
    # every reader of the m table serves it
    marg, traj = engine.batch_smooth(3, draw_index=2)
    for b in range(3):
        m = [[int(v) for v in r[:k]] for r in cond[b]]
        P = R.transition_masses(trans[b])
        assert np.array_equal(traj[b], R.trajectories(m, P, int(seeds[b]), 3, 2))
        assert np.array_equal(marg[b, :Ts[b], :k], R.marginals(m, P))
    lag_marg, _ = engine.batch_smooth_lag(max(Ts))                            # (a lag past every length: the full smoother's rows)
    assert np.array_equal(lag_marg, marg)
    st = engine.batch_smooth_stats(obs)
    ts = engine.batch_traj_stats(2, draw_index=2, observes=obs)
    assert np.all(st["occ"].sum(axis=1) > 0) and np.array_equal(ts["occ"].sum(axis=2)[:, 0], np.array(Ts, np.float64))
    fm, _ = engine.batch_forecast(2)
    pr = engine.batch_predictive()
    path, score = engine.batch_decode()
    assert np.all(np.isfinite(fm[:, :, :k])) and np.allclose(fm[:, :, :k].sum(axis=2), 1.0) and np.all(np.isfinite(score))
    assert np.all(pr[:, 0, :k] == 1.0 / k)
    for b in range(3):                                                      # the decoded path walks states the conditional run's particles occupy
        assert len(path[b]) == Ts[b] and all(cond[b][t, path[b][t]] > 0 for t in range(Ts[b]))
        assert np.array_equal(pr[b, Ts[b], :k], fm[b, 0, :k])               # the predictive row past the last observe is the forecast's first
    # ... and a run after it is the run before it
    engine.batch_run(seeds)
    again = engine.batch_results()
    assert again[0] == res[0] and all(np.array_equal(x, y) for x, y in zip(again[1:], res[1:]))
    assert all(np.array_equal(engine.batch_masses(b), rows[b]) for b in range(3))
