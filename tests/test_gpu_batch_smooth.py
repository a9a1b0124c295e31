"""Backward smoothing of a batch (include/cpprob_hip.h: cpprob_hip_batch_smooth, _smooth_device; csrc/batch_smooth.hpp) against the
plain-Python restatement of its arithmetic (tests/backward_ref.py) on the rows the run left (cpprob_hip_batch_copy_store).  The
trajectories are a pure function of integers and uncontracted IEEE operations: array_equal.  The marginals are compared within
1e-12 absolute: at most T k^2 operations of 2^-52 relative on quantities <= 1, 9e-13 at the largest shape here (T = 64, k = 8) --
this project trusts the device's division only up to the last bits."""
import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
from oracle import exact

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
RESAMPLERS = [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED]
TOL = 1e-12


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the one-shot batches an online batch is compared with (a begin on `engine` would replace it)."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


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


def _reference(engine, b, obs_b, means, trans, seed, n_traj, draw_index=0):
    """(marginals [T_b, k], trajectories [T_b, n_traj]) of problem b from the rows its run left."""
    vals, _, logw = engine.batch_store(b)
    ll = R.log_likelihoods(obs_b, means)
    # (the restated table rows are the run's own: its final log-weights are table doubles)
    assert np.all(logw == np.array(ll[-1])[vals[-1]]), "problem %d: restated log-likelihoods differ from the run's table" % b
    m, P = R.filtering_masses(vals, ll), R.transition_masses(trans)
    return R.marginals(m, P), R.trajectories_fast(m, P, int(seed), n_traj, draw_index)


def _assert_problem(b, marg_b, traj_b, ref_g, ref_x, what=""):
    T, k = ref_g.shape
    err = float(np.abs(marg_b[:T, :k] - ref_g).max())
    print("%sproblem %d: T = %d, k = %d, largest marginal difference %.3g, trajectories %s" % (what, b, T, k, err, traj_b.shape))
    assert traj_b.dtype == np.int32 and traj_b.shape == ref_x.shape, (what, b)
    assert np.array_equal(traj_b, ref_x), "%sproblem %d: trajectories differ from the reference" % (what, b)
    assert err <= TOL, "%sproblem %d: marginals differ from the reference by %.3g" % (what, b, err)
    assert np.all(marg_b[T:] == 0.0) and np.all(marg_b[:, k:] == 0.0), "%sproblem %d: padding is not zero" % (what, b)


# ---- 1. uniform batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 777, 4099])
@pytest.mark.parametrize("rs", RESAMPLERS)
def test_uniform_hmm3_batch(engine, rs, n):
    """One particle, a ragged last tile, more than four tiles; a single lane, a ragged last wavefront, a second tile of trajectories."""
    B, T = 5, 16
    obs = [exact.simulate_hmm(T, 900 + b) for b in range(B)]
    seeds = _seeds(B, 3 + n)
    engine.batch_begin(cp.MODEL_HMM3, np.array(obs), n, resampler=rs)
    engine.batch_run(seeds)
    for M in (1, 1000, 1025):
        marg, traj = engine.batch_smooth(M)
        assert marg.shape == (B, T, 3) and len(traj) == B
        for b in range(B):
            g, x = _reference(engine, b, obs[b], exact.HMM_MEAN, exact.HMM_T, seeds[b], M)
            _assert_problem(b, marg[b], traj[b], g, x, "n = %d, M = %d, " % (n, M))
    assert cp.capi.batch_smooth_layout([T] * B, 1025).tolist() == [b * T * 1025 for b in range(B + 1)]


# ---- 2. described batch ----------------------------------------------------------------------------------------------------------
def _described(k):
    """Six problems with a table each: lengths {1, 2, 7, 64} (T = 1 has no backward step), particle counts {3, 256, 1500, 8192};
    problem 1's table has a zero transition entry; problems 4 and 5 carry the table and observes of
    tests/test_gpu_batch_problems.py::test_requantised_generations_with_per_problem_tables widened to k states: the last state sits
    far from the others and next to the observes, and is entered rarely, so it is absent from most generations and M_t is not the
    step's bound."""
    Ts, ns = [1, 2, 7, 64, 7, 64], [3, 1500, 256, 8192, 3, 256]
    means, trans = _tables(k, len(Ts), 31 + k)
    obs = _table_observes(means, Ts, 31 + k)
    for b, y0 in ((4, -0.5), (5, -1.2)):
        means[b] = np.concatenate([np.linspace(-1.0, 0.0, k - 1), [10.0]]) if k > 2 else np.array([-1.0, 10.0])
        trans[b, :k - 1, :k - 1] = 5.0
        trans[b, :k - 1, k - 1] = 0.01
        trans[b, k - 1, :] = 1.0
        obs[b] = np.full(Ts[b], 30.0)
        obs[b][0] = y0
    return Ts, ns, means, trans, obs


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("k", [2, 3, 5, 7, 8])
def test_described_table_batch(engine, k, rs):
    Ts, ns, means, trans, obs = _described(k)
    B, M = len(Ts), 300
    seeds = _seeds(B, 19 + k)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans), resampler=rs)
    engine.batch_run(seeds)
    marg, traj = engine.batch_smooth(M)
    assert marg.shape == (B, 64, 8)
    for b in range(B):
        g, x = _reference(engine, b, obs[b], means[b], trans[b], seeds[b], M)
        _assert_problem(b, marg[b], traj[b], g, x, "k = %d, " % k)
    vals = engine.batch_store(4)[0]
    assert np.any(np.all(vals != k - 1, axis=1)), "the far state should be absent from some generation of problem 4"
    assert cp.capi.batch_smooth_layout(Ts, M).tolist() == [M * sum(Ts[:b]) for b in range(B + 1)]


def test_long_problem_reads_its_masses_from_memory(engine):
    """A problem longer than the 512 steps whose masses a tile stages in LDS, beside a short one that is staged."""
    Ts, ns, M = [600, 5], [37, 260], 70
    obs = [exact.simulate_hmm(T, 40 + b) for b, T in enumerate(Ts)]
    seeds = _seeds(2, 5)
    engine.batch_begin_problems(cp.MODEL_HMM3, obs, ns)
    engine.batch_run(seeds)
    marg, traj = engine.batch_smooth(M)
    for b in range(2):
        g, x = _reference(engine, b, obs[b], exact.HMM_MEAN, exact.HMM_T, seeds[b], M)
        _assert_problem(b, marg[b], traj[b], g, x)


# ---- 3. a batch advanced in pieces -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last_readout", [True, False])
@pytest.mark.parametrize("model,k", [(cp.MODEL_HMM3, 3), (cp.MODEL_HMM_TABLE, 8)])
def test_online_batch_is_the_one_shot_batch_of_the_lengths_reached(engine, ref_engine, model, k, last_readout):
    caps, ns, M = [12, 12, 12], [777, 3, 1025], 100
    advances = [(5, 0, 0), (3, 0, 5), (0, 0, 3)]                     # pieces of 0, 5 and 3 observes; problem 1 stays at length 0
    if model == cp.MODEL_HMM3:
        tables, obs = None, [exact.simulate_hmm(12, 60 + b) for b in range(3)]
        means, trans = [exact.HMM_MEAN] * 3, [exact.HMM_T] * 3
    else:
        means, trans = _tables(k, 3, 41)
        tables, obs = (means, trans), _table_observes(means, caps, 41)
    seeds = _seeds(3, 11)
    engine.batch_begin_online(model, caps, ns, seeds, tables=tables)
    marg, traj = engine.batch_smooth(M)                               # no observes yet
    assert np.all(marg == 0.0) and all(x.shape == (0, M) for x in traj)
    lens = [0, 0, 0]
    for a, dT in enumerate(advances):
        engine.batch_advance([obs[b][lens[b]:lens[b] + dT[b]] for b in range(3)], readout=last_readout or a + 1 < len(advances))
        lens = [lens[b] + dT[b] for b in range(3)]
        marg, traj = engine.batch_smooth(M)
        assert marg.shape == (3, 12, 3 if model == cp.MODEL_HMM3 else 8)
        idx = [b for b in range(3) if lens[b] >= 1]
        tb = None if tables is None else (means[idx], trans[idx])
        ref_engine.batch_begin_problems(model, [obs[b][:lens[b]] for b in idx], [ns[b] for b in idx], tables=tb)
        ref_engine.batch_run(seeds[idx])
        ref_marg, ref_traj = ref_engine.batch_smooth(M)
        for i, b in enumerate(idx):
            assert np.array_equal(traj[b], ref_traj[i]), "advance %d, problem %d" % (a, b)
            assert np.array_equal(marg[b, :lens[b]], ref_marg[i, :lens[b]]), "advance %d, problem %d" % (a, b)
            g, x = _reference(engine, b, obs[b][:lens[b]], means[b], trans[b], seeds[b], M)
            _assert_problem(b, marg[b], traj[b], g, x, "advance %d, " % a)
        for b in range(3):
            if lens[b] == 0:
                assert traj[b].shape == (0, M) and np.all(marg[b] == 0.0), (a, b)
    assert lens == [8, 0, 8]


# ---- 4. draw_index, the device variant, and what the call leaves alone -----------------------------------------------------------
def test_draw_index_device_variant_and_untouched_results(engine):
    import torch
    Ts, ns, means, trans, obs = _described(8)
    B, M = len(Ts), 130
    seeds = _seeds(B, 29)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans))
    engine.batch_run(seeds)
    before = (engine.batch_results(), [engine.batch_store(b) for b in range(B)], engine.batch_paths())
    marg0, traj0 = engine.batch_smooth(M, 0)
    marg1, traj1 = engine.batch_smooth(M, 1)
    top, _ = engine.batch_smooth(M, (1 << 16) - 1)
    assert np.array_equal(marg0, marg1) and np.array_equal(marg0, top), "the marginals depend on draw_index"
    assert any(not np.array_equal(x, y) for x, y in zip(traj0, traj1)), "draw_index 0 and 1 give the same trajectories"
    for di, traj in ((0, traj0), (1, traj1)):
        for b in range(B):
            g, x = _reference(engine, b, obs[b], means[b], trans[b], seeds[b], M, di)
            _assert_problem(b, marg0[b], traj[b], g, x, "draw_index %d, " % di)
    # the marginals alone, and trajectories alone
    only_m, none = engine.batch_smooth(0)
    assert np.array_equal(only_m, marg0) and all(x.shape == (T, 0) for x, T in zip(none, Ts))
    first = cp.capi.batch_smooth_layout(Ts, M)
    flat = np.full(int(first[-1]), -5, np.int32)
    assert engine.L.cpprob_hip_batch_smooth(engine.h, M, 1, None, 0, flat.ctypes.data, flat.size) == 0
    assert np.array_equal(flat, np.concatenate([x.reshape(-1) for x in traj1]))
    # the device variant, behind guard bands
    n_entries, n_doubles, pad = int(first[-1]), marg0.size, 256
    d_traj = torch.full((n_entries + 2 * pad,), -9, dtype=torch.int8, device="cuda:0")
    d_marg = torch.full((n_doubles + 2 * pad,), 12345.5, dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_smooth_device(d_marg[pad:pad + n_doubles], d_traj[pad:pad + n_entries], n_traj=M, draw_index=1)
    engine.sync()
    got_x, got_m = d_traj.cpu().numpy(), d_marg.cpu().numpy()
    assert np.all(got_x[:pad] == -9) and np.all(got_x[pad + n_entries:] == -9)
    assert np.all(got_m[:pad] == 12345.5) and np.all(got_m[pad + n_doubles:] == 12345.5)
    assert np.array_equal(got_x[pad:pad + n_entries].astype(np.int32), np.concatenate([x.reshape(-1) for x in traj1]))
    assert np.array_equal(got_m[pad:pad + n_doubles].reshape(marg0.shape), marg0)
    # nothing the other entry points return has changed
    after = (engine.batch_results(), [engine.batch_store(b) for b in range(B)], engine.batch_paths())
    assert before[0][0] == after[0][0]
    assert all(np.array_equal(x, y) for x, y in zip(before[0][1:], after[0][1:]))
    assert all(np.array_equal(x, y) for sb, sa in zip(before[1], after[1]) for x, y in zip(sb, sa))
    assert all(np.array_equal(x, y) for pb, pa in zip(before[2], after[2]) for x, y in zip(pb, pa))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_smooth_refusals():
    import ctypes as C
    import torch  # noqa: F401
    eng = cp.Engine(0)
    try:
        with pytest.raises(cp.CpprobHipError) as e:
            eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K, eng.batch_shapes = 1, 1, 1, 3, None
            eng.batch_smooth(4)
        assert e.value.code == ESTATE
        obs = [exact.simulate_hmm(T, 70 + b) for b, T in enumerate([3, 2])]
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20])
        with pytest.raises(cp.CpprobHipError) as e:          # begun, not run
            eng.batch_smooth(4)
        assert e.value.code == ESTATE
        eng.batch_run(_seeds(2))
        M, need_m, need_x = 4, 2 * 3 * 3, 4 * 5
        marg = np.full(need_m, -5.0)
        traj = np.full(need_x, -5, np.int32)
        rc = eng.L.cpprob_hip_batch_smooth(eng.h, M, 0, marg.ctypes.data, need_m - 1, traj.ctypes.data, need_x)
        assert rc == EINVAL and np.all(marg == -5.0) and np.all(traj == -5)
        rc = eng.L.cpprob_hip_batch_smooth(eng.h, M, 0, marg.ctypes.data, need_m, traj.ctypes.data, need_x - 1)
        assert rc == EINVAL and np.all(marg == -5.0) and np.all(traj == -5)
        rc = eng.L.cpprob_hip_batch_smooth(eng.h, M, 1 << 16, marg.ctypes.data, need_m, traj.ctypes.data, need_x)
        assert rc == EINVAL and np.all(marg == -5.0) and np.all(traj == -5)
        rc = eng.L.cpprob_hip_batch_smooth(eng.h, (1 << 20) + 1, 0, marg.ctypes.data, need_m, None, 0)
        assert rc == EINVAL and np.all(marg == -5.0)
        assert eng.L.cpprob_hip_batch_smooth(eng.h, M, 0, marg.ctypes.data, need_m, traj.ctypes.data, need_x) == 0
        assert np.all(marg >= 0.0) and np.all((traj >= 0) & (traj < 3))
        d = torch.full((need_x,), -9, dtype=torch.int8, device="cuda:0")
        torch.cuda.current_stream().synchronize()
        rc = eng.L.cpprob_hip_batch_smooth_device(eng.h, M, 0, None, 0, C.c_void_p(d.data_ptr()), need_x - 1)
        eng.sync()
        assert rc == EINVAL and bool((d == -9).all())
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20], keep_history=False)
        eng.batch_run(_seeds(2))
        with pytest.raises(cp.CpprobHipError) as e:
            eng.batch_smooth(4)
        assert e.value.code == ESTATE and "keep_history" in str(e.value)
    finally:
        eng.close()
