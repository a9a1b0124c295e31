"""Expected sufficient statistics of a batch (include/cpprob_hip.h: cpprob_hip_batch_smooth_stats, _smooth_stats_device;
csrc/batch_suffstats.hpp) against the plain-Python restatement of their arithmetic (tests/suffstats_ref.py) on the rows the run left
(cpprob_hip_batch_copy_store), and particle EM on them (cpprob_amd/em.py) against exact Baum-Welch.

Tolerance per entry: T (1e-12 + T 2^-53) max(1, |y|max)^p with p = 0, 0, 1, 2 for xi, occ, occ_y, occ_yy -- this project's budget of
1e-12 a marginal entry (tests/test_gpu_batch_smooth.py: the device's division is trusted up to the last bits) summed over the T
steps, plus the T additions of the accumulator, each half an ulp of a sum that is at most T."""
import ctypes as C

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import suffstats_ref as S
from oracle import exact

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
FIELDS = (("xi", 0), ("occ", 0), ("occ_y", 1), ("occ_yy", 2))


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
    """tests/test_gpu_batch_smooth.py::_tables: table 1 has a zero transition entry."""
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


def _reference(engine, b, obs_b, means, trans):
    """The reference statistics of problem b from the rows its run left."""
    vals, _, logw = engine.batch_store(b)
    ll = R.log_likelihoods(obs_b, means)
    assert np.all(logw == np.array(ll[-1])[vals[-1]]), "problem %d: restated log-likelihoods differ from the run's table" % b
    return S.stats(R.filtering_masses(vals, ll), R.transition_masses(trans), obs_b)


def _assert_problem(b, got, ref, obs_b, k, what=""):
    """got: the dict of problem b's arrays ([8, 8] and [8])."""
    T = len(obs_b)
    ymax = max(1.0, float(np.abs(obs_b).max())) if T else 1.0
    worst = []
    for f, p in FIELDS:
        tol = T * (1e-12 + T * 2.0 ** -53) * ymax ** p
        err = float(np.abs(got[f] - ref[f]).max())
        worst.append("%s %.3g (bound %.3g)" % (f, err, tol))
        assert err <= tol, "%sproblem %d: %s differs from the reference by %.3g, bound %.3g" % (what, b, f, err, tol)
    print("%sproblem %d: T = %d, k = %d, largest differences: %s" % (what, b, T, k, ", ".join(worst)))
    assert np.all(got["xi"][k:] == 0.0) and np.all(got["xi"][:, k:] == 0.0), "%sproblem %d: xi's padding is not zero" % (what, b)
    assert all(np.all(got[f][k:] == 0.0) for f in ("occ", "occ_y", "occ_yy")), "%sproblem %d: padding is not zero" % (what, b)


def _of(stats, b):
    return {f: v[b] for f, v in stats.items()}


# ---- 1. against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 777])
def test_uniform_hmm3_batch(engine, n):
    """Five problems: two workgroups, the second holding one wavefront with work."""
    B, T = 5, 16
    obs = [exact.simulate_hmm(T, 900 + b) for b in range(B)]
    engine.batch_begin(cp.MODEL_HMM3, np.array(obs), n)
    engine.batch_run(_seeds(B, 3 + n))
    stats = engine.batch_smooth_stats(np.array(obs))
    assert stats["xi"].shape == (B, 8, 8) and all(stats[f].shape == (B, 8) for f in ("occ", "occ_y", "occ_yy"))
    marg, _ = engine.batch_smooth(0)
    for b in range(B):
        _assert_problem(b, _of(stats, b), _reference(engine, b, obs[b], exact.HMM_MEAN, exact.HMM_T), obs[b], 3, "n = %d, " % n)
        assert np.abs(stats["occ"][b, :3] - marg[b].sum(axis=0)).max() <= T * (1e-12 + T * 2.0 ** -53), "occ is not the marginals' column sums"
    blind = engine.batch_smooth_stats()
    assert np.array_equal(blind["xi"], stats["xi"]) and np.array_equal(blind["occ"], stats["occ"])
    assert np.all(blind["occ_y"] == 0.0) and np.all(blind["occ_yy"] == 0.0)


def _described(k):
    """Five problems with a table each, ragged lengths up to 64 with T = 1 among them (no backward step); problem 1's table has a
    zero transition entry; problem 4 carries the table and observes of tests/test_gpu_batch_smooth.py::_described's far state: the
    last state is entered rarely and absent from most generations."""
    Ts, ns = [1, 2, 7, 64, 64], [3, 1500, 256, 8192, 256]
    means, trans = _tables(k, len(Ts), 31 + k)
    obs = _table_observes(means, Ts, 31 + k)
    means[4] = np.concatenate([np.linspace(-1.0, 0.0, k - 1), [10.0]]) if k > 2 else np.array([-1.0, 10.0])
    trans[4, :k - 1, :k - 1] = 5.0
    trans[4, :k - 1, k - 1] = 0.01
    trans[4, k - 1, :] = 1.0
    obs[4] = np.full(Ts[4], 30.0)
    obs[4][0] = -1.2
    return Ts, ns, means, trans, obs


@pytest.mark.parametrize("k", [2, 3, 8])
def test_described_table_batch(engine, k):
    Ts, ns, means, trans, obs = _described(k)
    B = len(Ts)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans))
    engine.batch_run(_seeds(B, 19 + k))
    stats = engine.batch_smooth_stats(obs)
    marg, _ = engine.batch_smooth(0)
    for b in range(B):
        _assert_problem(b, _of(stats, b), _reference(engine, b, obs[b], means[b], trans[b]), obs[b], k, "k = %d, " % k)
        assert np.abs(stats["occ"][b] - marg[b].sum(axis=0)).max() <= Ts[b] * (1e-12 + Ts[b] * 2.0 ** -53)
    assert np.all(stats["xi"][0] == 0.0), "T = 1 has no transition"
    vals = engine.batch_store(4)[0]
    assert np.any(np.all(vals != k - 1, axis=1)), "the far state should be absent from some generation of problem 4"


# ---- 2. an online batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", [(cp.MODEL_HMM3, 3), (cp.MODEL_HMM_TABLE, 8)])
def test_online_batch_is_the_one_shot_batch_of_the_lengths_reached(engine, ref_engine, model, k):
    """After every advance the records equal the one-shot batch's bit for bit, whichever call counted the new rows: the statistics
    call first, a smoothing call first, or a statistics call with nothing new."""
    caps, ns = [12, 12, 12], [777, 3, 1025]
    advances = [(5, 0, 0), (3, 0, 5), (0, 0, 3)]                     # problem 1 stays at length 0
    if model == cp.MODEL_HMM3:
        tables, obs = None, [exact.simulate_hmm(12, 60 + b) for b in range(3)]
    else:
        means, trans = _tables(k, 3, 41)
        tables, obs = (means, trans), _table_observes(means, caps, 41)
    seeds = _seeds(3, 11)
    engine.batch_begin_online(model, caps, ns, seeds, tables=tables)
    none = engine.batch_smooth_stats([[], [], []])                   # no observes yet
    assert all(np.all(v == 0.0) for v in none.values())
    lens = [0, 0, 0]
    for a, dT in enumerate(advances):
        engine.batch_advance([obs[b][lens[b]:lens[b] + dT[b]] for b in range(3)])
        lens = [lens[b] + dT[b] for b in range(3)]
        seen = [obs[b][:lens[b]] for b in range(3)]
        if a == 1:
            marg_first, _ = engine.batch_smooth(0)                   # (this call counts the new rows, the statistics call none)
        stats = engine.batch_smooth_stats(seen)
        again = engine.batch_smooth_stats(seen)
        marg, _ = engine.batch_smooth(0)
        idx = [b for b in range(3) if lens[b] >= 1]
        tb = None if tables is None else (means[idx], trans[idx])
        ref_engine.batch_begin_problems(model, [seen[b] for b in idx], [ns[b] for b in idx], tables=tb)
        ref_engine.batch_run(seeds[idx])
        ref_stats = ref_engine.batch_smooth_stats([seen[b] for b in idx])
        ref_marg, _ = ref_engine.batch_smooth(0)
        for i, b in enumerate(idx):
            for f, _ in FIELDS:
                assert np.array_equal(stats[f][b], ref_stats[f][i]), "advance %d, problem %d: %s" % (a, b, f)
                assert np.array_equal(again[f][b], stats[f][b]), "advance %d, problem %d: %s changed between two calls" % (a, b, f)
            assert np.array_equal(marg[b, :lens[b]], ref_marg[i, :lens[b]]), "advance %d, problem %d: marginals after the statistics" % (a, b)
        if a == 1:
            assert np.array_equal(marg_first, marg)
        for b in range(3):
            if lens[b] == 0:
                assert all(np.all(stats[f][b] == 0.0) for f, _ in FIELDS), (a, b)
    assert lens == [8, 0, 8]


# ---- 3. the device variant, and what the call leaves alone -----------------------------------------------------------------------
def test_device_variant_and_untouched_results(engine):
    import torch
    Ts, ns, means, trans, obs = _described(8)
    B = len(Ts)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans))
    engine.batch_run(_seeds(B, 29))
    before = (engine.batch_results(), [engine.batch_store(b) for b in range(B)], engine.batch_paths())
    marg0, traj0 = engine.batch_smooth(50)
    stats = engine.batch_smooth_stats(obs)
    marg1, traj1 = engine.batch_smooth(50)
    assert np.array_equal(marg0, marg1) and all(np.array_equal(x, y) for x, y in zip(traj0, traj1)), "the statistics call changed the smoother's output"
    again = engine.batch_smooth_stats(obs)
    assert all(np.array_equal(stats[f], again[f]) for f, _ in FIELDS), "a smoothing call changed the statistics"
    flat = np.concatenate(obs)
    n_doubles, pad = B * 88, 256
    d_stats = torch.full((n_doubles + 2 * pad,), 12345.5, dtype=torch.float64, device="cuda:0")
    d_obs = torch.full((flat.size + 2 * pad,), 1e300, dtype=torch.float64, device="cuda:0")
    d_obs[pad:pad + flat.size] = torch.from_numpy(flat).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_smooth_stats_device(d_stats[pad:pad + n_doubles], d_obs[pad:pad + flat.size])
    engine.sync()
    got = d_stats.cpu().numpy()
    assert np.all(got[:pad] == 12345.5) and np.all(got[pad + n_doubles:] == 12345.5), "the device variant wrote outside its records"
    dev = cp.capi.split_stats(got[pad:pad + n_doubles])
    assert all(np.array_equal(dev[f], stats[f]) for f, _ in FIELDS), "the device variant differs from the host call"
    assert bool((d_obs[:pad] == 1e300).all()) and bool((d_obs[pad + flat.size:] == 1e300).all())
    # a larger buffer than needed: only the records are written; no observes: the weighted sums are zero
    d_stats.fill_(-3.0)
    torch.cuda.current_stream().synchronize()
    engine.batch_smooth_stats_device(d_stats)
    engine.sync()
    got = d_stats.cpu().numpy()
    assert np.all(got[n_doubles:] == -3.0)
    blind = cp.capi.split_stats(got[:n_doubles])
    assert np.array_equal(blind["xi"], stats["xi"]) and np.array_equal(blind["occ"], stats["occ"]) and np.all(blind["occ_y"] == 0.0) and np.all(blind["occ_yy"] == 0.0)
    # nothing the other entry points return has changed
    after = (engine.batch_results(), [engine.batch_store(b) for b in range(B)], engine.batch_paths())
    assert before[0][0] == after[0][0]
    assert all(np.array_equal(x, y) for x, y in zip(before[0][1:], after[0][1:]))
    assert all(np.array_equal(x, y) for sb, sa in zip(before[1], after[1]) for x, y in zip(sb, sa))
    assert all(np.array_equal(x, y) for pb, pa in zip(before[2], after[2]) for x, y in zip(pb, pa))


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_stats_refusals():
    import torch  # noqa: F401
    eng = cp.Engine(0)
    try:
        eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K, eng.batch_shapes = 1, 1, 1, 3, None
        with pytest.raises(cp.CpprobHipError) as e:          # no batch
            eng.batch_smooth_stats()
        assert e.value.code == ESTATE
        obs = [exact.simulate_hmm(T, 70 + b) for b, T in enumerate([3, 2])]
        flat = np.concatenate(obs)
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20])
        with pytest.raises(cp.CpprobHipError) as e:          # begun, not run
            eng.batch_smooth_stats(obs)
        assert e.value.code == ESTATE
        eng.batch_run(_seeds(2))
        rec = np.full(2 * 88, -5.0)
        call = eng.L.cpprob_hip_batch_smooth_stats
        assert call(eng.h, flat.ctypes.data, flat.size, rec.ctypes.data, rec.size - 1) == EINVAL and np.all(rec == -5.0)
        assert call(eng.h, flat.ctypes.data, flat.size - 1, rec.ctypes.data, rec.size) == EINVAL and np.all(rec == -5.0)
        assert call(eng.h, flat.ctypes.data, flat.size + 1, rec.ctypes.data, rec.size) == EINVAL and np.all(rec == -5.0)
        assert call(eng.h, flat.ctypes.data, flat.size, None, rec.size) == EINVAL
        assert call(eng.h, flat.ctypes.data, flat.size, rec.ctypes.data, rec.size) == 0
        st = cp.capi.split_stats(rec)
        assert np.abs(st["occ"].sum(axis=1) - [3.0, 2.0]).max() <= 1e-12 and np.abs(st["xi"].sum(axis=(1, 2)) - [2.0, 1.0]).max() <= 1e-12
        d = torch.full((2 * 88,), -9.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.current_stream().synchronize()
        rc = eng.L.cpprob_hip_batch_smooth_stats_device(eng.h, None, 0, C.c_void_p(d.data_ptr()), 2 * 88 - 1)
        eng.sync()
        assert rc == EINVAL and bool((d == -9.0).all())
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20], keep_history=False)
        eng.batch_run(_seeds(2))
        with pytest.raises(cp.CpprobHipError) as e:
            eng.batch_smooth_stats(obs)
        assert e.value.code == ESTATE and "keep_history" in str(e.value)
    finally:
        eng.close()


# ---- 5. particle EM end to end ---------------------------------------------------------------------------------------------------
def em_case():
    """tests/test_suffstats_ref_host.py::em_case: k = 2, T = 64, true means -1.5 / +1.5 and self-transition 0.9; the start is means
    -0.5 / +0.5 and uniform transitions."""
    rng = np.random.default_rng(4242)
    true_means = np.array([-1.5, 1.5])
    s, obs = int(rng.integers(0, 2)), np.zeros(64)
    for t in range(64):
        if t > 0 and rng.random() >= 0.9:
            s = 1 - s
        obs[t] = true_means[s] + rng.standard_normal()
    return obs, np.array([-0.5, 0.5]), np.full((2, 2), 0.5)


def test_particle_em_tracks_exact_em(engine):
    """B = 4 restarts of the case (the same start, run seeds 4242 + 1000 b + iteration), n = 256, 10 iterations: after every
    iteration every restart's means are within 0.05 and its transition rows within 0.02 of Baum-Welch run alongside, and its last
    log-evidence exceeds its first."""
    obs, means0, trans0 = em_case()
    B, iters = 4, 10
    em_means, em_trans = S.exact_em(obs, means0, trans0, iters)
    seeds = np.array([4242 + 1000 * b for b in range(B)], np.uint64)
    means, trans, ev = cp.hmm_table_em(engine, obs, np.tile(means0, (B, 1)), np.tile(trans0, (B, 1, 1)), 256, seeds, iters)
    assert means.shape == (iters + 1, B, 2) and trans.shape == (iters + 1, B, 2, 2) and ev.shape == (iters, B)
    dm = np.abs(means - em_means[:, None, :]).max(axis=2)          # [iterations + 1, B]
    dt = np.abs(trans - em_trans[:, None, :, :]).max(axis=(2, 3))
    for b in range(B):
        print("restart %d: means off by at most %.4f, transition rows by %.4f; log-evidence %.3f -> %.3f; fitted means %s"
              % (b, dm[:, b].max(), dt[:, b].max(), ev[0, b], ev[-1, b], means[-1, b]))
    assert dm.max() <= 0.05 and dt.max() <= 0.02, "means off by %.4f, transition rows by %.4f" % (dm.max(), dt.max())
    assert np.all(ev[-1] > ev[0])
    assert np.array_equal(means[0], np.tile(means0, (B, 1)))
