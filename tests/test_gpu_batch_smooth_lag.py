"""Fixed-lag smoothing of a batch (include/cpprob_hip.h: cpprob_hip_batch_smooth_lag, _smooth_lag_device; csrc/batch_smooth.hpp)
against tests/lag_ref.py on the rows the run left (cpprob_hip_batch_copy_store), as tests/test_gpu_batch_smooth.py::_reference does.
Marginals within 1e-12 absolute of the reference (that file's derivation: at most T k^2 operations of 2^-52 relative on quantities
<= 1); trajectories array_equal; the rows whose end is the last step array_equal to the device's own cpprob_hip_batch_smooth (one
device function walks both); an online batch's rows array_equal however it was cut into advances."""
import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import lag_ref as G
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


def _masses(engine, b, obs_b, means, trans):
    """(m, P) of problem b from the rows its run left."""
    vals, _, logw = engine.batch_store(b)
    ll = R.log_likelihoods(obs_b, means)
    assert np.all(logw == np.array(ll[-1])[vals[-1]]), "problem %d: restated log-likelihoods differ from the run's table" % b
    return R.filtering_masses(vals, ll), R.transition_masses(trans)


def _assert_rows(what, b, marg_b, ref_g, frm, k):
    """marg_b [n_rows, spp] against rows frm .. of the reference, its padding zero."""
    rows = ref_g.shape[0] - frm
    err = float(np.abs(marg_b[:rows, :k] - ref_g[frm:]).max()) if rows else 0.0
    print("%s problem %d: rows %d .. %d, largest marginal difference %.3g" % (what, b, frm, ref_g.shape[0], err))
    assert err <= TOL, "%s problem %d: marginals differ from the reference by %.3g" % (what, b, err)
    assert np.all(marg_b[rows:] == 0.0) and np.all(marg_b[:, k:] == 0.0), "%s problem %d: padding is not zero" % (what, b)


# ---- 1. described batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("k", [2, 3, 5, 7, 8])
def test_described_table_batch(engine, k, rs):
    Ts, ns, M = [1, 2, 7, 23], [1, 300, 777, 1025], 33
    B = len(Ts)
    means, trans = _tables(k, B, 31 + k)
    obs = _table_observes(means, Ts, 31 + k)
    seeds = _seeds(B, 19 + k)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans), resampler=rs)
    engine.batch_run(seeds)
    mp = [_masses(engine, b, obs[b], means[b], trans[b]) for b in range(B)]
    full = {di: engine.batch_smooth(M, di) for di in (0, 3)}
    ref_x = {di: [R.trajectories_fast(m, P, int(seeds[b]), M, di) for b, (m, P) in enumerate(mp)] for di in (0, 3)}
    for di in (0, 3):
        for b in range(B):
            assert np.array_equal(full[di][1][b], ref_x[di][b]), (di, b)
    for lag in (0, 1, 3, 64):
        ref_g = [G.fixed_lag_marginals(m, P, lag) for m, P in mp]
        W = [min(lag + 1, T) for T in Ts]
        for frm in (None, [1, 0, 7, 20]):
            f = frm or [0] * B
            what = "k = %d, lag = %d, from = %s," % (k, lag, frm)
            marg, traj = engine.batch_smooth_lag(lag, frm, M, 3)
            assert marg.shape == (B, max(T - x for T, x in zip(Ts, f)), 8) and len(traj) == B
            for b in range(B):
                _assert_rows(what, b, marg[b], ref_g[b], f[b], k)
                # the rows whose end is the last step: the full smoother's own bits
                lo = max(Ts[b] - W[b], f[b])
                assert np.array_equal(marg[b, lo - f[b]:Ts[b] - f[b]], full[3][0][b, lo:Ts[b]]), "%s problem %d: tail rows differ from batch_smooth's" % (what, b)
                assert traj[b].dtype == np.int32 and traj[b].shape == (W[b], M)
                assert np.array_equal(traj[b], full[3][1][b][Ts[b] - W[b]:]), "%s problem %d: window differs from batch_smooth's last rows" % (what, b)
                assert np.array_equal(traj[b], ref_x[3][b][Ts[b] - W[b]:]), "%s problem %d: window differs from the reference" % (what, b)
        _, traj0 = engine.batch_smooth_lag(lag, None, M, 0)
        for b in range(B):
            assert np.array_equal(traj0[b], full[0][1][b][Ts[b] - W[b]:]) and np.array_equal(traj0[b], ref_x[0][b][Ts[b] - W[b]:]), (lag, b)
    marg64, _ = engine.batch_smooth_lag(64)
    assert np.array_equal(marg64, full[0][0]), "lag = 64 is not batch_smooth's marginals"
    # the marginals alone and the trajectories alone, through the C ABI
    first = cp.capi.batch_smooth_layout([min(4, T) for T in Ts], M)
    flat = np.full(int(first[-1]), -5, np.int32)
    assert engine.L.cpprob_hip_batch_smooth_lag(engine.h, 3, None, 0, M, 3, None, 0, flat.ctypes.data, flat.size) == 0
    _, traj3 = engine.batch_smooth_lag(3, None, M, 3)
    assert np.array_equal(flat, np.concatenate([x.reshape(-1) for x in traj3]))


# ---- 2. uniform batch ------------------------------------------------------------------------------------------------------------
def test_uniform_hmm3_batch(engine):
    B, T, n, lag, M = 3, 16, 4099, 2, 1025
    obs = [exact.simulate_hmm(T, 900 + b) for b in range(B)]
    seeds = _seeds(B, 3 + n)
    engine.batch_begin(cp.MODEL_HMM3, np.array(obs), n)
    engine.batch_run(seeds)
    marg, traj = engine.batch_smooth_lag(lag, None, M)
    full_m, full_x = engine.batch_smooth(M)
    assert marg.shape == (B, T, 3)
    for b in range(B):
        m, P = _masses(engine, b, obs[b], exact.HMM_MEAN, exact.HMM_T)
        _assert_rows("uniform,", b, marg[b], G.fixed_lag_marginals(m, P, lag), 0, 3)
        assert np.array_equal(marg[b, T - 3:], full_m[b, T - 3:])
        assert np.array_equal(traj[b], G.window_trajectories(m, P, int(seeds[b]), M, lag)) and np.array_equal(traj[b], full_x[b][T - 3:])


# ---- 3. a batch advanced in pieces -----------------------------------------------------------------------------------------------
def _cuts(name, reach):
    """Per-advance pieces [dT_0, dT_1, dT_2] that take the three problems from length 0 to `reach`."""
    if name == "ones":
        return [[1 if a < reach[b] else 0 for b in range(3)] for a in range(max(reach))]
    if name == "mixed":           # advances larger than lag + 1, and empty ones
        pattern = [5, 0, 9, 1, 0, 12, 2, 0, 7, 1, 30]
    else:                         # different cuts a problem
        pattern = None
    out, at = [], [0, 0, 0]
    per = [[3, 11, 0, 1, 40], [0, 1, 1, 6, 2, 40], [2, 0, 0, 1, 40]]
    a = 0
    while at != list(reach):
        dT = [min((pattern[a % len(pattern)] if pattern else per[b][min(a, len(per[b]) - 1)]), reach[b] - at[b]) for b in range(3)]
        out.append(dT)
        at = [at[b] + dT[b] for b in range(3)]
        a += 1
    return out


@pytest.mark.parametrize("cut", ["ones", "mixed", "ragged"])
@pytest.mark.parametrize("model,k", [(cp.MODEL_HMM3, 3), (cp.MODEL_HMM_TABLE, 8)])
def test_online_rows_do_not_depend_on_the_cuts(engine, ref_engine, model, k, cut):
    caps, ns, lag, M = [40, 40, 12], [300, 7, 1025], 3, 33
    if model == cp.MODEL_HMM3:
        tables, obs = None, [exact.simulate_hmm(c, 60 + b) for b, c in enumerate(caps)]
        means, trans = [exact.HMM_MEAN] * 3, [exact.HMM_T] * 3
    else:
        means, trans = _tables(k, 3, 41)
        tables, obs = (means, trans), _table_observes(means, caps, 41)
    spp = 3 if model == cp.MODEL_HMM3 else 8

    def one_shot(lens, seeds):
        idx = [b for b in range(3) if lens[b] >= 1]
        tb = None if tables is None else (means[idx], trans[idx])
        ref_engine.batch_begin_problems(model, [obs[b][:lens[b]] for b in idx], [ns[b] for b in idx], tables=tb)
        ref_engine.batch_run(seeds[idx])
        return idx, ref_engine.batch_smooth_lag(lag, None, M), ref_engine.batch_smooth(M)

    def stream(seeds, base):
        """Feeds the cuts up to [37, 22, 0] and then [40, 30, 5]; returns the series assembled advance by advance at both lengths."""
        engine.batch_begin_online(model, caps, ns, seeds, tables=tables)
        lens, series = [0, 0, 0], np.zeros((3, max(caps), spp))
        for stage, reach in enumerate(([37, 22, 0], [40, 30, 5])):
            left = [reach[b] - lens[b] for b in range(3)]
            for a, dT in enumerate(_cuts(cut, left)):
                frm = [max(0, lens[b] - lag) for b in range(3)]
                engine.batch_advance([obs[b][lens[b]:lens[b] + dT[b]] for b in range(3)], readout=(a % 2 == 0))
                lens = [lens[b] + dT[b] for b in range(3)]
                marg, _ = engine.batch_smooth_lag(lag, frm)
                for b in range(3):
                    series[b, frm[b]:lens[b]] = marg[b, :lens[b] - frm[b]]
                    assert np.all(marg[b, lens[b] - frm[b]:] == 0.0)
            assert lens == reach
            whole, win = engine.batch_smooth_lag(lag, None, M)
            full_m, full_x = engine.batch_smooth(M)                      # the existing call, over the cached table
            idx, (ref_m, ref_w), (ref_fm, ref_fx) = one_shot(lens, seeds)
            for b in range(3):
                what = "%s stage %d, problem %d" % (base, stage, b)
                assert np.array_equal(series[b, :lens[b]], whole[b, :lens[b]]), what + ": the assembled rows are not the one call's"
                assert np.all(whole[b, lens[b]:] == 0.0), what
                if lens[b] == 0:
                    assert win[b].shape == (0, M) and full_x[b].shape == (0, M) and np.all(full_m[b] == 0.0)
                    continue
                i = idx.index(b)
                assert np.array_equal(whole[b, :lens[b]], ref_m[i, :lens[b]]), what + ": differs from the one-shot batch"
                assert np.array_equal(win[b], ref_w[i]), what + ": window differs from the one-shot batch"
                assert np.array_equal(full_m[b, :lens[b]], ref_fm[i, :lens[b]]) and np.array_equal(full_x[b], ref_fx[i]), what + ": batch_smooth differs from the one-shot batch"
                m, P = _masses(engine, b, obs[b][:lens[b]], means[b], trans[b])
                _assert_rows(what, b, whole[b, :lens[b]], G.fixed_lag_marginals(m, P, lag), 0, k)
                assert np.array_equal(win[b], G.window_trajectories(m, P, int(seeds[b]), M, lag)), what
        return series

    first = stream(_seeds(3, 11), "first batch,")
    # the same context again, other seeds: nothing of the first batch's table may survive
    second = stream(_seeds(3, 501), "second batch,")
    assert not np.array_equal(first, second)


# ---- 4. a window longer than the staged rows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", [599, 520])
def test_long_window_reads_its_masses_from_memory(engine, lag):
    """W = 600 and W = 521 rows of 64 bytes exceed the 32 KiB a tile stages; the short problem beside it is staged."""
    Ts, ns, M = [600, 5], [64, 260], 33
    obs = [exact.simulate_hmm(T, 40 + b) for b, T in enumerate(Ts)]
    seeds = _seeds(2, 5)
    engine.batch_begin_problems(cp.MODEL_HMM3, obs, ns)
    engine.batch_run(seeds)
    marg, traj = engine.batch_smooth_lag(lag, None, M)
    full_m, full_x = engine.batch_smooth(M)
    for b in range(2):
        m, P = _masses(engine, b, obs[b], exact.HMM_MEAN, exact.HMM_T)
        W = min(lag + 1, Ts[b])
        _assert_rows("lag %d," % lag, b, marg[b], G.fixed_lag_marginals(m, P, lag), 0, 3)
        assert np.array_equal(marg[b, Ts[b] - W:Ts[b]], full_m[b, Ts[b] - W:Ts[b]])
        assert traj[b].shape == (W, M) and np.array_equal(traj[b], full_x[b][Ts[b] - W:])
        assert np.array_equal(traj[b], G.window_trajectories(m, P, int(seeds[b]), M, lag))


# ---- 5. the device variant, and what the call leaves alone -----------------------------------------------------------------------
def test_device_variant_and_untouched_results(engine):
    import torch
    Ts, ns, M, lag, di = [1, 2, 7, 23], [1, 300, 777, 1025], 33, 3, 1
    frm = [1, 0, 2, 20]
    B = len(Ts)
    means, trans = _tables(8, B, 39)
    obs = _table_observes(means, Ts, 39)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans))
    engine.batch_run(_seeds(B, 29))
    before = (engine.batch_results(), [engine.batch_store(b) for b in range(B)], engine.batch_paths(), engine.batch_smooth(M, di))
    marg, traj = engine.batch_smooth_lag(lag, frm, M, di)
    n_rows = marg.shape[1] + 2                                           # more rows than needed: zero
    first = cp.capi.batch_smooth_layout([min(lag + 1, T) for T in Ts], M)
    n_entries, n_doubles, pad = int(first[-1]), B * n_rows * 8, 256
    d_traj = torch.full((n_entries + 2 * pad,), -9, dtype=torch.int8, device="cuda:0")
    d_marg = torch.full((n_doubles + 2 * pad,), 12345.5, dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_smooth_lag_device(lag, frm, d_marg[pad:pad + n_doubles].view(B, n_rows, 8), d_traj[pad:pad + n_entries], n_traj=M, draw_index=di)
    engine.sync()
    got_x, got_m = d_traj.cpu().numpy(), d_marg.cpu().numpy()
    assert np.all(got_x[:pad] == -9) and np.all(got_x[pad + n_entries:] == -9)
    assert np.all(got_m[:pad] == 12345.5) and np.all(got_m[pad + n_doubles:] == 12345.5)
    assert np.array_equal(got_x[pad:pad + n_entries].astype(np.int32), np.concatenate([x.reshape(-1) for x in traj]))
    got_m = got_m[pad:pad + n_doubles].reshape(B, n_rows, 8)
    assert np.array_equal(got_m[:, :n_rows - 2], marg) and np.all(got_m[:, n_rows - 2:] == 0.0)
    after = (engine.batch_results(), [engine.batch_store(b) for b in range(B)], engine.batch_paths(), engine.batch_smooth(M, di))
    assert before[0][0] == after[0][0]
    assert all(np.array_equal(x, y) for x, y in zip(before[0][1:], after[0][1:]))
    assert all(np.array_equal(x, y) for sb, sa in zip(before[1], after[1]) for x, y in zip(sb, sa))
    assert all(np.array_equal(x, y) for pb, pa in zip(before[2], after[2]) for x, y in zip(pb, pa))
    assert np.array_equal(before[3][0], after[3][0]) and all(np.array_equal(x, y) for x, y in zip(before[3][1], after[3][1]))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_lag_refusals():
    import ctypes as C
    import torch  # noqa: F401
    eng = cp.Engine(0)
    u32 = C.POINTER(C.c_uint32)
    try:
        with pytest.raises(cp.CpprobHipError) as e:
            eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K, eng.batch_shapes = 1, 1, 1, 3, None
            eng.batch_smooth_lag(2)
        assert e.value.code == ESTATE
        obs = [exact.simulate_hmm(T, 70 + b) for b, T in enumerate([3, 2])]
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20])
        with pytest.raises(cp.CpprobHipError) as e:          # begun, not run
            eng.batch_smooth_lag(2)
        assert e.value.code == ESTATE
        eng.batch_run(_seeds(2))
        M, lag, n_rows = 4, 1, 3
        need_m, need_x = 2 * n_rows * 3, M * (2 + 2)
        marg = np.full(need_m, -5.0)
        traj = np.full(need_x, -5, np.int32)

        def call(lag=lag, frm=None, n_rows=n_rows, M=M, di=0, n_m=need_m, n_x=need_x):
            p = None if frm is None else np.array(frm, np.uint32).ctypes.data_as(u32)
            return eng.L.cpprob_hip_batch_smooth_lag(eng.h, lag, p, n_rows, M, di, marg.ctypes.data, n_m, traj.ctypes.data, n_x)

        def untouched():
            return bool(np.all(marg == -5.0) and np.all(traj == -5))
        for what, kw in (("from past the length", dict(frm=[0, 3])), ("n_rows too small", dict(n_rows=2, n_m=2 * 2 * 3)), ("lag", dict(lag=(1 << 24) + 1)),
                         ("marginals capacity", dict(n_m=need_m - 1)), ("trajectories capacity", dict(n_x=need_x - 1)), ("draw_index", dict(di=1 << 16)),
                         ("n_traj", dict(M=(1 << 20) + 1))):
            assert call(**kw) == EINVAL and untouched(), what
        assert call(frm=[0, 3]) == EINVAL and b"problem 1" in eng.L.cpprob_hip_last_error(eng.h)
        assert call(n_rows=2, n_m=12) == EINVAL and b"problem 0" in eng.L.cpprob_hip_last_error(eng.h)
        assert call(frm=[3, 2], n_rows=0, n_m=0) == 0 and np.all(marg == -5.0)       # from_b = L_b: no rows
        assert np.all((traj >= 0) & (traj < 3))
        traj[:] = -5
        assert call() == 0
        assert np.all(marg >= 0.0) and np.all((traj >= 0) & (traj < 3))
        d = torch.full((need_x,), -9, dtype=torch.int8, device="cuda:0")
        torch.cuda.current_stream().synchronize()
        rc = eng.L.cpprob_hip_batch_smooth_lag_device(eng.h, lag, None, n_rows, M, 0, None, 0, C.c_void_p(d.data_ptr()), need_x - 1)
        eng.sync()
        assert rc == EINVAL and bool((d == -9).all())
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20], keep_history=False)
        eng.batch_run(_seeds(2))
        with pytest.raises(cp.CpprobHipError) as e:
            eng.batch_smooth_lag(2)
        assert e.value.code == ESTATE and "keep_history" in str(e.value)
    finally:
        eng.close()
