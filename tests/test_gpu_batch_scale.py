"""Per-state emission scales of MODEL_HMM_TABLE batches on the device (include/cpprob_hip.h: cpprob_hip_batch_begin_problems_scaled,
_begin_online_scaled, _retable_scaled*, _mstep_scaled_device, _copy_scales; csrc/batch_scale.hpp) against tests/scale_ref.py, against
the unit-scale batch where every sigma is 1.0, against a freshly begun scaled batch after a re-table, against the exact filter and
smoother, and the device-resident EM against the host loop."""
import math

import numpy as np
import pytest

import cpprob_amd as cp
import retable_ref as R
import scale_ref as S
from cpprob_amd import em
from test_scale_ref_host import exact_stats, mstep_cases

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -3, -4
MODES = {"history": dict(keep_history=True), "masses": dict(keep_history=False, keep_masses=True)}
RESAMPLERS = [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED]


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the batch the one under test is compared with."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _seeds(base, B):
    return np.array([base + 7919 * b for b in range(B)], np.uint64)


def _tables(B, k, seed):
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    sigmas = rng.uniform(0.3, 2.5, (B, k))
    return means, trans, sigmas


def _observes(Ts, k, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-3.0, 3.0 + 0.5 * k, T) + rng.standard_normal(T) for T in Ts]


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()                  # (the engine's stream is not ordered behind torch's)
    return t


def _readout(eng, mode, obs, scales=True):
    """Everything a run leaves, as nested lists of arrays."""
    B = len(obs)
    out = {"tables": [eng.batch_step_tables(b) for b in range(B)]}
    if scales:
        out["scales"] = [list(eng.batch_scales(b)) for b in range(B)]
    sums, stats, ess, res = eng.batch_results()
    out["summaries"] = [[s[f] for f in sorted(s)] for s in sums]
    out["results"] = [stats, ess, res]
    st = eng.batch_smooth_stats(obs)
    out["smooth_stats"] = [st[f] for f in sorted(st)]
    out["decode"] = list(eng.batch_decode())
    if mode == "history":
        out["store"] = [list(eng.batch_store(b)) for b in range(B)]
    else:
        out["masses"] = [eng.batch_masses(b) for b in range(B)]
    return out


def _assert_same(got, want, where=""):
    if isinstance(want, dict):
        assert sorted(got) == sorted(want)
        for key in want:
            _assert_same(got[key], want[key], where + "/" + key)
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _assert_same(g, w, "%s[%d]" % (where, i))
    elif want is None:
        assert got is None, where
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.shape == w.shape and g.dtype == w.dtype, where
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), "%s differs (%d of %d entries)" % (where, int(np.sum(g != w)), g.size)


def _code(call):
    with pytest.raises(cp.CpprobHipError) as e:
        call()
    return e.value.code, str(e.value)


# ---- 1. every sigma 1.0: the unit batch, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("resampler", RESAMPLERS)
@pytest.mark.parametrize("k", [2, 8])
def test_unit_scales_are_the_unit_batch(engine, ref_engine, k, resampler, mode):
    Ts, n = (1, 33, 40), 64
    obs = _observes(Ts, k, 3 + k)
    means, trans, _ = _tables(3, k, 7)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans, np.ones((3, k))), resampler=resampler, **MODES[mode])
    ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans), resampler=resampler, **MODES[mode])
    for eng in (engine, ref_engine):
        eng.batch_run(_seeds(11, 3))
    _assert_same(_readout(engine, mode, obs, scales=False), _readout(ref_engine, mode, obs, scales=False))
    for b in range(3):
        sg, ln = engine.batch_scales(b)
        assert np.array_equal(sg, np.ones(k)) and [v.hex() for v in ln] == [math.log(2 * math.pi).hex()] * k


# ---- 2. the scaled begin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5, 8])
def test_scaled_begin_writes_the_reference_rows(engine, k):
    Ts = (1, 33, 70)
    obs = _observes(Ts, k, 21)
    obs[2][5] = np.inf
    means, trans, sigmas = _tables(3, k, 22)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 64, tables=(means, trans, sigmas))
    for b in range(3):
        rows, thr = engine.batch_step_tables(b)
        assert np.array_equal(rows, S.rows(obs[b], means[b], sigmas[b], k))
        assert np.array_equal(thr, R.thresholds(trans[b], k))
        sg, ln = engine.batch_scales(b)
        assert np.array_equal(sg, sigmas[b]) and np.array_equal(ln, [S.log_norm(s) for s in sigmas[b]])


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("chunk", [1, 7])
def test_online_scaled_batch_in_chunks_is_the_one_shot_batch(engine, ref_engine, chunk, mode):
    k, n, caps = 3, 64, (9, 24, 16)
    obs = _observes(caps, k, 31)
    tables = _tables(3, k, 32)
    seeds = _seeds(77, 3)
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, caps, n, seeds, tables=tables, **MODES[mode])
    at = 0
    while at < max(caps):
        engine.batch_advance([o[at:at + chunk] for o in obs])
        at += chunk
        reached = [o[:at] for o in obs]
        ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, reached, n, tables=tables, **MODES[mode])
        ref_engine.batch_run(seeds)
        for b in range(3):
            _assert_same(list(engine.batch_step_tables(b)), list(ref_engine.batch_step_tables(b)), "tables[%d]" % b)
        got, want = engine.batch_results(), ref_engine.batch_results()
        for b in range(3):
            L = len(reached[b])
            assert got[0][b] == want[0][b]
            for g, w in zip(got[1:], want[1:]):
                assert np.array_equal(g[b, :L], w[b, :L])
    code, _ = _code(lambda: engine.batch_learn_begin(np.ones(max(caps)), 1))
    assert code == ESTATE                                     # (the arming comes before the first advance)


def test_a_bad_sigma_is_refused_and_the_batch_before_stays(engine):
    k, Ts = 3, (5, 9)
    obs = _observes(Ts, k, 41)
    means, trans, sigmas = _tables(2, k, 42)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 64, tables=(means, trans, sigmas))
    engine.batch_run(_seeds(5, 2))
    before = _readout(engine, "history", obs)
    for bad in (0.0, -1.0, np.nan, np.inf, 1e-170, 1e160):
        s2 = sigmas.copy()
        s2[1, 2] = bad
        for call in (lambda: engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 64, tables=(means, trans, s2)),
                     lambda: engine.batch_begin_online(cp.MODEL_HMM_TABLE, Ts, 64, _seeds(1, 2), tables=(means, trans, s2)),
                     lambda: engine.batch_retable((means, trans, s2), obs)):
            code, msg = _code(call)
            assert code == EINVAL and "problem 1" in msg, msg
    _assert_same(_readout(engine, "history", obs), before)


# ---- 3. the filter is right --------------------------------------------------------------------------------------------------------------
def test_scaled_filter_and_smoother_against_the_exact_ones(engine):
    """k = 3, two states with equal means told apart by their spread.  The SMC evidence is unbiased: over 32 seeds the mean of
    Z-hat / Z lies within 5 of its standard errors of 1.  E[Z-hat phi-hat] = Z phi for the smoother's marginals phi-hat as well (the
    unnormalised estimate is unbiased), so the mean of (Z-hat / Z) phi-hat lies within 5 standard errors of the exact marginal; and
    the plain mean of phi-hat, whose bias is -Cov(phi-hat, Z-hat / Z) by the same identity, within 5 standard errors plus
    sd(phi-hat) sd(Z-hat / Z) (Cauchy-Schwarz; both from the 32 runs).  The existing smoothing tests compare bits and hold no bias
    allowance at n = 256 that could be used here.  Measured: sd(Z-hat / Z) = 0.28; the largest plain-mean allowance over steps and
    states is 0.055 (5 standard errors 0.042, bias bound 0.013), the largest deviation 0.013."""
    k, T, n, runs = 3, 24, 256, 32
    means, sigmas = np.array([0.0, 0.0, 2.0]), np.array([0.3, 1.0, 2.5])
    trans = np.array([[0.8, 0.1, 0.1], [0.15, 0.7, 0.15], [0.2, 0.2, 0.6]])
    rng = np.random.default_rng(99)
    x, y = 0, np.zeros(T)
    for t in range(T):
        x = rng.choice(k, p=trans[x])
        y[t] = rng.normal(means[x], sigmas[x])
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, [y] * runs, n, tables=(np.tile(means, (runs, 1)), np.tile(trans, (runs, 1, 1)), np.tile(sigmas, (runs, 1))))
    engine.batch_run(_seeds(12345, runs))
    lz = np.array([s["log_evidence"] for s in engine.batch_results()[0]])
    marg = engine.batch_smooth()[0][:, :T, :k]
    # the exact filter and smoother (test_scale_ref_host.exact_stats returns sums; the marginals are restated here)
    _, occ, _, _, ll = exact_stats(y, means, trans, sigmas)
    from oracle import exact
    lik = np.exp(exact.normal_logpdf(y[:, None], means[None, :], sigmas[None, :]))
    alpha, c = np.zeros((T, k)), np.zeros(T)
    a = np.full(k, 1.0 / k) * lik[0]
    for t in range(T):
        if t:
            a = (alpha[t - 1] @ trans) * lik[t]
        c[t] = a.sum()
        alpha[t] = a / c[t]
    beta = np.ones((T, k))
    for t in range(T - 2, -1, -1):
        beta[t] = (trans @ (lik[t + 1] * beta[t + 1])) / c[t + 1]
    gamma = alpha * beta
    gamma /= gamma.sum(axis=1, keepdims=True)
    assert abs(np.log(c).sum() - ll) < 1e-9 and np.allclose(gamma.sum(axis=0), occ)
    r = np.exp(lz - ll)
    se = r.std(ddof=1) / math.sqrt(runs)
    print("mean Z-hat / Z = %.4f, standard error %.4f" % (r.mean(), se))
    assert abs(r.mean() - 1.0) <= 5.0 * se
    w = r[:, None, None] * marg
    assert np.all(np.abs(w.mean(axis=0) - gamma) <= 5.0 * w.std(axis=0, ddof=1) / math.sqrt(runs) + 1e-12)
    sd = marg.std(axis=0, ddof=1)
    print("plain mean: largest allowance %.4f (5 standard errors %.4f + bias bound %.4f), largest deviation %.4f"
          % ((5.0 * sd / math.sqrt(runs) + sd * r.std(ddof=1)).max(), (5.0 * sd / math.sqrt(runs)).max(), (sd * r.std(ddof=1)).max(), np.abs(marg.mean(axis=0) - gamma).max()))
    assert np.all(np.abs(marg.mean(axis=0) - gamma) <= 5.0 * sd / math.sqrt(runs) + sd * r.std(ddof=1) + 1e-12)


# ---- 4. re-tabling ---------------------------------------------------------------------------------------------------------------------
def _retable(eng, form, tables, obs):
    if form == "host":
        eng.batch_retable(tables, obs)
    else:
        eng.batch_retable_device(_dev(tables[0]), _dev(tables[1]), _dev(np.concatenate(obs)), sigmas=_dev(tables[2]))
        eng.sync()


RETABLE_CASES = [(k, form, mode) for k in (2, 5, 8) for form in ("host", "device") for mode in sorted(MODES)]


@pytest.mark.parametrize("k,form,mode", RETABLE_CASES, ids=["k%d-%s-%s" % c for c in RETABLE_CASES])
def test_scaled_retable_equals_a_fresh_scaled_begin(engine, ref_engine, k, form, mode):
    Ts, n = (1, 33, 70), 64
    resampler = RESAMPLERS[RETABLE_CASES.index((k, form, mode)) % 2]
    obs = _observes(Ts, k, 50 + k)
    A, Bt = _tables(3, k, 51), _tables(3, k, 52)
    S2 = _seeds(900, 3)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=A, resampler=resampler, **MODES[mode])
    engine.batch_run(_seeds(5, 3))
    _retable(engine, form, Bt, obs)
    assert engine.batch_retable_grid() == R.grid_y(max(Ts), 3) == 3 and not engine.batch_retable_status().any()
    engine.batch_run(S2)
    ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=Bt, resampler=resampler, **MODES[mode])
    ref_engine.batch_run(S2)
    _assert_same(_readout(engine, mode, obs), _readout(ref_engine, mode, obs))


@pytest.mark.parametrize("form", ["host", "device"])
def test_scaled_retable_where_a_workgroup_walks_several_tiles(engine, ref_engine, form):
    """B = 1, T = 2100: 66 tiles of 32 rows over the grid's cap of 64 workgroups -- the first two walk two tiles."""
    k, T, n = 5, 2100, 64
    obs = _observes((T,), k, 61)
    A, Bt = _tables(1, k, 62), _tables(1, k, 63)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=A, keep_history=False, keep_masses=True)
    _retable(engine, form, Bt, obs)
    assert engine.batch_retable_grid() == R.GRID_MAX == 64 and (T + R.ROWS_PER_TRIP - 1) // R.ROWS_PER_TRIP > R.GRID_MAX
    rows, thr = engine.batch_step_tables(0)
    assert np.array_equal(rows, S.rows(obs[0], Bt[0][0], Bt[2][0], k)) and np.array_equal(thr, R.thresholds(Bt[1][0], k))
    engine.batch_run(_seeds(3, 1))
    ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=Bt, keep_history=False, keep_masses=True)
    ref_engine.batch_run(_seeds(3, 1))
    _assert_same(_readout(engine, "masses", obs), _readout(ref_engine, "masses", obs))


def test_a_bad_sigma_on_the_device_keeps_the_old_table(engine, ref_engine):
    k, Ts, n = 5, (1, 33, 70), 64
    obs = _observes(Ts, k, 71)
    A, Bt = _tables(3, k, 72), _tables(3, k, 73)
    bad = tuple(a.copy() for a in Bt)
    bad[2][1, 3] = 1e-170                                     # (2 pi sigma^2 underflows)
    mixed = tuple(a.copy() for a in Bt)
    for a, old in zip(mixed, A):
        a[1] = old[1]
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=A)
    _retable(engine, "device", bad, obs)
    assert list(engine.batch_retable_status()) == [0, S.BAD_SCALE, 0]
    engine.batch_run(_seeds(8, 3))
    ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=mixed)
    ref_engine.batch_run(_seeds(8, 3))
    _assert_same(_readout(engine, "history", obs), _readout(ref_engine, "history", obs))
    for nonfinite in (np.nan, np.inf, 0.0, -2.0):
        bad[2][1, 3] = nonfinite
        _retable(engine, "device", bad, obs)
        assert list(engine.batch_retable_status()) == [0, S.BAD_SCALE, 0]
    bad[0][1, 0], bad[1][1, 2, :] = np.nan, 0.0
    _retable(engine, "device", bad, obs)
    assert list(engine.batch_retable_status()) == [0, S.BAD_SCALE | R.BAD_MEAN | R.NO_MASS, 0]


def test_unit_and_scaled_calls_do_not_mix(engine):
    k, Ts = 3, (4, 6)
    obs = _observes(Ts, k, 81)
    means, trans, sigmas = _tables(2, k, 82)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 64, tables=(means, trans, sigmas))
    assert _code(lambda: engine.batch_retable((means, trans), obs))[0] == ESTATE
    assert _code(lambda: engine.batch_retable_device(_dev(means), _dev(trans), _dev(np.concatenate(obs))))[0] == ESTATE
    rows = [engine.batch_step_tables(b)[0] for b in range(2)]
    assert all(np.array_equal(rows[b], S.rows(obs[b], means[b], sigmas[b], k)) for b in range(2))
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 64, tables=(means, trans))
    assert _code(lambda: engine.batch_retable((means, trans, sigmas), obs))[0] == ESTATE
    assert _code(lambda: engine.batch_retable_device(_dev(means), _dev(trans), _dev(np.concatenate(obs)), sigmas=_dev(sigmas)))[0] == ESTATE
    assert _code(lambda: engine.batch_scales(0, k))[0] == ESTATE
    assert np.array_equal(engine.batch_step_tables(0)[0], R.rows(obs[0], means[0], k, math.log(2 * math.pi)))


# ---- 5. the M-step kernel (and the device's square root) -------------------------------------------------------------------------------
def _mstep_device(engine, recs, means, trans, sigmas, floor):
    import torch
    m, t, s, ln = _dev(means), _dev(trans), _dev(sigmas), _dev(np.full(sigmas.shape, -7.0))
    engine.batch_mstep_device(_dev(recs), m, t, sigmas=s, sigma_floor=floor, log_norms=ln)
    engine.sync()
    torch.cuda.synchronize()
    return m.cpu().numpy(), t.cpu().numpy(), s.cpu().numpy(), ln.cpu().numpy()


@pytest.mark.parametrize("k", [2, 5, 8])
def test_mstep_kernel_on_the_records_of_a_run(engine, k):
    B, n = 6, 256
    obs = _observes([40 + 3 * b for b in range(B)], k, 91)
    means, trans, sigmas = _tables(B, k, 92)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans, sigmas))
    engine.batch_run(_seeds(17, B))
    st = engine.batch_smooth_stats(obs)
    recs = np.concatenate([st["xi"].reshape(B, 64), st["occ"], st["occ_y"], st["occ_yy"]], axis=1)
    floor = 1e-3
    m, t, s, ln = _mstep_device(engine, recs, means, trans, sigmas, floor)
    for b in range(B):
        wm, ws, wl, wt = S.m_step(recs[b], means[b], sigmas[b], np.full(k, -7.0), trans[b], k, floor)
        assert np.array_equal(m[b], wm) and np.array_equal(t[b], wt)
        assert np.array_equal(s[b], ws), (s[b] - ws)           # (the device's square root is numpy's, bit for bit)
        assert np.array_equal(ln[b], wl)
    hm, ht, hs = em.m_step(st, means, trans, sigmas, floor)
    assert np.array_equal(hm, m) and np.array_equal(ht, t) and np.array_equal(hs, s)


def test_mstep_kernel_on_the_constructed_records(engine):
    cases = mstep_cases()
    obs = _observes((3, 3), 2, 95)
    for name, rec, means, sigmas, trans, floor in cases:
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 64, tables=(np.tile(means, (2, 1)), np.tile(trans, (2, 1, 1)), np.tile(sigmas, (2, 1))))
        m, t, s, ln = _mstep_device(engine, np.tile(rec, (2, 1)), np.tile(means, (2, 1)), np.tile(trans, (2, 1, 1)), np.tile(sigmas, (2, 1)), floor)
        wm, ws, wl, wt = S.m_step(rec, means, sigmas, np.full(2, -7.0), trans, 2, floor)
        for b in range(2):
            assert np.array_equal(m[b], wm) and np.array_equal(t[b], wt) and np.array_equal(s[b], ws) and np.array_equal(ln[b], wl, equal_nan=True), name
    assert _code(lambda: _mstep_device(engine, np.tile(cases[0][1], (2, 1)), np.zeros((2, 2)), np.ones((2, 2, 2)), np.ones((2, 2)), 0.0))[0] == EINVAL


# ---- 6. device-resident EM ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
def test_resident_scaled_em_is_the_host_loop(engine, mode):
    B, k, T, n, iters = 4, 3, 40, 64, 3
    rng = np.random.default_rng(7)
    obs = [np.where(rng.random(T) < 0.5, rng.normal(-2.0, 0.5, T), rng.normal(2.0, 2.0, T)) for _ in range(B)]
    means, trans, _ = _tables(B, k, 101)
    sigmas0 = np.ones((B, k))
    seeds = _seeds(300, B)
    kw = dict(keep_history=mode == "history", sigmas0=sigmas0, sigma_floor=1e-3)
    host = em.hmm_table_em(engine, obs, means, trans, n, seeds, iters, **kw)
    res = em.hmm_table_em(engine, obs, means, trans, n, seeds, iters, resident=True, **kw)
    assert len(host) == len(res) == 4 and host[3].shape == (iters + 1, B, k)
    for h, r in zip(host, res):
        assert h.shape == r.shape and np.array_equal(h, r)
    assert not np.array_equal(host[3][-1], sigmas0)
    # without sigmas0 the call returns what it returned
    plain = em.hmm_table_em(engine, obs, means, trans, n, seeds, 1, keep_history=mode == "history")
    assert len(plain) == 3


# ---- the fitting and labelling helpers carry the scales ----------------------------------------------------------------------------------
def test_helpers_with_scales(engine, ref_engine):
    """hmm_table_decode(sigmas=) is a scaled begin, run and decode; the Gibbs samplers with sigmas0 return a chain of sigmas and are
    the same chains bit for bit with retable=True; without sigmas0 they return what they returned."""
    from cpprob_amd import decode, gibbs, pgibbs
    B, k, n = 3, 2, 64
    obs = _observes((20, 33, 40), k, 111)
    means, trans, sigmas = _tables(B, k, 112)
    seeds = _seeds(50, B)
    paths, scores, ev = decode.hmm_table_decode(engine, obs, means, trans, n, seeds, sigmas=sigmas)
    ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans, sigmas))
    ref_engine.batch_run(seeds)
    _assert_same([paths, scores], list(ref_engine.batch_decode()))
    assert np.array_equal(ev, [s["log_evidence"] for s in ref_engine.batch_results()[0]])
    for fit in (gibbs.hmm_table_gibbs, pgibbs.hmm_table_particle_gibbs):
        a = fit(engine, obs, means, trans, n, seeds, 3, np.random.default_rng(1), sigmas0=sigmas)
        b = fit(engine, obs, means, trans, n, seeds, 3, np.random.default_rng(1), sigmas0=sigmas, retable=True)
        plain = fit(engine, obs, means, trans, n, seeds, 1, np.random.default_rng(1))
        assert len(a) == len(plain) + 1 and a[-1].shape == (4, B, k) and np.all(a[-1] > 0.0) and not np.array_equal(a[-1][1], sigmas)
        _assert_same(list(a), list(b), fit.__name__)
