"""Poisson emissions of MODEL_HMM_TABLE batches on the device (include/cpprob_hip.h: cpprob_hip_batch_begin_problems_poisson,
_begin_online_poisson, _retable_poisson*, _mstep_poisson_device, _online_tables_poisson, _copy_rates; csrc/batch_poisson.hpp) against
tests/poisson_ref.py, against a freshly begun Poisson batch after a re-table, against the exact filter and smoother, the device-resident EM
against the host loop, and the tied fit of eight recordings against Baum-Welch on their pooled exact statistics."""
import math

import numpy as np
import pytest

import cpprob_amd as cp
import poisson_ref as P
import retable_ref as R
import scale_ref as S
from cpprob_amd import em
from test_gpu_batch_scale import MODES, RESAMPLERS, _assert_same, _code, _dev, _seeds
from test_poisson_ref_host import INVALID, fused_pairs, mstep_cases

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -3, -4
TS, N = (1, 33, 70), 64


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the batch the one under test is compared with."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _tables(B, k, seed):
    rng = np.random.default_rng(seed)
    rates = np.sort(np.exp(rng.uniform(-1.0, 3.0, (B, k))), axis=1)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    return rates, trans


def _observes(Ts, seed):
    rng = np.random.default_rng(seed)
    return [rng.poisson(rng.choice([0.7, 3.0, 9.0, 20.0], T)).astype(np.float64) for T in Ts]


def _readout(eng, mode, obs):
    """What tests/test_gpu_batch_scale.py's _readout compares, with the rates in force where it has the scales."""
    B = len(obs)
    out = {"tables": [eng.batch_step_tables(b) for b in range(B)], "rates": [list(eng.batch_copy_rates(b)) for b in range(B)]}
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


def _begin(eng, obs, tables, mode="history", resampler=cp.RESAMPLE_SYSTEMATIC, n=N):
    eng.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=tables, resampler=resampler, emission="poisson", **MODES[mode])


# ---- 1. the begin ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5, 8])
def test_poisson_begin_writes_the_reference_rows(engine, k):
    """Three problems of 1, 33 and 70 counts, the last with the (count, rate) pairs at which a fused row would differ, and a fourth whose
    observes are no counts: its rows are -inf as the reference's; it is never run."""
    obs = _observes(TS, 21) + [np.array(INVALID + [0.0, 4095.0, 7.0])]
    rates, trans = _tables(4, k, 22)
    pairs = fused_pairs()
    rates[2] = [r for _, r in pairs[:k]]
    obs[2][:k] = [y for y, _ in pairs[:k]]
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=(rates, trans), emission="poisson")
    for b in range(4):
        rows, thr = engine.batch_step_tables(b)
        assert np.array_equal(rows, P.rows(obs[b], rates[b], k)), b
        assert np.array_equal(thr, R.thresholds(trans[b], k))
        rt, lr = engine.batch_copy_rates(b)
        assert np.array_equal(rt, rates[b]) and np.array_equal(lr, [S.table_log(r) for r in rates[b]])
    rows = engine.batch_step_tables(3)[0]
    assert np.all(np.isneginf(rows[:len(INVALID)])) and np.all(np.isfinite(rows[len(INVALID):, :k]))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("chunk", [1, 5, 70])
def test_online_poisson_batch_in_chunks_is_the_one_shot_batch(engine, ref_engine, chunk, mode):
    k = 5
    resampler = RESAMPLERS[(chunk + len(mode)) % 2]
    obs = _observes(TS, 31)
    tables = _tables(3, k, 32)
    seeds = _seeds(77, 3)
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, TS, N, seeds, tables=tables, resampler=resampler, emission="poisson", **MODES[mode])
    at = 0
    while at < max(TS):
        engine.batch_advance([o[at:at + chunk] for o in obs])
        at += chunk
        if chunk == 1 and at not in (1, 2, 33, 34, 70):
            continue                                          # (the one-shot batch at the lengths where a problem ends, and at the ends)
        reached = [o[:at] for o in obs]
        _begin(ref_engine, reached, tables, mode, resampler)
        ref_engine.batch_run(seeds)
        for b in range(3):
            _assert_same(list(engine.batch_step_tables(b)), list(ref_engine.batch_step_tables(b)), "tables[%d]" % b)
        got, want = engine.batch_results(), ref_engine.batch_results()
        for b in range(3):
            L = len(reached[b])
            assert got[0][b] == want[0][b]
            for g, w in zip(got[1:], want[1:]):
                assert np.array_equal(g[b, :L], w[b, :L])
    for b in range(3):
        assert np.array_equal(engine.batch_step_tables(b)[0], P.rows(obs[b], tables[0][b], k))


def test_online_tables_poisson_serve_the_future_steps(engine):
    k, caps = 3, (6, 9)
    obs = _observes(caps, 35)
    A, Bt = _tables(2, k, 36), _tables(2, k, 37)
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, caps, N, _seeds(3, 2), tables=A, emission="poisson")
    engine.batch_advance([o[:4] for o in obs])
    engine.batch_online_tables(Bt, emission="poisson")
    engine.batch_advance([o[4:] for o in obs])
    for b in range(2):
        want = np.concatenate([P.rows(obs[b][:4], A[0][b], k), P.rows(obs[b][4:], Bt[0][b], k)])
        assert np.array_equal(engine.batch_step_tables(b)[0], want)
        assert np.array_equal(engine.batch_copy_rates(b)[0], Bt[0][b])


# ---- 2. re-tabling -----------------------------------------------------------------------------------------------------------------------
def _retable(eng, form, tables, obs):
    if form == "host":
        eng.batch_retable(tables, obs, emission="poisson")
    else:
        eng.batch_retable_device(_dev(tables[0]), _dev(tables[1]), _dev(np.concatenate(obs)), emission="poisson")
        eng.sync()


RETABLE_CASES = [(k, form, mode) for k in (2, 5, 8) for form in ("host", "device") for mode in sorted(MODES)]


@pytest.mark.parametrize("k,form,mode", RETABLE_CASES, ids=["k%d-%s-%s" % c for c in RETABLE_CASES])
def test_poisson_retable_equals_a_fresh_poisson_begin(engine, ref_engine, k, form, mode):
    resampler = RESAMPLERS[RETABLE_CASES.index((k, form, mode)) % 2]
    obs = _observes(TS, 50 + k)
    A, Bt = _tables(3, k, 51), _tables(3, k, 52)
    S2 = _seeds(900, 3)
    _begin(engine, obs, A, mode, resampler)
    engine.batch_run(_seeds(5, 3))
    _retable(engine, form, Bt, obs)
    assert engine.batch_retable_grid() == R.grid_y(max(TS), 3) == 3 and not engine.batch_retable_status().any()
    engine.batch_run(S2)
    _begin(ref_engine, obs, Bt, mode, resampler)
    ref_engine.batch_run(S2)
    _assert_same(_readout(engine, mode, obs), _readout(ref_engine, mode, obs))


def test_a_bad_rate_on_the_device_keeps_the_old_table(engine, ref_engine):
    k = 5
    obs = _observes(TS, 71)
    A, Bt = _tables(3, k, 72), _tables(3, k, 73)
    bad = tuple(a.copy() for a in Bt)
    bad[0][1, 3] = 1e-310                                     # (a subnormal rate: no argument for table_log)
    mixed = tuple(a.copy() for a in Bt)
    for a, old in zip(mixed, A):
        a[1] = old[1]
    _begin(engine, obs, A)
    _retable(engine, "device", bad, obs)
    assert list(engine.batch_retable_status()) == [0, P.BAD_RATE, 0]
    engine.batch_run(_seeds(8, 3))
    _begin(ref_engine, obs, mixed)
    ref_engine.batch_run(_seeds(8, 3))
    _assert_same(_readout(engine, "history", obs), _readout(ref_engine, "history", obs))
    for other in (np.nan, np.inf, 0.0, -2.0):
        bad[0][1, 3] = other
        _retable(engine, "device", bad, obs)
        assert list(engine.batch_retable_status()) == [0, P.BAD_RATE, 0]
    bad[1][1, 2, :] = 0.0
    _retable(engine, "device", bad, obs)
    assert list(engine.batch_retable_status()) == [0, P.BAD_RATE | R.NO_MASS, 0]          # (bit 4 is not used)


# ---- 3. the refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_as_it_was(engine):
    k, Ts = 3, (5, 9)
    obs = _observes(Ts, 41)
    rates, trans = _tables(2, k, 42)
    sig = np.ones((2, k))
    _begin(engine, obs, (rates, trans))
    engine.batch_run(_seeds(5, 2))
    before = _readout(engine, "history", obs)
    # a bad rate at a host entry point
    for bad in (0.0, -1.0, np.nan, np.inf, 1e-310):
        r2 = rates.copy()
        r2[1, 2] = bad
        for call in (lambda: _begin(engine, obs, (r2, trans)),
                     lambda: engine.batch_begin_online(cp.MODEL_HMM_TABLE, Ts, N, _seeds(1, 2), tables=(r2, trans), emission="poisson"),
                     lambda: engine.batch_retable((r2, trans), obs, emission="poisson")):
            code, msg = _code(call)
            assert code == EINVAL and "problem 1" in msg and "rates" in msg, msg
    # another model, the shared table
    assert _code(lambda: engine.batch_begin_problems(cp.MODEL_HMM3, obs, N, tables=(rates, trans), emission="poisson"))[0] == EUNSUPPORTED
    with pytest.raises(ValueError):
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=None, emission="poisson")
    with pytest.raises(ValueError):
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=(rates, trans, sig), emission="poisson")
    # unit and scaled calls on the Poisson batch
    d_r, d_t, d_o, d_s = _dev(rates), _dev(trans), _dev(np.concatenate(obs)), _dev(sig)
    d_rec = _dev(np.ones((2, 88)))
    for call in (lambda: engine.batch_retable((rates, trans), obs),
                 lambda: engine.batch_retable((rates, trans, sig), obs),
                 lambda: engine.batch_retable_device(d_r, d_t, d_o),
                 lambda: engine.batch_retable_device(d_r, d_t, d_o, sigmas=d_s),
                 lambda: engine.batch_mstep_device(d_rec, d_r, d_t),
                 lambda: engine.batch_mstep_device(d_rec, d_r, d_t, sigmas=d_s),
                 lambda: engine.batch_scales(0, k)):
        code, msg = _code(call)
        assert code == ESTATE and ("Poisson" in msg or "no emission scales" in msg), msg
    assert _code(lambda: engine.batch_mstep_device(d_rec, d_r, d_t, emission="poisson", rate_floor=0.0))[0] == EINVAL
    _assert_same(_readout(engine, "history", obs), before)
    # Poisson calls on a unit and on a scaled batch
    for tables in ((rates, trans), (rates, trans, sig)):
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, N, tables=tables)
        for call in (lambda: engine.batch_retable((rates, trans), obs, emission="poisson"),
                     lambda: engine.batch_retable_device(d_r, d_t, d_o, emission="poisson"),
                     lambda: engine.batch_mstep_device(d_rec, d_r, d_t, emission="poisson"),
                     lambda: engine.batch_copy_rates(0, k)):
            code, msg = _code(call)
            assert code == ESTATE and "no Poisson emissions" in msg, msg
        want = S.rows(obs[0], rates[0], np.ones(k), k)
        assert np.array_equal(engine.batch_step_tables(0)[0], want)
    # online batches: the tables of another family, and online EM
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, Ts, N, _seeds(1, 2), tables=(rates, trans), emission="poisson", keep_history=False, keep_masses=True)
    for call in (lambda: engine.batch_online_tables((rates, trans)),
                 lambda: engine.batch_online_tables((rates, trans, sig)),
                 lambda: engine.batch_learn_begin(np.ones(max(Ts)), 1),
                 lambda: engine.batch_learn_begin(np.ones(max(Ts)), 1, sigma_floor=1e-3)):
        code, msg = _code(call)
        assert code == ESTATE and "Poisson" in msg, msg
    r2 = rates.copy()
    r2[1, 0] = 0.0
    code, msg = _code(lambda: engine.batch_online_tables((r2, trans), emission="poisson"))
    assert code == EINVAL and "problem 1" in msg
    engine.batch_advance(obs)
    assert np.array_equal(engine.batch_step_tables(1)[0], P.rows(obs[1], rates[1], k))
    for tables in ((rates, trans), (rates, trans, sig)):
        engine.batch_begin_online(cp.MODEL_HMM_TABLE, Ts, N, _seeds(1, 2), tables=tables)
        code, msg = _code(lambda: engine.batch_online_tables((rates, trans), emission="poisson"))
        assert code == ESTATE and "no Poisson emissions" in msg, msg


# ---- 4. the M-step kernel ----------------------------------------------------------------------------------------------------------------
def _mstep_device(engine, recs, rates, trans, floor):
    import torch
    m, t, lr = _dev(rates), _dev(trans), _dev(np.full(rates.shape, -7.0))
    engine.batch_mstep_device(_dev(recs), m, t, emission="poisson", rate_floor=floor, log_rates=lr)
    engine.sync()
    torch.cuda.synchronize()
    return m.cpu().numpy(), t.cpu().numpy(), lr.cpu().numpy()


@pytest.mark.parametrize("k", [2, 5, 8])
def test_mstep_kernel_on_the_records_of_a_run(engine, k):
    B, n = 6, 256
    obs = _observes([40 + 3 * b for b in range(B)], 91)
    rates, trans = _tables(B, k, 92)
    _begin(engine, obs, (rates, trans), n=n)
    engine.batch_run(_seeds(17, B))
    st = engine.batch_smooth_stats(obs)
    recs = np.concatenate([st["xi"].reshape(B, 64), st["occ"], st["occ_y"], st["occ_yy"]], axis=1)
    floor = 1.5                                               # (above some fitted rates, below others)
    m, t, lr = _mstep_device(engine, recs, rates, trans, floor)
    for b in range(B):
        wr, wl, wt = P.m_step(recs[b], rates[b], np.full(k, -7.0), trans[b], k, floor)
        assert np.array_equal(m[b], wr) and np.array_equal(t[b], wt) and np.array_equal(lr[b], wl)
    hm, ht = em.m_step(st, rates, trans, emission="poisson", rate_floor=floor)
    assert np.array_equal(hm, m) and np.array_equal(ht, t) and np.any(m > floor)


def test_mstep_kernel_on_the_constructed_records(engine):
    obs = _observes((3, 3), 95)
    for name, rec, rates, trans, floor in mstep_cases():
        _begin(engine, obs, (np.tile(rates, (2, 1)), np.tile(trans, (2, 1, 1))))
        m, t, lr = _mstep_device(engine, np.tile(rec, (2, 1)), np.tile(rates, (2, 1)), np.tile(trans, (2, 1, 1)), floor)
        wr, wl, wt = P.m_step(rec, rates, np.full(2, -7.0), trans, 2, floor)
        with np.errstate(all="ignore"):
            hm, ht = em.m_step(cp.capi.split_stats(rec[None, :]), rates[None, :], trans[None, :, :], emission="poisson", rate_floor=floor)
        for b in range(2):
            assert np.array_equal(m[b], wr) and np.array_equal(t[b], wt) and np.array_equal(lr[b], wl, equal_nan=True), name
            assert np.array_equal(m[b], hm[0]) and np.array_equal(t[b], ht[0]), name
        if name == "subnormal":
            assert math.isnan(lr[0, 0]) and 0.0 < m[0, 0] < S.MIN_NORMAL


# ---- 5. device-resident EM ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [None, [0, 0, 1]], ids=["untied", "tied"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_resident_poisson_em_is_the_host_loop(engine, mode, groups):
    B, k, n, iters = 3, 3, 64, 3
    rng = np.random.default_rng(7)
    obs = [rng.poisson(np.where(rng.random(T) < 0.5, 1.0, 9.0)).astype(np.float64) for T in (40, 33, 25)]
    rates, trans = _tables(B, k, 101)
    if groups is not None:
        rates[1], trans[1] = rates[0], trans[0]
    seeds = _seeds(300, B)
    kw = dict(keep_history=mode == "history", emission="poisson", rate_floor=1e-6, groups=None if groups is None else np.array(groups))
    host = em.hmm_table_em(engine, obs, rates, trans, n, seeds, iters, **kw)
    res = em.hmm_table_em(engine, obs, rates, trans, n, seeds, iters, resident=True, **kw)
    assert len(host) == len(res) == 3 and host[0].shape == (iters + 1, B, k)
    for h, r in zip(host, res):
        assert h.shape == r.shape and np.array_equal(h, r)
    assert not np.array_equal(host[0][-1], rates) and np.all(host[0] > 0.0) and np.all(np.isfinite(host[2]))
    if groups is not None:
        assert np.array_equal(host[0][:, 0], host[0][:, 1]) and not np.array_equal(host[0][-1, 0], host[0][-1, 2])
    with pytest.raises(ValueError):
        em.hmm_table_em(engine, obs, rates, trans, n, seeds, 1, emission="poisson", sigmas0=np.ones((B, k)))


# ---- 6. the helpers ----------------------------------------------------------------------------------------------------------------------
def test_helpers_with_poisson(engine, ref_engine):
    from cpprob_amd import decode, forecast
    B, k = 3, 3
    obs = _observes((20, 33, 40), 111)
    rates, trans = _tables(B, k, 112)
    seeds = _seeds(50, B)
    paths, scores, ev = decode.hmm_table_decode(engine, obs, rates, trans, N, seeds, emission="poisson")
    _begin(ref_engine, obs, (rates, trans))
    ref_engine.batch_run(seeds)
    _assert_same([paths, scores], list(ref_engine.batch_decode()))
    assert np.array_equal(ev, [s["log_evidence"] for s in ref_engine.batch_results()[0]])
    marg = ref_engine.batch_forecast(4)[0]
    pred = ref_engine.batch_predictive()
    for b in range(B):
        f = marg[b][:, :k]
        mean, var = forecast.observation_forecast(marg[b], rates[b], emission="poisson")
        assert np.allclose(mean, f @ rates[b], rtol=1e-13) and np.allclose(var, f @ rates[b] + f @ rates[b] ** 2 - (f @ rates[b]) ** 2, rtol=1e-12)
        assert np.all(var >= mean - 1e-12)                    # (a mixture of Poisson laws is over-dispersed)
        got = forecast.predictive_log_likelihood(pred[b], rates[b], obs[b], emission="poisson")
        pmf = np.array([[math.exp(y * math.log(r) - r - math.lgamma(y + 1.0)) for r in rates[b]] for y in obs[b]])
        want = np.log((pred[b][:len(obs[b]), :k] * pmf).sum(axis=1))
        assert np.allclose(got, want, rtol=1e-11, atol=1e-12)


# ---- 7. the filter is right ----------------------------------------------------------------------------------------------------------------
def _poisson_logpmf(y, rates):
    return np.array([[v * math.log(r) - r - math.lgamma(v + 1.0) for r in rates] for v in y])


def exact_forward_backward(y, rates, trans):
    """(log-likelihood, smoothed marginals [T, k], xi [k, k], occ [k], occ_y [k]) of a Poisson HMM with a uniform initial law: the scaled
    forward-backward recursion, restated here."""
    A = np.asarray(trans, np.float64)
    A = A / A.sum(axis=1, keepdims=True)
    T, k = len(y), len(rates)
    lik = np.exp(_poisson_logpmf(y, rates))
    alpha, c = np.zeros((T, k)), np.zeros(T)
    a = np.full(k, 1.0 / k) * lik[0]
    for t in range(T):
        if t:
            a = (alpha[t - 1] @ A) * lik[t]
        c[t] = a.sum()
        alpha[t] = a / c[t]
    beta = np.ones((T, k))
    for t in range(T - 2, -1, -1):
        beta[t] = (A @ (lik[t + 1] * beta[t + 1])) / c[t + 1]
    gamma = alpha * beta
    gamma /= gamma.sum(axis=1, keepdims=True)
    xi = np.zeros((k, k))
    for t in range(T - 1):
        x = alpha[t][:, None] * A * (lik[t + 1] * beta[t + 1])[None, :] / c[t + 1]
        xi += x / x.sum()
    y = np.asarray(y, np.float64)
    return float(np.log(c).sum()), gamma, xi, gamma.sum(axis=0), gamma.T @ y


def test_poisson_filter_and_smoother_against_the_exact_ones(engine):
    """k = 3, rates (0.5, 4, 12), a sticky transition, T = 24, n = 256, 32 seeds.  The criteria of
    tests/test_gpu_batch_scale.py::test_scaled_filter_and_smoother_against_the_exact_ones: the SMC evidence is unbiased, so the mean of
    Z-hat / Z lies within 5 of its standard errors of 1; the mean of (Z-hat / Z) phi-hat within 5 standard errors of the exact
    marginal; the plain mean of phi-hat within 5 standard errors plus sd(phi-hat) sd(Z-hat / Z) (Cauchy-Schwarz).  The states of a
    Poisson table do not overlap as those of the Gaussian test do: at two of the 72 entries the exact marginal of the state of rate 0.5
    is 2.0e-9 and 3.6e-12 and no particle of any run is in it, so the standard error estimated from the 32 runs is 0 there.  Every
    standard error is therefore held from below by sqrt(gamma (1 - gamma) / (n runs)), that of n runs independent draws from the exact
    marginal (5.0e-7 and 2.1e-8 at those two entries; nowhere else does it decide).  Measured: mean Z-hat / Z = 1.0657, standard error
    0.0815; the largest plain-mean allowance is 0.0743 (5 standard errors 0.0488, bias bound 0.0255), the largest deviation 0.0040."""
    k, T, n, runs = 3, 24, 256, 32
    rates = np.array([0.5, 4.0, 12.0])
    trans = np.array([[0.8, 0.1, 0.1], [0.15, 0.7, 0.15], [0.2, 0.2, 0.6]])
    rng = np.random.default_rng(99)
    x, y = 0, np.zeros(T)
    for t in range(T):
        x = rng.choice(k, p=trans[x])
        y[t] = rng.poisson(rates[x])
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, [y] * runs, n, tables=(np.tile(rates, (runs, 1)), np.tile(trans, (runs, 1, 1))), emission="poisson")
    engine.batch_run(_seeds(12345, runs))
    lz = np.array([s["log_evidence"] for s in engine.batch_results()[0]])
    marg = engine.batch_smooth()[0][:, :T, :k]
    ll, gamma, _, _, _ = exact_forward_backward(y, rates, trans)
    r = np.exp(lz - ll)
    se = r.std(ddof=1) / math.sqrt(runs)
    print("mean Z-hat / Z = %.4f, standard error %.4f, sd %.4f" % (r.mean(), se, r.std(ddof=1)))
    assert abs(r.mean() - 1.0) <= 5.0 * se
    # a standard error estimated from 32 runs is nothing where the state is so rare that (almost) no run saw a particle in it: it is held
    # from below by that of n runs independent draws from the exact marginal, sqrt(gamma (1 - gamma) / (n runs))
    floor = np.sqrt(gamma * (1.0 - gamma) / (n * runs))
    w = r[:, None, None] * marg
    se_w = w.std(axis=0, ddof=1) / math.sqrt(runs)
    sd = marg.std(axis=0, ddof=1)
    se_m = sd / math.sqrt(runs)
    dev_w, dev_m = np.abs(w.mean(axis=0) - gamma), np.abs(marg.mean(axis=0) - gamma)
    for t, s in zip(*np.nonzero((dev_w > 5.0 * se_w + 1e-12) | (dev_m > 5.0 * se_m + sd * r.std(ddof=1) + 1e-12))):
        print("step %d state %d: exact %.3e, weighted mean %.3e (se %.3e), plain mean %.3e (se %.3e), %d of %d runs saw the state, binomial se %.3e"
              % (t, s, gamma[t, s], w.mean(axis=0)[t, s], se_w[t, s], marg.mean(axis=0)[t, s], se_m[t, s], int(np.sum(marg[:, t, s] > 0.0)), runs, floor[t, s]))
    assert np.all(dev_w <= 5.0 * np.maximum(se_w, floor) + 1e-12)
    print("plain mean: largest allowance %.4f (5 standard errors %.4f + bias bound %.4f), largest deviation %.4f"
          % ((5.0 * se_m + sd * r.std(ddof=1)).max(), (5.0 * se_m).max(), (sd * r.std(ddof=1)).max(), dev_m.max()))
    assert np.all(dev_m <= 5.0 * np.maximum(se_m, floor) + sd * r.std(ddof=1) + 1e-12)


# ---- 8. EM recovers the rates --------------------------------------------------------------------------------------------------------------
POOLED_TS = [64, 48, 64, 33, 64, 57, 64, 40]


def pooled_case():
    """Eight recordings of 33 .. 64 counts of one sticky two-state process, rates (1, 8), self-transition 0.9; the start is rates
    (2, 5) and uniform rows."""
    rng = np.random.default_rng(31032)
    true_rates = np.array([1.0, 8.0])
    seqs = []
    for T in POOLED_TS:
        s, obs = int(rng.integers(0, 2)), np.zeros(T)
        for t in range(T):
            if t > 0 and rng.random() >= 0.9:
                s = 1 - s
            obs[t] = rng.poisson(true_rates[s])
        seqs.append(obs)
    return seqs, np.array([2.0, 5.0]), np.full((2, 2), 0.5)


def pooled_exact_em(seqs, rates0, trans0, iterations):
    """Baum-Welch on the pooled exact statistics (exact_forward_backward, summed over the recordings)."""
    rates, trans = np.array(rates0, np.float64), np.array(trans0, np.float64)
    rs, ts = [rates.copy()], [trans.copy()]
    for _ in range(iterations):
        xi, occ, occ_y = np.zeros((2, 2)), np.zeros(2), np.zeros(2)
        for o in seqs:
            _, _, a, b, c = exact_forward_backward(o, rates, trans)
            xi, occ, occ_y = xi + a, occ + b, occ_y + c
        trans, rates = xi / xi.sum(axis=1, keepdims=True), occ_y / occ
        rs.append(rates.copy()), ts.append(trans.copy())
    return np.array(rs), np.array(ts)


def gaussian_ratios():
    """What tests/test_gpu_batch_tied_fit.py::test_tied_particle_em_tracks_pooled_baum_welch holds the tied Gaussian fit to, as a share of
    its reference's own scale: its bounds on the distance from pooled Baum-Welch (means, transition entries) over the largest
    iterate-to-iterate move of that Baum-Welch recursion (no GPU: the recursion is exact)."""
    import test_gpu_batch_tied_fit as G
    seqs, means0, trans0 = G.pooled_case()
    bw_m, bw_t = G.pooled_exact_em(seqs, means0, trans0, 10)
    return G.MEANS_BOUND / np.abs(np.diff(bw_m, axis=0)).max(), G.TRANS_BOUND / np.abs(np.diff(bw_t, axis=0)).max()


def test_tied_poisson_em_tracks_pooled_baum_welch(engine):
    """All eight recordings in one group, n = 256, 10 iterations, resident.  The yardstick is Baum-Welch on the pooled exact statistics;
    its own scale is its largest iterate-to-iterate move.  The particle route's distance from it, as a share of that scale, stays below
    the share the tied Gaussian test holds its fit to (gaussian_ratios; profiles/r32_notes.md), for the rates and for the transition
    entries.  The fitted rates end nearer to (1, 8) than the start.  Measured: Baum-Welch's largest move 2.598 (rates) and 0.297
    (transition entries); the particle route off by at most 0.00513 and 0.00269, shares 0.00198 and 0.00905; the Gaussian test's shares
    0.00644 and 0.01379."""
    seqs, rates0, trans0 = pooled_case()
    nB, iters = len(seqs), 10
    bw_r, bw_t = pooled_exact_em(seqs, rates0, trans0, iters)
    scale_r, scale_t = np.abs(np.diff(bw_r, axis=0)).max(), np.abs(np.diff(bw_t, axis=0)).max()
    ratio_r, ratio_t = gaussian_ratios()
    seeds = np.array([4242 + 1000 * b for b in range(nB)], np.uint64)
    r0, t0 = np.tile(rates0, (nB, 1)), np.tile(trans0, (nB, 1, 1))
    rates, trans, ev = em.hmm_table_em(engine, seqs, r0, t0, 256, seeds, iters, groups=np.zeros(nB, np.int64), resident=True, emission="poisson")
    assert rates.shape == (iters + 1, nB, 2) and all(np.array_equal(rates[:, b], rates[:, 0]) for b in range(nB))
    dr = np.abs(rates[:, 0] - bw_r).max()
    dt = np.abs(trans[:, 0] - bw_t).max()
    print("pooled Baum-Welch: rates %s, self-transitions %s; its largest iterate-to-iterate move: rates %.5f, transition entries %.5f"
          % (bw_r[-1], np.diag(bw_t[-1]), scale_r, scale_t))
    print("tied Poisson fit: rates %s; off by at most %.5f (rates), %.5f (transition entries): shares %.5f and %.5f of the scale; the Gaussian test's shares %.5f and %.5f"
          % (rates[-1, 0], dr, dt, dr / scale_r, dt / scale_t, ratio_r, ratio_t))
    print("summed log-evidence %.3f -> %.3f" % (ev[0].sum(), ev[-1].sum()))
    assert dr / scale_r <= ratio_r and dt / scale_t <= ratio_t
    assert ev[-1].sum() > ev[0].sum()
    assert np.abs(rates[-1, 0] - [1.0, 8.0]).max() < np.abs(rates0 - [1.0, 8.0]).max()
