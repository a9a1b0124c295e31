"""Categorical emissions of a batch on the device (csrc/batch_categorical.hpp) against tests/categorical_ref.py, bit for bit.  A described
begin refuses a problem of length 0 for every family, so the ragged batches hold T = 1, 2, 37 and the refusal of T = 0 is asserted."""
import functools

import numpy as np
import pytest

import backward_ref as R
import categorical_ref as CR
import cpprob_amd as cp
import exact_ref as X
import retable_ref as RT

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
B_TWO_WALKS = 4 * 2048 + 1                                  # kWaves * kSymbolGridMax + 1: the first wavefront walks a second problem
# 8 x 1.31e-9, the largest distance between the restatement chain (exact_ref + suffstats_ref + categorical_ref) and the float64 recursion
# over exactly test_exact_fit_is_baum_welch's cases, measured on the CPU by tools/measure_categorical_tolerance.py (profiles/r40_notes.md)
TOL_BAUM_WELCH = 8 * 1.31e-9


@functools.lru_cache(maxsize=None)
def _case(k, V, Ts, seed=0):
    rng = np.random.default_rng(1000 * k + 10 * V + seed)
    nb = len(Ts)
    E = np.maximum(rng.dirichlet(np.ones(V), (nb, k)), 1e-3)
    return {"obs": [rng.integers(0, V, T).astype(np.float64) for T in Ts], "E": E, "A": rng.uniform(0.05, 1.0, (nb, k, k))}


def code(call, match=None):
    with pytest.raises(cp.capi.CpprobHipError, match=match) as e:
        call()
    return e.value.code


def _assert_tables(engine, obs, E, A, which=None):
    for b in range(engine.batch_B) if which is None else which:
        rows, thr = engine.batch_step_tables(b)
        got_e, got_l = engine.batch_copy_emission(b)
        assert np.array_equal(rows, CR.rows(obs[b], E[b])) and np.array_equal(thr, RT.thresholds(A[b], A.shape[1])), b
        assert np.array_equal(got_e, E[b]) and np.array_equal(got_l, CR.log_matrix(E[b])), b


def _assert_records(engine, obs, E, A, exact, which=None):
    k, V = E.shape[1], E.shape[2]
    if exact:
        engine.batch_run_exact()
    else:
        engine.batch_run(np.arange(engine.batch_B, dtype=np.uint64) + np.uint64(7))
    st, base = engine.batch_symbol_stats(obs), engine.batch_smooth_stats(obs)
    assert all(np.array_equal(st[name], base[name], equal_nan=True) for name in base)
    refs = {}
    for b in range(engine.batch_B):
        i = b if which is None else which[b]
        if i not in refs:
            m = engine.batch_masses(b)
            if exact:
                want_m, _, dead = X.run(CR.rows(obs[b], E[b])[:, :k].tolist(), R.transition_masses(A[b]))
                assert np.array_equal(m, np.array(want_m)) and engine.batch_exact_evidence()[1][b] == dead
            refs[i] = CR.symbol_counts(m, R.transition_masses(A[b]), obs[b], V)
        assert np.array_equal(st["cnt"][b], refs[i], equal_nan=True), b
    return st


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
@pytest.mark.parametrize("V", [1, 2, 9, 64])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_device_equals_the_restatement(engine, k, V, exact):
    import torch
    c, new = _case(k, V, (1, 2, 37)), _case(k, V, (1, 2, 37), seed=1)
    engine.batch_begin_problems_categorical(c["obs"], 16, c["E"], c["A"], keep_history=False, keep_masses=True)
    _assert_tables(engine, c["obs"], c["E"], c["A"])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (new["E"], new["A"], np.concatenate(c["obs"]))]
    torch.cuda.synchronize()
    engine.batch_retable_categorical_device(*dev)
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, c["obs"], new["E"], new["A"])
    st = _assert_records(engine, c["obs"], new["E"], new["A"], exact)
    rec = np.concatenate([st["xi"].reshape(3, -1), st["occ"], st["occ_y"], st["occ_yy"], st["cnt"].reshape(3, -1)], axis=1)
    engine.batch_mstep_categorical_device(torch.from_numpy(rec).to("cuda:0"), dev[0], dev[1], 1e-4)
    engine.sync()
    host = cp.m_step_categorical(st, new["E"], new["A"], 1e-4)
    for b in range(3):
        want = CR.m_step(rec[b], new["E"][b], new["A"][b], 1e-4)
        assert all(np.array_equal(d[b].cpu().numpy(), w) and np.array_equal(h[b], w) for d, h, w in zip(dev, host, want)), b


def test_observes_that_are_no_symbol_and_a_wavefront_that_walks_two_problems(engine):
    """NaN, 2.5, -1 and V at step 2: the exact run is dead there, every marginal is NaN, and only the bins 0 and 1 take it."""
    c = _case(3, 9, (5, 5, 5, 5), seed=2)
    obs = [np.array([0.0, 1.0, y, 1.0, 0.0]) for y in (np.nan, 2.5, -1.0, 9.0)]
    engine.batch_begin_problems_categorical(obs, 8, c["E"], c["A"], keep_history=False, keep_masses=True)
    st = _assert_records(engine, obs, c["E"], c["A"], True)
    assert list(engine.batch_exact_evidence()[1]) == [2] * 4 and np.isnan(st["cnt"][:, :3, :2]).all() and not st["cnt"][:, :, 2:].any() and not st["cnt"][:, 3:].any()
    c = _case(2, 2, (2,) * 5, seed=3)
    which = np.arange(B_TWO_WALKS) % 5
    obs, E, A = [c["obs"][i] for i in which], c["E"][which], c["A"][which]
    engine.batch_begin_problems_categorical(obs, 4, E, A, keep_history=False, keep_masses=True)
    _assert_records(engine, obs, E, A, True, which)


@pytest.mark.parametrize("bad", [0.0, -0.5, np.nan, 1e-310], ids=["zero", "negative", "nan", "subnormal"])
def test_a_bad_matrix_is_refused_for_its_problem_alone(engine, bad):
    import torch
    c, new = _case(3, 5, (4, 6, 3)), _case(3, 5, (4, 6, 3), seed=1)
    E = new["E"].copy()
    E[1, 2, 4] = bad
    assert code(lambda: engine.batch_begin_problems_categorical(c["obs"], 8, E, c["A"]), "problem 1: emission probabilities") == EINVAL
    engine.batch_begin_problems_categorical(c["obs"], 8, c["E"], c["A"])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (E, new["A"], np.concatenate(c["obs"]))]
    torch.cuda.synchronize()
    engine.batch_retable_categorical_device(*dev)
    assert list(engine.batch_retable_status()) == [0, CR.BAD_PROB, 0] and CR.check(E[1], new["A"][1]) == CR.BAD_PROB
    _assert_tables(engine, c["obs"], c["E"], c["A"], [1])
    _assert_tables(engine, c["obs"], E, new["A"], [0, 2])
    assert code(lambda: engine.batch_retable_categorical(E, new["A"], c["obs"]), "problem 1") == EINVAL


def test_bad_arguments_and_cross_family_calls(engine):
    import torch
    c = _case(2, 3, (4, 5))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    obs, E, A, means, rec = t(np.concatenate(c["obs"])), t(c["E"]), t(c["A"]), t(np.ones((2, 2))), t(np.zeros((2, CR.RECORD)))
    torch.cuda.synchronize()
    # (T = 0: no described begin takes it)
    assert code(lambda: engine.batch_begin_problems_categorical([c["obs"][0], np.zeros(0)], 8, c["E"], c["A"]), "every problem needs 1") == EINVAL
    for V in (0, 65):
        assert code(lambda: engine.batch_begin_problems_categorical(c["obs"], 8, np.full((2, 2, V), 0.1), c["A"])) == EINVAL
    engine.batch_begin_problems_categorical(c["obs"], 8, c["E"], c["A"], keep_history=False, keep_masses=True)
    engine.batch_run_exact()
    for floor in (0.0, -1.0, np.nan, np.inf, 1e-310):
        assert code(lambda: engine.batch_mstep_categorical_device(rec, E, A, floor)) == EINVAL
    calls = [lambda: engine.batch_retable_device(means, A, obs), lambda: engine.batch_retable_device(means, A, obs, sigmas=means),
             lambda: engine.batch_retable_device(means, A, obs, emission="poisson"), lambda: engine.batch_mstep_device(rec, means, A),
             lambda: engine.batch_mstep_device(rec, means, A, emission="poisson"), lambda: engine.batch_copy_rates(0), lambda: engine.batch_scales(0),
             lambda: engine.batch_draw_tables_device(rec, t(np.zeros(2, np.int64)), 0, means, A)]
    assert [code(f) for f in calls] == [ESTATE] * len(calls)
    _assert_tables(engine, c["obs"], c["E"], c["A"])          # (the batch as it was, and its run still serves)
    assert np.isfinite(engine.batch_symbol_stats(c["obs"])["cnt"]).all()
    for emission, tables in (("normal", (c["A"][:, 0], c["A"])), ("normal", (c["A"][:, 0], c["A"], c["A"][:, 1])), ("poisson", (c["A"][:, 0], c["A"]))):
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, c["obs"], 8, tables=tables, keep_history=False, keep_masses=True, emission=emission)
        before = engine.batch_step_tables(1)
        engine.batch_run_exact()
        calls = [lambda: engine.batch_retable_categorical_device(E, A, obs), lambda: engine.batch_retable_categorical(c["E"], c["A"], c["obs"]),
                 lambda: engine.batch_symbol_stats_device(rec, obs), lambda: engine.batch_symbol_stats(c["obs"]),
                 lambda: engine.batch_mstep_categorical_device(rec, E, A), lambda: engine.batch_copy_emission(0, 2, 3)]
        assert [code(f) for f in calls] == [ESTATE] * len(calls)
        assert all(np.array_equal(x, y) for x, y in zip(before, engine.batch_step_tables(1)))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
def test_resident_fit_equals_the_host_loop(engine, exact):
    c = _case(3, 5, (12, 9, 12, 9), seed=4)
    host = cp.hmm_categorical_em(engine, c["obs"], c["E"], c["A"], 32, np.arange(4), 3, exact=exact)
    res = cp.hmm_categorical_em(engine, c["obs"], c["E"], c["A"], 32, np.arange(4), 3, exact=exact, resident=True)
    assert all(np.array_equal(x, y) for x, y in zip(host, res)) and np.isfinite(host[2]).all() and not np.array_equal(host[0][0], host[0][3])


def baum_welch(obs, E0, A0, iterations, floor=1e-6):
    """Float64 Baum-Welch of one discrete HMM, uniform initial state, hmm_categorical_em's M-step (the floor, no renormalisation)."""
    E, A = np.array(E0, np.float64), np.array(A0, np.float64)
    y, (k, V), Es, As = np.asarray(obs, np.int64), E.shape, [E.copy()], [A.copy()]
    for _ in range(iterations):
        P, lik = A / A.sum(axis=1, keepdims=True), E[:, y].T
        alpha, beta = np.zeros((len(y), k)), np.ones((len(y), k))
        a = np.full(k, 1.0 / k)
        for t in range(len(y)):
            alpha[t] = a * lik[t] / (a * lik[t]).sum()
            a = alpha[t] @ P
        xi = np.zeros((k, k))
        for t in range(len(y) - 2, -1, -1):
            x = alpha[t][:, None] * P * (lik[t + 1] * beta[t + 1])[None, :]
            xi += x / x.sum()
            beta[t] = P @ (lik[t + 1] * beta[t + 1])
            beta[t] /= beta[t].sum()
        gamma = alpha * beta / (alpha * beta).sum(axis=1, keepdims=True)
        cnt = np.array([gamma[y == v].sum(axis=0) for v in range(V)]).T
        A = np.where(xi.sum(axis=1, keepdims=True) > 0, xi / xi.sum(axis=1, keepdims=True), A)
        p = cnt / cnt.sum(axis=1, keepdims=True)
        E = np.where(p >= floor, p, floor)
        Es.append(E.copy())
        As.append(A.copy())
    return np.array(Es), np.array(As)


@pytest.mark.parametrize("k,V", [(2, 4), (3, 9)])
def test_exact_fit_is_baum_welch(engine, k, V):
    c = _case(k, V, (37, 37), seed=5)
    E, A, _ = cp.hmm_categorical_em(engine, c["obs"], c["E"], c["A"], 8, [1, 2], 5, exact=True)
    for b in range(2):
        want_E, want_A = baum_welch(c["obs"][b], c["E"][b], c["A"][b], 5)
        dE, dA = np.abs(E[:, b] - want_E).max(), np.abs(A[1:, b] - want_A[1:]).max()
        print("k %d V %d problem %d: matrix %.3g, transition rows %.3g" % (k, V, b, dE, dA))
        assert dE <= TOL_BAUM_WELCH and dA <= TOL_BAUM_WELCH
