"""Batched SMC over problems that differ (include/cpprob_hip.h: cpprob_hip_batch_begin_problems; csrc/batch_smc.hpp, a described batch):
every problem brings its own transition table and emission means, its own number of observes and its own particle count.  Problem b
must still be what a one-problem run with its table, observes, particle count and seed computes -- the oracle's states and ancestors,
its flags, ESS and evidence, its statistics -- independent of the other problems, of the dispatch order and of every packed offset.
The tolerances are those of tests/test_gpu_batch.py (_check_problem, test_batch_equals_the_one_problem_engine)."""
import json
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp
from oracle import exact
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RESAMPLERS = [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED]


def _seeds(B, base=77):
    return np.array([base + 7919 * b for b in range(B)], np.uint64)


def _tables(k, B, seed):
    """B tables of k states: means spread over a few units, transition weights in [0.05, 1]; table 1 (if any) has a zero entry."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    if B > 1:
        trans[1, 0, k - 1] = 0.0
    return means, trans


def _table_obs(means_b, T, rng):
    return means_b[rng.integers(0, len(means_b), T)] + rng.standard_normal(T)


def _set_table(engine, means_b, trans_b):
    engine.set_hmm(means_b, trans_b)
    O.set_hmm(means_b, trans_b)


def _check_problem(engine, b, obs, n, seed, rs, model, summ, stats, ess, res, k=3, keep=True):
    """tests/test_gpu_batch.py::_check_problem on a problem's own rows (the caller has set the problem's table): the oracle's states,
    ancestors, flags, ESS, evidence, log-weights and statistics.  keep = False: the oracle's filtering statistics instead.  HMM_TABLE:
    within 1e-9, the bound tests/test_gpu_inference.py::test_filtering_only_run_weight_sums_form sets for the same quantity (the
    weights are 32-bit fixed point: 2^-33 relative each, a ratio of two sums of them).  HMM3: within 1e-12, the smoothing bound above
    (counts times three doubles: a few ulps of a probability)."""
    ref = O.smc(model, obs, n, int(seed), rs, 2.0)
    assert np.array_equal(res, ref["resampled"])
    np.testing.assert_allclose(ess, ref["ess"], rtol=1e-9)
    assert abs(summ["log_evidence"] - ref["log_z"]) < 1e-9
    assert summ["step_form"] == (cp.capi.FORM_COUNTS if model == cp.MODEL_HMM3 else cp.capi.FORM_FIXED)
    if not keep:
        print("problem %d filter max diff %.3e" % (b, np.abs(stats[:, :k] - ref["filter"]).max()))
        np.testing.assert_allclose(stats[:, :k], ref["filter"], rtol=0, atol=1e-12 if model == cp.MODEL_HMM3 else 1e-9)
        assert np.all(stats[:, k:] == 0.0)
        return ref
    vals, anc, logw = engine.batch_store(b)
    assert vals.shape == (len(obs), n) and anc.shape == (len(obs), n) and logw.shape == (n,)
    assert np.array_equal(vals, ref["hist"]), "problem %d: states differ from the oracle" % b
    assert np.array_equal(anc, ref["anc"]), "problem %d: ancestors differ from the oracle" % b
    np.testing.assert_allclose(logw, ref["logw"], rtol=1e-12, atol=1e-12)
    if model == cp.MODEL_HMM3:
        np.testing.assert_allclose(stats, O.smoothing(ref["hist"], ref["anc"], ref["logw"]), rtol=0, atol=1e-12)
    else:
        q = O.fix_weights(logw, summ["max_logw"]).astype(np.float64)
        np.testing.assert_allclose(stats[:, :k], O.smoothing_linear(vals, anc, q, k=k), rtol=1e-11, atol=1e-13)
        assert np.all(stats[:, k:] == 0.0)
    paths = np.take_along_axis(vals, O.lineage(anc), axis=1)
    assert paths.shape == vals.shape and np.array_equal(paths[-1], vals[-1])
    return ref


def _check_one_problem_engine(engine, b, model, obs, n, seed, rs, keep, summ, stats, ess, res):
    """Every field tests/test_gpu_batch.py::test_batch_equals_the_one_problem_engine compares (the problem's table is set)."""
    engine.begin(cp.ALG_SMC, model, obs, n, seed=int(seed), resampler=rs, ess_threshold=2.0, keep_history=keep)
    engine.run(0)
    s1, st1, ess1, res1 = engine.results()
    assert np.array_equal(res, res1)
    np.testing.assert_allclose(ess, ess1, rtol=1e-9)
    assert abs(summ["log_evidence"] - s1["log_evidence"]) < 1e-9 and abs(summ["log_norm"] - s1["log_norm"]) < 1e-9
    # a filtering-only one-problem run that met a generation > 6 nats below its bound has repeated itself in floating point
    repeated = s1["step_form"] == cp.capi.FORM_FLOAT and summ["step_form"] == cp.capi.FORM_FIXED
    if repeated:
        print("problem %d (n = %d): one-problem run repeated in floating point; batch requantised %d, max_logw %.6f against %.6f"
              % (b, n, summ["n_requantised"], summ["max_logw"], s1["max_logw"]))
        assert not keep and summ["n_requantised"] > 0 and s1["n_requantised"] == 0
    else:
        assert abs(summ["max_logw"] - s1["max_logw"]) < 1e-12
        assert summ["step_form"] == s1["step_form"] and summ["n_requantised"] == s1["n_requantised"]
        assert keep or summ["n_requantised"] == 0
    for f in ("n_predict", "stats_per_predict", "is_int", "n_resampled"):
        assert summ[f] == s1[f], f
    # (the two forms' statistics differ by the 32-bit quantisation of the weights: the bound of the oracle's filter comparison)
    np.testing.assert_allclose(stats, st1, rtol=0 if repeated else 1e-11, atol=1e-9 if repeated else 1e-12)
    if keep:
        vals, anc, logw = engine.batch_store(b)
        assert np.array_equal(vals, engine.values()) and np.array_equal(anc, engine.ancestors())
        assert np.array_equal(logw, engine.logw())
    return s1


# ---- 1. per-problem tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_per_problem_tables_are_the_oracle_problem_by_problem(engine, k, rs):
    B, T, n = 12, 16, 1500
    means, trans = _tables(k, B, 100 + k)
    assert (trans == 0.0).sum() == 1
    rng = np.random.default_rng(k)
    obs = [_table_obs(means[b], T, rng) for b in range(B)]
    seeds = _seeds(B, 5)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans), resampler=rs)
    engine.batch_run(seeds)
    summ, stats, ess, res = engine.batch_results()
    assert stats.shape == (B, T, 8) and ess.shape == (B, T) and res.shape == (B, T)
    for b in range(B):
        _set_table(engine, means[b], trans[b])
        _check_problem(engine, b, obs[b], n, seeds[b], rs, cp.MODEL_HMM_TABLE, summ[b], stats[b], ess[b], res[b], k=k)
        assert summ[b]["n_predict"] == T


# ---- 2. ragged shapes -----------------------------------------------------------------------------------------------------------
# every T of {1, 2, 5, 16, 40, 128} and every n of {1, 2, 777, 1024, 1025, 4099, 8192} occurs; (128, 8192) once
RAGGED = [(5, 2), (128, 8192), (1, 777), (2, 1), (16, 1024), (40, 1025), (5, 4099), (1, 1), (40, 777), (16, 8192)]


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
def test_ragged_problems_are_the_oracle_and_the_one_problem_engine(engine, model, rs, keep):
    """HMM_TABLE: means several units apart, so at n = 1, 2 a generation often sits > 6 nats below its step's bound and the batch
    weighs it against its exact maximum inside the step (n_requantised > 0 on some problem, asserted), with and without history.
    Every problem equals the oracle, and the one-problem engine in every field test_batch_equals_the_one_problem_engine compares
    -- except that a one-problem run WITHOUT history cannot repair such a generation (settle_fixed's repair replays the history)
    and repeats itself in the floating-point form: for those problems (asserted to be exactly the requantised ones of the
    keep_history = 0 cells) step_form, n_requantised and max_logw are each path's own, and every other field is still compared."""
    assert {T for T, _ in RAGGED} == {1, 2, 5, 16, 40, 128} and {n for _, n in RAGGED} == {1, 2, 777, 1024, 1025, 4099, 8192}
    assert RAGGED.count((128, 8192)) == 1
    B = len(RAGGED)
    Ts, ns = [T for T, _ in RAGGED], [n for _, n in RAGGED]
    T_max = max(Ts)
    k = 3 if model == cp.MODEL_HMM3 else 5
    means, trans = _tables(5, B, 9)
    rng = np.random.default_rng(17)
    if model == cp.MODEL_HMM3:
        obs = [exact.simulate_hmm(T, 2000 + b) for b, T in enumerate(Ts)]
        tables = None
    else:
        obs = [_table_obs(means[b], T, rng) for b, T in enumerate(Ts)]
        tables = (means, trans)
    seeds = _seeds(B, 19)
    engine.batch_begin_problems(model, obs, ns, tables=tables, resampler=rs, keep_history=keep)
    engine.batch_run(seeds)
    summ, stats, ess, res = engine.batch_results()
    spp = 3 if model == cp.MODEL_HMM3 else 8
    assert stats.shape == (B, T_max, spp) and ess.shape == (B, T_max) and res.shape == (B, T_max)
    for b in range(B):
        T, n = RAGGED[b]
        if model == cp.MODEL_HMM_TABLE:
            _set_table(engine, means[b], trans[b])
        assert summ[b]["n_predict"] == T
        # the padded rows are exactly zero
        assert np.all(stats[b, T:] == 0.0) and np.all(ess[b, T:] == 0.0) and np.all(res[b, T:] == 0)
        _check_problem(engine, b, obs[b], n, seeds[b], rs, model, summ[b], stats[b, :T], ess[b, :T], res[b, :T], k=k, keep=keep)
        _check_one_problem_engine(engine, b, model, obs[b], n, seeds[b], rs, keep, summ[b], stats[b, :T], ess[b, :T], res[b, :T])
    if model == cp.MODEL_HMM_TABLE:
        assert sum(s["n_requantised"] > 0 for s in summ) >= 2, [s["n_requantised"] for s in summ]
    if not keep:
        with pytest.raises(cp.CpprobHipError):
            engine.batch_store(0)


def test_results_device_of_a_ragged_batch_is_padded_with_zeros(engine):
    import torch
    shapes = [(3, 100), (9, 600), (1, 5), (6, 1025)]
    B, T_max = len(shapes), 9
    obs = [exact.simulate_hmm(T, 20 + b) for b, (T, _) in enumerate(shapes)]
    # a longer batch first: the workspace the ragged batch reuses is not clean
    engine.batch_begin(cp.MODEL_HMM3, np.stack([exact.simulate_hmm(12, 50 + b) for b in range(6)]), 2000)
    engine.batch_run(_seeds(6))
    engine.batch_begin_problems(cp.MODEL_HMM3, obs, [n for _, n in shapes], resampler=cp.RESAMPLE_STRATIFIED)
    engine.batch_run(_seeds(B))
    out = torch.full((B, 4 + T_max * 3), -7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_results_device(out)
    engine.sync()
    got = out.cpu().numpy()
    summ, stats, ess, res = engine.batch_results()
    for b, (T, _) in enumerate(shapes):
        assert got[b, 0] == summ[b]["log_evidence"] and got[b, 1] == summ[b]["ess_final"]
        assert got[b, 2] == summ[b]["log_norm"] and got[b, 3] == summ[b]["max_logw"]
        assert np.array_equal(got[b, 4:], stats[b].reshape(-1))
        assert np.all(got[b, 4 + 3 * T:] == 0.0) and np.all(stats[b, :T].sum(axis=1) > 0.99)
        assert np.all(ess[b, T:] == 0.0) and np.all(res[b, T:] == 0)


# ---- 3. a uniform batch through the new begin is the old batch --------------------------------------------------------------------
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
def test_uniform_batch_through_the_new_begin_is_the_old_batch(engine, model, keep):
    T, n, B = 16, 3000, 6
    means, trans = _tables(5, 1, 3)
    _set_table(engine, means[0], trans[0])
    obs = np.stack([exact.simulate_hmm(T, 40 + b) for b in range(B)])
    seeds = _seeds(B, 123)
    for rs in RESAMPLERS:
        engine.batch_begin(model, obs, n, resampler=rs, keep_history=keep)
        engine.batch_run(seeds)
        old = engine.batch_results()
        old_stores = [engine.batch_store(b) for b in range(B)] if keep else []
        engine.batch_begin_problems(model, list(obs), n, resampler=rs, keep_history=keep)      # tables = None: the shared table
        engine.batch_run(seeds)
        new = engine.batch_results()
        assert new[0] == old[0]
        for x, y in zip(new[1:], old[1:]):
            assert x.shape == y.shape and np.array_equal(x, y)
        for b in range(len(old_stores)):
            for x, y in zip(engine.batch_store(b), old_stores[b]):
                assert x.shape == y.shape and np.array_equal(x, y)
        if model == cp.MODEL_HMM_TABLE:
            # ... and with the same table given B times over
            engine.batch_begin_problems(model, list(obs), n, tables=(np.repeat(means, B, 0), np.repeat(trans, B, 0)), resampler=rs, keep_history=keep)
            engine.batch_run(seeds)
            rep = engine.batch_results()
            assert rep[0] == old[0] and all(np.array_equal(x, y) for x, y in zip(rep[1:], old[1:]))


# ---- 4. independence --------------------------------------------------------------------------------------------------------------
def _run_problems(engine, model, obs, ns, tables, seeds, rs=cp.RESAMPLE_SYSTEMATIC):
    engine.batch_begin_problems(model, obs, ns, tables=tables, resampler=rs)
    engine.batch_run(seeds)
    summ, stats, ess, res = engine.batch_results()
    return summ, stats, ess, res, [engine.batch_store(b) for b in range(len(obs))]


@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
def test_a_problem_does_not_depend_on_the_batch(engine, model):
    shapes = [(12, 1500), (3, 40), (30, 5000), (7, 1024), (12, 1500), (1, 8192), (25, 2), (12, 3000), (5, 777)]
    B = len(shapes)
    means, trans = _tables(4, B, 21)
    rng = np.random.default_rng(2)
    if model == cp.MODEL_HMM3:
        obs = [exact.simulate_hmm(T, 300 + b) for b, (T, _) in enumerate(shapes)]
    else:
        obs = [_table_obs(means[b], T, rng) for b, (T, _) in enumerate(shapes)]
    ns = [n for _, n in shapes]
    seeds = _seeds(B, 9)
    tab = (lambda idx: None) if model == cp.MODEL_HMM3 else (lambda idx: (means[idx], trans[idx]))
    full = _run_problems(engine, model, obs, ns, tab(np.arange(B)), seeds)
    T4 = shapes[4][0]

    def same(got, at):
        """Problem 4 of the full batch against problem `at` of `got`: its own rows (the padding depends on the batch's longest)."""
        summ, stats, ess, res, stores = got
        assert summ[at] == full[0][4]
        assert np.array_equal(stats[at][:T4], full[1][4][:T4]) and np.array_equal(ess[at][:T4], full[2][4][:T4]) and np.array_equal(res[at][:T4], full[3][4][:T4])
        assert np.all(stats[at][T4:] == 0.0)
        for x, y in zip(stores[at], full[4][4]):
            assert x.shape == y.shape and np.array_equal(x, y)

    one = _run_problems(engine, model, obs[4:5], ns[4:5], tab(np.arange(4, 5)), seeds[4:5])                   # alone
    same(one, 0)
    perm = np.random.default_rng(0).permutation(B)                                                              # permuted
    got = _run_problems(engine, model, [obs[i] for i in perm], [ns[i] for i in perm], tab(perm), seeds[perm])
    same(got, int(np.where(perm == 4)[0][0]))
    # the neighbours replaced by problems of other shapes and tables: the dispatch order and every offset change
    other_shapes = [(40, 8192), (2, 2), (1, 1), (50, 4099), shapes[4], (9, 100), (60, 1025), (2, 8192), (33, 33)]
    m2, t2 = _tables(4, B, 77)
    m2[4], t2[4] = means[4], trans[4]
    if model == cp.MODEL_HMM3:
        obs2 = [exact.simulate_hmm(T, 900 + b) for b, (T, _) in enumerate(other_shapes)]
    else:
        obs2 = [_table_obs(m2[b], T, rng) for b, (T, _) in enumerate(other_shapes)]
    obs2[4] = obs[4]
    got = _run_problems(engine, model, obs2, [n for _, n in other_shapes], None if model == cp.MODEL_HMM3 else (m2, t2), seeds)
    same(got, 4)


# ---- 5. requantisation with per-problem tables ------------------------------------------------------------------------------------
def test_requantised_generations_with_per_problem_tables(engine):
    """tests/test_gpu_batch.py::test_requantised_generations_resample_like_the_one_problem_engine's construction as problems 0-1 of
    a batch whose other problems carry benign tables and observes near their means: n_requantised of every problem is the
    one-problem engine's -- which is > 0 for problems 0-1 and 0 for the rest (asserted on the one-problem engine first)."""
    bad_means, bad_trans = [-1.0, 0.0, 10.0], [[5.0, 5.0, 0.01], [5.0, 5.0, 0.01], [1.0, 1.0, 1.0]]
    T, B = 8, 6
    means, trans = _tables(3, B, 4)
    means[:] = np.array([-1.0, 0.0, 1.0]) + 0.1 * np.arange(B)[:, None]          # benign: neighbouring states, observes between them
    means[0] = means[1] = bad_means
    trans[0] = trans[1] = bad_trans
    rng = np.random.default_rng(8)
    obs = [means[b][rng.integers(0, 3, T)] + 0.3 * rng.standard_normal(T) for b in range(B)]
    for b, y0 in enumerate([-0.5, -1.2]):
        obs[b] = np.full(T, 30.0)
        obs[b][0] = y0                                                              # step 0 leaves (almost surely) no particle in state 2
    seeds = _seeds(B, 41)
    for n in (3, 8):
        for rs in RESAMPLERS:
            single = []
            for b in range(B):
                _set_table(engine, means[b], trans[b])
                engine.begin(cp.ALG_SMC, cp.MODEL_HMM_TABLE, obs[b], n, seed=int(seeds[b]), resampler=rs, ess_threshold=2.0)
                engine.run(0)
                single.append((engine.results(), engine.values(), engine.ancestors()))
            assert all(single[b][0][0]["n_requantised"] > 0 for b in (0, 1))
            assert all(single[b][0][0]["n_requantised"] == 0 for b in range(2, B))
            engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans), resampler=rs)
            engine.batch_run(seeds)
            summ, stats, ess, res = engine.batch_results()
            for b in range(B):
                (s1, st1, ess1, res1), vals1, anc1 = single[b]
                assert summ[b]["n_requantised"] == s1["n_requantised"]
                assert summ[b]["n_resampled"] == s1["n_resampled"] and np.array_equal(res[b], res1)
                assert abs(summ[b]["log_evidence"] - s1["log_evidence"]) < 1e-9 and summ[b]["max_logw"] == s1["max_logw"]
                np.testing.assert_allclose(ess[b], ess1, rtol=1e-9)
                np.testing.assert_allclose(stats[b], st1, rtol=1e-11, atol=1e-12)
                vals, anc, _ = engine.batch_store(b)
                assert np.array_equal(vals, vals1) and np.array_equal(anc, anc1)
                _set_table(engine, means[b], trans[b])
                _check_problem(engine, b, obs[b], n, seeds[b], rs, cp.MODEL_HMM_TABLE, summ[b], stats[b], ess[b], res[b], k=3)


# ---- 6. against an exact answer that owes nothing to the oracle ------------------------------------------------------------------
def forward_log_evidence(means, trans, obs):
    """log p(y_0..T-1) of the k-state table HMM by the forward recursion in log space: uniform initial state, x_t ~ row x_{t-1} of
    the transition weights (normalised), y_t ~ N(means[x_t], 1)."""
    means, trans = np.asarray(means, np.float64), np.asarray(trans, np.float64)
    logP = np.log(trans / trans.sum(axis=1, keepdims=True))

    def lse(a, axis):
        m = a.max(axis=axis, keepdims=True)
        return (m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True))).squeeze(axis)

    def emit(y):
        return -0.5 * (y - means) ** 2 - 0.5 * np.log(2.0 * np.pi)

    la = -np.log(len(means)) + emit(obs[0])
    for y in obs[1:]:
        la = lse(la[:, None] + logP, 0) + emit(y)
    return float(lse(la, 0))


def evidence_grid(side_spread, side_self):
    """Tables on a grid of (mean spread, self-transition weight), k = 3, and one observation sequence of 16."""
    spreads, selfs = np.linspace(0.5, 2.0, side_spread), np.linspace(0.2, 0.9, side_self)
    means, trans = [], []
    for d in spreads:
        for p in selfs:
            means.append([-d, 0.0, d])
            trans.append(np.full((3, 3), (1.0 - p) / 2.0) + np.eye(3) * (p - (1.0 - p) / 2.0))
    obs = exact.simulate_hmm(16, 4242)
    return np.array(means), np.array(trans), obs


def evidence_ratio_check(log_z_hat, means, trans, obs):
    ratio = np.array([np.exp(lz - forward_log_evidence(means[b], trans[b], obs)) for b, lz in enumerate(log_z_hat)])
    se = ratio.std(ddof=1) / np.sqrt(len(ratio))
    return ratio.mean(), se


def test_evidence_grid_against_the_forward_recursion(engine):
    """One sequence (T = 16) under B = 512 tables, n = 2048: the mean over problems of exp(log Z-hat_b - log Z_b) lies within 4
    standard errors of 1 (the form of tests/test_gpu_batch.py::test_batch_against_the_exact_posterior).  Grid and n were fixed after
    the same check passed on the CPU with the oracle in the GPU's place on a 64-table subgrid (every fourth spread, every second
    self-transition weight, the same seeds): tests/test_batch_problems_host.py::test_evidence_grid_precheck_with_the_oracle
    repeats that check (mean 1.0054, standard error 0.0074)."""
    means, trans, obs = evidence_grid(32, 16)
    B, n = len(means), 2048
    assert B == 512
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, [obs] * B, n, tables=(means, trans), keep_history=False)
    engine.batch_run(_seeds(B, 31))
    summ, _, _, _ = engine.batch_results()
    mean, se = evidence_ratio_check([s["log_evidence"] for s in summ], means, trans, obs)
    print("evidence ratio: mean %.6f, standard error %.6f" % (mean, se))
    assert abs(mean - 1.0) < 4 * se + 1e-12, (mean, se)


# ---- 7. coexistence ---------------------------------------------------------------------------------------------------------------
def test_both_begins_and_single_runs_coexist_on_one_context(engine):
    T, n, B = 16, 2048, 4
    obs_u = np.stack([exact.simulate_hmm(T, 70 + b) for b in range(B)])
    seeds_u = _seeds(B, 1)
    shapes = [(40, 4099), (3, 10), (16, 1024), (7, 8192), (1, 100)]
    obs_h = [exact.simulate_hmm(Tb, 170 + b) for b, (Tb, _) in enumerate(shapes)]
    ns_h = [nb for _, nb in shapes]
    seeds_h = _seeds(len(shapes), 2)
    single_obs = exact.simulate_hmm(T, 12)

    def single_begin():
        engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, single_obs, 20000, seed=3)

    def single_read():
        return engine.results(), engine.values()

    def batch_read(b):
        return engine.batch_results(), engine.batch_store(b)

    def equal(got, ref):
        assert got[0][0] == ref[0][0]
        for x, y in zip(got[0][1:] + got[1], ref[0][1:] + ref[1]):
            assert x.shape == y.shape and np.array_equal(x, y)

    # stand-alone references
    single_begin(); engine.run(0)
    ref_single = single_read()
    engine.batch_begin(cp.MODEL_HMM3, obs_u, n); engine.batch_run(seeds_u)
    ref_u = batch_read(2)
    engine.batch_begin_problems(cp.MODEL_HMM3, obs_h, ns_h); engine.batch_run(seeds_h)
    ref_h = batch_read(3)
    # uniform -> heterogeneous -> uniform on the one context, a single-population begin / run interleaved with each
    for _ in range(2):                                            # the same seeds twice: the same outputs
        engine.batch_begin(cp.MODEL_HMM3, obs_u, n)
        single_begin()
        engine.batch_run(seeds_u)
        engine.run(0)
        got = single_read()
        assert got[0][0] == ref_single[0][0] and all(np.array_equal(x, y) for x, y in zip(got[0][1:], ref_single[0][1:])) and np.array_equal(got[1], ref_single[1])
        equal(batch_read(2), ref_u)
        engine.batch_begin_problems(cp.MODEL_HMM3, obs_h, ns_h)
        single_begin()
        engine.batch_run(seeds_h)
        engine.run(0)
        got = single_read()
        assert got[0][0] == ref_single[0][0] and np.array_equal(got[1], ref_single[1])
        equal(batch_read(3), ref_h)
        engine.batch_run(seeds_h)                                 # run again without a begin
        equal(batch_read(3), ref_h)
    engine.batch_begin(cp.MODEL_HMM3, obs_u, n)
    engine.batch_run(seeds_u)
    equal(batch_read(2), ref_u)


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("rs", RESAMPLERS)
def test_uniform_batch_on_the_workspace_of_a_described_one(engine, rs, keep):
    """Both begins share one workspace and one kernel: a uniform batch begun after a described one finds that batch's descriptors,
    dispatch order and per-problem thresholds still on the device and must read none of them.  B = 3 both times, so every stale slot
    has a problem that would use it; n = 1025 needs a second pass over the population.  Every problem of the uniform batch is the
    oracle's under the table set in between."""
    k, B = 5, 3
    shapes = [(9, 777), (2, 2), (5, 1025)]
    means, trans = _tables(k, B, 61)
    rng = np.random.default_rng(23)
    obs = [_table_obs(means[b], T, rng) for b, (T, _) in enumerate(shapes)]
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, [n for _, n in shapes], tables=(means, trans), resampler=rs, keep_history=keep)
    engine.batch_run(_seeds(B, 3))
    m2, t2 = _tables(k, 1, 62)
    assert not np.array_equal(m2[0], means[0]) and not np.array_equal(t2[0], trans[0])
    _set_table(engine, m2[0], t2[0])
    T, n = 4, 1025
    obs_u = np.stack([_table_obs(m2[0], T, rng) for _ in range(B)])
    seeds = _seeds(B, 4)
    engine.batch_begin(cp.MODEL_HMM_TABLE, obs_u, n, resampler=rs, keep_history=keep)
    engine.batch_run(seeds)
    summ, stats, ess, res = engine.batch_results()
    assert stats.shape == (B, T, 8) and ess.shape == (B, T) and res.shape == (B, T)
    for b in range(B):
        assert summ[b]["n_predict"] == T
        _check_problem(engine, b, obs_u[b], n, seeds[b], rs, cp.MODEL_HMM_TABLE, summ[b], stats[b], ess[b], res[b], k=k, keep=keep)


# ---- 8. C++ / CLI -----------------------------------------------------------------------------------------------------------------
def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


def test_cpp_hmm_table_batch_through_cpprob_main(engine, tmp_path):
    """cpprob_main --batch_tables_file: one table-HMM problem a line ([means] [transition] [observes]), seeds --seed + line index,
    through cpprob::gpu::hmm_table_batch: one JSON object a line, each equal to the batch of the C ABI."""
    main = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")
    Ts, k, n, seed = [16, 3, 40, 1, 9], 4, 3000, 40
    B = len(Ts)
    means, trans = _tables(k, B, 55)
    rng = np.random.default_rng(6)
    obs = [_table_obs(means[b], T, rng) for b, T in enumerate(Ts)]
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(B)))
    base = [main, "--model_folder", str(tmp_path), "--smc", "--n_samples", str(n), "--seed", str(seed), "--ess_threshold", "2.0", "--batch_tables_file"]
    p = subprocess.run(base + ["tables.txt", "--json"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == B
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans))
    engine.batch_run(np.arange(seed, seed + B, dtype=np.uint64))
    summ, stats, _, _ = engine.batch_results()
    for b in range(B):
        assert lines[b]["n"] == n and lines[b]["builtin"] is True
        assert abs(lines[b]["log_evidence"] - summ[b]["log_evidence"]) < 1e-12
        got = np.array([h["p"] for h in lines[b]["predicts"]])
        assert got.shape == (Ts[b], k)
        np.testing.assert_allclose(got, stats[b, :Ts[b], :k], rtol=0, atol=1e-15)
    # a malformed line: the transition list is not k x k long
    bad = "%s %s %s\n" % (_numbers(means[0]), _numbers(trans[0]), _numbers(obs[0]))
    bad += "%s %s %s\n" % (_numbers(means[1]), _numbers(trans[1].reshape(-1)[:-1]), _numbers(obs[1]))
    (tmp_path / "bad.txt").write_text(bad)
    p = subprocess.run(base + ["bad.txt"], capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "line 1" in p.stderr
