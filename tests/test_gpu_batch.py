"""Batched SMC on the GPU (include/cpprob_hip.h: cpprob_hip_batch_*; csrc/batch_smc.hpp): B problems, one launch, one workgroup
per problem.  Every problem must be what a one-problem run with its seed computes: the oracle's states and ancestors, its
resampling flags, ESS and evidence, and its statistics; independent of the batch's shape and of the other problems."""
import numpy as np
import pytest

import cpprob_amd as cp
from oracle import exact
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TABLES = {
    2: ([-1.0, 1.5], [[0.7, 0.3], [0.4, 0.6]]),
    5: ([-2.0, -1.0, 0.0, 1.0, 2.5], [[3, 1, 1, 0, 1], [1, 3, 1, 1, 0], [0, 1, 3, 1, 1], [1, 0, 1, 3, 1], [1, 1, 0, 1, 3]]),
}


def _obs(B, T, first=1000):
    return np.stack([exact.simulate_hmm(T, first + b) for b in range(B)])


def _seeds(B, base=77):
    return np.array([base + 7919 * b for b in range(B)], np.uint64)


def _set_table(engine, k):
    means, trans = TABLES[k]
    engine.set_hmm(means, trans)
    O.set_hmm(means, trans)


def _check_problem(engine, b, obs, n, seed, rs, model, summ, stats, ess, res, k=3):
    ref = O.smc(model, obs, n, int(seed), rs, 2.0)
    vals, anc, logw = engine.batch_store(b)
    assert np.array_equal(vals, ref["hist"]), "problem %d: states differ from the oracle" % b
    assert np.array_equal(anc, ref["anc"]), "problem %d: ancestors differ from the oracle" % b
    assert np.array_equal(res, ref["resampled"])
    np.testing.assert_allclose(ess, ref["ess"], rtol=1e-9)
    assert abs(summ["log_evidence"] - ref["log_z"]) < 1e-9
    np.testing.assert_allclose(logw, ref["logw"], rtol=1e-12, atol=1e-12)
    if model == cp.MODEL_HMM3:
        assert summ["step_form"] == cp.capi.FORM_COUNTS
        np.testing.assert_allclose(stats, O.smoothing(ref["hist"], ref["anc"], ref["logw"]), rtol=0, atol=1e-12)
    else:
        assert summ["step_form"] == cp.capi.FORM_FIXED
        q = O.fix_weights(logw, summ["max_logw"]).astype(np.float64)
        np.testing.assert_allclose(stats[:, :k], O.smoothing_linear(vals, anc, q, k=k), rtol=1e-11, atol=1e-13)
        assert np.all(stats[:, k:] == 0.0)
    # the surviving traces: every final particle's lineage through the store
    paths = np.take_along_axis(vals, O.lineage(anc), axis=1)
    assert paths.shape == vals.shape and np.array_equal(paths[-1], vals[-1])
    return ref


# (T, n, B): the large T x n cells hold fewer problems
GRID = [(1, 777, 16), (5, 1, 16), (5, 2, 16), (16, 1024, 16), (40, 4099, 4), (128, 8192, 2), (16, 8192, 3)]


@pytest.mark.parametrize("rs", [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED])
@pytest.mark.parametrize("T,n,B", GRID)
def test_hmm3_batch_is_the_oracle_problem_by_problem(engine, T, n, B, rs):
    obs = _obs(B, T)
    seeds = _seeds(B)
    engine.batch_begin(cp.MODEL_HMM3, obs, n, resampler=rs)
    engine.batch_run(seeds)
    summ, stats, ess, res = engine.batch_results()
    assert stats.shape == (B, T, 3)
    for b in range(B):
        _check_problem(engine, b, obs[b], n, seeds[b], rs, cp.MODEL_HMM3, summ[b], stats[b], ess[b], res[b])
        assert summ[b]["n_requantised"] == 0 and summ[b]["n_predict"] == T


@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("rs", [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED])
@pytest.mark.parametrize("T,n,B", [(1, 777, 8), (5, 2, 8), (16, 1024, 8), (40, 4099, 3), (128, 8192, 2)])
def test_table_hmm_batch_is_the_oracle_problem_by_problem(engine, T, n, B, rs, k):
    _set_table(engine, k)
    means = np.array(TABLES[k][0])
    rng = np.random.default_rng(T * 31 + n)
    obs = means[rng.integers(0, k, (B, T))] + rng.standard_normal((B, T))
    seeds = _seeds(B, 5)
    engine.batch_begin(cp.MODEL_HMM_TABLE, obs, n, resampler=rs)
    engine.batch_run(seeds)
    summ, stats, ess, res = engine.batch_results()
    assert stats.shape == (B, T, 8)
    for b in range(B):
        _check_problem(engine, b, obs[b], n, seeds[b], rs, cp.MODEL_HMM_TABLE, summ[b], stats[b], ess[b], res[b], k=k)


def test_exact_maximum_branch_requantises_and_stays_exact(engine):
    """A generation whose heaviest particle sits more than 6 nats below the step's bound is weighed against its exact maximum
    (the single path's settle_fixed, here a branch in the step): counted in n_requantised, still the oracle's run."""
    _set_table(engine, 2)
    T, n, B = 10, 1, 6
    rng = np.random.default_rng(3)
    obs = np.array(TABLES[2][0])[rng.integers(0, 2, (B, T))] + 0.3 * rng.standard_normal((B, T))
    obs[0, 1:] = 30.0                      # outlying: a particle in the far state sits ~70 nats below the bound
    obs[1, 1:] = -30.0
    seeds = _seeds(B, 11)
    for rs in (cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED):
        engine.batch_begin(cp.MODEL_HMM_TABLE, obs, n, resampler=rs)
        engine.batch_run(seeds)
        summ, stats, ess, res = engine.batch_results()
        assert summ[0]["n_requantised"] > 0 or summ[1]["n_requantised"] > 0
        for b in range(B):
            _check_problem(engine, b, obs[b], n, seeds[b], rs, cp.MODEL_HMM_TABLE, summ[b], stats[b], ess[b], res[b], k=2)
        # the neighbours without outliers take the bound, as their one-problem runs do
        for b in range(2, B):
            assert summ[b]["n_requantised"] == 0


@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
@pytest.mark.parametrize("keep", [True, False])
def test_batch_equals_the_one_problem_engine(engine, model, keep):
    if model == cp.MODEL_HMM_TABLE:
        _set_table(engine, 5)
    T, n, B = 16, 3000, 5
    obs = _obs(B, T, 40)
    seeds = _seeds(B, 123)
    for rs in (cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED):
        engine.batch_begin(model, obs, n, resampler=rs, keep_history=keep)
        engine.batch_run(seeds)
        summ, stats, ess, res = engine.batch_results()
        for b in range(B):
            engine.begin(cp.ALG_SMC, model, obs[b], n, seed=int(seeds[b]), resampler=rs, ess_threshold=2.0, keep_history=keep)
            engine.run(0)
            s1, st1, ess1, res1 = engine.results()
            assert np.array_equal(res[b], res1)
            np.testing.assert_allclose(ess[b], ess1, rtol=1e-9)
            assert abs(summ[b]["log_evidence"] - s1["log_evidence"]) < 1e-9
            assert abs(summ[b]["max_logw"] - s1["max_logw"]) < 1e-12 and abs(summ[b]["log_norm"] - s1["log_norm"]) < 1e-9
            for f in ("n_predict", "stats_per_predict", "is_int", "n_resampled", "step_form", "n_requantised"):
                assert summ[b][f] == s1[f], f
            np.testing.assert_allclose(stats[b], st1, rtol=1e-11, atol=1e-12)
            if keep:
                vals, anc, logw = engine.batch_store(b)
                assert np.array_equal(vals, engine.values()) and np.array_equal(anc, engine.ancestors())
                assert np.array_equal(logw, engine.logw())
        if not keep:
            with pytest.raises(cp.CpprobHipError):
                engine.batch_store(0)


def _run(engine, model, obs, n, seeds, rs=cp.RESAMPLE_SYSTEMATIC):
    engine.batch_begin(model, obs, n, resampler=rs)
    engine.batch_run(seeds)
    summ, stats, ess, res = engine.batch_results()
    stores = [engine.batch_store(b) for b in range(len(obs))]
    return summ, stats, ess, res, stores


@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
def test_results_do_not_depend_on_the_batch(engine, model):
    if model == cp.MODEL_HMM_TABLE:
        _set_table(engine, 5)
    T, n, B = 12, 1500, 9
    obs = _obs(B, T, 300)
    seeds = _seeds(B, 9)
    full = _run(engine, model, obs, n, seeds)

    def same(b_full, got, b_got):
        summ, stats, ess, res, stores = got
        assert summ[b_got] == full[0][b_full]
        assert np.array_equal(stats[b_got], full[1][b_full]) and np.array_equal(ess[b_got], full[2][b_full]) and np.array_equal(res[b_got], full[3][b_full])
        for x, y in zip(stores[b_got], full[4][b_full]):
            assert np.array_equal(x, y)

    one = _run(engine, model, obs[4:5], n, seeds[4:5])             # B = 1
    same(4, one, 0)
    perm = np.random.default_rng(0).permutation(B)                  # permuted
    got = _run(engine, model, obs[perm], n, seeds[perm])
    for i, b in enumerate(perm):
        same(b, got, i)
    other = obs.copy()                                              # neighbours replaced
    other[[0, 1, 2, 3, 5, 6, 7, 8]] = _obs(8, T, 900)
    got = _run(engine, model, other, n, seeds)
    same(4, got, 4)


def test_batch_against_the_exact_posterior(engine):
    """B = 1024 problems of hmm<16> at n = 4096: every problem's smoothed marginals near forward-backward's, and the evidence
    unbiased -- the mean over problems of exp(log Z-hat_b - log Z_b) within 4 standard errors of 1."""
    T, n, B = 16, 4096, 1024
    obs = _obs(B, T, 5000)
    engine.batch_begin(cp.MODEL_HMM3, obs, n)
    engine.batch_run(_seeds(B, 31))
    summ, stats, ess, res = engine.batch_results()
    ratio = np.zeros(B)
    worst = 0.0
    for b in range(B):
        gamma, _, logz = exact.hmm_forward_backward(obs[b])
        worst = max(worst, np.abs(stats[b] - gamma).max())
        ratio[b] = np.exp(summ[b]["log_evidence"] - logz)
    assert worst < 0.12, worst
    se = ratio.std(ddof=1) / np.sqrt(B)
    assert abs(ratio.mean() - 1.0) < 4 * se + 1e-12, (ratio.mean(), se)


def test_batch_and_single_runs_coexist_on_one_context(engine):
    T, n, B = 16, 2048, 4
    obs = _obs(B, T, 70)
    seeds = _seeds(B, 1)
    single_obs = exact.simulate_hmm(T, 12)

    def single():
        engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, single_obs, 20000, seed=3)
        engine.run(0)
        return engine.results(), engine.values()

    def batch():
        engine.batch_run(seeds)
        return engine.batch_results(), engine.batch_store(2)

    ref_single = single()
    engine.batch_begin(cp.MODEL_HMM3, obs, n)
    ref_batch = batch()
    # interleaved: begin single, run batch, run single, read both
    engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, single_obs, 20000, seed=3)
    engine.batch_run(seeds)
    engine.run(0)
    got_single = (engine.results(), engine.values())
    got_batch = (engine.batch_results(), engine.batch_store(2))
    assert got_single[0][0] == ref_single[0][0]
    for x, y in zip(got_single[0][1:], ref_single[0][1:]):
        assert np.array_equal(x, y)
    assert np.array_equal(got_single[1], ref_single[1])
    assert got_batch[0][0] == ref_batch[0][0]
    for x, y in zip(got_batch[0][1:] + got_batch[1], ref_batch[0][1:] + ref_batch[1]):
        assert np.array_equal(x, y)
    # the same seeds twice: the same outputs
    again = batch()
    assert again[0][0] == ref_batch[0][0]
    for x, y in zip(again[0][1:] + again[1], ref_batch[0][1:] + ref_batch[1]):
        assert np.array_equal(x, y)


def test_results_device_matches_the_host_read_back(engine):
    import torch
    T, n, B = 9, 600, 7
    obs = _obs(B, T, 20)
    engine.batch_begin(cp.MODEL_HMM3, obs, n, resampler=cp.RESAMPLE_STRATIFIED)
    engine.batch_run(_seeds(B))
    out = torch.zeros((B, 4 + T * 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_results_device(out)
    engine.sync()
    got = out.cpu().numpy()
    summ, stats, _, _ = engine.batch_results()
    for b in range(B):
        assert got[b, 0] == summ[b]["log_evidence"] and got[b, 1] == summ[b]["ess_final"]
        assert got[b, 2] == summ[b]["log_norm"] and got[b, 3] == summ[b]["max_logw"]
        assert np.array_equal(got[b, 4:], stats[b].reshape(-1))


def test_out_of_scope_configurations_are_refused_by_begin(engine):
    obs = _obs(2, 4)
    cases = [dict(model=cp.MODEL_HMM3, resampler=cp.RESAMPLE_MULTINOMIAL), dict(model=cp.MODEL_HMM3, ess_threshold=0.5),
             dict(model=cp.MODEL_HMM3, ess_threshold=1.0), dict(model=cp.MODEL_HMM3, algorithm=cp.ALG_SIS),
             dict(model=cp.MODEL_LINEAR_GAUSSIAN_1D), dict(model=cp.MODEL_GAUSSIAN_UNKNOWN_MEAN), dict(model=cp.MODEL_GAUSSIAN_README),
             dict(model=cp.MODEL_GAUSSIAN_2D_UNKNOWN_MEAN)]
    for kw in cases:
        model = kw.pop("model")
        with pytest.raises(cp.CpprobHipError) as e:
            engine.batch_begin(model, obs, 100, **kw)
        assert e.value.code == -4 and "single-population path" in str(e.value)
    for kw in (dict(flags=1), dict(keep_history=True, resampler=5)):
        with pytest.raises(cp.CpprobHipError) as e:
            engine.batch_begin(cp.MODEL_HMM3, obs, 100, **kw)
        assert e.value.code == -1
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_begin(cp.MODEL_HMM3, obs, cp.capi.BATCH_MAX_PARTICLES + 1)
    assert e.value.code == -1


def test_requantised_generations_resample_like_the_one_problem_engine(engine):
    """Populations of several particles in two states that BOTH sit far below the step's bound (the third state, which sets it, is
    left behind after step 0): every later generation is weighed against its exact maximum, and the comb still draws the oracle's
    ancestors among distinct weights.  n_requantised and every other number equal the one-problem engine's (settle_fixed)."""
    means, trans = [-1.0, 0.0, 10.0], [[5.0, 5.0, 0.01], [5.0, 5.0, 0.01], [1.0, 1.0, 1.0]]
    engine.set_hmm(means, trans)
    O.set_hmm(means, trans)
    T, B = 8, 4
    obs = np.full((B, T), 30.0)
    obs[:, 0] = [-0.5, -1.2, 0.3, -0.1]              # step 0 leaves (almost surely) no particle in state 2
    seeds = _seeds(B, 41)
    for n in (3, 8):
        for rs in (cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED):
            engine.batch_begin(cp.MODEL_HMM_TABLE, obs, n, resampler=rs)
            engine.batch_run(seeds)
            summ, stats, ess, res = engine.batch_results()
            stores = [engine.batch_store(b) for b in range(B)]
            for b in range(B):
                assert summ[b]["n_requantised"] > 0
                _check_problem(engine, b, obs[b], n, seeds[b], rs, cp.MODEL_HMM_TABLE, summ[b], stats[b], ess[b], res[b], k=3)
                engine.begin(cp.ALG_SMC, cp.MODEL_HMM_TABLE, obs[b], n, seed=int(seeds[b]), resampler=rs, ess_threshold=2.0)
                engine.run(0)
                s1, st1, ess1, res1 = engine.results()
                assert summ[b]["n_requantised"] == s1["n_requantised"]
                assert summ[b]["n_resampled"] == s1["n_resampled"] and np.array_equal(res[b], res1)
                assert abs(summ[b]["log_evidence"] - s1["log_evidence"]) < 1e-9 and summ[b]["max_logw"] == s1["max_logw"]
                np.testing.assert_allclose(ess[b], ess1, rtol=1e-9)
                np.testing.assert_allclose(stats[b], st1, rtol=1e-11, atol=1e-12)
                assert np.array_equal(stores[b][0], engine.values()) and np.array_equal(stores[b][1], engine.ancestors())


@pytest.mark.parametrize("row", ["systematic", "stratified"])
def test_near_ties_at_the_batch_kernels_partition_edges(engine, row):
    """tests/golden/near_ties_batch.json: every case puts one comb decision of particle k on a tie or one ulp from it, with k at the
    first / last particle of a lane's run, a wavefront or an LDS pass of the batched kernel.  All cases of a resampler run as the
    problems of ONE batch, and every problem draws the oracle's ancestors."""
    import near_ties_batch as NB
    cases = [c for c in NB.load_cases() if c["row"] == row]
    rs = cp.RESAMPLE_SYSTEMATIC if row == "systematic" else cp.RESAMPLE_STRATIFIED
    obs = np.array([[float.fromhex(h) for h in c["obs"]] for c in cases])
    seeds = np.array([c["seed"] for c in cases], np.uint64)
    engine.batch_begin(cp.MODEL_HMM3, obs, NB.N, resampler=rs)
    engine.batch_run(seeds)
    summ, stats, ess, res = engine.batch_results()
    for b, c in enumerate(cases):
        vals, anc, _ = engine.batch_store(b)
        orc = O.smc(O.MODEL_HMM3, obs[b], NB.N, c["seed"], rs, 2.0)
        assert np.array_equal(vals, orc["hist"]), c
        assert np.array_equal(anc, orc["anc"]), "%s gen %d %s gap %+d: ancestors differ from the oracle" % (row, c["gen"], c["position"], c["gap"])
        assert abs(summ[b]["log_evidence"] - orc["log_z"]) < 1e-10


def test_cpp_inference_batch_through_cpprob_main(engine, tmp_path):
    """cpprob_main --batch_observes_file: one hmm<16> problem a line, seeds --seed + line index, through cpprob::gpu::inference_batch:
    one JSON object a line, each equal to the batched run of the C ABI; the plain form prints one estimate a line."""
    import json
    import os
    import subprocess
    main = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")
    B, T, n, seed = 5, 16, 3000, 40
    obs = _obs(B, T, 700)
    (tmp_path / "batch.txt").write_text("".join("[" + " ".join(repr(float(x)) for x in row) + "]\n" for row in obs))
    base = [main, "--model_folder", str(tmp_path), "--model", "hmm16", "--smc", "--n_samples", str(n), "--seed", str(seed), "--ess_threshold", "2.0",
            "--batch_observes_file", "batch.txt"]
    p = subprocess.run(base + ["--json"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == B
    engine.batch_begin(cp.MODEL_HMM3, obs, n)
    engine.batch_run(np.arange(seed, seed + B, dtype=np.uint64))
    summ, stats, _, _ = engine.batch_results()
    for b in range(B):
        assert lines[b]["n"] == n and lines[b]["builtin"] is True
        assert abs(lines[b]["log_evidence"] - summ[b]["log_evidence"]) < 1e-12
        got = np.array([h["p"] for h in lines[b]["predicts"]])
        np.testing.assert_allclose(got, stats[b], rtol=0, atol=1e-15)
    p = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    est = [l for l in p.stdout.splitlines() if l and (l[0].isdigit() or l[0] == "-")]
    assert len(est) == B and abs(float(est[0].split()[0]) - summ[0]["log_evidence"]) < 1e-12
    # a model the batched path does not hold is refused with a message, not run
    (tmp_path / "lg.txt").write_text("[" + " ".join(["0.5"] * 25) + "]\n")
    p = subprocess.run([main, "--model_folder", str(tmp_path), "--model", "linear_gaussian_1d25", "--smc", "--n_samples", "100", "--ess_threshold", "2.0",
                        "--batch_observes_file", "lg.txt"], capture_output=True, text=True, timeout=600)
    assert p.returncode != 0 and "CPPROB_REGISTER_BUILTIN" in p.stderr
