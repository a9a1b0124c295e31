"""Diagonal-Gaussian vector emissions of a batch on the device (csrc/batch_diag.hpp) against tests/diag_ref.py, bit for bit."""
import functools

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import diag_ref as DR
import exact_ref as X
import retable_ref as RT
import scale_ref as S
import suffstats_ref as SS

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
B_TWO_WALKS = 4 * 2048 + 1                                  # kWaves * kSymbolGridMax + 1: the first wavefront walks a second problem
# 8 x 2.66e-9, the largest distance between the restatement chain (exact_ref + backward_ref + diag_ref) and the float64 recursion over
# exactly test_exact_fit_is_baum_welch's cases, measured on the CPU by tools/measure_diag_tolerance.py (profiles/r41_notes.md)
TOL_BAUM_WELCH = 8 * 2.66e-9


@functools.lru_cache(maxsize=None)
def _case(k, D, Ts, seed=0):
    rng = np.random.default_rng(1000 * k + 10 * D + seed)
    nb = len(Ts)
    return {"obs": [rng.normal(0.0, 2.0, (T, D)) for T in Ts], "M": rng.normal(0.0, 2.0, (nb, k, D)), "S": rng.uniform(0.5, 2.0, (nb, k, D)),
            "A": rng.uniform(0.05, 1.0, (nb, k, k))}


def dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def code(call, match=None):
    with pytest.raises(cp.capi.CpprobHipError, match=match) as e:
        call()
    return e.value.code


def _assert_tables(engine, obs, M, Sg, A, which=None):
    for b in range(engine.batch_B) if which is None else which:
        rows, thr = engine.batch_step_tables(b)
        got_m, got_s, got_l = engine.batch_copy_diag(b)
        assert np.array_equal(rows, DR.rows(obs[b], M[b], Sg[b])) and np.array_equal(thr, RT.thresholds(A[b], A.shape[1])), b
        assert np.array_equal(got_m, M[b]) and np.array_equal(got_s, Sg[b]) and np.array_equal(got_l, DR.log_norms(Sg[b])), b


def _assert_records(engine, obs, M, Sg, A, exact, which=None):
    """Runs the batch and holds its records against the restatement (one reference a distinct case); returns the records [B, 600]."""
    k, D = M.shape[1], M.shape[2]
    if exact:
        engine.batch_run_exact()
    else:
        engine.batch_run(np.arange(engine.batch_B, dtype=np.uint64) + np.uint64(7))
    st, refs = engine.batch_diag_stats(obs), {}
    rec = np.concatenate([st["xi"].reshape(len(obs), -1), st["occ"], st["occ_y"], st["occ_yy"], np.stack([st["sy"], st["syy"]], axis=2).reshape(len(obs), -1)], axis=1)
    for b in range(engine.batch_B):
        i = b if which is None else which[b]
        if i not in refs:
            m, P = engine.batch_masses(b), R.transition_masses(A[b])
            if exact:
                want_m, _, dead = X.run(DR.rows(obs[b], M[b], Sg[b])[:, :k].tolist(), P)
                assert np.array_equal(m, np.array(want_m)) and engine.batch_exact_evidence()[1][b] == dead
            sy, syy = DR.sums(m, P, obs[b], D)
            base = SS.record(SS.stats([[int(v) for v in row[:k]] for row in m], P, obs[b][:, 0]))
            refs[i] = np.concatenate([base, np.stack([sy, syy], axis=1).reshape(-1)])
        assert np.array_equal(rec[b], refs[i], equal_nan=True), b
    return st, rec


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
@pytest.mark.parametrize("D", [1, 2, 9, 32])
@pytest.mark.parametrize("k", [2, 8])
def test_device_equals_the_restatement(engine, k, D, exact):
    c, new = _case(k, D, (1, 2, 37)), _case(k, D, (1, 2, 37), seed=1)
    engine.batch_begin_problems_diag(c["obs"], 16, c["M"], c["S"], c["A"], keep_history=False, keep_masses=True)
    _assert_tables(engine, c["obs"], c["M"], c["S"], c["A"])
    d = dev(new["M"], new["S"], new["A"], np.concatenate(c["obs"]).reshape(-1))
    engine.batch_retable_diag_device(*d)
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, c["obs"], new["M"], new["S"], new["A"])
    st, rec = _assert_records(engine, c["obs"], new["M"], new["S"], new["A"], exact)
    engine.batch_mstep_diag_device(dev(rec)[0], d[0], d[1], d[2], 1e-2)
    engine.sync()
    host = cp.m_step_diag(st, new["M"], new["S"], new["A"], 1e-2)
    for b in range(3):
        want = DR.m_step(rec[b], new["M"][b], new["S"][b], new["A"][b], 1e-2)
        assert all(np.array_equal(t[b].cpu().numpy(), w) and np.array_equal(h[b], w) for t, h, w in zip(d, host, want)), b


def test_one_coordinate_is_the_scaled_family(engine):
    c = _case(3, 1, (1, 2, 37), seed=2)
    obs1, M1, S1 = [o[:, 0] for o in c["obs"]], c["M"][:, :, 0], c["S"][:, :, 0]
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs1, 8, tables=(M1, c["A"], S1), keep_history=False, keep_masses=True)
    want_rows, want_ln = [engine.batch_step_tables(b)[0] for b in range(3)], [engine.batch_scales(b)[1] for b in range(3)]
    engine.batch_run_exact()
    base = engine.batch_smooth_stats(obs1)
    want = dev(np.concatenate([base["xi"].reshape(3, -1), base["occ"], base["occ_y"], base["occ_yy"]], axis=1), M1, c["A"], S1)
    engine.batch_mstep_device(want[0], want[1], want[2], sigmas=want[3], sigma_floor=1e-2)
    engine.sync()
    engine.batch_begin_problems_diag(c["obs"], 8, c["M"], c["S"], c["A"], keep_history=False, keep_masses=True)
    for b in range(3):
        assert np.array_equal(engine.batch_step_tables(b)[0], want_rows[b]) and np.array_equal(engine.batch_copy_diag(b)[2], want_ln[b]), b
    st, rec = _assert_records(engine, c["obs"], c["M"], c["S"], c["A"], True)
    assert all(np.array_equal(st[name], base[name]) for name in base)
    assert np.array_equal(st["sy"][:, :, 0], base["occ_y"]) and np.array_equal(st["syy"][:, :, 0], base["occ_yy"])
    got = dev(rec, c["M"], c["S"], c["A"])
    engine.batch_mstep_diag_device(*got, 1e-2)
    engine.sync()
    assert all(np.array_equal(g.cpu().numpy().reshape(w.shape), w.cpu().numpy()) for g, w in zip(got[1:], (want[1], want[3], want[2])))


def test_two_tiles_through_one_buffer_and_a_wavefront_that_walks_two_problems(engine):
    """4 * 2048 + 1 problems of T = 37: retable_grid_y gives 1, so every re-table workgroup walks two tiles through its one LDS buffer,
    the second of 5 rows; the first wavefront of the statistics walk takes a second problem."""
    c, new = _case(2, 9, (37,) * 5, seed=3), _case(2, 9, (37,) * 5, seed=4)
    which = np.arange(B_TWO_WALKS) % 5
    obs, (M0, S0, A0), (M, Sg, A) = [c["obs"][i] for i in which], [c[n][which] for n in "MSA"], [new[n][which] for n in "MSA"]
    assert RT.grid_y(37, B_TWO_WALKS) == 1
    engine.batch_begin_problems_diag(obs, 4, M0, S0, A0, keep_history=False, keep_masses=True)
    engine.batch_retable_diag_device(*dev(M, Sg, A, np.concatenate(obs).reshape(-1)))
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, obs, M, Sg, A, [0, B_TWO_WALKS // 2, B_TWO_WALKS - 1])
    _assert_records(engine, obs, M, Sg, A, True, which)


@pytest.mark.parametrize("bad", [0.0, -0.5, np.nan, 1e-310], ids=["zero", "negative", "nan", "subnormal"])
def test_an_infinite_coordinate_and_a_bad_sigma_refused_for_its_problem_alone(engine, bad):
    c, new = _case(3, 5, (4, 6, 3)), _case(3, 5, (4, 6, 3), seed=1)
    obs = [o.copy() for o in c["obs"]]
    obs[0][2, 3] = -np.inf
    Sg = new["S"].copy()
    Sg[1, 2, 4] = bad
    assert code(lambda: engine.batch_begin_problems_diag(obs, 8, c["M"], Sg, c["A"]), "problem 1: emission scales") == EINVAL
    engine.batch_begin_problems_diag(obs, 8, c["M"], c["S"], c["A"], keep_history=False, keep_masses=True)
    assert np.isneginf(engine.batch_step_tables(0)[0][2]).all() and np.isfinite(engine.batch_step_tables(0)[0][[0, 1, 3], :3]).all()
    engine.batch_run_exact()
    assert list(engine.batch_exact_evidence()[1]) == [2, -1, -1]
    engine.batch_retable_diag_device(*dev(new["M"], Sg, new["A"], np.concatenate(obs).reshape(-1)))
    assert list(engine.batch_retable_status()) == [0, S.BAD_SCALE, 0] and DR.check(new["M"][1], Sg[1], new["A"][1]) == S.BAD_SCALE
    _assert_tables(engine, obs, c["M"], c["S"], c["A"], [1])
    _assert_tables(engine, obs, new["M"], Sg, new["A"], [0, 2])
    assert code(lambda: engine.batch_retable_diag(new["M"], Sg, new["A"], obs), "problem 1") == EINVAL


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
def test_resident_fit_equals_the_host_loop(engine, exact):
    c = _case(3, 5, (12, 9, 12, 9), seed=5)
    host = cp.hmm_diag_em(engine, c["obs"], c["M"], c["S"], c["A"], 32, np.arange(4), 3, exact=exact)
    res = cp.hmm_diag_em(engine, c["obs"], c["M"], c["S"], c["A"], 32, np.arange(4), 3, exact=exact, resident=True)
    assert all(np.array_equal(x, y) for x, y in zip(host, res)) and np.isfinite(host[3]).all() and not np.array_equal(host[0][0], host[0][3])


def baum_welch(obs, M0, S0, A0, iterations, floor=1e-3):
    """Float64 Baum-Welch of one HMM with diagonal-Gaussian emissions, uniform initial state, hmm_diag_em's M-step (the floor)."""
    M, Sg, A, y = np.array(M0, np.float64), np.array(S0, np.float64), np.array(A0, np.float64), np.asarray(obs, np.float64)
    k, hist = M.shape[0], [(M.copy(), Sg.copy(), A.copy())]
    for _ in range(iterations):
        P = A / A.sum(axis=1, keepdims=True)
        logb = -0.5 * ((((y[:, None, :] - M[None]) / Sg[None]) ** 2).sum(axis=2) + np.log(2 * np.pi * Sg * Sg).sum(axis=1)[None])
        lik = np.exp(logb - logb.max(axis=1, keepdims=True))
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
        occ = gamma.sum(axis=0)[:, None]
        A = np.where(xi.sum(axis=1, keepdims=True) > 0, xi / xi.sum(axis=1, keepdims=True), A)
        M = (gamma.T @ y) / occ
        v = (gamma.T @ (y * y)) / occ - M * M
        Sg = np.where(v >= floor * floor, np.sqrt(np.maximum(v, 0.0)), floor)
        hist.append((M.copy(), Sg.copy(), A.copy()))
    return [np.array(h) for h in zip(*hist)]


def test_exact_fit_is_baum_welch(engine):
    c = _case(2, 3, (37, 37), seed=6)
    got = cp.hmm_diag_em(engine, c["obs"], c["M"], c["S"], c["A"], 8, [1, 2], 5, exact=True)
    for b in range(2):
        want = baum_welch(c["obs"][b], c["M"][b], c["S"][b], c["A"][b], 5)
        dist = [np.abs(g[1:, b] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: means %.3g, sigmas %.3g, transition rows %.3g" % (b, *dist))
        assert max(dist) <= TOL_BAUM_WELCH


def test_cross_family_calls_are_refused_and_the_batch_stays(engine):
    c = _case(2, 3, (4, 5))
    obs1 = [o[:, 0] for o in c["obs"]]
    obs, M, Sg, A, means, rec88, rec = dev(np.concatenate(c["obs"]).reshape(-1), c["M"], c["S"], c["A"], np.ones((2, 2)), np.zeros((2, 88)), np.zeros((2, DR.RECORD)))
    for D in (0, 33):
        assert code(lambda: engine.batch_begin_problems_diag(c["obs"], 8, np.ones((2, 2, D)), np.ones((2, 2, D)), c["A"])) == EINVAL
    engine.batch_begin_problems_diag(c["obs"], 8, c["M"], c["S"], c["A"], keep_history=False, keep_masses=True)
    engine.batch_run_exact()
    calls = [lambda: engine.batch_retable_device(means, A, obs), lambda: engine.batch_retable_device(means, A, obs, sigmas=means),
             lambda: engine.batch_retable_device(means, A, obs, emission="poisson"), lambda: engine.batch_retable_categorical_device(M, A, obs),
             lambda: engine.batch_mstep_device(rec88, means, A), lambda: engine.batch_mstep_device(rec88, means, A, sigmas=means),
             lambda: engine.batch_mstep_device(rec88, means, A, emission="poisson"), lambda: engine.batch_mstep_categorical_device(rec, M, A),
             lambda: engine.batch_draw_tables_device(rec88, dev(np.zeros(2, np.int64))[0], 0, means, A),
             lambda: engine.batch_learn_begin(np.ones(8), 1), lambda: engine.batch_online_tables((np.ones((2, 2)), c["A"])),
             lambda: engine.batch_smooth_stats(obs1), lambda: engine.batch_smooth_stats(), lambda: engine.batch_smooth_stats_device(rec88, obs),
             lambda: engine.batch_symbol_stats(obs1), lambda: engine.batch_symbol_stats_device(rec, obs), lambda: engine.batch_traj_stats(4, 0, obs1)]
    assert [code(f) for f in calls] == [ESTATE] * len(calls)
    _assert_tables(engine, c["obs"], c["M"], c["S"], c["A"])      # (the batch as it was, and its run still serves)
    assert np.isfinite(engine.batch_diag_stats(c["obs"])["sy"]).all()
    assert code(lambda: engine.batch_diag_stats(obs1)) == EINVAL and code(lambda: engine.batch_mstep_diag_device(rec, M, Sg, A, 0.0)) == EINVAL
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs1, 8, tables=(c["M"][:, :, 0], c["A"], c["S"][:, :, 0]), keep_history=False, keep_masses=True)
    before = engine.batch_step_tables(1)
    engine.batch_run_exact()
    calls = [lambda: engine.batch_retable_diag_device(M, Sg, A, obs), lambda: engine.batch_retable_diag(c["M"], c["S"], c["A"], c["obs"]),
             lambda: engine.batch_diag_stats_device(rec, obs), lambda: engine.batch_diag_stats(c["obs"]),
             lambda: engine.batch_mstep_diag_device(rec, M, Sg, A), lambda: engine.batch_copy_diag(0, 2, 3)]
    assert [code(f) for f in calls] == [ESTATE] * len(calls)
    assert all(np.array_equal(x, y) for x, y in zip(before, engine.batch_step_tables(1)))
