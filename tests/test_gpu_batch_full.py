"""Full-covariance Gaussian vector emissions of a batch on the device (csrc/batch_full.hpp) against tests/full_ref.py, bit for bit."""
import functools

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import full_ref as FR
import retable_ref as RT
import suffstats_ref as SS

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
B_TWO_WALKS = 4 * 2048 + 1                                  # kWaves * kSymbolGridMax + 1: the walk's first wavefront takes a second problem
# 8 x 1.70e-9, the largest distance between the restatement chain (exact_ref + backward_ref + full_ref) and the float64 recursion over
# exactly test_exact_fit_is_baum_welch's case, measured on the CPU by tools/measure_full_tolerance.py (profiles/r42_notes.md)
TOL_BAUM_WELCH = 8 * 1.70e-9
TRI = np.tril_indices(16)


@functools.lru_cache(maxsize=None)
def _case(k, D, Ts, seed=0):
    rng = np.random.default_rng(1000 * k + 10 * D + seed)
    nb = len(Ts)
    W = rng.normal(0.0, 1.0, (nb, k, D, D))
    return {"obs": [rng.normal(0.0, 2.0, (T, D)) for T in Ts], "M": rng.normal(0.0, 2.0, (nb, k, D)),
            "C": W @ W.transpose(0, 1, 3, 2) + 0.5 * np.eye(D), "A": rng.uniform(0.05, 1.0, (nb, k, k))}


def dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def code(call, match=None):
    with pytest.raises(cp.capi.CpprobHipError, match=match) as e:
        call()
    return e.value.code


def _assert_tables(engine, obs, M, C, A, which=None):
    for b in range(engine.batch_B) if which is None else which:
        rows, thr = engine.batch_step_tables(b)
        got_m, got_L, got_l = engine.batch_copy_full(b)
        L = [FR.factor(c) for c in C[b]]
        assert np.array_equal(rows, FR.rows(obs[b], M[b], C[b])) and np.array_equal(thr, RT.thresholds(A[b], A.shape[1])), b
        assert np.array_equal(got_m, M[b]) and np.array_equal(got_L, np.array(L)) and np.array_equal(got_l, [FR.log_norm(f) for f in L]), b


def _assert_records(engine, obs, M, C, A, exact, which=None):
    """Runs the batch and holds its records against the restatement (one reference a distinct case); returns the dict and [B, 1304]."""
    k, D = M.shape[1], M.shape[2]
    if exact:
        engine.batch_run_exact()
    else:
        engine.batch_run(np.arange(engine.batch_B, dtype=np.uint64) + np.uint64(7))
    st, refs, nb = engine.batch_full_stats(obs), {}, len(obs)
    rec = np.concatenate([st["xi"].reshape(nb, -1), st["occ"], st["occ_y"], st["occ_yy"], st["sy"].reshape(nb, -1), st["syy"][:, :, TRI[0], TRI[1]].reshape(nb, -1)], axis=1)
    for b in range(engine.batch_B):
        i = b if which is None else which[b]
        if i not in refs:
            m, P = engine.batch_masses(b), R.transition_masses(A[b])
            base = SS.record(SS.stats([[int(v) for v in row[:k]] for row in m], P, obs[b][:, 0]))
            refs[i] = np.concatenate([base, FR.sums(m, P, obs[b], D)])
        assert np.array_equal(rec[b], refs[i], equal_nan=True), b
    return st, rec


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
@pytest.mark.parametrize("D", [1, 2, 5, 16])
@pytest.mark.parametrize("k", [2, 8])
def test_device_equals_the_restatement(engine, k, D, exact):
    c, new = _case(k, D, (1, 2, 37)), _case(k, D, (1, 2, 37), seed=1)
    engine.batch_begin_problems_full(c["obs"], 16, c["M"], c["C"], c["A"], keep_history=False, keep_masses=True)
    _assert_tables(engine, c["obs"], c["M"], c["C"], c["A"])
    d = dev(new["M"], new["C"], new["A"], np.concatenate(c["obs"]).reshape(-1))
    engine.batch_retable_full_device(*d)
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, c["obs"], new["M"], new["C"], new["A"])
    st, rec = _assert_records(engine, c["obs"], new["M"], new["C"], new["A"], exact)
    engine.batch_mstep_full_device(dev(rec)[0], d[0], d[1], d[2], 1e-2)
    engine.sync()
    host = cp.m_step_full(st, new["M"], new["C"], new["A"], 1e-2)
    for b in range(3):
        want = FR.m_step(rec[b], new["M"][b], new["C"][b], new["A"][b], 1e-2)
        assert all(np.array_equal(t[b].cpu().numpy(), w) and np.array_equal(h[b], w) for t, h, w in zip(d, host, want)), b


def test_many_problems_two_tiles_through_one_buffer(engine):
    """4 * 2048 + 1 problems, the longest of T = 37: retable_grid_y gives 1, so a long problem's re-table workgroup walks two tiles through
    one LDS buffer; the walk's first wavefront and the moments' workgroups take further problems; the M-step has 513 workgroups."""
    Ts = (37, 3, 2, 1, 3)
    c, new = _case(2, 2, Ts, seed=3), _case(2, 2, Ts, seed=4)
    which = np.arange(B_TWO_WALKS) % 5
    obs, (M0, C0, A0), (M, C, A) = [c["obs"][i] for i in which], [c[n][which] for n in "MCA"], [new[n][which] for n in "MCA"]
    assert RT.grid_y(37, B_TWO_WALKS) == 1
    engine.batch_begin_problems_full(obs, 4, M0, C0, A0, keep_history=False, keep_masses=True)
    d = dev(M, C, A, np.concatenate(obs).reshape(-1))
    engine.batch_retable_full_device(*d)
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, obs, M, C, A, [0, 1, B_TWO_WALKS // 2, B_TWO_WALKS - 1])
    st, rec = _assert_records(engine, obs, M, C, A, True, which)
    engine.batch_mstep_full_device(dev(rec)[0], d[0], d[1], d[2], 1e-2)
    engine.sync()
    host = cp.m_step_full(st, M, C, A, 1e-2)
    assert all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(d, host))


@pytest.mark.parametrize("D", [1, 5])
def test_diagonal_covariances_are_the_diag_family_and_one_coordinate_the_scaled(engine, D):
    c = _case(3, D, (1, 2, 37), seed=2)
    Sg = np.random.default_rng(D).uniform(0.5, 2.0, c["M"].shape)
    C = np.zeros(c["C"].shape)
    C[..., np.arange(D), np.arange(D)] = Sg * Sg
    engine.batch_begin_problems_diag(c["obs"], 8, c["M"], Sg, c["A"], keep_history=False, keep_masses=True)
    want = [(engine.batch_step_tables(b), engine.batch_copy_diag(b)[2]) for b in range(3)]
    engine.batch_run_exact()
    base = engine.batch_diag_stats(c["obs"])
    if D == 1:
        obs1 = [o[:, 0] for o in c["obs"]]
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs1, 8, tables=(c["M"][:, :, 0], c["A"], Sg[:, :, 0]), keep_history=False, keep_masses=True)
        for b in range(3):
            assert np.array_equal(engine.batch_step_tables(b)[0], want[b][0][0]) and np.array_equal(engine.batch_scales(b)[1], want[b][1]), b
    engine.batch_begin_problems_full(c["obs"], 8, c["M"], C, c["A"], keep_history=False, keep_masses=True)
    for b in range(3):
        (rows, thr), ln = want[b]
        got = engine.batch_step_tables(b)
        assert np.array_equal(got[0], rows) and np.array_equal(got[1], thr) and np.array_equal(engine.batch_copy_full(b)[2], ln), b
    engine.batch_run_exact()
    st = engine.batch_full_stats(c["obs"])
    assert all(np.array_equal(st[n], base[n]) for n in ("xi", "occ", "occ_y", "occ_yy"))
    assert np.array_equal(st["sy"][:, :, :D], base["sy"][:, :, :D]) and np.array_equal(st["syy"][:, :, np.arange(D), np.arange(D)], base["syy"][:, :, :D])


@pytest.mark.parametrize("bad", ["pivot", "nan"])
def test_a_covariance_that_does_not_factor_is_refused_for_its_problem_alone(engine, bad):
    c, new = _case(3, 5, (4, 6, 3)), _case(3, 5, (4, 6, 3), seed=1)
    C = new["C"].copy()
    if bad == "pivot":
        C[1, 2] = C[1, 2] - 1.0001 * np.linalg.eigvalsh(C[1, 2])[0] * np.eye(5)    # (the smallest eigenvalue below zero: the last pivot fails)
    else:
        C[1, 2, 4, 1] = np.nan
    assert FR.factor(C[1, 2]) is None
    assert code(lambda: engine.batch_begin_problems_full(c["obs"], 8, c["M"], C, c["A"]), "problem 1: a covariance") == EINVAL
    engine.batch_begin_problems_full(c["obs"], 8, c["M"], c["C"], c["A"], keep_history=False, keep_masses=True)
    engine.batch_retable_full_device(*dev(new["M"], C, new["A"], np.concatenate(c["obs"]).reshape(-1)))
    assert list(engine.batch_retable_status()) == [0, FR.BAD_COV, 0]
    _assert_tables(engine, c["obs"], c["M"], c["C"], c["A"], [1])
    _assert_tables(engine, c["obs"], new["M"], C, new["A"], [0, 2])
    assert code(lambda: engine.batch_retable_full(new["M"], C, new["A"], c["obs"]), "problem 1") == EINVAL


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
def test_resident_fit_equals_the_host_loop(engine, exact):
    c = _case(3, 5, (12, 9, 12, 9), seed=5)
    host = cp.hmm_full_em(engine, c["obs"], c["M"], c["C"], c["A"], 32, np.arange(4), 3, exact=exact)
    res = cp.hmm_full_em(engine, c["obs"], c["M"], c["C"], c["A"], 32, np.arange(4), 3, exact=exact, resident=True)
    assert all(np.array_equal(x, y) for x, y in zip(host, res)) and np.isfinite(host[3]).all() and not np.array_equal(host[0][0], host[0][3])


def correlated_case():
    """k = 2, D = 3, two sequences of 37 steps from states with correlated coordinates (the case tools/measure_full_tolerance.py measures)."""
    rng = np.random.default_rng(42)
    mix = np.array([[1.0, 0.0, 0.0], [0.8, 0.6, 0.0], [-0.5, 0.3, 0.7]])
    obs = [(rng.normal(0.0, 1.0, (37, 3)) @ mix.T) + np.where(rng.random((37, 1)) < 0.5, 1.5, -1.5) for _ in range(2)]
    M = rng.normal(0.0, 1.0, (2, 2, 3))
    C = np.broadcast_to(mix @ mix.T + 0.5 * np.eye(3), (2, 2, 3, 3)).copy()
    return obs, M, C, rng.uniform(0.2, 1.0, (2, 2, 2))


def baum_welch(obs, M0, C0, A0, iterations, floor=1e-6):
    """Float64 Baum-Welch of one HMM with full-covariance Gaussian emissions, uniform initial state, hmm_full_em's M-step."""
    M, C, A, y = np.array(M0, np.float64), np.array(C0, np.float64), np.array(A0, np.float64), np.asarray(obs, np.float64)
    k, hist = M.shape[0], [(M.copy(), C.copy(), A.copy())]
    for _ in range(iterations):
        P = A / A.sum(axis=1, keepdims=True)
        r = y[:, None, :] - M[None]
        logb = -0.5 * (np.einsum("tsi,sij,tsj->ts", r, np.linalg.inv(C), r) + np.log(np.linalg.det(2 * np.pi * C))[None])
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
        occ = gamma.sum(axis=0)
        A = np.where(xi.sum(axis=1, keepdims=True) > 0, xi / xi.sum(axis=1, keepdims=True), A)
        M = (gamma.T @ y) / occ[:, None]
        C = np.einsum("ts,ti,tj->sij", gamma, y, y) / occ[:, None, None] - M[:, :, None] * M[:, None, :]
        d = np.arange(C.shape[1])
        C[:, d, d] = np.maximum(C[:, d, d], floor * floor)
        hist.append((M.copy(), C.copy(), A.copy()))
    return [np.array(h) for h in zip(*hist)]


def test_exact_fit_is_baum_welch(engine):
    obs, M, C, A = correlated_case()
    got = cp.hmm_full_em(engine, obs, M, C, A, 8, [1, 2], 5, exact=True)
    for b in range(2):
        want = baum_welch(obs[b], M[b], C[b], A[b], 5)
        dist = [np.abs(g[1:, b] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: means %.3g, covariances %.3g, transition rows %.3g" % (b, *dist))
        assert max(dist) <= TOL_BAUM_WELCH


def test_cross_family_calls_are_refused_and_the_batch_stays(engine):
    c = _case(2, 3, (4, 5))
    obs1, Sg = [o[:, 0] for o in c["obs"]], np.ones((2, 2, 3))
    obs, M, C, A, S3, means, rec88, rec600, rec = dev(np.concatenate(c["obs"]).reshape(-1), c["M"], c["C"], c["A"], Sg, np.ones((2, 2)), np.zeros((2, 88)),
                                                      np.zeros((2, 600)), np.zeros((2, FR.RECORD)))
    for D in (0, 17):
        assert code(lambda: engine.batch_begin_problems_full(c["obs"], 8, np.ones((2, 2, D)), np.ones((2, 2, D, D)), c["A"])) == EINVAL
    engine.batch_begin_problems_full(c["obs"], 8, c["M"], c["C"], c["A"], keep_history=False, keep_masses=True)
    engine.batch_run_exact()
    calls = [lambda: engine.batch_retable_device(means, A, obs), lambda: engine.batch_retable_device(means, A, obs, sigmas=means),
             lambda: engine.batch_retable_categorical_device(M, A, obs),
             lambda: engine.batch_retable_diag_device(M, S3, A, obs), lambda: engine.batch_retable_diag(c["M"], Sg, c["A"], c["obs"]),
             lambda: engine.batch_mstep_device(rec88, means, A), lambda: engine.batch_mstep_device(rec88, means, A, sigmas=means),
             lambda: engine.batch_mstep_categorical_device(rec600, M, A),
             lambda: engine.batch_mstep_diag_device(rec600, M, S3, A), lambda: engine.batch_diag_stats(c["obs"]), lambda: engine.batch_diag_stats_device(rec600, obs),
             lambda: engine.batch_copy_diag(0, 2, 3), lambda: engine.batch_draw_tables_device(rec88, dev(np.zeros(2, np.int64))[0], 0, means, A),
             lambda: engine.batch_learn_begin(np.ones(8), 1), lambda: engine.batch_online_tables((np.ones((2, 2)), c["A"])),
             lambda: engine.batch_smooth_stats(obs1), lambda: engine.batch_smooth_stats_device(rec88, obs),
             lambda: engine.batch_symbol_stats(obs1), lambda: engine.batch_traj_stats(4, 0, obs1)]
    assert [code(f) for f in calls] == [ESTATE] * len(calls)
    assert code(lambda: engine.batch_draw_tables_device(rec88, dev(np.zeros(2, np.int64))[0], 0, means, A), "full-covariance") == ESTATE
    _assert_tables(engine, c["obs"], c["M"], c["C"], c["A"])      # (the batch as it was, and its run still serves)
    assert np.isfinite(engine.batch_full_stats(c["obs"])["syy"]).all()
    assert code(lambda: engine.batch_full_stats(obs1)) == EINVAL and code(lambda: engine.batch_mstep_full_device(rec, M, C, A, 0.0)) == EINVAL
    engine.batch_begin_problems_diag(c["obs"], 8, c["M"], Sg, c["A"], keep_history=False, keep_masses=True)
    engine.batch_run_exact()
    calls = [lambda: engine.batch_retable_full_device(M, C, A, obs), lambda: engine.batch_retable_full(c["M"], c["C"], c["A"], c["obs"]),
             lambda: engine.batch_full_stats_device(rec, obs), lambda: engine.batch_full_stats(c["obs"]),
             lambda: engine.batch_mstep_full_device(rec, M, C, A), lambda: engine.batch_copy_full(0, 2, 3)]
    assert [code(f) for f in calls] == [ESTATE] * len(calls)
