"""Switching-regression emissions of a batch on the device (csrc/batch_reg.hpp) against tests/reg_ref.py, bit for bit."""
import functools

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import full_ref as FR
import reg_ref as RR
import retable_ref as RT
import suffstats_ref as SS

pytestmark = pytest.mark.gpu

ESTATE = -3
B_TWO_WALKS = 4 * 2048 + 1                                  # kWaves * kSymbolGridMax + 1: the walk, the moments and the M-step stride
# 8 x 3.57e-10, the largest distance between the restatement chain (exact_ref + backward_ref + full_ref + reg_ref) and the float64
# recursion over exactly test_exact_fit_is_baum_welch's case, measured on the CPU by tools/measure_reg_tolerance.py (profiles/r44_notes.md)
TOL_BAUM_WELCH = 8 * 3.57e-10
TRI = np.tril_indices(16)


@functools.lru_cache(maxsize=None)
def _case(k, P, Ts, seed=0):
    rng = np.random.default_rng(1000 * k + 10 * P + seed)
    nb = len(Ts)
    return {"obs": [rng.normal(0.0, 1.5, (T, 1 + P)) for T in Ts], "C": rng.normal(0.0, 1.0, (nb, k, P)), "S": rng.uniform(0.5, 2.0, (nb, k)),
            "A": rng.uniform(0.05, 1.0, (nb, k, k))}


def dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def _begin(engine, obs, c, n=16):
    return engine.batch_begin_problems_reg(obs, n, c["C"], c["S"], c["A"], keep_history=False, keep_masses=True)


def _assert_tables(engine, obs, C, S, A, which=None):
    for b in range(engine.batch_B) if which is None else which:
        rows, thr = engine.batch_step_tables(b)
        got = engine.batch_copy_reg(b)
        assert np.array_equal(rows, RR.rows(obs[b], C[b], S[b])) and np.array_equal(thr, RT.thresholds(A[b], A.shape[1])), b
        assert np.array_equal(got[0], C[b]) and np.array_equal(got[1], S[b]) and np.array_equal(got[2], [RR.S.log_norm(v) for v in S[b]]), b


def _records(engine, obs, A, exact, which=None):
    """Runs the batch and holds its records against the restatement (one reference a distinct case); returns the dict and [B, 1304]."""
    k, D, nb = A.shape[1], obs[0].shape[1], len(obs)
    engine.batch_run_exact() if exact else engine.batch_run(np.arange(nb, dtype=np.uint64) + np.uint64(7))
    st, refs = engine.batch_reg_stats(obs), {}
    rec = np.concatenate([st["xi"].reshape(nb, -1), st["occ"], st["occ_y"], st["occ_yy"], st["sy"].reshape(nb, -1), st["syy"][:, :, TRI[0], TRI[1]].reshape(nb, -1)], axis=1)
    for b in range(nb):
        i = b if which is None else which[b]
        if i not in refs:
            m, P = engine.batch_masses(b), R.transition_masses(A[b])
            refs[i] = np.concatenate([SS.record(SS.stats([[int(v) for v in row[:k]] for row in m], P, obs[b][:, 0])), FR.sums(m, P, obs[b], D)])
        assert np.array_equal(rec[b], refs[i], equal_nan=True), b
    return st, rec


def _mstep(engine, rec, C, S, A, floor=1e-2):
    d = dev(rec, C, S, A, np.full(S.shape, np.nan))
    engine.batch_mstep_reg_device(d[0], d[1], d[2], d[3], floor, log_norms=d[4])
    engine.sync()
    return [t.cpu().numpy() for t in (d[1], d[2], d[4], d[3])]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
@pytest.mark.parametrize("P", [1, 2, 5, 15])
@pytest.mark.parametrize("k", [2, 8])
def test_device_equals_the_restatement(engine, k, P, exact):
    """Three problems of T = 1, 2 and 37 (two tiles of 32): an odd count, so the M-step's last half-workgroup is idle."""
    c, new = _case(k, P, (1, 2, 37)), _case(k, P, (1, 2, 37), seed=1)
    _begin(engine, c["obs"], c)
    _assert_tables(engine, c["obs"], c["C"], c["S"], c["A"])
    engine.batch_retable_reg_device(*dev(new["C"], new["S"], new["A"], np.concatenate(c["obs"]).reshape(-1)))
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, c["obs"], new["C"], new["S"], new["A"])
    st, rec = _records(engine, c["obs"], new["A"], exact)
    got, host = _mstep(engine, rec, new["C"], new["S"], new["A"]), cp.m_step_reg(st, new["C"], new["S"], new["A"], 1e-2)
    for b in range(3):
        want = RR.m_step(rec[b], new["C"][b], new["S"][b], new["A"][b], 1e-2)
        assert all(np.array_equal(g[b], w, equal_nan=True) for g, w in zip(got, want)), b
        assert all(np.array_equal(h[b], w) for h, w in zip(host, (want[0], want[1], want[3]))), b


def test_many_problems_stride_every_kernel(engine):
    Ts = (37, 3, 2, 1, 3)
    c, new = _case(2, 2, Ts, seed=3), _case(2, 2, Ts, seed=4)
    which = np.arange(B_TWO_WALKS) % 5
    obs, old, (C, S, A) = [c["obs"][i] for i in which], {n: c[n][which] for n in "CSA"}, [new[n][which] for n in "CSA"]
    _begin(engine, obs, old, 4)
    engine.batch_retable_reg_device(*dev(C, S, A, np.concatenate(obs).reshape(-1)))
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, obs, C, S, A, [0, 1, B_TWO_WALKS // 2, B_TWO_WALKS - 1])
    st, rec = _records(engine, obs, A, True, which)
    got, host = _mstep(engine, rec, C, S, A), cp.m_step_reg(st, C, S, A, 1e-2)
    assert all(np.array_equal(got[i], host[j]) for i, j in ((0, 0), (1, 1), (3, 2))) and not np.array_equal(got[0], C)


def test_one_covariate_of_ones_is_the_scaled_family(engine):
    c = _case(3, 1, (1, 2, 37), seed=2)
    obs, obs1 = [np.column_stack([o[:, 0], np.ones(len(o))]) for o in c["obs"]], [o[:, 0] for o in c["obs"]]
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs1, 8, tables=(c["C"][:, :, 0], c["A"], c["S"]), keep_history=False, keep_masses=True)
    want = [(engine.batch_step_tables(b), engine.batch_scales(b)[1]) for b in range(3)]
    engine.batch_run_exact()
    base = engine.batch_smooth_stats(obs1)
    d = dev(np.concatenate([base["xi"].reshape(3, -1), base["occ"], base["occ_y"], base["occ_yy"]], axis=1), c["C"][:, :, 0], c["A"], c["S"], np.full((3, 3), np.nan))
    engine.batch_mstep_device(d[0], d[1], d[2], sigmas=d[3], sigma_floor=1e-2, log_norms=d[4])
    engine.sync()
    _begin(engine, obs, c, 8)
    for b in range(3):
        got = engine.batch_step_tables(b)
        assert np.array_equal(got[0], want[b][0][0]) and np.array_equal(got[1], want[b][0][1]) and np.array_equal(engine.batch_copy_reg(b)[2], want[b][1]), b
    st, rec = _records(engine, obs, c["A"], True)
    assert all(np.array_equal(st[n], base[n]) for n in ("xi", "occ", "occ_y", "occ_yy"))
    got = _mstep(engine, rec, c["C"], c["S"], c["A"])
    assert all(np.array_equal(g.reshape(-1), t.cpu().numpy().reshape(-1), equal_nan=True) for g, t in zip(got, (d[1], d[3], d[4], d[2])))


def test_bad_tables_are_refused_for_their_problem_alone_and_collinear_states_are_kept(engine):
    c, new = _case(3, 2, (4, 6, 3)), _case(3, 2, (4, 6, 3), seed=1)
    C, S = new["C"].copy(), new["S"].copy()
    C[0, 1, 1], S[2, 0] = np.nan, 0.0
    _begin(engine, c["obs"], c, 8)
    engine.batch_retable_reg_device(*dev(C, S, new["A"], np.concatenate(c["obs"]).reshape(-1)))
    assert list(engine.batch_retable_status()) == [4, 0, 8]
    _assert_tables(engine, c["obs"], c["C"], c["S"], c["A"], [0, 2])
    _assert_tables(engine, c["obs"], C, S, new["A"], [1])
    obs = [np.column_stack([o, o[:, 2]]) for o in c["obs"]]            # (covariates 1 and 2 are one column: every last pivot is exactly 0.0)
    dup = {"C": np.concatenate([c["C"], c["C"][:, :, :1]], axis=2), "S": c["S"], "A": c["A"]}
    _begin(engine, obs, dup, 8)
    st, rec = _records(engine, obs, c["A"], True)
    got, host = _mstep(engine, rec, dup["C"], dup["S"], dup["A"]), cp.m_step_reg(st, dup["C"], dup["S"], dup["A"], 1e-2)
    assert np.array_equal(got[0], dup["C"]) and np.array_equal(got[1], dup["S"]) and np.isnan(got[2]).all() and not np.array_equal(got[3], dup["A"])
    assert all(np.array_equal(got[i], host[j]) for i, j in ((0, 0), (1, 1), (3, 2)))
    calls = [lambda: engine.batch_retable_full_device(*dev(c["C"], np.ones((3, 3, 2, 2)), c["A"], np.zeros(39))), lambda: engine.batch_full_stats(obs),
             lambda: engine.batch_smooth_stats([o[:, 0] for o in obs]), lambda: engine.batch_mstep_device(*dev(rec[:, :88], c["S"], c["A"])),
             lambda: engine.batch_draw_tables_device(*dev(rec[:, :88], np.zeros(3, np.int64)), 0, *dev(c["S"], c["A"]))]
    for call in calls:                                                  # (another family's calls: refused, and the batch stays)
        with pytest.raises(cp.capi.CpprobHipError) as e:
            call()
        assert e.value.code == ESTATE
    _assert_tables(engine, obs, dup["C"], dup["S"], dup["A"])


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
def test_resident_fit_equals_the_host_loop(engine, exact):
    c = _case(3, 3, (12, 9, 12, 9), seed=5)
    host = cp.hmm_reg_em(engine, c["obs"], c["C"], c["S"], c["A"], 32, np.arange(4), 3, exact=exact)
    res = cp.hmm_reg_em(engine, c["obs"], c["C"], c["S"], c["A"], 32, np.arange(4), 3, exact=exact, resident=True)
    assert all(np.array_equal(x, y) for x, y in zip(host, res)) and np.isfinite(host[3]).all() and not np.array_equal(host[0][0], host[0][3])


def switching_case():
    """k = 2, P = 2 with an intercept, two sequences of 200 steps from overlapping regimes (the case tools/measure_reg_tolerance.py
    measures): slopes 0.5 and -0.5, intercepts 0.3 and -0.3, noise 1.0, so that no posterior is 0 or 1."""
    rng = np.random.default_rng(44)
    obs = []
    for _ in range(2):
        x, s = rng.normal(0.0, 1.0, 200), np.cumsum(rng.random(200) < 0.1) % 2
        obs.append(np.column_stack([np.where(s == 0, 0.3 + 0.5 * x, -0.3 - 0.5 * x) + rng.normal(0.0, 1.0, 200), np.ones(200), x]))
    C = np.array([[[0.5, 0.8], [-0.5, -0.8]]] * 2) + rng.normal(0.0, 0.1, (2, 2, 2))
    return obs, C, np.full((2, 2), 1.5), np.array([[[0.8, 0.2], [0.3, 0.7]]] * 2)


def baum_welch(obs, C0, S0, A0, iterations, floor=1e-3):
    """Float64 Baum-Welch of one switching regression, uniform initial state, weighted least squares by numpy.linalg.solve."""
    C, Sg, A, y, x = np.array(C0, np.float64), np.array(S0, np.float64), np.array(A0, np.float64), obs[:, 0], obs[:, 1:]
    k, hist = len(C), [(C.copy(), Sg.copy(), A.copy())]
    for _ in range(iterations):
        P = A / A.sum(axis=1, keepdims=True)
        logb = -0.5 * (((y[:, None] - x @ C.T) / Sg) ** 2 + np.log(2 * np.pi * Sg * Sg))
        lik = np.exp(logb - logb.max(axis=1, keepdims=True))
        alpha, beta, a, xi = np.zeros((len(y), k)), np.ones((len(y), k)), np.full(k, 1.0 / k), np.zeros((k, k))
        for t in range(len(y)):
            alpha[t] = a * lik[t] / (a * lik[t]).sum()
            a = alpha[t] @ P
        for t in range(len(y) - 2, -1, -1):
            pair = alpha[t][:, None] * P * (lik[t + 1] * beta[t + 1])[None, :]
            xi += pair / pair.sum()
            beta[t] = P @ (lik[t + 1] * beta[t + 1])
            beta[t] /= beta[t].sum()
        g = alpha * beta / (alpha * beta).sum(axis=1, keepdims=True)
        A = xi / xi.sum(axis=1, keepdims=True)
        C = np.array([np.linalg.solve((x * g[:, s:s + 1]).T @ x, (x * g[:, s:s + 1]).T @ y) for s in range(k)])
        Sg = np.maximum(np.sqrt((g * (y[:, None] - x @ C.T) ** 2).sum(axis=0) / g.sum(axis=0)), floor)
        hist.append((C.copy(), Sg.copy(), A.copy()))
    return [np.array(h) for h in zip(*hist)]


def test_exact_fit_is_baum_welch(engine):
    obs, C, Sg, A = switching_case()
    got = cp.hmm_reg_em(engine, obs, C, Sg, A, 8, [1, 2], 5, exact=True)
    for b in range(2):
        want = baum_welch(obs[b], C[b], Sg[b], A[b], 5)
        dist = [np.abs(g[1:, b] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: coefficients %.3g, sigmas %.3g, transition rows %.3g" % (b, *dist))
        assert max(dist) <= TOL_BAUM_WELCH
