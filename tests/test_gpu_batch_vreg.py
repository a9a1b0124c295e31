"""Markov-switching vector regressions of a batch on the device (csrc/batch_vreg.hpp) against tests/vreg_ref.py, bit for bit."""
import functools

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import exact_ref as X
import full_ref as FR
import retable_ref as RT
import suffstats_ref as SS
import vreg_ref as VR

pytestmark = pytest.mark.gpu

ESTATE = -3
B_STRIDES = 4 * 2048 + 1                                    # the M-step's 2048 workgroups take a third pair; the re-table's blockIdx.x passes 8192
# 8 x BASE_BAUM_WELCH, the largest distance between the restatement chain (vreg_ref.exact_em) and the float64 recursion over exactly
# test_exact_fit_is_baum_welch's case, measured on the CPU by tools/measure_vreg_tolerance.py (profiles/r45_notes.md)
BASE_BAUM_WELCH = 3.88e-10
TOL_BAUM_WELCH = 8 * BASE_BAUM_WELCH
TRI = np.tril_indices(16)
SHAPES = [(1, 1), (1, 15), (2, 1), (2, 3), (3, 13), (8, 8), (15, 1)]


@functools.lru_cache(maxsize=None)
def _case(k, Q, P, Ts, seed=0):
    rng = np.random.default_rng(10000 * k + 100 * Q + P + 7919 * seed)
    nb = len(Ts)
    W = rng.normal(0.0, 1.0, (nb, k, Q, Q))
    return {"obs": [rng.normal(0.0, 1.5, (T, Q + P)) for T in Ts], "C": rng.normal(0.0, 1.0, (nb, k, Q, P)),
            "V": W @ W.transpose(0, 1, 3, 2) + 0.5 * np.eye(Q), "A": rng.uniform(0.05, 1.0, (nb, k, k))}


def dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def _begin(engine, obs, c, n=16):
    return engine.batch_begin_problems_vreg(obs, n, c["C"], c["V"], c["A"], keep_history=False, keep_masses=True)


def _assert_tables(engine, obs, C, V, A, which=None):
    for b in range(engine.batch_B) if which is None else which:
        rows, thr = engine.batch_step_tables(b)
        got_c, got_L, got_l = engine.batch_copy_vreg(b)
        L = [FR.factor(v) for v in V[b]]
        assert np.array_equal(rows, VR.rows(obs[b], C[b], V[b])) and np.array_equal(thr, RT.thresholds(A[b], A.shape[1])), b
        assert np.array_equal(got_c, C[b]) and np.array_equal(got_L, np.array(L)) and np.array_equal(got_l, [FR.log_norm(f) for f in L]), b


def _records(engine, obs, C, V, A, which=None):
    """Runs the batch exactly and holds masses, evidences and records against the restatement (one reference a distinct case); returns
    the dict and [B, 1304]."""
    k, D, nb = A.shape[1], obs[0].shape[1], len(obs)
    engine.batch_run_exact()
    log_z, st, refs = engine.batch_exact_evidence()[0], engine.batch_vreg_stats(obs), {}
    rec = np.concatenate([st["xi"].reshape(nb, -1), st["occ"], st["occ_y"], st["occ_yy"], st["sy"].reshape(nb, -1), st["syy"][:, :, TRI[0], TRI[1]].reshape(nb, -1)], axis=1)
    for b in range(nb):
        i = b if which is None else which[b]
        if i not in refs:
            P = R.transition_masses(A[b])
            m, z, _ = X.run(VR.rows(obs[b], C[b], V[b])[:, :k].tolist(), P)
            refs[i] = (np.array(m), z, np.concatenate([SS.record(SS.stats([[int(v) for v in row[:k]] for row in m], P, obs[b][:, 0])), FR.sums(m, P, obs[b], D)]))
        assert np.array_equal(engine.batch_masses(b), refs[i][0]) and log_z[b] == refs[i][1] and np.array_equal(rec[b], refs[i][2], equal_nan=True), b
    return st, rec


def _mstep(engine, rec, C, V, A, floor=1e-2):
    d = dev(rec, C, V, A)
    engine.batch_mstep_vreg_device(*d, floor)
    engine.sync()
    return [t.cpu().numpy() for t in d[1:]]


@pytest.mark.parametrize("Q,P", SHAPES)
@pytest.mark.parametrize("k", [2, 8])
def test_device_equals_the_restatement(engine, k, Q, P):
    """Three problems of T = 1, 2 and 37 (two tiles of 32): an odd count, so the M-step's last half-workgroup is idle."""
    c, new = _case(k, Q, P, (1, 2, 37)), _case(k, Q, P, (1, 2, 37), seed=1)
    _begin(engine, c["obs"], c)
    _assert_tables(engine, c["obs"], c["C"], c["V"], c["A"])
    engine.batch_retable_vreg_device(*dev(new["C"], new["V"], new["A"], np.concatenate(c["obs"]).reshape(-1)))
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, c["obs"], new["C"], new["V"], new["A"])
    st, rec = _records(engine, c["obs"], new["C"], new["V"], new["A"])
    got, host = _mstep(engine, rec, new["C"], new["V"], new["A"]), cp.m_step_vreg(st, new["C"], new["V"], new["A"], 1e-2)
    for b in range(3):
        want = VR.m_step(rec[b], new["C"][b], new["V"][b], new["A"][b], 1e-2)
        assert all(np.array_equal(g[b], w) and np.array_equal(h[b], w) for g, h, w in zip(got, host, want)), b
    assert not np.array_equal(got[0][2], new["C"][2])


def test_many_problems_stride_both_kernels(engine):
    Ts = (37, 3, 2, 1, 3)
    c, new = _case(2, 2, 2, Ts, seed=3), _case(2, 2, 2, Ts, seed=4)
    which = np.arange(B_STRIDES) % 5
    obs, old, (C, V, A) = [c["obs"][i] for i in which], {n: c[n][which] for n in "CVA"}, [new[n][which] for n in "CVA"]
    _begin(engine, obs, old, 4)
    engine.batch_retable_vreg_device(*dev(C, V, A, np.concatenate(obs).reshape(-1)))
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, obs, C, V, A, [0, 1, B_STRIDES // 2, B_STRIDES - 1])
    st, rec = _records(engine, obs, C, V, A, which)
    got, host = _mstep(engine, rec, C, V, A), cp.m_step_vreg(st, C, V, A, 1e-2)
    assert all(np.array_equal(g, h) for g, h in zip(got, host)) and not np.array_equal(got[0][-1], C[-1])


def _fit(engine, obs, stats, mstep, *tables):
    """(every problem's rows and words, the evidences, the device M-step's tables) of the begun batch."""
    tabs = [engine.batch_step_tables(b) for b in range(engine.batch_B)]
    engine.batch_run_exact()
    st, ev, nb = stats(obs), engine.batch_exact_evidence()[0], len(obs)
    rec = np.concatenate([st["xi"].reshape(nb, -1), st["occ"], st["occ_y"], st["occ_yy"], st["sy"].reshape(nb, -1), st["syy"][:, :, TRI[0], TRI[1]].reshape(nb, -1)], axis=1)
    d = dev(rec, *tables)
    mstep(*d, 2.0 ** -7)                                    # (a floor whose square is exact: a floored variance's root is the floor again)
    engine.sync()
    return tabs, ev, [t.cpu().numpy() for t in d[1:]]


def test_one_response_is_the_regression_family(engine):
    c = _case(3, 1, 4, (1, 2, 37), seed=2)
    Sg = np.random.default_rng(2).integers(2, 9, (3, 3)) * 0.25            # (sigma sigma is exact: its root is sigma again)
    engine.batch_begin_problems_reg(c["obs"], 8, c["C"][:, :, 0], Sg, c["A"], keep_history=False, keep_masses=True)
    ln = [engine.batch_copy_reg(b)[2] for b in range(3)]
    want = _fit(engine, c["obs"], engine.batch_reg_stats, engine.batch_mstep_reg_device, c["C"][:, :, 0], Sg, c["A"])
    engine.batch_begin_problems_vreg(c["obs"], 8, c["C"], (Sg * Sg)[:, :, None, None], c["A"], keep_history=False, keep_masses=True)
    assert all(np.array_equal(engine.batch_copy_vreg(b)[2], ln[b]) for b in range(3))
    got = _fit(engine, c["obs"], engine.batch_vreg_stats, engine.batch_mstep_vreg_device, c["C"], (Sg * Sg)[:, :, None, None], c["A"])
    assert all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(got[0], want[0])) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2][0][:, :, 0], want[2][0]) and np.array_equal(np.sqrt(got[2][1][:, :, 0, 0]), want[2][1]) and np.array_equal(got[2][2], want[2][2])
    assert not np.array_equal(want[2][0], c["C"][:, :, 0])


def test_one_covariate_of_ones_is_the_full_family(engine):
    c = _case(3, 4, 1, (1, 2, 37), seed=2)
    y, obs = [o[:, :4] for o in c["obs"]], [np.column_stack([o[:, :4], np.ones(len(o))]) for o in c["obs"]]
    engine.batch_begin_problems_full(y, 8, c["C"][:, :, :, 0], c["V"], c["A"], keep_history=False, keep_masses=True)
    want = _fit(engine, y, engine.batch_full_stats, engine.batch_mstep_full_device, c["C"][:, :, :, 0], c["V"], c["A"])
    _begin(engine, obs, c, 8)
    got = _fit(engine, obs, engine.batch_vreg_stats, engine.batch_mstep_vreg_device, c["C"], c["V"], c["A"])
    assert all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(got[0], want[0])) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2][0][:, :, :, 0], want[2][0]) and np.array_equal(got[2][1], want[2][1]) and np.array_equal(got[2][2], want[2][2])
    assert not np.array_equal(want[2][1], c["V"])


def test_kept_states(engine):
    """Problem 0: state 1 without mass.  Problem 1: a NaN in state 0's record.  Problem 2: covariates 0 and 1 are one column, the second
    pivot is exactly 0.0 and every state is kept.  Kept states come back untouched, the others are fitted."""
    c = _case(3, 2, 3, (12, 9, 12), seed=6)
    obs = [o.copy() for o in c["obs"]]
    obs[2][:, 3] = obs[2][:, 2]
    _begin(engine, obs, c, 8)
    _, rec = _records(engine, obs, c["C"], c["V"], c["A"])
    rec[0, 64 + 1], rec[1, 216 + 4] = 0.0, np.nan
    got = _mstep(engine, rec, c["C"], c["V"], c["A"])
    kept = [[False, True, False], [True, False, False], [True, True, True]]
    for b in range(3):
        want = VR.m_step(rec[b], c["C"][b], c["V"][b], c["A"][b], 1e-2)
        assert all(np.array_equal(g[b], w) for g, w in zip(got, want)), b
        assert [bool(np.array_equal(got[0][b, s], c["C"][b, s]) and np.array_equal(got[1][b, s], c["V"][b, s])) for s in range(3)] == kept[b], b


def test_bad_tables_are_refused_for_their_problem_alone_and_other_families_calls_for_the_batch(engine):
    c, new = _case(3, 2, 3, (4, 6, 3)), _case(3, 2, 3, (4, 6, 3), seed=1)
    C, V, flat = new["C"].copy(), new["V"].copy(), np.concatenate(c["obs"]).reshape(-1)
    C[0, 1, 1, 2], V[2, 0, 1, 1] = np.inf, -1.0
    _begin(engine, c["obs"], c, 8)
    engine.batch_retable_vreg_device(*dev(C, V, new["A"], flat))
    assert list(engine.batch_retable_status()) == [4, 0, 64]
    _assert_tables(engine, c["obs"], c["C"], c["V"], c["A"], [0, 2])
    _assert_tables(engine, c["obs"], C, V, new["A"], [1])
    with pytest.raises(cp.capi.CpprobHipError, match="vector-regression") as e:     # (a regression call on this batch: refused, and the batch stays)
        engine.batch_retable_reg_device(*dev(c["C"][:, :, 0], np.ones((3, 3)), c["A"], flat))
    assert e.value.code == ESTATE
    _assert_tables(engine, c["obs"], C, V, new["A"], [1])
    engine.batch_begin_problems_reg([o[:, 1:] for o in c["obs"]], 8, c["C"][:, :, 0], np.ones((3, 3)), c["A"], keep_history=False, keep_masses=True)
    with pytest.raises(cp.capi.CpprobHipError, match="vector-regression") as e:     # (... and this family's call on a regression batch)
        engine.batch_retable_vreg_device(*dev(c["C"], c["V"], c["A"], flat))
    assert e.value.code == ESTATE


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
def test_resident_fit_equals_the_host_loop(engine, exact):
    c = _case(3, 2, 3, (12, 9, 12, 9), seed=5)
    host = cp.hmm_vreg_em(engine, c["obs"], c["C"], c["V"], c["A"], 32, np.arange(4), 3, exact=exact)
    res = cp.hmm_vreg_em(engine, c["obs"], c["C"], c["V"], c["A"], 32, np.arange(4), 3, exact=exact, resident=True)
    assert all(np.array_equal(x, y) for x, y in zip(host, res)) and np.isfinite(host[3]).all() and not np.array_equal(host[0][0], host[0][3])


def switching_case():
    """k = 2 regimes of a bivariate VAR(1) with an intercept (Q = 2, P = 3), two series of 200 steps (the case
    tools/measure_vreg_tolerance.py measures): the regimes overlap, so that no posterior is 0 or 1."""
    rng = np.random.default_rng(45)
    B0 = np.array([[[0.3, 0.5, 0.1], [-0.2, 0.0, 0.4]], [[-0.3, -0.4, 0.2], [0.2, 0.1, -0.3]]])
    obs = []
    for _ in range(2):
        s, Y = np.cumsum(rng.random(201) < 0.1) % 2, np.zeros((201, 2))
        for t in range(1, 201):
            Y[t] = B0[s[t]] @ np.concatenate([[1.0], Y[t - 1]]) + rng.multivariate_normal([0.0, 0.0], [[1.0, 0.3], [0.3, 0.8]])
        obs.append(cp.var_design(Y, 1))
    C = np.array([B0] * 2) + rng.normal(0.0, 0.1, (2, 2, 2, 3))
    return obs, C, np.array([[np.eye(2) * 1.5] * 2] * 2), np.array([[[0.8, 0.2], [0.3, 0.7]]] * 2)


def baum_welch(obs, C0, V0, A0, iterations, floor=1e-3):
    """Float64 Baum-Welch of one Markov-switching vector regression, uniform initial state, weighted least squares by numpy.linalg."""
    C, V, A = np.array(C0, np.float64), np.array(V0, np.float64), np.array(A0, np.float64)
    k, Q = C.shape[0], C.shape[1]
    y, x, hist = obs[:, :Q], obs[:, Q:], [(C.copy(), V.copy(), A.copy())]
    for _ in range(iterations):
        P = A / A.sum(axis=1, keepdims=True)
        res = [y - x @ C[s].T for s in range(k)]
        logb = np.stack([-0.5 * (np.einsum("tq,qr,tr->t", res[s], np.linalg.inv(V[s]), res[s]) + np.log(np.linalg.det(2 * np.pi * V[s]))) for s in range(k)], axis=1)
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
        C = np.array([np.linalg.solve((x * g[:, s:s + 1]).T @ x, (x * g[:, s:s + 1]).T @ y).T for s in range(k)])
        r = [y - x @ C[s].T for s in range(k)]
        V = np.array([(r[s] * g[:, s:s + 1]).T @ r[s] / g[:, s].sum() for s in range(k)])
        V[:, np.arange(Q), np.arange(Q)] = np.maximum(V[:, np.arange(Q), np.arange(Q)], floor * floor)
        hist.append((C.copy(), V.copy(), A.copy()))
    return [np.array(h) for h in zip(*hist)]


def test_exact_fit_is_baum_welch(engine):
    obs, C, V, A = switching_case()
    got = cp.hmm_vreg_em(engine, obs, C, V, A, 8, [1, 2], 5, exact=True, var_floor=1e-3)
    for b in range(2):
        want = baum_welch(obs[b], C[b], V[b], A[b], 5)
        dist = [np.abs(g[1:, b] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: coefficients %.3g, covariances %.3g, transition rows %.3g" % (b, *dist))
        assert max(dist) <= TOL_BAUM_WELCH
