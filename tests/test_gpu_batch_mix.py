"""Gaussian-mixture vector emissions of a batch on the device (csrc/batch_mix.hpp) against tests/mix_ref.py, bit for bit."""
import functools

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import mix_ref as MR
import retable_ref as RT
import suffstats_ref as SS

pytestmark = pytest.mark.gpu

EINVAL = -1
B_TWO_WALKS = 4 * 2048 + 1                                  # kWaves * kSymbolGridMax + 1: the walk's first wavefront takes a second problem
# 8 x 4.01e-10, the largest distance between the restatement chain (exact_ref + backward_ref + mix_ref) and the float64 recursion over
# exactly test_exact_fit_is_baum_welch's case, measured on the CPU by tools/measure_mix_tolerance.py (profiles/r43_notes.md)
TOL_BAUM_WELCH = 8 * 4.01e-10
NAMES = "WMSA"


@functools.lru_cache(maxsize=None)
def _case(k, M, D, Ts, seed=0):
    rng = np.random.default_rng(10000 * k + 100 * M + 10 * D + seed)
    nb = len(Ts)
    return {"obs": [rng.normal(0.0, 2.0, (T, D)) for T in Ts], "W": rng.uniform(0.1, 1.0, (nb, k, M)), "M": rng.normal(0.0, 2.0, (nb, k, M, D)),
            "S": rng.uniform(0.5, 2.0, (nb, k, M, D)), "A": rng.uniform(0.05, 1.0, (nb, k, k))}


def dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def code(call, match=None):
    with pytest.raises(cp.capi.CpprobHipError, match=match) as e:
        call()
    return e.value.code


def _assert_tables(engine, obs, W, Mu, Sg, A, which=None):
    for b in range(engine.batch_B) if which is None else which:
        rows, thr = engine.batch_step_tables(b)
        lw, mu, sg, ln = engine.batch_copy_mix(b)
        assert np.array_equal(rows, MR.rows(obs[b], W[b], Mu[b], Sg[b])) and np.array_equal(thr, RT.thresholds(A[b], A.shape[1])), b
        assert np.array_equal(lw, MR.log_weights(W[b])) and np.array_equal(mu, Mu[b]) and np.array_equal(sg, Sg[b]), b
        assert np.array_equal(ln, [MR.DG.log_norms(s) for s in Sg[b]]), b


def _record(st):
    nb = len(st["occ"])
    blocks = np.concatenate([st["occ_c"][..., None], st["sy"], st["syy"]], axis=-1)
    return np.concatenate([st["xi"].reshape(nb, -1), st["occ"], st["occ_y"], st["occ_yy"], blocks.reshape(nb, -1)], axis=1)


def _assert_records(engine, obs, W, Mu, Sg, A, exact, which=None, tail=()):
    """Runs the batch and holds its records against the restatement (one reference a distinct case; for the problems of `tail` the
    mixture's 2112 doubles alone); returns the dict and [B, 2200]."""
    k = Mu.shape[1]
    if exact:
        engine.batch_run_exact()
    else:
        engine.batch_run(np.arange(engine.batch_B, dtype=np.uint64) + np.uint64(7))
    st, refs = engine.batch_mix_stats(obs), {}
    rec = _record(st)
    for b in range(engine.batch_B):
        i = b if which is None else which[b]
        if i not in refs:
            m, P = engine.batch_masses(b), R.transition_masses(A[b])
            base = np.zeros(88) if b in tail else SS.record(SS.stats([[int(v) for v in row[:k]] for row in m], P, obs[b][:, 0]))
            refs[i] = np.concatenate([base, MR.sums(m, P, obs[b], W[b], Mu[b], Sg[b])])
        assert np.array_equal(rec[b, 88 if b in tail else 0:], refs[i][88 if b in tail else 0:], equal_nan=True), b
    return st, rec


def _assert_m_step(engine, st, rec, d, new, which, floor=1e-2):
    engine.batch_mstep_mix_device(dev(rec)[0], d[0], d[1], d[2], d[3], floor)
    engine.sync()
    host = cp.m_step_mix(st, *new, floor)
    assert all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(d, host))
    for b in which:
        assert all(np.array_equal(h[b], w) for h, w in zip(host, MR.m_step(rec[b], *[t[b] for t in new], floor))), b


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
@pytest.mark.parametrize("D", [1, 5, 16])
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("k", [2, 8])
def test_device_equals_the_restatement(engine, k, M, D, exact):
    c, new = _case(k, M, D, (1, 2, 37)), _case(k, M, D, (1, 2, 37), seed=1)
    old, tabs = [c[n] for n in NAMES], [new[n] for n in NAMES]
    engine.batch_begin_problems_mix(c["obs"], 16, *old, keep_history=False, keep_masses=True)
    _assert_tables(engine, c["obs"], *old)
    d = dev(*tabs, np.concatenate(c["obs"]).reshape(-1))
    engine.batch_retable_mix_device(*d)
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, c["obs"], *tabs)
    st, rec = _assert_records(engine, c["obs"], *tabs, exact)
    _assert_m_step(engine, st, rec, d[:4], tabs, range(3))


def test_many_problems_two_tiles_through_one_buffer(engine):
    """4 * 2048 + 1 problems, the longest of T = 37: retable_grid_y gives 1, so a long problem's re-table workgroup walks two tiles through
    one LDS buffer; the walk's first wavefront and the moments' workgroups take further problems."""
    Ts = (37, 3, 2, 1, 3)
    c, new = _case(2, 2, 2, Ts, seed=3), _case(2, 2, 2, Ts, seed=4)
    which = np.arange(B_TWO_WALKS) % 5
    obs, old, tabs = [c["obs"][i] for i in which], [c[n][which] for n in NAMES], [new[n][which] for n in NAMES]
    assert RT.grid_y(37, B_TWO_WALKS) == 1
    engine.batch_begin_problems_mix(obs, 4, *old, keep_history=False, keep_masses=True)
    d = dev(*tabs, np.concatenate(obs).reshape(-1))
    engine.batch_retable_mix_device(*d)
    assert not engine.batch_retable_status().any()
    _assert_tables(engine, obs, *tabs, [0, 1, B_TWO_WALKS // 2, B_TWO_WALKS - 1])
    st, rec = _assert_records(engine, obs, *tabs, True, which)
    _assert_m_step(engine, st, rec, d[:4], tabs, range(5))


@pytest.mark.parametrize("D", [1, 5])
def test_one_component_is_the_diagonal_family(engine, D):
    c = _case(3, 1, D, (1, 2, 37), seed=2)
    Mu, Sg = c["M"][:, :, 0], c["S"][:, :, 0]
    engine.batch_begin_problems_diag(c["obs"], 8, Mu, Sg, c["A"], keep_history=False, keep_masses=True)
    want = [engine.batch_step_tables(b) for b in range(3)]
    engine.batch_run_exact()
    base = engine.batch_diag_stats(c["obs"])
    dm = cp.m_step_diag(base, Mu, Sg, c["A"], 1e-2)
    engine.batch_begin_problems_mix(c["obs"], 8, c["W"], c["M"], c["S"], c["A"], keep_history=False, keep_masses=True)
    for b in range(3):
        got = engine.batch_step_tables(b)
        assert np.array_equal(got[0], want[b][0]) and np.array_equal(got[1], want[b][1]), b
    engine.batch_run_exact()
    st = engine.batch_mix_stats(c["obs"])
    assert all(np.array_equal(st[n], base[n]) for n in ("xi", "occ", "occ_y", "occ_yy")) and np.array_equal(st["occ_c"][:, :, 0], base["occ"])
    assert np.array_equal(st["sy"][:, :, 0, :D], base["sy"][:, :, :D]) and np.array_equal(st["syy"][:, :, 0, :D], base["syy"][:, :, :D])
    W, M1, S1, A = cp.m_step_mix(st, c["W"], c["M"], c["S"], c["A"], 1e-2)
    assert np.array_equal(M1[:, :, 0], dm[0]) and np.array_equal(S1[:, :, 0], dm[1]) and np.array_equal(A, dm[2]) and (W == 1.0).all()


def test_zero_weight_far_component_and_infinite_observe(engine):
    """A zero weight is accepted and its component receives exactly 0.0; so does a component more than 1000 nats below its state's best;
    an infinite observe gives a -inf row, and the record is the restatement's, which skips that step."""
    c = _case(2, 3, 2, (6, 37, 5), seed=6)
    W, Mu, obs = c["W"].copy(), c["M"].copy(), [o.copy() for o in c["obs"]]
    W[0, 1, 2], Mu[1, 0, 1], obs[2][3, 1] = 0.0, 500.0, -np.inf
    engine.batch_begin_problems_mix(obs, 16, W, Mu, c["S"], c["A"], keep_history=False, keep_masses=True)
    _assert_tables(engine, obs, W, Mu, c["S"], c["A"])
    assert np.isneginf(engine.batch_step_tables(2)[0][3]).all() and engine.batch_copy_mix(0)[0][1, 2] == -np.inf
    st, _ = _assert_records(engine, obs, W, Mu, c["S"], c["A"], True, tail=[2])       # (problem 2's run is dead at the infinite observe)
    assert (st["occ_c"][0, 1, 2] == 0.0) and (st["sy"][0, 1, 2] == 0.0).all() and (st["occ_c"][0, 1, :2] > 0.0).all()
    assert (st["occ_c"][1, 0, 1] == 0.0) and (st["syy"][1, 0, 1] == 0.0).all() and (st["occ_c"][1, 0, 0] > 0.0)
    new = cp.m_step_mix(st, W, Mu, c["S"], c["A"])
    assert new[0][0, 1, 2] == 0.0 and new[1][0, 1, 2, 0] == Mu[0, 1, 2, 0] and MR.check(new[0][0], new[1][0], new[2][0], new[3][0]) == 0


@pytest.mark.parametrize("bad,bit", [("weight", 128), ("total", 128), ("share", 128), ("mean", 4), ("sigma", 8)])
def test_a_bad_table_raises_its_bit_and_the_problem_keeps_its_rows(engine, bad, bit):
    c, new = _case(3, 3, 5, (4, 37, 3)), _case(3, 3, 5, (4, 37, 3), seed=1)
    W, Mu, Sg, A = [new[n].copy() for n in NAMES]
    if bad == "weight":
        W[1, 2, 1] = -0.5
    elif bad == "total":
        W[1, 0] = 0.0
    elif bad == "share":
        W[1, 1, 0] = 1e-320
    elif bad == "mean":
        Mu[1, 2, 2, 4] = np.inf
    else:
        Sg[1, 0, 1, 3] = 0.0
    assert MR.check(W[1], Mu[1], Sg[1], A[1]) == bit
    for M, D in ((9, 5), (2, 17)):
        assert code(lambda: engine.batch_begin_problems_mix(c["obs"], 8, np.ones((3, 3, M)), np.ones((3, 3, M, D)), np.ones((3, 3, M, D)), c["A"])) == EINVAL
    assert code(lambda: engine.batch_begin_problems_mix(c["obs"], 8, W, Mu, Sg, A), "problem 1") == EINVAL
    old = [c[n] for n in NAMES]
    engine.batch_begin_problems_mix(c["obs"], 8, *old, keep_history=False, keep_masses=True)
    engine.batch_retable_mix_device(*dev(W, Mu, Sg, A, np.concatenate(c["obs"]).reshape(-1)))
    assert list(engine.batch_retable_status()) == [0, bit, 0]
    _assert_tables(engine, c["obs"], *old, [1])
    _assert_tables(engine, c["obs"], W, Mu, Sg, A, [0, 2])
    assert code(lambda: engine.batch_retable_mix(W, Mu, Sg, A, c["obs"]), "problem 1") == EINVAL


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "particles"])
def test_resident_fit_equals_the_host_loop(engine, exact):
    c = _case(3, 3, 5, (12, 9, 12, 9), seed=5)
    tabs = [c[n] for n in NAMES]
    host = cp.hmm_mix_em(engine, c["obs"], *tabs, 32, np.arange(4), 3, exact=exact)
    res = cp.hmm_mix_em(engine, c["obs"], *tabs, 32, np.arange(4), 3, exact=exact, resident=True)
    assert all(np.array_equal(x, y) for x, y in zip(host, res)) and np.isfinite(host[4]).all() and not np.array_equal(host[1][0], host[1][3])


def two_mode_case():
    """k = 2, M = 2, D = 2, two sequences of 200 steps: the states sit at x = -1 and x = 1 and overlap (noise 0.7), each with two components at y = -2 and y = 2 (the case tools/measure_mix_tolerance.py measures; the float64 reference neither swaps nor kills a component in five
    iterations, which that tool checks)."""
    rng = np.random.default_rng(11)
    centres = np.array([[[-1.0, -2.0], [-1.0, 2.0]], [[1.0, -2.0], [1.0, 2.0]]])
    obs = []
    for _ in range(2):
        s = np.cumsum(rng.random(200) < 0.1) % 2
        obs.append(centres[s, rng.integers(0, 2, 200)] + rng.normal(0.0, 0.7, (200, 2)))
    Mu = np.broadcast_to(centres + np.array([0.4, -0.3]), (2, 2, 2, 2)).copy()
    return obs, np.full((2, 2, 2), 0.5), Mu, np.full((2, 2, 2, 2), 1.0), np.broadcast_to(np.array([[0.8, 0.2], [0.3, 0.7]]), (2, 2, 2)).copy()


def baum_welch(obs, W0, M0, S0, A0, iterations, floor=1e-6):
    """Float64 Baum-Welch of one HMM with Gaussian-mixture emissions, uniform initial state, hmm_mix_em's M-step."""
    W, Mu, Sg, A, y = [np.array(a, np.float64) for a in (W0, M0, S0, A0, obs)]
    k, hist = Mu.shape[0], [(W.copy(), Mu.copy(), Sg.copy(), A.copy())]
    for _ in range(iterations):
        P = A / A.sum(axis=1, keepdims=True)
        z = (y[:, None, None, :] - Mu[None]) / Sg[None]
        logc = np.log(W / W.sum(axis=1, keepdims=True))[None] - 0.5 * ((z * z).sum(axis=3) + np.log(2 * np.pi * Sg * Sg).sum(axis=2)[None])
        logb = logc.max(axis=2) + np.log(np.exp(logc - logc.max(axis=2, keepdims=True)).sum(axis=2))
        resp = np.exp(logc - logb[:, :, None])
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
        v = gamma[:, :, None] * resp
        occ_c = v.sum(axis=0)
        A = np.where(xi.sum(axis=1, keepdims=True) > 0, xi / xi.sum(axis=1, keepdims=True), A)
        W = occ_c / occ_c.sum(axis=1, keepdims=True)
        Mu = np.einsum("tsc,td->scd", v, y) / occ_c[:, :, None]
        Sg = np.sqrt(np.maximum(np.einsum("tsc,td->scd", v, y * y) / occ_c[:, :, None] - Mu * Mu, floor * floor))
        hist.append((W.copy(), Mu.copy(), Sg.copy(), A.copy()))
    return [np.array(h) for h in zip(*hist)]


def test_exact_fit_is_baum_welch(engine):
    obs, W, Mu, Sg, A = two_mode_case()
    got = cp.hmm_mix_em(engine, obs, W, Mu, Sg, A, 8, [1, 2], 5, exact=True)
    for b in range(2):
        want = baum_welch(obs[b], W[b], Mu[b], Sg[b], A[b], 5)
        dist = [np.abs(g[1:, b] - w[1:]).max() for g, w in zip(got, want)]
        print("problem %d: weights %.3g, means %.3g, sigmas %.3g, transition rows %.3g" % (b, *dist))
        assert max(dist) <= TOL_BAUM_WELCH
