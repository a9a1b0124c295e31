"""Per-state emission scales on the host (csrc/batch_scale.hpp, tests/scale_ref.py, cpprob_amd.em.m_step with sigmas): the table
logarithm against an exact one, its exported form against the restatement, the scaled rows against the unit rows and against the
oracle's density, the M-step's edge cases, and EM on exact statistics.  No GPU.

table_log's error, measured here over ARGS (16043 arguments: the powers of two 2^-1022 .. 2^1023 in steps of 7 with two neighbours on
either side, 64 mantissas at nine exponents, seeded random arguments over e^+-700, e^+-1 and 1 +- 1e-3, the fold point and 2 pi)
against decimal's logarithm at 50 digits: worst 2.74 ulp of the exact value (at 1.00096: the result is small and carries the
division's and the series' roundings in full), worst absolute error 3.93e-16 over the arguments with |log| <= 5.  The bound
asserted is twice the measured ulp error, rounded up: 6."""
import ctypes as C
import math
import random
from decimal import Decimal, getcontext

import numpy as np
import pytest

import retable_ref as R
import scale_ref as S
from oracle import exact

ULP_BOUND = 6


def _args():
    rng = random.Random(20261020)
    xs = []
    for e in range(-1022, 1024, 7):
        for d in (-2, -1, 0, 1, 2):
            x = math.ldexp(1.0, e)
            for _ in range(abs(d)):
                x = math.nextafter(x, math.inf if d > 0 else 0.0)
            if S.MIN_NORMAL <= x < math.inf:
                xs.append(x)
    xs += [math.ldexp(1.0 + i / 64.0, e) for e in (-1022, -700, -30, -1, 0, 1, 30, 700, 1023) for i in range(64)]
    xs += [math.exp(rng.uniform(-700.0, 700.0)) for _ in range(6000)]
    xs += [math.exp(rng.uniform(-1.0, 1.0)) for _ in range(6000)]
    xs += [1.0 + rng.uniform(-1e-3, 1e-3) for _ in range(2000)]
    xs += [S.SQRT2, math.nextafter(S.SQRT2, 0.0), math.nextafter(S.SQRT2, 2.0), 2 * math.pi]
    return xs


ARGS = _args()


@pytest.fixture(scope="module")
def measured():
    """(worst error in ulps of the exact value, worst absolute error where |log| <= 5) of scale_ref.table_log over ARGS."""
    getcontext().prec = 50
    worst, worst_abs = 0.0, 0.0
    for x in ARGS:
        ex = Decimal(x).ln()
        g = S.table_log(x)
        fe = float(ex)
        if fe == 0.0:
            assert g == 0.0
            continue
        err = abs(Decimal(g) - ex)
        worst = max(worst, float(err / Decimal(math.ulp(fe))))
        if abs(fe) <= 5.0:
            worst_abs = max(worst_abs, float(err))
    print("table_log: worst %.3f ulp, worst absolute %.3e (|log| <= 5) over %d arguments" % (worst, worst_abs, len(ARGS)))
    return worst, worst_abs


def test_table_log_against_exact(measured):
    assert measured[0] <= ULP_BOUND


def test_table_log_two_pi_bits():
    assert S.table_log(2 * 3.14159265358979323846 * 1.0 * 1.0).hex() == math.log(2 * math.pi).hex()
    assert S.log_norm(1.0).hex() == math.log(2 * 3.14159265358979323846 * 1.0 * 1.0).hex()


def test_exported_table_log_is_the_restatement():
    import cpprob_amd as cp
    L = cp.load_library()
    got = np.array([L.cpprob_hip_table_log(C.c_double(x)) for x in ARGS])
    want = np.array([S.table_log(x) for x in ARGS])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


Y = np.concatenate([np.random.default_rng(5).normal(0.0, 3.0, 200), [0.0, -0.0, 1e300, -1e300, np.inf, -np.inf, 5e-324]])


@pytest.mark.parametrize("k", [2, 5, 8])
def test_unit_scaled_rows_are_the_unit_rows(k):
    means = np.random.default_rng(k).normal(0.0, 2.0, k)
    got = S.rows(Y, means, np.ones(k), k)
    want = R.rows(Y, means, k, math.log(2 * math.pi))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_mixed_scaled_rows_against_the_oracle(measured):
    """Both sides form ((y - mean) / sigma)^2 with the same operations; their logarithms of 2 pi sigma^2 (|log| <= 5 for the sigmas
    here, 0.05 .. 3) differ by at most table_log's absolute error, the sum rounds once on either side, and the product by -0.5 is exact:
    half the logarithm's error plus one ulp of the row."""
    k = 8
    sigmas = np.array([0.05, 0.3, 0.5, 1.0, 1.7, 2.0, 2.5, 3.0])
    means = np.linspace(-3.0, 3.0, k)
    y = Y[np.isfinite(Y) & (np.abs(Y) < 1e3)]
    got = S.rows(y, means, sigmas, k)
    for s in range(k):
        want = exact.normal_logpdf(y, means[s], sigmas[s])
        bound = 0.5 * measured[1] + np.spacing(np.abs(want))
        assert np.all(np.abs(got[:, s] - want) <= bound), s
    assert np.all(np.isneginf(S.rows([np.inf, -np.inf], means, sigmas, k)))
    assert np.all(np.isneginf(S.rows(y, means[:3], sigmas[:3], 3)[:, 3:]))


def _record(k, xi, occ, occ_y, occ_yy):
    rec = np.zeros(R.RECORD)
    rec[:64].reshape(8, 8)[:k, :k] = xi
    rec[64:64 + k], rec[72:72 + k], rec[80:80 + k] = occ, occ_y, occ_yy
    return rec


def mstep_cases():
    """(name, record, means, sigmas, trans, floor) of the M-step's edge cases, k = 2: state 0 is the case, state 1 an ordinary state."""
    xi = np.array([[3.0, 1.0], [2.0, 2.0]])
    tr = np.array([[0.5, 0.5], [0.5, 0.5]])
    ord_occ, ord_y, ord_yy = 4.0, 2.0, 5.0                  # mean 0.5, v = 1.25 - 0.25 = 1
    out = []
    for name, occ, occ_y, occ_yy, floor in (
            ("no mass", 0.0, 0.0, 0.0, 1e-3),
            ("cancellation", 10.0, 10.0 * 1e8, 10.0 * (1e16 + 1e-6), 1e-3),
            ("nan", 2.0, 1.0, math.nan, 1e-3),
            ("exactly the floor squared", 4.0, 0.0, 0.25, 0.25),
            ("overflow", 1e-10, 0.0, 1e300, 1e-3),
            ("subnormal norm", 4.0, 0.0, 0.0, 1e-160)):
        out.append((name, _record(2, xi, [occ, ord_occ], [occ_y, ord_y], [occ_yy, ord_yy]), np.array([7.0, -1.0]), np.array([3.0, 4.0]), tr, floor))
    return out


def test_mstep_cases():
    import cpprob_amd.em as em
    import cpprob_amd.capi as capi
    for name, rec, means, sigmas, trans, floor in mstep_cases():
        ln0 = np.array([S.log_norm(s) for s in sigmas])
        m, sg, ln, tr = S.m_step(rec, means, sigmas, ln0, trans, 2, floor)
        bits = S.check(m, sg, tr, 2)
        assert sg[1] == 1.0 and m[1] == 0.5 and ln[1].hex() == math.log(2 * math.pi).hex(), name
        if name == "no mass":
            assert (m[0], sg[0], ln[0]) == (7.0, 3.0, ln0[0]) and bits == 0
        elif name in ("cancellation", "nan"):
            assert sg[0] == floor and bits == 0
        elif name == "exactly the floor squared":
            assert sg[0] == 0.25 == math.sqrt(0.0625) and bits == 0
        elif name == "overflow":
            assert sg[0] == math.inf and math.isnan(ln[0]) and bits == S.BAD_SCALE
        else:
            assert sg[0] == 1e-160 and 0.0 < S.norm_arg(sg[0]) < S.MIN_NORMAL and math.isnan(ln[0]) and bits == S.BAD_SCALE
        # the package's numpy M-step is the same statements
        m2, t2, s2 = em.m_step(capi.split_stats(rec[None, :]), means[None, :], trans[None, :, :], sigmas[None, :], floor)
        assert np.array_equal(m2[0], m) and np.array_equal(t2[0], tr) and np.array_equal(s2[0], sg), name
        # ... and without sigmas it returns what it returned
        m3, t3 = em.m_step(capi.split_stats(rec[None, :]), means[None, :], trans[None, :, :])
        assert np.array_equal(m3, m2) and np.array_equal(t3, t2)


def test_check_bits():
    tr = np.array([[0.5, 0.5], [0.5, 0.5]])
    for bad in (0.0, -1.0, math.inf, math.nan, 1e-170, 1e160):
        assert S.check([0.0, 1.0], [1.0, bad], tr, 2) == S.BAD_SCALE, bad
    assert S.check([0.0, 1.0], [1e-150, 1e150], tr, 2) == 0
    assert S.check([math.inf, 1.0], [1.0, 0.0], [[0.0, 0.0], [1.0, -1.0]], 2) == 15


# ---- EM on exact statistics: suffstats_ref.exact_stats with the emission's sigma an argument -------------------------------------------
def exact_stats(obs, means, trans, sigmas):
    obs = np.asarray(obs, np.float64)
    A = np.asarray(trans, np.float64)
    A = A / A.sum(axis=1, keepdims=True)
    T, k = len(obs), len(means)
    lik = np.exp(exact.normal_logpdf(obs[:, None], np.asarray(means)[None, :], np.asarray(sigmas)[None, :]))
    alpha, c = np.zeros((T, k)), np.zeros(T)
    a = np.full(k, 1.0 / k) * lik[0]
    c[0] = a.sum()
    alpha[0] = a / c[0]
    for t in range(1, T):
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
    return xi, gamma.sum(axis=0), gamma.T @ obs, gamma.T @ (obs * obs), float(np.log(c).sum())


def _stats_dict(k, xi, occ, occ_y, occ_yy):
    st = {"xi": np.zeros((1, 8, 8)), "occ": np.zeros((1, 8)), "occ_y": np.zeros((1, 8)), "occ_yy": np.zeros((1, 8))}
    st["xi"][0, :k, :k], st["occ"][0, :k], st["occ_y"][0, :k], st["occ_yy"][0, :k] = xi, occ, occ_y, occ_yy
    return st


def _simulate(seed, means, sigmas, trans, T):
    rng = np.random.default_rng(seed)
    k = len(means)
    x = rng.integers(k)
    y = np.zeros(T)
    for t in range(T):
        x = rng.choice(k, p=trans[x])
        y[t] = rng.normal(means[x], sigmas[x])
    return y


def _em(y, means, trans, sigmas, iterations):
    """em.m_step on exact statistics: the log-likelihood of every iteration's tables and the last tables."""
    import cpprob_amd.em as em
    k = len(means)
    m, t, s = np.array(means)[None, :], np.array(trans)[None, :, :], np.array(sigmas)[None, :]
    lls = []
    for _ in range(iterations):
        xi, occ, occ_y, occ_yy, ll = exact_stats(y, m[0], t[0], s[0])
        lls.append(ll)
        m, t, s = em.m_step(_stats_dict(k, xi, occ, occ_y, occ_yy), m, t, s)
    return lls, m[0], t[0], s[0]


@pytest.mark.parametrize("seed,k", [(1, 2), (2, 3), (3, 3)])
def test_scaled_em_never_decreases_the_likelihood(seed, k):
    """EM's guarantee; the allowance is the rounding of a sum of T = 300 logarithms, 1e-10 of its value."""
    means = np.linspace(-2.0, 2.0, k)
    sigmas = np.array([0.4, 1.5, 0.8])[:k]
    trans = np.full((k, k), 0.2 / (k - 1)) + np.eye(k) * (0.8 - 0.2 / (k - 1))
    y = _simulate(seed, means, sigmas, trans, 300)
    lls, _, _, _ = _em(y, means + 0.7, np.full((k, k), 1.0 / k), np.ones(k), 11)
    assert len(lls) == 11
    for a, b in zip(lls, lls[1:]):
        assert b >= a - 1e-10 * abs(a), lls


def test_scaled_em_recovers_the_scales():
    """4000 steps of a well-separated two-state sequence with sigmas (0.5, 2.0): the package's M-step, iterated on exact statistics
    from sigma = 1, against the fixed point of an EM restated here (numpy's own formulas, run from the truth until it stands still),
    within 3 standard errors sigma / sqrt(2 occ) of that fixed point."""
    means, sigmas, trans = np.array([-5.0, 5.0]), np.array([0.5, 2.0]), np.array([[0.9, 0.1], [0.1, 0.9]])
    y = _simulate(11, means, sigmas, trans, 4000)
    m, t, s = means.copy(), trans.copy(), sigmas.copy()
    for _ in range(200):
        xi, occ, occ_y, occ_yy, _ = exact_stats(y, m, t, s)
        m2, t2, s2 = occ_y / occ, xi / xi.sum(axis=1, keepdims=True), np.sqrt(occ_yy / occ - (occ_y / occ) ** 2)
        done = max(np.abs(m2 - m).max(), np.abs(s2 - s).max()) < 1e-13
        m, t, s = m2, t2, s2
        if done:
            break
    assert done
    _, _, _, got = _em(y, np.array([-3.0, 3.0]), np.full((2, 2), 0.5), np.ones(2), 60)
    se = s / np.sqrt(2.0 * occ)
    print("fixed point", s, "fitted", got, "standard errors", se)
    assert np.all(np.abs(got - s) <= 3.0 * se)
