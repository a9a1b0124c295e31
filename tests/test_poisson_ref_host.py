"""Poisson emissions on the host (csrc/batch_poisson.hpp, tests/poisson_ref.py, cpprob_amd.em.m_step with emission="poisson"): the
log-factorials against lgamma, the count a double is, the M-step's branches, the rows against the textbook expression, and the
(observe, rate) pairs at which a fused multiply-add would change a row.  No GPU.

The log-factorials' bound: lf[c] is a sum of c terms table_log(i), each within 3 ulp of the exact logarithm (table_log's measured worst
is 2.74, tests/test_scale_ref_host.py), added by c additions of half an ulp of the running sum each; terms and partial sums are at most
the result, so the relative error stays below 3.5 c 2^-52.  Measured here against math.lgamma(c + 1) over all 4096 counts: the largest
relative error is 2.507e-15 (11.29 units of 2^-52, at c = 3451), the largest share of the bound 0.309 (at c = 2)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import poisson_ref as P
import retable_ref as R
import scale_ref as S


def test_log_factorials_against_lgamma():
    assert len(P.LF) == P.MAX_COUNT + 1 and P.LF[0] == 0.0 and P.LF[1] == 0.0
    worst, worst_at, ratio, ratio_at = 0.0, 0, 0.0, 0
    for c in range(2, P.MAX_COUNT + 1):
        want = math.lgamma(c + 1.0)
        rel = abs(P.LF[c] - want) / want
        bound = 3.5 * c * 2.0 ** -52
        if rel > worst:
            worst, worst_at = rel, c
        if rel / bound > ratio:
            ratio, ratio_at = rel / bound, c
        assert rel < bound, (c, rel, bound)
    print("log-factorials: largest relative error %.3e (%.2f x 2^-52) at c = %d; largest share of the bound %.3f at c = %d"
          % (worst, worst * 2.0 ** 52, worst_at, ratio, ratio_at))


def test_exported_table_log_gives_the_same_table():
    import ctypes as C
    import cpprob_amd as cp
    L = cp.load_library()
    lf = [0.0, 0.0]
    for i in range(2, P.MAX_COUNT + 1):
        lf.append(lf[-1] + L.cpprob_hip_table_log(C.c_double(float(i))))
    assert np.array_equal(np.array(lf).view(np.uint64), P.LF_ARRAY.view(np.uint64))


INVALID = [math.nan, math.inf, -math.inf, -1.0, 0.5, 4096.0]


def test_count():
    for y in INVALID:
        assert P.count(y) == -1, y
    assert P.count(4095.0) == 4095 and P.count(0.0) == 0 and P.count(-0.0) == 0 and P.count(1.0) == 1
    assert P.count(math.nextafter(4095.0, 0.0)) == -1 and P.count(5e-324) == -1 and P.count(1e300) == -1
    for y in INVALID:
        assert P.entry(y, 2.0, S.table_log(2.0)) == -math.inf


def test_bad_rate_and_check_bits():
    tr = np.array([[0.5, 0.5], [0.5, 0.5]])
    for r in (0.0, -1.0, math.inf, math.nan, 1e-310, 5e-324):
        assert P.bad(r) and P.check([1.0, r], tr, 2) == P.BAD_RATE, r
    for r in (S.MIN_NORMAL, 1e-300, 1.0, 1e308):
        assert not P.bad(r) and P.check([r, 1.0], tr, 2) == 0
    # bit 4 is not used: the transition rows' bits and bit 16
    assert P.check([math.inf, 1.0], [[0.0, 0.0], [1.0, -1.0]], 2) == R.BAD_WEIGHT | R.NO_MASS | P.BAD_RATE


def _record(k, xi, occ, occ_y):
    rec = np.zeros(R.RECORD)
    rec[:64].reshape(8, 8)[:k, :k] = xi
    rec[64:64 + k], rec[72:72 + k] = occ, occ_y
    rec[80:80 + k] = 1.0                                   # (occ_yy: not read)
    return rec


def mstep_cases():
    """(name, record, rates, trans, floor) of the M-step's edge cases, k = 2: state 0 is the case, state 1 an ordinary state."""
    xi = np.array([[3.0, 1.0], [2.0, 2.0]])
    tr = np.array([[0.5, 0.5], [0.5, 0.5]])
    out = []
    for name, occ, occ_y, floor in (
            ("above the floor", 4.0, 10.0, 1e-6),
            ("exactly the floor", 4.0, 1.0, 0.25),
            ("below the floor", 4.0, 1e-9, 1e-6),
            ("no counts", 4.0, 0.0, 1e-6),
            ("no mass", 0.0, 0.0, 1e-6),
            ("nan", 2.0, math.nan, 1e-6),
            ("overflow", 1e-10, 1e300, 1e-6),
            ("subnormal", 4.0, 0.0, 1e-310)):
        out.append((name, _record(2, xi, [occ, 4.0], [occ_y, 2.0]), np.array([7.0, 3.0]), tr, floor))
    return out


def test_mstep_cases():
    import cpprob_amd.em as em
    import cpprob_amd.capi as capi
    for name, rec, rates, trans, floor in mstep_cases():
        lr0 = np.array([S.table_log(r) for r in rates])
        rt, lr, tr = P.m_step(rec, rates, lr0, trans, 2, floor)
        bits = P.check(rt, tr, 2)
        assert rt[1] == 0.5 and lr[1] == S.table_log(0.5) and np.array_equal(tr, [[0.75, 0.25], [0.5, 0.5]]), name
        if name == "above the floor":
            assert rt[0] == 2.5 and lr[0] == S.table_log(2.5) and bits == 0
        elif name == "exactly the floor":
            assert rt[0] == 0.25 and lr[0] == S.table_log(0.25) and bits == 0
        elif name in ("below the floor", "no counts", "nan"):
            assert rt[0] == floor and lr[0] == S.table_log(floor) and bits == 0, name
        elif name == "no mass":
            assert rt[0] == 7.0 and lr[0] == lr0[0] and bits == 0
        elif name == "overflow":
            assert rt[0] == math.inf and math.isnan(lr[0]) and bits == P.BAD_RATE
        else:
            assert rt[0] == 1e-310 and 0.0 < rt[0] < S.MIN_NORMAL and math.isnan(lr[0]) and bits == P.BAD_RATE
        # the package's numpy M-step is the same statements
        with np.errstate(all="ignore"):
            m2, t2 = em.m_step(capi.split_stats(rec[None, :]), rates[None, :], trans[None, :, :], emission="poisson", rate_floor=floor)
        assert np.array_equal(m2[0], rt) and np.array_equal(t2[0], tr), name
    with pytest.raises(ValueError):
        em.m_step(capi.split_stats(rec[None, :]), rates[None, :], trans[None, :, :], sigmas=np.ones((1, 2)), emission="poisson")
    with pytest.raises(ValueError):
        em.m_step(capi.split_stats(rec[None, :]), rates[None, :], trans[None, :, :], emission="poisson", rate_floor=0.0)


def test_rows_against_the_textbook_expression():
    """y log(rate) - rate - lgamma(y + 1) with the library's logarithm and lgamma, to a relative 1e-11 of the largest of the three terms
    (the row itself may cancel to nothing)."""
    rates = np.array([1e-3, 0.5, 1.0, 4.0, 12.0, 100.0, 1500.0, 4000.0])
    y = np.concatenate([np.arange(0, 40), [63, 64, 100, 255, 1000, 2047, 2048, 4094, 4095]]).astype(np.float64)
    got = P.rows(y, rates, 8)
    for s, lam in enumerate(rates):
        for i, v in enumerate(y):
            terms = (v * math.log(lam), lam, math.lgamma(v + 1.0))
            want = terms[0] - terms[1] - terms[2]
            assert abs(got[i, s] - want) <= 1e-11 * max(abs(t) for t in terms), (v, lam)
    assert np.all(np.isneginf(P.rows(INVALID, rates, 8)))
    assert np.all(np.isneginf(P.rows(y, rates[:3], 3)[:, 3:]))


def _fused_entry(y, rate, log_rate):
    """poisson_entry with y log_rate - rate in one rounding, in exact rational arithmetic."""
    r = float(Fraction(y) * Fraction(log_rate) - Fraction(rate))
    return r - P.LF[P.count(y)]


def fused_pairs(n=24, seed=20261021):
    """(y, rate) pairs at which fusing y * log_rate - rate into one rounding changes the row: a seeded search over counts 1 .. 300 and
    rates exp(u), u uniform over +-4, with the fused form evaluated exactly (Fraction) and rounded once."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        y, rate = float(rng.integers(1, 301)), float(np.exp(rng.uniform(-4.0, 4.0)))
        lr = S.table_log(rate)
        if _fused_entry(y, rate, lr) != P.entry(y, rate, lr):
            out.append((y, rate))
    return out


def test_fused_pairs_differ():
    pairs = fused_pairs()
    assert len(pairs) == 24
    for y, rate in pairs:
        lr = S.table_log(rate)
        a, b = P.entry(y, rate, lr), _fused_entry(y, rate, lr)
        assert a != b and math.isfinite(a) and math.isfinite(b), (y, rate)
        assert abs(a - b) <= 4.0 * max(math.ulp(y * lr), math.ulp(a))          # (one rounding apart, not another formula)


def test_python_helpers_take_poisson():
    """observation_forecast and predictive_log_likelihood against plain numpy; the Gibbs samplers refuse."""
    import cpprob_amd.forecast as fc
    import cpprob_amd.gibbs as gibbs
    import cpprob_amd.pgibbs as pgibbs
    rng = np.random.default_rng(3)
    lam = np.array([0.5, 4.0, 12.0])
    f = rng.dirichlet(np.ones(3), 5)
    f8 = np.concatenate([f, np.zeros((5, 5))], axis=1)
    mean, var = fc.observation_forecast(f8, lam, emission="poisson")
    assert np.allclose(mean, f @ lam, rtol=1e-14) and np.allclose(var, f @ lam + f @ lam ** 2 - (f @ lam) ** 2, rtol=1e-13)
    y = np.array([0.0, 3.0, 11.0, 40.0, 1.0])
    got = fc.predictive_log_likelihood(f8, lam, y, emission="poisson")
    pmf = np.array([[math.exp(v * math.log(l) - l - math.lgamma(v + 1.0)) for l in lam] for v in y])
    assert np.allclose(got, np.log((f * pmf).sum(axis=1)), rtol=1e-12)
    with pytest.raises(ValueError):
        fc.observation_forecast(f8, lam, sigmas=np.ones(3), emission="poisson")
    with pytest.raises(NotImplementedError, match="poisson"):
        gibbs.sample_tables({}, 2, rng, emission="poisson")
    with pytest.raises(NotImplementedError, match="poisson"):
        gibbs.hmm_table_gibbs(None, [y], lam[None, :2], np.full((1, 2, 2), 0.5), 8, [1], 1, rng, emission="poisson")
    with pytest.raises(NotImplementedError, match="poisson"):
        pgibbs.hmm_table_particle_gibbs(None, [y], lam[None, :2], np.full((1, 2, 2), 0.5), 8, [1], 1, rng, emission="poisson")
