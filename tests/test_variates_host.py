"""CPU twins of tests/test_gpu_variates.py: the same cases (tests/variate_cases.py) on the oracle's generator functions, which restate
the device's, against the exact references of tests/variate_ref.py -- and the conditions on the reference side that those cases rest on.

What counts as right.  An integer-valued generator returns k that is the exact quantile at some u' with |u' - u| <= delta: delta = 0 for
uniform_smallint (integer arithmetic) and for discrete on rows whose exact boundaries C_i / C_k 2^32 keep 2^-20 away from every word (or
sit on one and are computed exactly); for poisson delta is the bound variate_cases.poisson_delta derives from the generator's arithmetic,
<= 2^-40 for every tested mean, and k never exceeds the exact quantile of 1 - 2^-54.  uniform_real returns one of the two doubles next to
the exact a + (b - a) u, inside [a, b).  normal is within 3 2^-52 relative of sqrt(-2 ln u) sin / cos (pi w), exact where that is 0 or +-s.
"""
import numpy as np
import pytest

from oracle import oracle as O

import variate_cases as V
import variate_ref as R

M64 = (1 << 64) - 1


class OracleBackend:
    def __init__(self):
        self.L = O.lib()

    def from_bits(self, which, params, blocks):
        L, out1 = self.L, None
        if which == V.SMALLINT:
            a, b = params
            out0 = [((L.orc_smallint_from_bits(int(blk[0]), a & M64, b & M64) + (1 << 63)) & M64) - (1 << 63) for blk in blocks]
        elif which == V.DISCRETE:
            w = np.array(params, dtype=np.float64)
            out0 = [L.orc_discrete_from_bits(int(blk[0]), w, len(w)) for blk in blocks]
        elif which == V.UNIFORM_REAL:
            out0 = [L.orc_uniform_real_from_bits(int(blk[0]), int(blk[1]), params[0], params[1]) for blk in blocks]
        elif which == V.POISSON:
            out0 = [L.orc_poisson_from_bits(int(blk[0]), int(blk[1]), params[0]) for blk in blocks]
        else:
            z = np.array([O.box_muller(blk) for blk in blocks])
            out0, out1 = z[:, 0], z[:, 1]
        return np.array(out0, dtype=np.float64), out1

    def by_seed(self, which, params, seed, pid0, draw, n):
        L, pids = self.L, range(pid0, pid0 + n)
        if which == V.SMALLINT:
            a, b = params
            return [((L.orc_draw_smallint(seed, p, draw, a & M64, b & M64) + (1 << 63)) & M64) - (1 << 63) for p in pids]
        if which == V.DISCRETE:
            w = np.array(params, dtype=np.float64)
            return [L.orc_draw_discrete(seed, p, draw, w, len(w)) for p in pids]
        if which == V.UNIFORM_REAL:
            return [L.orc_draw_uniform_real(seed, p, draw, params[0], params[1]) for p in pids]
        if which == V.POISSON:
            return [L.orc_draw_poisson(seed, p, draw, params[0]) for p in pids]
        return [L.orc_draw_normal(seed, p, draw, params[0], params[1]) for p in pids]


@pytest.fixture(scope="module")
def be():
    return OracleBackend()


def test_reference_uniforms_are_the_pinned_bits():
    """The reference's word and pair selection against the oracle's by-seed uniforms, at aligned, odd and 32-bit-crossing ids."""
    L = O.lib()
    for pid0 in V.PID0S + V.PID0S_WIDE:
        words = R.seed_words(O, 7, pid0, 3, 9)
        pairs = R.seed_pairs(O, 7, pid0, 3, 9)
        for i in range(9):
            assert words[i] == L.orc_draw_word(7, pid0 + i, 3)
            assert R.bits53(*pairs[i]) * 2.0 ** -53 == L.orc_draw_u01_53(7, pid0 + i, 3)
    assert R.bits53(*R.words_of_bits53(2 ** 53 - 1, junk=0x7FF)) == 2 ** 53 - 1
    assert R.normal_v(R.block_of_v(2 ** 53 - 1, 12345678901234)) == (2 ** 53 - 1, 12345678901234)


def test_reference_poisson_tables():
    """The tabulated CDF against mpmath's closed form (the regularised incomplete gamma function), and k_top on both sides."""
    import mpmath
    for mean in (0.3, 4.0, 745.0, 1.0e4):
        tab = R.poisson_table(mean)
        with mpmath.workdps(60):
            for k in sorted({0, int(mean), tab.k_top - 1, tab.k_top}):
                if k < 0:
                    continue
                exact = mpmath.gammainc(k + 1, mpmath.mpf(mean), mpmath.inf, regularized=True)
                assert abs(tab.cdf[k] - exact) < mpmath.mpf(10) ** -45
            top = 1 - mpmath.mpf(2) ** -54
            assert tab.cdf[tab.k_top] >= top and (tab.k_top == 0 or tab.cdf[tab.k_top - 1] < top)
    assert R.poisson_table(0.0).k_top == 0 and R.poisson_table(2.0 ** -60).k_top == 0 and R.poisson_table(4.0).k_top < 40


def test_poisson_delta_is_small_enough():
    for mean in V.POISSON_MEANS:
        assert V.poisson_delta(R.poisson_table(mean)) <= 2.0 ** -40


def test_discrete_rows_have_no_boundary_in_rounding_reach():
    V.check_discrete_rows_are_safe()
    assert not R.discrete_row_is_safe([1.0, 1e-17, 1.0])              # (the criterion does bite: C_0 / C_2 2^32 is 1e-8 below 2^31)


def test_smallint_constructed_bits(be):
    V.check_smallint_bits(be)


def test_smallint_by_seed(be):
    V.check_smallint_seed(be, O)


def test_discrete_constructed_bits(be):
    V.check_discrete_bits(be)


def test_discrete_by_seed(be):
    V.check_discrete_seed(be, O)


def test_uniform_real_constructed_bits(be):
    V.check_uniform_real_bits(be)


def test_uniform_real_by_seed(be):
    V.check_uniform_real_seed(be, O)


@pytest.mark.parametrize("mean", V.POISSON_MEANS)
def test_poisson_constructed_bits(be, mean):
    V.check_poisson_bits(be, (mean,))


def test_poisson_by_seed(be):
    V.check_poisson_seed(be, O)


def test_normal_constructed_and_random_bits(be):
    V.check_normal_bits(be, O)


def test_normal_by_seed(be):
    V.check_normal_seed(be, O)
