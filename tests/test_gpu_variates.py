"""The device's variate generators against their exact quantile functions (tests/variate_ref.py), on chosen bits through
cpprob_hip_variate_from_bits and by seed through the shipped cpprob_hip_draw_* entries.  The cases, the criteria and the derivation of the
Poisson bound are in tests/variate_cases.py; tests/test_variates_host.py runs the same cases on the CPU oracle and checks the reference.

  smallint, discrete   the exact quantile (array_equal); a zero-weight index is never drawn
  uniform_real         one of the two doubles next to the exact a + (b - a) u, and a <= x < b
  poisson              the exact quantile at some u' within delta(mean) <= 2^-40 of u, never above the exact quantile of 1 - 2^-54
  normal               |got - ref| <= 3 2^-52 |ref|; exact where the reference is 0 or +-s
"""
import numpy as np
import pytest

from devmem import dtensor, dzeros

from oracle import oracle as O
import cpprob_amd as cp

import variate_cases as V

pytestmark = pytest.mark.gpu

EINVAL = -1                                    # CPPROB_HIP_EINVAL


class DeviceBackend:
    def __init__(self, engine):
        self.e = engine

    def from_bits(self, which, params, blocks):
        import torch
        n = len(blocks)
        d_blocks = dtensor(blocks.view(np.int32))
        out0 = dzeros(n, dtype=torch.float64)
        out1 = dzeros(n, dtype=torch.float64) if which == V.NORMAL else None
        self.e.variate_from_bits(which, [float(p) for p in params], d_blocks, out0, out1)
        self.e.sync()
        return out0.cpu().numpy(), (out1.cpu().numpy() if out1 is not None else None)

    def by_seed(self, which, params, seed, pid0, draw, n):
        import torch
        out = dzeros(n, dtype=torch.float64 if which in (V.UNIFORM_REAL, V.NORMAL) else torch.int32)
        if which == V.SMALLINT:
            self.e.draw_uniform_smallint(seed, pid0, draw, params[0], params[1], out)
        elif which == V.DISCRETE:
            self.e.draw_discrete(seed, pid0, draw, list(params), out)
        elif which == V.UNIFORM_REAL:
            self.e.draw_uniform_real(seed, pid0, draw, params[0], params[1], out)
        elif which == V.POISSON:
            self.e.draw_poisson(seed, pid0, draw, params[0], out)
        else:
            self.e.draw_normal(seed, pid0, draw, params[0], params[1], out)
        self.e.sync()
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def be(engine):
    return DeviceBackend(engine)


def test_constants_agree():
    assert (cp.capi.VARIATE_SMALLINT, cp.capi.VARIATE_DISCRETE, cp.capi.VARIATE_UNIFORM_REAL, cp.capi.VARIATE_POISSON, cp.capi.VARIATE_NORMAL) == \
        (V.SMALLINT, V.DISCRETE, V.UNIFORM_REAL, V.POISSON, V.NORMAL)
    assert cp.capi.POISSON_MAX_MEAN == V.POISSON_MAX_MEAN


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


def test_refusals_leave_the_context_usable(be):
    """CPPROB_HIP_EINVAL for parameters the generators are not defined on, from the draw entries and from the from-bits entry; the context
    draws correctly afterwards."""
    one = V._blocks_word0([0])
    for which, params in V.REFUSED:
        with pytest.raises(cp.CpprobHipError) as err:
            be.by_seed(which, params, 1, 0, 0, 4)
        assert err.value.code == EINVAL, (which, params)
        if which != V.SMALLINT:                                      # (the from-bits entry returns doubles: its smallint takes any b - a < 2^32)
            with pytest.raises(cp.CpprobHipError) as err:
                be.from_bits(which, params, one)
            assert err.value.code == EINVAL, (which, params)
    for which, params in ((V.SMALLINT, (0, 2 ** 32)), (V.SMALLINT, (0.5, 2)), (V.SMALLINT, (3, 2)), (V.SMALLINT, (0,)), (V.DISCRETE, ()),
                          (V.DISCRETE, [1.0] * 9), (V.POISSON, ()), (V.NORMAL, (0.0,)), (5, ())):
        with pytest.raises(cp.CpprobHipError) as err:
            be.from_bits(which, params, one)
        assert err.value.code == EINVAL, (which, params)
    V.check_discrete_bits(be)
    got = be.by_seed(V.POISSON, (V.POISSON_MAX_MEAN,), 1, 0, 0, 4)   # the limit itself is accepted
    assert np.all((got > 9000) & (got < 11000))
