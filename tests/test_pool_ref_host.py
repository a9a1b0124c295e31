"""tests/pool_ref.py against cpprob_amd.em.pool_stats, the numpy statement the device's pooling kernel is held to, and the fixtures
against themselves: the order of the additions is visible in them.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import cpprob_amd as cp
from cpprob_amd import em
from cpprob_amd.capi import split_stats, split_traj_stats

import pool_ref as P


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_case_has_the_sizes_around_the_look_ahead():
    groups, sizes = P.case_groups()
    A = P.pool_ahead()
    assert sizes[:5] == [1, A - 1, A, A + 1, 2 * A + 3] and sum(sizes) == 40 and sizes[5] >= 1
    assert [len(m) for m in P.members(groups)] == sizes
    # interleaved: no group of more than one member is a run of neighbours
    for m in P.members(groups):
        assert len(m) == 1 or m[-1] - m[0] + 1 > len(m), m
    # a last workgroup with idle wavefronts, for R = 1 and R = 3
    assert len(sizes) % 4 != 0 and (3 * len(sizes)) % 4 != 0


@pytest.mark.parametrize("R", [1, 3])
def test_the_fixtures_see_the_order(R):
    groups, rec = P.case(R, 7 + R)
    assert np.abs(rec).max() / np.abs(rec).min() > 2.0 ** 50
    assert (rec[:, :, 64:] > 0).any() and (rec[:, :, 64:] < 0).any() and np.all(rec != 0.0)
    up, down = P.pool(rec, groups, broadcast=False), P.pool(rec, groups, broadcast=False, descending=True)
    assert up.shape == down.shape == (6, R, P.RECORD)
    assert not np.array_equal(_bits(up), _bits(down))
    # the group of one is its record either way; the exact sums are what both round
    one = P.members(groups)[0][0]
    assert np.array_equal(_bits(up[0]), _bits(rec[one])) and np.array_equal(_bits(down[0]), _bits(rec[one]))
    exact = P.pool_exact(rec, groups)
    flat = up.reshape(6, -1)
    err = max(abs(Fraction(float(flat[g, e])) - exact[g][e]) / max(abs(exact[g][e]), Fraction(1, 2 ** 40)) for g in range(6) for e in range(flat.shape[1]))
    assert any(Fraction(float(flat[g, e])) != exact[g][e] for g in range(6) for e in range(flat.shape[1])) and err < Fraction(1, 2 ** 10)


@pytest.mark.parametrize("R", [1, 3])
def test_pool_stats_is_the_restatement(R):
    groups, rec = P.case(R, 20 + R)
    for broadcast in (True, False):
        want = P.pool(rec, groups, broadcast=broadcast)
        got = em.pool_stats(rec, groups, broadcast=broadcast)
        assert got.shape == want.shape and got.dtype == np.float64 and np.array_equal(_bits(got), _bits(want)), broadcast
    if R == 1:
        got = cp.pool_stats(rec[:, 0], groups)
        assert got.shape == (40, P.RECORD) and np.array_equal(_bits(got), _bits(P.pool(rec, groups)[:, 0]))
    # broadcast=False rows are the broadcast rows of each group's first member
    full, compact = em.pool_stats(rec, groups), em.pool_stats(rec, groups, broadcast=False)
    lead = [m[0] for m in P.members(groups)]
    assert np.array_equal(_bits(compact), _bits(full[lead]))
    for m in P.members(groups):
        for b in m:
            assert np.array_equal(_bits(full[b]), _bits(full[m[0]]))
    # the input is not written
    assert np.array_equal(_bits(rec), _bits(P.case(R, 20 + R)[1]))


def test_pool_stats_takes_the_dicts():
    groups, rec = P.case(3, 33)
    want = P.pool(rec, groups)
    got = em.pool_stats(split_traj_stats(rec), groups)
    for name, w in split_traj_stats(want).items():
        assert got[name].shape == w.shape and np.array_equal(_bits(got[name]), _bits(w)), name
    got = em.pool_stats(split_stats(rec[:, 1]), groups, broadcast=False)
    for name, w in split_stats(P.pool(rec[:, 1], groups, broadcast=False)).items():
        assert got[name].shape == w.shape and np.array_equal(_bits(got[name]), _bits(w)), name


def test_groups_of_one_return_the_records_and_a_negative_zero_becomes_zero():
    rec = np.random.default_rng(3).normal(size=(5, P.RECORD))
    rec[2, 70] = -0.0
    got = em.pool_stats(rec, np.arange(5)[::-1].copy(), broadcast=True)
    want = rec.copy()
    want[2, 70] = 0.0                                       # (0.0 + -0.0)
    assert np.array_equal(_bits(got), _bits(want))
    compact = em.pool_stats(rec, np.arange(5)[::-1].copy(), broadcast=False)
    assert np.array_equal(_bits(compact), _bits(want[::-1]))


@pytest.mark.parametrize("groups", [[0, 1, 3], [0, -1, 1], [1, 1, 2], [0, 1], [[0, 1, 2]], [0.0, 1.0, 1.0]])
def test_pool_stats_refuses_what_is_no_partition(groups):
    with pytest.raises(ValueError):
        em.pool_stats(np.zeros((3, P.RECORD)), np.asarray(groups))
