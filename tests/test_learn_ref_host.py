"""tests/learn_ref.py on the CPU: in Fractions, with gamma[t] = 1 / (t + 1) and no M-step, L times the record EQUALS
tests/onlinestats_ref.py's record (the discounted push is the running mean of the plain sums); in doubles the tau is the same bits
however the stream is cut while no M-step fires; a record row without mass leaves its transition row and its mean as they were.

The exact cases keep the integers small (masses below 16, transition rows of sixteenths, observes of quarters) so that the
denominators of a 64-step walk stay short; the identity does not depend on their size."""
from fractions import Fraction
import math

import numpy as np
import pytest

import learn_ref as G
import onlinestats_ref as N

LOG_NORM = math.log(2 * 3.14159265358979323846 * 1.0 * 1.0)


def make_case(k, T, seed, small=False):
    """(m, trans, obs): integer masses with state k - 1 absent from some generations, a transition table with a zero entry and,
    where T >= 2, a generation that holds state 0 alone with trans[0][1] = 0 (D[1] = 0 at the step after it)."""
    rng = np.random.default_rng(seed)
    if small:
        trans = rng.integers(1, 5, (k, k)).astype(np.float64)
    else:
        trans = rng.uniform(0.05, 1.0, (k, k))
    trans[k - 1, 0] = 0.0
    trans[0, 1] = 0.0
    if small:
        trans[np.arange(k), np.arange(k)] += 64 - trans.sum(1)             # rows of sixty-fourths: the words are exact
        assert np.all(trans >= 0) and np.all(trans.sum(1) == 64)
        trans /= 64.0
    top = 16 if small else 1 << 40
    m = [[int(v) for v in rng.integers(1, top, k)] for _ in range(T)]
    for t in range(T):
        if t % 3 == 1:
            m[t][k - 1] = 0
    if T >= 2:
        m[T // 2 - 1 if T > 2 else 0] = [int(rng.integers(1, top))] + [0] * (k - 1)
    obs = np.round(rng.uniform(-4.0, 4.0, T) * 4) / 4 if small else rng.uniform(-4.0, 4.0, T)
    return m, trans, obs


@pytest.mark.parametrize("k", [2, 5, 8])
@pytest.mark.parametrize("T", [1, 2, 7, 64])
def test_the_harmonic_steps_give_the_running_mean_exactly(k, T):
    m, trans, obs = make_case(k, T, 100 * k + T, small=True)
    gamma = [Fraction(1, t + 1) for t in range(T)]
    lr = G.Learner(np.zeros(k), trans, k, gamma, None, LOG_NORM, Fraction)
    cut = T // 3
    lr.advance(m[:cut], obs[:cut])
    lr.advance(m[cut:], obs[cut:])
    P = G.masses_of_words(lr.thr, k)
    want = N.record(m, P, obs, F=Fraction)
    assert [T * v for v in lr.record] == want
    assert sum(lr.record[64:72]) == 1 and sum(lr.record[:64]) == Fraction(T - 1, T)
    if T >= 2:
        assert lr.fallbacks >= 1, "a row with D = 0 should have taken the defensive rule"
    assert lr.changed == 0 and lr.status == 0


@pytest.mark.parametrize("k", [2, 5, 8])
def test_any_cut_gives_the_same_tau_while_no_m_step_fires(k):
    T = 9
    m, trans, obs = make_case(k, T, 30 + k)
    if k == 2:
        trans[0, 1], trans[1, 0] = 0.3, 0.2                                 # (k = 2: with a zero entry the weights into state 0 are (1, 0) under any table)
    gamma = [(t + 1) ** -0.6 for t in range(T)]

    def walk(cuts, t_min):
        lr = G.Learner(np.zeros(k), trans, k, gamma, t_min, LOG_NORM)
        at = 0
        for L in list(cuts) + [T]:
            lr.advance(m[at:L], obs[at:L])
            at = max(at, L)
        return lr
    whole = walk([], None)
    for cuts in ([1, 2, 3, 4, 5, 6, 7, 8], [0, 0, 4], [3, 3, 8], [9, 9]):
        lr = walk(cuts, None)
        assert np.array_equal(G.tau_array(lr.tau), G.tau_array(whole.tau)), cuts
        assert np.array_equal(G.record_array(lr.record), G.record_array(whole.record)), cuts
    # a burn-in the stream reaches only with its last advance: the tau is still the same, the table is not
    late = walk([3, 8], T)
    assert np.array_equal(G.tau_array(late.tau), G.tau_array(whole.tau)) and late.changed == 1
    # an M-step in between changes the words the later pushes read
    early = walk([3, 8], 3)
    assert early.changed >= 2 and not np.array_equal(G.tau_array(early.tau), G.tau_array(whole.tau))


def test_a_record_row_without_mass_leaves_its_row_and_its_mean():
    """A state that no generation holds: its occupation and its row of xi are 0.0, the M-step keeps its mean and its transition row."""
    k, T = 3, 7
    rng = np.random.default_rng(5)
    trans = rng.uniform(0.05, 1.0, (k, k))
    means = np.array([-1.5, 0.25, 2.0])
    m = [[int(v) for v in rng.integers(1, 1 << 40, k)] for _ in range(T)]
    for row in m:
        row[1] = 0
    obs = rng.uniform(-4.0, 4.0, T)
    gamma = [(t + 1) ** -0.6 for t in range(T)]
    lr = G.Learner(means, trans, k, gamma, 2, LOG_NORM)
    lr.advance(m, obs)
    rec = G.record_array(lr.record)
    assert np.all(rec[8:8 + k] == 0.0) and rec[64 + 1] == 0.0
    assert lr.status == 0 and lr.changed == 1
    assert np.array_equal(lr.trans[1], trans[1]) and lr.means[1] == means[1]
    assert not np.array_equal(lr.trans[0], trans[0]) and lr.means[0] != means[0] and lr.means[2] != means[2]
    assert np.allclose(lr.trans[[0, 2]].sum(1), 1.0)
    # nothing new: the M-step does not fire again, the record is read out again
    before = (lr.means.copy(), lr.trans.copy(), lr.thr.copy())
    lr.advance([], [])
    assert np.array_equal(G.record_array(lr.record), rec) and lr.changed == 1
    assert np.array_equal(lr.means, before[0]) and np.array_equal(lr.trans, before[1]) and np.array_equal(lr.thr, before[2])
