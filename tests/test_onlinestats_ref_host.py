"""tests/onlinestats_ref.py against the backward walk, on the CPU: in Fractions the forward-only record EQUALS the backward walk's 88
numbers (the mathematics of csrc/batch_onlinestats.hpp); in doubles the reference gives the same bits however the steps are cut into
calls, and differs from tests/suffstats_ref.py's stats() by rounding only.

The doubles bound.  The two routes order their roundings differently, so their distance grows with the steps summed: the figure is
r = max over the 88 columns of |forward - backward| / max(1, |backward|), in units of T * 2^-52.  Measured with the two CPU references
on the cases of this file (profiles/r25_notes.md lists them): the worst r is 0.62 (k = 8, T = 2; 0.10 at T = 64, 0.03 at T = 600);
the bound asserted is 4 times the worst, R_BOUND * T * 2^-52 -- the factor guards against other case seeds, the exact identity is
the check of the mathematics."""
from fractions import Fraction

import numpy as np
import pytest

import backward_ref as R
import onlinestats_ref as N
import suffstats_ref as S

R_WORST = 0.62                                  # measured, see above
R_BOUND = 4 * R_WORST


def make_case(k, T, seed, absent=True, zero_entry=True, dead_row=True):
    """(m, P, obs): integer masses with state k - 1 absent from some generations (absent), a transition table with a zero entry
    (zero_entry) and, where T >= 2, a generation that holds state 0 alone with trans[0][1] = 0, so that D[1] = 0 at the step after
    it (dead_row)."""
    rng = np.random.default_rng(seed)
    trans = rng.uniform(0.05, 1.0, (k, k))
    if zero_entry:
        trans[k - 1, 0] = 0.0
    if dead_row:
        trans[0, 1] = 0.0
    P = R.transition_masses(trans)
    m = [[int(v) for v in rng.integers(1, 1 << 40, k)] for _ in range(T)]
    for t in range(T):
        if absent and t % 3 == 1:
            m[t][k - 1] = 0
    if dead_row and T >= 2:
        m[T // 2 - 1 if T > 2 else 0] = [int(rng.integers(1, 1 << 40))] + [0] * (k - 1)
    obs = rng.uniform(-4.0, 4.0, T)
    return m, P, obs


def ratio(fwd, bwd, T):
    fwd, bwd = np.asarray(fwd), np.asarray(bwd)
    return float(np.max(np.abs(fwd - bwd) / np.maximum(1.0, np.abs(bwd)))) / (T * 2.0 ** -52)


@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("T", [1, 2, 9])
def test_forward_only_equals_the_backward_walk_exactly(k, T):
    m, P, obs = make_case(k, T, 100 * k + T)
    run = N.Running(Fraction)
    run.consume(m, P, obs)
    fwd = run.read(m)
    bwd = N.backward_record(m, P, obs, Fraction)
    assert fwd == bwd
    if T >= 2:
        assert run.fallbacks >= 1, "a row with D = 0 should have taken the defensive rule"
        assert any(P[s][sn] == 0 for s in range(k) for sn in range(k))
        assert any(row[k - 1] == 0 for row in m)
    occ = fwd[64:72]
    assert sum(occ) == T and all(v == 0 for v in occ[k:])
    assert sum(fwd[:64]) == T - 1
    for s in range(8):
        for sn in range(8):
            if s >= k or sn >= k:
                assert fwd[8 * s + sn] == 0


def test_exact_identity_without_the_special_rows_and_without_observes():
    m, P, _ = make_case(3, 9, 5, absent=False, zero_entry=False, dead_row=False)
    assert N.record(m, P, None, F=Fraction) == N.backward_record(m, P, None, Fraction)
    assert all(v == 0 for v in N.record(m, P, None, F=Fraction)[72:])
    assert N.record([], P, None) == [0.0] * 88


def test_the_fraction_walk_in_floats_is_suffstats_ref():
    """backward_record is stats()' walk: over floats it gives stats()' bits, so the exact identity speaks about that walk."""
    for k, T in ((2, 9), (3, 9), (8, 9), (3, 1)):
        m, P, obs = make_case(k, T, 7 * k + T)
        assert np.array_equal(N.as_array(N.backward_record(m, P, obs, float)), S.record(S.stats(m, P, obs)))


@pytest.mark.parametrize("k", [2, 3, 8])
def test_any_cut_gives_the_same_bits(k):
    m, P, obs = make_case(k, 9, 30 + k)
    whole = N.as_array(N.record(m, P, obs))
    for cuts in ([1, 2, 3, 4, 5, 6, 7, 8], [0, 0, 4], [3, 3, 8], [9, 9]):
        assert np.array_equal(N.as_array(N.record(m, P, obs, cuts=cuts)), whole), cuts
    # reading in between changes nothing
    run = N.Running()
    for L in (2, 5, 9):
        run.consume(m[:L], P, obs)
        part = N.as_array(run.read(m[:L]))
        assert np.array_equal(part, N.as_array(N.record(m[:L], P, obs)))
        assert np.array_equal(N.as_array(run.read(m[:L])), part)
    assert np.array_equal(part, whole)


DOUBLE_CASES = [(k, T) for k in (2, 3, 8) for T in (1, 2, 9, 64)] + [(3, 300), (3, 613), (8, 600)]


@pytest.mark.parametrize("k,T", DOUBLE_CASES)
def test_doubles_against_the_backward_walk(k, T):
    m, P, obs = make_case(k, T, 1000 + 10 * T + k)
    fwd = N.as_array(N.record(m, P, obs))
    bwd = S.record(S.stats(m, P, obs))
    r = ratio(fwd, bwd, T)
    print("k = %d, T = %d: r = %.4f" % (k, T, r))
    assert r <= R_BOUND
