"""The conditional SMC run's reference (tests/csmc_ref.py) on the CPU: one sweep "conditional run, then one backward-simulated
trajectory" leaves the exactly enumerated posterior of a small table HMM invariant at n = 2 particles, where the same sweep on an
unconditional run's masses does not; and the structure of the rows it leaves.  Nothing runs on a GPU."""
import numpy as np

import backward_ref as R
import csmc_law as LAW
import csmc_ref as CS


def test_one_sweep_leaves_the_posterior_invariant():
    """N = 16384 reference paths drawn from the exact posterior, seeds 0 .. N - 1, n = 2: every one of the 8 path frequencies after the
    sweep lies within 5 sqrt(p (1 - p) / N) of the exact p -- a statement about iid draws of the posterior."""
    p, bound = LAW.exact_law(), LAW.bound()
    assert abs(p.sum() - 1.0) < 1e-12 and np.all(p > 0.0)
    before = np.abs(LAW.histogram(LAW.reference_paths()) - p) / bound
    assert before.max() <= 1.0, "the reference paths themselves are draws of the posterior"
    miss = np.abs(LAW.conditional_histogram() - p) / bound
    print("conditional sweep: worst cell at %.3f of the 5 sigma bound (cells %s)" % (miss.max(), np.round(miss, 3).tolist()))
    assert np.all(miss <= 1.0), miss


def test_the_unconditional_sweep_does_not():
    """With masses from the oracle's unconditional n = 2 run instead, at least one cell misses by more than twice the bound."""
    p, bound = LAW.exact_law(), LAW.bound()
    miss = np.abs(LAW.unconditional_histogram() - p) / bound
    print("unconditional sweep: worst cell at %.3f of the 5 sigma bound (cells %s)" % (miss.max(), np.round(miss, 3).tolist()))
    assert miss.max() > 2.0, miss


def _problem(k, T, seed):
    rng = np.random.default_rng(seed)
    trans = rng.uniform(0.05, 1.0, (k, k))
    ll = (-rng.uniform(0.0, 8.0, (T, k))).tolist()
    return ll, R.thresholds(trans), rng.integers(0, k, T)


def test_one_particle_gives_one_hot_rows_at_the_reference():
    for k in (2, 5, 8):
        ll, thr, ref = _problem(k, 6, 3 + k)
        m = CS.masses(ll, thr, 99, 1, ref)
        for t in range(6):
            assert [s for s in range(k) if m[t][s] > 0] == [int(ref[t])]
            assert m[t][int(ref[t])] == int(R.filtering_masses([[int(ref[t])]], [ll[t]])[0][int(ref[t])])


def test_rows_are_the_masses_of_n_particles_with_the_reference_among_them():
    for k, n in ((2, 2), (3, 5), (5, 257), (8, 1025)):
        ll, thr, ref = _problem(k, 4, 11 * k + n)
        xs, m = CS.states(ll, thr, 1234 + n, n, ref)
        assert xs.shape == (4, n) and np.array_equal(xs[:, 0], ref) and xs.min() >= 0 and xs.max() < k
        assert m == R.filtering_masses(xs, ll), "every row is the masses of a generation of n particles"
        assert CS.masses(ll, thr, 1234 + n, n, ref) == m
        # the first generation is the forward run's own: uniform_smallint on the particle's word of draw 0
        other = CS.states(ll, thr, 1234 + n, n, (ref + 1) % k)[0]
        assert np.array_equal(other[0, 1:], xs[0, 1:])


def test_a_reference_state_past_k_is_the_last_state():
    ll, thr, ref = _problem(3, 5, 8)
    bad = np.array(ref)
    bad[1], bad[3] = 7, 3
    good = np.array(ref)
    good[1], good[3] = 2, 2
    assert CS.masses(ll, thr, 5, 4, bad) == CS.masses(ll, thr, 5, 4, good)
    assert CS.masses(ll, thr, 5, 4, bad + 8) == CS.masses(ll, thr, 5, 4, good), "the low three bits count"
