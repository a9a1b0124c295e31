"""The invariance experiment of tests/csmc_law.py as ONE batch on the device: B = 16384 problems of T = 3 steps, n = 2 particles,
one shared table.  Problem i runs a conditional run under seed i on a reference path drawn from the exactly enumerated posterior and
draws one backward trajectory; the 8 path frequencies lie within 5 sqrt(p (1 - p) / B) of the exact law, and -- the masses being
the reference's bits -- the histogram is the CPU test's, exactly.  The same sweep on cpprob_hip_batch_run's masses misses a cell by
more than twice that bound."""
import numpy as np
import pytest

import cpprob_amd as cp
import csmc_law as LAW

pytestmark = pytest.mark.gpu


def _begin(engine):
    engine.set_hmm(np.array(LAW.MEANS), np.array(LAW.TRANS))
    engine.batch_begin(cp.MODEL_HMM_TABLE, np.tile(np.array(LAW.OBS), (LAW.N, 1)), LAW.N_PARTICLES, keep_history=False, keep_masses=True)


def test_one_sweep_of_the_batch_leaves_the_posterior_invariant(engine):
    p, bound = LAW.exact_law(), LAW.bound()
    _begin(engine)
    engine.batch_run_conditional(np.arange(LAW.N, dtype=np.uint64), LAW.reference_paths().reshape(-1))
    _, traj = engine.batch_smooth(1)
    hist = LAW.histogram(np.array([t[:, 0] for t in traj]))
    miss = np.abs(hist - p) / bound
    print("conditional sweep on the device: worst cell at %.3f of the 5 sigma bound (cells %s)" % (miss.max(), np.round(miss, 3).tolist()))
    assert np.all(miss <= 1.0), miss
    assert np.array_equal(hist, LAW.conditional_histogram()), "the device's histogram differs from the CPU reference's"


def test_the_unconditional_sweep_of_the_batch_does_not(engine):
    p, bound = LAW.exact_law(), LAW.bound()
    _begin(engine)
    engine.batch_run(np.arange(LAW.N, dtype=np.uint64))
    _, traj = engine.batch_smooth(1)
    hist = LAW.histogram(np.array([t[:, 0] for t in traj]))
    miss = np.abs(hist - p) / bound
    print("unconditional sweep on the device: worst cell at %.3f of the 5 sigma bound (cells %s)" % (miss.max(), np.round(miss, 3).tolist()))
    assert miss.max() > 2.0, miss
    assert np.array_equal(hist, LAW.unconditional_histogram()), "the device's histogram differs from the oracle's"
