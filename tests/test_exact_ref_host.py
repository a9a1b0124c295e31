"""The host pieces of the exact filter runs (include/cpprob_hip.h: cpprob_hip_batch_run_exact, csrc/batch_exact.hpp): the symbols are
declared, listed and bound; hmm_table_em's refusal; and the distance of the statement tests/exact_ref.py restates -- which the device is
held to bit for bit -- from the exact law, a float64 forward-backward on the true transition probabilities."""
import os
import re

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd.capi as cp
import exact_ref as X
import poisson_ref as PR
from cpprob_amd.em import hmm_table_em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cpprob_hip_batch_run_exact": 1, "cpprob_hip_batch_exact_evidence": 4, "cpprob_hip_batch_exact_evidence_device": 4}
# Four times the largest deviations measured over the six cases below (profiles/r38_notes.md, "Distance to the exact law"): filtering
# marginals, log-likelihood, smoothed marginals.  The factor: only these seeds were measured.
DEV_FILTER, DEV_LOG_Z, DEV_SMOOTH = 3.85e-9, 2.71e-8, 9.87e-9
TOL_FILTER, TOL_LOG_Z, TOL_SMOOTH = 4 * DEV_FILTER, 4 * DEV_LOG_Z, 4 * DEV_SMOOTH


def test_symbols_are_declared_listed_and_bound():
    header = open(os.path.join(ROOT, "include", "cpprob_hip.h")).read()
    L = cp.load_library()
    for s, n_args in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % s, header) and s in cp.SYMBOLS and len(getattr(L, s).argtypes) == n_args, s
    assert all(callable(getattr(cp.Engine, name)) for name in ("batch_run_exact", "batch_exact_evidence", "batch_exact_evidence_device"))


def test_exact_em_refuses_a_particle_store_before_the_library():
    with pytest.raises(ValueError, match="keep_history=False"):
        hmm_table_em(None, [np.zeros(3)], np.zeros((1, 2)), np.ones((1, 2, 2)), 8, [1], 1, exact=True, keep_history=True)


def law_case(k, family, T=37):
    """(ll [T][k], trans [k][k]) of one sequence: transition entries >= 1e-3, rows within 20 nats of each other."""
    rng = np.random.default_rng(1000 * k + len(family))
    trans = rng.uniform(1e-3, 1.0, (k, k)) ** 3 + 1e-3
    x = rng.integers(0, k, T)
    if family == "poisson":
        rates = np.linspace(3.0, 8.0, k)
        ll = PR.rows(rng.poisson(rates[x]).astype(np.float64), rates, k)[:, :k]
    else:
        means = np.linspace(-1.5, 1.5, k)
        ll = np.array(R.log_likelihoods(means[x] + rng.standard_normal(T), means))
    assert float((ll.max(axis=1) - ll.min(axis=1)).max()) < 20.0
    return ll, trans


def deviations(k, family):
    ll, trans = law_case(k, family)
    P = R.transition_masses(trans)
    m, log_z, dead = X.run(ll.tolist(), P)
    assert dead == -1
    alpha, want_z, gamma = X.float_forward_backward(ll, trans / trans.sum(axis=1, keepdims=True))
    filt = np.array(m)[:, :k]
    filt = filt / filt.sum(axis=1, keepdims=True)
    smooth = R.marginals([[int(v) for v in row[:k]] for row in m], P)
    return float(np.abs(filt - alpha).max()), abs(log_z - want_z), float(np.abs(smooth - gamma).max())


@pytest.mark.parametrize("family", ["unit", "poisson"])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_restatement_is_the_exact_law_within_its_quantisations(k, family):
    d_filter, d_log_z, d_smooth = deviations(k, family)
    print("k = %d, %s rows: filtering %.3g, log_z %.3g, smoothed %.3g" % (k, family, d_filter, d_log_z, d_smooth))
    assert d_filter <= TOL_FILTER and d_log_z <= TOL_LOG_Z and d_smooth <= TOL_SMOOTH
