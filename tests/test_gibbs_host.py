"""CPU tests of cpprob_amd.gibbs.sample_tables, the conjugate draw of a table given one trajectory's sufficient statistics: its rows
are distributions, it is the statement its docstring makes (restated here on a generator of the same seed), and with the counts scaled
up it concentrates on em.m_step's tables at the rate the posterior's own spread gives."""
import numpy as np
import pytest

import cpprob_amd
import trajstats_ref as TS
from cpprob_amd.em import m_step
from cpprob_amd.gibbs import sample_tables


def _stats(B, k, seed, T=200):
    """One random path's record a problem, stacked as Engine.batch_traj_stats returns them with the trajectory axis indexed away."""
    rng = np.random.default_rng(seed)
    recs = [TS.stats(rng.integers(0, k, T), rng.uniform(-4.0, 4.0, T)) for _ in range(B)]
    return {f: np.stack([r[f] for r in recs]) for f in ("xi", "occ", "occ_y", "occ_yy")}


def test_exported_beside_em():
    assert cpprob_amd.gibbs.sample_tables is cpprob_amd.sample_tables and callable(cpprob_amd.hmm_table_gibbs)
    assert "particle" in cpprob_amd.hmm_table_gibbs.__doc__ and "not a particle-gibbs" in cpprob_amd.hmm_table_gibbs.__doc__.lower()


@pytest.mark.parametrize("k", [2, 5, 8])
def test_rows_are_distributions(k):
    means, trans = sample_tables(_stats(6, k, 3), k, np.random.default_rng(1))
    assert means.shape == (6, k) and trans.shape == (6, k, k)
    assert np.all(trans > 0.0) and np.all(np.isfinite(means))
    # a row is k doubles divided by their sum: every quotient and the k - 1 additions of the check round once, each by at most 2^-53
    # of a value <= 1
    assert np.abs(trans.sum(-1) - 1.0).max() <= (2 * k - 1) * 2.0 ** -53


def test_draw_is_the_stated_one_and_reproducible():
    k, B = 3, 4
    st = _stats(B, k, 5)
    got_m, got_t = sample_tables(st, k, np.random.default_rng(77), alpha=0.5, mu0=1.0, tau0=3.0)
    again_m, again_t = sample_tables(st, k, np.random.default_rng(77), alpha=0.5, mu0=1.0, tau0=3.0)
    assert np.array_equal(got_m, again_m) and np.array_equal(got_t, again_t)
    rng = np.random.default_rng(77)
    G = rng.standard_gamma(0.5 + st["xi"][:, :k, :k])
    want_t = G / G.sum(-1, keepdims=True)
    z = rng.standard_normal((B, k))
    prec = 1 / 3.0**2 + st["occ"][:, :k]
    want_m = (1.0 / 3.0**2 + st["occ_y"][:, :k]) / prec + z / np.sqrt(prec)
    assert np.array_equal(got_t, want_t) and np.array_equal(got_m, want_m)
    other_m, other_t = sample_tables(st, k, np.random.default_rng(78), alpha=0.5, mu0=1.0, tau0=3.0)
    assert not np.array_equal(other_m, got_m) and not np.array_equal(other_t, got_t)
    # states >= k of the record are not read
    poisoned = {f: v.copy() for f, v in st.items()}
    poisoned["xi"][:, k:] = np.nan
    poisoned["xi"][:, :, k:] = np.nan
    poisoned["occ"][:, k:] = np.nan
    poisoned["occ_y"][:, k:] = np.nan
    pm, pt = sample_tables(poisoned, k, np.random.default_rng(77), alpha=0.5, mu0=1.0, tau0=3.0)
    assert np.array_equal(pm, got_m) and np.array_equal(pt, got_t)
    with pytest.raises(ValueError):
        sample_tables({"xi": st["xi"][0], "occ": st["occ"][0], "occ_y": st["occ_y"][0]}, k, rng)


def test_large_counts_concentrate_on_the_m_step():
    """Counts scaled by 10^6: the draw lies within 6 posterior standard deviations of m_step's tables.  A mean: its posterior is
    N(.., 1 / prec), and the posterior mean differs from occ_y / occ by the prior's pull, |occ_y / occ - mu0| / (tau0^2 prec), added
    to the bound.  A transition entry: Dirichlet(a) has variance p (1 - p) / (a_0 + 1) at p = a / a_0, and its mean differs from the
    frequency by at most k alpha / a_0."""
    k, B, scale = 3, 5, 1e6
    st = {f: v * scale for f, v in _stats(B, k, 9).items()}
    mle_m, mle_t = m_step(st, np.zeros((B, k)), np.full((B, k, k), 1.0 / k))
    means, trans = sample_tables(st, k, np.random.default_rng(2))
    prec = 1 / 10.0**2 + st["occ"][:, :k]
    bound_m = 6.0 / np.sqrt(prec) + np.abs(mle_m) / (10.0**2 * prec)
    assert np.all(np.abs(means - mle_m) <= bound_m), np.abs(means - mle_m).max()
    a0 = (1.0 + st["xi"][:, :k, :k]).sum(-1, keepdims=True)
    p = (1.0 + st["xi"][:, :k, :k]) / a0
    bound_t = 6.0 * np.sqrt(p * (1 - p) / (a0 + 1)) + k * 1.0 / a0
    assert np.all(np.abs(trans - mle_t) <= bound_t), (np.abs(trans - mle_t) / bound_t).max()
    assert bound_m.max() < 1e-3 and bound_t.max() < 1e-3      # (the bounds themselves have shrunk: the draw IS the M-step to three digits)
