"""Particle Gibbs with backward sampling for HMM tables (cpprob_amd/pgibbs.py: hmm_table_particle_gibbs) on the device: its wiring
against the loop written out here with the host forms, and its law against Gibbs with exact forward filtering / backward sampling on
the CPU at n = 4 particles -- where the retained path is what keeps the chain on the posterior.

The statistical test is tests/test_gpu_gibbs.py's own: per entry (the two means, the two diagonal transition entries) the
chain-averaged posterior means of 8 particle-Gibbs chains and 8 exact chains differ by at most 4 sqrt(se_exact^2 + se_particle^2), the
standard errors taken across chains; that file's samplers, summaries, starts and sequence are imported, with its B and SWEEPS.  What
hmm_table_gibbs (the unconditional filter) gives at the same n = 4 is printed beside it, without an assertion."""
import numpy as np
import pytest

import cpprob_amd as cp
from cpprob_amd.gibbs import sample_tables
from test_gpu_gibbs import B, BURN, SWEEPS, exact_gibbs, simulated_sequence, starts, summaries

pytestmark = pytest.mark.gpu

N = 4


def test_driver_is_the_loop_it_states(engine):
    """hmm_table_particle_gibbs equals begin, run (sweep 0) or batch_run_conditional on the previous sweep's batch_smooth(1) path,
    batch_traj_stats(1, draw_index = sweep), sample_tables, written out with the host forms."""
    obs = [simulated_sequence()[:40], simulated_sequence(7)[:23], simulated_sequence(9)[:31]]
    nb, sweeps = 3, 5
    means0 = np.array([[-1.0, 1.0], [-0.5, 0.5], [-3.0, 0.0]])
    trans0 = np.tile(np.full((2, 2), 0.5), (nb, 1, 1))
    seeds = np.array([5, 6, 7], np.uint64)
    got = cp.hmm_table_particle_gibbs(engine, obs, means0, trans0, 6, seeds, sweeps, np.random.default_rng(3), tau0=5.0)
    rng = np.random.default_rng(3)
    means, trans = means0.copy(), trans0.copy()
    m_hist, t_hist, path = [means.copy()], [trans.copy()], None
    for i in range(sweeps):
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 6, tables=(means, trans), keep_history=False, keep_masses=True)
        if i == 0:
            engine.batch_run(seeds)
        else:
            engine.batch_run_conditional(seeds + np.uint64(i), path)
        path = [t[:, 0] for t in engine.batch_smooth(1, draw_index=i)[1]]
        st = engine.batch_traj_stats(1, draw_index=i, observes=obs)
        means, trans = sample_tables({f: v[:, 0] for f, v in st.items()}, 2, rng, tau0=5.0)
        m_hist.append(means.copy())
        t_hist.append(trans.copy())
    assert len(got) == 2 and got[0].shape == (sweeps + 1, nb, 2) and got[1].shape == (sweeps + 1, nb, 2, 2)
    assert np.array_equal(got[0], np.array(m_hist)) and np.array_equal(got[1], np.array(t_hist))
    assert not np.array_equal(got[0][1], got[0][2])


def test_particle_gibbs_chain_matches_exact_ffbs_gibbs_at_four_particles(engine):
    obs = simulated_sequence()
    means0, trans0 = starts()
    e_means, e_trans = exact_gibbs(obs, means0, trans0, SWEEPS, np.random.default_rng(101))
    p_means, p_trans = cp.hmm_table_particle_gibbs(engine, obs, means0, trans0, N, np.arange(B, dtype=np.uint64) + 900, SWEEPS, np.random.default_rng(202))
    u_means, u_trans, _ = cp.hmm_table_gibbs(engine, obs, means0, trans0, N, np.arange(B, dtype=np.uint64) + 900, SWEEPS, np.random.default_rng(202), keep_history=False)
    e_avg, e_se = summaries(e_means, e_trans)
    p_avg, p_se = summaries(p_means, p_trans)
    u_avg, u_se = summaries(u_means, u_trans)
    width = 4.0 * np.sqrt(e_se**2 + p_se**2)
    for j, name in enumerate(("means[0]", "means[1]", "trans[0][0]", "trans[1][1]")):
        print("%s: exact %.4f (se %.4f), particle Gibbs n = %d %.4f (se %.4f), difference %.4f, allowed %.4f; hmm_table_gibbs n = %d %.4f (se %.4f), difference %.4f" % (
            name, e_avg[j], e_se[j], N, p_avg[j], p_se[j], abs(p_avg[j] - e_avg[j]), width[j], N, u_avg[j], u_se[j], abs(u_avg[j] - e_avg[j])))
    assert np.all(np.abs(p_avg - e_avg) <= width), "particle Gibbs - exact = %s, allowed %s" % (p_avg - e_avg, width)
    # the labels did not switch, and the chains found the levels
    assert np.all(p_means[BURN + 1:, :, 0] < p_means[BURN + 1:, :, 1]) and np.all(e_means[BURN + 1:, :, 0] < e_means[BURN + 1:, :, 1])
    assert abs(e_avg[0] + 2.0) < 0.5 and abs(e_avg[1] - 2.0) < 0.5
