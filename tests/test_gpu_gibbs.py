"""The batched Gibbs sampler for HMM tables (cpprob_amd/gibbs.py: hmm_table_gibbs) on the device: its wiring against a loop written
out here from Engine calls and sample_tables, and its law against Gibbs with exact forward filtering / backward sampling on the CPU.

The statistical test is a z-test whose width is the two samplers' own Monte-Carlo error: per entry (the two means, the two diagonal
transition entries) the chain-averaged posterior means of 8 particle chains and 8 exact chains must differ by at most
4 sqrt(se_exact^2 + se_particle^2), the standard errors taken across chains.  Two exact runs with different seeds pass against each
other with z <= 0.79 (measured on the CPU, generator seeds 101 and 303: standard errors 0.0044 .. 0.0055 for the means, 0.0012 ..
0.0019 for the diagonal entries, so the allowed difference is about 0.03 for a mean and 0.008 for a diagonal entry); the
O(1 / n) bias of the particle approximation at n = 256 over two well-separated states lies well inside."""
import numpy as np
import pytest

import cpprob_amd as cp
from cpprob_amd.gibbs import sample_tables
from oracle import exact

pytestmark = pytest.mark.gpu

TRUE_MEANS = np.array([-2.0, 2.0])
TRUE_TRANS = np.array([[0.9, 0.1], [0.2, 0.8]])
T, B, N, SWEEPS, BURN = 150, 8, 256, 200, 50


def simulated_sequence(seed=2024):
    rng = np.random.default_rng(seed)
    x, obs = int(rng.integers(0, 2)), np.zeros(T)
    for t in range(T):
        if t > 0:
            x = int(rng.random() >= TRUE_TRANS[x, 0])
        obs[t] = TRUE_MEANS[x] + rng.standard_normal()
    return obs


def exact_gibbs(obs, means0, trans0, sweeps, rng):
    """Gibbs with exact forward filtering / backward sampling, the chains side by side: a uniform initial state, the forward filter of
    tests/suffstats_ref.py::exact_stats, one backward-sampled path a chain and sweep, its counting statistics, and the same conjugate
    draw (sample_tables, default prior).  Returns (means [sweeps + 1, B, k], trans [sweeps + 1, B, k, k])."""
    means, trans = np.array(means0, np.float64), np.array(trans0, np.float64)
    nb, k = means.shape
    n_steps = len(obs)
    m_hist, t_hist = [means.copy()], [trans.copy()]
    rows = np.arange(nb)
    for _ in range(sweeps):
        A = trans / trans.sum(axis=2, keepdims=True)
        lik = np.exp(exact.normal_logpdf(obs[:, None, None], means[None, :, :], 1.0))            # [T, B, k]
        alpha = np.zeros((n_steps, nb, k))
        a = lik[0] / k
        alpha[0] = a / a.sum(axis=1, keepdims=True)
        for t in range(1, n_steps):
            a = np.einsum("bs,bsj->bj", alpha[t - 1], A) * lik[t]
            alpha[t] = a / a.sum(axis=1, keepdims=True)
        u = rng.random((n_steps, nb))
        x = np.zeros((n_steps, nb), np.int64)
        w = alpha[n_steps - 1]
        for t in range(n_steps - 1, -1, -1):
            if t < n_steps - 1:
                w = alpha[t] * A[rows, :, x[t + 1]]
            c = np.cumsum(w, axis=1)
            x[t] = np.minimum((c < (u[t] * c[:, -1])[:, None]).sum(axis=1), k - 1)
        st = {"xi": np.zeros((nb, 8, 8)), "occ": np.zeros((nb, 8)), "occ_y": np.zeros((nb, 8))}
        for b in range(nb):
            np.add.at(st["xi"][b], (x[:-1, b], x[1:, b]), 1.0)
            st["occ"][b, :k] = np.bincount(x[:, b], minlength=k)
            st["occ_y"][b, :k] = np.bincount(x[:, b], weights=obs, minlength=k)
        means, trans = sample_tables(st, k, rng)
        m_hist.append(means.copy())
        t_hist.append(trans.copy())
    return np.array(m_hist), np.array(t_hist)


def summaries(means, trans, burn=BURN):
    """(chain-averaged posterior means of means[0], means[1], trans[0][0], trans[1][1], their standard errors across chains)."""
    per_chain = np.stack([means[burn + 1:, :, 0].mean(axis=0), means[burn + 1:, :, 1].mean(axis=0),
                          trans[burn + 1:, :, 0, 0].mean(axis=0), trans[burn + 1:, :, 1, 1].mean(axis=0)], axis=1)      # [B, 4]
    return per_chain.mean(axis=0), per_chain.std(axis=0, ddof=1) / np.sqrt(per_chain.shape[0])


def starts():
    return np.tile([-1.0, 1.0], (B, 1)), np.tile(np.full((2, 2), 0.5), (B, 1, 1))


def test_driver_is_the_loop_it_states(engine):
    """hmm_table_gibbs equals begin, run, batch_traj_stats(1, draw_index = sweep), sample_tables written out; the filtering-only
    chain that keeps the masses is the same chain."""
    obs = simulated_sequence()[:40]
    nb, sweeps = 3, 4
    means0 = np.array([[-1.0, 1.0], [-0.5, 0.5], [-3.0, 0.0]])
    trans0 = np.tile(np.full((2, 2), 0.5), (nb, 1, 1))
    seeds = np.array([5, 6, 7], np.uint64)
    got = cp.hmm_table_gibbs(engine, obs, means0, trans0, 128, seeds, sweeps, np.random.default_rng(3), tau0=5.0)
    rng = np.random.default_rng(3)
    means, trans = means0.copy(), trans0.copy()
    m_hist, t_hist, ev = [means.copy()], [trans.copy()], []
    for i in range(sweeps):
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, [obs] * nb, 128, tables=(means, trans))
        engine.batch_run(seeds + np.uint64(i))
        st = engine.batch_traj_stats(1, draw_index=i, observes=[obs] * nb)
        ev.append([s["log_evidence"] for s in engine.batch_results()[0]])
        means, trans = sample_tables({f: v[:, 0] for f, v in st.items()}, 2, rng, tau0=5.0)
        m_hist.append(means.copy())
        t_hist.append(trans.copy())
    assert got[0].shape == (sweeps + 1, nb, 2) and got[1].shape == (sweeps + 1, nb, 2, 2) and got[2].shape == (sweeps, nb)
    assert np.array_equal(got[0], np.array(m_hist)) and np.array_equal(got[1], np.array(t_hist)) and np.array_equal(got[2], np.array(ev))
    assert not np.array_equal(got[0][1], got[0][2])
    kept = cp.hmm_table_gibbs(engine, obs, means0, trans0, 128, seeds, sweeps, np.random.default_rng(3), keep_history=False, tau0=5.0)
    assert all(np.array_equal(x, y) for x, y in zip(got, kept)), "the chain on the masses alone differs from the chain with history"


def test_particle_chain_matches_exact_ffbs_gibbs(engine):
    obs = simulated_sequence()
    means0, trans0 = starts()
    e_means, e_trans = exact_gibbs(obs, means0, trans0, SWEEPS, np.random.default_rng(101))
    p_means, p_trans, ev = cp.hmm_table_gibbs(engine, obs, means0, trans0, N, np.arange(B, dtype=np.uint64) + 900, SWEEPS, np.random.default_rng(202))
    assert np.all(np.isfinite(ev))
    e_avg, e_se = summaries(e_means, e_trans)
    p_avg, p_se = summaries(p_means, p_trans)
    width = 4.0 * np.sqrt(e_se**2 + p_se**2)
    for name, e, p, se_e, se_p, w in zip(("means[0]", "means[1]", "trans[0][0]", "trans[1][1]"), e_avg, p_avg, e_se, p_se, width):
        print("%s: exact %.4f (se %.4f), particle %.4f (se %.4f), difference %.4f, allowed %.4f" % (name, e, se_e, p, se_p, abs(p - e), w))
    assert np.all(np.abs(p_avg - e_avg) <= width), "particle - exact = %s, allowed %s" % (p_avg - e_avg, width)
    # the labels did not switch, and the chains found the levels
    assert np.all(p_means[BURN + 1:, :, 0] < p_means[BURN + 1:, :, 1]) and np.all(e_means[BURN + 1:, :, 0] < e_means[BURN + 1:, :, 1])
    assert abs(e_avg[0] + 2.0) < 0.5 and abs(e_avg[1] - 2.0) < 0.5
