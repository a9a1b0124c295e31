"""Tied tables through the fitting loops: cpprob_amd.hmm_table_em(groups=...) on the host route (the records pooled in numpy) and
resident (cpprob_hip_batch_tie once, cpprob_hip_batch_pool_stats_device in place an iteration) against each other and against a loop
written here on tests/pool_ref.py, array_equal; the two Gibbs samplers with groups; and the fit of eight short recordings of one
process against Baum-Welch on their pooled exact statistics."""
import numpy as np
import pytest

import cpprob_amd as cp
from cpprob_amd.em import m_step

import pool_ref as P
import suffstats_ref as S

pytestmark = pytest.mark.gpu

TS = [9, 1, 40, 33, 17, 5]
GROUPS = np.array([0, 1, 0, 2, 1, 0])
NS = [64, 300, 64, 1025, 64, 128]
B, K = len(TS), 3


def _problem(seed, with_sigmas):
    """One table a group, repeated to its members bit for bit; ragged lengths, per-problem particle counts."""
    rng = np.random.default_rng(seed)
    g_means = np.sort(rng.uniform(-3.0, 3.0, (3, K)), axis=1) + 0.5 * np.arange(K)
    g_trans = rng.uniform(0.05, 1.0, (3, K, K))
    g_sig = rng.uniform(0.6, 1.5, (3, K))
    means, trans, sig = g_means[GROUPS], g_trans[GROUPS], g_sig[GROUPS]
    obs = [means[b][rng.integers(0, K, T)] + sig[b][0] * rng.standard_normal(T) for b, T in enumerate(TS)]
    return obs, means, trans, (sig if with_sigmas else None), np.array([11 + 101 * b for b in range(B)], np.uint64)


def _members_equal(arr, groups):
    """arr [iterations + 1, B, ...]: after every iteration a group's members hold the same bits."""
    bits = np.ascontiguousarray(arr).view(np.uint64)
    return all(np.array_equal(bits[:, b], bits[:, m[0]]) for m in P.members(groups) for b in m)


def _loop(engine, obs, means, trans, sigmas, seeds, iterations, resampler, keep_history, groups):
    """hmm_table_em's host route restated on the engine's calls, the records pooled by tests/pool_ref.py."""
    means, trans = means.copy(), trans.copy()
    sigmas = None if sigmas is None else sigmas.copy()
    m_hist, t_hist, s_hist, ev = [means.copy()], [trans.copy()], [None if sigmas is None else sigmas.copy()], np.zeros((iterations, B))
    for it in range(iterations):
        tables = (means, trans) if sigmas is None else (means, trans, sigmas)
        engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, NS, tables=tables, resampler=resampler, keep_history=keep_history, keep_masses=not keep_history)
        engine.batch_run(seeds + np.uint64(it))
        stats = engine.batch_smooth_stats(obs)
        ev[it] = [s["log_evidence"] for s in engine.batch_results()[0]]
        pooled = {name: P.pool(v, groups) for name, v in stats.items()}
        if sigmas is None:
            means, trans = m_step(pooled, means, trans)
        else:
            means, trans, sigmas = m_step(pooled, means, trans, sigmas, 1e-3)
        m_hist.append(means.copy()), t_hist.append(trans.copy()), s_hist.append(None if sigmas is None else sigmas.copy())
    out = (np.array(m_hist), np.array(t_hist), ev)
    return out if sigmas is None else out + (np.array(s_hist),)


def _count(engine, monkeypatch):
    calls = {"batch_begin_problems": 0, "batch_tie": 0, "batch_pool_stats_device": 0, "batch_retable_device": 0}
    for name in calls:
        inner = getattr(engine, name)

        def counted(*a, _inner=inner, _name=name, **kw):
            calls[_name] += 1
            return _inner(*a, **kw)
        monkeypatch.setattr(engine, name, counted, raising=False)
    return calls


@pytest.mark.parametrize("resampler", [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED], ids=["systematic", "stratified"])
@pytest.mark.parametrize("with_sigmas", [False, True], ids=["unit", "scaled"])
@pytest.mark.parametrize("keep_history", [True, False], ids=["history", "masses"])
def test_tied_em_resident_host_and_restated(engine, monkeypatch, keep_history, with_sigmas, resampler):
    obs, means, trans, sigmas, seeds = _problem(5, with_sigmas)
    iters = 3
    want = _loop(engine, obs, means, trans, sigmas, seeds, iters, resampler, keep_history, GROUPS)
    host = cp.hmm_table_em(engine, obs, means, trans, NS, seeds, iters, resampler=resampler, keep_history=keep_history, sigmas0=sigmas, groups=GROUPS)
    calls = _count(engine, monkeypatch)
    res = cp.hmm_table_em(engine, obs, means, trans, NS, seeds, iters, resampler=resampler, keep_history=keep_history, sigmas0=sigmas, groups=GROUPS, resident=True)
    assert calls == {"batch_begin_problems": 1, "batch_tie": 1, "batch_pool_stats_device": iters, "batch_retable_device": iters - 1}
    assert len(want) == len(host) == len(res) == (4 if with_sigmas else 3)
    for w, h, r, what in zip(want, host, res, ("means", "transition", "log_evidence", "sigmas")):
        assert h.shape == w.shape and h.dtype == w.dtype and np.array_equal(h, w), "host: " + what
        assert r.shape == w.shape and r.dtype == w.dtype and np.array_equal(r, w), "resident: " + what
    assert want[0].shape == (iters + 1, B, K) and want[2].shape == (iters, B)
    for arr in (want[0], want[1]) + ((want[3],) if with_sigmas else ()):
        assert _members_equal(arr, GROUPS)
    assert not np.array_equal(want[0][iters], want[0][0]) and not np.array_equal(want[1][iters], want[1][0])
    # the evidences stay per problem, and the tie made a difference: the untied fit of a member is another one
    assert len(set(want[2][0])) == B
    untied = cp.hmm_table_em(engine, obs, means, trans, NS, seeds, iters, resampler=resampler, keep_history=keep_history, sigmas0=sigmas)
    assert not np.array_equal(untied[0][1], want[0][1]) and np.array_equal(untied[2][0], want[2][0])


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
def test_groups_of_one_are_the_untied_fit(engine, resident):
    obs, means, trans, _, seeds = _problem(6, False)
    means = means + 0.01 * np.arange(B)[:, None]
    want = cp.hmm_table_em(engine, obs, means, trans, NS, seeds, 3, resident=resident)
    got = cp.hmm_table_em(engine, obs, means, trans, NS, seeds, 3, resident=resident, groups=np.arange(B)[::-1].copy())
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_gibbs_with_groups(engine, monkeypatch):
    obs, means, trans, _, seeds = _problem(7, False)
    sweeps = 3
    # groups of one: the same chain, the generator consumed alike
    r0, r1 = np.random.default_rng(2), np.random.default_rng(2)
    want = cp.hmm_table_gibbs(engine, obs, means, trans, 64, seeds, sweeps, r0)
    got = cp.hmm_table_gibbs(engine, obs, means, trans, 64, seeds, sweeps, r1, groups=np.arange(B))
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and r0.bit_generator.state == r1.bit_generator.state
    # tied: the members are equal in every sweep, three tables are drawn a sweep, and retable=True gives the same chain
    r2, r3 = np.random.default_rng(4), np.random.default_rng(4)
    shapes, inner = [], cp.gibbs.sample_tables

    def recorded(stats, *a, **kw):
        shapes.append(np.asarray(stats["xi"]).shape)
        return inner(stats, *a, **kw)
    monkeypatch.setattr(cp.gibbs, "sample_tables", recorded)
    tied = cp.hmm_table_gibbs(engine, obs, means, trans, 64, seeds, sweeps, r2, groups=GROUPS)
    monkeypatch.setattr(cp.gibbs, "sample_tables", inner)
    assert shapes == [(3, 8, 8)] * sweeps                   # one call a sweep, on G records
    again = cp.hmm_table_gibbs(engine, obs, means, trans, 64, seeds, sweeps, r3, groups=GROUPS, retable=True)
    assert tied[0].shape == (sweeps + 1, B, K) and tied[2].shape == (sweeps, B)
    assert _members_equal(tied[0], GROUPS) and _members_equal(tied[1], GROUPS) and not np.array_equal(tied[0][sweeps], tied[0][0])
    assert all(np.array_equal(a, t) for a, t in zip(again, tied)) and r2.bit_generator.state == r3.bit_generator.state
    # with emission scales
    _, _, _, sigmas, _ = _problem(7, True)
    scaled = cp.hmm_table_gibbs(engine, obs, means, trans, 64, seeds, sweeps, np.random.default_rng(5), groups=GROUPS, sigmas0=sigmas)
    assert len(scaled) == 4 and all(_members_equal(scaled[i], GROUPS) for i in (0, 1, 3)) and not np.array_equal(scaled[3][sweeps], scaled[3][0])


def test_particle_gibbs_with_groups(engine):
    obs, means, trans, _, seeds = _problem(8, False)
    sweeps = 3
    r0, r1 = np.random.default_rng(3), np.random.default_rng(3)
    want = cp.hmm_table_particle_gibbs(engine, obs, means, trans, 64, seeds, sweeps, r0, alpha=1.5)
    got = cp.hmm_table_particle_gibbs(engine, obs, means, trans, 64, seeds, sweeps, r1, alpha=1.5, groups=np.arange(B))
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and r0.bit_generator.state == r1.bit_generator.state
    r2, r3 = np.random.default_rng(6), np.random.default_rng(6)
    tied = cp.hmm_table_particle_gibbs(engine, obs, means, trans, 64, seeds, sweeps, r2, alpha=1.5, groups=GROUPS)
    again = cp.hmm_table_particle_gibbs(engine, obs, means, trans, 64, seeds, sweeps, r3, alpha=1.5, groups=GROUPS, retable=True)
    assert tied[0].shape == (sweeps + 1, B, K) and _members_equal(tied[0], GROUPS) and _members_equal(tied[1], GROUPS)
    assert not np.array_equal(tied[0][sweeps], tied[0][0])
    assert all(np.array_equal(a, t) for a, t in zip(again, tied)) and r2.bit_generator.state == r3.bit_generator.state


# ---- eight short recordings of one process, one table ----------------------------------------------------------------------------
POOLED_TS = [64, 48, 64, 33, 64, 57, 64, 40]
# twice what the MI355X showed when the bounds were set (0.00247 and 0.00121, profiles/r32_notes.md); one sequence holds 0.05 and 0.02
# (tests/test_gpu_batch_suffstats.py::test_particle_em_tracks_exact_em), and eight sequences' pooled particle errors sit well inside
MEANS_BOUND, TRANS_BOUND = 0.0049, 0.0024


def pooled_case():
    """tests/test_gpu_batch_suffstats.py::em_case's process (means -1.5 / +1.5, self-transition 0.9), eight sequences from one
    generator; the start is means -0.5 / +0.5 and uniform rows."""
    rng = np.random.default_rng(31031)
    true_means = np.array([-1.5, 1.5])
    seqs = []
    for T in POOLED_TS:
        s, obs = int(rng.integers(0, 2)), np.zeros(T)
        for t in range(T):
            if t > 0 and rng.random() >= 0.9:
                s = 1 - s
            obs[t] = true_means[s] + rng.standard_normal()
        seqs.append(obs)
    return seqs, np.array([-0.5, 0.5]), np.full((2, 2), 0.5)


def pooled_exact_em(seqs, means0, trans0, iterations):
    """Baum-Welch on the pooled exact statistics (suffstats_ref.exact_stats, summed over the sequences)."""
    means, trans = np.array(means0, np.float64), np.array(trans0, np.float64)
    ms, ts = [means.copy()], [trans.copy()]
    for _ in range(iterations):
        xi, occ, occ_y = np.zeros((2, 2)), np.zeros(2), np.zeros(2)
        for o in seqs:
            a, b, c, _, _ = S.exact_stats(o, means, trans)
            xi, occ, occ_y = xi + a, occ + b, occ_y + c
        trans, means = xi / xi.sum(axis=1, keepdims=True), occ_y / occ
        ms.append(means.copy()), ts.append(trans.copy())
    return np.array(ms), np.array(ts)


def test_tied_particle_em_tracks_pooled_baum_welch(engine):
    """All eight sequences in one group, n = 256, 10 iterations, seeds 4242 + 1000 b (+ iteration), resident: after every iteration
    the shared table's means are within MEANS_BOUND and its transition entries within TRANS_BOUND of Baum-Welch on the pooled exact
    statistics run alongside; the summed log-evidence rises; and the fitted means lie nearer to -1.5 / +1.5 than the untied fits of
    the same sequences and seeds do on average."""
    seqs, means0, trans0 = pooled_case()
    nB, iters = len(seqs), 10
    bw_means, bw_trans = pooled_exact_em(seqs, means0, trans0, iters)
    assert np.abs(bw_means[-1] - [-1.4995, 1.5315]).max() < 1e-4 and np.abs(np.diag(bw_trans[-1]) - [0.8997, 0.8614]).max() < 1e-4
    seeds = np.array([4242 + 1000 * b for b in range(nB)], np.uint64)
    m0, t0 = np.tile(means0, (nB, 1)), np.tile(trans0, (nB, 1, 1))
    means, trans, ev = cp.hmm_table_em(engine, seqs, m0, t0, 256, seeds, iters, groups=np.zeros(nB, np.int64), resident=True)
    assert means.shape == (iters + 1, nB, 2) and ev.shape == (iters, nB) and _members_equal(means, np.zeros(nB, int)) and _members_equal(trans, np.zeros(nB, int))
    dm = np.abs(means[:, 0] - bw_means).max(axis=1)
    dt = np.abs(trans[:, 0] - bw_trans).max(axis=(1, 2))
    print("tied fit: means off by at most %.5f, transition entries by %.5f; summed log-evidence %.3f -> %.3f; fitted means %s, self-transitions %s"
          % (dm.max(), dt.max(), ev[0].sum(), ev[-1].sum(), means[-1, 0], np.diag(trans[-1, 0])))
    untied = cp.hmm_table_em(engine, seqs, m0, t0, 256, seeds, iters, resident=True)[0][-1]
    truth = np.array([-1.5, 1.5])
    d_tied, d_untied = np.abs(means[-1, 0] - truth).max(), np.abs(untied - truth).max(axis=1).mean()
    print("distance of the fitted means from -1.5 / +1.5: tied %.4f, untied %.4f on average (worst %.4f)" % (d_tied, d_untied, np.abs(untied - truth).max()))
    assert dm.max() <= MEANS_BOUND and dt.max() <= TRANS_BOUND, "means off by %.5f, transition entries by %.5f" % (dm.max(), dt.max())
    assert ev[-1].sum() > ev[0].sum()
    assert d_tied < d_untied
