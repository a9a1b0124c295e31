"""Exact filter runs of a batch on the device (include/cpprob_hip.h: cpprob_hip_batch_run_exact, csrc/batch_exact.hpp): the m table,
the evidences and the dead steps equal tests/exact_ref.py's bit for bit; the readers serve the run as their Python references serve
the restated table; the refusals and what the run leaves of the runs around it; and hmm_table_em(exact=True).
(No entry point reads rows t >= T_b of the m table, so that they stay untouched is the kernel's loop bound and not tested here.)"""
import functools

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import decode_ref as D
import exact_ref as X
import forecast_ref as F
import poisson_ref as PR
import scale_ref as S
import suffstats_ref as SS
import trajstats_ref as TS
from test_exact_ref_host import TOL_LOG_Z, TOL_SMOOTH

pytestmark = pytest.mark.gpu

ESTATE, EUNSUPPORTED = -3, -4
B_TWO_WALKS = 4 * 2048 + 1                                  # kWaves * kExactGridMax + 1: the first wavefront walks a second problem


@functools.lru_cache(maxsize=None)
def _case(k, Ts, family, seed=0):
    """A described batch: observes, tables, the emission keyword, and per problem the rows ll [T][k] and the integers P."""
    rng = np.random.default_rng(100 * k + seed)
    nb = len(Ts)
    trans = rng.uniform(0.05, 1.0, (nb, k, k))
    par = np.sort(rng.uniform(1.0, 9.0, (nb, k)), axis=1) if family == "poisson" else np.sort(rng.uniform(-3.0, 3.0, (nb, k)), axis=1)
    x = [rng.integers(0, k, T) for T in Ts]
    if family == "poisson":
        obs = [rng.poisson(par[b][x[b]]).astype(np.float64) for b in range(nb)]
        tables, ll = (par, trans), [PR.rows(obs[b], par[b], k)[:, :k] for b in range(nb)]
    else:
        obs = [par[b][x[b]] + rng.standard_normal(Ts[b]) for b in range(nb)]
        sig = rng.uniform(0.5, 2.0, (nb, k))
        tables = (par, trans, sig) if family == "scaled" else (par, trans)
        ll = [S.rows(obs[b], par[b], sig[b], k)[:, :k] if family == "scaled" else np.array(R.log_likelihoods(obs[b], par[b])) for b in range(nb)]
    return {"obs": obs, "tables": tables, "emission": "poisson" if family == "poisson" else "normal", "ll": ll, "P": [R.transition_masses(t) for t in trans], "k": k}


def _begin(engine, c, n=8):
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, c["obs"], n, tables=c["tables"], keep_history=False, keep_masses=True, emission=c["emission"])


def _refs(c):
    return [X.run(np.asarray(ll).tolist(), P) for ll, P in zip(c["ll"], c["P"])]


def _assert_run(engine, refs, which=None):
    """The device's rows, evidences and dead steps against refs[which[b]] (which None: refs[b])."""
    log_z, dead = engine.batch_exact_evidence()
    for b in range(engine.batch_B):
        m, z, d = refs[b if which is None else which[b]]
        assert np.array_equal(engine.batch_masses(b), np.array(m)), "problem %d: rows differ" % b
        assert np.array_equal(log_z[b], z) and dead[b] == d, "problem %d: log_z %r (%r), dead %d (%d)" % (b, log_z[b], z, dead[b], d)


@pytest.mark.parametrize("family", ["unit", "scaled", "poisson"])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_described_ragged_batches_equal_the_restatement(engine, k, family):
    c = _case(k, (1, 2, 37), family)
    _begin(engine, c)
    engine.batch_run_exact()
    _assert_run(engine, _refs(c))


def test_a_wavefront_that_walks_two_problems_and_a_shared_table(engine):
    c = _case(2, (3, 1, 2, 3, 2), "unit", seed=1)
    which = np.arange(B_TWO_WALKS) % 5
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, [c["obs"][i] for i in which], 4, tables=tuple(t[which] for t in c["tables"]), keep_history=False, keep_masses=True)
    engine.batch_run_exact()
    _assert_run(engine, _refs(c), which)
    u = _case(3, (9, 9), "unit", seed=2)                    # a uniform batch: both problems under problem 0's table
    engine.set_hmm(u["tables"][0][0], u["tables"][1][0])
    engine.batch_begin(cp.MODEL_HMM_TABLE, np.array(u["obs"]), 16, keep_history=False, keep_masses=True)
    engine.batch_run_exact()
    _assert_run(engine, [X.run(np.array(R.log_likelihoods(o, u["tables"][0][0])).tolist(), u["P"][0]) for o in u["obs"]])


def test_edges_of_the_statement(engine):
    """k = 3, three problems: state 2 unreachable after step 0 under observes that make it the likeliest; an infinite observe at step 2
    of 6; a state 30 nats below the rest (weight 0)."""
    means = np.array([[-1.0, 0.0, 1.0], [-1.0, 0.0, 1.0], [0.0, 0.5, 8.0]])
    trans = np.array([[[0.7, 0.3, 0.0], [0.4, 0.6, 0.0], [0.5, 0.5, 0.0]], [[0.5, 0.3, 0.2]] * 3, [[0.5, 0.3, 0.2]] * 3])
    obs = [np.array([1.0, 1.1, 0.9, 1.2, 1.0]), np.array([0.1, -0.4, np.inf, 0.3, 0.2, 0.0]), np.array([0.0, 8.0, 0.25, 4.0])]
    ll = [np.array(R.log_likelihoods(o, m)) for o, m in zip(obs, means)]
    assert ll[0][1].argmax() == 2 and ll[2][0][2] < ll[2][0].max() - 30.0
    refs = [X.run(l.tolist(), R.transition_masses(t)) for l, t in zip(ll, trans)]
    assert [r[2] for r in refs] == [-1, 2, -1] and refs[1][1] == -np.inf and refs[0][0][1][2] == 0.0 and refs[2][0][0][2] == 0.0
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 8, tables=(means, trans), keep_history=False, keep_masses=True)
    engine.batch_run_exact()
    _assert_run(engine, refs)
    got = engine.batch_masses(1)
    assert not got[2:].any() and got[:2, :3].all() and not got[:, 3:].any()


@pytest.mark.parametrize("reader", ["smooth_stats", "smooth", "traj_stats", "decode", "predictive"])
def test_the_readers_serve_an_exact_run_unchanged(engine, reader):
    c = _case(3, (1, 2, 9), "unit", seed=3)
    seeds = np.array([11, 12, 13], np.uint64)
    _begin(engine, c)
    engine.batch_run(seeds)                                 # (the backward draws' keys; the exact run overwrites its rows)
    engine.batch_run_exact()
    ms = [[[int(v) for v in row[:3]] for row in r[0]] for r in _refs(c)]
    out = {"smooth_stats": lambda: engine.batch_smooth_stats(c["obs"]), "smooth": lambda: engine.batch_smooth(5, draw_index=2), "traj_stats": lambda: engine.batch_traj_stats(5, 2, c["obs"]),
           "decode": engine.batch_decode, "predictive": engine.batch_predictive}[reader]()
    for b, (m, P, o, ll) in enumerate(zip(ms, c["P"], c["obs"], c["ll"])):
        T, traj = len(m), R.trajectories(m, P, int(seeds[b]), 5, draw_index=2)
        if reader == "smooth_stats":
            assert all(np.array_equal(out[name][b], SS.stats(m, P, o)[name]) for name in ("xi", "occ", "occ_y", "occ_yy"))
        elif reader == "smooth":
            assert np.array_equal(out[0][b, :T, :3], R.marginals(m, P)) and np.array_equal(out[1][b], traj)
        elif reader == "traj_stats":
            want = cp.capi.split_traj_stats(TS.records(traj, o)[None])
            assert all(np.array_equal(out[name][b], want[name][0]) for name in want)
        elif reader == "decode":
            path, score = D.decode(m, ll, *D.log_table(P))
            assert np.array_equal(out[0][b], path) and out[1][b] == score
        else:
            assert np.array_equal(out[b, :T + 1, :3], F.predictive(m, P))


def test_refusals_and_what_the_run_leaves(engine):
    import torch
    c = _case(3, (4, 6), "unit", seed=4)
    rc = lambda e: e.L.cpprob_hip_batch_run_exact(e.h)      # noqa: E731
    fresh = cp.Engine(0)
    try:
        assert rc(fresh) == ESTATE                          # no batch begun
        fresh.batch_begin_online(cp.MODEL_HMM_TABLE, [4, 6], 8, [1, 2], tables=c["tables"], keep_history=False, keep_masses=True)
        assert rc(fresh) == EUNSUPPORTED
        fresh.batch_begin(cp.MODEL_HMM3, np.zeros((2, 4)), 8, keep_history=False, keep_masses=True)
        assert rc(fresh) == EUNSUPPORTED
    finally:
        fresh.close()
    seeds = np.array([5, 6], np.uint64)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, c["obs"], 8, tables=c["tables"])      # keep_history = 1
    engine.batch_run(seeds)
    before = engine.batch_results()
    assert rc(engine) == ESTATE and b"keep_history = 0" in engine.L.cpprob_hip_last_error(engine.h)
    after = engine.batch_results()                          # nothing was written, and the results still serve
    assert before[0] == after[0] and all(np.array_equal(x, y) for x, y in zip(before[1:], after[1:]))
    _begin(engine, c)
    engine.batch_run(seeds)
    want = engine.batch_results(), [engine.batch_masses(b) for b in range(2)]
    engine.batch_run_exact()
    for call in (engine.batch_results, lambda: engine.batch_summaries_device(torch.zeros(8, dtype=torch.float64, device="cuda:0"))):
        with pytest.raises(cp.capi.CpprobHipError, match="an exact run keeps masses"):
            call()
    engine.batch_run(seeds)                                 # ... and a run after it is the run on a fresh begin
    got = engine.batch_results(), [engine.batch_masses(b) for b in range(2)]
    assert want[0][0] == got[0][0] and all(np.array_equal(x, y) for x, y in zip(want[0][1:] + tuple(want[1]), got[0][1:] + tuple(got[1])))
    with pytest.raises(cp.capi.CpprobHipError, match="has not been the batch's last run"):
        engine.batch_exact_evidence()
    new = _case(3, (4, 6), "unit", seed=5)                  # a re-table, then an exact run: the run of a batch begun with the new tables
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (new["tables"][0], new["tables"][1], np.concatenate(c["obs"]))]
    torch.cuda.synchronize()
    engine.batch_retable_device(*dev)
    engine.batch_run_exact()
    _assert_run(engine, [X.run(np.array(R.log_likelihoods(o, m)).tolist(), P) for o, m, P in zip(c["obs"], new["tables"][0], new["P"])])


@pytest.mark.parametrize("family,tied", [("unit", False), ("scaled", False), ("poisson", False), ("unit", True)])
def test_exact_em_host_loop_and_resident_agree(engine, family, tied):
    c = _case(2, (12, 9, 12, 9), family, seed=6)
    t = [np.repeat(a[:2], 2, axis=0) for a in c["tables"]] if tied else list(c["tables"])
    kw = dict(keep_history=False, exact=True, emission=c["emission"], sigmas0=t[2] if family == "scaled" else None, groups=np.array([0, 0, 1, 1]) if tied else None)
    host = cp.hmm_table_em(engine, c["obs"], t[0], t[1], 8, np.arange(4), 3, **kw)
    res = cp.hmm_table_em(engine, c["obs"], t[0], t[1], 8, np.arange(4), 3, resident=True, **kw)
    assert len(host) == len(res) and all(np.array_equal(x, y) for x, y in zip(host, res)) and np.isfinite(host[2]).all()


def test_exact_em_is_baum_welch_and_the_default_stays(engine):
    c = _case(2, (14, 11), "unit", seed=7)
    means0, trans0 = c["tables"]
    means, trans, ev = cp.hmm_table_em(engine, c["obs"], means0, trans0, 8, [1, 2], 3, keep_history=False, exact=True)
    for b in range(2):
        want_m, want_t = SS.exact_em(c["obs"][b], means0[b], trans0[b], 3)
        print("problem %d: means %.3g, transition rows %.3g" % (b, np.abs(means[:, b] - want_m).max(), np.abs(trans[1:, b] - want_t[1:]).max()))
        assert np.abs(means[:, b] - want_m).max() <= 3 * TOL_SMOOTH and np.abs(trans[1:, b] - want_t[1:]).max() <= 3 * TOL_SMOOTH
        assert abs(ev[0, b] - SS.exact_stats(c["obs"][b], means0[b], trans0[b])[4]) <= TOL_LOG_Z
    # exact=False: the particle loop's own calls, as before
    got = cp.hmm_table_em(engine, c["obs"], means0, trans0, 64, [1, 2], 1, keep_history=False)
    _begin(engine, c, 64)
    engine.batch_run(np.array([1, 2], np.uint64))
    m1, t1 = cp.em.m_step(engine.batch_smooth_stats(c["obs"]), means0, trans0)
    assert np.array_equal(got[0][1], m1) and np.array_equal(got[1][1], t1) and np.array_equal(got[2][0], [s["log_evidence"] for s in engine.batch_results()[0]])
