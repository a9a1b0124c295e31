"""The buffers of a context's batch state through their whole life: one context begins batch after batch -- every buffer of the state is
used, then outgrown by a larger batch or a larger call, then used again; every ring of pinned descriptor slots wraps, without and
with a growth in between -- and whatever it returns is array_equal to what a fresh context returns that made the last begin and its
calls alone.  Nothing a call leaves behind (a capacity, a ring's count, a watermark, a block a growth replaced) may show in a result.

The device-form calls are made back to back, six of each without a synchronisation in between -- more than a ring has slots --, each
with arguments of its own and an output of its own: a slot written again before its copy has run would hand a call the descriptors of
a later one.  Shapes are the smallest that take every branch: 3 states, at most 40 particles and 9 observes a problem."""
import numpy as np
import pytest

import cpprob_amd as cp
import cpprob_amd.capi as capi
import devmem

pytestmark = pytest.mark.gpu

K = 3
CALLS = 6                                      # back-to-back calls: the rings have 4 slots


def shapes(B):
    b = np.arange(B)
    return 1 + (3 * b + 2) % 9, 8 + (7 * b) % 33            # lengths 1 .. 9, particles 8 .. 40


def tables(B, salt=0):
    rng = np.random.default_rng(100 + 7 * B + salt)
    means = np.sort(rng.normal(0.0, 1.5, (B, K)), axis=1)
    trans = rng.uniform(0.2, 1.0, (B, K, K)) + 2.0 * np.eye(K)
    sigmas = rng.uniform(0.5, 1.5, (B, K))
    return means, trans, sigmas


def observes(B, lengths, salt=0):
    rng = np.random.default_rng(200 + 11 * B + salt)
    return [rng.normal(0.0, 2.0, int(T)) for T in lengths]


def seeds(B, salt=0):
    return np.arange(B, dtype=np.uint64) * 17 + 1000 * B + salt


def results(eng, out, name):
    sums, stats, ess, res = eng.batch_results()
    out[name + " summaries"] = np.array([[s[f] for f in sorted(s)] for s in sums], np.float64)
    out[name + " stats"], out[name + " ess"], out[name + " resampled"] = stats, ess, res


def described(eng, B, n_traj_host):
    """A described batch with a particle store and every call that serves it, then a filtering batch that keeps its masses and a
    conditional run: {name: array}."""
    import torch
    out = {}
    T, n = shapes(B)
    means, trans, _ = tables(B)
    obs = observes(B, T)
    eng.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans))
    eng.batch_run(seeds(B))
    results(eng, out, "run")
    # six traces and six smoothing calls, no synchronisation in between: the particle caps, the trajectory counts and the draws differ
    caps = [0, 3, 5, 1, 7, 2][:CALLS]
    paths = []
    for m in caps:
        first, wfirst = capi.batch_paths_layout(T, n, m)
        paths.append((devmem.dzeros(int(first[-1]), dtype=torch.int8), devmem.dzeros(int(wfirst[-1]), dtype=torch.float64)))
    trajs = [1, 4, 2, 6, 3, 5][:CALLS]
    smooth = [(devmem.dzeros(B, int(T.max()), 8, dtype=torch.float64), devmem.dzeros(int(capi.batch_smooth_layout(T, m)[-1]), dtype=torch.int8)) for m in trajs]
    for m, (p, w) in zip(caps, paths):
        eng.batch_paths_device(p, w, max_particles=m)
    for i, (m, (marg, tr)) in enumerate(zip(trajs, smooth)):
        eng.batch_smooth_device(marginals=marg, traj_i8=tr, n_traj=m, draw_index=i)
    eng.sync()
    for i, (p, w) in enumerate(paths):
        out["paths_device %d" % i], out["paths_device %d logw" % i] = p.cpu().numpy(), w.cpu().numpy()
    for i, (marg, tr) in enumerate(smooth):
        out["smooth_device %d" % i], out["smooth_device %d traj" % i] = marg.cpu().numpy(), tr.cpu().numpy()
    # the host forms: the staging grows with n_traj_host
    marg, tr = eng.batch_smooth(n_traj=n_traj_host, draw_index=7)
    out["smooth"], out["smooth traj"] = marg, np.concatenate([t.reshape(-1) for t in tr])
    p, w = eng.batch_paths()
    out["paths"], out["paths logw"] = np.concatenate([x.reshape(-1) for x in p]), np.concatenate(w)
    path, score = eng.batch_decode()
    out["decode"], out["decode score"] = np.concatenate(path), score
    st = eng.batch_smooth_stats(obs)
    for key in sorted(st):
        out["smooth_stats " + key] = np.array(st[key])
    # a tie and the pooled records
    eng.batch_tie(np.arange(B) % 2)
    rec = np.random.default_rng(300 + B).uniform(0.0, 4.0, (B, 2, 88))
    out["pool_stats"] = eng.batch_pool_stats(rec, per_problem=2)
    out["pool_stats compact"] = eng.batch_pool_stats(rec, per_problem=2, broadcast=False)
    # a re-table with its observes, then one without: the batch stands as after a begin with the new tables
    for salt in (1, 2):
        means2, trans2, _ = tables(B, salt)
        eng.batch_retable((means2, trans2), obs if salt == 1 else None)
        out["retable %d status" % salt] = eng.batch_retable_status()
        eng.batch_run(seeds(B, salt))
        results(eng, out, "retable %d" % salt)
        path, score = eng.batch_decode()
        out["retable %d decode" % salt], out["retable %d score" % salt] = np.concatenate(path), score
    # a filtering batch that keeps its masses: a conditional run from the host's reference paths, then smoothing from the masses
    eng.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans), keep_history=False, keep_masses=True)
    ref = [np.random.default_rng(400 + B + b).integers(0, K, int(T[b])) for b in range(B)]
    eng.batch_run_conditional(seeds(B, 3), ref)
    out["conditional masses"] = np.concatenate([eng.batch_masses(b).reshape(-1) for b in range(B)])
    marg, tr = eng.batch_smooth(n_traj=3, draw_index=1)
    out["conditional smooth"], out["conditional smooth traj"] = marg, np.concatenate([t.reshape(-1) for t in tr])
    return out


def scaled(eng, B):
    """A described batch with emission scales: a run, a scaled re-table, a run."""
    out = {}
    T, n = shapes(B)
    means, trans, sigmas = tables(B)
    obs = observes(B, T)
    eng.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans, sigmas))
    eng.batch_run(seeds(B))
    results(eng, out, "run")
    means2, trans2, sigmas2 = tables(B, 1)
    eng.batch_retable((means2, trans2, sigmas2), obs)
    eng.batch_run(seeds(B, 1))
    results(eng, out, "retable")
    for b in range(B):
        out["scales %d" % b], out["log_norms %d" % b] = eng.batch_scales(b, K)
    return out


def pieces(B, caps, calls, last):
    """`calls` advances of an online batch: [[new observes of problem b]]; the last hands every problem `last` observes."""
    rng = np.random.default_rng(500 + B)
    out, reached = [], np.zeros(B, np.int64)
    for i in range(calls):
        dT = np.full(B, last) if i == calls - 1 else (np.arange(B) + i) % 2
        dT = np.minimum(dT, caps - reached)
        reached += dT
        out.append([rng.normal(0.0, 2.0, int(d)) for d in dT])
    return out


def online(eng, B):
    """An online batch advanced six times back to back, its running statistics; then the batch begun again, armed twice and advanced
    six times by learning advances, the last of which brings more observes than any before it."""
    out = {}
    caps, n = np.full(B, 9), shapes(B)[1]
    means, trans, _ = tables(B)
    eng.batch_begin_online(cp.MODEL_HMM_TABLE, caps, n, seeds(B), tables=(means, trans))
    steps = pieces(B, caps, CALLS, 2)
    for piece in steps:
        eng.batch_advance(piece)
    out["lengths"] = eng.batch_lengths()
    results(eng, out, "advance")
    for b in range(B):
        vals, anc, logw = eng.batch_store(b)
        out["store %d" % b], out["store %d anc" % b], out["store %d logw" % b] = vals, anc, logw
    st = eng.batch_online_stats([np.concatenate([piece[b] for piece in steps]) for b in range(B)])
    for key in sorted(st):
        out["online_stats " + key] = np.array(st[key])
    out["online_stats progress"] = eng.batch_online_stats_progress()
    # the learner: armed twice in a row (the second arming releases what the first allocated)
    eng.batch_begin_online(cp.MODEL_HMM_TABLE, caps, n, seeds(B, 1), tables=(means, trans))
    gamma = 1.0 / (1.0 + np.arange(12))
    eng.batch_learn_begin(0.5 * gamma + 0.5, 1)
    eng.batch_learn_begin(gamma, 2)
    steps = pieces(B, caps, CALLS, 4)
    assert max(sum(len(o) for o in p) for p in steps[:-1]) < sum(len(o) for o in steps[-1])
    for piece in steps:
        eng.batch_advance_learn(piece)
    out["learn lengths"] = eng.batch_lengths()
    out["learn means"], out["learn trans"], out["learn status"] = eng.batch_learn_tables(K)
    out["learn record"] = eng.batch_learn_record()
    results(eng, out, "learn")
    return out


def same(got, want, what):
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert np.array_equal(got[name], want[name]), "%s: %s differs from a fresh context's" % (what, name)


@pytest.fixture(scope="module")
def live():
    """The context that lives through every sequence of this module."""
    import torch  # noqa: F401  (first: shares libamdhip64 with the library)
    eng = cp.Engine(0)
    yield eng
    eng.close()


def fresh(run, *args):
    eng = cp.Engine(0)
    try:
        return run(eng, *args)
    finally:
        eng.close()


def test_described_batches_that_shrink_and_grow_equal_a_fresh_contexts(live):
    # B = 5; B = 2 (nothing grows, the rings' counts carry on); B = 9 (everything grows); the host smoothing's staging grows every time
    for B, n_traj in ((5, 4), (2, 200), (9, 300)):
        same(described(live, B, n_traj), fresh(described, B, n_traj), "described, %d problems" % B)


def test_scaled_batches_that_grow_equal_a_fresh_contexts(live):
    for B in (2, 9):
        same(scaled(live, B), fresh(scaled, B), "scaled, %d problems" % B)


def test_online_batches_that_grow_equal_a_fresh_contexts(live):
    for B in (3, 7):
        same(online(live, B), fresh(online, B), "online, %d problems" % B)


def test_a_described_batch_after_the_online_ones_equals_a_fresh_contexts(live):
    # (the state has held online batches and a learner: their buffers stay with it, and none of them shows)
    same(described(live, 5, 2), fresh(described, 5, 2), "described after online")


def test_a_context_is_destroyed_with_every_buffer_it_grew_and_a_second_one_follows():
    import torch  # noqa: F401
    first = cp.Engine(0)
    got = online(first, 4)
    described(first, 6, 5)
    scaled(first, 3)
    first.close()                              # (every buffer, ring and learner allocation of the state goes here)
    same(got, fresh(online, 4), "the second context")
