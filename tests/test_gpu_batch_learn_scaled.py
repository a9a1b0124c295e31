"""Online EM of an online batch with per-state emission scales (include/cpprob_hip.h: cpprob_hip_batch_learn_begin_scaled,
_advance_learn* on a scaled batch, _learn_tables_scaled*; csrc/batch_learn_scaled.hpp) on the device.  The resident scaled stream
against a host-stepped one on a plain scaled online batch -- batch_advance, the m table, tests/learn_ref.py's Learner with the scaled
M-step, check and rows of tests/scale_ref.py, batch_online_tables with the sigmas --, array_equal after every advance.  B = 3 streams
of 24 steps fed in chunks of 1 and 5: problem 2 sits one advance out; problem 1 observes the constant 0.0, so that every state's
variance is 0, its sigma the floor of 1e-160, 2 pi sigma^2 subnormal and every one of its M-steps dropped with bit 8.  Frozen (a
burn-in above every capacity) the stream is the plain scaled online batch; armed by the plain batch_learn_begin it learns means and
transition rows and leaves the sigmas.  The same two routes on tests/test_gpu_batch_learn.py's ragged schedule: seven problems of 1
to 300 particles and ragged capacities, a piece of 40 observes, a problem that never receives an observe."""
import numpy as np
import pytest

import cpprob_amd as cp
import learn_ref as G
import retable_ref as R
import scale_ref as S
from test_gpu_batch_learn import CAPS, NS, SCHEDULE, assert_same, new_masses, snapshot

pytestmark = pytest.mark.gpu

ESTATE, EINVAL = -3, -1
B, T, N, T_MIN, FLOOR = 3, 24, 64, 3, 1e-160


ScaledLearner = S.ScaledLearner


def _seeds(nb=B):
    return np.array([77 + 7919 * b for b in range(nb)], np.uint64)


def _gamma(n=T):
    return (np.arange(n) + 1.0) ** -0.6


def _tables(k, seed, nb=B):
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (nb, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (nb, k, k))
    sigmas = rng.uniform(0.4, 2.0, (nb, k))
    return means, trans, sigmas


def _observes(tables, seed, caps=None):
    """Problem b's observes up to its capacity (caps None: B streams of T steps, problem 1 observing the constant 0.0)."""
    rng = np.random.default_rng(seed)
    k = tables[0].shape[1]
    obs = []
    for b, cap in enumerate([T] * B if caps is None else caps):
        x = rng.integers(0, k, cap)
        obs.append(tables[0][b][x] + tables[2][b][x] * rng.standard_normal(cap))
    if caps is None:
        obs[1] = np.zeros(T)
    return obs


def _schedule(chunk):
    """Advances of `chunk` observes a problem until every problem holds T; problem 2 sits advance 1 out."""
    lens, out = [0] * B, []
    while min(lens) < T:
        dT = [0 if (b == 2 and len(out) == 1) else min(chunk, T - lens[b]) for b in range(B)]
        out.append(dT)
        lens = [lens[b] + dT[b] for b in range(B)]
    return out


def _begin(eng, tables, history, resampler, caps=None, ns=N):
    """caps None: B streams of capacity T; ns: one particle count, or one a problem."""
    caps = [T] * B if caps is None else caps
    eng.batch_begin_online(cp.MODEL_HMM_TABLE, caps, ns, _seeds(len(caps)), tables=tables, resampler=resampler, keep_history=history, keep_masses=not history)


def _resident(eng, k, tables, obs, schedule, history, resampler, t_min, floor, caps=None, ns=N):
    _begin(eng, tables, history, resampler, caps, ns)
    nb = len(obs)
    eng.batch_learn_begin(_gamma(max(len(o) for o in obs)), t_min, sigma_floor=floor)
    lens, out = [0] * nb, []
    for dT in schedule:
        eng.batch_advance_learn([obs[b][lens[b]:lens[b] + dT[b]] for b in range(nb)])
        lens = [lens[b] + dT[b] for b in range(nb)]
        out.append((snapshot(eng, history, not history), eng.batch_learn_tables(k, scales=True), [eng.batch_scales(b, k) for b in range(nb)], eng.batch_learn_record()))
    return out


def _host_stepped(eng, k, tables, obs, schedule, history, resampler, floor, got, caps=None, ns=N):
    _begin(eng, tables, history, resampler, caps, ns)
    B = len(obs)
    learners = [ScaledLearner(tables[0][b], tables[1][b], tables[2][b], k, _gamma(max(len(o) for o in obs)), T_MIN, floor) for b in range(B)]
    lens = [0] * B
    for a, dT in enumerate(schedule):
        piece = [obs[b][lens[b]:lens[b] + dT[b]] for b in range(B)]
        eng.batch_advance(piece)
        for b in range(B):
            learners[b].advance(new_masses(eng, b, k, history, lens[b], lens[b] + dT[b]), piece[b])
        lens = [lens[b] + dT[b] for b in range(B)]
        snap = snapshot(eng, history, not history)              # (before the new tables: their words serve the NEXT steps)
        means, trans, sigmas = (np.stack([getattr(lr, f) for lr in learners]) for f in ("means", "trans", "sigmas"))
        eng.batch_online_tables((means, trans, sigmas))
        note = "advance %d" % a
        rsnap, (m, t, sg, st), scales, rec = got[a]
        for x, y, what in ((m, means, "means"), (t, trans, "transition"), (sg, sigmas, "sigmas")):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), "%s: %s" % (note, what)
        for b in range(B):
            assert np.array_equal(scales[b][0], learners[b].sigmas) and np.array_equal(scales[b][1].view(np.uint64), learners[b].log_norms.view(np.uint64)), note + ": scales"
        assert np.array_equal(st, [lr.status for lr in learners]), note + ": status"
        assert np.array_equal(rec, np.stack([G.record_array(lr.record) for lr in learners])), note + ": record"
        snap["thr"] = tuple(eng.batch_step_tables(b)[1] for b in range(B))
        assert all(np.array_equal(w, lr.thr) for w, lr in zip(snap["thr"], learners)), note + ": words"
        assert_same(rsnap, snap, note)
    return learners


CASES = [(chunk, k, history, resampler) for chunk in (1, 5) for k, history, resampler in
         ((2, True, cp.RESAMPLE_SYSTEMATIC), (3, False, cp.RESAMPLE_STRATIFIED), (8, False, cp.RESAMPLE_SYSTEMATIC), (3, True, cp.RESAMPLE_STRATIFIED))]


@pytest.mark.parametrize("chunk,k,history,resampler", CASES, ids=["chunk%d-k%d-%s-%s" % (c, k, "history" if h else "masses", "strat" if r == cp.RESAMPLE_STRATIFIED else "sys") for c, k, h, r in CASES])
def test_the_resident_scaled_stream_is_the_host_stepped_one(engine, chunk, k, history, resampler):
    tables = _tables(k, 10 + k)
    obs = _observes(tables, 20 + k)
    schedule = _schedule(chunk)
    assert schedule[1][2] == 0 and all(sum(dT[b] for dT in schedule) == T for b in range(B))
    got = _resident(engine, k, tables, obs, schedule, history, resampler, T_MIN, FLOOR)
    learners = _host_stepped(engine, k, tables, obs, schedule, history, resampler, FLOOR, got)
    # problem 1: every M-step dropped with bit 8, its table, sigmas and log_norms those of the begin; the others learned their sigmas
    assert learners[1].status == S.BAD_SCALE and learners[1].changed == 0 and got[-1][1][3][1] == S.BAD_SCALE
    assert np.array_equal(got[-1][1][2][1], tables[2][1]) and np.array_equal(got[-1][1][0][1], tables[0][1])
    assert learners[0].changed >= 3 and learners[2].changed >= 3 and not np.array_equal(got[-1][1][2][0], tables[2][0])


RAGGED = [(k, history, floor) for k in (2, 8) for history in (True, False) for floor in (1e-3, None)]


@pytest.mark.parametrize("k,history,floor", RAGGED, ids=["k%d-%s-%s" % (k, "history" if h else "masses", "floor" if f else "plain") for k, h, f in RAGGED])
def test_the_resident_scaled_stream_on_the_ragged_schedule(engine, k, history, floor):
    """tests/test_gpu_batch_learn.py's CAPS, NS and SCHEDULE under the scaled learner: seven problems (two workgroups of the learn
    kernel) of 1 to 300 particles; a piece of 40 observes, so that the rows kernel's grid is 2; problem 2 never receives an observe
    (the learn kernel's T <= 0 branch), problem 6 receives one and never reaches the burn-in.  floor None: the plain arming on a
    scaled batch.  This is also where the learn kernel's own copy of table_log runs at sigmas nobody chose: every log_norm of every
    advance is held to tests/scale_ref.py's."""
    nb = len(CAPS)
    assert nb == 7 and max(max(dT) for dT in SCHEDULE) == 40 and R.grid_y(40, nb) == 2 and (min(NS), max(NS)) == (1, 300)
    assert all(dT[2] == 0 for dT in SCHEDULE) and sum(dT[6] for dT in SCHEDULE) == 1 < T_MIN
    resampler = cp.RESAMPLE_SYSTEMATIC if history else cp.RESAMPLE_STRATIFIED
    tables = _tables(k, 60 + k, nb)
    obs = _observes(tables, 70 + k, CAPS)
    got = _resident(engine, k, tables, obs, SCHEDULE, history, resampler, T_MIN, floor, CAPS, NS)
    learners = _host_stepped(engine, k, tables, obs, SCHEDULE, history, resampler, floor, got, CAPS, NS)
    for a in range(len(SCHEDULE)):
        _, (m, t, sg, st), scales, rec = got[a]
        assert not rec[2].any() and np.array_equal(m[2], tables[0][2]) and np.array_equal(t[2], tables[1][2]) and np.array_equal(sg[2], tables[2][2]) and st[2] == 0
        assert np.array_equal(scales[2][0], tables[2][2]) and np.array_equal(scales[2][1], [S.log_norm(s) for s in tables[2][2]])
        assert np.array_equal(m[6], tables[0][6]) and np.array_equal(sg[6], tables[2][6])
        if floor is None:
            assert np.array_equal(sg, tables[2]), "advance %d: the sigmas moved" % a
    assert learners[2].changed == 0 and learners[2].done == 0 and learners[6].changed == 0 and learners[6].done == 1
    assert learners[3].changed >= 3 and not np.array_equal(got[-1][1][0][3], tables[0][3])
    assert (floor is None) == np.array_equal(got[-1][1][2][3], tables[2][3])


@pytest.mark.parametrize("history", [True, False], ids=["history", "masses"])
def test_a_frozen_scaled_learning_stream_is_the_plain_scaled_online_batch(engine, history):
    k, schedule = 3, _schedule(5)
    tables = _tables(k, 31)
    obs = _observes(tables, 32)
    got = _resident(engine, k, tables, obs, schedule, history, cp.RESAMPLE_SYSTEMATIC, T + 1, 1e-3)
    _begin(engine, tables, history, cp.RESAMPLE_SYSTEMATIC)
    lens = [0] * B
    for a, dT in enumerate(schedule):
        engine.batch_advance([obs[b][lens[b]:lens[b] + dT[b]] for b in range(B)])
        lens = [lens[b] + dT[b] for b in range(B)]
        assert_same(got[a][0], snapshot(engine, history, not history), "advance %d" % a)
        m, t, sg, st = got[a][1]
        assert np.array_equal(m, tables[0]) and np.array_equal(t, tables[1]) and np.array_equal(sg, tables[2]) and not st.any()


def test_a_plain_learn_begin_on_a_scaled_batch_keeps_the_sigmas(engine):
    k, schedule = 3, _schedule(5)
    tables = _tables(k, 41)
    obs = _observes(tables, 42)
    got = _resident(engine, k, tables, obs, schedule, False, cp.RESAMPLE_SYSTEMATIC, T_MIN, None)
    learners = _host_stepped(engine, k, tables, obs, schedule, False, cp.RESAMPLE_SYSTEMATIC, None, got)
    for a in range(len(schedule)):
        assert np.array_equal(got[a][1][2], tables[2]), "advance %d: the sigmas moved" % a
    assert all(lr.changed >= 3 for lr in learners) and not np.array_equal(got[-1][1][0], tables[0])


def test_scaled_learning_refusals_and_the_device_copy(engine):
    import torch
    k = 2
    tables = _tables(k, 51)
    obs = _observes(tables, 52)
    _begin(engine, tables[:2], False, cp.RESAMPLE_SYSTEMATIC)             # a unit batch
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_learn_begin(_gamma(), T_MIN, sigma_floor=1e-3)
    assert e.value.code == ESTATE
    engine.batch_learn_begin(_gamma(), T_MIN)
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_learn_tables(k, scales=True)
    assert e.value.code == ESTATE
    _begin(engine, tables, False, cp.RESAMPLE_SYSTEMATIC)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(cp.CpprobHipError) as e:
            engine.batch_learn_begin(_gamma(), T_MIN, sigma_floor=bad)
        assert e.value.code == EINVAL
    engine.batch_learn_begin(_gamma(), T_MIN, sigma_floor=1e-3)
    engine.batch_advance_learn([o[:7] for o in obs])
    m, t, sg, st = engine.batch_learn_tables(k, scales=True)
    d = [torch.zeros(s, dtype=torch.float64, device="cuda:0") for s in ((B, k), (B, k, k), (B, k))]
    torch.cuda.synchronize()
    engine.batch_learn_tables_device(d[0], d[1], sigmas=d[2])
    engine.sync()
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(d, (m, t, sg)))
    # the host route on the armed scaled batch replaces the device tables and scales
    engine.batch_online_tables(tables)
    m, t, sg, _ = engine.batch_learn_tables(k, scales=True)
    assert np.array_equal(m, tables[0]) and np.array_equal(t, tables[1]) and np.array_equal(sg, tables[2])


# ---- it recovers the scales ----------------------------------------------------------------------------------------------------------
LAW_B, LAW_T, LAW_N, LAW_CHUNK, LAW_TMIN, LAW_FLOOR = 16, 512, 256, 8, 32, 1e-3
TRUE_MEANS, TRUE_SIGMAS, TRUE_TRANS = np.array([-2.0, 2.0]), np.array([0.5, 2.0]), np.array([[0.8, 0.2], [0.2, 0.8]])
START_MEANS, START_SIGMAS, START_TRANS = np.array([-0.5, 0.5]), np.array([1.0, 1.0]), np.array([[0.6, 0.4], [0.4, 0.6]])
# The largest distance, over the 16 streams and the two states, of the device's final sigmas from the same recursion under the exact
# filter, measured on an MI355X (profiles/r29_notes.md): max 0.0231, median 0.0050 (the reference itself ends 0.36 from the truth after
# 512 steps, the start is 1.0 from it); the bound is LAW_FACTOR = 3 times the measured value.
LAW_SPREAD_SIGMAS, LAW_FACTOR = 0.0231, 3.0


def exact_scaled_online_em(y, means, sigmas, trans, gamma, chunk, t_min, floor):
    """The recursion of csrc/batch_learn_scaled.hpp with the exact filter in place of the particles' masses (test_gpu_batch_learn's
    exact_online_em with the emission's sigma a state's own and fitted)."""
    k = len(means)
    means, sigmas, trans = np.array(means, np.float64), np.array(sigmas, np.float64), np.array(trans, np.float64)
    tau, phi = np.zeros((k, 88)), None
    for t, yt in enumerate(y):
        g = gamma[t]
        q = trans / trans.sum(1, keepdims=True)
        lik = np.exp(-0.5 * ((yt - means) / sigmas) ** 2) / sigmas
        new = np.zeros((k, 88))
        if t == 0:
            nphi = lik / lik.sum()
        else:
            a = phi[:, None] * q
            w = a / a.sum(0, keepdims=True)
            for sn in range(k):
                v = ((1.0 - g) * tau).copy()
                for s in range(k):
                    v[s, 8 * s + sn] += g
                new[sn] = w[:, sn] @ v
            nphi = a.sum(0) * lik
            nphi /= nphi.sum()
        for sn in range(k):
            new[sn, 64 + sn] += g
            new[sn, 72 + sn] += g * yt
            new[sn, 80 + sn] += g * yt * yt
        tau, phi = new, nphi
        L = t + 1
        if L % chunk == 0 and L >= t_min:
            rec = phi @ tau
            for s in range(k):
                row = rec[8 * s:8 * s + k].sum()
                if row > 0:
                    trans[s] = rec[8 * s:8 * s + k] / row
                if rec[64 + s] > 0:
                    means[s] = rec[72 + s] / rec[64 + s]
                    v = rec[80 + s] / rec[64 + s] - means[s] * means[s]
                    sigmas[s] = np.sqrt(v) if v >= floor * floor else floor
    return means, sigmas, trans


def test_it_recovers_the_scales(engine):
    rng = np.random.default_rng(2029)
    obs = []
    for _ in range(LAW_B):
        x = np.zeros(LAW_T, int)
        x[0] = rng.integers(0, 2)
        for t in range(1, LAW_T):
            x[t] = x[t - 1] if rng.random() < TRUE_TRANS[0, 0] else 1 - x[t - 1]
        obs.append(TRUE_MEANS[x] + TRUE_SIGMAS[x] * rng.standard_normal(LAW_T))
    tables0 = (np.tile(START_MEANS, (LAW_B, 1)), np.tile(START_TRANS, (LAW_B, 1, 1)), np.tile(START_SIGMAS, (LAW_B, 1)))
    seeds = np.array([5 + 7919 * b for b in range(LAW_B)], np.uint64)
    m, t, st, sums, sg = cp.hmm_table_online_em(engine, obs, tables0, LAW_N, seeds, LAW_CHUNK, step_exponent=0.6, t_min=LAW_TMIN, sigma_floor=LAW_FLOOR)
    assert sg.shape == (LAW_T // LAW_CHUNK + 1, LAW_B, 2) and np.array_equal(sg[0], tables0[2]) and not st.any()
    gamma = cp.online_em.step_sizes(LAW_T, 0.6)
    ref = [exact_scaled_online_em(obs[b], START_MEANS, START_SIGMAS, START_TRANS, gamma, LAW_CHUNK, LAW_TMIN, LAW_FLOOR) for b in range(LAW_B)]
    ds = np.array([np.abs(sg[-1, b] - ref[b][1]).max() for b in range(LAW_B)])
    print("it recovers the scales: distance of the final sigmas to the CPU reference over the %d streams: max %.4f median %.4f; the reference's distance "
          "to the truth: max %.4f; the start's: %.4f" % (LAW_B, ds.max(), np.median(ds), max(np.abs(r[1] - TRUE_SIGMAS).max() for r in ref), np.abs(START_SIGMAS - TRUE_SIGMAS).max()))
    assert ds.max() <= LAW_FACTOR * LAW_SPREAD_SIGMAS
