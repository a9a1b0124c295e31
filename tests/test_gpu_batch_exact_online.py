"""Exact streams on the device (cpprob_hip_batch_advance_exact, _advance_learn_exact; csrc/batch_exact.hpp, csrc/batch_exact_learn.hpp):
however a stream is cut it is the one-shot exact run of the lengths reached; the online readers serve it; the fused learning advance is
a host-stepped exact stream under tests/learn_ref.py after every advance; refusals leave the batch on its route.  All array_equal."""
import types

import numpy as np
import pytest

import cpprob_amd as cp
import exact_ref as X
import learn_ref as G
import learn_tied_ref as TR
import scale_ref as S
import test_gpu_batch_exact as E
import test_gpu_batch_learn_scaled as LS
from test_gpu_batch_learn import LOG_NORM, new_masses

pytestmark = pytest.mark.gpu

ESTATE, EUNSUPPORTED = -3, -4
CAPS, REACHED = (37, 5, 22, 9, 31), (37, 0, 20, 9, 30)     # problem 1 never receives an observe
DEAD = {3: 3, 4: 10}                                        # a NaN observe inside a chunk of 5, and on the first step of one


def _feed(obs, reached, chunk, advance, sit_out=2, after=None):
    """Chunks of `chunk` observes up to `reached`; problem sit_out is idle in the second advance."""
    lens, a = [0] * len(obs), 0
    while lens != list(reached):
        dT = [0 if (b == sit_out and a == 1) else min(chunk, reached[b] - lens[b]) for b in range(len(obs))]
        piece = [obs[b][lens[b]:lens[b] + dT[b]] for b in range(len(obs))]
        advance(piece)
        if after:
            after(piece, lens, dT)
        lens, a = [lens[b] + dT[b] for b in range(len(obs))], a + 1


def _online(eng, tables, caps, **kw):
    eng.batch_begin_online(cp.MODEL_HMM_TABLE, list(caps), 8, np.arange(len(caps), dtype=np.uint64) + 5, tables=tables, keep_history=False, keep_masses=True, **kw)


def _state(eng, live=None):
    """What an exact batch holds: per problem the m rows and the step rows, and the evidences."""
    bs = list(range(eng.batch_B) if live is None else live)
    log_z, dead = eng.batch_exact_evidence()
    return [eng.batch_masses(b) for b in bs] + [eng.batch_step_tables(b)[0] for b in bs] + [log_z[bs], dead[bs]]


def _assert_state(a, b, note=""):
    assert len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)), note


@pytest.mark.parametrize("chunk", [1, 5, 37])
@pytest.mark.parametrize("family", ["unit", "scaled", "poisson"])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_resuming_is_invisible(engine, k, family, chunk):
    c = E._case(k, CAPS, family, seed=8)
    obs = [o.copy() for o in c["obs"]]
    for b, t in DEAD.items():
        obs[b][t] = np.nan
    _online(engine, c["tables"], CAPS, emission=c["emission"])
    _feed(obs, REACHED, chunk, engine.batch_advance_exact)
    log_z, dead = engine.batch_exact_evidence()
    assert (log_z[1], dead[1]) == (0.0, -1) and list(dead) == [-1, -1, -1, 3, 10] and list(np.isneginf(log_z)) == [False, False, False, True, True]
    live = [0, 2, 3, 4]
    got = _state(engine, live)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, [obs[b][:REACHED[b]] for b in live], 8, tables=tuple(t[live] for t in c["tables"]), keep_history=False, keep_masses=True,
                                emission=c["emission"])
    engine.batch_run_exact()
    _assert_state(got, _state(engine), "k %d, %s, chunks of %d" % (k, family, chunk))
    if (k, family, chunk) == (3, "unit", 5):                # ... and the restatement itself, where no row is NaN
        for i, b in ((0, 0), (1, 2)):
            m, z, d = X.run(np.asarray(c["ll"][b][:REACHED[b]]).tolist(), c["P"][b])
            assert np.array_equal(got[i], np.array(m)) and got[-2][i] == z and got[-1][i] == d


def test_a_wavefront_of_the_advance_walks_a_second_problem(engine):
    c = E._case(2, (3, 1, 2, 3, 2), "unit", seed=1)
    nb = E.B_TWO_WALKS + 2                                  # kExactGridMax * kWaves + 3
    which = np.arange(nb) % 5
    obs, tables = [c["obs"][i] for i in which], tuple(t[which] for t in c["tables"])
    _online(engine, tables, [len(o) for o in obs])
    _feed(obs, [len(o) for o in obs], 1, engine.batch_advance_exact, sit_out=nb - 1)
    sample = list(range(5)) + list(range(nb - 5, nb))
    got, ev = _state(engine, sample), engine.batch_exact_evidence()
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 8, tables=tables, keep_history=False, keep_masses=True)
    engine.batch_run_exact()
    _assert_state(got, _state(engine, sample))
    assert all(np.array_equal(x, y) for x, y in zip(ev, engine.batch_exact_evidence()))


def test_the_readers_serve_a_stream_however_it_was_cut(engine):
    c, out = E._case(3, (9, 4, 7), "unit", seed=9), []
    for chunk in (1, 9):
        stats = []
        _online(engine, c["tables"], (9, 4, 7))
        _feed(c["obs"], (9, 4, 7), chunk, engine.batch_advance_exact, after=lambda piece, lens, dT: stats.append(engine.batch_online_stats(piece)))
        lag, dec = engine.batch_smooth_lag(2, n_traj=3, draw_index=1), engine.batch_decode_lag(2)
        out.append([lag[0], *lag[1], *dec, engine.batch_predictive(), *(stats[-1][key] for key in sorted(stats[-1]))])
    _assert_state(*out)
    assert out[0][0].any() and out[0][-1].any()


def _learning(eng, k, tables, obs, chunk, t_min, floor, ref, groups=None):
    """The resident exact stream, then the host-stepped one (batch_advance_exact, the reference's learn step, batch_online_tables)."""
    nb, scaled, reached, got = len(obs), len(tables) == 3, [len(o) for o in obs], []
    _online(eng, tables, reached)
    if groups is not None:
        eng.batch_tie(groups)
    eng.batch_learn_begin(LS._gamma(max(reached)), t_min, sigma_floor=floor, tied=groups is not None)
    _feed(obs, reached, chunk, eng.batch_advance_learn_exact,
          after=lambda *a: got.append((_state(eng), [eng.batch_step_tables(b)[1] for b in range(nb)], eng.batch_learn_tables(k, scales=scaled), eng.batch_learn_record())))
    _online(eng, tables, reached)
    it = iter(got)

    def step(piece, lens, dT):
        ref.advance([new_masses(eng, b, k, False, lens[b], lens[b] + dT[b]) for b in range(nb)], piece)
        state, L = _state(eng), ref.learners                # (before the new tables: their words serve the NEXT steps)
        new = tuple(np.stack([getattr(lr, f) for lr in L]) for f in (("means", "trans", "sigmas") if scaled else ("means", "trans")))
        eng.batch_online_tables(new)
        rstate, rthr, rtabs, rrec = next(it)
        _assert_state(rstate, state, "lengths %s" % lens)
        assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(rtabs[:-1], new)), "tables after lengths %s" % lens
        assert np.array_equal(rtabs[-1], [lr.status for lr in L]) and np.array_equal(rrec, np.stack([G.record_array(lr.record) for lr in L]))
        assert all(np.array_equal(rthr[b], L[b].thr) and np.array_equal(eng.batch_step_tables(b)[1], L[b].thr) for b in range(nb))
    _feed(obs, reached, chunk, eng.batch_advance_exact, after=step)


LEARN = [(family, k, chunk, LS.T_MIN) for family in ("unit", "fitted", "kept") for k in (2, 8) for chunk in (1, 5)] + [("unit", 2, 5, LS.T + 1)]


@pytest.mark.parametrize("family,k,chunk,t_min", LEARN, ids=["%s-k%d-chunk%d-tmin%d" % c for c in LEARN])
def test_the_fused_learning_advance_is_the_host_stepped_exact_stream(engine, family, k, chunk, t_min):
    """tests/test_gpu_batch_learn_scaled.py's three streams of 24 steps: problem 2 sits an advance out; problem 1 observes the constant 0.0:
    under the fitted scales its M-steps are refused with bit 8 and its table stays.  t_min = 25: no M-step, the plain exact stream."""
    full = LS._tables(k, 10 + k)
    obs, gamma = LS._observes(full, 20 + k), LS._gamma()
    tables, floor = (full[:2], None) if family == "unit" else (full, LS.FLOOR if family == "fitted" else None)
    L = [G.Learner(full[0][b], full[1][b], k, gamma, t_min, LOG_NORM) if family == "unit" else S.ScaledLearner(full[0][b], full[1][b], full[2][b], k, gamma, t_min, floor)
         for b in range(LS.B)]
    _learning(engine, k, tables, obs, chunk, t_min, floor, types.SimpleNamespace(learners=L, advance=lambda ms, ys: [lr.advance(m, y) for lr, m, y in zip(L, ms, ys)]))
    assert all(lr.changed == 0 for lr in L) if t_min > LS.T else (L[0].changed >= 3 and L[2].changed >= 3)
    assert family != "fitted" or (L[1].status == S.BAD_SCALE and L[1].changed == 0)


def test_the_fused_advance_under_a_tie(engine):
    k, groups, caps = 3, [0, 1, 0, 1], (24, 17, 9, 24)
    gm, gt = LS._tables(k, 33, 2)[:2]
    tables = (gm[groups], gt[groups])
    obs = [tables[0][b][np.random.default_rng(b).integers(0, k, T)] + np.random.default_rng(50 + b).standard_normal(T) for b, T in enumerate(caps)]
    ref = TR.TiedLearner(tables[0], tables[1], k, groups, LS._gamma(), LS.T_MIN, LOG_NORM)
    _learning(engine, k, tables, obs, 5, LS.T_MIN, None, ref, groups=groups)
    assert sum(ref.changed) >= 3 and np.array_equal(ref.learners[0].means, ref.learners[2].means)


MASSES = dict(keep_history=False, keep_masses=True)
REFUSALS = {  # begin keywords, the calls before, the refused call, its code, the call that still serves
    "history": (dict(keep_history=True), [], "batch_advance_exact", ESTATE, "batch_advance"),
    "no-masses": (dict(keep_history=False), [], "batch_advance_exact", ESTATE, "batch_advance"),
    "hmm3": (dict(MASSES, model=cp.MODEL_HMM3), [], "batch_advance_exact", EUNSUPPORTED, "batch_advance"),
    "unarmed": (MASSES, [], "batch_advance_learn_exact", ESTATE, "batch_advance_exact"),
    "armed": (MASSES, ["arm"], "batch_advance_exact", ESTATE, "batch_advance_learn_exact"),
    "particle-then-exact": (MASSES, ["batch_advance"], "batch_advance_exact", ESTATE, "batch_advance"),
    "exact-then-particle": (MASSES, ["batch_advance_exact"], "batch_advance", ESTATE, "batch_advance_exact"),
    "poisson-learner": (dict(MASSES, emission="poisson"), ["arm"], "batch_advance_learn_exact", ESTATE, "batch_advance_exact"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_the_batch_on_its_own_route(engine, case):
    kw, before, refused, code, serves = REFUSALS[case]
    kw = dict(kw)
    model = kw.pop("model", cp.MODEL_HMM_TABLE)
    tables = None if model == cp.MODEL_HMM3 else (np.array([[1.0, 4.0]] * 2), np.array([[[0.7, 0.3], [0.2, 0.8]]] * 2))
    piece = [np.array([1.0]), np.array([2.0, 3.0])]
    engine.batch_begin_online(model, [4, 6], 8, [1, 2], tables=tables, **kw)
    for call in before:
        if call != "arm":
            getattr(engine, call)(piece)
        elif case != "poisson-learner":
            engine.batch_learn_begin(LS._gamma(6), 2)
        else:                                               # the learner refuses a Poisson batch by name: the stream stays un-armed
            with pytest.raises(cp.CpprobHipError, match="Poisson") as e:
                engine.batch_learn_begin(LS._gamma(6), 2)
            assert e.value.code == ESTATE
    lens = list(engine.batch_lengths())
    with pytest.raises(cp.CpprobHipError) as e:
        getattr(engine, refused)(piece)
    assert e.value.code == code and list(engine.batch_lengths()) == lens
    getattr(engine, serves)(piece)
    assert list(engine.batch_lengths()) == [lens[0] + 1, lens[1] + 2]
