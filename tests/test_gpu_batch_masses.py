"""Filtering-only batches that keep the backward smoother's masses (include/cpprob_hip.h: CPPROB_HIP_BATCH_KEEP_MASSES,
cpprob_hip_batch_copy_masses): batch_smc_kernel writes the row m_t[0..8) of every generation where its counts stand, and
cpprob_hip_batch_smooth*, _smooth_lag* and _smooth_stats* serve the batch from those rows without a counting launch, a particle
store or ancestors.

The oracle throughout is the TWIN: the same batch begun with keep_history=True and the same seeds on a second context.  Its store,
through tests/backward_ref.py, tests/lag_ref.py and tests/suffstats_ref.py, is tied to the references by the tests of the smoothing
calls themselves; here everything is array_equal to the twin -- the rows to backward_ref.filtering_masses of the twin's store (what
batch_smooth_count_kernel derives from it), every smoothing result to the twin's own, bit for bit, since the kernels behind the calls
are the same and read the same table."""
import ctypes as C

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
from oracle import exact
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
RESAMPLERS = [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED]
GAP_LIMIT = 6.0                                # kFixGapLimit


@pytest.fixture(scope="module")
def twin():
    """A second context: the keep_history=True batch beside the one under test (a begin on `engine` would replace it)."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _seeds(nb, base=77):
    return np.array([base + 7919 * b for b in range(nb)], np.uint64)


def _tables(k, nb, seed):
    """tests/test_gpu_batch_problems.py::_tables: table 1 has a zero transition entry."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (nb, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (nb, k, k))
    if nb > 1:
        trans[1, 0, k - 1] = 0.0
    return means, trans


def _table_observes(means, Ts, seed):
    rng = np.random.default_rng(seed)
    k = means.shape[1]
    return [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]


def _store_masses(eng, b, obs_b, means):
    """[T_b, 8]: filtering_masses of the rows problem b's keep_history=True run left, states >= k zero."""
    vals = eng.batch_store(b)[0]
    out = np.zeros((vals.shape[0], 8))
    if vals.shape[0]:
        m = np.array(R.filtering_masses(vals, R.log_likelihoods(obs_b[:vals.shape[0]], means)), np.float64)
        out[:, :m.shape[1]] = m
    return out


def _assert_masses(engine, twin, obs, means_of, what=""):
    for b in range(engine.batch_B):
        got, want = engine.batch_masses(b), _store_masses(twin, b, obs[b], means_of(b))
        assert got.shape == want.shape and got.dtype == np.float64, (what, b, got.shape, want.shape)
        assert np.array_equal(got, want), "%sproblem %d: the kept rows differ from the masses of the twin's store at steps %s" % (
            what, b, np.nonzero((got != want).any(axis=1))[0][:8].tolist())


def _same_results(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


# ---- 1. the rows -----------------------------------------------------------------------------------------------------------------
MODELS = [("hmm3", 3), ("table", 2), ("table", 3), ("table", 5), ("table", 8)]


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("model,k", MODELS)
def test_uniform_batches_keep_the_masses_of_the_twins_store(engine, twin, model, k, rs):
    """n: one particle, one lane's run short, one wavefront, a tile and a lane more, a second pass's first lanes, the LDS limit;
    T: no resampling at all (the final books alone), one resampling, many."""
    B = 3
    hmm3 = model == "hmm3"
    mid = cp.MODEL_HMM3 if hmm3 else cp.MODEL_HMM_TABLE
    if hmm3:
        means = np.array(exact.HMM_MEAN)
    else:
        mt, tt = _tables(k, 1, 50 + k)
        means = mt[0]
        engine.set_hmm(means, tt[0])
        twin.set_hmm(means, tt[0])
    for T in (1, 2, 17):
        obs = [exact.simulate_hmm(T, 300 + b) for b in range(B)] if hmm3 else _table_observes(np.repeat(means[None], B, 0), [T] * B, 300 + T)
        plain = None
        for n in (1, 3, 64, 257, 1027, 8192):
            seeds = _seeds(B, 5 + n + T)
            engine.batch_begin(mid, np.array(obs), n, resampler=rs, keep_history=False, keep_masses=True)
            engine.batch_run(seeds)
            twin.batch_begin(mid, np.array(obs), n, resampler=rs)
            twin.batch_run(seeds)
            _assert_masses(engine, twin, obs, lambda b: means, "T = %d, n = %d, " % (T, n))
            with_rows = engine.batch_results()
            if n in (3, 1027):                                   # the filtering results are those of the batch without the bit
                engine.batch_begin(mid, np.array(obs), n, resampler=rs, keep_history=False)
                engine.batch_run(seeds)
                plain = engine.batch_results()
                assert _same_results(with_rows, plain), "T = %d, n = %d: the filtering results changed with the bit" % (T, n)
        assert plain is not None


def _ragged(model, k):
    Ts, ns = [1, 2, 7, 16], [1, 5, 300, 1500]
    if model == "hmm3":
        return Ts, ns, None, None, [exact.simulate_hmm(T, 70 + b) for b, T in enumerate(Ts)]
    means, trans = _tables(k, len(Ts), 90 + k)
    return Ts, ns, means, trans, _table_observes(means, Ts, 90 + k)


def _begin_ragged(eng, model, obs, ns, means, trans, rs, **kw):
    if model == "hmm3":
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, ns, resampler=rs, **kw)
    else:
        eng.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans), resampler=rs, **kw)


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("model,k", [("hmm3", 3), ("table", 5)])
def test_described_ragged_batch(engine, twin, model, k, rs):
    """Lengths {1, 2, 7, 16} with particle counts {1, 5, 300, 1500}: rows past a problem's length are never written or read."""
    Ts, ns, means, trans, obs = _ragged(model, k)
    seeds = _seeds(len(Ts), 23)
    _begin_ragged(engine, model, obs, ns, means, trans, rs, keep_history=False, keep_masses=True)
    engine.batch_run(seeds)
    _begin_ragged(twin, model, obs, ns, means, trans, rs)
    twin.batch_run(seeds)
    _assert_masses(engine, twin, obs, lambda b: exact.HMM_MEAN if model == "hmm3" else means[b])
    assert [engine.batch_masses(b).shape for b in range(4)] == [(T, 8) for T in Ts]
    with_rows = engine.batch_results()
    _begin_ragged(engine, model, obs, ns, means, trans, rs, keep_history=False)
    engine.batch_run(seeds)
    assert _same_results(with_rows, engine.batch_results())


# ---- 2. the smoothing calls --------------------------------------------------------------------------------------------------------
def _assert_smoothing_equals_the_twins(engine, twin, obs, Ts, what=""):
    """Every smoothing call on the batch with masses returns the twin's bits, and none of them launches the counting pass."""
    B, T_max = len(Ts), max(Ts)

    def same(got, want, call):
        assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), "%s%s: the marginals differ from the twin's" % (what, call)
        assert len(got[1]) == len(want[1]) == B
        for b in range(B):
            assert got[1][b].shape == want[1][b].shape and np.array_equal(got[1][b], want[1][b]), "%s%s: problem %d's trajectories differ from the twin's" % (what, call, b)
        assert engine.batch_smooth_grid()[0] == 0, "%s%s: a counting launch on a batch that keeps its masses" % (what, call)

    for M, di in ((1, 0), (5, 0), (1025, 0), (5, 3), (0, 0)):
        same(engine.batch_smooth(M, di), twin.batch_smooth(M, di), "smooth(%d, %d)" % (M, di))
        assert twin.batch_smooth_grid()[0] > 0                   # (the twin counts: the assertion above is not vacuous)
    frm = [min(T, b % 3) for b, T in enumerate(Ts)]
    for lag in (0, 1, 3, T_max, T_max + 5):
        for f in (None, frm):
            for M in (0, 5):
                same(engine.batch_smooth_lag(lag, f, M, 2), twin.batch_smooth_lag(lag, f, M, 2), "smooth_lag(%d, %s, %d)" % (lag, f, M))
    for o in (obs, None):
        got, want = engine.batch_smooth_stats(o), twin.batch_smooth_stats(o)
        assert all(np.array_equal(got[f], want[f]) for f in ("xi", "occ", "occ_y", "occ_yy")), "%sthe statistics differ from the twin's" % what
        assert engine.batch_smooth_grid() == (0, 0)
        assert np.any(got["occ_y"] != 0.0) == (o is not None)


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("model,k", [("hmm3", 3), ("table", 5)])
def test_smoothing_of_a_ragged_batch_equals_the_twins(engine, twin, model, k, rs):
    Ts, ns, means, trans, obs = _ragged(model, k)
    seeds = _seeds(len(Ts), 29)
    _begin_ragged(engine, model, obs, ns, means, trans, rs, keep_history=False, keep_masses=True)
    engine.batch_run(seeds)
    _begin_ragged(twin, model, obs, ns, means, trans, rs)
    twin.batch_run(seeds)
    before = engine.batch_results()
    _assert_smoothing_equals_the_twins(engine, twin, obs, Ts)
    assert _same_results(before, engine.batch_results())         # the smoothing calls change nothing the run left
    _assert_masses(engine, twin, obs, lambda b: exact.HMM_MEAN if model == "hmm3" else means[b], "after the smoothing calls, ")


def test_smoothing_of_a_uniform_batch_and_the_device_variants(engine, twin):
    """A uniform HMM3 batch (its m table is addressed by T, no descriptors in the run), then each _device variant once, behind guard
    bands, against the twin's host results."""
    import torch
    B, T, n, M, di, lag = 5, 17, 257, 33, 1, 3
    obs = [exact.simulate_hmm(T, 500 + b) for b in range(B)]
    seeds = _seeds(B, 31)
    engine.batch_begin(cp.MODEL_HMM3, np.array(obs), n, keep_history=False, keep_masses=True)
    engine.batch_run(seeds)
    twin.batch_begin(cp.MODEL_HMM3, np.array(obs), n)
    twin.batch_run(seeds)
    _assert_smoothing_equals_the_twins(engine, twin, np.array(obs), [T] * B)
    pad = 256

    def guarded(n_items, dtype, fill):
        return torch.full((n_items + 2 * pad,), fill, dtype=dtype, device="cuda:0")

    def inner(t, n_items, fill):
        a = t.cpu().numpy()
        assert np.all(a[:pad] == fill) and np.all(a[pad + n_items:] == fill), "a write outside the buffer"
        return a[pad:pad + n_items]

    # the full call
    want_m, want_x = twin.batch_smooth(M, di)
    n_x = int(cp.capi.batch_smooth_layout([T] * B, M)[-1])
    d_m, d_x = guarded(want_m.size, torch.float64, 12345.5), guarded(n_x, torch.int8, -9)
    torch.cuda.current_stream().synchronize()
    engine.batch_smooth_device(d_m[pad:pad + want_m.size], d_x[pad:pad + n_x], n_traj=M, draw_index=di)
    engine.sync()
    assert np.array_equal(inner(d_m, want_m.size, 12345.5).reshape(want_m.shape), want_m)
    assert np.array_equal(inner(d_x, n_x, -9).astype(np.int32), np.concatenate([x.reshape(-1) for x in want_x]))
    # the fixed-lag call
    frm = [b % 3 for b in range(B)]
    want_m, want_x = twin.batch_smooth_lag(lag, frm, M, di)
    n_x = int(cp.capi.batch_smooth_layout([min(lag + 1, T)] * B, M)[-1])
    d_m, d_x = guarded(want_m.size, torch.float64, 12345.5), guarded(n_x, torch.int8, -9)
    torch.cuda.current_stream().synchronize()
    engine.batch_smooth_lag_device(lag, frm, d_m[pad:pad + want_m.size].view(*want_m.shape), d_x[pad:pad + n_x], n_traj=M, draw_index=di)
    engine.sync()
    assert np.array_equal(inner(d_m, want_m.size, 12345.5).reshape(want_m.shape), want_m)
    assert np.array_equal(inner(d_x, n_x, -9).astype(np.int32), np.concatenate([x.reshape(-1) for x in want_x]))
    # the statistics
    want = twin.batch_smooth_stats(np.array(obs))
    flat = np.ascontiguousarray(np.array(obs)).reshape(-1)
    d_s, d_o = guarded(B * 88, torch.float64, 12345.5), torch.from_numpy(flat).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_smooth_stats_device(d_s[pad:pad + B * 88], d_o)
    engine.sync()
    got = cp.capi.split_stats(inner(d_s, B * 88, 12345.5).copy())
    assert all(np.array_equal(got[f], want[f]) for f in ("xi", "occ", "occ_y", "occ_yy"))
    assert engine.batch_smooth_grid() == (0, 0)


# ---- 3. M_t is not the step's reference --------------------------------------------------------------------------------------------
def _bound_and_maximum(twin, b, obs_b, means):
    """(B_t, M_t, rows) of every generation of problem b of the twin: the largest ll of the step, the largest over the occupied
    states, and the rows as they would be with the step's weights q[s] = fix_weight(ll[s], B_t) in the place of the masses' own."""
    vals = twin.batch_store(b)[0]
    ll = np.array(R.log_likelihoods(obs_b, means))
    cnt = np.array([np.bincount(v, minlength=len(means)) for v in vals])
    wrong = np.array([[int(c) * int(q) for c, q in zip(cnt[t], O.fix_weights(ll[t], float(ll[t].max())))] for t in range(len(vals))], np.float64)
    return ll.max(axis=1), np.where(cnt > 0, ll, -np.inf).max(axis=1), wrong


@pytest.mark.parametrize("rs", RESAMPLERS)
def test_the_rows_are_weighed_against_the_exact_maximum_not_the_bound(engine, twin, rs):
    """State 2 sets every step's bound by 0.6 .. 1.6 nats (observes in [1.3, 1.8] between the means 0 and 2: ll_2 - ll_1 = 2 y - 2) --
    far inside kFixGapLimit, so no generation is requantised and the step's reference stays the bound -- and no transition leads into
    it: whatever the initial draw does, from generation 1 on it is empty and M_t < B_t.  The step's own weights
    q[s] = fix_weight(ll[s], B_t) are then NOT the rows' weights."""
    means, trans = [-1.0, 0.0, 2.0], [[1.0, 1.0, 0.0], [1.0, 2.0, 0.0], [3.0, 1.0, 0.0]]
    B, T = 4, 9
    obs = [1.3 + 0.05 * ((3 * t + 2 * b) % 11) for b in range(B) for t in range(T)]
    obs = list(np.array(obs).reshape(B, T))
    seeds = _seeds(B, 43)
    for eng in (engine, twin):
        eng.set_hmm(means, trans)
    for n in (5, 300):
        engine.batch_begin(cp.MODEL_HMM_TABLE, np.array(obs), n, resampler=rs, keep_history=False, keep_masses=True)
        engine.batch_run(seeds)
        twin.batch_begin(cp.MODEL_HMM_TABLE, np.array(obs), n, resampler=rs)
        twin.batch_run(seeds)
        summ = twin.batch_results()[0]
        assert all(s["n_requantised"] == 0 for s in summ) and all(s["n_requantised"] == 0 for s in engine.batch_results()[0])
        for b in range(B):
            bound, M, wrong = _bound_and_maximum(twin, b, obs[b], means)
            below = M < bound
            assert np.all(below[1:]) and np.all(bound - M < GAP_LIMIT), "problem %d: the construction failed (bound - M = %s)" % (b, bound - M)
            # (with the step's own weights the rows would be other numbers: the case is not vacuous)
            got = engine.batch_masses(b)[:, :3]
            assert np.all((got != wrong).any(axis=1)[below]) and np.array_equal(got[~below], wrong[~below])
        _assert_masses(engine, twin, obs, lambda b: means, "n = %d, " % n)
        got, want = engine.batch_smooth(7), twin.batch_smooth(7)
        assert np.array_equal(got[0], want[0]) and all(np.array_equal(x, y) for x, y in zip(got[1], want[1]))


@pytest.mark.parametrize("rs", RESAMPLERS)
def test_requantised_generations_keep_the_twins_masses(engine, twin, rs):
    """tests/test_gpu_batch.py::test_requantised_generations_resample_like_the_one_problem_engine's construction: after step 0 both
    surviving states sit far below every step's bound, the generations are weighed against their exact maximum (n_requantised > 0) --
    there the step's reference IS M_t."""
    means, trans = [-1.0, 0.0, 10.0], [[5.0, 5.0, 0.01], [5.0, 5.0, 0.01], [1.0, 1.0, 1.0]]
    T, B = 8, 4
    obs = np.full((B, T), 30.0)
    obs[:, 0] = [-0.5, -1.2, 0.3, -0.1]
    seeds = _seeds(B, 41)
    for eng in (engine, twin):
        eng.set_hmm(means, trans)
    for n in (3, 8):
        engine.batch_begin(cp.MODEL_HMM_TABLE, obs, n, resampler=rs, keep_history=False, keep_masses=True)
        engine.batch_run(seeds)
        twin.batch_begin(cp.MODEL_HMM_TABLE, obs, n, resampler=rs)
        twin.batch_run(seeds)
        nreq = [s["n_requantised"] for s in engine.batch_results()[0]]
        assert all(x > 0 for x in nreq) and nreq == [s["n_requantised"] for s in twin.batch_results()[0]]
        _assert_masses(engine, twin, list(obs), lambda b: means, "n = %d, " % n)
        got, want = engine.batch_smooth(7), twin.batch_smooth(7)
        assert np.array_equal(got[0], want[0]) and all(np.array_equal(x, y) for x, y in zip(got[1], want[1]))


# ---- 4. batches advanced in pieces -------------------------------------------------------------------------------------------------
def _pieces(Ts, how):
    """The advances of problems of lengths Ts: one observe at a time, uneven pieces, or pieces that leave some problems out."""
    if how == "one":
        return [[1 if t < T else 0 for T in Ts] for t in range(max(Ts))]
    out, at, i = [], [0] * len(Ts), 0
    sizes = [3, 1, 5, 2, 7]
    while any(a < T for a, T in zip(at, Ts)):
        dT = []
        for b, T in enumerate(Ts):
            d = min(sizes[(i + b) % len(sizes)], T - at[b])
            if how == "some" and (i + b) % 3 == 0:
                d = 0                                            # this piece gives problem b nothing
            dT.append(d)
        if how == "some" and not any(dT):
            dT = [min(1, T - a) for a, T in zip(at, Ts)]
        out.append(dT)
        at = [a + d for a, d in zip(at, dT)]
        i += 1
    return out


@pytest.mark.parametrize("how", ["one", "uneven", "some"])
@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("model,k", [("hmm3", 3), ("table", 5)])
def test_online_batches_equal_the_online_twin_after_every_advance(engine, twin, model, k, rs, how):
    Ts, ns, caps = [12, 1, 7, 9], [300, 5, 1, 1500], [12, 3, 9, 9]
    B, lag = len(Ts), 2
    hmm3 = model == "hmm3"
    mid = cp.MODEL_HMM3 if hmm3 else cp.MODEL_HMM_TABLE
    if hmm3:
        means, trans, tables = None, None, None
        obs = [exact.simulate_hmm(T, 170 + b) for b, T in enumerate(Ts)]
    else:
        means, trans = _tables(k, B, 13)
        tables = (means, trans)
        obs = _table_observes(means, Ts, 13)
    means_of = (lambda b: exact.HMM_MEAN) if hmm3 else (lambda b: means[b])
    seeds = _seeds(B, 61)
    engine.batch_begin_online(mid, caps, ns, seeds, tables=tables, resampler=rs, keep_history=False, keep_masses=True)
    twin.batch_begin_online(mid, caps, ns, seeds, tables=tables, resampler=rs)
    # before any observe: empties and zeros, as today
    assert all(engine.batch_masses(b).shape == (0, 8) for b in range(B))
    m0, x0 = engine.batch_smooth_lag(lag, None, 3)
    assert m0.size == 0 and all(x.shape == (0, 3) for x in x0)
    assert np.all(engine.batch_smooth(2)[0] == 0.0) and all(np.all(v == 0.0) for v in engine.batch_smooth_stats().values())
    at = [0] * B
    pieces = _pieces(Ts, how)
    starved, reached = False, [0] * B                          # some piece gives nothing to a problem that still has observes left
    for dT in pieces:
        starved = starved or any(d == 0 and a < T for d, a, T in zip(dT, reached, Ts))
        reached = [a + d for a, d in zip(reached, dT)]
    assert how != "some" or starved
    for dT in pieces:
        new = [obs[b][at[b]:at[b] + dT[b]] for b in range(B)]
        engine.batch_advance(new)
        twin.batch_advance(new)
        frm = [max(0, a - lag) for a in at]                      # the steps the new observes can still change
        at = [a + d for a, d in zip(at, dT)]
        seen = [obs[b][:at[b]] for b in range(B)]
        what = "lengths %s: " % at
        _assert_masses(engine, twin, seen, means_of, what)
        for f in (None, frm):
            got, want = engine.batch_smooth_lag(lag, f, 4, 1), twin.batch_smooth_lag(lag, f, 4, 1)
            assert np.array_equal(got[0], want[0]) and all(np.array_equal(x, y) for x, y in zip(got[1], want[1])), what + "fixed-lag results differ from the twin's"
            assert engine.batch_smooth_grid()[0] == 0
        got, want = engine.batch_smooth_stats(seen), twin.batch_smooth_stats(seen)
        assert all(np.array_equal(got[f], want[f]) for f in got), what + "statistics differ from the twin's"
    assert at == Ts
    # ... and at the end the one-shot batch of the lengths reached
    online = ([engine.batch_masses(b) for b in range(B)], engine.batch_smooth(6, 2), engine.batch_smooth_lag(lag, None, 6, 2), engine.batch_smooth_stats(obs),
              engine.batch_results())
    _begin_ragged(engine, model, obs, ns, means, trans, rs, keep_history=False, keep_masses=True)
    engine.batch_run(seeds)
    shot = ([engine.batch_masses(b) for b in range(B)], engine.batch_smooth(6, 2), engine.batch_smooth_lag(lag, None, 6, 2), engine.batch_smooth_stats(obs))
    assert all(np.array_equal(x, y) for x, y in zip(online[0], shot[0]))
    for i in (1, 2):
        T_shot = shot[i][0].shape[1]                             # (the online batch pads to its largest capacity)
        assert np.array_equal(online[i][0][:, :T_shot], shot[i][0]) and np.all(online[i][0][:, T_shot:] == 0.0)
        assert all(np.array_equal(x, y) for x, y in zip(online[i][1], shot[i][1]))
    assert all(np.array_equal(online[3][f], shot[3][f]) for f in shot[3])
    summ = engine.batch_results()[0]
    assert [s["log_evidence"] for s in summ] == [s["log_evidence"] for s in online[4][0]]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    B, T, n = 3, 4, 10
    obs = np.array([exact.simulate_hmm(T, 800 + b) for b in range(B)])
    seeds = _seeds(B, 9)

    def code(fn):
        with pytest.raises(cp.CpprobHipError) as e:
            fn()
        return e.value.code

    # without the bit: no masses, and a filtering-only batch is not smoothed
    for keep in (True, False):
        engine.batch_begin(cp.MODEL_HMM3, obs, n, keep_history=keep)
        engine.batch_run(seeds)
        assert code(lambda: engine.batch_masses(0)) == ESTATE
    assert code(lambda: engine.batch_smooth(2)) == ESTATE and "keeps no particle store" in engine.L.cpprob_hip_last_error(engine.h).decode()
    assert code(lambda: engine.batch_smooth_lag(1)) == ESTATE
    assert code(lambda: engine.batch_smooth_stats()) == ESTATE
    # the bit with keep_history = 1, and the other bits
    assert code(lambda: engine.batch_begin(cp.MODEL_HMM3, obs, n, keep_history=True, keep_masses=True)) == EINVAL
    assert "filtering-only" in engine.L.cpprob_hip_last_error(engine.h).decode()
    for flags in (1, 3, 4):
        assert code(lambda: engine.batch_begin(cp.MODEL_HMM3, obs, n, keep_history=False, flags=flags)) == EINVAL
    # with the bit: before the run nothing is served; after it the lineage read-outs stay refused
    engine.batch_begin(cp.MODEL_HMM3, obs, n, keep_history=False, keep_masses=True)
    assert code(lambda: engine.batch_masses(0)) == ESTATE
    engine.batch_run(seeds)
    assert engine.batch_masses(B - 1).shape == (T, 8)
    assert code(lambda: engine.batch_store(0)) == ESTATE
    assert code(lambda: engine.batch_paths()) == ESTATE
    assert code(lambda: engine.batch_masses(B)) == EINVAL
    assert code(lambda: engine.batch_masses(-1)) == EINVAL
    out = np.full(T * 8, -7.0)
    assert engine.L.cpprob_hip_batch_copy_masses(engine.h, 0, out.ctypes.data, T * 8 - 1) == EINVAL and np.all(out == -7.0)
    assert engine.L.cpprob_hip_batch_copy_masses(engine.h, 0, None, T * 8) == EINVAL
    assert engine.L.cpprob_hip_batch_copy_masses(engine.h, 0, out.ctypes.data, T * 8) == 0 and np.array_equal(out.reshape(T, 8), engine.batch_masses(0))
    assert engine.L.cpprob_hip_batch_copy_masses(None, 0, out.ctypes.data, T * 8) == EINVAL
    assert C.sizeof(cp.capi.BatchConfig) == 48


# ---- 6. particle EM without a particle store ---------------------------------------------------------------------------------------
def test_em_on_filtering_only_batches_equals_em_on_kept_histories(engine):
    B, k, T, n, iters = 4, 2, 32, 256, 3
    rng = np.random.default_rng(17)
    truth_means, truth_trans = np.array([-1.5, 1.5]), np.array([[0.9, 0.1], [0.2, 0.8]])
    x, obs = 0, []
    for _ in range(T):
        x = int(rng.random() >= truth_trans[x, 0])
        obs.append(truth_means[x] + rng.standard_normal())
    obs = np.array(obs)
    means0 = np.sort(rng.uniform(-2.0, 2.0, (B, k)), axis=1)
    trans0 = rng.uniform(0.2, 1.0, (B, k, k))
    seeds = _seeds(B, 5)
    kept = cp.hmm_table_em(engine, obs, means0, trans0, n, seeds, iters)
    masses = cp.hmm_table_em(engine, obs, means0, trans0, n, seeds, iters, keep_history=False)
    assert engine.batch_smooth_grid()[0] == 0 and engine.batch_masses(0).shape == (T, 8)
    for a, b, name in zip(kept, masses, ("means", "transition rows", "log-evidence")):
        assert a.shape == b.shape and np.array_equal(a, b), "the fitted %s differ between the two kinds of batch" % name
    assert not np.array_equal(kept[0][0], kept[0][-1])             # (the fit moved the tables)
