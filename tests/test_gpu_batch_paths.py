"""Posterior traces of a batch (include/cpprob_hip.h: cpprob_hip_batch_paths, _paths_device; csrc/batch_paths.hpp): one launch
resolves the surviving lineages of every problem.  The kernel copies integers and table doubles, so every comparison in this file is
array_equal / ==: against the host walk over cpprob_hip_batch_copy_store's rows (oracle.lineage), against the one-problem engine's
cpprob_hip_copy_paths, and, for a batch advanced in pieces, against the one-shot batch of the lengths reached."""
import numpy as np
import pytest

import cpprob_amd as cp
from oracle import exact
from oracle import oracle as O

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
RESAMPLERS = [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED]
# n = 1, a partial tile, exactly one tile, one past a tile, several tiles and the maximum; T = 1 and T > 1
SHAPES_T = [1, 2, 1, 5, 16, 7, 3, 4]
SHAPES_N = [1, 1, 777, 2, 1024, 1025, 4099, 8192]
CAPS = [1, 1000, 1024, 9000]
K = 5


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the one-shot batches an online batch is compared with (a begin on `engine` would replace it)."""
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


def _problems(model, Ts, seed=31):
    """(observes, tables or None) of len(Ts) problems."""
    if model == cp.MODEL_HMM3:
        return [exact.simulate_hmm(T, 900 + b) for b, T in enumerate(Ts)], None
    means, trans = _tables(K, len(Ts), seed)
    rng = np.random.default_rng(seed)
    return [means[b][rng.integers(0, K, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)], (means, trans)


def _host_walk(engine, b):
    """Today's route: problem b's rows to the host, the lineage walked there."""
    vals, anc, logw = engine.batch_store(b)
    if vals.shape[0] == 0:
        return vals, logw[:0]
    return np.take_along_axis(vals, O.lineage(anc), axis=1), logw


def _assert_paths_are_the_host_walk(engine, paths, logw, Ts, ns):
    assert len(paths) == len(Ts) and len(logw) == len(Ts)
    for b, (T, n) in enumerate(zip(Ts, ns)):
        ref_p, ref_w = _host_walk(engine, b)
        assert paths[b].dtype == np.int32 and paths[b].shape == (T, n), b
        assert logw[b].dtype == np.float64 and logw[b].shape == ((n,) if T else (0,)), b
        assert np.array_equal(paths[b], ref_p), "problem %d: paths differ from the host walk" % b
        assert np.all(logw[b] == ref_w), "problem %d: log-weights differ from the store's" % b


# ---- 1. described batch, the eight ragged shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
def test_ragged_batch_paths_are_the_host_walk_and_the_one_problem_engine(engine, model, rs):
    obs, tables = _problems(model, SHAPES_T)
    seeds = _seeds(len(SHAPES_T), 19)
    engine.batch_begin_problems(model, obs, SHAPES_N, tables=tables, resampler=rs)
    engine.batch_run(seeds)
    paths, logw = engine.batch_paths()
    _assert_paths_are_the_host_walk(engine, paths, logw, SHAPES_T, SHAPES_N)
    # three problems against the single-population path's own resolved lineages: a one-tile, a two-tile and the largest problem
    for b in (4, 5, 7):
        if tables is not None:
            engine.set_hmm(tables[0][b], tables[1][b])
        engine.begin(cp.ALG_SMC, model, obs[b], SHAPES_N[b], seed=int(seeds[b]), resampler=rs, ess_threshold=2.0, keep_history=True)
        engine.run(0)
        assert np.array_equal(paths[b], engine.paths()), "problem %d: paths differ from the one-problem engine's" % b
        assert np.all(logw[b] == engine.logw()), b
    # (the one-problem runs left the batch as it was)
    again, _ = engine.batch_paths()
    assert all(np.array_equal(x, y) for x, y in zip(paths, again))


# ---- 2. uniform batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
def test_uniform_batch_paths(engine, model):
    B, T, n = 5, 6, 1500
    obs, tables = _problems(model, [T] * B, seed=5)
    if tables is not None:
        engine.set_hmm(tables[0][0], tables[1][0])
    engine.batch_begin(model, np.array(obs), n)
    engine.batch_run(_seeds(B, 3))
    paths, logw = engine.batch_paths()
    _assert_paths_are_the_host_walk(engine, paths, logw, [T] * B, [n] * B)
    first, wfirst = cp.capi.batch_paths_layout([T] * B, [n] * B)
    assert first.tolist() == [b * T * n for b in range(B + 1)] and wfirst.tolist() == [b * n for b in range(B + 1)]


# ---- 3. the particle cap ---------------------------------------------------------------------------------------------------------
def test_capped_paths_are_the_first_columns(engine):
    obs, tables = _problems(cp.MODEL_HMM_TABLE, SHAPES_T)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, SHAPES_N, tables=tables)
    engine.batch_run(_seeds(len(SHAPES_T), 23))
    full_p, full_w = engine.batch_paths()
    for cap in CAPS:
        paths, logw = engine.batch_paths(max_particles=cap)
        for b, (T, n) in enumerate(zip(SHAPES_T, SHAPES_N)):
            m = min(n, cap)
            assert paths[b].shape == (T, m) and logw[b].shape == (m,), (cap, b)
            assert np.array_equal(paths[b], full_p[b][:, :m]), (cap, b)
            assert np.all(logw[b] == full_w[b][:m]), (cap, b)


# ---- 4. a batch advanced in pieces -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [cp.MODEL_HMM3, cp.MODEL_HMM_TABLE])
def test_online_batch_paths_are_the_one_shot_batch_of_the_lengths_reached(engine, ref_engine, model):
    caps, ns = [8, 8, 3], [1025, 3, 777]
    advances = [((3, 0, 1), False), ((0, 2, 2), False), ((5, 1, 0), True)]
    obs, tables = _problems(model, caps, seed=41)
    seeds = _seeds(3, 11)
    engine.batch_begin_online(model, caps, ns, seeds, tables=tables)
    lens = [0, 0, 0]
    for a, (dT, readout) in enumerate(advances):
        engine.batch_advance([obs[b][lens[b]:lens[b] + dT[b]] for b in range(3)], readout=readout)
        lens = [lens[b] + dT[b] for b in range(3)]
        paths, logw = engine.batch_paths()
        idx = [b for b in range(3) if lens[b] >= 1]
        tb = None if tables is None else (tables[0][idx], tables[1][idx])
        ref_engine.batch_begin_problems(model, [obs[b][:lens[b]] for b in idx], [ns[b] for b in idx], tables=tb)
        ref_engine.batch_run(seeds[idx])
        ref_p, ref_w = ref_engine.batch_paths()
        for i, b in enumerate(idx):
            assert paths[b].shape == (lens[b], ns[b])
            assert np.array_equal(paths[b], ref_p[i]), "advance %d, problem %d" % (a, b)
            assert np.all(logw[b] == ref_w[i]), "advance %d, problem %d" % (a, b)
        for b in range(3):
            if lens[b] == 0:
                assert paths[b].shape == (0, ns[b]) and logw[b].shape == (0,), (a, b)
        if a == 0:
            assert lens == [3, 0, 1]
        # the capped form of an online batch, once
        if a == 1:
            cp_p, cp_w = engine.batch_paths(max_particles=2)
            for b in range(3):
                assert np.array_equal(cp_p[b], paths[b][:, :2]) and np.all(cp_w[b] == logw[b][:2])
    assert lens == [8, 3, 3]


# ---- 5. the device variant -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1000])
def test_device_variant_behind_the_run_without_a_host_sync(engine, cap):
    import torch
    obs, tables = _problems(cp.MODEL_HMM_TABLE, SHAPES_T)
    first, wfirst = cp.capi.batch_paths_layout(SHAPES_T, SHAPES_N, cap)
    n_entries, n_weights, pad = int(first[-1]), int(wfirst[-1]), 256
    d_paths = torch.full((n_entries + 2 * pad,), -9, dtype=torch.int8, device="cuda:0")
    d_logw = torch.full((n_weights + 2 * pad,), 12345.5, dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, SHAPES_N, tables=tables)
    engine.batch_run(_seeds(len(SHAPES_T), 29))
    engine.batch_paths_device(d_paths[pad:pad + n_entries], d_logw[pad:pad + n_weights], max_particles=cap)
    engine.sync()
    got_p, got_w = d_paths.cpu().numpy(), d_logw.cpu().numpy()
    assert np.all(got_p[:pad] == -9) and np.all(got_p[pad + n_entries:] == -9)
    assert np.all(got_w[:pad] == 12345.5) and np.all(got_w[pad + n_weights:] == 12345.5)
    paths, logw = engine.batch_paths(max_particles=cap)
    assert np.array_equal(got_p[pad:pad + n_entries].astype(np.int32), np.concatenate([p.reshape(-1) for p in paths]))
    assert np.all(got_w[pad:pad + n_weights] == np.concatenate(logw))
    # without the weights
    d_only = torch.full((n_entries,), -9, dtype=torch.int8, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_paths_device(d_only, None, max_particles=cap)
    engine.sync()
    assert np.array_equal(d_only.cpu().numpy(), got_p[pad:pad + n_entries])


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
def test_paths_errors():
    import ctypes as C
    import torch  # noqa: F401
    eng = cp.Engine(0)
    try:
        with pytest.raises(cp.CpprobHipError) as e:
            eng.batch_B, eng.batch_T, eng.batch_n = 1, 1, 1
            eng.batch_paths()
        assert e.value.code == ESTATE
        obs, _ = _problems(cp.MODEL_HMM3, [3, 2])
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20])
        with pytest.raises(cp.CpprobHipError) as e:          # begun, not run
            eng.batch_paths()
        assert e.value.code == ESTATE
        eng.batch_run(_seeds(2))
        need_p, need_w = 3 * 10 + 2 * 20, 30
        buf = np.full(need_p, -5, np.int32)
        w = np.full(need_w, -5.0)
        rc = eng.L.cpprob_hip_batch_paths(eng.h, 0, buf.ctypes.data, need_p - 1, w.ctypes.data, need_w)
        assert rc == EINVAL and np.all(buf == -5) and np.all(w == -5.0)
        rc = eng.L.cpprob_hip_batch_paths(eng.h, 0, buf.ctypes.data, need_p, w.ctypes.data, need_w - 1)
        assert rc == EINVAL and np.all(buf == -5) and np.all(w == -5.0)
        assert eng.L.cpprob_hip_batch_paths(eng.h, 0, buf.ctypes.data, need_p, None, 0) == 0
        assert np.all(buf >= 0)
        d = torch.full((need_p,), -9, dtype=torch.int8, device="cuda:0")
        torch.cuda.current_stream().synchronize()
        rc = eng.L.cpprob_hip_batch_paths_device(eng.h, 0, C.c_void_p(d.data_ptr()), need_p - 1, None, 0)
        eng.sync()
        assert rc == EINVAL and bool((d == -9).all())
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20], keep_history=False)
        eng.batch_run(_seeds(2))
        with pytest.raises(cp.CpprobHipError) as e:
            eng.batch_paths()
        assert e.value.code == ESTATE and "keep_history" in str(e.value)
    finally:
        eng.close()
