"""Trajectory sufficient statistics of a batch (include/cpprob_hip.h: cpprob_hip_batch_traj_stats, _traj_stats_device;
csrc/batch_trajstats.hpp) against the plain-Python record (tests/trajstats_ref.py) of the very trajectories cpprob_hip_batch_smooth
returns for the same draw_index: the counts are integers and the sums sequential IEEE additions, so every comparison is array_equal."""
import ctypes as C

import numpy as np
import pytest

import cpprob_amd as cp
import trajstats_ref as TS
from oracle import exact

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3
TILE = cp.capi.TRAJ_STATS_TILE
FIELDS = ("xi", "occ", "occ_y", "occ_yy")


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the one-shot batches an online batch is compared with (a begin on `engine` would replace it)."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _seeds(nb, base=77):
    return np.array([base + 7919 * b for b in range(nb)], np.uint64)


def _records(stats):
    """[B, n_traj, 88] of the dict Engine.batch_traj_stats returns."""
    B, M = stats["occ"].shape[:2]
    return np.concatenate([stats["xi"].reshape(B, M, 64), stats["occ"], stats["occ_y"], stats["occ_yy"]], axis=-1)


def _check(engine, n_traj, draw_index, obs, what):
    """The call's records against the reference applied to batch_smooth's columns; returns them [B, n_traj, 88]."""
    stats = engine.batch_traj_stats(n_traj, draw_index, obs)
    reached = sum(len(o) for o in obs)
    tiles = engine.batch_traj_stats_grid()
    assert tiles == (-(-n_traj // TILE) if reached else 0), "%s: %d tiles for %d trajectories" % (what, tiles, n_traj)
    assert stats["xi"].shape == (len(obs), n_traj, 8, 8) and all(stats[f].shape == (len(obs), n_traj, 8) for f in FIELDS[1:])
    got = _records(stats)
    _, traj = engine.batch_smooth(n_traj, draw_index)
    assert engine.batch_traj_stats_grid() == 0, "another smoothing call resets the grid"
    for b, o in enumerate(obs):
        assert traj[b].shape == (len(o), n_traj)
        want = TS.records(traj[b], o)
        assert np.array_equal(got[b], want), "%s, problem %d, n_traj %d: records differ from the reference on batch_smooth's trajectories" % (what, b, n_traj)
    blind = _records(engine.batch_traj_stats(n_traj, draw_index))
    assert np.array_equal(blind[:, :, :72], got[:, :, :72]) and np.all(blind[:, :, 72:] == 0.0), "%s: without observes" % what
    return got


def _untouched(engine, call):
    """batch_results, batch_smooth and batch_decode return the same arrays before and after `call`."""
    def snap():
        res = engine.batch_results()
        marg, traj = engine.batch_smooth(5, 1)
        paths, score = engine.batch_decode()
        return res, marg, traj, paths, score
    before = snap()
    call()
    after = snap()
    assert before[0][0] == after[0][0] and all(np.array_equal(x, y) for x, y in zip(before[0][1:], after[0][1:]))
    assert np.array_equal(before[1], after[1]) and all(np.array_equal(x, y) for x, y in zip(before[2], after[2]))
    assert all(np.array_equal(x, y) for x, y in zip(before[3], after[3])) and np.array_equal(before[4], after[4])


def _device_form(engine, n_traj, draw_index, obs, host):
    import torch
    B = len(obs)
    flat = np.concatenate(obs)
    n_doubles, pad = B * n_traj * 88, 256
    d_stats = torch.full((n_doubles + 2 * pad,), 12345.5, dtype=torch.float64, device="cuda:0")
    d_obs = torch.from_numpy(flat).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_traj_stats_device(d_stats[pad:pad + n_doubles], n_traj, draw_index, d_obs)
    engine.sync()
    got = d_stats.cpu().numpy()
    assert np.all(got[:pad] == 12345.5) and np.all(got[pad + n_doubles:] == 12345.5), "the device form wrote outside its records"
    assert np.array_equal(got[pad:pad + n_doubles].reshape(B, n_traj, 88), host), "the device form differs from the host call"
    assert engine.batch_traj_stats_grid() == -(-n_traj // TILE)


# ---- 1. a uniform HMM3 batch -----------------------------------------------------------------------------------------------------
def test_uniform_hmm3_batch(engine):
    B, T, n = 3, 9, 64
    obs = [exact.simulate_hmm(T, 900 + b) for b in range(B)]
    engine.batch_begin(cp.MODEL_HMM3, np.array(obs), n)
    engine.batch_run(_seeds(B, 3))
    assert engine.batch_traj_stats_grid() == 0
    got = {m: _check(engine, m, 0, obs, "hmm3") for m in (1, 2, TILE + 1)}
    assert np.array_equal(got[1], got[TILE + 1][:, :1]) and np.array_equal(got[2], got[TILE + 1][:, :2]), "a trajectory depends on n_traj"
    assert np.all(got[TILE + 1][:, :, :64].sum(axis=2) == T - 1) and np.all(got[TILE + 1][:, :, 64:72].sum(axis=2) == T)
    xi = got[TILE + 1][:, :, :64].reshape(B, -1, 8, 8)
    assert np.all(xi[:, :, 3:] == 0.0) and np.all(xi[:, :, :, 3:] == 0.0) and np.all(got[TILE + 1][:, :, 67:72] == 0.0)
    other = _check(engine, 2, 7, obs, "hmm3, draw_index 7")
    assert not np.array_equal(other, got[2]), "another draw_index gives other records"
    _device_form(engine, TILE + 1, 0, obs, got[TILE + 1])
    _untouched(engine, lambda: engine.batch_traj_stats(TILE + 1, 0, obs))
    # the uniform batch's observes as an array [B, T]
    assert np.array_equal(_records(engine.batch_traj_stats(2, 0, np.array(obs))), got[2])


# ---- 2. a described table batch, with its history and with the masses alone --------------------------------------------------------
def _described():
    """k = 5, ragged lengths with T = 1 (no backward step) and T = 600 (its 64 T bytes exceed what a workgroup stages) among them;
    problem 1's table has a zero transition entry."""
    k, Ts, ns = 5, [1, 2, 7, 33, 600], [1, 3, 70, 300, 64]
    rng = np.random.default_rng(36)
    means = np.sort(rng.uniform(-3.0, 3.0, (len(Ts), k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (len(Ts), k, k))
    trans[1, 0, k - 1] = 0.0
    obs = [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    return k, Ts, ns, means, trans, obs


def test_described_table_batch_and_the_masses_alone(engine):
    k, Ts, ns, means, trans, obs = _described()
    B = len(Ts)
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans))
    engine.batch_run(_seeds(B, 19))
    got = {m: _check(engine, m, 3, obs, "described") for m in (1, 2, TILE + 1)}
    assert np.array_equal(got[2], got[TILE + 1][:, :2])
    big = got[TILE + 1]
    assert np.all(big[0, :, :64] == 0.0) and np.all(big[0, :, 64:72].sum(axis=1) == 1.0), "T = 1 has no transition"
    assert np.all(big[4, :, :64].sum(axis=1) == 599.0)
    assert np.all(big[1, :, 8 * 0 + k - 1] == 0.0), "a transition of probability zero was drawn"
    _device_form(engine, TILE + 1, 3, obs, big)
    _untouched(engine, lambda: engine.batch_traj_stats(2, 3, obs))
    # the same batch filtering-only, from the masses the run keeps: the same bits
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, ns, tables=(means, trans), keep_history=False, keep_masses=True)
    engine.batch_run(_seeds(B, 19))
    for m in (1, TILE + 1):
        kept = _records(engine.batch_traj_stats(m, 3, obs))
        assert engine.batch_traj_stats_grid() == -(-m // TILE)
        assert np.array_equal(kept, big[:, :m]), "keep_masses, n_traj %d: records differ from the batch with history" % m


# ---- 3. an online batch ------------------------------------------------------------------------------------------------------------
def test_online_batch_however_it_is_cut(engine, ref_engine):
    """Fed in uneven pieces and checked at lengths [5, 0, 1] and at the end: the records are the one-shot batch's of the lengths
    reached, whichever call counted the new rows, and the same for another cutting."""
    k, caps, ns = 5, [23, 9, 5], [70, 1, 300]
    rng = np.random.default_rng(8)
    means = np.sort(rng.uniform(-3.0, 3.0, (3, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (3, k, k))
    obs = [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b, T in enumerate(caps)]
    seeds = _seeds(3, 11)
    n_traj, d = TILE + 1, 2

    def one_shot(lens):
        idx = [b for b in range(3) if lens[b] >= 1]
        ref_engine.batch_begin_problems(cp.MODEL_HMM_TABLE, [obs[b][:lens[b]] for b in idx], [ns[b] for b in idx], tables=(means[idx], trans[idx]))
        ref_engine.batch_run(seeds[idx])
        rec = _records(ref_engine.batch_traj_stats(n_traj, d, [obs[b][:lens[b]] for b in idx]))
        out = np.zeros((3, n_traj, 88))
        out[idx] = rec
        return out

    finals = []
    for cut in ([(5, 0, 1), (1, 9, 0), (17, 0, 4)], [(2, 0, 0), (3, 0, 1), (0, 4, 4), (18, 5, 0)]):
        engine.batch_begin_online(cp.MODEL_HMM_TABLE, caps, ns, seeds, tables=(means, trans))
        none = engine.batch_traj_stats(2, d, [[], [], []])
        assert all(np.all(v == 0.0) for v in none.values()) and engine.batch_traj_stats_grid() == 0, "nothing reached: zero records, no launch"
        lens = [0, 0, 0]
        for a, dT in enumerate(cut):
            engine.batch_advance([obs[b][lens[b]:lens[b] + dT[b]] for b in range(3)])
            lens = [lens[b] + dT[b] for b in range(3)]
            seen = [obs[b][:lens[b]] for b in range(3)]
            if a == 1:
                engine.batch_smooth(0)                                   # (this call counts the new rows, the statistics call none)
            if lens == [5, 0, 1] or lens == caps:
                got = _check(engine, n_traj, d, seen, "online at %s" % lens)
                assert np.array_equal(got, one_shot(lens)), "online at %s: records differ from the one-shot batch's" % lens
                assert np.array_equal(_records(engine.batch_traj_stats(n_traj, d, seen)), got), "a second call gives other records"
                if lens[1] == 0:
                    assert np.all(got[1] == 0.0), "a problem without observes has zero records"
            elif a == 0:
                engine.batch_traj_stats(1, d, seen)                      # (this call counts the new rows, the later ones none of them again)
        assert lens == caps
        finals.append(got)
    assert np.array_equal(finals[0], finals[1]), "the records depend on how the observes were cut"


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    eng = cp.Engine(0)
    try:
        eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K, eng.batch_shapes = 1, 1, 1, 3, None
        with pytest.raises(cp.CpprobHipError) as e:          # no batch
            eng.batch_traj_stats(1)
        assert e.value.code == ESTATE
        obs = [exact.simulate_hmm(T, 70 + b) for b, T in enumerate([3, 2])]
        flat = np.concatenate(obs)
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20])
        with pytest.raises(cp.CpprobHipError) as e:          # begun, not run
            eng.batch_traj_stats(1, 0, obs)
        assert e.value.code == ESTATE
        eng.batch_run(_seeds(2))
        M = 3
        rec = np.full(2 * M * 88, -5.0)
        call = eng.L.cpprob_hip_batch_traj_stats
        for n_traj, di, n_obs, cap in ((0, 0, flat.size, rec.size), ((1 << 20) + 1, 0, flat.size, rec.size), (M, 1 << 16, flat.size, rec.size),
                                       (M, 0, flat.size, rec.size - 1), (M, 0, flat.size - 1, rec.size), (M, 0, flat.size + 1, rec.size)):
            assert call(eng.h, n_traj, di, flat.ctypes.data, n_obs, rec.ctypes.data, cap) == EINVAL, (n_traj, di, n_obs, cap)
            assert np.all(rec == -5.0)
        assert call(eng.h, M, 0, flat.ctypes.data, flat.size, None, rec.size) == EINVAL
        assert eng.batch_traj_stats_grid() == 0
        assert call(eng.h, M, 0, flat.ctypes.data, flat.size, rec.ctypes.data, rec.size) == 0
        st = cp.capi.split_traj_stats(rec.reshape(2, M, 88))
        assert np.array_equal(st["occ"].sum(axis=2), [[3.0] * M, [2.0] * M]) and np.array_equal(st["xi"].sum(axis=(2, 3)), [[2.0] * M, [1.0] * M])
        d = torch.full((2 * M * 88,), -9.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.current_stream().synchronize()
        rc = eng.L.cpprob_hip_batch_traj_stats_device(eng.h, M, 0, None, 0, C.c_void_p(d.data_ptr()), 2 * M * 88 - 1)
        eng.sync()
        assert rc == EINVAL and bool((d == -9.0).all())
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20], keep_history=False)
        eng.batch_run(_seeds(2))
        with pytest.raises(cp.CpprobHipError) as e:          # neither history nor masses
            eng.batch_traj_stats(1, 0, obs)
        assert e.value.code == ESTATE and "keep_history" in str(e.value)
    finally:
        eng.close()
