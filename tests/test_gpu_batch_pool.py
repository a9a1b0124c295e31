"""cpprob_hip_batch_tie and cpprob_hip_batch_pool_stats / _pool_stats_device on the device against cpprob_amd.em.pool_stats, bit for bit:
the kernel-text test's case (B = 40, interleaved groups of 1, A - 1, A, A + 1, 2 A + 3 members and the rest, A = kPoolAhead; records
over 2^-30 .. 2^30) in compact, broadcast and in-place form, the real records of a run batch, the life of a tie (a re-table keeps it, a
begin forgets it, a second tie replaces it), and every refusal with nothing written."""
import numpy as np
import pytest
import torch

import cpprob_amd as cp
from cpprob_amd import em

import pool_ref as P

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _begin_case(engine, T=2):
    """A begun batch of 40 problems is all the tie needs: no run."""
    engine.batch_begin(cp.MODEL_HMM3, np.zeros((40, T)), 32)


def _dev(engine, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:%d" % engine.device)
    torch.cuda.current_stream(t.device).synchronize()
    return t


@pytest.mark.parametrize("R", [1, 3])
def test_the_case_in_every_form(engine, R):
    groups, rec = P.case(R, 50 + R)
    _begin_case(engine, T=R % 2 + 1)
    engine.batch_tie(groups)
    got_groups, G = engine.batch_tie_get()
    assert G == 6 and got_groups.dtype == np.int32 and np.array_equal(got_groups, groups)
    full_w, compact_w = em.pool_stats(rec, groups), em.pool_stats(rec, groups, broadcast=False)
    assert _same(full_w, P.pool(rec, groups)) and not _same(compact_w, P.pool(rec, groups, broadcast=False, descending=True))
    # the host form
    assert _same(engine.batch_pool_stats(rec, per_problem=R), full_w)
    assert _same(engine.batch_pool_stats(rec, per_problem=R, broadcast=False), compact_w)
    if R == 1:
        assert _same(engine.batch_pool_stats(rec[:, 0]), full_w[:, 0])
    # the device form: apart (NaN on the way in), compact, and in place
    d_rec = _dev(engine, rec)
    d_full = _dev(engine, np.full(rec.shape, np.nan))
    d_compact = _dev(engine, np.full((G, R, P.RECORD), np.nan))
    engine.batch_pool_stats_device(d_rec, d_full, per_problem=R)
    engine.batch_pool_stats_device(d_rec, d_compact, per_problem=R, broadcast=False)
    engine.sync()
    assert _same(d_full.cpu().numpy(), full_w) and _same(d_compact.cpu().numpy(), compact_w) and _same(d_rec.cpu().numpy(), rec)
    engine.batch_pool_stats_device(d_rec, d_rec, per_problem=R)
    engine.sync()
    assert _same(d_rec.cpu().numpy(), full_w)


def _raw(stats):
    """The dict of batch_smooth_stats / batch_traj_stats as the records it came from, [B, 88] / [B, n_traj, 88]."""
    lead = stats["occ"].shape[:-1]
    return np.ascontiguousarray(np.concatenate([stats["xi"].reshape(lead + (64,)), stats["occ"], stats["occ_y"], stats["occ_yy"]], axis=-1))


@pytest.mark.parametrize("k", [2, 8])
def test_the_records_of_a_run_batch(engine, k):
    """B = 7 ragged problems, groups [0, 1, 0, 2, 2, 0, 2]: the smoother's records and those of three trajectories a problem."""
    rng = np.random.default_rng(90 + k)
    groups = np.array([0, 1, 0, 2, 2, 0, 2])
    T, n = [12, 1, 7, 9, 12, 3, 5], [3, 777, 1025, 3, 777, 1025, 3]
    means = np.sort(rng.uniform(-3.0, 3.0, (7, k)), axis=1)
    trans = rng.uniform(0.05, 1.0, (7, k, k))
    obs = [means[b][rng.integers(0, k, t)] + rng.standard_normal(t) for b, t in enumerate(T)]
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=(means, trans))
    engine.batch_tie(groups)
    engine.batch_run(np.arange(7, dtype=np.uint64) + 5)
    smooth = engine.batch_smooth_stats(obs)
    traj = engine.batch_traj_stats(3, draw_index=2, observes=obs)
    assert np.array_equal(engine.batch_tie_get()[0], groups)          # the run and the passes leave the tie
    for stats, R in ((smooth, 1), (traj, 3)):
        rec = _raw(stats)
        assert rec.shape == ((7, 88) if R == 1 else (7, 3, 88)) and np.any(rec[..., :64] != 0.0) and np.any(rec[..., 72:80] != 0.0)
        for broadcast in (True, False):
            want = em.pool_stats(stats, groups, broadcast=broadcast)
            got = engine.batch_pool_stats(rec, per_problem=R, broadcast=broadcast)
            assert _same(got, _raw(want)), (R, broadcast)
        d = _dev(engine, rec)
        engine.batch_pool_stats_device(d, d, per_problem=R)
        engine.sync()
        assert _same(d.cpu().numpy(), _raw(em.pool_stats(stats, groups)))
    # states >= k are zero in every record, and stay so
    assert k == 8 or not engine.batch_pool_stats(_raw(smooth))[:, 64 + k:72].any()


def test_a_retable_keeps_the_tie_and_a_begin_forgets_it(engine):
    rng = np.random.default_rng(12)
    groups = np.array([1, 0, 1, 0], np.int32)
    means, trans = np.sort(rng.normal(size=(4, 2)), axis=1), rng.uniform(0.1, 1.0, (4, 2, 2))
    obs = [rng.normal(size=t) for t in (3, 5, 2, 4)]
    rec = rng.normal(size=(4, 88))
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 64, tables=(means, trans))
    engine.batch_tie(groups)
    want = em.pool_stats(rec, groups)
    assert _same(engine.batch_pool_stats(rec), want)
    engine.batch_retable((means + 0.25, trans), obs)
    got_groups, G = engine.batch_tie_get()
    assert G == 2 and np.array_equal(got_groups, groups) and _same(engine.batch_pool_stats(rec), want)
    # a second tie replaces the first
    engine.batch_tie([0, 0, 0, 1])
    assert engine.batch_tie_get()[1] == 2 and np.array_equal(engine.batch_tie_get()[0], [0, 0, 0, 1])
    assert _same(engine.batch_pool_stats(rec), em.pool_stats(rec, [0, 0, 0, 1]))
    # any begin forgets it
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, 64, tables=(means, trans))
    out = np.full((4, 88), 7.0)
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_pool_stats(rec, out=out)
    assert e.value.code == ESTATE and np.all(out == 7.0)
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_tie_get()
    assert e.value.code == ESTATE
    d = _dev(engine, rec)
    with pytest.raises(cp.CpprobHipError) as e:
        engine.batch_pool_stats_device(d, d)
    assert e.value.code == ESTATE
    engine.sync()
    assert _same(d.cpu().numpy(), rec)


def test_an_online_batch_is_tied_too(engine):
    rng = np.random.default_rng(13)
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, [4, 4, 4], 32, np.arange(3, dtype=np.uint64), tables=(np.sort(rng.normal(size=(3, 2)), axis=1), rng.uniform(0.1, 1.0, (3, 2, 2))))
    engine.batch_tie([0, 1, 0])
    rec = rng.normal(size=(3, 88))
    assert _same(engine.batch_pool_stats(rec, broadcast=False), em.pool_stats(rec, [0, 1, 0], broadcast=False))


def test_a_context_without_a_batch_is_out_of_order():
    eng = cp.Engine(0)
    try:
        rec, out = np.zeros((2, 88)), np.full((2, 88), 7.0)
        for call in (lambda: eng.batch_tie([0, 0]), lambda: eng.batch_tie_get(), lambda: eng.batch_pool_stats(rec, out=out)):
            with pytest.raises(cp.CpprobHipError) as e:
                call()
            assert e.value.code == ESTATE
        assert np.all(out == 7.0)
    finally:
        eng.close()


def test_refusals_write_nothing(engine):
    groups, rec = P.case(1, 3)
    rec = rec[:, 0]
    _begin_case(engine)
    engine.batch_tie(groups)

    def refused(code, call):
        with pytest.raises(cp.CpprobHipError) as e:
            call()
        assert e.value.code == code, str(e.value)

    # the tie: a wrong count, a negative id, an unused id -- and the tie in force stays
    for bad in (groups[:39], np.concatenate([groups, [0]]), np.where(np.arange(40) == 5, -1, groups), np.where(groups == 3, 6, groups), groups + 1):
        refused(EINVAL, lambda bad=bad: engine.batch_tie(bad))
    assert np.array_equal(engine.batch_tie_get()[0], groups) and engine.batch_tie_get()[1] == 6
    # the pooling, host form: out untouched
    out = np.full((40, 88), 7.0)
    small = np.full((39, 88), 7.0)
    refused(EINVAL, lambda: engine.batch_pool_stats(rec[:39], out=out))                                  # n_doubles < 88 B R
    refused(EINVAL, lambda: engine.batch_pool_stats(rec, out=small))                                     # n_out too small (broadcast)
    refused(EINVAL, lambda: engine.batch_pool_stats(rec, broadcast=False, out=np.full((5, 88), 7.0)))   # n_out too small (compact)
    refused(EINVAL, lambda: engine.batch_pool_stats(rec, per_problem=0, out=out))                        # R == 0
    refused(EINVAL, lambda: engine.batch_pool_stats(rec, per_problem=2, out=out))                        # R = 2 wants twice the records
    refused(EINVAL, lambda: engine.batch_pool_stats(rec, per_problem=1 << 30, out=out))                  # G R beyond a grid (and the records)
    assert np.all(out == 7.0) and np.all(small == 7.0)
    # the device form: overlaps other than the in-place one, and the compact form in place
    d = _dev(engine, np.concatenate([rec, rec]))
    flat = d.reshape(-1)
    refused(EINVAL, lambda: engine.batch_pool_stats_device(flat[:40 * 88], flat[88:88 + 40 * 88]))
    refused(EINVAL, lambda: engine.batch_pool_stats_device(flat[88:88 + 40 * 88], flat[:40 * 88]))
    refused(EINVAL, lambda: engine.batch_pool_stats_device(flat[:40 * 88], flat[:40 * 88], broadcast=False))
    refused(EINVAL, lambda: engine.batch_pool_stats_device(flat[:39 * 88], flat[40 * 88:]))
    refused(EINVAL, lambda: engine.batch_pool_stats_device(flat[:40 * 88], flat[40 * 88:79 * 88]))
    engine.sync()
    assert _same(d.cpu().numpy(), np.concatenate([rec, rec]))
    # neighbours apart are no overlap
    engine.batch_pool_stats_device(flat[:40 * 88], flat[40 * 88:])
    engine.sync()
    assert _same(d.cpu().numpy()[40:], em.pool_stats(rec, groups)) and _same(d.cpu().numpy()[:40], rec)
