"""The conjugate draw of a Gibbs sweep on the device (cpprob_hip_batch_draw_tables_device; csrc/batch_gibbs.hpp) against its plain-Python
restatement tests/gibbs_ref.py, and the resident samplers against chains stepped from the host with the existing calls.  Logarithm,
square root and division are the same IEEE operations on both sides, so every comparison is array_equal."""
import numpy as np
import pytest

import gibbs_ref as GR
from cpprob_amd import em, gibbs, pgibbs
from cpprob_amd.capi import MODEL_HMM_TABLE, CpprobHipError

pytestmark = pytest.mark.gpu

B, PAD, GUARD = 5, 16, -777.25
SEEDS = np.array([11 + 7919 * b for b in range(B)], np.uint64)
# max_attempts = 1 (k = 2, unit, alpha = 1.0, sweep 3): found with gibbs_ref on the CPU -- problems 1 and 3 draw all six variates at their
# first attempt, problems 0, 2 and 4 do not
CAP_SEEDS, CAP_DRAWN = np.array([1, 13, 3, 34, 6], np.uint64), [False, True, False, True, False]


def _records():
    """[B, 88]: an all-zero transition row (the shape is alpha), a state never visited, counts of 1e4 (a large d), fractional counts."""
    rec = np.zeros((B, 88))
    for b in range(B):
        for s in range(8):
            rec[b, 8 * s:8 * s + 8] = [(3 * b + 2 * s + j) % 5 for j in range(8)]
            occ, y = rec[b, 8 * s:8 * s + 8].sum() + 1.0, 0.5 * s - 1.0 + 0.125 * b
            rec[b, 64 + s], rec[b, 72 + s], rec[b, 80 + s] = occ, occ * y, occ * (y * y + 0.81)
    rec[0, 0:8] = 0.0
    rec[0, [65, 73, 81]] = 0.0
    rec[1] *= 1e4
    rec[2] *= 0.375
    rec[3] += 0.3
    return rec


def _tables(k, scaled, nb=B):
    means = np.array([[0.5 * s - 1.0 + 0.01 * b for s in range(k)] for b in range(nb)])
    trans = np.array([[[1.0 + (s == j) for j in range(k)] for s in range(k)] for b in range(nb)]) / (k + 1.0)
    return means, trans, (np.array([[0.7 + 0.1 * s + 0.02 * b for s in range(k)] for b in range(nb)]) if scaled else None)


def _begin(engine, k, scaled, emission="normal"):
    means, trans, sigmas = _tables(k, scaled)
    obs = [np.arange(4.0) + b for b in range(B)]
    engine.batch_begin_problems(MODEL_HMM_TABLE, obs, 64, tables=(means, trans) if sigmas is None else (means, trans, sigmas), emission=emission)
    return means, trans, sigmas


def _device(arrays):
    """Guarded device copies: each array's values followed by PAD sentinels; returns (views, whole tensors)."""
    import torch
    whole = [None if a is None else torch.cat([torch.from_numpy(a.reshape(-1)), torch.full((PAD,), GUARD, dtype=torch.float64)]).to("cuda:0") for a in arrays]
    torch.cuda.current_stream().synchronize()
    return [None if w is None else w[:-PAD] for w in whole], whole


def _draw(engine, rec, seeds, sweep, tables, **kw):
    """One device draw from host arrays: (means, trans, sigmas or None, status) as numpy, shaped as `tables`; the guards are checked."""
    import torch
    view, whole = _device(tables)
    d_rec = torch.from_numpy(rec).to("cuda:0")
    d_seeds = torch.from_numpy(seeds.view(np.int64)).to("cuda:0")
    status = torch.full((B + PAD,), -9, dtype=torch.int32, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_draw_tables_device(d_rec, d_seeds, sweep, view[0], view[1], sigmas=view[2], status=status[:B], **kw)
    engine.sync()
    assert all(w is None or bool((w[-PAD:] == GUARD).all()) for w in whole) and bool((status[B:] == -9).all()), "a store past the caller's arrays"
    return tuple(None if v is None else v.cpu().numpy().reshape(t.shape) for v, t in zip(view, tables)) + (status[:B].cpu().numpy(),)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("means", "rows", "sigmas", "status")):
        assert (g is None and w is None) or np.array_equal(g, w), "%s: %s differ from the restatement" % (what, name)


@pytest.mark.parametrize("alpha", [1.0, 2.5])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_draw_equals_restatement(engine, k, scaled, alpha):
    tables, rec = _begin(engine, k, scaled), _records()
    got = _draw(engine, rec, SEEDS, 7, tables, alpha=alpha, mu0=0.25, tau0=3.0, a0=2.0, b0=0.5)
    want = GR.draw_tables(rec, SEEDS, 7, *tables, alpha=alpha, mu0=0.25, tau0=3.0, a0=2.0, b0=0.5)
    assert not want[3].any() and not np.array_equal(want[0], tables[0])
    _same(got, want, "k = %d" % k)
    _same(_draw(engine, rec, SEEDS, 7, tables, alpha=alpha, mu0=0.25, tau0=3.0, a0=2.0, b0=0.5), got, "the same call again")
    other = _draw(engine, rec, SEEDS, 8, tables, alpha=alpha, mu0=0.25, tau0=3.0, a0=2.0, b0=0.5)
    assert not np.array_equal(other[0], got[0]) and not np.array_equal(other[1], got[1]), "another sweep, the same words"


def test_attempt_cap(engine):
    """max_attempts = 1: status 32 exactly where the restatement finds no complete draw; those problems keep their tables."""
    tables, rec = _begin(engine, 2, False), _records()
    want = GR.draw_tables(rec, CAP_SEEDS, 3, *tables, max_attempts=1)
    assert [st == 0 for st in want[3]] == CAP_DRAWN and all(st in (0, GR.NO_DRAW) for st in want[3])
    got = _draw(engine, rec, CAP_SEEDS, 3, tables, max_attempts=1)
    _same(got, want, "max_attempts = 1")
    for b in range(B):
        assert CAP_DRAWN[b] or (np.array_equal(got[0][b], tables[0][b]) and np.array_equal(got[1][b], tables[1][b])), "problem %d lost its table" % b


@pytest.mark.parametrize("begun, sigmas, kw, code", [
    ("unit", False, {"alpha": 0.5}, -1), ("scaled", True, {"a0": 0.5}, -1), ("unit", False, {"max_attempts": 0}, -1), ("unit", False, {"max_attempts": 65}, -1),
    ("unit", True, {}, -3), ("scaled", False, {}, -3), ("poisson", False, {}, -3)])
def test_refusals(engine, begun, sigmas, kw, code):
    """EINVAL (-1) for a prior or a cap the generator does not serve, ESTATE (-3) for the wrong family; nothing is enqueued."""
    import torch
    if begun == "poisson":
        rates, trans, _ = _tables(2, False)
        engine.batch_begin_problems(MODEL_HMM_TABLE, [np.arange(4.0)] * B, 64, tables=(np.abs(rates) + 1.0, trans), emission="poisson")
    else:
        _begin(engine, 2, begun == "scaled")
    tables = _tables(2, sigmas)
    view, _ = _device(tables)
    d_rec = torch.from_numpy(_records()).to("cuda:0")
    d_seeds = torch.from_numpy(SEEDS.view(np.int64)).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    with pytest.raises(CpprobHipError) as err:
        engine.batch_draw_tables_device(d_rec, d_seeds, 0, view[0], view[1], sigmas=view[2], **kw)
    assert err.value.code == code and ("Poisson" in str(err.value) or begun != "poisson")
    engine.sync()
    assert all(v is None or np.array_equal(v.cpu().numpy().reshape(t.shape), t) for v, t in zip(view, tables)), "a refused call stored something"


def _host_chain(engine, particle, obs, means, trans, sigmas, groups, n, seeds, sweeps):
    """The chain stepped from the host with the existing calls and gibbs_ref's draw: the histories the resident route must return."""
    import torch
    Bc = means.shape[0]
    ts = seeds if groups is None else seeds[em.check_tied_start(groups, means, trans, sigmas)[2][groups]]
    traj = [torch.empty(sum(len(o) for o in obs), dtype=torch.int8, device="cuda:0") for _ in range(2)]
    hist, ev = [(means, trans, sigmas)], np.zeros((sweeps, Bc))
    engine.batch_begin_problems(MODEL_HMM_TABLE, obs, n, tables=(means, trans) if sigmas is None else (means, trans, sigmas), keep_history=False, keep_masses=True)
    for i in range(sweeps):
        if particle and i > 0:
            engine.batch_run_conditional_device(seeds + np.uint64(i), traj[(i - 1) & 1])
        else:
            engine.batch_run(seeds + np.uint64(i))
            ev[i] = [s["log_evidence"] for s in engine.batch_results()[0]]
        if particle:
            engine.batch_smooth_device(traj_i8=traj[i & 1], n_traj=1, draw_index=i)
        st = engine.batch_traj_stats(1, draw_index=i, observes=obs)
        rec = np.concatenate([st["xi"].reshape(Bc, 1, 64), st["occ"], st["occ_y"], st["occ_yy"]], axis=-1)[:, 0]
        if groups is not None:
            rec = em.pool_stats(rec, groups)
        means, trans, sigmas, status = GR.draw_tables(rec, ts, i, means, trans, sigmas)
        hist.append((means, trans, sigmas))
        engine.batch_retable((means, trans) if sigmas is None else (means, trans, sigmas), obs if i == 0 else None)
    return hist, ev, status


@pytest.mark.parametrize("variant", ["unit", "scaled", "tied"])
@pytest.mark.parametrize("particle", [False, True])
def test_resident_chain_equals_host_stepped(engine, particle, variant):
    Bc, k, T, n, sweeps = 3, 2, 12, 64, 3
    obs = [np.array([((-1.0) ** (t // 3) + 0.25 * np.sin(1.7 * t + b)) for t in range(T)]) for b in range(Bc)]
    groups = np.array([0, 0, 1], np.int32) if variant == "tied" else None
    means, trans, sigmas = _tables(k, variant == "scaled", Bc)
    if groups is not None:
        means[1] = means[0]
    seeds = np.array([5, 6, 7], np.uint64)
    hist, ev, status = _host_chain(engine, particle, obs, means, trans, sigmas, groups, n, seeds, sweeps)
    if particle:
        got = pgibbs.hmm_table_particle_gibbs(engine, obs, means, trans, n, seeds, sweeps, None, sigmas0=sigmas, groups=groups, resident=True)
    else:
        got = gibbs.hmm_table_gibbs(engine, obs, means, trans, n, seeds, sweeps, None, keep_history=False, sigmas0=sigmas, groups=groups, resident=True)
        assert np.array_equal(got[2], ev), "the sweeps' evidences"
    assert np.array_equal(got[0], np.array([h[0] for h in hist])) and np.array_equal(got[1], np.array([h[1] for h in hist])), "the tables' history"
    assert sigmas is None or np.array_equal(got[-2], np.array([h[2] for h in hist])), "the sigmas' history"
    assert np.array_equal(got[-1], status) and not np.array_equal(got[0][1], got[0][0])
    assert groups is None or (np.array_equal(got[0][:, 0], got[0][:, 1]) and np.array_equal(got[1][:, 0], got[1][:, 1])), "a group's members hold one table"
