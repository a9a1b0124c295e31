"""Re-tabling a begun batch (include/cpprob_hip.h: cpprob_hip_batch_retable, _retable_device and their companions;
csrc/batch_retable.hpp) against the reference the feature names: a second context that BEGINS with the new tables.  The sequence under
test -- begin with tables A, run, re-table to tables B, run with seeds S -- must return, array_equal, what begin(B), run(S) returns:
the per-step tables and threshold words as the device holds them, the results, the statistics, the decode, the particle store with its
log-weights and the traces (keep_history), the masses and a conditional run (keep_masses).  B = 6 problems of the ragged lengths
{1, 31, 32, 33, 70, 70}: the rows of a workgroup trip, one either side of it, more than two trips."""
import numpy as np
import pytest

import cpprob_amd as cp
import retable_ref as R
from cpprob_amd import em

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EUNSUPPORTED = -1, -3, -4
TS = [1, R.ROWS_PER_TRIP - 1, R.ROWS_PER_TRIP, R.ROWS_PER_TRIP + 1, 70, 70]
B = len(TS)
MODES = {"history": dict(keep_history=True), "masses": dict(keep_history=False, keep_masses=True), "filter": dict(keep_history=False)}


@pytest.fixture(scope="module")
def ref_engine():
    """A second context: the batches that BEGIN with the tables the engine under test is re-tabled to."""
    import torch  # noqa: F401
    eng = cp.Engine(0)
    yield eng
    eng.close()


def _seeds(base):
    return np.array([base + 7919 * b for b in range(B)], np.uint64)


def _tables(k, seed):
    """Unnormalised transition rows (their totals matter); table 1 has a zero entry and a row with equal consecutive thresholds."""
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, k)), axis=1) + 0.5 * np.arange(k)
    trans = rng.uniform(0.05, 1.0, (B, k, k))
    trans[1, 0, k - 1] = 0.0
    trans[1, 1, 0] = 0.0
    return means, trans


def _observes(k, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-3.0, 3.0 + 0.5 * k, T) + rng.standard_normal(T) for T in TS]


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()                  # (the engine's stream is not ordered behind torch's)
    return t


def _begin(eng, obs, n, tables, mode, resampler):
    eng.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=tables, resampler=resampler, **MODES[mode])


def _retable(eng, form, tables, obs, staged=False):
    if form == "host":
        eng.batch_retable(tables, None if staged else obs)
    else:
        eng.batch_retable_device(_dev(tables[0]), _dev(tables[1]), _dev(np.concatenate(obs)))
        eng.sync()                                                               # (the tensors above die with this frame)


def _readout(eng, mode, obs, k):
    """Everything a run leaves, as nested lists of arrays."""
    out = {"tables": [eng.batch_step_tables(b) for b in range(B)]}
    if mode != "conditional":
        sums, stats, ess, res = eng.batch_results()
        out["summaries"] = [[s[f] for f in sorted(s)] for s in sums]
        out["results"] = [stats, ess, res]
    if mode in ("history", "masses", "conditional"):
        st = eng.batch_smooth_stats(obs)
        out["smooth_stats"] = [st[f] for f in sorted(st)]
        out["decode"] = list(eng.batch_decode())
        out["logp"] = [list(eng.batch_decode_logp(b)) for b in range(B)]
    if mode == "history":
        out["store"] = [list(eng.batch_store(b)) for b in range(B)]
        out["paths"] = list(eng.batch_paths())
    if mode in ("masses", "conditional"):
        out["masses"] = [eng.batch_masses(b) for b in range(B)]
    return out


def _assert_same(got, want, where=""):
    if isinstance(want, dict):
        assert sorted(got) == sorted(want)
        for key in want:
            _assert_same(got[key], want[key], where + "/" + key)
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _assert_same(g, w, "%s[%d]" % (where, i))
    elif want is None:
        assert got is None, where
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.shape == w.shape and g.dtype == w.dtype, where
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), "%s differs (%d of %d entries)" % (where, int(np.sum(g != w)), g.size)


def _estate(call):
    with pytest.raises(cp.CpprobHipError) as e:
        call()
    assert e.value.code == ESTATE, e.value


def _assert_waits_for_a_run(eng, mode, obs):
    """Between a re-table and the run every read-out is refused as after a begin."""
    import torch
    _estate(eng.batch_results)
    _estate(lambda: eng.batch_summaries_device(torch.zeros((B, 4), dtype=torch.float64, device="cuda:0")))
    _estate(lambda: eng.batch_results_device(torch.zeros((B, 4 + max(TS) * 8), dtype=torch.float64, device="cuda:0")))
    _estate(lambda: eng.batch_smooth_stats(obs))
    _estate(eng.batch_decode)
    _estate(lambda: eng.batch_smooth(0))
    _estate(lambda: eng.batch_store(0))
    _estate(eng.batch_paths)
    _estate(lambda: eng.batch_masses(0))
    eng.batch_step_tables(0)                                                     # (the tables themselves read at any time)


CASES = [(n, k, mode) for n in (1, 64, 1500) for k in (2, 8) for mode in MODES]


@pytest.mark.parametrize("n,k,mode", CASES, ids=["n%d-k%d-%s" % c for c in CASES])
def test_retabled_batch_equals_a_fresh_begin(engine, ref_engine, n, k, mode):
    """begin(A), run, re-table(B), run(S) against begin(B), run(S); then a second re-table in a row -- B -> C -> run -- against
    begin(C).  The form and the resampler alternate over the cases so that each pairs with each (ids name n, k and the batch)."""
    i = CASES.index((n, k, mode))
    form = ("host", "device")[i % 2]
    resampler = (cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED)[(i // 2 + i // 6) % 2]
    obs = _observes(k, 40 + k)
    A, Bt, Ct = _tables(k, 1), _tables(k, 2), _tables(k, 3)
    S = _seeds(1000 + i)
    _begin(engine, obs, n, A, mode, resampler)
    assert engine.batch_retable_grid() == 0
    engine.batch_run(_seeds(5))
    _retable(engine, form, Bt, obs)
    assert engine.batch_retable_grid() == R.grid_y(max(TS), B) == 3                 # 70 steps: three trips of 32 rows
    assert not engine.batch_retable_status().any()
    _assert_waits_for_a_run(engine, mode, obs)
    engine.batch_run(S)
    _begin(ref_engine, obs, n, Bt, mode, resampler)
    ref_engine.batch_run(S)
    _assert_same(_readout(engine, mode, obs, k), _readout(ref_engine, mode, obs, k), "B")
    # twice in a row, the second in the other form (the host form's observes are staged by now where the first was the host's)
    other = "device" if form == "host" else "host"
    _retable(engine, form, A, obs, staged=form == "host")
    _retable(engine, other, Ct, obs)
    _assert_waits_for_a_run(engine, mode, obs)
    S2 = _seeds(2000 + i)
    engine.batch_run(S2)
    _begin(ref_engine, obs, n, Ct, mode, resampler)
    ref_engine.batch_run(S2)
    _assert_same(_readout(engine, mode, obs, k), _readout(ref_engine, mode, obs, k), "C")
    if mode == "masses":
        # a conditional run after one more re-table, its reference paths the decode's
        ref = ref_engine.batch_decode()[0]
        _retable(engine, form, Bt, obs, staged=True)
        _estate(lambda: engine.batch_masses(0))
        engine.batch_run_conditional(S, ref)
        _begin(ref_engine, obs, n, Bt, mode, resampler)
        ref_engine.batch_run_conditional(S, ref)
        _assert_same(_readout(engine, "conditional", obs, k), _readout(ref_engine, "conditional", obs, k), "conditional")


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("resampler", [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED])
def test_both_forms_under_both_resamplers_before_any_run(engine, ref_engine, form, resampler):
    """A re-table BEFORE the first run, on a batch begun with the context's table (set_hmm) in place of per-problem ones."""
    k, n = 5, 300
    obs = _observes(k, 9)
    A, Bt = _tables(k, 11), _tables(k, 12)
    engine.set_hmm(A[0][0], A[1][0])
    engine.batch_begin_problems(cp.MODEL_HMM_TABLE, obs, n, tables=None, resampler=resampler, keep_history=True)
    _retable(engine, form, Bt, obs)
    engine.batch_run(_seeds(31))
    _begin(ref_engine, obs, n, Bt, "history", resampler)
    ref_engine.batch_run(_seeds(31))
    _assert_same(_readout(engine, "history", obs, k), _readout(ref_engine, "history", obs, k), form)


@pytest.mark.parametrize("k", [2, 8])
def test_an_invalid_table_keeps_the_old_one(engine, ref_engine, k):
    """The device form checks on the device: problems 2 (a mean not finite), 3 (a negative weight) and 4 (a row without mass) are
    named by batch_retable_status and run on with table A; the others run with table B."""
    n, mode = 64, "history"
    obs = _observes(k, 77)
    A, Bt = _tables(k, 21), _tables(k, 22)
    bad = (Bt[0].copy(), Bt[1].copy())
    bad[0][2, k - 1] = np.nan
    bad[1][3, 0, 1] = -0.5
    bad[1][4, 1, :] = 0.0
    mixed = (Bt[0].copy(), Bt[1].copy())
    for b in (2, 3, 4):
        mixed[0][b], mixed[1][b] = A[0][b], A[1][b]
    _begin(engine, obs, n, A, mode, cp.RESAMPLE_SYSTEMATIC)
    engine.batch_run(_seeds(1))
    _retable(engine, "device", bad, obs)
    assert list(engine.batch_retable_status()) == [0, 0, R.BAD_MEAN, R.BAD_WEIGHT, R.NO_MASS, 0]
    engine.batch_run(_seeds(8))
    _begin(ref_engine, obs, n, mixed, mode, cp.RESAMPLE_SYSTEMATIC)
    ref_engine.batch_run(_seeds(8))
    _assert_same(_readout(engine, mode, obs, k), _readout(ref_engine, mode, obs, k))
    # the host form refuses the same tables with the begin's words, and nothing changes
    for tables, words in (((bad[0], Bt[1]), "problem 2: state means must be finite"), ((Bt[0], bad[1]), "problem 3: transition weights must be finite and >= 0")):
        with pytest.raises(cp.CpprobHipError) as e:
            engine.batch_retable(tables, obs)
        assert e.value.code == EINVAL and words in str(e.value)
    _assert_same(_readout(engine, mode, obs, k), _readout(ref_engine, mode, obs, k), "after the refusals")


def test_rows_and_thresholds_are_the_references(engine):
    """The device's rows and words against tests/retable_ref.py, handed the host's log(2 pi)."""
    import math
    k = 5
    obs = _observes(k, 5)
    A, Bt = _tables(k, 51), _tables(k, 52)
    _begin(engine, obs, 64, A, "filter", cp.RESAMPLE_SYSTEMATIC)
    _retable(engine, "device", Bt, obs)
    log_norm = math.log(2 * 3.14159265358979323846 * 1.0 * 1.0)
    for b in range(B):
        rows, thr = engine.batch_step_tables(b)
        assert np.array_equal(rows, R.rows(obs[b], Bt[0][b], k, log_norm)), b
        assert np.array_equal(thr, R.thresholds(Bt[1][b], k)), b
    assert R.thresholds(Bt[1][1], k)[8] == 0                                     # (the zero entry in front: a word of 0)


def test_mstep_on_the_device_is_em_m_step(engine):
    import torch
    k, n = 3, 64
    obs = _observes(k, 3)
    means, trans = _tables(k, 61)
    _begin(engine, obs, n, (means, trans), "history", cp.RESAMPLE_SYSTEMATIC)
    engine.batch_run(_seeds(4))
    rec = torch.zeros((B, 88), dtype=torch.float64, device="cuda:0")
    d_obs, d_means, d_trans = _dev(np.concatenate(obs)), _dev(means), _dev(trans)
    engine.batch_smooth_stats_device(rec, d_obs)
    engine.sync()
    host = rec.cpu().numpy().copy()
    host[1, 8:16] = 0.0                                                          # a row without mass (problem 1, state 1)
    host[2, 64] = 0.0                                                            # a state without mass (problem 2, state 0)
    rec.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    engine.batch_mstep_device(rec, d_means, d_trans)
    engine.sync()
    want_m, want_t = em.m_step(cp.capi.split_stats(host), means, trans)
    assert np.array_equal(d_means.cpu().numpy(), want_m) and np.array_equal(d_trans.cpu().numpy(), want_t)
    assert np.array_equal(want_t[1, 1], trans[1, 1]) and want_m[2, 0] == means[2, 0] and not np.array_equal(want_t[1, 0], trans[1, 0])
    # the problem of length 1 has no transitions: its rows keep their values, its means moved where a state was visited
    assert np.array_equal(want_t[0], trans[0])
    for b in range(B):
        m, t = R.m_step(host[b], means[b], trans[b], k)
        assert np.array_equal(m, want_m[b]) and np.array_equal(t, want_t[b])


def test_summaries_on_the_device_are_the_results_heads(engine):
    import torch
    k = 2
    obs = _observes(k, 13)
    _begin(engine, obs, 64, _tables(k, 71), "filter", cp.RESAMPLE_STRATIFIED)
    engine.batch_run(_seeds(2))
    out = torch.zeros((B, 4), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    engine.batch_summaries_device(out)
    engine.sync()
    sums = engine.batch_results()[0]
    want = np.array([[s["log_evidence"], s["ess_final"], s["log_norm"], s["max_logw"]] for s in sums])
    assert np.array_equal(out.cpu().numpy(), want)


def test_where_re_tabling_is_refused(engine):
    k = 3
    obs = _observes(k, 1)
    tables = _tables(k, 81)
    flat = np.concatenate(obs)

    def code(call):
        with pytest.raises(cp.CpprobHipError) as e:
            call()
        return e.value.code, str(e.value)
    fresh = cp.Engine(0)
    try:
        fresh.batch_B, fresh.batch_T, fresh.batch_n, fresh.batch_K, fresh.batch_shapes = B, max(TS), 8, 8, (np.array(TS, np.uint32), np.full(B, 8, np.uint32))
        assert code(lambda: fresh.batch_retable(tables, obs))[0] == ESTATE
        assert code(fresh.batch_retable_status)[0] == ESTATE
        assert code(lambda: fresh.batch_step_tables(0))[0] == ESTATE
        assert fresh.batch_retable_grid() == 0
    finally:
        fresh.close()
    # HMM3: the table is the model's
    engine.batch_begin_problems(cp.MODEL_HMM3, obs, 8)
    c, msg = code(lambda: engine.batch_retable(tables, obs))
    assert c == EUNSUPPORTED and "the model's" in msg
    rows, thr = engine.batch_step_tables(4)
    assert rows.shape == (70, 8) and thr is None
    # a uniform batch: one shared table
    engine.set_hmm(tables[0][0], tables[1][0])
    engine.batch_begin(cp.MODEL_HMM_TABLE, np.zeros((B, 4)), 8)
    c, msg = code(lambda: engine.batch_retable(tables, [np.zeros(4)] * B))
    assert c == EUNSUPPORTED and "shares one table" in msg
    rows, thr = engine.batch_step_tables(B - 1)
    assert rows.shape == (4, 8) and np.array_equal(thr, R.thresholds(tables[1][0], k))
    # an online batch
    engine.batch_begin_online(cp.MODEL_HMM_TABLE, TS, 8, _seeds(1), tables=tables)
    engine.batch_advance([o[:1] for o in obs])
    c, msg = code(lambda: engine.batch_retable(tables, [o[:1] for o in obs]))
    assert c == EUNSUPPORTED and "online" in msg
    # a batch of problems: the observes' total, a NULL without staged observes, and a table of the wrong kind change nothing
    _begin(engine, obs, 8, tables, "filter", cp.RESAMPLE_SYSTEMATIC)
    engine.batch_run(_seeds(3))
    want = engine.batch_results()
    c, msg = code(lambda: engine.batch_retable(tables, flat[:-1]))
    assert c == EINVAL and "lengths sum to" in msg
    c, msg = code(lambda: engine.batch_retable(tables, None))
    assert c == EINVAL and "staged" in msg
    assert code(engine.batch_retable_status)[0] == ESTATE
    _assert_same(list(engine.batch_results()), list(want), "after the refusals")
    # a begin forgets the staged observes of the batch before it
    engine.batch_retable(tables, obs)
    engine.batch_retable(tables, None)
    _begin(engine, obs, 8, tables, "filter", cp.RESAMPLE_SYSTEMATIC)
    assert code(lambda: engine.batch_retable(tables, None))[0] == EINVAL
