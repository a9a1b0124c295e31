"""Decoding a batch (include/cpprob_hip.h: cpprob_hip_batch_decode, _decode_device, cpprob_hip_batch_decode_lag, _decode_lag_device,
cpprob_hip_batch_decode_logp; csrc/batch_decode.hpp) against the plain-Python restatement of its arithmetic (tests/decode_ref.py), fed
the library's own log table, the masses formed from the rows the run left (cpprob_hip_batch_copy_store) or kept
(cpprob_hip_batch_copy_masses) and the host's log-likelihood rows.  Paths, fixed-lag rows and scores are pure functions of those bits
and IEEE additions: array_equal and exact equality of doubles everywhere but in the comparison of two logarithms."""
import ctypes as C
import math

import numpy as np
import pytest

import backward_ref as R
import cpprob_amd as cp
import decode_ref as D
from oracle import exact

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -3


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


def _case(name):
    """(model, Ts, ns, means [B, k], trans [B, k, k], observes, seeds): hmm3 a uniform batch, tableK a described one with ragged
    lengths, a problem of one particle and per-problem tables, uniformK a uniform batch under the one table of set_hmm."""
    if name == "hmm3":
        B, T = 3, 5
        return (cp.MODEL_HMM3, [T] * B, [100] * B, np.array([exact.HMM_MEAN] * B), np.array([exact.HMM_T] * B),
                [exact.simulate_hmm(T, 900 + b) for b in range(B)], _seeds(B, 3))
    if name.startswith("uniform"):
        k, B, T = int(name[7:]), 3, 6
        means, trans = _tables(k, 1, 57 + k)
        rng = np.random.default_rng(157 + k)
        obs = [means[0][rng.integers(0, k, T)] + rng.standard_normal(T) for _ in range(B)]
        return cp.MODEL_HMM_TABLE, [T] * B, [64] * B, np.repeat(means, B, 0), np.repeat(trans, B, 0), obs, _seeds(B, 23)
    k = int(name[5:])
    Ts, ns = [9, 4, 1, 23], [1, 64, 300, 1025]
    means, trans = _tables(k, 4, 31 + k)
    rng = np.random.default_rng(131 + k)
    obs = [means[b][rng.integers(0, k, T)] + rng.standard_normal(T) for b, T in enumerate(Ts)]
    return cp.MODEL_HMM_TABLE, Ts, ns, means, trans, obs, _seeds(4, 19 + k)


def _begin(engine, case, resampler=cp.RESAMPLE_SYSTEMATIC, **kw):
    model, Ts, ns, means, trans, obs, seeds = case
    if model == cp.MODEL_HMM3 or len(set(Ts)) == 1:
        if model == cp.MODEL_HMM_TABLE:
            engine.set_hmm(means[0], trans[0])
        engine.batch_begin(model, np.array(obs), ns[0], resampler=resampler, **kw)
    else:
        engine.batch_begin_problems(model, obs, ns, tables=(means, trans), resampler=resampler, **kw)
    engine.batch_run(seeds)


def _table(engine, b, k):
    lp, lp0 = engine.batch_decode_logp(b)
    assert np.all(lp[k:] == -np.inf) and np.all(lp[:, k:] == -np.inf)
    return lp[:k, :k].tolist(), lp0


def _reference(engine, case, kept=False):
    """[(m, ll, lp, lp0, words, path, score)] of the problems."""
    _, Ts, _, means, trans, obs, _ = case
    k = means.shape[1]
    out = []
    for b in range(len(Ts)):
        ll = R.log_likelihoods(obs[b], means[b])
        if kept:
            m = [[int(x) for x in row[:k]] for row in engine.batch_masses(b)]
        else:
            vals, _, logw = engine.batch_store(b)
            assert np.all(logw == np.array(ll[-1])[vals[-1]]), "problem %d: restated log-likelihoods differ from the run's table" % b
            m = R.filtering_masses(vals, ll)
        lp, lp0 = _table(engine, b, k)
        words, _ = D.forward(m, ll, lp, lp0)
        path, score = D.decode(m, ll, lp, lp0)
        out.append((m, ll, lp, lp0, words, path, score))
    return out


def _check_all(engine, case, ref):
    Ts = case[1]
    paths, score = engine.batch_decode()
    assert len(paths) == len(Ts) and score.shape == (len(Ts),)
    for b, T in enumerate(Ts):
        assert paths[b].dtype == np.int32 and np.array_equal(paths[b], ref[b][5]), "problem %d: paths differ" % b
        assert score[b] == ref[b][6], "problem %d: score %r, reference %r" % (b, score[b], ref[b][6])
    for lag in (0, 1, 3, max(Ts)):
        st, sc = engine.batch_decode_lag(lag)
        assert st.shape == (len(Ts), max(Ts)) and np.array_equal(sc, score)
        for b, T in enumerate(Ts):
            assert np.array_equal(st[b], D.decode_lag(ref[b][4], lag, 0, max(Ts))), "lag %d, problem %d" % (lag, b)
            tail = [t for t in range(T) if t + lag >= T - 1]
            assert np.array_equal(st[b, tail], paths[b][tail])
    frm = [min(T, f) for T, f in zip(Ts, (2, 4, 1, 20))]
    st, _ = engine.batch_decode_lag(1, frm)
    assert st.shape[1] == max(T - f for T, f in zip(Ts, frm))
    for b in range(len(Ts)):
        assert np.array_equal(st[b], D.decode_lag(ref[b][4], 1, frm[b], st.shape[1])), "from_steps, problem %d" % b
    return paths, score


@pytest.mark.parametrize("resampler", [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED], ids=["systematic", "stratified"])
@pytest.mark.parametrize("name", ["hmm3", "uniform5", "table2", "table5", "table8"])
def test_decode_is_the_references_with_history_and_with_masses(engine, name, resampler):
    if not name.startswith("uniform"):
        return _history_and_masses(engine, name, resampler)
    eng = cp.Engine(0)                                             # (set_hmm: the shared context keeps the table the other tests left it)
    try:
        _history_and_masses(eng, name, resampler)
    finally:
        eng.close()


def _history_and_masses(engine, name, resampler):
    case = _case(name)
    _begin(engine, case, resampler)
    ref = _reference(engine, case)
    a = _check_all(engine, case, ref)
    if case[2][0] == 1:
        # n = 1: the support is the particle, the decoded path its trace
        trace = engine.batch_paths()[0][0]
        assert np.array_equal(a[0][0], trace[:, 0])
        # table 1: P[0][k-1] = 0 is never taken
        p, k = a[0][1], case[3].shape[1]
        assert ref[1][2][0][k - 1] == -math.inf and not np.any((p[:-1] == 0) & (p[1:] == k - 1))
    _begin(engine, case, resampler, keep_history=False, keep_masses=True)
    kept = _reference(engine, case, kept=True)
    for b in range(len(case[1])):
        assert kept[b][0] == ref[b][0], "problem %d: the kept masses are not the store's" % b
    b_ = _check_all(engine, case, kept)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b_[0])) and np.array_equal(a[1], b_[1])


def _viterbi(lp, lp0, ll):
    """An exact k-state Viterbi over every state: numpy's argmax names the first of equal entries."""
    lp, ll = np.array(lp), np.array(ll)
    v = lp0 + ll[0]
    bp = np.zeros(ll.shape, np.int64)
    for t in range(1, len(ll)):
        cand = v[:, None] + lp
        bp[t] = cand.argmax(axis=0)
        v = cand.max(axis=0) + ll[t]
    x = [int(v.argmax())]
    for t in range(len(ll) - 1, 0, -1):
        x.insert(0, int(bp[t][x[0]]))
    return np.array(x, np.int32), float(v.max())


def test_full_support_is_the_exact_viterbi(engine):
    """k = 3, n = 512, T = 24, means one unit apart (CPPROB_HIP_MODEL_HMM3): every state is occupied at every step -- the seed was
    chosen on the CPU oracle's run of this problem, whose smallest state count is 66 --, so the decode is the exact Viterbi path of
    the realised law."""
    obs = exact.simulate_hmm(24, 500)
    engine.batch_begin(cp.MODEL_HMM3, np.array([obs]), 512)
    engine.batch_run(np.array([1], np.uint64))
    vals, _, _ = engine.batch_store(0)
    ll = R.log_likelihoods(obs, exact.HMM_MEAN)
    m = R.filtering_masses(vals, ll)
    assert all(x > 0 for row in m for x in row), "a state without mass"
    lp, lp0 = _table(engine, 0, 3)
    paths, score = engine.batch_decode()
    want, sc = _viterbi(lp, lp0, ll)
    assert np.array_equal(paths[0], want) and score[0] == sc


def test_log_table_against_math_log(engine):
    """-inf exactly where P = 0; elsewhere within 1 ulp of math.log (two correct logarithms may differ by that much)."""
    for name in ("hmm3", "table2", "table5", "table8"):
        case = _case(name)
        _begin(engine, case)
        k = case[3].shape[1]
        for b in range(len(case[1])):
            lp, lp0 = engine.batch_decode_logp(b)
            P = R.transition_masses(case[4][b])
            want0 = math.log(1.0 / float(k))
            assert abs(lp0 - want0) <= math.ulp(want0)
            for s in range(8):
                for sn in range(8):
                    if s >= k or sn >= k or P[s][sn] == 0:
                        assert lp[s, sn] == -math.inf, (name, b, s, sn)
                    else:
                        want = math.log(float(P[s][sn]) * 2.0 ** -32)
                        assert abs(lp[s, sn] - want) <= math.ulp(want), (name, b, s, sn, lp[s, sn], want)
        if name != "hmm3":
            assert R.transition_masses(case[4][1])[0][k - 1] == 0


def test_device_forms_and_untouched_results(engine):
    import torch
    case = _case("table5")
    _begin(engine, case)
    Ts = case[1]
    before = (engine.batch_results(), engine.batch_smooth(33), engine.batch_forecast(3, 17))
    paths, score = engine.batch_decode()
    st, _ = engine.batch_decode_lag(2)
    flat = np.concatenate(paths)
    # the outputs alone
    only = np.full(flat.size, -5, np.int32)
    assert engine.L.cpprob_hip_batch_decode(engine.h, only.ctypes.data, only.size, None, 0) == 0 and np.array_equal(only, flat)
    only_s = np.full(len(Ts), -5.0)
    assert engine.L.cpprob_hip_batch_decode(engine.h, None, 0, only_s.ctypes.data, only_s.size) == 0 and np.array_equal(only_s, score)
    # the device forms, behind guard bands
    pad = 256
    d_path = torch.full((flat.size + 2 * pad,), -9, dtype=torch.int8, device="cuda:0")
    d_st = torch.full((st.size + 2 * pad,), -9, dtype=torch.int8, device="cuda:0")
    d_sc = torch.full((len(Ts) + 2 * pad,), 12345.5, dtype=torch.float64, device="cuda:0")
    torch.cuda.current_stream().synchronize()
    engine.batch_decode_device(d_path[pad:pad + flat.size], d_sc[pad:pad + len(Ts)])
    engine.batch_decode_lag_device(2, d_st[pad:pad + st.size].view(st.shape))
    engine.sync()
    gp, gs, gc = d_path.cpu().numpy(), d_st.cpu().numpy(), d_sc.cpu().numpy()
    assert np.all(gp[:pad] == -9) and np.all(gp[pad + flat.size:] == -9)
    assert np.all(gs[:pad] == -9) and np.all(gs[pad + st.size:] == -9)
    assert np.all(gc[:pad] == 12345.5) and np.all(gc[pad + len(Ts):] == 12345.5)
    assert np.array_equal(gp[pad:pad + flat.size].astype(np.int32), flat)
    assert np.array_equal(gs[pad:pad + st.size].astype(np.int32).reshape(st.shape), st)
    assert np.array_equal(gc[pad:pad + len(Ts)], score)
    # nothing the other entry points return has changed
    after = (engine.batch_results(), engine.batch_smooth(33), engine.batch_forecast(3, 17))
    assert before[0][0] == after[0][0] and all(np.array_equal(x, y) for x, y in zip(before[0][1:], after[0][1:]))
    assert np.array_equal(before[1][0], after[1][0]) and all(np.array_equal(x, y) for x, y in zip(before[1][1], after[1][1]))
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1])
    # the one-call form
    p2, s2, ev = cp.hmm_table_decode(engine, case[5], case[3], case[4], case[2], case[6])
    assert all(np.array_equal(x, y) for x, y in zip(p2, paths)) and np.array_equal(s2, score)
    assert np.array_equal(ev, [s["log_evidence"] for s in before[0][0]])
    p3, _, _ = cp.hmm_table_decode(engine, case[5], case[3], case[4], case[2], case[6], keep_history=False, lag=2)
    assert all(np.array_equal(p3[b], st[b, :T]) for b, T in enumerate(Ts))


def test_decode_refusals():
    import torch
    eng = cp.Engine(0)
    try:
        eng.batch_B, eng.batch_T, eng.batch_n, eng.batch_K, eng.batch_shapes = 1, 1, 1, 3, None
        lp, lp0 = np.zeros(64), C.c_double(0.0)
        logp = eng.L.cpprob_hip_batch_decode_logp
        assert logp(eng.h, 0, lp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(lp0)) == ESTATE
        for call in (lambda: eng.batch_decode(), lambda: eng.batch_decode_lag(1)):
            with pytest.raises(cp.CpprobHipError) as e:          # no batch at all
                call()
            assert e.value.code == ESTATE
        obs = [exact.simulate_hmm(T, 70 + b) for b, T in enumerate([3, 2])]
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20])
        assert logp(eng.h, 1, lp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(lp0)) == 0 and lp0.value < 0.0     # the table is there from the begin on
        assert logp(eng.h, 2, lp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(lp0)) == EINVAL
        assert logp(eng.h, 0, None, C.byref(lp0)) == EINVAL
        for call in (lambda: eng.batch_decode(), lambda: eng.batch_decode_lag(1)):
            with pytest.raises(cp.CpprobHipError) as e:          # begun, not run
                call()
            assert e.value.code == ESTATE
        eng.batch_run(_seeds(2))
        path, st, score = np.full(5, -5, np.int32), np.full(6, -5, np.int32), np.full(2, -5.0)
        dec, lag = eng.L.cpprob_hip_batch_decode, eng.L.cpprob_hip_batch_decode_lag
        u32 = C.POINTER(C.c_uint32)
        assert dec(eng.h, path.ctypes.data, 4, score.ctypes.data, 2) == EINVAL
        assert dec(eng.h, path.ctypes.data, 5, score.ctypes.data, 1) == EINVAL
        assert lag(eng.h, (1 << 24) + 1, None, 3, st.ctypes.data, 6, score.ctypes.data, 2) == EINVAL
        assert lag(eng.h, 1, None, 2, st.ctypes.data, 6, score.ctypes.data, 2) == EINVAL               # problem 0 owes 3 rows
        assert "problem 0" in eng.L.cpprob_hip_last_error(eng.h).decode()
        past = np.array([0, 3], np.uint32)                       # problem 1: from = L + 1
        assert lag(eng.h, 1, past.ctypes.data_as(u32), 3, st.ctypes.data, 6, score.ctypes.data, 2) == EINVAL
        assert "problem 1" in eng.L.cpprob_hip_last_error(eng.h).decode()
        assert lag(eng.h, 1, None, 3, st.ctypes.data, 5, score.ctypes.data, 2) == EINVAL
        assert lag(eng.h, 1, None, 3, st.ctypes.data, 6, score.ctypes.data, 1) == EINVAL
        assert np.all(path == -5) and np.all(st == -5) and np.all(score == -5.0)
        edge = np.array([3, 2], np.uint32)                       # from = L: allowed, no row
        assert lag(eng.h, 1, edge.ctypes.data_as(u32), 1, st.ctypes.data, 2, score.ctypes.data, 2) == 0
        assert np.all(st[:2] == -1) and np.all(st[2:] == -5) and np.all(score < 0.0)
        assert dec(eng.h, path.ctypes.data, 5, score.ctypes.data, 2) == 0 and np.all((path >= 0) & (path < 3))
        assert lag(eng.h, 1 << 24, None, 3, st.ctypes.data, 6, None, 0) == 0
        assert st.reshape(2, 3).tolist() == [path[:3].tolist(), path[3:].tolist() + [-1]]
        d = torch.full((5,), -9, dtype=torch.int8, device="cuda:0")
        ds = torch.full((2,), -9.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.current_stream().synchronize()
        assert eng.L.cpprob_hip_batch_decode_device(eng.h, C.c_void_p(d.data_ptr()), 4, C.c_void_p(ds.data_ptr()), 2) == EINVAL
        assert eng.L.cpprob_hip_batch_decode_lag_device(eng.h, 1, None, 3, C.c_void_p(d.data_ptr()), 5, C.c_void_p(ds.data_ptr()), 2) == EINVAL
        eng.sync()
        assert bool((d == -9).all()) and bool((ds == -9.0).all())
        eng.batch_begin_problems(cp.MODEL_HMM3, obs, [10, 20], keep_history=False)      # a plain filtering batch
        eng.batch_run(_seeds(2))
        for call in (lambda: eng.batch_decode(), lambda: eng.batch_decode_lag(1)):
            with pytest.raises(cp.CpprobHipError) as e:
                call()
            assert e.value.code == ESTATE and "keep_history" in str(e.value)
    finally:
        eng.close()
