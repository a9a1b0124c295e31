"""The run's last step with the read-out folded in (step_counts.hpp: step_fold_tail) against the two-launch form
(CPPROB_HIP_FLAG_SEPARATE_TRACE_READOUT): the same integers and the same doubles, bit for bit, at every hierarchy depth
(<= 64 tiles, <= 4096, beyond), for every resampler of the prefix-count form, over back-to-back runs (the counters and arrival
words a folded run leaves are where the next one starts) and for filtering-only runs.
"""
import os

import numpy as np
import pytest

import cpprob_amd as cp

pytestmark = pytest.mark.gpu

SEP = cp.capi.FLAG_SEPARATE_TRACE_READOUT
RESAMPLERS = [cp.RESAMPLE_SYSTEMATIC, cp.RESAMPLE_STRATIFIED, cp.RESAMPLE_MULTINOMIAL]


def _obs(golden_dir, T):
    return np.load(os.path.join(golden_dir, "observations.npz"))["hmm16"][:T]


def _summary(eng):
    s = eng.summary()
    return {k: s[k] for k in ("log_evidence", "ess_final", "n_resampled")}


def _outputs(eng, keep):
    out = {"stats": eng.stats(), "stats_again": eng.stats(), "summary": _summary(eng), "trace": eng.step_trace()}
    if keep:
        out.update(values=eng.values(), ancestors=eng.ancestors(), paths=eng.paths())
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "summary":
            for f in a[k]:
                assert np.array_equal(np.asarray(a[k][f]), np.asarray(b[k][f])), (k, f, a[k][f], b[k][f])
        elif k == "trace":
            for x, y in zip(a[k], b[k]):
                assert np.array_equal(np.asarray(x), np.asarray(y)), k
        else:
            assert np.array_equal(a[k], b[k]), k


def _run(eng, obs, n, rs, flags, keep, run_index=0):
    eng.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=77, resampler=rs, ess_threshold=2.0, keep_history=keep, flags=flags)
    eng.run(run_index)
    return _outputs(eng, keep)


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("T", [1, 2, 16])
@pytest.mark.parametrize("n", [1, 1000, 1024, 1025, 65536, 65537, 1_000_000, 4_194_305])
def test_folded_readout_equals_separate_launch(engine, golden_dir, n, T, rs):
    obs = _obs(golden_dir, T)
    folded = _run(engine, obs, n, rs, 0, True)
    separate = _run(engine, obs, n, rs, SEP, True)
    _assert_same(folded, separate)
    st = folded["stats"]
    assert st.shape[0] == T and np.all(np.isfinite(st))
    assert np.allclose(st.sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("n", [1025, 65537, 4_194_305])
def test_folded_readout_back_to_back_runs(engine, golden_dir, n, rs):
    """Five runs on one context with different run indices: each folded run must start from cleared counters."""
    obs = _obs(golden_dir, 16)
    engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=5, resampler=rs, ess_threshold=2.0, flags=SEP)
    ref = []
    for r in range(5):
        engine.run(r)
        ref.append(_outputs(engine, True))
    engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=5, resampler=rs, ess_threshold=2.0, flags=0)
    for r in range(5):
        engine.run(r)
        _assert_same(_outputs(engine, True), ref[r])
    assert not np.array_equal(ref[0]["stats"], ref[1]["stats"])


@pytest.mark.parametrize("rs", RESAMPLERS)
@pytest.mark.parametrize("T", [1, 2, 16])
@pytest.mark.parametrize("n", [1, 1025, 65537, 1_000_000, 4_194_305])
def test_folded_filtering_only_equals_separate_launch(engine, golden_dir, n, T, rs):
    obs = _obs(golden_dir, T)
    folded = _run(engine, obs, n, rs, 0, False)
    separate = _run(engine, obs, n, rs, SEP, False)
    _assert_same(folded, separate)
    for r in (3, 4):                                   # back to back, other run indices
        engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=77, resampler=rs, ess_threshold=2.0, keep_history=False, flags=0)
        engine.run(r)
        a = _outputs(engine, False)
        engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, obs, n, seed=77, resampler=rs, ess_threshold=2.0, keep_history=False, flags=SEP)
        engine.run(r)
        _assert_same(a, _outputs(engine, False))


@pytest.mark.parametrize("rs", RESAMPLERS)
def test_folded_run_leaves_no_state_for_the_next_form(engine, golden_dir, rs):
    """A folded run, then a run of another form on the same context (fixed-point masses: its own read-out launches)."""
    hmm, lg = _obs(golden_dir, 16), np.load(os.path.join(golden_dir, "observations.npz"))["lgssm100"][:12]
    out = []
    for first_flags in (0, SEP):
        engine.begin(cp.ALG_SMC, cp.MODEL_HMM3, hmm, 1025, seed=9, resampler=rs, ess_threshold=2.0, flags=first_flags)
        engine.run()
        engine.begin(cp.ALG_SMC, cp.MODEL_LINEAR_GAUSSIAN_1D, lg, 4099, seed=3, resampler=rs, ess_threshold=0.5)
        engine.run()
        out.append(_outputs(engine, True))
    _assert_same(out[0], out[1])
