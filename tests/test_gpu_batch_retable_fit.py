"""The fitting loops on a batch that is begun once: cpprob_amd.hmm_table_em(resident=True) -- the whole loop enqueued on tensors that
stay on the device (batch_run, batch_smooth_stats_device, batch_summaries_device, batch_mstep_device, batch_retable_device) -- and the
two Gibbs samplers with retable=True (batch_retable in place of a begin from the second sweep on) return, array_equal, what the loops
that begin a fresh batch every time return.  cpprob_main --em_iterations N --em_on_device (cpprob::gpu::Options::fit_on_device) prints the
bytes it prints without the flag."""
import os
import subprocess

import numpy as np
import pytest

import cpprob_amd as cp

pytestmark = pytest.mark.gpu

MAIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cpprob_amd", "bin", "cpprob_main")
TS = [1, 7, 40, 33, 32, 19]
B, K, N = len(TS), 3, 64


def _problem(seed):
    rng = np.random.default_rng(seed)
    means = np.sort(rng.uniform(-3.0, 3.0, (B, K)), axis=1) + 0.5 * np.arange(K)
    trans = rng.uniform(0.05, 1.0, (B, K, K))
    trans[1, 0, K - 1] = 0.0
    obs = [means[b][rng.integers(0, K, T)] + rng.standard_normal(T) for b, T in enumerate(TS)]
    return obs, means, trans, np.array([11 + 101 * b for b in range(B)], np.uint64)


def _count_begins(engine, monkeypatch):
    calls = {"begin": 0, "retable": 0, "retable_device": 0}
    for name, key in (("batch_begin_problems", "begin"), ("batch_retable", "retable"), ("batch_retable_device", "retable_device")):
        inner = getattr(engine, name)

        def counted(*a, _inner=inner, _key=key, **kw):
            calls[_key] += 1
            return _inner(*a, **kw)
        monkeypatch.setattr(engine, name, counted, raising=False)
    return calls


@pytest.mark.parametrize("keep_history", [True, False])
def test_resident_em_is_the_host_loop(engine, monkeypatch, keep_history):
    obs, means, trans, seeds = _problem(5)
    want = cp.hmm_table_em(engine, obs, means, trans, N, seeds, 4, keep_history=keep_history)
    calls = _count_begins(engine, monkeypatch)
    got = cp.hmm_table_em(engine, obs, means, trans, N, seeds, 4, keep_history=keep_history, resident=True)
    assert calls == {"begin": 1, "retable": 0, "retable_device": 3}
    for g, w, what in zip(got, want, ("means", "transition", "log_evidence")):
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), what
    assert want[0].shape == (5, B, K) and want[2].shape == (4, B) and not np.array_equal(want[0][4], want[0][0])
    # the problem of length 1 has no transitions: its rows stay
    assert np.array_equal(got[1][4][0], trans[0])


@pytest.mark.parametrize("keep_history", [True, False])
def test_gibbs_on_a_retabled_batch_is_the_same_chain(engine, monkeypatch, keep_history):
    obs, means, trans, seeds = _problem(6)
    want = cp.hmm_table_gibbs(engine, obs, means, trans, N, seeds, 3, np.random.default_rng(2), keep_history=keep_history)
    calls = _count_begins(engine, monkeypatch)
    got = cp.hmm_table_gibbs(engine, obs, means, trans, N, seeds, 3, np.random.default_rng(2), keep_history=keep_history, retable=True)
    assert calls == {"begin": 1, "retable": 2, "retable_device": 0}
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert not np.array_equal(want[0][3], want[0][0])


def test_particle_gibbs_on_a_retabled_batch_is_the_same_chain(engine, monkeypatch):
    obs, means, trans, seeds = _problem(7)
    want = cp.hmm_table_particle_gibbs(engine, obs, means, trans, N, seeds, 3, np.random.default_rng(3), alpha=1.5)
    calls = _count_begins(engine, monkeypatch)
    got = cp.hmm_table_particle_gibbs(engine, obs, means, trans, N, seeds, 3, np.random.default_rng(3), alpha=1.5, retable=True)
    assert calls == {"begin": 1, "retable": 2, "retable_device": 0}
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert not np.array_equal(want[0][3], want[0][0])


def _numbers(x):
    return "[" + " ".join(repr(float(v)) for v in np.asarray(x).reshape(-1)) + "]"


@pytest.mark.parametrize("more", [(), ("--filtering_only", "--keep_masses"), ("--decode",)], ids=["history", "masses", "decode"])
def test_cli_fit_on_device_prints_the_same_bytes(tmp_path, more):
    """tests/test_gpu_batch_suffstats_cli.py's way: the fit through cpprob_main, with and without --em_on_device."""
    obs, means, trans, _ = _problem(8)
    (tmp_path / "tables.txt").write_text("".join("%s %s %s\n" % (_numbers(means[b]), _numbers(trans[b]), _numbers(obs[b])) for b in range(B)))
    base = [MAIN, "--model_folder", str(tmp_path), "--smc", "--ess_threshold", "2", "--n_samples", str(N), "--seed", "12", "--batch_tables_file", "tables.txt",
            "--em_iterations", "3"] + list(more)
    want = subprocess.run(base, capture_output=True, timeout=600)
    got = subprocess.run(base + ["--em_on_device"], capture_output=True, timeout=600)
    assert want.returncode == 0 and got.returncode == 0, got.stderr[-2000:]
    assert got.stdout == want.stdout and len(want.stdout.strip().splitlines()) >= 2 * B
    # the fitted tables moved: the lines are not the input's
    assert _numbers(means[1]).encode() not in want.stdout
